#!/usr/bin/env python3
"""Device time of `converge_batch` - a rollout whose instances stop on their own and whose waves leave when all their
lanes have stopped - against what brought a batch to its targets before: `rollout_batch([t] * max_ticks, summary=True,
summary_tol=tol)` with the tick count of the slowest instance.  The single-pose iiwa skill and the headline stack, random
reachable targets at distances spread over four decades (0.06 rad per joint at most), `max_ticks` = the slowest instance's tick count.
    python tools/converge_bench.py [B ...  default 16384 131072] [--out FILE]
Timing: HIP events around the call on device tensors, `WARMUP` calls first, the median of `REPS`; the calls rotate through
`SETS` copies of the inputs and every call gets new state and output tensors.  What (a) should cost is derived from the
run's own `ticks`: w = mean over waves of (largest ticks in the wave + 1) / (max_ticks + 1); (a) <= 1.15 w (b) is the
expectation.  `--out` writes the tables (markdown) to a file as well.
    python tools/converge_bench.py --ik [T ...  default 1024 8192] [--out FILE]
Multi-seed IK instead: `ik_batch(first_hit=True)` - a target's first converged seed stops its other seeds - against
`ik_batch()`, the single-pose skill, T targets x 16 seeds of which about a quarter run out of ticks (the achieved share is
printed), `max_ticks` = 40, several times the median arrival.  The expectation beside the ratio: the ticks the launch lasts
with the rule over those without it, from the two launches' own `ticks` (`launch_cost`).
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402

import casclik_amd as cc    # noqa: E402
from casclik_amd import jit, skills      # noqa: E402

SIZES = [int(a) for a in sys.argv[1:] if a.isdigit()] or [16384, 131072]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
WARMUP, REPS, SETS = 2, 7, 4
DT, CAP, UNIQUE = 0.05, 200, 4096


def reach_inputs(fk, B, seed):
    """start states inside 80 % of the joint range and the tool pose at a state near each: UNIQUE distinct instances,
    drawn with replacement into a batch of B (so every wave holds a random mix of near and far targets)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(fk["lower"], float), np.asarray(fk["upper"], float)
    Q = rng.uniform(0.8 * lo, 0.8 * hi, size=(UNIQUE, lo.size))
    near = Q + (10.0 ** rng.uniform(-5.0, -1.2, size=(UNIQUE, 1))) * rng.normal(size=Q.shape)
    Y = np.zeros((UNIQUE, 7))
    for b in range(UNIQUE):
        T = fk["chain"].fk_numeric(near[b])
        Y[b, :3], Y[b, 3:] = T[:3, 3], skills.quat_from_matrix(T[:3, :3])
    pick = rng.integers(0, UNIQUE, B)
    return Q[pick], Y[pick]


def timed(fn):
    """median device time of fn(k) in microseconds; k counts the calls (the input set to use)"""
    for k in range(WARMUP):
        fn(k)
    torch.cuda.synchronize()
    out = []
    for k in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(WARMUP + k)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def unit_line(ctrl):
    info = jit._load(os.path.join(jit.CACHE, "clik_shape_%s.so" % ctrl._kernels["converge"])).clik_jit_converge_info
    info.restype, info.argtypes = C.c_longlong, [C.c_int]
    per_cu = min(4, jit.SUMMARY_LDS_BYTES // info(2) * info(4))
    return "block: %d wave(s), %d bytes of LDS -> %d waves per CU (one per SIMD: the kernel holds the register file); " \
           "scratch per lane as the loaded code object states it: %d bytes" % (info(4), info(2), per_cu, info(5))


def measure(name, ctrl, tol, B):
    fk = skills.iiwa()
    sets = []
    for k in range(SETS):
        Q, Y = reach_inputs(fk, B, seed=20 + k)
        sets.append((torch.from_numpy(Q).cuda(), torch.from_numpy(Y).cuda()))
    # the slowest instance's tick count, over all input sets
    ticks = [ctrl.converge_batch(q, y, tol=tol, max_ticks=CAP, dt=DT)[3] for q, y in sets]
    late = sum(int((t["status"] != 0).sum()) for t in ticks)       # (not reached within CAP ticks: reported, not timed for)
    n = int(max(int(t["ticks"][t["status"] == 0].max()) for t in ticks))
    tk = np.minimum(ticks[0]["ticks"].cpu().numpy(), n)        # (a late instance runs out of ticks at max_ticks)
    waves = np.pad(tk, (0, -len(tk) % 64)).reshape(-1, 64).max(axis=1)
    w = float(np.mean((waves + 1.0) / (n + 1.0)))
    tol_b = np.where(np.isfinite(tol), tol, 1e300)      # (summary_tol takes finite values: a row that cannot block)
    times = np.zeros(n)

    def a(k):
        q, y = sets[k % SETS]
        return ctrl.converge_batch(q, y, tol=tol, max_ticks=n, dt=DT)

    def b(k):
        q, y = sets[k % SETS]
        return ctrl.rollout_batch(times, q, input_var=y, dt=DT, summary=True, summary_tol=tol_b)

    ta, tb = timed(a), timed(b)
    ratio = ta[0] / tb[0]
    out = ["", "### %s: %d instances, max_ticks = %d" % (name, B, n), "",
           "| path | device time, median of %d (min .. max), us |" % REPS, "|---|---|",
           "| (a) `converge_batch` | %.1f (%.1f .. %.1f) |" % ta,
           "| (b) `rollout_batch(summary=True, summary_tol=tol)` | %.1f (%.1f .. %.1f) |" % tb, "",
           "w = %.4f, (a) / (b) = %.4f, bound 1.15 w = %.4f: %s" % (w, ratio, 1.15 * w, "met" if ratio <= 1.15 * w else "MISSED"),
           "", "ticks histogram (input set 0): " + " ".join("%d:%d" % (i, c) for i, c in enumerate(np.bincount(tk)) if c),
           "mean ticks %.2f, waves %d (the device has 1024 SIMDs); %d of %d instances not within tolerance after %d ticks"
           % (tk.mean(), len(waves), late, SETS * B, CAP)]
    print("\n".join(out), flush=True)
    return out


IK_SEEDS, IK_FAR, IK_TICKS, IK_TOL, SIMDS = 16, 7, 40, 1e-5, 1024


def ik_inputs(fk, T, seed):
    """(targets [T, 7], seeds [T, 16, 7]): UNIQUE distinct targets - the tool pose at a state inside half the joint range -
    drawn with replacement, each with its own seeds around that state: nine at 0.003 .. 0.1 rad (a standard deviation
    per joint), which arrive, and IK_FAR = seven at 1 .. 3.2 rad (clipped to the joint range), about half of which cross a
    singularity on their way and are not there after IK_TICKS ticks (the oracle's host loop on 24 targets: 21 % of all
    seeds run out of ticks, every target's first arrival after 8 .. 10 ticks)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(fk["lower"], float), np.asarray(fk["upper"], float)
    star = rng.uniform(0.5 * lo, 0.5 * hi, size=(UNIQUE, lo.size))
    Y = np.zeros((UNIQUE, 7))
    for b in range(UNIQUE):
        M = fk["chain"].fk_numeric(star[b])
        Y[b, :3], Y[b, 3:] = M[:3, 3], skills.quat_from_matrix(M[:3, :3])
    scale = np.concatenate([10.0 ** np.linspace(-2.5, -1.0, IK_SEEDS - IK_FAR), 10.0 ** np.linspace(0.0, 0.5, IK_FAR)])
    seeds = star[:, None, :] + scale[None, :, None] * rng.normal(size=(UNIQUE, IK_SEEDS, lo.size))
    seeds = np.clip(seeds, lo, hi)
    pick = rng.integers(0, UNIQUE, T)
    return Y[pick], seeds[pick]


def launch_cost(ticks):
    """what a launch with these tick counts costs in ticks, as w is derived above: a wave runs the tests 0 .. its largest
    `ticks`; with no more waves than SIMDs the launch lasts as long as its slowest wave, with more a SIMD runs its waves
    (taken round-robin) one after the other and the launch lasts as long as the slowest SIMD"""
    waves = np.pad(ticks, (0, -len(ticks) % 64)).reshape(-1, 64).max(axis=1) + 1.0
    per_simd = np.pad(waves, (0, -len(waves) % SIMDS)).reshape(-1, SIMDS).sum(axis=0)
    return float(per_simd.max()), len(waves)


def measure_ik(ctrl, T):
    fk = skills.iiwa()
    sets = []
    for k in range(SETS):
        Y, seeds = ik_inputs(fk, T, seed=40 + k)
        sets.append((torch.from_numpy(Y).cuda(), torch.from_numpy(seeds).cuda()))
    kw = dict(tol=IK_TOL, max_ticks=IK_TICKS, dt=DT)
    # the tick counts of input set 0 with and without the rule, from the launches ik_batch makes
    Y, seeds = sets[0]
    Q0 = seeds.reshape(T * IK_SEEDS, -1).contiguous()
    Ys = Y.unsqueeze(1).expand(T, IK_SEEDS, Y.shape[1]).reshape(T * IK_SEEDS, -1).contiguous()
    plain = ctrl.converge_batch(Q0, Ys, **kw)[3]
    grouped = ctrl.converge_batch(Q0, Ys, group=IK_SEEDS, **kw)[3]
    pt, ps = plain["ticks"].cpu().numpy(), plain["status"].cpu().numpy()
    gt, gs = grouped["ticks"].cpu().numpy(), grouped["status"].cpu().numpy()
    ok = (ps == 0).reshape(T, IK_SEEDS)
    arrival = np.where(ok, pt.reshape(T, IK_SEEDS), IK_TICKS + 1).min(axis=1)
    cost_p, n_waves = launch_cost(pt)
    cost_g, _ = launch_cost(gt)
    one, two = ctrl.ik_batch(Y, seeds, **kw), ctrl.ik_batch(Y, seeds, first_hit=True, **kw)
    same = all(bool((one[1][k] == two[1][k]).all()) for k in ("seed", "ticks", "status"))
    dq = float((one[0] - two[0]).abs().max())

    def a(k):
        return ctrl.ik_batch(*sets[k % SETS], first_hit=True, **kw)

    def b(k):
        return ctrl.ik_batch(*sets[k % SETS], **kw)

    # the launch alone - `converge_batch` on the T x 16 instances with and without the rule -, apart from what `ik_batch`
    # does around it on the host and in torch kernels (expanding the targets, `select_seeds`, gathering the picks)
    flat = [(s.reshape(T * IK_SEEDS, -1).contiguous(),
             y.unsqueeze(1).expand(T, IK_SEEDS, y.shape[1]).reshape(T * IK_SEEDS, -1).contiguous()) for y, s in sets]

    def c(k):
        return ctrl.converge_batch(*flat[k % SETS], group=IK_SEEDS, **kw)

    def d(k):
        return ctrl.converge_batch(*flat[k % SETS], **kw)

    ta, tb, tc, td = timed(a), timed(b), timed(c), timed(d)
    out = ["", "### multi-seed IK, single pose (iiwa): %d targets x %d seeds = %d instances, max_ticks = %d" % (
               T, IK_SEEDS, T * IK_SEEDS, IK_TICKS), "",
           "| path | device time, median of %d (min .. max), us |" % REPS, "|---|---|",
           "| (a) `ik_batch(first_hit=True)` | %.1f (%.1f .. %.1f) |" % ta,
           "| (b) `ik_batch()` | %.1f (%.1f .. %.1f) |" % tb,
           "| (c) the launch alone: `converge_batch(group=%d)` | %.1f (%.1f .. %.1f) |" % ((IK_SEEDS,) + tc),
           "| (d) the launch alone: `converge_batch()` | %.1f (%.1f .. %.1f) |" % td, "",
           "(a) / (b) = %.4f, (c) / (d) = %.4f; expected from the tick counts of input set 0: %.4f (a launch of %d waves "
           "lasts %.0f ticks with the rule, %.0f without)" % (ta[0] / tb[0], tc[0] / td[0], cost_g / cost_p, n_waves,
                                                              cost_g, cost_p),
           "", "seeds out of ticks without the rule: %.1f %% (status 1: %d of %d); targets with an arrival: %d of %d, "
           "median first arrival %.0f ticks, latest %d; seeds cancelled with the rule: %.1f %%" % (
               100.0 * (ps == 1).mean(), (ps == 1).sum(), ps.size, ok.any(axis=1).sum(), T,
               np.median(arrival[ok.any(axis=1)]), arrival[ok.any(axis=1)].max(), 100.0 * (gs == 5).mean()),
           "largest ticks per wave, mean: %.1f with the rule, %.1f without; same seed, ticks and status from both paths: "
           "%s, max |q(a) - q(b)| = %.2e" % (
               np.pad(gt, (0, -len(gt) % 64)).reshape(-1, 64).max(axis=1).mean(),
               np.pad(pt, (0, -len(pt) % 64)).reshape(-1, 64).max(axis=1).mean(), same, dq)]
    print("\n".join(out), flush=True)
    return out


def main_ik():
    """`--ik`: `ik_batch(first_hit=True)` against `ik_batch()`, the single-pose skill, T x 16 seeds (default T = 1024 8192)"""
    ctrl = cc.PseudoInverseController(skill_spec=skills.pose_skill(skills.iiwa()))
    ctrl.setup_problem_functions()
    text = []
    for T in [int(a) for a in sys.argv[1:] if a.isdigit()] or [1024, 8192]:
        text += measure_ik(ctrl, T)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(text) + "\n")


def main():
    fk = skills.iiwa()
    text = []
    for name, spec, opts, by_label in (
            ("single pose (iiwa)", skills.pose_skill(fk), None, {"tool_pose": 1e-5}),
            ("headline stack (config 3)", skills.stack_skill(fk), dict(skills.STACK_OPTIONS),
             {"tool_pose": 1e-4, "joint_centering": np.inf, "joint_limits": 1e-9})):
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=opts)
        ctrl.setup_problem_functions()
        tol = np.zeros(sum(sl.stop - sl.start for sl in ctrl.constraint_rows().values()))
        for label, sl in ctrl.constraint_rows().items():
            tol[sl] = by_label[label]
        for B in SIZES:
            text += measure(name, ctrl, tol, B)
        text += ["", name + " " + unit_line(ctrl)]
        print(text[-1], flush=True)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main_ik() if "--ik" in sys.argv else main()
