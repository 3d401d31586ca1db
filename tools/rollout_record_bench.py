#!/usr/bin/env python3
"""Device time per tick of rollouts that record their trajectory and follow one target per tick (`rollout_batch(...,
record_every=k)`, `input_var [n_ticks, B, n_y]`) against the unrecorded rollout and against today's only alternative,
one launch per `k` ticks (the chunked loop), for the headline skill (config 3, 256 ticks per launch) and config 4 (64
ticks per launch) at B instances - DESIGN.md section 5.
    python tools/rollout_record_bench.py [B=16384] [--write] [--headline-only]
Timing: HIP events around the launch(es) on device tensors, one warm-up first, the best of `REPS` repetitions.  The
chunked loop is timed the same way around all of its launches, so its figure includes what the launches cost the device
queue but no host work that the device does not wait for.  `--write` puts the table into profiles/rollout_record.md and
adds a row to BASELINE.md.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402

import casclik_amd as cc    # noqa: E402
from casclik_amd import skills      # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args else 16384
WRITE = "--write" in sys.argv
REPS = 5


def timed(fn):
    """best device time of fn() in microseconds (HIP events around it), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3)
    return best


def measure(name, ctrl, n_ticks, dt, vmax):
    fk = skills.iiwa()
    Q, Y = skills.synthetic_inputs(fk, B, seed=1, distribution="mixed")
    Qd, Yd = torch.from_numpy(Q).cuda(), torch.from_numpy(Y).cuda()
    Y3 = Yd[None].repeat(n_ticks, 1, 1)
    Y3[:, :, :3] += 1e-3 * torch.arange(n_ticks, device="cuda", dtype=torch.float64)[:, None, None]
    times = np.zeros(n_ticks)
    rows = []

    def roll(y, k, n=n_ticks, q=Qd):
        return ctrl.rollout_batch(times[:n], q, input_var=y, dt=dt, max_speed=vmax, record_every=k)

    rows.append(("unrecorded, one target", timed(lambda: roll(Yd, None)) / n_ticks, None))
    for k in (1, 8, 64):
        rec = timed(lambda: roll(Yd, k)) / n_ticks

        def chunked():
            q = Qd
            for _ in range(n_ticks // k):
                q = roll(Yd, None, n=k, q=q)[0]
        rows.append(("record_every=%d" % k, rec, timed(chunked) / n_ticks))
    rows.append(("target per tick", timed(lambda: roll(Y3, None)) / n_ticks, None))
    rows.append(("target per tick + record_every=1", timed(lambda: roll(Y3, 1)) / n_ticks, None))
    out = ["", "### %s: %d instances, %d ticks per launch (`%s`)" % (
        name, B, n_ticks, ctrl.kernel_variant(B) if hasattr(ctrl, "kernel_variant") else ctrl.kernel_name), "",
        "| rollout | us per tick (device) | chunked loop: a launch per k ticks |", "|---|---|---|"]
    for label, us, alt in rows:
        out.append("| %s | %.3f | %s |" % (label, us, "-" if alt is None else "%.3f" % alt))
    print("\n".join(out), flush=True)
    return out, rows


def main():
    fk = skills.iiwa()
    head = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
    head.setup_problem_functions()
    qp = cc.ReactiveQPController(skill_spec=skills.qp_skill(fk))
    qp.setup_problem_functions()
    qp.setup_solver()
    text, keep = [], {}
    cases = (("config 3 (headline)", head, 256, np.pi / 5), ("config 4 (QP)", qp, 64, 1.0))
    for name, ctrl, n, vmax in cases[:1] if "--headline-only" in sys.argv else cases:
        out, rows = measure(name, ctrl, n, 0.008, vmax)
        text += out
        keep[name] = rows
    if WRITE and len(keep) == 2:
        path = os.path.join(ROOT, "profiles", "rollout_record.md")
        marker = "<!-- rollout_record_bench -->"
        old = open(path).read() if os.path.exists(path) else "# Recording rollouts\n\n" + marker + "\n"
        cut = old.index(marker) + len(marker) if marker in old else len(old)
        with open(path, "w") as f:
            f.write(old[:cut] + "\n" + "\n".join(text) + "\n")
        h, q = keep["config 3 (headline)"], keep["config 4 (QP)"]
        with open(os.path.join(ROOT, "BASELINE.md"), "a") as f:
            f.write("\nRecording rollouts (tools/rollout_record_bench.py, B = %d, device us per tick; profiles/rollout_record.md): "
                    "config 3, 256 ticks per launch: unrecorded %.2f, record_every 1 / 8 / 64: %.2f / %.2f / %.2f, a target per "
                    "tick %.2f; config 4, 64 ticks per launch: %.2f, %.2f / %.2f / %.2f, %.2f.\n"
                    % (B, h[0][1], h[1][1], h[2][1], h[3][1], h[4][1], q[0][1], q[1][1], q[2][1], q[3][1], q[4][1]))


if __name__ == "__main__":
    main()
