#!/usr/bin/env python3
"""Device time of `constraint_values_batch` (clik_monitor.hpp) on the headline skill, against its yardsticks - DESIGN.md
section 5:
  e only        131072 rows (16384 instances x 8 records) against the `solve_batch` tick on 131072 instances of the same
                skill: the read-out does a strict subset of that tick's work;
  jacobian=True the same rows against a device-to-device copy that moves as many bytes as the call reads and writes;
  host-inclusive a 256-tick Moe-2016 pinv rollout with `record_every=1` followed by ONE values call, against the same
                rollout followed by the host evaluation (the oracle's ExprEvaluator) of the records.
    python tools/constraint_values_bench.py [B=16384] [R=8] [--write] [--device-only]
`CLIK_JIT_DEFINES=-DCLIK_MONITOR_LANE_STORES` builds the kernel's measuring variant (every lane stores its own e rows).
Timing: every variant works on a ring of four input / output buffer sets (as bench.py rotates its ticks); `INNER` launches
are captured into one graph per variant and a replay is timed between two HIP events, `ROUNDS` interleaved rounds of all
variants in one process; median and minimum are reported.
`--write` puts the table into profiles/constraint_values.md.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np          # noqa: E402
import torch                # noqa: E402

import casclik_amd as cc    # noqa: E402
from casclik_amd import skills      # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args else 16384
R = int(args[1]) if len(args) > 1 else 8
WRITE = "--write" in sys.argv
RING, INNER, ROUNDS = 4, 20, 9


def interleaved(variants):
    """{name: (median, min)} us per call of each fn(slot): INNER calls captured into one graph per variant (the Python
    side of a call costs more than these kernels run, and a replayed graph has none), ROUNDS interleaved rounds of
    replays, each between two HIP events"""
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in variants.items():
        for s in range(RING):
            fn(s)
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(INNER):
                fn(i % RING)
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            samples[name].append(a.elapsed_time(b) * 1e3 / INNER)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in samples.items()}


def device_part():
    fk = skills.iiwa()
    ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
    ctrl.setup_problem_functions()
    d = ctrl.descriptor
    rows = R * B
    m_tot, n = max(sl.stop for sl in ctrl.constraint_rows().values()), d.n_q + d.n_x
    slots = []
    # (4096 synthetic states and targets, drawn with replacement and jittered: the targets come from a host FK per row)
    Q0, Y0 = skills.synthetic_inputs(fk, 4096, seed=10, distribution="mixed")
    rng = np.random.default_rng(11)
    for s in range(RING):
        idx = rng.integers(0, len(Q0), size=rows)
        Q, Y = Q0[idx] + rng.normal(scale=1e-3, size=(rows, Q0.shape[1])), np.ascontiguousarray(Y0[idx])
        Qd, Yd = torch.from_numpy(Q).cuda(), torch.from_numpy(Y).cuda()
        slots.append({"Q3": Qd.reshape(R, B, -1), "Y3": Yd.reshape(R, B, -1), "Q": Qd, "Y": Yd,
                      "E": torch.empty((R, B, m_tot), dtype=torch.float64, device="cuda")})
    read_b = rows * (d.n_q + d.n_y) * 8
    write_e = rows * m_tot * 8
    write_j = rows * (2 * m_tot + m_tot * n) * 8
    # a copy of k bytes reads k and writes k: half the bytes the call moves, so that both move the same total
    copy_e = [(torch.empty((read_b + write_e) // 16, dtype=torch.float64, device="cuda").normal_(),
               torch.empty((read_b + write_e) // 16, dtype=torch.float64, device="cuda")) for _ in range(RING)]
    copy_j = [(torch.empty((read_b + write_j) // 16, dtype=torch.float64, device="cuda").normal_(),
               torch.empty((read_b + write_j) // 16, dtype=torch.float64, device="cuda")) for _ in range(RING)]
    ctrl.constraint_values_batch(0.0, slots[0]["Q3"], input_var=slots[0]["Y3"])      # (instantiates the kernel)
    # e, J and e_t of every slot are allocated once (the method would take J and e_t from the graph's pool, one block
    # for all captured launches): the C entry point, on the capturing stream
    from casclik_amd.controllers.base_controller import current_stream, ptr
    for sl in slots:
        sl["J"] = torch.empty((R, B, m_tot, n), dtype=torch.float64, device="cuda")
        sl["Et"] = torch.empty((R, B, m_tot), dtype=torch.float64, device="cuda")

    def full(s):
        sl = slots[s]
        rc = ctrl._lib.clik_pinv_constraint_values(ctrl._handle, R, B, None, 0, 0, ptr(sl["Q3"]), None, ptr(sl["Y3"]),
                                                   B * d.n_y, ptr(sl["E"]), ptr(sl["J"]), ptr(sl["Et"]),
                                                   current_stream(ctrl._device))
        assert rc == 0, rc
    bound = [ctrl.bind_batch(sl["Q"], input_var=sl["Y"]) for sl in slots]
    # the same tick by the kernel that reads the skill image, as the read-out does (the default has the numbers compiled in)
    plain = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk),
                                       options=dict(skills.STACK_OPTIONS, function_opts={"jit_values": False}))
    plain.setup_problem_functions()
    bound_img = [plain.bind_batch(sl["Q"], input_var=sl["Y"]) for sl in slots]
    res = interleaved({
        "tick": lambda s: bound[s](0.0),
        "tick_img": lambda s: bound_img[s](0.0),
        "e": lambda s: ctrl.constraint_values_batch(0.0, slots[s]["Q3"], input_var=slots[s]["Y3"], out=slots[s]["E"]),
        "ejt": full,
        "copy_e": lambda s: copy_e[s][1].copy_(copy_e[s][0]),
        "copy_j": lambda s: copy_j[s][1].copy_(copy_j[s][0]),
    })
    out = ["", "### Headline skill (config 3), %d rows = %d instances x %d records, `%s` tick" % (
        rows, B, R, ctrl.kernel_variant(rows)), "",
        "| launch | us, median (min) of %d replays of %d captured launches | bytes read + written |" % (ROUNDS, INNER), "|---|---|---|",
        "| `solve_batch` tick on %d instances (yardstick) | %.2f (%.2f) | |" % ((rows,) + res["tick"]),
        "| the same tick by the image-reading kernel (`%s`) | %.2f (%.2f) | |" % ((plain.kernel_variant(rows),) + res["tick_img"]),
        "| `constraint_values_batch`, e only | %.2f (%.2f) | %.1f MB |" % (res["e"] + ((read_b + write_e) / 1e6,)),
        "| device-to-device copy moving the same bytes | %.2f (%.2f) | %.1f MB |" % (res["copy_e"] + ((read_b + write_e) / 1e6,)),
        "| `constraint_values_batch(jacobian=True)`: e, J, e_t | %.2f (%.2f) | %.1f MB |" % (res["ejt"] + ((read_b + write_j) / 1e6,)),
        "| device-to-device copy moving the same bytes | %.2f (%.2f) | %.1f MB |" % (res["copy_j"] + ((read_b + write_j) / 1e6,)),
        "", "e only / tick = %.3f; jacobian=True / copy = %.2f (build flags: %s)" % (res["e"][0] / res["tick"][0], res["ejt"][0] / res["copy_j"][0],
                                                                                   os.environ.get("CLIK_JIT_DEFINES") or "none")]
    print("\n".join(out), flush=True)
    return out


def host_inclusive_part():
    import notebook_figures as cf
    import figure_skills
    import time_skills
    from oracle import clik_oracle
    n_ticks, Bm = 256, 64
    spec = time_skills.moe_spec(cf.moe_fk())
    ctrl = cc.PseudoInverseController(skill_spec=spec, options={"time_on_device": True})
    ctrl.setup_problem_functions()
    Q = time_skills.UR5_HOME + np.random.default_rng(0).normal(scale=0.05, size=(Bm, 6))
    times = cf.MOE_DT * np.arange(n_ticks)
    Td, Qd = torch.from_numpy(times).cuda(), torch.from_numpy(Q).cuda()
    kw = dict(dt=cf.MOE_DT, max_speed=figure_skills.MOE_MAX_SPEED, record_every=1)

    def device_loop():
        rec = ctrl.rollout_batch(Td, Qd, **kw)[-1]
        return rec, ctrl.constraint_values_batch(Td, rec["q"])
    device_loop()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        t = time.perf_counter()
        rec, e = device_loop()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    t = time.perf_counter()
    rec = ctrl.rollout_batch(Td, Qd, **kw)[-1]
    q_host = rec["q"].cpu().numpy()
    ref = np.stack([np.concatenate([clik_oracle.ExprEvaluator(spec, times[r], q_host[r], None).vector(c.expression)[0]
                                    for c in spec.constraints], axis=1) for r in range(n_ticks)])
    host = time.perf_counter() - t
    err = float(np.abs(e.cpu().numpy() - ref).max())
    out = ["", "### Host-inclusive: Moe-2016 pinv rollout, %d ticks, %d instances, `record_every=1`, then the error curve" % (
        n_ticks, Bm), "", "| loop | wall time |", "|---|---|",
        "| time table + recording rollout + ONE `constraint_values_batch` (three launches) | %.2f ms |" % (best * 1e3),
        "| the same rollout + host evaluation of the %d records (`ExprEvaluator`) | %.1f ms |" % (n_ticks, host * 1e3),
        "", "max |device - host| over the curve: %.2g" % err]
    print("\n".join(out), flush=True)
    return out


def main():
    out = device_part() + ([] if "--device-only" in sys.argv else host_inclusive_part())
    if WRITE:
        path = os.path.join(ROOT, "profiles", "constraint_values.md")
        text = open(path).read() if os.path.exists(path) else "# constraint_values_batch\n"
        mark = "<!-- tools/constraint_values_bench.py -->"
        text = text.split(mark)[0].rstrip("\n") + "\n\n" + mark + "\n" + "\n".join(out) + "\n"
        with open(path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
