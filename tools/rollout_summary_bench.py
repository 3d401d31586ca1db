#!/usr/bin/env python3
"""Device time per tick of the rollout that summarises its constraint values while it runs (`rollout_batch(...,
summary=True)`) for the headline skill (config 3), 256 ticks per launch, against
  (a) the plain rollout, and
  (b) what answered the same questions before: the `record_every=1` rollout plus `constraint_summary_batch` on its record.
    python tools/rollout_summary_bench.py [B ...  default 16384 131072] [--write]
Timing as tools/rollout_record_bench.py: HIP events around the call(s) on device tensors, one warm-up first, the best of
`REPS` repetitions; every call gets new state, record and output tensors.  Beside the times: the peak of device memory a
call allocates (torch's allocator, over what the inputs hold) and the LDS bytes of a block of the new kernels.  `--write`
puts the tables between the two markers of profiles/rollout_summary.md.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import torch                # noqa: E402

import casclik_amd as cc    # noqa: E402
from casclik_amd import skills      # noqa: E402

SIZES = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [16384, 131072]
WRITE = "--write" in sys.argv
REPS = 5
N_TICKS, DT, VMAX, TOL = 256, 0.008, np.pi / 5, 1e-3


def timed(fn):
    """(best device time of fn() in microseconds, peak bytes it allocated), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    best = float("inf")
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3)
    return best, torch.cuda.max_memory_allocated() - base


def measure(ctrl, B):
    fk = skills.iiwa()
    Q, Y = skills.synthetic_inputs(fk, B, seed=1, distribution="mixed")
    Qd, Yd = torch.from_numpy(Q).cuda(), torch.from_numpy(Y).cuda()
    times = np.zeros(N_TICKS)
    kw = dict(input_var=Yd, dt=DT, max_speed=VMAX)

    def plain():
        return ctrl.rollout_batch(times, Qd, **kw)

    def record_then_summarise():
        rec = ctrl.rollout_batch(times, Qd, record_every=1, **kw)[-1]
        # (the records are the states AFTER the ticks: the same number of records and the same work as the summary below,
        # whose records are the states before them)
        return ctrl.constraint_summary_batch(times, rec["q"], input_var=Yd, tol=TOL)

    def summarising():
        return ctrl.rollout_batch(times, Qd, summary=True, summary_tol=TOL, **kw)[-1]

    rows = [("(a) plain rollout", ctrl.kernel_variant(B)) + timed(plain),
            ("(b) `record_every=1` + `constraint_summary_batch`", ctrl.kernel_variant(B) + " + summary kernels")
            + timed(record_then_summarise),
            ("(c) `summary=True`", "lane, summarising") + timed(summarising)]
    out = ["", "### config 3 (headline): %d instances, %d ticks per launch" % (B, N_TICKS), "",
           "| path | kernel | us per tick (device) | peak bytes allocated by a call |", "|---|---|---|---|"]
    for label, kernel, us, peak in rows:
        out.append("| %s | %s | %.3f | %d |" % (label, kernel, us / N_TICKS, peak))
    a, b, c = (r[2] for r in rows)
    out += ["", "(c) / (b) = %.3f, (c) / (a) = %.3f" % (c / b, c / a)]
    print("\n".join(out), flush=True)
    return out


def lds_line(ctrl):
    """the LDS bytes of a block of the attached summarising kernels, from the loaded unit itself"""
    from casclik_amd import jit
    for so, lib in jit._loaded.items():
        if hasattr(lib, "clik_jit_rollsum_info") and ctrl._kernels.get("rollsum") and ctrl._kernels.get("rollsum") in so:
            info = lib.clik_jit_rollsum_info
            info.restype, info.argtypes = C.c_longlong, [C.c_int]
            return ("A block of the summarising kernels: Euler %d wave(s), %d bytes of LDS; Runge-Kutta %d wave(s), %d bytes; "
                    "scratch per lane as the loaded code object states it: %d / %d bytes."
                    % (info(7), info(4), info(8), info(2), info(5), info(6)))
    return ""


def main():
    fk = skills.iiwa()
    ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
    ctrl.setup_problem_functions()
    text = []
    for B in SIZES:
        text += measure(ctrl, B)
    text += ["", lds_line(ctrl)]
    print(text[-1])
    if WRITE:
        path = os.path.join(ROOT, "profiles", "rollout_summary.md")
        marker, end = "<!-- rollout_summary_bench -->", "<!-- rollout_summary_bench end -->"
        old = open(path).read() if os.path.exists(path) else "# Rollouts that summarise while they run\n\n"
        if marker not in old or end not in old:
            old += marker + "\n" + end + "\n"
        with open(path, "w") as f:
            f.write(old[:old.index(marker) + len(marker)] + "\n" + "\n".join(text) + "\n" + old[old.index(end):])


if __name__ == "__main__":
    main()
