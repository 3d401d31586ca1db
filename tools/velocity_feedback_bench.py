#!/usr/bin/env python3
"""Device time per tick of a skill with memory - the QP skill of tests/velocity_feedback_cases.py: config 4 plus an
acceleration limit around the last velocity, read in input_var[7:14] - over 256 ticks:
  (a) `rollout_batch` with `options["velocity_feedback"]`: one launch, the lane kernel feeds the velocity back;
  (b) the same lane kernel with the option off - a controller without it, held to the image-reading lane kernel
      (`jit_values` off, a `record_every` beyond the last tick, so the recording rollout runs and records nothing).  It
      computes another trajectory (its limit stays around the first velocity); it is the parent's code, what (a) adds to;
  (c) the launch-per-tick loop (a) replaces: `solve_batch` on device tensors, `q += dq * dt` and the fed entries
      rewritten with torch kernels in between, no host synchronisation inside the loop.
Then (a) and (b) once more with the limit set so wide (WIDE) that it never binds: the fed entries are still written and
read every tick, but the two launches now solve the same QPs and end in the same state, so their difference is what the
feed itself costs.  With the limit of the tests (b) stays bounded around the velocity before the launch, another
trajectory with other working sets, and the QP's passes are data dependent.
    python tools/velocity_feedback_bench.py [B ...  default 16384 131072] [--out FILE]
Timing as tools/converge_bench.py: HIP events around the call on device tensors, `WARMUP` calls first, the median of `REPS`
(min .. max beside it), the calls rotating through `SETS` copies of the inputs.  `--out` writes the table (markdown)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np          # noqa: E402
import torch                # noqa: E402

import casclik_amd as cc    # noqa: E402
from casclik_amd import skills      # noqa: E402
import velocity_feedback_cases as V        # noqa: E402
from converge_bench import reach_inputs, timed, REPS, SETS      # noqa: E402

SIZES = [int(a) for a in sys.argv[1:] if a.isdigit()] or [16384, 131072]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
N_TICKS, DT = 256, V.DT
WIDE = 1.0e3


def measure(fed, plain, loop, B, what="an acceleration limit"):
    fk = skills.iiwa()
    sets = []
    for k in range(SETS):
        Q, Y7 = reach_inputs(fk, B, seed=60 + k)
        sets.append((torch.from_numpy(Q).cuda(), torch.from_numpy(np.hstack([Y7, np.zeros((B, 7))])).cuda()))
    times = DT * np.arange(N_TICKS)

    def a(k):
        q, y = sets[k % SETS]
        return fed.rollout_batch(times, q, input_var=y, dt=DT)

    def b(k):
        q, y = sets[k % SETS]
        return plain.rollout_batch(times, q, input_var=y, dt=DT, record_every=N_TICKS + 1)

    def c(k):
        q, y = sets[k % SETS]
        q, y = q.clone(), y.clone()
        for tv in times:
            dq = loop.solve_batch(float(tv), q, input_var=y)[0]
            q.add_(dq, alpha=DT)
            y[:, 7:] = dq
        return q

    per = lambda t: tuple(x / N_TICKS for x in t)       # noqa: E731
    qa, qb = a(0)[0], b(0)[0]
    ta, tb = timed(a), timed(b)
    out = ["", "### QP skill with %s: %d instances, %d ticks" % (what, B, N_TICKS), "",
           "| path | device time per tick, median of %d (min .. max), us |" % REPS, "|---|---|",
           "| (a) one launch, velocity fed back | %.3f (%.3f .. %.3f) |" % per(ta),
           "| (b) the same lane kernel, option off | %.3f (%.3f .. %.3f) |" % per(tb)]
    tail = "(a) / (b) = %.4f; max |q(a) - q(b)| after %d ticks = %.2e" % (ta[0] / tb[0], N_TICKS, float((qa - qb).abs().max()))
    if loop is not None:
        # the loop (a) replaces, and that (a) computes what it computes
        tc = timed(c)
        out.append("| (c) one launch per tick, fed entries rewritten in between | %.3f (%.3f .. %.3f) |" % per(tc))
        tail += "; (a) / (c) = %.4f; max |q(a) - q(c)| = %.2e" % (ta[0] / tc[0], float((qa - c(0)).abs().max()))
    out += ["", tail]
    print("\n".join(out), flush=True)
    return out


def controllers(spec, optionss):
    out = []
    for options in optionss:
        ctrl = cc.ReactiveQPController(skill_spec=spec, options=options)
        ctrl.setup_problem_functions()
        ctrl.setup_solver()
        out.append(ctrl)
    return out


def main():
    fk = skills.iiwa()
    fed_off = ({"velocity_feedback": V.FB_IIWA}, {"function_opts": {"jit_values": False}})
    ctrls = controllers(V.qp_skill(fk), fed_off + ({},))
    wide = controllers(V.qp_skill(fk, a_dt=WIDE), fed_off)
    text = []
    for B in SIZES:
        text += measure(*ctrls, B)
        text += measure(*wide, None, B, what="a limit that never binds (a dt = %g)" % WIDE)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
