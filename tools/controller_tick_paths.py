#!/usr/bin/env python3
"""Host cost per call of the controllers' tick paths in two checkouts of this repository, measured alternately: what a
change of the Python controllers is held to (profiles/controller_tick_paths.md).

    python tools/controller_tick_paths.py PARENT_TREE CHILD_TREE [--repeats 5] [--markdown FILE]

Per repeat and tree, each in a process of its own: tools/solve_latency.py (solve() of both controllers),
tools/host_roundtrip.py 64 (numpy-in / numpy-out solve_batch and the bound tick at a batch where the host dominates)
and the QP controller's bound tick with hot_start=True (`qp_bound_tick` below) - each started as this file with
`--run TREE SCRIPT`, which imports the tree's own package before the script runs.  The margin is the
parent's own spread: a figure passes when the child's median over the repeats lies within the parent's median plus
(max - min) of the parent's repeats.  GPU box only; ends at the first run that fails."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time


def run_in_tree(tree, script, argv):
    """Run one measurement on the package of ``tree``: its ``casclik_amd`` is imported first, so whatever path the
    script puts in front afterwards, that is the package it measures.  ``script``: a file of the tree, or "qp-bound-tick"."""
    sys.path.insert(0, tree)
    import casclik_amd
    assert os.path.abspath(casclik_amd.__file__).startswith(tree + os.sep), (casclik_amd.__file__, tree)
    if script == "qp-bound-tick":
        return qp_bound_tick()
    import runpy
    sys.argv = [os.path.join(tree, script)] + list(argv)
    runpy.run_path(sys.argv[0], run_name="__main__")


def qp_bound_tick(B=64):
    import torch
    import casclik_amd as cc
    from casclik_amd import skills
    fk = skills.iiwa()
    ctrl = cc.ReactiveQPController(skill_spec=skills.qp_skill(fk))
    ctrl.setup_problem_functions()
    ctrl.setup_solver()
    Q, Y = skills.synthetic_inputs(fk, B, seed=0, distribution="mixed")
    tick = ctrl.bind_batch(torch.from_numpy(Q).cuda(), input_var=torch.from_numpy(Y).cuda(), hot_start=True)
    for _ in range(50):
        tick()
    torch.cuda.synchronize()
    n = 2000
    t0 = time.perf_counter()
    for _ in range(n):
        tick()
    torch.cuda.synchronize()
    print("qp bound tick hot_start: %.2f us per tick" % ((time.perf_counter() - t0) / n * 1e6))


# figure -> (script arguments relative to the tree | None: this file, pattern of its line)
RUNS = (
    (["tools/solve_latency.py"], {"pinv solve()": r"pinv stack\s+solve\(\): ([0-9.]+) us",
                                  "qp solve()": r"reactive qp\s+solve\(\): ([0-9.]+) us"}),
    (["tools/host_roundtrip.py", "64"], {"pinv solve_batch numpy B=64": r"numpy in / numpy out ([0-9.]+) us",
                                         "pinv bound tick B=64": r"device-resident ([0-9.]+) us"}),
    (None, {"qp bound tick hot_start B=64": r"qp bound tick hot_start: ([0-9.]+) us"}),
)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--run":
        return run_in_tree(os.path.abspath(sys.argv[2]), sys.argv[3], sys.argv[4:])
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("child")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    trees = (("parent", os.path.abspath(args.parent)), ("child", os.path.abspath(args.child)))
    got = {who: {} for who, _ in trees}
    for rep in range(args.repeats):
        for who, tree in trees:
            for script, figures in RUNS:
                cmd = [sys.executable, os.path.abspath(__file__), "--run", tree] + (script or ["qp-bound-tick"])
                run = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=120)
                if run.returncode != 0:
                    sys.exit("%s failed (%d):\n%s\n%s" % (" ".join(cmd), run.returncode, run.stdout[-2000:], run.stderr[-2000:]))
                for name, pattern in figures.items():
                    got[who].setdefault(name, []).append(float(re.search(pattern, run.stdout).group(1)))
        print("repeat %d done" % (rep + 1), flush=True)
    lines = ["| figure (us per call) | parent repeats | parent median | parent spread | child repeats | child median | within |",
             "|---|---|---|---|---|---|---|"]
    ok = True
    for name in got["parent"]:
        p, c = got["parent"][name], got["child"][name]
        pm, cm, spread = statistics.median(p), statistics.median(c), max(p) - min(p)
        fine = cm <= pm + spread
        ok = ok and fine
        lines.append("| %s | %s | %.2f | %.2f | %s | %.2f | %s |" % (
            name, " ".join("%.2f" % v for v in p), pm, spread, " ".join("%.2f" % v for v in c), cm, "yes" if fine else "NO"))
    lines.append("")
    lines.append("verdict: %s" % ("every child median lies within the parent's median plus its spread" if ok
                                  else "a child median lies beyond the parent's median plus its spread"))
    print("\n".join(lines))
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
