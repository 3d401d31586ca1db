#!/usr/bin/env python
"""Run the calls of tests/controller_call_cases.py - solve_batch, bind_batch, resident_start and solve of both
controllers, accepted and refused - and write what each one answers to tests/golden/controller_calls.json.

The recording is what a later change of the Python controllers is held to (tests/test_gpu_controller_calls.py): run this
on the commit BEFORE such a change, never on the changed code.  Needs a GPU.

  python tools/record_controller_calls.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "controller_calls.json"))
    args = ap.parse_args()
    import controller_call_cases as ccc
    env = ccc.Env()
    got = {}
    for group in ccc.GROUPS:
        got.update(ccc.run_group(env, group))
        print("%s: %d cases so far" % (group, len(got)), flush=True)
    with open(args.out, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    refused = sum("raises" in v for v in got.values())
    print("%d cases recorded (%d refused) in %s" % (len(got), refused, args.out))


if __name__ == "__main__":
    main()
