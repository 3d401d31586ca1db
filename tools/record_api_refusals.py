#!/usr/bin/env python
"""Run the table of tests/api_refusal_cases.py against the library that is built and write what every refused call
answers - {case id: [return code, clik_last_error text]} - to tests/golden/api_refusals.json.

The recording is what a later change of the host API is held to (tests/test_api_refusals.py, tests/test_gpu_api_refusals.py):
run this on the commit BEFORE such a change, never on the changed code.

  python tools/record_api_refusals.py            the cases on host-only handles and the calls without a handle (no GPU)
  python tools/record_api_refusals.py --device   the cases on device handles as well, and what describes the skills a device
                                                  handle holds (needs a GPU)
  --out FILE                                      write there instead (entries of the file that this run does not make stay)
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
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "api_refusals.json"))
    args = ap.parse_args()
    import api_refusal_cases as arc
    from casclik_amd import _capi, skills
    lib = _capi.load_library()
    if args.device:
        import torch
        scratch = torch.zeros(1 << 17, dtype=torch.float64, device="cuda")
        runner = arc.Runner(lib, skills.iiwa(), skills.ur5(), True, scratch.data_ptr())
        got = runner.run_all(("dev", "full"))
        got.update(runner.setup_results())
        got.update(runner.describe_handles())
    else:
        import numpy as np
        scratch = np.zeros(1 << 17)
        runner = arc.Runner(lib, skills.iiwa(), skills.ur5(), False, scratch.ctypes.data)
        got = runner.run_all(("host", "free"))
        got.update(runner.describe_handles(("host",)))
    runner.close()
    old = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
    old.update(got)
    with open(args.out, "w") as f:
        json.dump(old, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases recorded, %d in %s" % (len(got), len(old), args.out))


if __name__ == "__main__":
    main()
