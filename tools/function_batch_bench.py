#!/usr/bin/env python3
"""Device time of `DeviceFunction` (clik_function.hpp) over the records of a rollout, against its yardsticks:
  tool, manip    the test functions of tests/function_cases.py at R x B rows taken from a recording rollout of the UR5
                 pose skill, per row and against the memory floor (the bytes the call must move over 8 TB/s);
  parent         `constraint_values_batch` (e only) of that pose skill on the same rows: the hand-written forward
                 kinematics + Jacobian, the closest thing the tree measured before;
  host loop      the `Function.__call__` loop the call replaces, measured at 256 rows and SCALED to R x B.
    python tools/function_batch_bench.py [B=16384] [R=256] [--write]
Timing: every variant works on a ring of input / output buffer sets; `INNER` launches are captured into one graph per
variant and a replay is timed between two HIP events, `ROUNDS` interleaved rounds of all variants in one process; median
and minimum are reported.  `--write` puts the tables into profiles/function_batch.md.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np          # noqa: E402
import torch                # noqa: E402

import casclik_amd as cc    # noqa: E402
from casclik_amd import codegen, jit, skills      # noqa: E402
import function_cases as fc                       # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args else 16384
R = int(args[1]) if len(args) > 1 else 256
WRITE = "--write" in sys.argv
RING, INNER, ROUNDS = 2, 5, 7
HBM_BYTES_PER_US = 8.0e6        # 8 TB/s


def interleaved(variants):
    """{name: (median, min)} us per call of each fn(slot), see the module text"""
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


def resources():
    """registers / LDS / scratch of the four test kernels from the compiler's remarks (no GPU needed)"""
    out = ["", "### The four test kernels (compiler remarks, gfx950)", "",
           "| function | inputs -> outputs (entries) | VGPRs | SGPRs | scratch | occupancy | LDS per block |", "|---|---|---|---|---|---|---|"]
    for name in fc.NAMES:
        fn = fc.get(name)
        (_, r), = jit.unit_resources(jit.unit_text(jit._FUNCTION_TEMPLATE, "", codegen.emit_function(fn)), "").items()
        ins, outs = codegen.function_layout(fn)
        slots = max([sum(a * b for a, b, _ in ins)] + [a * b for a, b, _ in outs])
        out.append("| `%s` | %s -> %s | %d | %d | %d | %d | %d B |" % (
            name, " + ".join(str(a * b) for a, b, _ in ins), " + ".join(str(a * b) for a, b, _ in outs), r["VGPRs"],
            r["TotalSGPRs"], r["ScratchSize"], r["Occupancy"], 4 * 64 * 8 * slots))
    return out


def main():
    fk = skills.ur5()
    spec = skills.pose_skill(fk)
    ctrl = cc.PseudoInverseController(skill_spec=spec)
    ctrl.setup_problem_functions()
    ctrl.setup_solver()
    rng = np.random.default_rng(3)
    lo, hi = np.array(fk["lower"]), np.array(fk["upper"])
    dt = 0.008
    slots = []
    tool, manip = cc.DeviceFunction(fc.get("tool")), cc.DeviceFunction(fc.get("manip"))
    times = torch.from_numpy(dt * np.arange(R)).cuda()
    for s in range(RING):
        Q = rng.uniform(0.4 * lo, 0.4 * hi, size=(B, 6))
        Y = np.concatenate([rng.uniform(-0.4, 0.4, size=(B, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (B, 1))], axis=1)
        Qd, Yd = torch.from_numpy(Q).cuda(), torch.from_numpy(Y).cuda()
        rec = ctrl.rollout_batch(dt * np.arange(R), Qd, input_var=Yd, dt=dt, max_speed=0.6, record_every=1)[-1]
        q = rec["q"]
        slots.append({"q": q, "Y": Yd, "E": torch.empty((R, B, 6), dtype=torch.float64, device="cuda"),
                      "tool": (torch.empty((R, B, 4, 4), dtype=torch.float64, device="cuda"),
                               torch.empty((R, B, 3), dtype=torch.float64, device="cuda")),
                      "manip": (torch.empty((R, B, 3), dtype=torch.float64, device="cuda"),
                                torch.empty((R, B, 3, 6), dtype=torch.float64, device="cuda"),
                                torch.empty((R, B), dtype=torch.float64, device="cuda"))})
        del rec
    rows = R * B
    res = interleaved({
        "tool": lambda s: tool(slots[s]["q"], out=slots[s]["tool"]),
        "manip": lambda s: manip(times, slots[s]["q"], out=slots[s]["manip"]),
        "parent": lambda s: ctrl.constraint_values_batch(0.0, slots[s]["q"], input_var=slots[s]["Y"], out=slots[s]["E"]),
    })
    bytes_of = {"tool": rows * (6 + 19) * 8, "manip": rows * (6 + 22) * 8 + R * 8, "parent": rows * (6 + 6) * 8 + B * 7 * 8}
    out = ["", "### %d rows = %d records x %d instances of a recording rollout (UR5 pose skill)" % (rows, R, B), "",
           "| launch | us, median (min) of %d replays of %d captured launches | ns per row | bytes moved | memory floor at 8 TB/s | time / floor |" % (ROUNDS, INNER),
           "|---|---|---|---|---|---|"]
    label = {"tool": "`tool` (T 4x4 and p)", "manip": "`manip` (p, J_p 3x6, manipulability cost)",
             "parent": "`constraint_values_batch`, e only, pose skill (parent commit's kernel)"}
    for k in ("tool", "manip", "parent"):
        floor = bytes_of[k] / HBM_BYTES_PER_US
        out.append("| %s | %.1f (%.1f) | %.3f | %.0f MB | %.1f us | %.2f |" % (
            label[k], res[k][0], res[k][1], res[k][0] * 1e3 / rows, bytes_of[k] / 1e6, floor, res[k][0] / floor))
    out += ["", "`tool` / parent = %.2f, `manip` / parent = %.2f" % (res["tool"][0] / res["parent"][0],
                                                                    res["manip"][0] / res["parent"][0])]
    # the host loop DeviceFunction replaces, at 256 rows, scaled
    qh = slots[0]["q"][:, 0].cpu().numpy()[:256]
    n = len(qh)
    host = {}
    for name, call in (("tool", lambda i: fc.get("tool")(qh[i])), ("manip", lambda i: fc.get("manip")(0.0, qh[i]))):
        call(0)
        t = time.perf_counter()
        for i in range(n):
            call(i)
        host[name] = (time.perf_counter() - t) / n
    out += ["", "### The host loop it replaces (`Function.__call__` per row, measured at %d rows)" % n, "",
            "| function | host, per row | host, SCALED to %d rows | device, one launch | ratio |" % rows, "|---|---|---|---|---|"]
    for name in ("tool", "manip"):
        out.append("| `%s` | %.0f us | %.0f s (scaled) | %.1f us | %.1e |" % (
            name, host[name] * 1e6, host[name] * rows, res[name][0], host[name] * rows * 1e6 / res[name][0]))
    out += resources()
    print("\n".join(out), flush=True)
    if WRITE:
        path = os.path.join(ROOT, "profiles", "function_batch.md")
        text = open(path).read() if os.path.exists(path) else "# DeviceFunction\n"
        mark = "<!-- tools/function_batch_bench.py -->"
        text = text.split(mark)[0].rstrip("\n") + "\n\n" + mark + "\n" + "\n".join(out) + "\n"
        with open(path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
