#!/usr/bin/env python3
"""Device time of ONE `constraint_summary_batch` launch pair (clik_summary.hpp) on the headline skill over a recorded
trajectory, against the route it replaces: `constraint_values_batch` (e only) over the same trajectory, alone and followed
by the torch reductions that yield `abs_max`, `last` and `rms` (that route cannot produce the violation outputs).
    python tools/constraint_summary_bench.py [B=16384] [R=256] [--write] [--resources]
Device tensors in, every buffer allocated beforehand (the C entry points, on the current stream), a ring of two
trajectories; `INNER` calls are timed between two HIP events, `ROUNDS` interleaved rounds of all variants in one process
after a warm-up round; median and minimum are reported.  `--resources` compiles the unit and prints the registers, LDS and
scratch of its two kernels (no GPU needed); `--write` puts the tables into profiles/constraint_summary.md.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402

import casclik_amd as cc    # noqa: E402
from casclik_amd import jit, skills      # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if args else 16384
R = int(args[1]) if len(args) > 1 else 256
WRITE = "--write" in sys.argv
RING, INNER, ROUNDS = 2, 5, 9
MARK = "<!-- tools/constraint_summary_bench.py %s -->"


def resources_part():
    """registers / LDS / scratch of the two kernels, from the compiler's resource remarks"""
    import ctypes as C
    ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(skills.iiwa()), options=dict(skills.STACK_OPTIONS))
    req = jit.unit_request(ctrl)
    assert req.eligible
    out = ["", "### Kernel resources (headline skill, compiler remarks)", "",
           "| kernel | VGPR | AGPR | SGPR | LDS bytes | scratch | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|---|"]
    res = jit.unit_resources(jit.unit_text(jit._SUMMARY_TEMPLATE, req.init, req.extern), req.init)
    so, _ = jit.build_shape_library(req.init, template=jit._SUMMARY_TEMPLATE, extern=req.extern)      # (the shipped object)
    unit = C.CDLL(so)
    unit.clik_jit_summary_info.restype = C.c_longlong
    lds = int(unit.clik_jit_summary_info(2))
    for name, r in sorted(res.items()):
        short = "constraint_summary_combine_kernel" if "combine" in name else "constraint_summary_kernel"
        out.append("| `%s` | %d | %d | %d | %d | %d | %d |" % (
            short, r.get("VGPRs", 0), r.get("AGPRs", 0), r.get("TotalSGPRs", r.get("SGPRs", 0)), 0 if "combine" in name else lds,
            r.get("ScratchSize", 0), r.get("Occupancy", 0)))
    print("\n".join(out), flush=True)
    return out


def interleaved(variants):
    """{name: (median, min)} us per call of each fn(slot)"""
    import torch
    for fn in variants.values():            # (warm-up: every variant on every slot)
        for s in range(RING):
            fn(s)
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(INNER):
                fn(i % RING)
            b.record()
            b.synchronize()
            samples[name].append(a.elapsed_time(b) * 1e3 / INNER)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in samples.items()}


def device_part():
    import torch
    from casclik_amd.controllers.base_controller import current_stream, ptr
    fk = skills.iiwa()
    ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
    ctrl.setup_problem_functions()
    d, dev = ctrl.descriptor, ctrl._device
    m_tot = max(sl.stop for sl in ctrl.constraint_rows().values())
    # (4096 synthetic states and targets, drawn with replacement and jittered; one target per instance for all records)
    Q0, Y0 = skills.synthetic_inputs(fk, 4096, seed=10, distribution="mixed")
    rng = np.random.default_rng(11)
    slots = []
    for s in range(RING):
        Y = np.ascontiguousarray(Y0[rng.integers(0, len(Q0), size=B)])
        Q = Q0[rng.integers(0, len(Q0), size=R * B)] + rng.normal(scale=1e-3, size=(R * B, Q0.shape[1]))
        slots.append({"Q": torch.from_numpy(Q.reshape(R, B, -1)).to(dev), "Y": torch.from_numpy(Y).to(dev),
                      "E": torch.empty((R, B, m_tot), dtype=torch.float64, device=dev)})
    tol = torch.full((m_tot,), 1e-3, dtype=torch.float64, device=dev)
    first = ctrl.constraint_summary_batch(0.0, slots[0]["Q"], input_var=slots[0]["Y"], tol=1e-3)    # (instantiates)
    e0 = ctrl.constraint_values_batch(0.0, slots[0]["Q"], input_var=slots[0]["Y"], out=slots[0]["E"])
    n_work = int(ctrl._lib.clik_pinv_summary_work_bytes(ctrl._handle, R, B))
    for sl in slots:
        sl["work"] = torch.empty(n_work // 8 + 1, dtype=torch.float64, device=dev)
        sl["out"] = {k: torch.empty((B, m_tot), dtype=v.dtype, device=dev) for k, v in first.items()}

    def summary(s):
        sl, o = slots[s], slots[s]["out"]
        rc = ctrl._lib.clik_pinv_constraint_summary(
            ctrl._handle, R, B, None, 0, 0, ptr(sl["Q"]), None, ptr(sl["Y"]), 0, ptr(tol), ptr(sl["work"]),
            sl["work"].numel() * 8, ptr(o["abs_max"]), ptr(o["abs_max_at"]), ptr(o["last"]), ptr(o["rms"]),
            ptr(o["viol_max"]), ptr(o["viol_count"]), ptr(o["settled_at"]), current_stream(dev))
        assert rc == 0, rc

    def values(s):
        sl = slots[s]
        rc = ctrl._lib.clik_pinv_constraint_values(ctrl._handle, R, B, None, 0, 0, ptr(sl["Q"]), None, ptr(sl["Y"]), 0,
                                                   ptr(sl["E"]), None, None, current_stream(dev))
        assert rc == 0, rc

    def values_reduced(s):
        values(s)
        E = slots[s]["E"]
        return E.abs().amax(dim=0), E[-1], (E * E).mean(dim=0).sqrt()

    # the two routes agree before they are timed
    summary(0)
    amax, last, rms = values_reduced(0)
    torch.cuda.synchronize()
    o = slots[0]["out"]
    agree = (float((o["abs_max"] - amax).abs().max()), float((o["last"] - last).abs().max()),
             float((o["rms"] - rms).abs().max()))
    assert torch.equal(e0, slots[0]["E"])
    res = interleaved({"values": values, "values_reduced": values_reduced, "summary": summary})
    read_b = (R * B * d.n_q + B * d.n_y) * 8
    c = jit.summary_chunk_length(R, B)
    out = ["", "### Headline skill (config 3), %d instances x %d records, chunks of %d records" % (B, R, c), "",
           "| route | us, median (min) of %d rounds of %d calls | bytes written |" % (ROUNDS, INNER), "|---|---|---|",
           "| `constraint_values_batch`, e only (one launch) | %.1f (%.1f) | %.1f MB |" % (res["values"] + (R * B * m_tot * 8 / 1e6,)),
           "| ... followed by the torch reductions for `abs_max`, `last`, `rms` | %.1f (%.1f) | %.1f MB + the reductions' |" % (
               res["values_reduced"] + (R * B * m_tot * 8 / 1e6,)),
           "| `constraint_summary_batch`, all seven outputs (two launches) | %.1f (%.1f) | %.1f MB work + %.1f MB results |" % (
               res["summary"] + (n_work / 1e6, B * m_tot * (4 * 8 + 3 * 4) / 1e6)),
           "", "Both routes read %.1f MB.  summary / values launch = %.3f; summary / (values + reductions) = %.3f." % (
               read_b / 1e6, res["summary"][0] / res["values"][0], res["summary"][0] / res["values_reduced"][0]),
           "max |summary - torch reduction| on the first trajectory: abs_max %.3g, last %.3g, rms %.3g." % agree]
    print("\n".join(out), flush=True)
    return out


def main():
    parts = {}
    if "--resources" in sys.argv:
        parts["resources"] = resources_part()
    if "--resources-only" not in sys.argv:
        parts["times"] = device_part()
    if WRITE:
        path = os.path.join(ROOT, "profiles", "constraint_summary.md")
        text = open(path).read() if os.path.exists(path) else "# constraint_summary_batch\n"
        for key, out in parts.items():
            begin, end = MARK % key, MARK % ("end " + key)
            block = begin + "\n" + "\n".join(out) + "\n" + end
            if begin in text and end in text:
                text = text.split(begin)[0] + block + text.split(end)[1]
            else:
                text = text.rstrip("\n") + "\n\n" + block + "\n"
        with open(path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
