#!/usr/bin/env python3
"""Registers / scratch / occupancy of the value-specialised kernels of a BASELINE skill, from the compiler's resource
remarks (no GPU needed).      python tools/kernel_resources.py [stack|pose|qp] [-DFLAG ...] [--asm=listing.s] [--obj=device.o]
--rec: the recording / per-tick-target rollouts of that skill (jit._VALUE_REC_TEMPLATE / _QP_VALUE_REC_TEMPLATE) instead.
--summary: the two constraint-summary kernels of that skill (jit._SUMMARY_TEMPLATE: image-reading, no numbers compiled in).
--rollsum: the two summarising rollouts of that skill (jit._ROLLSUM_TEMPLATE / _QP_ROLLSUM_TEMPLATE: image-reading, Euler and
Runge-Kutta; their LDS is dynamic - tools/rollout_summary_bench.py prints the launcher's figure).
--converge: the converging rollout of that skill (jit._CONVERGE_TEMPLATE / _QP_CONVERGE_TEMPLATE: pinv_converge_static_kernel /
qp_converge_static_kernel, image-reading, Euler; LDS dynamic - tools/converge_bench.py prints the launcher's figure);
--converge=G: the same unit with the group rule for groups of G lanes (-DCLIK_CONVERGE_GROUP=G, G in 2 .. 64).
--feedback=f0,f1,...: with --rec, --rollsum or --converge[=G] the variant of that unit with the velocity feedback map
compiled in (-DCLIK_VELOCITY_FEEDBACK={f0,f1,...}: one entry per robot and virtual variable, an index into input_var or -1;
--rec is then the image-reading recording rollout, jit.FEEDBACK_UNITS - the lane kernels alone carry the feedback)."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from casclik_amd import jit, skills                  # noqa: E402
import casclik_amd as cc                             # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "qp"
flags = [a for a in sys.argv[2:] if a.startswith(("-D", "-f", "-g"))]
for a in sys.argv[2:]:
    if a.startswith("--mllvm="):                      # e.g. --mllvm=-disable-machine-licm
        flags += ["-mllvm", a.split("=", 1)[1]]
asm_out = [a.split("=", 1)[1] for a in sys.argv[2:] if a.startswith("--asm=")]
obj_out = [a.split("=", 1)[1] for a in sys.argv[2:] if a.startswith("--obj=")]     # device code object (llvm-objdump -d)
# kernel headers from a scratch copy (experiments next to a running build)
csrc = ([a.split("=", 1)[1] for a in sys.argv[2:] if a.startswith("--csrc=")] or [None])[-1]
fk = skills.iiwa()
if which == "qp":
    ctrl = cc.ReactiveQPController(skill_spec=skills.qp_skill(fk))
    template = jit._QP_VALUE_REC_TEMPLATE if "--rec" in sys.argv else jit._QP_VALUE_TEMPLATE
elif which == "stack":
    ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
    template = jit._VALUE_REC_TEMPLATE if "--rec" in sys.argv else jit._VALUE_TEMPLATE
else:
    ctrl = cc.PseudoInverseController(skill_spec=skills.pose_skill(fk))
    template = jit._VALUE_REC_TEMPLATE if "--rec" in sys.argv else jit._VALUE_TEMPLATE
req = jit.unit_request(ctrl, words=True)
words, defines = req.words, jit.VALUE_DEFINES
if "--summary" in sys.argv:
    template, words, defines = jit._SUMMARY_TEMPLATE, None, ()
if "--rollsum" in sys.argv:
    template, words, defines = jit.UNITS["rollsum", req.kind]["template"], None, ()
group = [a for a in sys.argv[2:] if a == "--converge" or a.startswith("--converge=")]
if group:
    # (--converge=G: the unit with the group rule for groups of G lanes, as converge_batch(..., group=G) asks for it)
    template, words = jit.CONVERGE_UNITS["converge", req.kind]["template"], None
    defines = jit.converge_group_defines(int(group[-1].split("=", 1)[1]) if "=" in group[-1] else 1)
feedback = [a.split("=", 1)[1] for a in sys.argv[2:] if a.startswith("--feedback=")]
if feedback:
    if "--rec" in sys.argv:
        template, words, defines = jit.FEEDBACK_UNITS["rec", req.kind]["template"], None, ()
    elif not ("--rollsum" in sys.argv or group):
        sys.exit("--feedback goes with --rec, --rollsum or --converge")
    defines = tuple(defines) + jit.velocity_feedback_defines([int(k) for k in feedback[-1].split(",")])
text = jit.unit_text(template, req.init, req.extern, words)
# (the scheduling strategy the shipped object is compiled with, casclik_amd/jit.py::sched_strategy - unless one is given)
how = dict(extra=defines, csrc=csrc, more=flags, sched=None if any("sched-strategy" in f for f in flags) else "unit")
try:
    res = jit.unit_resources(text, req.init, **how)
except RuntimeError as exc:
    sys.exit(str(exc))
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "k.hip")
    open(src, "w").write(text)
    if asm_out:
        # (the listing tools/isa_count.py reads)
        subprocess.run(jit.unit_command(text, req.init, src, asm_out[0], kind="asm", **how), check=True)
    if obj_out:
        subprocess.run(jit.unit_command(text, req.init, src, obj_out[0], kind="code_object", **how), check=True)
for name, r in sorted(res.items()):
    short = name.split("(")[0][-70:]
    print("%-72s VGPR %3d AGPR %3d SGPR %3d scratch %4d occupancy %d" % (
        short, r.get("VGPRs", 0), r.get("AGPRs", 0), r.get("SGPRs", 0), r.get("ScratchSize", 0), r.get("Occupancy", 0)))
