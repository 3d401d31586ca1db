"""CPU: the recording / per-tick-target rollouts of the BASELINE skills compile for gfx950 without scratch memory, as
kernels of their own (``*_rec_kernel``) beside the rollouts that record nothing."""
import ctypes as C
import os
import subprocess

import pytest

import casclik_amd as cc
from casclik_amd import skills


def _resources(tmp_path, text, init, flags):
    from casclik_amd import jit
    from casclik_amd.build import parse_resource_remarks, FLAGS
    hipcc = jit._hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    src = tmp_path / "rec.hip"
    src.write_text(text)
    # (compiled as shipped: with the scheduling strategy jit.py picks for this translation unit)
    out = subprocess.run([hipcc] + FLAGS + flags + jit.sched_flags(jit.sched_strategy(text, init)) + [
        "-c", str(src), "-o", str(tmp_path / "rec.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-2000:]
    return parse_resource_remarks(out.stdout.decode())


def _with_words(template, words):
    return template.replace("%(nwords)d", str(len(words))).replace("%(words)s", ", ".join(w + "ull" for w in words))


def test_recording_rollouts_of_the_config3_skill_have_no_scratch(tmp_path):
    """four lanes per instance and one lane per instance, Euler and Runge-Kutta, with the skill's numbers compiled in
    (jit._VALUE_REC_TEMPLATE) and reading the image (jit._REC_TEMPLATE)"""
    from casclik_amd import jit, _capi
    from casclik_amd.lowering import lower_skill
    lib = _capi.load_library()
    spec = skills.stack_skill(skills.iiwa())
    cdesc = _capi.desc_to_c(lower_skill(spec))
    copts = _capi.pinv_opts_to_c(cc.PseudoInverseController(skill_spec=spec, options=dict(skills.STACK_OPTIONS)).options)
    ok, init = jit.shape_of(lib, cdesc, copts)
    assert ok
    words = jit.host_image_words(lib, "pinv", cdesc, copts)
    res = _resources(tmp_path, _with_words(jit._VALUE_REC_TEMPLATE, words) % {"init": init, "extern": ""}, init,
                     ["-DCLIK_VALUE_KERNEL"])
    kernels = {k: v for k, v in res.items() if "_rec_kernel" in k}
    assert len(kernels) == 4 and len(res) == 4, sorted(res)         # (nothing but the recording rollouts in this unit)
    assert sum("pinv_rollout_static_team_rec_kernel" in k for k in kernels) == 2
    assert sum("pinv_rollout_static_values_rec_kernel" in k for k in kernels) == 2
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0, (name, r)
    res = _resources(tmp_path, jit._REC_TEMPLATE % {"init": init, "extern": ""}, init, [])
    assert len(res) == 4 and all("_rec_kernel" in k for k in res), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)


def test_recording_rollouts_of_the_config4_skill_have_no_scratch(tmp_path):
    from casclik_amd import jit, _capi
    from casclik_amd.lowering import lower_skill
    lib = _capi.load_library()
    spec = skills.qp_skill(skills.iiwa())
    d = lower_skill(spec)
    cdesc = _capi.desc_to_c(d)
    qc = cc.ReactiveQPController(skill_spec=spec)
    state_w = list(qc._robot_var_weights) + list(qc._virtual_var_weights[:d.n_x])
    copts = _capi.qp_opts_to_c(qc.weight_shifter, state_w, qc._slack_var_weights, int(qc.options.get("max_iter", 0)))
    buf = C.create_string_buffer(8192)
    assert lib.clik_qp_shape_describe(C.byref(cdesc), buf, len(buf)) == 1
    init = buf.value.decode()
    words = jit.host_image_words(lib, "qp", cdesc, copts)
    for text, flags, kernel in ((_with_words(jit._QP_VALUE_REC_TEMPLATE, words), ["-DCLIK_VALUE_KERNEL"],
                                 "qp_rollout_static_box_values_rec_kernel"),
                                (jit._QP_REC_TEMPLATE, [], "qp_rollout_static_rec_kernel")):
        res = _resources(tmp_path, text % {"init": init, "extern": ""}, init, flags)
        assert len(res) == 2 and all(kernel in k for k in res), sorted(res)
        for name, r in res.items():
            assert r["ScratchSize"] == 0, (name, r)


def test_skills_with_more_sets_than_the_recording_rollout_holds_get_none():
    """six SetConstraints (64 mode bodies) spill in the recording rollout: jit.attach_rec instantiates none for them"""
    from casclik_amd import jit
    assert jit.REC_MAX_SETS == 5
    assert "clik_jit_rollout_rec" in jit._REC_TEMPLATE and "clik_jit_value_rollout_rec" in jit._VALUE_REC_TEMPLATE
    assert "clik_jit_qp_rollout_rec" in jit._QP_REC_TEMPLATE and "clik_jit_qp_value_rollout_rec" in jit._QP_VALUE_REC_TEMPLATE


def test_the_recording_kernels_stay_out_of_the_other_translation_units():
    """The compiler's code for the rollouts that record nothing depends on what else their translation unit declares
    (declaring the recording templates beside them reordered their fused multiply-adds and moved the team Euler rollout
    off the tick kernel's result): the recording kernels live in headers that only the recording units include."""
    from casclik_amd import jit
    from casclik_amd.build import CSRC
    for name in os.listdir(CSRC):
        # (clik_api.hip holds no kernel; its clik_*_attach_rec_kernel entry points are not meant)
        if name.endswith((".hpp", ".hip")) and name not in ("clik_pinv_rec.hpp", "clik_qp_rec.hpp", "clik_api.hip"):
            text = open(os.path.join(CSRC, name)).read()
            assert "_rec_kernel" not in jit._code_only(text) and "_rec.hpp" not in jit._code_only(text), name
    for tmpl in (jit._TEMPLATE, jit._VALUE_TEMPLATE, jit._QP_TEMPLATE, jit._QP_VALUE_TEMPLATE):
        assert "_rec.hpp" not in tmpl
    for tmpl, header in ((jit._REC_TEMPLATE, "clik_pinv_rec.hpp"), (jit._VALUE_REC_TEMPLATE, "clik_pinv_rec.hpp"),
                         (jit._QP_REC_TEMPLATE, "clik_qp_rec.hpp"), (jit._QP_VALUE_REC_TEMPLATE, "clik_qp_rec.hpp")):
        assert '#include "%s"' % header in tmpl
