"""CPU: the recording / per-tick-target rollouts of the BASELINE skills compile for gfx950 without scratch memory, as
kernels of their own (``*_rec_kernel``) beside the rollouts that record nothing."""
import os

import pytest

import casclik_amd as cc
from casclik_amd import skills


def _request(ctrl):
    """the request of a BASELINE skill's controller with its image words; its units are compiled as shipped"""
    from casclik_amd import jit
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req = jit.unit_request(ctrl, words=True)
    assert req.eligible and req.extern == ""
    return req


def test_recording_rollouts_of_the_config3_skill_have_no_scratch():
    """four lanes per instance and one lane per instance, Euler and Runge-Kutta, with the skill's numbers compiled in
    (jit._VALUE_REC_TEMPLATE) and reading the image (jit._REC_TEMPLATE)"""
    from casclik_amd import jit
    req = _request(cc.PseudoInverseController(skill_spec=skills.stack_skill(skills.iiwa()), options=dict(skills.STACK_OPTIONS)))
    init = req.init
    res = jit.unit_resources(jit.unit_text(jit._VALUE_REC_TEMPLATE, init, "", req.words), init, jit.VALUE_DEFINES)
    kernels = {k: v for k, v in res.items() if "_rec_kernel" in k}
    assert len(kernels) == 4 and len(res) == 4, sorted(res)         # (nothing but the recording rollouts in this unit)
    assert sum("pinv_rollout_static_team_rec_kernel" in k for k in kernels) == 2
    assert sum("pinv_rollout_static_values_rec_kernel" in k for k in kernels) == 2
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0, (name, r)
    res = jit.unit_resources(jit.unit_text(jit._REC_TEMPLATE, init), init)
    assert len(res) == 4 and all("_rec_kernel" in k for k in res), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, (name, r)


def test_recording_rollouts_of_the_config4_skill_have_no_scratch():
    from casclik_amd import jit
    req = _request(cc.ReactiveQPController(skill_spec=skills.qp_skill(skills.iiwa())))
    for tmpl, words, defines, kernel in ((jit._QP_VALUE_REC_TEMPLATE, req.words, jit.VALUE_DEFINES,
                                          "qp_rollout_static_box_values_rec_kernel"),
                                         (jit._QP_REC_TEMPLATE, None, (), "qp_rollout_static_rec_kernel")):
        res = jit.unit_resources(jit.unit_text(tmpl, req.init, "", words), req.init, defines)
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
