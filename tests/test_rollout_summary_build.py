"""CPU: the summarising rollouts (clik_rollout_summary.hpp, jit._ROLLSUM_TEMPLATE / _QP_ROLLSUM_TEMPLATE) - their
translation units cross-compiled for gfx950 without scratch, two kernels each (Euler and Runge-Kutta) and nothing else; a
recorded request replayed by ``prebuild_recorded`` under the name the attach asks for; the tags of every other template
untouched by the new header; and what ``rollout_batch(..., summary=, summary_tol=)`` refuses on the host."""
import hashlib
import os
import re
import shutil

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import jit, skills
from casclik_amd.controllers.base_controller import rollout_summary_request

from extern_skills import mixed_frame_skill

_OLD_TEMPLATES = ("_TEMPLATE", "_VALUE_TEMPLATE", "_QP_TEMPLATE", "_QP_VALUE_TEMPLATE", "_REC_TEMPLATE", "_VALUE_REC_TEMPLATE",
                  "_QP_REC_TEMPLATE", "_QP_VALUE_REC_TEMPLATE", "_TIME_TEMPLATE", "_MONITOR_TEMPLATE", "_SUMMARY_TEMPLATE",
                  "_FUNCTION_TEMPLATE")


def _unit(name):
    """(shape initialiser, generated constraint code, template) of the summarising rollout of a fixture"""
    fk = skills.iiwa()
    if name == "qp":
        ctrl = cc.ReactiveQPController(skill_spec=skills.qp_skill(fk))
    elif name == "stack":
        ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
    else:
        ctrl = cc.PseudoInverseController(skill_spec=mixed_frame_skill(fk), options={"multidim_sets": False})  # (a virtual variable)
    req = jit.unit_request(ctrl)
    assert req.eligible
    return req.init, req.extern, jit.UNITS["rollsum", req.kind]["template"]


@pytest.mark.parametrize("name", ["stack", "mixed", "qp"])
def test_summarising_rollout_compiles_for_gfx950_without_scratch(name):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    init, extern, tmpl = _unit(name)
    res = jit.unit_resources(jit.unit_text(tmpl, init, extern), init)         # (compiled as shipped)
    kernel = "qp_rollout_static_sum_kernel" if name == "qp" else "pinv_rollout_static_sum_kernel"
    assert len(res) == 2 and all(kernel in k for k in res), sorted(res)        # (Euler and Runge-Kutta, nothing else)
    for k, r in res.items():
        assert r["ScratchSize"] == 0, (k, r)
        print(name, k[-50:], r)


def test_the_new_kernels_stay_in_their_own_units():
    from casclik_amd.build import CSRC
    for fn in os.listdir(CSRC):
        if fn.endswith((".hpp", ".hip")) and fn not in ("clik_rollout_summary.hpp", "clik_api.hip"):
            text = jit._code_only(open(os.path.join(CSRC, fn)).read())
            assert "clik_rollout_summary" not in text and "rollsum" not in text and "RollSum" not in text, fn
    api = jit._code_only(open(os.path.join(CSRC, "clik_api.hip")).read())
    assert "_sum_kernel" not in api and "clik_rollout_summary.hpp" not in api        # entry points, no kernel
    for tmpl in _OLD_TEMPLATES:
        text = getattr(jit, tmpl)
        assert "clik_rollout_summary.hpp" not in text and "rollout_sum" not in text, tmpl
    # the header includes nothing: its units name the headers it reuses, read-only
    text = open(os.path.join(CSRC, "clik_rollout_summary.hpp")).read()
    assert re.findall(r'#include [<"]([^>"]+)[>"]', jit._code_only(text)) == []
    assert "atomic" not in jit._code_only(text)
    assert re.findall(r'#include "([^"]+)"', jit._ROLLSUM_TEMPLATE) == ["clik_pinv_rec.hpp", "clik_summary.hpp",
                                                                        "clik_rollout_summary.hpp"]
    assert re.findall(r'#include "([^"]+)"', jit._QP_ROLLSUM_TEMPLATE) == ["clik_qp_rec.hpp", "clik_summary.hpp",
                                                                           "clik_rollout_summary.hpp"]
    assert 'extern "C" hipError_t clik_jit_rollout_sum(' in jit._ROLLSUM_TEMPLATE
    assert 'extern "C" hipError_t clik_jit_qp_rollout_sum(' in jit._QP_ROLLSUM_TEMPLATE


def test_existing_templates_keep_their_tags(tmp_path, monkeypatch):
    """clik_rollout_summary.hpp is hashed into the tags of the two units that include it (through ``_unit_stamp``) and into
    no other: a copy of csrc/ with the header edited"""
    from casclik_amd.build import CSRC
    digest = lambda fn: hashlib.sha256(jit._code_only(open(os.path.join(CSRC, fn)).read()).encode()).hexdigest()[:12]   # noqa: E731
    for tmpl in (jit._ROLLSUM_TEMPLATE, jit._QP_ROLLSUM_TEMPLATE):
        assert jit._unit_stamp(tmpl) == digest("clik_summary.hpp") + digest("clik_rollout_summary.hpp")
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, str(copy), ignore=shutil.ignore_patterns("_obj"))
    stamp = jit._source_stamp()
    old = {t: jit._cache_tag("{1}", "code", False, [], getattr(jit, t)) for t in _OLD_TEMPLATES}
    old[""] = jit._cache_tag("{1}", "code", False, [], "")
    mine = {t: jit._cache_tag("{1}", "code", False, [], t) for t in (jit._ROLLSUM_TEMPLATE, jit._QP_ROLLSUM_TEMPLATE)}
    monkeypatch.setattr(jit, "CSRC", str(copy))
    text = open(os.path.join(CSRC, "clik_rollout_summary.hpp")).read()
    (copy / "clik_rollout_summary.hpp").write_text(text + "\n// a remark\n/* and another */\n")
    for t, tag in mine.items():
        assert jit._cache_tag("{1}", "code", False, [], t) == tag
    (copy / "clik_rollout_summary.hpp").write_text(text + "\nnamespace clik { constexpr int kRollSumEdited = 1; }\n")
    assert jit._source_stamp() == stamp
    for t, tag in mine.items():
        assert jit._cache_tag("{1}", "code", False, [], t) != tag
    for t, tag in old.items():
        assert jit._cache_tag("{1}", "code", False, [], getattr(jit, t) if t else "") == tag, t


def test_a_recorded_request_replays_under_the_name_the_attach_asks_for(tmp_path, monkeypatch):
    """CLIK_JIT_RECORD writes the request of a summarising-rollout unit; prebuild_recorded compiles it under the cache name
    the controller will ask for; the committed records hold the units of the GPU tests' skills"""
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    init, extern, tmpl = _unit("qp")
    monkeypatch.setenv("CLIK_JIT_RECORD", str(tmp_path / "records"))
    monkeypatch.setattr(jit, "CACHE", str(tmp_path / "cache"))
    monkeypatch.setenv("CLIK_JIT_NO_COMPILER", "1")
    so, tag = jit.build_shape_library(init, template=tmpl, extern=extern)
    assert so is None                                       # (nothing cached, no compiler: recorded and nothing else)
    name = "req_%s" % jit._request_id(init, extern, False, [], tmpl)
    assert sorted(os.listdir(tmp_path / "records")) == [name + ".hip", name + ".json"]
    monkeypatch.delenv("CLIK_JIT_NO_COMPILER")
    monkeypatch.delenv("CLIK_JIT_RECORD")
    assert jit.prebuild_recorded(str(tmp_path / "records")) == (1, 0, 0), getattr(jit.prebuild_recorded, "failures", None)
    assert os.path.exists(tmp_path / "cache" / ("clik_shape_%s.so" % tag))
    monkeypatch.setenv("CLIK_JIT_NO_COMPILER", "1")
    assert jit.build_shape_library(init, template=tmpl, extern=extern) == (
        str(tmp_path / "cache" / ("clik_shape_%s.so" % tag)), tag)
    # the committed records of the units the GPU tests instantiate
    for fixture in ("stack", "mixed", "qp"):
        init, extern, tmpl = _unit(fixture)
        assert os.path.exists(os.path.join(jit.RECORDS, "req_%s.json" % jit._request_id(init, extern, False, [], tmpl))), fixture


def test_what_the_host_refuses():
    """``rollout_batch(..., summary=, summary_tol=)`` as checked before anything reaches a device"""
    assert rollout_summary_request(False, None, 0, 20) == (False, None)
    assert rollout_summary_request(True, None, 1, 20) == (True, None)
    ok, tol = rollout_summary_request(True, 1e-3, 9, 20)
    assert ok and tol.dtype == np.float64 and tol.shape == (20,) and (tol == 1e-3).all()
    ok, tol = rollout_summary_request(True, np.arange(20.0), 9, 20)
    assert ok and np.array_equal(tol, np.arange(20.0))
    with pytest.raises(ValueError, match="summary=True"):
        rollout_summary_request(False, 1e-3, 9, 20)                 # a tolerance without a summary
    for bad in (-1e-3, float("nan"), float("inf"), np.full(19, 1e-3), np.where(np.arange(20) == 3, -1.0, 1e-3)):
        with pytest.raises(ValueError, match="tol"):
            rollout_summary_request(True, bad, 9, 20)
    with pytest.raises(ValueError, match="at least one tick"):
        rollout_summary_request(True, None, 0, 20)                  # a summary of no record
    with pytest.raises(ValueError, match="at least one tick"):
        rollout_summary_request(True, 1e-3, 0, 20)
