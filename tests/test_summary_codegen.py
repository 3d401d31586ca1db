"""CPU: the constraint-summary kernels (clik_summary.hpp, jit._SUMMARY_TEMPLATE) - their translation unit cross-compiled
for gfx950 without scratch, in a unit no other kernel shares; the tags of every other template untouched by the new
header; a recorded request replayed by ``prebuild_recorded``; and the rules by which the chunks' partials combine, as a
numpy restatement held against the plain reduction on hand-made values."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import _capi, jit, skills
from casclik_amd.controllers.base_controller import summary_tolerances
from casclik_amd.lowering import lower_skill

from extern_skills import double_pendulum_skill


def _fixture(name):
    """(spec, controller that is not set up, "pinv" | "qp")"""
    if name == "stack":
        spec = skills.stack_skill(skills.iiwa())
        return spec, cc.PseudoInverseController(skill_spec=spec, options=dict(skills.STACK_OPTIONS)), "pinv"
    spec = double_pendulum_skill(track=True)
    return spec, cc.ReactiveQPController(skill_spec=spec, robot_var_weights=[1.0, 1.0]), "qp"


@pytest.mark.parametrize("name", ["stack", "pendulum"])
def test_summary_unit_compiles_for_gfx950_without_scratch(name):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req = jit.unit_request(_fixture(name)[1])
    assert req.eligible
    if name == "pendulum":
        assert req.descriptor.extern_code            # (its constraints run as generated code)
    res = jit.unit_resources(jit.unit_text(jit._SUMMARY_TEMPLATE, req.init, req.extern), req.init)
    assert len(res) == 2, sorted(res)        # (the two phases: none of the tick / rollout / constraint-value kernels)
    assert sorted("combine" in k for k in res) == [False, True]
    for kernel, r in res.items():
        assert "constraint_summary" in kernel
        assert r["ScratchSize"] == 0, r
        print(name, kernel[-40:], r)


def test_the_summary_kernels_stay_out_of_the_other_translation_units():
    from casclik_amd.build import CSRC
    for fn in os.listdir(CSRC):
        if fn.endswith((".hpp", ".hip")) and fn not in ("clik_summary.hpp", "clik_api.hip"):
            text = jit._code_only(open(os.path.join(CSRC, fn)).read())
            assert "clik_summary" not in text and "constraint_summary" not in text and "SummaryArgs" not in text, fn
    for tmpl in (jit._TEMPLATE, jit._VALUE_TEMPLATE, jit._QP_TEMPLATE, jit._QP_VALUE_TEMPLATE, jit._REC_TEMPLATE,
                 jit._VALUE_REC_TEMPLATE, jit._QP_REC_TEMPLATE, jit._QP_VALUE_REC_TEMPLATE, jit._TIME_TEMPLATE,
                 jit._MONITOR_TEMPLATE, jit._FUNCTION_TEMPLATE):
        assert "clik_summary.hpp" not in tmpl and "constraint_summary" not in tmpl
    assert re.findall(r'#include "([^"]+)"', jit._SUMMARY_TEMPLATE) == ["clik_summary.hpp"]
    api = jit._code_only(open(os.path.join(CSRC, "clik_api.hip")).read())
    assert "constraint_summary_kernel" not in api and "clik_summary.hpp" not in api      # entry points, no kernel
    text = open(os.path.join(CSRC, "clik_summary.hpp")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["clik_pinv_kernels.hpp"]
    assert "atomic" not in jit._code_only(text)


def test_existing_templates_keep_their_tags():
    """clik_summary.hpp is hashed into the tags of the unit that includes it and into no other"""
    from casclik_amd.build import CSRC
    stamp = jit._source_stamp()
    monitor = hashlib.sha256(jit._code_only(open(os.path.join(CSRC, "clik_monitor.hpp")).read()).encode()).hexdigest()[:12]
    function = hashlib.sha256(jit._code_only(open(os.path.join(CSRC, "clik_function.hpp")).read()).encode()).hexdigest()[:12]
    for tmpl, unit in (("", ""), (jit._QP_TEMPLATE, ""), (jit._REC_TEMPLATE, ""), (jit._QP_REC_TEMPLATE, ""),
                       (jit._TIME_TEMPLATE, ""), (jit._MONITOR_TEMPLATE, monitor), (jit._FUNCTION_TEMPLATE, function)):
        assert jit._unit_stamp(tmpl) == unit
        want = hashlib.sha256(("{1}" + "ext" + stamp + unit + "-DX" + tmpl).encode()).hexdigest()[:16]
        assert jit._cache_tag("{1}", "ext", False, ["-DX"], tmpl) == want
    own = hashlib.sha256(jit._code_only(open(os.path.join(CSRC, "clik_summary.hpp")).read()).encode()).hexdigest()[:12]
    assert jit._unit_stamp(jit._SUMMARY_TEMPLATE) == own
    want = hashlib.sha256(("{1}" + stamp + own + jit._SUMMARY_TEMPLATE).encode()).hexdigest()[:16]
    assert jit._cache_tag("{1}", "", False, [], jit._SUMMARY_TEMPLATE) == want


def test_a_recorded_summary_request_replays(tmp_path, monkeypatch):
    """CLIK_JIT_RECORD writes the request of a summary unit; prebuild_recorded compiles it under the cache name the
    controller will ask for; the committed records hold the units of the GPU tests' five skills"""
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req = jit.unit_request(_fixture("stack")[1])
    assert req.eligible
    init = req.init
    monkeypatch.setenv("CLIK_JIT_RECORD", str(tmp_path / "records"))
    monkeypatch.setattr(jit, "CACHE", str(tmp_path / "cache"))
    monkeypatch.setenv("CLIK_JIT_NO_COMPILER", "1")
    so, tag = jit.build_shape_library(init, template=jit._SUMMARY_TEMPLATE)
    assert so is None                                       # (nothing cached, no compiler: recorded and nothing else)
    name = "req_%s" % jit._request_id(init, "", False, [], jit._SUMMARY_TEMPLATE)
    assert sorted(os.listdir(tmp_path / "records")) == [name + ".hip", name + ".json"]
    monkeypatch.delenv("CLIK_JIT_NO_COMPILER")
    monkeypatch.delenv("CLIK_JIT_RECORD")
    assert jit.prebuild_recorded(str(tmp_path / "records")) == (1, 0, 0), getattr(jit.prebuild_recorded, "failures", None)
    assert os.path.exists(tmp_path / "cache" / ("clik_shape_%s.so" % tag))
    monkeypatch.setenv("CLIK_JIT_NO_COMPILER", "1")
    assert jit.build_shape_library(init, template=jit._SUMMARY_TEMPLATE) == (str(tmp_path / "cache" / ("clik_shape_%s.so" % tag)), tag)
    # the committed record of this very request, and four more summary units
    assert os.path.exists(os.path.join(jit.RECORDS, name + ".json"))
    n = 0
    for fn in os.listdir(jit.RECORDS):
        if fn.endswith(".json"):
            with open(os.path.join(jit.RECORDS, fn)) as f:
                n += json.load(f).get("template") == jit._SUMMARY_TEMPLATE
    assert n >= 5, n


# ---- chunking and the combine rules ------------------------------------------------------------------------------------------
def test_chunk_length_is_a_function_of_the_shape_alone():
    lib = _capi.load_library()
    for R, B, want in ((1, 1, 8), (19, 257, 8), (8192, 1, 8), (8193, 1, 9), (256, 16384, 16), (10000, 16384, 625),
                       (100, 1 << 20, 100), (4096, 257, 8), (4097, 257, 9)):
        assert jit.summary_chunk_length(R, B) == want == lib.clik_summary_chunk_length(R, B), (R, B)
    text = open(os.path.join(jit.CSRC, "clik_summary.hpp")).read()
    assert (jit.SUMMARY_TARGET_BLOCKS, jit.SUMMARY_MIN_CHUNK, jit.SUMMARY_GROUP) == tuple(
        int(re.search(r"constexpr long long %s = (\d+);" % k, text).group(1))
        for k in ("kSummaryTargetBlocks", "kSummaryMinChunk", "kSummaryGroup"))


def _partials(e, lo, hi, is_set, tol, c):
    """phase one, restated: per chunk of c records what a lane leaves in the work tensor"""
    out = []
    for r0 in range(0, len(e), c):
        ch = e[r0:r0 + c]
        a = np.abs(ch)
        v = np.maximum(np.maximum(lo - ch, ch - hi), 0.0) if is_set else np.zeros_like(ch)
        d = v if is_set else a
        uns = np.nonzero(d > tol)[0]
        out.append({"amax": a.max(), "at": r0 + int(a.argmax()), "ssq": float((ch * ch).sum()), "vmax": v.max(),
                    "vcount": int((v > 0).sum()), "uns": r0 + int(uns[-1]) if uns.size else -1})
    return out


def _combine(parts, R):
    """phase two, restated (clik_summary.hpp: constraint_summary_combine_kernel): in chunk order"""
    amax, at, ssq, vmax, vcount, uns = -1.0, 0, 0.0, 0.0, 0, -1
    for p in parts:
        if p["amax"] > amax:            # (strictly: the lowest record among equal maxima)
            amax, at = p["amax"], p["at"]
        ssq += p["ssq"]
        vmax = max(vmax, p["vmax"])
        vcount += p["vcount"]
        uns = max(uns, p["uns"])        # (records ascend with the chunks: the last chunk that holds one)
    return {"abs_max": amax, "abs_max_at": at, "rms": np.sqrt(ssq / R), "viol_max": vmax, "viol_count": vcount,
            "settled_at": uns + 1}


def test_combine_rules_on_hand_made_partials():
    c = 4
    # equal maxima in chunks 0 and 2 (and twice inside chunk 2): the first record wins
    e = np.array([0.5, -2.0, 1.0, 0.25, 0.5, 1.5, -0.5, 0.0, 2.0, -2.0, 0.1, 0.05, 0.02])
    got = _combine(_partials(e, 0.0, 0.0, False, 0.3, c), len(e))
    assert got["abs_max"] == 2.0 and got["abs_max_at"] == 1
    assert got["settled_at"] == 10                  # (|e| <= 0.3 from record 10 on: the last chunk with an unsettled one is 2)
    assert abs(got["rms"] - np.sqrt((e * e).mean())) < 1e-15
    assert got["viol_max"] == 0.0 and got["viol_count"] == 0
    # the answer lies in a MIDDLE chunk: nothing unsettled in the last one
    e = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.9, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1])
    got = _combine(_partials(e, 0.0, 0.0, False, 0.5, c), len(e))
    assert got["settled_at"] == 6 and got["abs_max_at"] == 0
    # never unsettled / unsettled at the last record
    assert _combine(_partials(e, 0.0, 0.0, False, 5.0, c), len(e))["settled_at"] == 0
    assert _combine(_partials(e, 0.0, 0.0, False, 0.05, c), len(e))["settled_at"] == len(e)
    # a set row: d is the violation, one side unbounded
    e = np.array([0.5, -0.2, 0.1, -0.4, 0.3, 0.2, -0.05, 0.6, 0.7])
    got = _combine(_partials(e, 0.0, np.inf, True, 0.1, c), len(e))
    assert got["viol_count"] == 3 and got["viol_max"] == 0.4 and got["settled_at"] == 4
    assert got["abs_max"] == 0.7 and got["abs_max_at"] == 8
    # any chunk length gives the plain reduction
    rng = np.random.default_rng(0)
    e = rng.normal(size=37)
    for c in (1, 5, 8, 36, 37, 50):
        got = _combine(_partials(e, -0.5, 1.0, True, 0.2, c), len(e))
        v = np.maximum(np.maximum(-0.5 - e, e - 1.0), 0.0)
        uns = np.nonzero(v > 0.2)[0]
        assert (got["abs_max"], got["abs_max_at"]) == (np.abs(e).max(), np.abs(e).argmax())
        assert (got["viol_max"], got["viol_count"], got["settled_at"]) == (v.max(), (v > 0).sum(), uns[-1] + 1)


def test_tolerances_are_checked_on_the_host():
    assert summary_tolerances(None, 5) is None
    assert np.array_equal(summary_tolerances(0.5, 3), [0.5, 0.5, 0.5])
    assert np.array_equal(summary_tolerances([0.0, 1.0], 2), [0.0, 1.0])
    for bad in ([1.0, 2.0], -1.0, float("nan"), float("inf"), [0.1, -0.1, 0.1]):
        with pytest.raises(ValueError, match="tol"):
            summary_tolerances(bad, 3)


def test_methods_need_set_up_and_the_c_abi_checks_come_first(monkeypatch):
    spec, ctrl, _ = _fixture("stack")
    with pytest.raises(RuntimeError, match="setup"):
        ctrl.constraint_summary_batch(0.0, np.zeros((2, 7)), input_var=np.zeros((2, 7)))
    lib = _capi.load_library()
    monkeypatch.setenv("CLIK_HOST_ONLY", "1")
    d = lower_skill(spec)
    desc, opts = _capi.desc_to_c(d), _capi.pinv_opts_to_c(ctrl.options)
    h = C.c_void_p()
    assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h)) == 0
    q = C.c_void_p(64)          # (never dereferenced: every call below returns before a launch)
    try:
        assert lib.clik_pinv_attach_summary_kernel(None, None, None) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_attach_summary_kernel(h, None, None) == 0                    # (detaching takes any handle)
        assert lib.clik_pinv_attach_summary_kernel(h, q, q) == _capi.CLIK_EINVAL          # (attaching needs the device)
        assert lib.clik_pinv_summary_work_bytes(h, 10, 10) == 0
        args = lambda n_rec, B, qq, o, tol, st: (n_rec, B, None, 0, 0, qq, None, q, 0, tol, q, 1 << 20,      # noqa: E731
                                                 o, o, o, o, o, o, st, None)
        assert lib.clik_pinv_constraint_summary(None, *args(1, 1, q, q, None, None)) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_constraint_summary(h, *args(-1, 1, q, q, None, None)) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_constraint_summary(h, *args(0, 5, None, None, None, None)) == _capi.CLIK_OK
        assert lib.clik_pinv_constraint_summary(h, *args(1, 1, None, q, None, None)) == _capi.CLIK_EINVAL
        assert b"q must be" in lib.clik_last_error()
        assert lib.clik_pinv_constraint_summary(h, *args(1, 1, q, None, None, None)) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_constraint_summary(h, *args(1, 1, q, q, q, None)) == _capi.CLIK_EINVAL
        assert b"go together" in lib.clik_last_error()
        assert lib.clik_pinv_constraint_summary(h, *args(1, 1, q, q, None, None)) == _capi.CLIK_EUNSUPPORTED
        assert b"instantiated" in lib.clik_last_error()
    finally:
        assert lib.clik_pinv_destroy(h) == 0
