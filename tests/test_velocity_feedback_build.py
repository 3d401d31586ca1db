"""CPU: the variants of the lane-per-instance rollouts with the velocity feedback compiled in (clik_rollout_lane.hpp under
-DCLIK_VELOCITY_FEEDBACK={...}) - cross-compiled for gfx950 without scratch, with the registers' occupancy, LDS and waves
per block of the plain units; the map as the loaded units report it; the plain units' requests unchanged, so that every
committed record still names them; the committed records of the variants the GPU tests ask for; and what the option's
validation refuses, which needs no device."""
import ctypes as C
import os

import numpy as np
import pytest

from casclik_amd import jit, skills
from casclik_amd.controllers.base_controller import velocity_feedback_request

import converge_cases as K
import velocity_feedback_cases as V

WHATS = ("rec", "rollsum", "converge")
# (skill, unit, group) of every variant tests/test_gpu_velocity_feedback.py launches
GPU_UNITS = [("qp", "rec", 1), ("qp", "rollsum", 1), ("pinv", "rec", 1), ("pinv", "rollsum", 1), ("pinv", "converge", 1),
             ("pinv", "converge", 4), ("path", "rec", 1), ("timed", "rec", 1)]

_REQ = {}


def _request(name):
    if name not in _REQ:
        spec, ctrl, qp, fb = V.make(name, skills.iiwa(), skills.ur5())
        req = jit.unit_request(ctrl)
        assert req.eligible
        _REQ[name] = (req, fb)
    return _REQ[name]


def _template(what, kind, fed):
    if fed and (what, kind) in jit.FEEDBACK_UNITS:
        return jit.FEEDBACK_UNITS[what, kind]["template"]
    return (jit.UNITS.get((what, kind)) or jit.CONVERGE_UNITS[what, kind])["template"]


def _info(so, symbol):
    fn = getattr(jit._load(so), symbol)
    fn.restype, fn.argtypes = C.c_longlong, [C.c_int]
    return fn


def test_the_defines_of_a_map():
    assert jit.velocity_feedback_defines(None) == () and jit.velocity_feedback_defines((-1, -1)) == ()
    assert jit.velocity_feedback_defines(V.FB_IIWA) == ("-DCLIK_VELOCITY_FEEDBACK={7,8,9,10,11,12,13}",)
    assert jit.velocity_feedback_defines(V.FB_PATH) == ("-DCLIK_VELOCITY_FEEDBACK={-1,-1,-1,-1,-1,-1,0}",)
    assert jit._feedback_of(jit.converge_group_defines(4) + jit.velocity_feedback_defines(V.FB_PATH)) == V.FB_PATH
    assert jit._feedback_of(jit.converge_group_defines(4)) is None
    # the variants have rows of their own only where the plain unit has no info query to ask: the recording rollouts
    assert sorted(jit.FEEDBACK_UNITS) == [("rec", "pinv"), ("rec", "qp")]
    for key, unit in jit.FEEDBACK_UNITS.items():
        plain = jit.UNITS[key]
        assert unit["template"] == plain["template"] + jit._REC_INFO_ENTRY and unit["values"] is None
        assert unit["symbols"] == plain["symbols"] and unit["attach"] == plain["attach"] and unit["refuse"] is plain["refuse"]


@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("name", ["qp", "pinv", "path"])
def test_variant_compiles_for_gfx950_without_scratch_and_as_many_waves(name, what):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req, fb = _request(name)
    res = {}
    for fed in (False, True):
        text = jit.unit_text(_template(what, req.kind, fed), req.init, req.extern)
        res[fed] = jit.unit_resources(text, req.init, extra=jit.velocity_feedback_defines(fb) if fed else ())
    assert sorted(res[True]) == sorted(res[False]) and len(res[True]) >= 1       # (the same kernels, no further one)
    for k, r in res[True].items():
        p = res[False][k]
        print(name, what, k[-50:], "plain", p, "fed", r)
        assert r["ScratchSize"] == 0 and p["ScratchSize"] == 0, (k, r)
        assert r["Occupancy"] == p["Occupancy"], (k, r, p)
        assert r.get("LDS Size", 0) == p.get("LDS Size", 0), (k, r, p)


@pytest.mark.parametrize("name,what,group", GPU_UNITS)
def test_the_loaded_unit_reports_the_map_and_the_plain_unit_s_figures(name, what, group):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req, fb = _request(name)
    base = {"rec": 5, "rollsum": 9, "converge": 7}[what]
    symbol = {"rec": "clik_jit_rec_info", "rollsum": "clik_jit_rollsum_info", "converge": "clik_jit_converge_info"}[what]
    figures = {"rec": (2, 3, 4), "rollsum": (2, 3, 4, 7, 8), "converge": (2, 3, 4, 6)}[what]
    defines = jit.converge_group_defines(group) + jit.velocity_feedback_defines(fb)
    so, _ = jit.build_shape_library(req.init, template=_template(what, req.kind, True), defines=defines, extern=req.extern)
    info = _info(so, symbol)
    assert jit.unit_feedback(info, base) == fb
    assert info(base + 1 + len(fb)) == -1
    if what == "converge":
        assert info(6) == group
    # the plain unit: no map, and the same LDS bytes, fit and waves per block
    if what == "rec":
        # (the committed recording units have no info query: the variant's text without the flag)
        plain_so, _ = jit.build_shape_library(req.init, template=_template(what, req.kind, True), extern=req.extern)
    else:
        plain_so, _ = jit.build_shape_library(req.init, template=_template(what, req.kind, False),
                                              defines=jit.converge_group_defines(group), extern=req.extern)
    plain = _info(plain_so, symbol)
    assert jit.unit_feedback(plain, base) is None and plain(base + 1) == -1
    for k in figures:
        assert info(k) == plain(k), (k, info(k), plain(k))
    assert info(4 if what == "rec" else 3) == 1
    print(name, what, group, [info(k) for k in figures])


def test_units_without_the_flag_are_the_committed_records():
    """no map, no define, the request of before: the plain units of the existing fixtures hash to their committed
    records, whose text no template edit has touched"""
    iiwa, ur5 = skills.iiwa(), skills.ur5()
    for name in ("pose", "stack", "qp"):
        req = jit.unit_request(K.make(name, iiwa, ur5)[1])
        for what in WHATS:
            tmpl = _template(what, req.kind, False)
            flags = list(jit.velocity_feedback_defines(None))
            rid = jit._request_id(req.init, req.extern, False, flags, tmpl)
            folder = jit.CONVERGE_RECORDS if what == "converge" else jit.RECORDS
            path = os.path.join(folder, "req_%s.json" % rid)
            assert os.path.exists(path), (name, what)
            if os.path.exists(path[:-5] + ".hip"):
                with open(path[:-5] + ".hip") as f:
                    assert f.read() == jit.unit_text(tmpl, req.init, req.extern), (name, what)


def test_the_committed_records_hold_the_variants_of_the_gpu_tests():
    tags = set(jit.recorded_tags())
    for name, what, group in GPU_UNITS:
        req, fb = _request(name)
        tmpl = _template(what, req.kind, True)
        flags = list(jit.converge_group_defines(group) + jit.velocity_feedback_defines(fb))
        rid = jit._request_id(req.init, req.extern, False, flags, tmpl)
        folder = {"converge": jit.CONVERGE_RECORDS, "rec": jit.FEEDBACK_RECORDS}.get(what, jit.RECORDS)
        assert os.path.exists(os.path.join(folder, "req_%s.json" % rid)), (name, what, group)
        sched = jit.sched_strategy(tmpl, req.init)
        assert jit._cache_tag(req.init, req.extern, False, flags + jit._sched_key(sched), tmpl) in tags, (name, what, group)


def test_a_map_that_does_not_fit_the_skill_does_not_compile():
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req, fb = _request("pinv")
    text = jit.unit_text(_template("rec", req.kind, True), req.init, req.extern)
    with pytest.raises(RuntimeError, match="one entry per robot and virtual variable"):
        jit.unit_resources(text, req.init, extra=("-DCLIK_VELOCITY_FEEDBACK={7,8}",))
    with pytest.raises(RuntimeError, match="an entry outside input_var"):
        jit.unit_resources(text, req.init, extra=("-DCLIK_VELOCITY_FEEDBACK={7,8,9,10,11,12,14}",))


def test_what_the_option_s_validation_refuses():
    """on the lowered skill alone: no handle on a device is needed"""
    for name in ("qp", "pinv", "path"):
        req, fb = _request(name)
        d = req.descriptor
        assert velocity_feedback_request(fb, d.n_q, d.n_x, d.n_y) == fb
        assert velocity_feedback_request(list(fb), d.n_q, d.n_x, d.n_y) == fb
        assert velocity_feedback_request(np.asarray(fb, dtype=np.int32), d.n_q, d.n_x, d.n_y) == fb
        assert velocity_feedback_request(None, d.n_q, d.n_x, d.n_y) is None
        assert velocity_feedback_request((-1,) * (d.n_q + d.n_x), d.n_q, d.n_x, d.n_y) is None
    assert velocity_feedback_request((13, -1, 0, -1, -1, -1, 7), 7, 0, 14) == (13, -1, 0, -1, -1, -1, 7)
    for bad, match in (((7, 8, 9), "must have 7 entries"), (tuple(range(7, 15)), "must have 7 entries"),
                       (tuple(range(8, 15)), r"in \[-1, 14\)"), ((-2, 7, 8, 9, 10, 11, 12), r"in \[-1, 14\)"),
                       ((7, 7, 8, 9, 10, 11, 12), "input_var\\[7\\] twice"), ((7.0, 8, 9, 10, 11, 12, 13), "must be an int"),
                       ((True, 8, 9, 10, 11, 12, 13), "must be an int"), (("7", 8, 9, 10, 11, 12, 13), "must be an int"),
                       (5, "sequence of ints")):
        with pytest.raises(ValueError, match=match):
            velocity_feedback_request(bad, 7, 0, 14)
    with pytest.raises(ValueError, match="needs a skill with input_var"):
        velocity_feedback_request((-1,) * 6 + (0,), 6, 1, 0)
    with pytest.raises(ValueError, match="must have 7 entries \\(6 robot and 1 virtual"):
        velocity_feedback_request((0,) * 6, 6, 1, 1)
