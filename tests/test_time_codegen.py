"""CPU: the time slots of a skill as generated code (codegen.emit_time_slots) - its shape, its values as host C++ against
SkillDescriptor.time_terms, its kernel compiled for gfx950 without scratch, in a translation unit no other kernel shares -
and the marshalling of `time_on_device` that needs no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import codegen, jit, skills
from casclik_amd import sym as cs
from casclik_amd.lowering import lower_skill

import time_skills

SKILLS = ["tracking", "moe", "mixed", "ops"]
# the largest slot tree (value or derivative) of these skills has this many distinct nodes at most: one rounding
# each, which is what the 1e-14 of the host comparison rests on
MAX_NODES = 48


@pytest.fixture(scope="module")
def descs():
    fk = skills.ur5()
    import notebook_figures
    return {"tracking": lower_skill(time_skills.tracking_spec(fk)),
            "moe": lower_skill(time_skills.moe_spec(notebook_figures.moe_fk())),
            "mixed": lower_skill(time_skills.mixed_spec()), "ops": lower_skill(time_skills.ops_time_spec())}


@pytest.mark.parametrize("name", SKILLS)
def test_source_stores_every_slot_once(descs, name):
    d = descs[name]
    assert d.n_tslots > 0
    text = codegen.emit_time_slots(d)
    assert "struct TimeSlots" in text and "eval(double t, double* tv)" in text
    assert "n_tslots = %d;" % d.n_tslots in text
    stores = re.findall(r"\btv\[(\d+)\] = ", text)
    assert len(stores) == 2 * d.n_tslots and len(text.split("tv[")) - 1 == 2 * d.n_tslots     # (and no read of tv)
    assert sorted(int(k) for k in stores) == list(range(2 * d.n_tslots))
    # the only leaf beside constants is the time: no state, input or kinematics reference
    assert not re.search(r"\b(z|ys|K)\b", jit._code_only(text).split("{", 2)[2])


def test_emitter_accepts_the_lowerer_and_shares_subexpressions(descs):
    from casclik_amd.lowering import _Lowerer
    low = _Lowerer(time_skills.tracking_spec(skills.ur5()))
    low.run()
    text = codegen.emit_time_slots(low)
    assert text == codegen.emit_time_slots(low.desc)
    assert text.count("sincos_joint(") == 1          # one sin / cos pair of 0.1 t serves three values and derivatives


def test_a_skill_without_time_dependence_gives_an_empty_body():
    d = lower_skill(skills.stack_skill(skills.iiwa()))
    assert d.n_tslots == 0
    text = codegen.emit_time_slots(d)
    assert "tv[" not in text and "const double" not in text and "n_tslots = 0;" in text


def test_an_operation_without_device_code_is_refused(descs):
    d = descs["mixed"]
    val, der = d.tslots[0]
    bad = cs.Scalar("erf", (val,))
    try:
        d.tslots.append((bad, der))
        with pytest.raises(NotImplementedError, match="no device code for operation 'erf'"):
            codegen.emit_time_slots(d)
    finally:
        d.tslots.pop()


_HOST_WRAPPER = """#include <cmath>
#define __device__
#define __forceinline__ inline
static inline void sincos_joint(double x, double& s, double& c) { sincos(x, &s, &c); }
%s
extern "C" void time_terms(double t, double* tv) { TimeSlots::eval(t, tv); }
"""


def _host_time_terms(d, tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    src = tmp_path / "ts.cpp"
    src.write_text(_HOST_WRAPPER % codegen.emit_time_slots(d))
    so = tmp_path / "ts.so"
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(so)])
    fn = C.CDLL(str(so)).time_terms
    fn.argtypes = [C.c_double, C.POINTER(C.c_double)]
    fn.restype = None
    return fn


@pytest.mark.parametrize("name", SKILLS)
def test_emitted_text_as_host_code_matches_the_host_evaluator(descs, name, tmp_path):
    """Both sides run host libm in the same operation order; what differs is x * x for pow(x, 2), repeated
    multiplication for pow(x, 3), sincos for separate sin / cos and nothing else: |a - b| <= 1e-14 (1 + |b|), some 90
    units in the last place for trees of at most MAX_NODES nodes at one rounding each."""
    d = descs[name]
    assert max(max(time_skills.count_nodes(v), time_skills.count_nodes(g)) for v, g in d.tslots) <= MAX_NODES
    fn = _host_time_terms(d, tmp_path)
    worst = 0.0
    # (the tracking skill also beyond the straight-line range of sincos_joint, where the device takes the library path)
    for t in np.concatenate([time_skills.TIMES, time_skills.TIMES_BEYOND_THE_FAST_RANGE]) if name == "tracking" else time_skills.TIMES:
        ref = d.time_terms(float(t))
        assert np.isfinite(ref).all(), (name, t)
        got = np.full(2 * d.n_tslots, np.nan)
        fn(float(t), got.ctypes.data_as(C.POINTER(C.c_double)))
        err = np.abs(got - ref) / (1.0 + np.abs(ref))
        worst = max(worst, err.max())
        assert (err <= 1e-14).all(), (name, t, got, ref)
    print("%s: worst host-code deviation %.3g" % (name, worst))


@pytest.mark.parametrize("name", SKILLS)
def test_time_kernel_compiles_for_gfx950_alone_and_without_scratch(descs, name):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    res = jit.unit_resources(jit.unit_text(jit._TIME_TEMPLATE, "", codegen.emit_time_slots(descs[name])), "")
    assert len(res) == 1, sorted(res)
    (kernel, r), = res.items()
    assert "time_terms_kernel" in kernel
    assert r["ScratchSize"] == 0, r
    print(name, r)


def test_the_time_kernel_stays_out_of_the_other_translation_units():
    from casclik_amd.build import CSRC
    for fn in os.listdir(CSRC):
        if fn.endswith((".hpp", ".hip")) and fn not in ("clik_time.hpp", "clik_api.hip"):
            text = jit._code_only(open(os.path.join(CSRC, fn)).read())
            assert "clik_time.hpp" not in text and "time_terms_kernel" not in text, fn
    for tmpl in (jit._TEMPLATE, jit._VALUE_TEMPLATE, jit._QP_TEMPLATE, jit._QP_VALUE_TEMPLATE, jit._REC_TEMPLATE,
                 jit._VALUE_REC_TEMPLATE, jit._QP_REC_TEMPLATE, jit._QP_VALUE_REC_TEMPLATE):
        assert "clik_time.hpp" not in tmpl and "time_terms" not in tmpl
    includes = re.findall(r'#include "([^"]+)"', jit._TIME_TEMPLATE)
    assert includes == ["clik_device.hpp", "clik_time.hpp"]
    assert 'extern "C" hipError_t clik_jit_time_terms(' in jit._TIME_TEMPLATE
    # clik_api.hip holds the entry points, no kernel
    assert "time_terms_kernel" not in jit._code_only(open(os.path.join(CSRC, "clik_api.hip")).read())


# ---- marshalling that needs no GPU -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pinv", "qp"])
def test_option_defaults_to_false_and_the_method_needs_it(kind):
    spec = time_skills.tracking_spec(skills.ur5())
    ctrl = cc.PseudoInverseController(skill_spec=spec) if kind == "pinv" else cc.ReactiveQPController(skill_spec=spec)
    # (the dictionary a caller reads back keeps the reference's keys: the option is read with this default)
    assert ctrl.options.get("time_on_device", False) is False
    with pytest.raises(NotImplementedError, match="time_on_device"):
        ctrl.time_terms_batch(np.zeros(3))
    with pytest.raises(ValueError, match="method"):
        ctrl.time_terms_batch(np.zeros(3), method="heun")
    on = type(ctrl)(skill_spec=spec, options={"time_on_device": True})
    assert on.options["time_on_device"] is True
    with pytest.raises(ValueError, match="method"):
        on.time_terms_batch(np.zeros(3), method="heun")
    with pytest.raises(RuntimeError, match="setup"):         # (option set, no handle yet)
        on.time_terms_batch(np.zeros(3))


def test_host_stage_times_are_single_rounded_adds():
    """the identity the time kernel keeps: t, t + 0.5 dt, t + 0.5 dt, t + dt, each one rounded add (0.5 dt is exact)"""
    from casclik_amd.controllers.base_controller import rollout_stage_times
    rng = np.random.default_rng(4)
    times = np.concatenate([time_skills.TIMES, rng.uniform(0.0, 30.0, 50)])
    for dt in (0.05, 0.008, 1e-3, 1.0 / 3.0):
        st = rollout_stage_times(times, dt, "rk4").reshape(-1, 4)
        half = 0.5 * dt
        assert half * 2.0 == dt
        for i, t in enumerate(times):
            want = [float(t), float(t) + half, float(t) + half, float(t) + dt]
            assert st[i].tobytes() == np.array(want).tobytes()
    assert rollout_stage_times(times, 0.05, "euler").tobytes() == times.tobytes()
    with pytest.raises(ValueError):
        rollout_stage_times(times, 0.05, "heun")


def test_c_abi_edges_on_host_only_handles(monkeypatch):
    """attaching stores a pointer (a host-only handle takes it); the launching entry points refuse a host-only handle
    and check their arguments before anything else"""
    from casclik_amd import _capi
    lib = _capi.load_library()
    monkeypatch.setenv("CLIK_HOST_ONLY", "1")
    d = lower_skill(time_skills.tracking_spec(skills.ur5()))
    desc = _capi.desc_to_c(d)
    opts = _capi.pinv_opts_to_c(cc.PseudoInverseController(skill_spec=time_skills.tracking_spec(skills.ur5())).options)
    h = C.c_void_p()
    assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h)) == 0
    try:
        assert lib.clik_pinv_attach_time_kernel(h, None) == 0
        assert lib.clik_pinv_attach_time_kernel(None, None) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_time_terms(None, 1, None, 1, 0.0, None, None) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_time_terms(h, 1, None, 1, 0.0, None, None) == _capi.CLIK_EINVAL
        assert b"host-only" in lib.clik_last_error()
        assert lib.clik_pinv_rollout_batch_dev(None, 1, 1, 0, 0.1, 0.0, None, None, None, None, None, None, None, None,
                                               0, 0, None, None, None, None, None) == _capi.CLIK_EINVAL
    finally:
        assert lib.clik_pinv_destroy(h) == 0
