"""CPU: the constraint-value kernel (clik_monitor.hpp, jit._MONITOR_TEMPLATE) - its translation unit cross-compiled for
gfx950 without scratch for a pinv shape, a QP shape, generated constraint code and time slots, in a unit no other kernel
shares - and what `constraint_values_batch` / `constraint_rows` / the C entry points do without a GPU."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import _capi, jit, skills
from casclik_amd.controllers.base_controller import constraint_row_slices, trajectory_rows
from casclik_amd.lowering import lower_skill

import time_skills
from extern_skills import dual_quaternion_skill

FIXTURES = ["stack", "qp", "dual_quaternion", "tracking"]


def _fixture(name):
    """(spec, controller that is not set up, "pinv" | "qp")"""
    if name == "stack":
        spec = skills.stack_skill(skills.iiwa())
        return spec, cc.PseudoInverseController(skill_spec=spec, options=dict(skills.STACK_OPTIONS)), "pinv"
    if name == "qp":
        spec = skills.qp_skill(skills.iiwa())
        return spec, cc.ReactiveQPController(skill_spec=spec), "qp"
    if name == "dual_quaternion":
        spec = dual_quaternion_skill(skills.ur5())
        return spec, cc.ReactiveQPController(skill_spec=spec), "qp"
    spec = time_skills.tracking_spec(skills.ur5())
    return spec, cc.PseudoInverseController(skill_spec=spec), "pinv"


@pytest.mark.parametrize("name", FIXTURES)
def test_monitor_unit_compiles_for_gfx950_without_scratch(name):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req = jit.unit_request(_fixture(name)[1])
    assert req.eligible
    d = req.descriptor
    if name == "dual_quaternion":
        assert d.extern_code                         # (the 8-row deviation runs as generated code)
    if name == "tracking":
        assert d.n_tslots > 0
    res = jit.unit_resources(jit.unit_text(jit._MONITOR_TEMPLATE, req.init, req.extern), req.init)
    assert len(res) == 1, sorted(res)        # (the one kernel of the unit: none of the tick / rollout kernels)
    for kernel, r in res.items():
        assert "constraint_values_kernel" in kernel
        assert r["ScratchSize"] == 0, r
        print(name, kernel[-24:], r)


def test_the_monitor_kernel_stays_out_of_the_other_translation_units():
    from casclik_amd.build import CSRC
    for fn in os.listdir(CSRC):
        if fn.endswith((".hpp", ".hip")) and fn not in ("clik_monitor.hpp", "clik_api.hip"):
            text = jit._code_only(open(os.path.join(CSRC, fn)).read())
            assert "clik_monitor" not in text and "constraint_values" not in text and "MonitorArgs" not in text, fn
    for tmpl in (jit._TEMPLATE, jit._VALUE_TEMPLATE, jit._QP_TEMPLATE, jit._QP_VALUE_TEMPLATE, jit._REC_TEMPLATE,
                 jit._VALUE_REC_TEMPLATE, jit._QP_REC_TEMPLATE, jit._QP_VALUE_REC_TEMPLATE, jit._TIME_TEMPLATE):
        assert "clik_monitor.hpp" not in tmpl and "constraint_values" not in tmpl
    assert re.findall(r'#include "([^"]+)"', jit._MONITOR_TEMPLATE) == ["clik_monitor.hpp"]
    assert 'extern "C" hipError_t clik_jit_constraint_values(' in jit._MONITOR_TEMPLATE
    api = jit._code_only(open(os.path.join(CSRC, "clik_api.hip")).read())
    assert "constraint_values_kernel" not in api and "clik_monitor.hpp" not in api      # entry points, no kernel
    # the header reads the static headers and declares nothing in them
    text = open(os.path.join(CSRC, "clik_monitor.hpp")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["clik_pinv_kernels.hpp"]


# what the source stamp of every OTHER instantiation is made of: the kernel headers before this one existed
_STAMP_HEADERS = ("clik_device.hpp", "clik_pinv_select.hpp", "clik_pinv_static.hpp", "clik_pinv_kernels.hpp",
                  "clik_pinv_team.hpp", "clik_qp_select.hpp", "clik_qp_static.hpp", "clik_qp_resident.hpp",
                  "clik_pinv_rec.hpp", "clik_qp_rec.hpp", "clik_rollout_lane.hpp", "clik_time.hpp")


def test_existing_templates_keep_their_request_ids_and_cache_tags():
    """What this pins: `clik_monitor.hpp` stays OUT of the source stamp all instantiations share - it is hashed into the
    tags of the units that include it and into no other, so editing it rebuilds nothing else - and no record under
    tests/golden/jit_records changes its name (request ids do not see the headers).  What it does not claim: the shared
    stamp also hashes include/clik.h, which gained the new entry points' declarations, so against the parent commit every
    cached object has a new tag and one build() recompiles them - as after every change of that header."""
    from casclik_amd.build import CSRC, DEVICE_FP
    h = hashlib.sha256()
    for fn in _STAMP_HEADERS:
        h.update(jit._code_only(open(os.path.join(CSRC, fn)).read()).encode())
    h.update(jit._code_only(open(os.path.join(jit.ROOT, "include", "clik.h")).read()).encode())
    h.update(" ".join(DEVICE_FP).encode())
    stamp = h.hexdigest()[:12]
    assert jit._source_stamp() == stamp
    for tmpl in ("", jit._QP_TEMPLATE, jit._REC_TEMPLATE, jit._QP_REC_TEMPLATE, jit._TIME_TEMPLATE):
        assert jit._unit_stamp(tmpl) == ""
        want = hashlib.sha256(("{1}" + "ext" + stamp + "-DX" + tmpl).encode()).hexdigest()[:16]
        assert jit._cache_tag("{1}", "ext", False, ["-DX"], tmpl) == want
    assert len(jit._unit_stamp(jit._MONITOR_TEMPLATE)) == 12
    assert jit._cache_tag("{1}", "", False, [], jit._MONITOR_TEMPLATE) != \
        hashlib.sha256(("{1}" + stamp + jit._MONITOR_TEMPLATE).encode()).hexdigest()[:16]
    # every record is still named after its request
    n = 0
    for fn in sorted(os.listdir(jit.RECORDS)):
        if fn.startswith("req_") and fn.endswith(".json"):
            with open(os.path.join(jit.RECORDS, fn)) as f:
                init, extern, stamps, extra, tmpl = jit._record_request(json.load(f))
            assert fn == "req_%s.json" % jit._request_id(init, extern, stamps, extra, tmpl), fn
            n += 1
    assert n > 100


# ---- what needs no GPU -----------------------------------------------------------------------------------------------------
def test_constraint_rows_are_the_tasks_rows_in_skill_order():
    d = lower_skill(skills.stack_skill(skills.iiwa()))
    rows = constraint_row_slices(d)
    assert list(rows.items()) == [("joint_limits", slice(0, 7)), ("tool_pose", slice(7, 13)),
                                  ("joint_centering", slice(13, 20))]
    rows = constraint_row_slices(lower_skill(skills.qp_skill(skills.iiwa())))       # (the VelocitySetConstraint counts)
    assert list(rows.items()) == [("joint_speed_limits", slice(0, 7)), ("tool_pose", slice(7, 13))]
    rows = constraint_row_slices(lower_skill(dual_quaternion_skill(skills.ur5())))
    assert rows["Q_dist2_cnstr"] == slice(rows["Q_dist2_cnstr"].start, rows["Q_dist2_cnstr"].start + 8)
    assert sorted(sl.start for sl in rows.values())[0] == 0 and max(sl.stop for sl in rows.values()) == 20


@pytest.mark.parametrize("name", ["stack", "qp"])
def test_methods_need_set_up(name):
    spec, ctrl, kind = _fixture(name)
    with pytest.raises(RuntimeError, match="setup"):
        ctrl.constraint_rows()
    with pytest.raises(RuntimeError, match="setup"):
        ctrl.constraint_values_batch(0.0, np.zeros((2, 7)), input_var=np.zeros((2, 7)))
    with pytest.raises(RuntimeError, match="setup"):
        ctrl.constraint_values(0.0, np.zeros(7), input_var=np.zeros(7))


def test_trajectory_arguments_are_checked_by_shape():
    assert trajectory_rows(np.zeros((5, 7)), 7, "robot_var")[1] == 2
    assert trajectory_rows(np.zeros((3, 5, 7)), 7, "robot_var")[1] == 3
    assert trajectory_rows(np.zeros((3, 5, 7)), 7, "input_var", (3, 5))[1] == 3
    with pytest.raises(ValueError, match="robot_var must have 7 columns"):
        trajectory_rows(np.zeros((3, 5, 6)), 7, "robot_var")
    with pytest.raises(ValueError, match=r"input_var \[R, B, 7\] has shape \(2, 5, 7\), robot_var 3 record"):
        trajectory_rows(np.zeros((2, 5, 7)), 7, "input_var", (3, 5))
    with pytest.raises(ValueError, match="virtual_var must be"):
        trajectory_rows(np.zeros((1, 3, 5, 2)), 2, "virtual_var")


def test_c_abi_edges_on_host_only_handles(monkeypatch):
    """the argument checks of the entry points come before anything touches a device: a host-only handle shows them"""
    lib = _capi.load_library()
    monkeypatch.setenv("CLIK_HOST_ONLY", "1")
    spec, ctrl, _ = _fixture("stack")
    d = lower_skill(spec)
    desc, opts = _capi.desc_to_c(d), _capi.pinv_opts_to_c(ctrl.options)
    h = C.c_void_p()
    assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h)) == 0
    q = C.c_void_p(64)          # (never dereferenced: every call below returns before a launch)
    try:
        assert lib.clik_pinv_n_constraint_rows(h) == 20 and lib.clik_pinv_n_constraint_rows(None) == 0
        assert lib.clik_pinv_attach_monitor_kernel(None, None) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_attach_monitor_kernel(h, None) == 0                      # (detaching takes any handle)
        assert lib.clik_pinv_attach_monitor_kernel(h, q) == _capi.CLIK_EINVAL         # (attaching needs the device)
        args = lambda n_rec, B, qq, e: (n_rec, B, None, 0, 0, qq, None, q, 0, e, None, None, None)      # noqa: E731
        assert lib.clik_pinv_constraint_values(None, *args(1, 1, q, q)) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_constraint_values(h, *args(-1, 1, q, q)) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_constraint_values(h, *args(0, 5, None, None)) == _capi.CLIK_OK
        assert lib.clik_pinv_constraint_values(h, *args(5, 0, None, None)) == _capi.CLIK_OK
        assert lib.clik_pinv_constraint_values(h, *args(1, 1, None, q)) == _capi.CLIK_EINVAL
        assert b"q must be" in lib.clik_last_error()
        assert lib.clik_pinv_constraint_values(h, *args(1, 1, q, None)) == _capi.CLIK_EINVAL
        assert b"all null" in lib.clik_last_error()
        assert lib.clik_pinv_constraint_values(h, *args(1, 1, q, q)) == _capi.CLIK_EUNSUPPORTED
        assert b"instantiated" in lib.clik_last_error()
    finally:
        assert lib.clik_pinv_destroy(h) == 0
    spec, qc, _ = _fixture("qp")
    d = lower_skill(spec)
    desc, qopts = _capi.desc_to_c(d), qc._c_options(d)
    assert lib.clik_qp_create(C.byref(desc), C.byref(qopts), C.byref(h)) == 0
    try:
        assert lib.clik_qp_n_constraint_rows(h) == 13
        assert lib.clik_qp_attach_monitor_kernel(h, None) == 0
        assert lib.clik_qp_constraint_values(h, 0, 0, None, 0, 0, None, None, None, 0, None, None, None, None) == 0
        assert lib.clik_qp_constraint_values(h, 2, 3, None, 0, 0, q, None, q, 0, None, None, None, None) == _capi.CLIK_EINVAL
        assert lib.clik_qp_constraint_values(h, 2, 3, None, 0, 0, q, None, q, 0, q, None, None, None) == _capi.CLIK_EUNSUPPORTED
        assert b"instantiated" in lib.clik_last_error()
    finally:
        assert lib.clik_qp_destroy(h) == 0


def test_a_record_names_the_record_that_holds_its_generated_code(tmp_path, monkeypatch):
    """the generated code of a skill is recorded once: a further unit of the same skill names that record
    (`extern_from`) and has no translation unit of its own; its name and its replayed text are those of a full record"""
    donor = "req_4d2ebb6b77deb3b9"              # (the double pendulum's QP tick kernel)
    with open(os.path.join(jit.RECORDS, donor + ".json")) as f:
        extern = json.load(f)["extern"]
    assert extern
    monkeypatch.setenv("CLIK_JIT_RECORD", str(tmp_path))
    monkeypatch.setenv("CLIK_JIT_NO_COMPILER", "1")
    init = "{2, 0}"                             # (never compiled: the request is recorded and nothing else happens)
    jit.build_shape_library(init, template=jit._MONITOR_TEMPLATE, extern=extern)
    jit.build_shape_library(init, template=jit._MONITOR_TEMPLATE, extern="")
    name = "req_%s" % jit._request_id(init, extern, False, [], jit._MONITOR_TEMPLATE)
    plain = "req_%s" % jit._request_id(init, "", False, [], jit._MONITOR_TEMPLATE)
    assert sorted(os.listdir(tmp_path)) == sorted([name + ".json", plain + ".json", plain + ".hip"])
    with open(tmp_path / (name + ".json")) as f:
        meta = json.load(f)
    assert meta["extern_from"] == donor and "extern" not in meta
    assert jit._record_request(meta, str(tmp_path))[1] == extern
    by_name = {os.path.basename(src)[:-4]: m for src, m, _ in jit._records(str(tmp_path))}
    assert by_name[name]["_text"] == jit._MONITOR_TEMPLATE % {"init": init, "extern": extern}
    assert "_text" not in by_name[plain]
    # the committed records of this form resolve, and every other record still has its translation unit
    for src, m, _ in jit._records():
        assert ("_text" in m) != os.path.exists(src), src


def test_a_record_whose_donor_is_gone_is_left_out_not_fatal(tmp_path):
    with open(tmp_path / "req_0000000000000000.json", "w") as f:
        json.dump({"stamps": False, "flags": [], "init": "{2, 0}", "extern_from": "req_ffffffffffffffff",
                   "template": jit._MONITOR_TEMPLATE}, f)
    assert jit._records(str(tmp_path)) == [] and jit.recorded_tags(str(tmp_path)) == []
