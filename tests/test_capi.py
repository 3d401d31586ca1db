"""The C-ABI library: loads, exports every symbol of include/clik.h, struct
layouts agree between C and ctypes, host-only entry points work (CPU only)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from casclik_amd import _capi, skills
from casclik_amd.lowering import lower_skill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clik.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_capi.LIB_PATH):
        from casclik_amd.build import build_hip
        build_hip()
    return _capi.load_library()


def test_exports_every_declared_symbol(lib):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(clik_[a-z_0-9]+)\s*\(", text)))
    assert len(declared) >= 16
    for name in declared:
        assert hasattr(lib, name), "libclik_hip.so does not export %s" % name
    assert sorted(_capi.exported_symbols()) == declared
    assert lib.clik_abi_version() == _capi.ABI_VERSION


_SNIPPET = """
/* a header in small: clik_in_a_comment(int x); is no declaration */
#define CLIK_MACRO(x) \\
    clik_in_a_macro(x)
typedef struct clik_thing { int32_t n; double v[3]; } clik_thing;
typedef struct clik_pinv clik_pinv;
extern "C" {
const char* clik_name(void);
int64_t clik_count ( const clik_pinv *h,int64_t  B );   // clik_in_a_line_comment(int x);
int clik_four_lines(const clik_pinv* h, int64_t B,
                    const double* q, /* the state */ double* dq,
                    int32_t *mode,
                    void* stream);
int clik_make(const clik_skill_desc* desc, const clik_qp_opts* opts, clik_qp** out);
int32_t clik_nothing();
}
"""


def test_parser_reads_synthetic_prototypes():
    """comments of both kinds, a macro, struct bodies, a prototype over four lines with a comment between two
    parameters, (void), an empty list, a ``const char*`` return, spaces in odd places"""
    assert _capi.parse_prototypes(_SNIPPET) == [
        ("clik_name", "const char*", []),
        ("clik_count", "int64_t", ["const clik_pinv*", "int64_t"]),
        ("clik_four_lines", "int", ["const clik_pinv*", "int64_t", "const double*", "double*", "int32_t*", "void*"]),
        ("clik_make", "int", ["const clik_skill_desc*", "const clik_qp_opts*", "clik_qp**"]),
        ("clik_nothing", "int32_t", []),
    ]
    vp = C.c_void_p
    assert _capi.prototype_ctypes(*_capi.parse_prototypes(_SNIPPET)[2]) == (C.c_int, [vp, C.c_int64, vp, vp, vp, vp])
    assert _capi.prototype_ctypes("clik_name", "const char*", []) == (C.c_char_p, [])
    assert _capi.prototype_ctypes(*_capi.parse_prototypes(_SNIPPET)[3]) == (
        C.c_int, [C.POINTER(_capi.clik_skill_desc), C.POINTER(_capi.clik_qp_opts), vp])
    assert _capi.parse_prototypes("int clik_unnamed(int64_t, const double*);") == [
        ("clik_unnamed", "int", ["int64_t", "const double*"])]


@pytest.mark.parametrize("decl, spelling", [("int clik_bad(const clik_pinv* h, float gain);", "float"),
                                            ("float clik_bad(void);", "float"),
                                            ("int clik_bad(const float* gains);", "const float*"),
                                            ("int clik_bad(double q[7]);", "double q[7]")])
def test_parser_refuses_an_unknown_type(decl, spelling):
    """no silent default: a type outside the mapping names the function and the spelling"""
    (proto,) = _capi.parse_prototypes(decl)
    with pytest.raises(_capi.ClikLibraryError) as err:
        _capi.prototype_ctypes(*proto)
    assert "clik_bad" in str(err.value) and repr(spelling) in str(err.value)


def test_parser_refuses_what_it_cannot_read():
    with pytest.raises(_capi.ClikLibraryError, match="clik_cb"):
        _capi.parse_prototypes("int clik_cb(void (*fn)(int), void* arg);")


def test_parser_finds_every_declared_name_of_the_header():
    """on include/clik.h the parser returns exactly the names the regular expression of
    test_exports_every_declared_symbol finds, each once: nothing is skipped"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(clik_[a-z_0-9]+)\s*\(", text)))
    protos = _capi.parse_prototypes(open(HEADER).read())
    assert sorted(name for name, _, _ in protos) == declared
    assert _capi.exported_symbols() == [name for name, _, _ in protos]


def test_loaded_functions_carry_the_header_prototypes(lib):
    """after load_library() every function has the header's parameter count and kinds; the three struct parameters are
    typed pointers, which refuse a wrong struct"""
    protos = _capi.header_prototypes()
    assert len(protos) >= 76
    scalars = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    structs = {"const clik_skill_desc*": _capi.clik_skill_desc, "const clik_pinv_opts*": _capi.clik_pinv_opts,
               "const clik_qp_opts*": _capi.clik_qp_opts}
    seen = set()
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(params), name
        for spelling, ctype in zip([ret] + params, [fn.restype] + list(fn.argtypes)):
            if spelling in scalars:
                assert ctype is scalars[spelling], (name, spelling)
            elif spelling in structs:
                assert ctype is not C.c_void_p and ctype._type_ is structs[spelling], (name, spelling)
                seen.add(spelling)
            elif spelling in ("const char*", "char*"):
                assert ctype is C.c_char_p, (name, spelling)
            else:
                assert spelling.endswith("*") and ctype is C.c_void_p, (name, spelling)
    assert seen == set(structs)
    with pytest.raises(C.ArgumentError):
        lib.clik_pinv_create(C.byref(_capi.clik_qp_opts()), None, None)


def test_a_declared_function_the_library_lacks_fails_at_load(lib, monkeypatch):
    monkeypatch.setattr(_capi, "_prototypes", _capi.header_prototypes() + [("clik_not_there", "int", [])])
    with pytest.raises(_capi.ClikLibraryError, match="clik_not_there"):
        _capi.load_library(_capi.LIB_PATH)


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clik.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(clik_joint),sizeof(clik_row),sizeof(clik_task),sizeof(clik_skill_desc),'
                   'sizeof(clik_pinv_opts),sizeof(clik_qp_opts),offsetof(clik_skill_desc,rows),offsetof(clik_task,gain));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_capi.clik_joint), C.sizeof(_capi.clik_row), C.sizeof(_capi.clik_task),
            C.sizeof(_capi.clik_skill_desc), C.sizeof(_capi.clik_pinv_opts), C.sizeof(_capi.clik_qp_opts),
            _capi.clik_skill_desc.rows.offset, _capi.clik_task.gain.offset]
    assert got == want


def test_shape_describe_and_generated_table(lib):
    """The AOT shape table must contain exactly what the run-time dispatcher
    derives for the BASELINE skills (tools/gen_shapes.py keeps them in sync)."""
    gen = open(os.path.join(ROOT, "casclik_amd", "csrc", "clik_shapes_gen.hpp")).read()
    for name, spec, extra in [("kStackIiwa", skills.stack_skill(), skills.STACK_OPTIONS),
                              ("kPose6Iiwa", skills.pose_skill(), None),
                              ("kPos3Iiwa", skills.position_skill(), None)]:
        opts = {"feedforward": True, "multidim_sets": False, "converge_final_set_to_max": False,
                "pinv_method": "damped", "damping_factor": 1e-7}
        opts.update(extra or {})
        desc = _capi.desc_to_c(lower_skill(spec))
        buf = C.create_string_buffer(4096)
        rc = lib.clik_shape_describe(C.byref(desc), C.byref(_capi.pinv_opts_to_c(opts)), buf, len(buf))
        assert rc == 1
        assert "ShapeDesc %s = %s;" % (name, buf.value.decode()) in gen


def test_create_rejects_malformed_descriptors(lib):
    desc = _capi.desc_to_c(lower_skill(skills.pose_skill()))
    opts = _capi.pinv_opts_to_c({"feedforward": True, "multidim_sets": False,
                                 "converge_final_set_to_max": False, "pinv_method": "damped",
                                 "damping_factor": 1e-7})
    h = C.c_void_p()
    desc.abi_version = 99
    assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h)) == -1
    assert b"ABI version" in lib.clik_last_error()
    desc.abi_version = _capi.ABI_VERSION
    desc.n_q = 15          # (beyond CLIK_MAX_DOF = 14; 9 ... 14 states get a handle that waits for an instantiated kernel)
    assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h)) == -2
    desc.n_q = 7
    desc.tasks[0].out_row0[0] = 500
    assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h)) == -1
    # multidimensional set without multidim_sets: the reference's NotImplementedError
    sdesc = _capi.desc_to_c(lower_skill(skills.stack_skill()))
    assert lib.clik_pinv_create(C.byref(sdesc), C.byref(opts), C.byref(h)) == -2
    assert b"multidim_sets" in lib.clik_last_error()
    assert lib.clik_pinv_create(None, C.byref(opts), C.byref(h)) == -1
    assert lib.clik_pinv_solve_batch(None, 1, None, None, None, None, None, None, None, None) == -1


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(_capi.ClikLibraryError, match="no CPU fallback|not found"):
        _capi.load_library(str(tmp_path / "libclik_hip.so"))


def test_host_only_handles_answer_queries_and_refuse_to_solve(lib, monkeypatch):
    """clik_pinv_create_host / clik_qp_create_host (include/clik.h): a handle without any device allocation - what
    casclik_amd/jit.py uses to get a skill's image words on a machine without a GPU; every solve entry point refuses it.
    The flag is per call: an ordinary create next to it is NOT host-only (here, without a GPU, it fails in hipMalloc
    instead of succeeding); CLIK_HOST_ONLY=1 still turns a whole process host-only."""
    desc = _capi.desc_to_c(lower_skill(skills.stack_skill()))
    opts = _capi.pinv_opts_to_c({"feedforward": True, "multidim_sets": True, "converge_final_set_to_max": False,
                                 "pinv_method": "damped", "damping_factor": 1e-7})
    h = C.c_void_p()
    assert lib.clik_pinv_create_host(C.byref(desc), C.byref(opts), C.byref(h)) == 0
    buf = (C.c_uint64 * 16384)()
    n = lib.clik_pinv_image_words(h, buf, len(buf))
    assert n > 100 and lib.clik_pinv_n_modes(h) == 2
    assert lib.clik_pinv_solve_batch(h, 4, None, None, None, None, None, None, None, None) == -1
    assert b"host-only" in lib.clik_last_error()
    assert lib.clik_pinv_destroy(h) == 0
    import torch
    if not torch.cuda.is_available():
        h2 = C.c_void_p()
        assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h2)) != 0      # (no device: hipMalloc fails)
    monkeypatch.setenv("CLIK_HOST_ONLY", "1")
    h3 = C.c_void_p()
    assert lib.clik_pinv_create(C.byref(desc), C.byref(opts), C.byref(h3)) == 0 and lib.clik_pinv_destroy(h3) == 0
    monkeypatch.delenv("CLIK_HOST_ONLY")
    from casclik_amd import jit
    qd = _capi.desc_to_c(lower_skill(skills.qp_skill()))
    words = jit.host_image_words(lib, "qp", qd, _capi.qp_opts_to_c(0.001, [1.0] * 7, [1.0] * 6))
    assert words and len(words) > 100


# kernel_name + clik_qp_kernel_variant of the config-4 skill on the iiwa and on the UR5 (shape-specialised kernels from
# the ahead-of-time table, box family) and of a hard pose task (no AOT shape: the built-in kernel), with one switch set at
# a time, for the image-reading kernels and with a value-specialised kernel attached.  A host-only handle counts no CUs, so no batch gets the four-waves cold tick
# (the GPU tests pin that one); every batch size and start gets the same label.
_QP_SELECT_B = (1, 64, 4096, 16384, 16385, 131072, 1 << 20)
_QP_SELECT_ENV = (None, "CLIK_FORCE_DYNAMIC=1", "CLIK_NO_AOT=1", "CLIK_QP_FOLIO=0")
_QP_SELECT_TABLE = {
    # (skill, switch, value kernel attached): label
    ("config4_iiwa", None, False): "qp_static_kQpPoseIiwa",
    ("config4_iiwa", None, True): "qp_static_kQpPoseIiwa/v",
    ("config4_iiwa", "CLIK_FORCE_DYNAMIC=1", False): "dynamic",
    ("config4_iiwa", "CLIK_FORCE_DYNAMIC=1", True): "dynamic",
    ("config4_iiwa", "CLIK_NO_AOT=1", False): "dynamic",
    ("config4_iiwa", "CLIK_NO_AOT=1", True): "dynamic",
    ("config4_iiwa", "CLIK_QP_FOLIO=0", False): "qp_static_kQpPoseIiwa",
    ("config4_iiwa", "CLIK_QP_FOLIO=0", True): "qp_static_kQpPoseIiwa/v",
    ("config4_ur5", None, False): "qp_static_kQpPoseUr5",
    ("config4_ur5", None, True): "qp_static_kQpPoseUr5/v",
    ("config4_ur5", "CLIK_FORCE_DYNAMIC=1", False): "dynamic",
    ("config4_ur5", "CLIK_FORCE_DYNAMIC=1", True): "dynamic",
    ("config4_ur5", "CLIK_NO_AOT=1", False): "dynamic",
    ("config4_ur5", "CLIK_NO_AOT=1", True): "dynamic",
    ("config4_ur5", "CLIK_QP_FOLIO=0", False): "qp_static_kQpPoseUr5",
    ("config4_ur5", "CLIK_QP_FOLIO=0", True): "qp_static_kQpPoseUr5/v",
    ("hard_pose_iiwa", None, False): "dynamic",
    ("hard_pose_iiwa", None, True): "dynamic",
    ("hard_pose_iiwa", "CLIK_FORCE_DYNAMIC=1", False): "dynamic",
    ("hard_pose_iiwa", "CLIK_FORCE_DYNAMIC=1", True): "dynamic",
    ("hard_pose_iiwa", "CLIK_NO_AOT=1", False): "dynamic",
    ("hard_pose_iiwa", "CLIK_NO_AOT=1", True): "dynamic",
    ("hard_pose_iiwa", "CLIK_QP_FOLIO=0", False): "dynamic",
    ("hard_pose_iiwa", "CLIK_QP_FOLIO=0", True): "dynamic",
}


@pytest.mark.parametrize("skill", ["config4_iiwa", "config4_ur5", "hard_pose_iiwa"])
@pytest.mark.parametrize("env", _QP_SELECT_ENV)
def test_qp_kernel_selection_table(lib, monkeypatch, skill, env):
    """The kernel choice of the QP path (qp_select, clik_qp_select.hpp) against a written-out table, on host-only handles:
    a host-only handle picks its ahead-of-time shape as a device handle does and reports the same kernel name.  The
    switches are read at creation; the value-specialised kernel is a stand-in that is never called, and a handle that no
    shape-specialised kernel serves refuses it."""
    import casclik_amd as cc
    for name in ("CLIK_FORCE_DYNAMIC", "CLIK_NO_AOT", "CLIK_QP_FOLIO", "CLIK_HOST_ONLY"):
        monkeypatch.delenv(name, raising=False)
    if env:
        monkeypatch.setenv(*env.split("="))
    fk = skills.ur5() if skill == "config4_ur5" else skills.iiwa()
    spec = skills.pose_skill(fk) if skill == "hard_pose_iiwa" else skills.qp_skill(fk)
    d = lower_skill(spec)
    copts = cc.ReactiveQPController(skill_spec=spec)._c_options(d)
    desc = _capi.desc_to_c(d)
    h = C.c_void_p()
    assert lib.clik_qp_create_host(C.byref(desc), C.byref(copts), C.byref(h)) == 0
    try:
        def labels():
            name = lib.clik_qp_kernel_name(h).decode()
            return {name + lib.clik_qp_kernel_variant(h, B, hot).decode() for B in _QP_SELECT_B for hot in (0, 1)}
        assert labels() == {_QP_SELECT_TABLE[(skill, env, False)]}

        def never(*args):
            raise AssertionError("the stand-in value kernel was called")
        stand_in = C.CFUNCTYPE(C.c_int)(never)
        shape_served = _QP_SELECT_TABLE[(skill, env, False)].startswith("qp_static_")
        assert lib.clik_qp_attach_value_kernel(h, C.cast(stand_in, C.c_void_p), None) == \
            (0 if shape_served else _capi.CLIK_EUNSUPPORTED)
        assert labels() == {_QP_SELECT_TABLE[(skill, env, True)]}
    finally:
        assert lib.clik_qp_destroy(h) == 0

def test_ticket_layout(tmp_path):
    """clik_ticket (resident ticks): 256 bytes, the words the Python layer indexes"""
    src = tmp_path / "tk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clik.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(clik_ticket),offsetof(clik_ticket,in_seq),offsetof(clik_ticket,stop),offsetof(clik_ticket,waves),'
                   'offsetof(clik_ticket,ticks_done),offsetof(clik_ticket,ring_depth),offsetof(clik_ticket,integrate_dt),'
                   'offsetof(clik_ticket,max_speed));return 0;}\n')
    exe = tmp_path / "tk"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    # (int32 words 16: ring_depth; float64 words 9, 10: integrate_dt, max_speed - casclik_amd/controllers/pseudo_inverse.py)
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [256, 0, 4 * 32, 4 * 48, 4 * 49, 4 * 16,
                                                                               8 * 9, 8 * 10]


# clik_pinv_kernel_variant for the stack skill (config 3: the four-lanes-per-instance family, one SetConstraint) and the
# pose skill (single-mode, forward kinematics), at these batch sizes, with one measuring switch set at a time, for the
# image-reading kernels and with a value-specialised kernel attached
_SELECT_B = (1, 4096, 16384, 16385, 32768, 32769, 131072, 524287, 524288, 1 << 20, (1 << 24) + 1)
_SELECT_TABLE = {
    ("stack", None, False): ["team4", "team4", "team4", "mp2", "mp2", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("stack", "CLIK_LANES=1", False): ["mp2", "mp2", "mp2", "mp2", "mp2", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("stack", "CLIK_LANES=4", False): ["team4"] * 11,
    ("stack", "CLIK_MODE_PARALLEL=0", False): ["team4", "team4", "team4", "lane", "lane", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("stack", "CLIK_LARGE_BATCH=0", False): ["team4", "team4", "team4", "mp2", "mp2", "lane", "lane", "lane", "lane", "lane", "lane"],
    ("stack", "CLIK_QUAD_FRONT=0", False): ["team4", "team4", "team4", "mp2", "mp2", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("stack", None, True): ["team4v", "team4v", "team4v", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("stack", "CLIK_LANES=1", True): ["lanev"] * 11,
    # (the value-specialised team tick addresses its rows with 24-bit row numbers: the lane kernel beyond)
    ("stack", "CLIK_LANES=4", True): ["team4v"] * 10 + ["lanev"],
    ("stack", "CLIK_MODE_PARALLEL=0", True): ["team4v", "team4v", "team4v", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("stack", "CLIK_LARGE_BATCH=0", True): ["team4v", "team4v", "team4v", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("stack", "CLIK_QUAD_FRONT=0", True): ["team4v", "team4v", "team4v", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("pose", None, False): ["lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("pose", "CLIK_LANES=1", False): ["lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("pose", "CLIK_LANES=4", False): ["lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("pose", "CLIK_MODE_PARALLEL=0", False): ["lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("pose", "CLIK_LARGE_BATCH=0", False): ["lane"] * 11,
    ("pose", "CLIK_QUAD_FRONT=0", False): ["lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane", "lane/occ2", "lane/occ2", "lane/occ2"],
    ("pose", None, True): ["quadv", "quadv", "quadv", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("pose", "CLIK_LANES=1", True): ["quadv", "quadv", "quadv", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("pose", "CLIK_LANES=4", True): ["quadv", "quadv", "quadv", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("pose", "CLIK_MODE_PARALLEL=0", True): ["quadv", "quadv", "quadv", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("pose", "CLIK_LARGE_BATCH=0", True): ["quadv", "quadv", "quadv", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev", "lanev"],
    ("pose", "CLIK_QUAD_FRONT=0", True): ["lanev"] * 11,
}


@pytest.mark.parametrize("skill", ["stack", "pose"])
@pytest.mark.parametrize("env", [None, "CLIK_LANES=1", "CLIK_LANES=4", "CLIK_MODE_PARALLEL=0", "CLIK_LARGE_BATCH=0",
                                 "CLIK_QUAD_FRONT=0"])
def test_kernel_variant_selection_table(lib, monkeypatch, skill, env):
    """The kernel choice of the pseudo-inverse path (pinv_select, clik_pinv_select.hpp) against a written-out table, on
    host-only handles.  The switches are read at creation; the value-specialised kernel attached is a stand-in that is
    never called (a host-only handle launches nothing)."""
    import casclik_amd as cc
    for name in ("CLIK_LANES", "CLIK_MODE_PARALLEL", "CLIK_LARGE_BATCH", "CLIK_QUAD_FRONT"):
        monkeypatch.delenv(name, raising=False)
    if env:
        monkeypatch.setenv(*env.split("="))
    fk = skills.iiwa()
    spec = skills.stack_skill(fk) if skill == "stack" else skills.pose_skill(fk)
    opts = dict(skills.STACK_OPTIONS) if skill == "stack" else {}
    desc = _capi.desc_to_c(lower_skill(spec))
    copts = _capi.pinv_opts_to_c(cc.PseudoInverseController(skill_spec=spec, options=opts).options)
    h = C.c_void_p()
    assert lib.clik_pinv_create_host(C.byref(desc), C.byref(copts), C.byref(h)) == 0
    try:
        assert lib.clik_pinv_kernel_name(h).decode() == ("kStackIiwa" if skill == "stack" else "kPose6Iiwa")
        got = [lib.clik_pinv_kernel_variant(h, B).decode() for B in _SELECT_B]
        assert got == _SELECT_TABLE[(skill, env, False)]

        def never(*args):
            raise AssertionError("the stand-in value kernel was called")
        stand_in = C.CFUNCTYPE(C.c_int)(never)
        assert lib.clik_pinv_attach_value_kernel(h, C.cast(stand_in, C.c_void_p), None) == 0
        got = [lib.clik_pinv_kernel_variant(h, B).decode() for B in _SELECT_B]
        assert got == _SELECT_TABLE[(skill, env, True)]
    finally:
        assert lib.clik_pinv_destroy(h) == 0
