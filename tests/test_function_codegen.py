"""CPU: a cs.Function as generated code (codegen.emit_function) - the shape of its text, its values as host C++ against
`Function.__call__` under the derived tolerance of function_cases.py, its kernel compiled for gfx950 without scratch in a
translation unit no other kernel shares - and what `DeviceFunction` does without a GPU: request identity, argument
marshalling, refusals."""
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess

import mpmath  # noqa: F401  (function_cases.exact_eval: the check of the tolerance rule must not skip)
import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import codegen, jit
from casclik_amd import sym as cs
from casclik_amd.function_batch import DeviceFunction, output_shape, plan_arguments

import function_cases as fc

SINCOS_PAIRS = {"tool": 6, "manip": 6, "pend": 2, "wide": 14,        # distinct arguments of sin / cos
                "ops_pow": 1, "ops_libm": 3, "ops_sel": 3, "trig": 1, "ties": 0}


# ---- emitted text ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_source_stores_every_output_entry_once_and_reads_none_back(name):
    fn = fc.get(name)
    text = codegen.emit_function(fn)
    ins, outs = codegen.function_layout(fn)
    n_x, n_y = sum(a * b for a, b, _ in ins), sum(a * b for a, b, _ in outs)
    assert "struct BatchFn" in text and "eval(const double (&x)[%d], double (&y)[%d])" % (n_x, n_y) in text
    assert "n_in = %d, n_out = %d, n_x = %d, n_y = %d;" % (len(ins), len(outs), n_x, n_y) in text
    body = text.split("(void)x;")[1]
    stores = re.findall(r"\by\[(\d+)\] = ", body)
    assert sorted(int(k) for k in stores) == list(range(n_y))
    assert len(body.split("y[")) - 1 == n_y                              # (and no read of y)
    assert all(int(k) < n_x for k in re.findall(r"\bx\[(\d+)\]", body))
    pairs = re.findall(r"sincos_joint\(([^,]+),", body)
    assert len(pairs) == len(set(pairs)) == SINCOS_PAIRS[name]
    assert not re.search(r"\b(z|ys|tv|K)\b", jit._code_only(body))      # no skill state, time slot or kernel-side FK
    assert text == codegen.emit_function(fc.make(name))                  # the text depends on the expression only


def test_an_unused_input_is_not_read_and_a_matrix_input_is_row_major():
    text = codegen.emit_function(fc.get("manip"))
    assert "in_w[2] = {1, 6};" in text and "in_off[2] = {0, 1};" in text and "out_w[3] = {3, 18, 1};" in text
    assert not re.search(r"\bx\[0\]", text)                              # t
    # M (3 x 2) of `wide` sits behind a (14): M[i, j] is x[14 + 2 i + j], and the scalar output weighs it 1 + i + 3 j
    a, M, s = cs.MX.sym("a", 14), cs.MX.sym("M", 3, 2), cs.MX.sym("s")
    for i in range(3):
        for j in range(2):
            text = codegen.emit_function(cs.Function("pick", [a, M, s], [M[i, j] * 2.0]))
            assert "y[0] = v0;" in text and "const double v0 = x[%d] * 2.0;" % (14 + 2 * i + j) in text


def test_a_foreign_symbol_and_an_unknown_operation_are_refused():
    q, z = cs.MX.sym("q", 2), cs.MX.sym("z", 2)
    with pytest.raises(NotImplementedError, match="symbol 'z' is not an input of the function 'f'"):
        codegen.emit_function(cs.Function("f", [q], [q[0] + z[1]]))
    bad = cs.MX(_array=np.array([[cs.Scalar("erf", (cs._as_array(q)[0, 0],))]], dtype=object))
    with pytest.raises(NotImplementedError, match="no device code for operation 'erf'"):
        codegen.emit_function(cs.Function("g", [q], [bad]))
    with pytest.raises(NotImplementedError, match="without inputs or outputs"):
        codegen.emit_function(cs.Function("h", [q], []))


# ---- host compilation ------------------------------------------------------------------------------------------------------
_HOST_WRAPPER = """#include <cmath>
#define __device__
#define __forceinline__ inline
static inline void sincos_joint(double x, double& s, double& c) { sincos(x, &s, &c); }
%s
extern "C" void fn_eval(const double* xin, double* yout)
{
    double x[BatchFn::n_x], y[BatchFn::n_y];
    for (int i = 0; i < BatchFn::n_x; ++i) x[i] = xin[i];
    BatchFn::eval(x, y);
    for (int i = 0; i < BatchFn::n_y; ++i) yout[i] = y[i];
}
"""


@pytest.fixture(scope="module")
def host_code(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    made = {}

    def get(name):
        if name not in made:
            d = tmp_path_factory.mktemp("fn_" + name)
            src = d / "fn.cpp"
            src.write_text(_HOST_WRAPPER % codegen.emit_function(fc.get(name)))
            so = d / "fn.so"
            subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(so)])
            f = C.CDLL(str(so)).fn_eval
            f.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
            f.restype = None
            ins, outs = codegen.function_layout(fc.get(name))
            n_y = sum(a * b for a, b, _ in outs)

            def run(args):
                x = np.concatenate([np.asarray(a, dtype=float).reshape(-1) for a in args])     # (row-major rows)
                y = np.full(n_y, np.nan)
                f(x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double)))
                return [y[o:o + a * b].reshape(a, b) for a, b, o in outs]
            made[name] = run
        return made[name]
    return get


@pytest.mark.parametrize("name", fc.NAMES)
def test_emitted_text_as_host_code_matches_the_host_evaluator(host_code, name):
    """the generated text under g++ without contraction against `Function.__call__`, every entry of every output at
    every point of the pool, under |a - b| <= 2 (bound + bound) of function_cases.running_bound"""
    run = host_code(name)
    vals, bnds = fc.reference(name)
    worst = 0.0
    for r in range(fc.lead(name)[0]):
        for b in range(fc.lead(name)[1]):
            for got, want, bound in zip(run(fc.point(name, r, b)), vals, bnds):
                ratio = fc.worst_ratio(got, want[r, b], bound[r, b])
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, r, b, got, want[r, b], bound[r, b])
    print("%s: worst host-code deviation, in units of the tolerance: %.3g" % (name, worst))


def test_the_jacobian_output_is_the_chains_numeric_derivative(host_code):
    """the 'fk_d' expansion against urdf.Chain.fk_derivative_numeric (products of the joints' matrices, one of them
    differentiated): J[i][k] = d T[i][3] / d q_k, under the same rule"""
    run = host_code("manip")
    chain = fc.ur5_chain()
    _, bnds = fc.reference("manip")
    for r, b in [(0, 0), (0, 100), (1, 7), (2, 256)]:
        args = fc.point("manip", r, b)
        dT = chain.fk_derivative_numeric(args[1])
        want = np.array([[dT[k][i, 3] for k in range(6)] for i in range(3)])
        assert fc.worst_ratio(run(args)[1], want, bnds[1][r, b]) <= 1.0
        assert fc.worst_ratio(fc.host_call(fc.get("manip"), args)[1], want, bnds[1][r, b]) <= 1.0


# ---- the bound itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_the_reference_side_stays_within_the_running_bound(name):
    """the same DAG at 40 digits (mpmath): |Function.__call__ - exact| <= 2 running_bound at every point of the pool -
    the rule the device is held to, applied to the host evaluator alone"""
    vals, bnds = fc.reference(name)
    his, los = fc.exact_reference(name)
    worst = 0.0
    for k, (want, hi, lo, bound) in enumerate(zip(vals, his, los, bnds)):
        for r in range(fc.lead(name)[0]):
            for b in range(fc.lead(name)[1]):
                ratio = fc.worst_exact_ratio(want[r, b], hi[r, b], lo[r, b], bound[r, b])
                assert ratio <= 1.0, (name, k, r, b, want[r, b], hi[r, b], bound[r, b])
                worst = max(worst, ratio)
    print("%s: worst |host - exact| in units of 2 bound: %.3g" % (name, worst))


def test_the_bound_sees_cancellation_and_the_switch_helper_fires():
    x = cs.MX.sym("x", 2)
    f = cs.Function("c", [x], [(x[0] + x[1]) - x[0], cs.fabs(x[0] - x[1])])
    b = fc.running_bound(f, (np.array([1e8, 1.0]),))
    assert b[0][0, 0] >= fc.U * 1e8                                       # the rounding of 1e8 + 1 survives the subtraction
    fc.assert_no_switch_nearby(f, (np.array([1.0, 2.0]),))
    with pytest.raises(AssertionError):
        fc.assert_no_switch_nearby(f, (np.array([1.0, 1.0 + 1e-9]),))
    # the logic helpers compare truth values with 0.0: no switch that rounding could flip, but their own arguments are
    g = cs.Function("l", [x], [cs.if_else(cs.logic_or(cs.logic_and(x[0] < 1.5, x[1] != 0.25), cs.logic_not(x[0] >= x[1])),
                                          x[0], x[1])])
    fc.assert_no_switch_nearby(g, (np.array([1.0, 2.0]),))
    fc.assert_no_switch_nearby(g, (np.array([2.0, 1.0]),))          # (every truth value 0 but the last)
    for near in ([1.5 - 1e-9, 2.0], [1.0, 0.25 + 1e-9], [1.0, 1.0 - 1e-9]):
        with pytest.raises(AssertionError):
            fc.assert_no_switch_nearby(g, (np.array(near),))
    with pytest.raises(AssertionError):                              # a condition that is no truth value
        fc.assert_no_switch_nearby(cs.Function("m", [x], [cs.if_else(x[0] * x[1], x[0], x[1])]), (np.array([1e-4, 1e-4]),))


# ---- derivatives, selections at their ties, IEEE edges -----------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.OPS)
def test_jacobian_outputs_are_the_central_differences_of_the_value_column(name):
    """autodiff.diff_scalar without a second implementation of its rules: the Jacobian outputs of `Function.__call__`
    against central differences (h = 1e-25) of the VALUE column alone at 80 digits, whose truncation (h^2 f''' / 6,
    1e-50) and rounding (1e-80 / h) are far below the rule |J - exact| <= 2 running_bound of the Jacobian entry"""
    fn = fc.get(name)
    value = cs.Function("value", fn._inputs, [fn._outputs[0]])
    vals, bnds = fc.reference(name)
    m = fn._outputs[0].shape[0]
    worst = 0.0
    for r, b in [(0, 0), (0, 1), (0, 64), (1, 2), (1, 100), (2, 3), (2, 200), (2, 256)]:
        args = fc.point(name, r, b)
        for k, n_k in ((0, 4), (1, 3)):
            for j in range(n_k):
                d = fc.central_difference(value, args, k, j)
                for i in range(m):
                    err = abs(float(d[i] - mpmath.mpf(vals[1 + k][r, b][i, j])))
                    tol = 2.0 * bnds[1 + k][r, b][i, j]
                    assert err <= (tol if tol > 0.0 else 1e-40), (name, r, b, k, i, j, err, tol)
                    if tol > 0.0:
                        worst = max(worst, err / tol)
    print("%s: worst |host Jacobian - central difference| in units of 2 bound: %.3g" % (name, worst))


def test_selections_at_their_ties_follow_the_stated_rules(host_code):
    """`ties`: fmin / fmax of equal arguments and of neighbouring doubles, their derivatives (the first argument's at a
    tie), sign and the derivative of fabs at +0.0, the four comparisons on equal arguments, if_else on 0.0 and 0.3 - the
    host evaluator and the generated text against the outputs written out by hand, bit for bit"""
    fn = fc.get("ties")
    run = host_code("ties")
    vals, bnds = fc.reference("ties")
    assert all((b == 0.0).all() for b in bnds)
    tied = 0
    for r in range(fc.lead("ties")[0]):
        for b in range(fc.lead("ties")[1]):
            args = fc.point("ties", r, b)
            tied += args[0][0] == args[0][1]
            for want, host, code in zip(fc.ties_expected(args), fc.host_call(fn, args), run(args)):
                assert want.tobytes() == host.tobytes() == code.tobytes(), (r, b, args, want, host, code)
    assert tied == 3 * 86
    # at a tie: both take the first argument's derivative, <= and == hold, != and < do not, 0.3 is true
    x, w = np.array([0.75, 0.75]), np.array([-1.0, 2.0])
    col, J, d = fc.host_call(fn, (x, 0.0, w, np.array([0.0, 0.3])))
    assert col[:, 0].tolist() == [0.75, 0.75, 0.0, -1.0, -1.0, 2.0, 2.0, 2.0, -1.0]
    assert J.tolist() == [[1.0, 0.0], [1.0, 0.0]] and d.tolist() == [[0.0]]


def test_the_host_evaluator_answers_as_ieee_does_where_python_raises():
    """log(0), log(-1), sqrt(-1), exp(800), 0 ** -1, tan / sin of inf, a negative base under a fractional exponent:
    what CasADi and the device return, not an exception; and a constant base (`2.0 ** x`)"""
    inf = float("inf")
    x = cs.MX.sym("x")
    one = {"log": cs.log, "sqrt": cs.sqrt, "exp": cs.exp, "tan": cs.tan, "sin": cs.sin, "cos": cs.cos, "asin": cs.asin,
           "acos": cs.acos, "atan": cs.atan, "tanh": cs.tanh, "fabs": cs.fabs, "sign": cs.sign}

    def at(op, v):
        return float(cs.Function("f", [x], [one[op](x)])(v))
    assert at("log", 0.0) == -inf and np.isnan(at("log", -1.0)) and at("log", inf) == inf
    assert np.isnan(at("sqrt", -1.0)) and at("sqrt", 0.0) == 0.0 and at("sqrt", inf) == inf
    assert at("exp", 800.0) == inf and at("exp", -800.0) == 0.0 and at("exp", -inf) == 0.0
    assert all(np.isnan(at(op, s * inf)) for op in ("tan", "sin", "cos") for s in (1.0, -1.0))
    assert np.isnan(at("asin", 1.5)) and np.isnan(at("acos", -1.5))
    assert at("atan", inf) == math.pi / 2 and at("tanh", 1e3) == 1.0 and at("tanh", -inf) == -1.0
    assert at("fabs", -inf) == inf and at("sign", -inf) == -1.0 and at("sign", 0.0) == 0.0
    for op in one:                      # a NaN goes through every one of them, sign excepted (no comparison holds)
        assert np.isnan(at(op, float("nan"))) or op == "sign"
    # pow
    y = cs.MX.sym("y")
    p = cs.Function("p", [x, y], [x ** y])
    assert float(p(0.0, -1.0)) == inf and float(p(0.0, -2.0)) == inf and float(p(0.0, -0.5)) == inf
    assert float(p(1e200, 2.0)) == inf and float(p(-1e200, 3.0)) == -inf and float(p(-1e200, 2.0)) == inf
    assert np.isnan(float(p(-8.0, 0.5))) and float(p(-8.0, 3.0)) == -512.0 and float(p(0.0, 0.0)) == 1.0
    assert float(cs.Function("q", [x], [x ** -1])(0.0)) == inf
    # a constant base
    r = 2.0 ** cs.vertcat(x, y)
    assert isinstance(r, cs.MX) and r.shape == (2, 1)
    assert cs.Function("r", [x, y], [r])(3.0, -1.0).toarray().ravel().tolist() == [8.0, 0.5]
    assert float(cs.Function("s", [x], [cs.jacobian(2.0 ** x, x)])(3.0)) == 8.0 * math.log(2.0)
    folded = cs.Function("c", [x], [cs.vertcat(cs.MX(2.0) ** cs.MX(-1075.0), cs.MX(0.0) ** cs.MX(-1.0), cs.log(cs.MX(0.0)))])
    assert folded(1.0).toarray().ravel().tolist() == [0.0, inf, -inf]
    # 1 / 0 as before
    assert float(cs.Function("d", [x], [1.0 / x])(0.0)) == inf
    # the points of the device's edge test (test_gpu_function_batch.py)
    for point, want in zip(fc.EDGE_POINTS, fc.EDGE_VALUES):
        assert fc.host_call(fc.get("edges"), (point,))[0].tobytes() == want.reshape(5, 1).tobytes()


# ---- device compilation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_function_kernel_compiles_for_gfx950_alone_and_without_scratch(name):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    res = jit.unit_resources(jit.unit_text(jit._FUNCTION_TEMPLATE, "", codegen.emit_function(fc.get(name))), "")
    assert len(res) == 1, sorted(res)
    (kernel, r), = res.items()
    assert "function_batch_kernel" in kernel
    assert r["ScratchSize"] == 0, r
    print(name, r)


# ---- isolation and caching -------------------------------------------------------------------------------------------------
_OLD_TEMPLATES = ("_TEMPLATE", "_VALUE_TEMPLATE", "_QP_TEMPLATE", "_QP_VALUE_TEMPLATE", "_REC_TEMPLATE", "_VALUE_REC_TEMPLATE",
                  "_QP_REC_TEMPLATE", "_QP_VALUE_REC_TEMPLATE", "_TIME_TEMPLATE", "_MONITOR_TEMPLATE")


def test_the_function_kernel_stays_out_of_the_other_translation_units():
    from casclik_amd.build import CSRC
    for fn in os.listdir(CSRC):
        if fn.endswith((".hpp", ".hip")) and fn != "clik_function.hpp":
            text = jit._code_only(open(os.path.join(CSRC, fn)).read())
            assert "clik_function" not in text and "function_batch" not in text and "FunctionArgs" not in text, fn
    for tmpl in _OLD_TEMPLATES:
        text = getattr(jit, tmpl)
        assert "clik_function.hpp" not in text and "function_batch" not in text and "BatchFn" not in text, tmpl
    assert re.findall(r'#include "([^"]+)"', jit._FUNCTION_TEMPLATE) == ["clik_function.hpp"]
    assert 'extern "C" hipError_t clik_jit_function_batch(' in jit._FUNCTION_TEMPLATE
    text = open(os.path.join(CSRC, "clik_function.hpp")).read()
    assert re.findall(r'#include [<"]([^>"]+)[>"]', text) == ["clik_pinv_kernels.hpp"]
    with open(os.path.join(jit.ROOT, "include", "clik.h")) as f:
        assert "function_batch" not in f.read()                          # no handle state: the C header is not touched


def test_existing_units_keep_their_stamps_and_the_new_one_follows_its_headers_code(tmp_path, monkeypatch):
    from casclik_amd.build import CSRC
    with open(os.path.join(CSRC, "clik_monitor.hpp")) as f:
        monitor = hashlib.sha256(jit._code_only(f.read()).encode()).hexdigest()[:12]
    for tmpl in _OLD_TEMPLATES:
        assert jit._unit_stamp(getattr(jit, tmpl)) == (monitor if tmpl == "_MONITOR_TEMPLATE" else ""), tmpl
    assert jit._unit_stamp("") == ""
    with open(os.path.join(CSRC, "clik_function.hpp")) as f:
        mine = f.read()
    assert jit._unit_stamp(jit._FUNCTION_TEMPLATE) == hashlib.sha256(jit._code_only(mine).encode()).hexdigest()[:12]
    # the shared source stamp does not see the header: a copy of csrc/ with the header edited
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, str(copy), ignore=shutil.ignore_patterns("_obj"))
    stamp = jit._source_stamp()
    tag = jit._cache_tag("", "code", False, [], jit._FUNCTION_TEMPLATE)
    other = jit._cache_tag("{1}", "code", False, [], jit._MONITOR_TEMPLATE)
    monkeypatch.setattr(jit, "CSRC", str(copy))
    assert jit._source_stamp() == stamp and jit._cache_tag("", "code", False, [], jit._FUNCTION_TEMPLATE) == tag
    (copy / "clik_function.hpp").write_text(mine + "\n// a remark\n/* and another */\n")
    assert jit._cache_tag("", "code", False, [], jit._FUNCTION_TEMPLATE) == tag
    (copy / "clik_function.hpp").write_text(mine + "\nnamespace clik { constexpr int kFunctionEdited = 1; }\n")
    assert jit._cache_tag("", "code", False, [], jit._FUNCTION_TEMPLATE) != tag
    assert jit._source_stamp() == stamp and jit._cache_tag("{1}", "code", False, [], jit._MONITOR_TEMPLATE) == other


# ---- request identity ------------------------------------------------------------------------------------------------------
def test_the_request_id_is_a_function_of_the_expression_only():
    ids = {name: jit.function_request_id(fc.get(name)) for name in fc.NAMES}
    assert len(set(ids.values())) == len(fc.NAMES)
    ids["edges"] = jit.function_request_id(fc.get("edges"))
    for name in fc.NAMES + ["edges"]:
        assert jit.function_request_id(fc.make(name)) == ids[name]       # new symbols, new nodes, the same request
        assert ids[name] == jit._request_id("", codegen.emit_function(fc.get(name)), False, [], jit._FUNCTION_TEMPLATE)
        # the instantiations the GPU tests ask for are recorded: build() replays them
        assert os.path.exists(os.path.join(jit.RECORDS, "req_%s.json" % ids[name])), name
        assert os.path.exists(os.path.join(jit.RECORDS, "req_%s.hip" % ids[name])), name


def test_without_a_compiler_and_a_cache_construction_records_and_refuses(tmp_path, monkeypatch):
    monkeypatch.setenv("CLIK_JIT_NO_COMPILER", "1")
    monkeypatch.setenv("CLIK_JIT_RECORD", str(tmp_path / "records"))
    monkeypatch.setattr(jit, "CACHE", str(tmp_path / "empty_cache"))
    q = cs.MX.sym("q", 2)
    fn = cs.Function("unrecorded", [q], [cs.sin(q[0]) * q[1] + 0.125])      # (no committed record holds this code)
    with pytest.raises(NotImplementedError, match="hipcc is missing and nothing is cached"):
        DeviceFunction(fn)
    with pytest.raises(NotImplementedError, match="hipcc is missing and nothing is cached"):
        fn.on_device()
    rid = jit.function_request_id(fn)
    assert sorted(os.listdir(tmp_path / "records")) == ["req_%s.hip" % rid, "req_%s.json" % rid]
    assert (tmp_path / "records" / ("req_%s.hip" % rid)).read_text() == \
        jit._FUNCTION_TEMPLATE % {"init": "", "extern": codegen.emit_function(fn)}
    # the recorded request replays to the tag a construction asks for
    (src, meta, tag), = jit._records(str(tmp_path / "records"))
    assert tag == jit._cache_tag("", codegen.emit_function(fn), False, [], jit._FUNCTION_TEMPLATE)


def test_refusals_that_name_what_is_missing(monkeypatch):
    assert cc.DeviceFunction is DeviceFunction
    monkeypatch.setenv("CLIK_JIT", "0")
    with pytest.raises(NotImplementedError, match="CLIK_JIT=0"):
        DeviceFunction(fc.get("pend"))
    monkeypatch.delenv("CLIK_JIT")
    q, z = cs.MX.sym("q", 2), cs.MX.sym("z", 2)
    with pytest.raises(NotImplementedError, match="symbol 'z' is not an input"):
        DeviceFunction(cs.Function("f", [q], [q[0] + z[1]]))
    # wider than the LDS of a compute unit holds for 256 rows: refused with the limit, never stored lane by lane
    w = cs.MX.sym("w", 81)
    with pytest.raises(NotImplementedError, match=r"163840 bytes per block of 256 rows, which holds 80 entries"):
        DeviceFunction(cs.Function("too_wide", [q], [cs.vertcat(*[q[0] * float(i) for i in range(81)])]))
    with pytest.raises(NotImplementedError, match="80 entries"):
        DeviceFunction(cs.Function("too_wide_in", [w], [w[0]]))
    assert jit.FUNCTION_WAVE_SLOTS == 80 and jit.FUNCTION_LDS_BYTES == 160 * 1024


# ---- argument marshalling --------------------------------------------------------------------------------------------------
R, B = 3, 5
SIZES = [(1, 1), (6, 1), (3, 2)]        # a 1-entry input, a column, a matrix
ACCEPTED = [
    # (shapes of the three arguments, lead, (kind, rec stride, inst stride) of each)
    (((), (B, 6), (B, 3, 2)), (B,), [("shared", 0, 0), ("per_instance", 0, 6), ("per_instance", 0, 6)]),
    (((1,), (6,), (3, 2)), (1,), [("shared", 0, 0), ("shared", 0, 0), ("shared", 0, 0)]),
    (((B,), (B, 6), (3, 2)), (B,), [("per_instance", 0, 1), ("per_instance", 0, 6), ("shared", 0, 0)]),
    (((R,), (R, B, 6), (R, B, 3, 2)), (R, B), [("per_record", 1, 0), ("full", 30, 6), ("full", 30, 6)]),
    (((R, B), (R, B, 6), (R, 1, 3, 2)), (R, B), [("full", 5, 1), ("full", 30, 6), ("per_record", 6, 0)]),
    (((R, 1), (B, 6), (R, B, 3, 2)), (R, B), [("per_record", 1, 0), ("per_instance", 0, 6), ("full", 30, 6)]),
    (((R, 1), (B, 6), (3, 2)), (R, B), [("per_record", 1, 0), ("per_instance", 0, 6), ("shared", 0, 0)]),
    (((R, B, 1), (6,), (3, 2)), (R, B), [("full", 5, 1), ("shared", 0, 0), ("shared", 0, 0)]),
    (((R, 1, 1), (R, 1, 6), (3, 2)), (R, 1), [("per_record", 1, 0), ("per_record", 6, 0), ("shared", 0, 0)]),
    (((), (0, 6), (3, 2)), (0,), [("shared", 0, 0), ("per_instance", 0, 6), ("shared", 0, 0)]),
    (((), (R, 0, 6), (3, 2)), (R, 0), [("shared", 0, 0), ("full", 0, 6), ("shared", 0, 0)]),
]
MALFORMED = [
    ((), (B, 5), (3, 2)),               # a column of the wrong length
    ((), (B, 6), (B, 2, 3)),            # a matrix the wrong way round
    ((), (B, 6), (B + 1, 3, 2)),        # two batch sizes
    ((B + 1,), (B, 6), (3, 2)),         # a 1-entry input with another batch size
    ((B,), (R, B, 6), (3, 2)),          # ... under (R, B) a 1-D one is per record: R entries, not B
    ((), (R, B, 6), (R + 1, B, 3, 2)),  # two record counts
    ((), (R, B, 6), (R, 2, 3, 2)),      # neither B nor 1 instances
    ((), (2, R, B, 6), (3, 2)),         # three dimensions in front
    ((R, B, 2), (R, B, 6), (3, 2)),     # a 1-entry input with a value dimension of 2
    ((R, B, 1, 1), (R, B, 6), (3, 2)),
    ((), (), (3, 2)),                   # a column without its value dimension
]


@pytest.mark.parametrize("shapes, lead, plans", ACCEPTED)
def test_accepted_argument_shapes_resolve_to_the_documented_strides(shapes, lead, plans):
    got_lead, got = plan_arguments(SIZES, shapes)
    assert got_lead == lead and got == plans
    B_ = lead[-1]
    for (kind, rs, is_), (s1, s2) in zip(got, SIZES):
        w = s1 * s2
        assert (rs, is_) == {"shared": (0, 0), "per_record": (w, 0), "per_instance": (0, w), "full": (B_ * w, w)}[kind]


@pytest.mark.parametrize("shapes", MALFORMED)
def test_malformed_argument_shapes_are_refused_by_name(shapes):
    with pytest.raises(ValueError, match=r"argument \d .*has shape \("):
        plan_arguments(SIZES, shapes)
    with pytest.raises(ValueError, match=r"^q of f "):
        plan_arguments(SIZES, shapes, names=["q of f"] * 3)


def test_argument_count_and_output_shapes():
    with pytest.raises(TypeError):
        plan_arguments(SIZES, [(), (6,)])
    assert output_shape((R, B), 1, 1) == (R, B) and output_shape((B,), 3, 1) == (B, 3)
    assert output_shape((R, B), 3, 6) == (R, B, 3, 6) and output_shape((B,), 1, 4) == (B, 1, 4)
