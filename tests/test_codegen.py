"""Generated constraint code (casclik_amd/codegen.py) against the oracle's forward-mode
dual numbers - on the CPU: the generated ``ExternTask<TI>::eval`` bodies are plain C++
once ``__device__`` is defined away, so g++ compiles them and ctypes calls them.
The oracle differentiates the same expression trees with dual numbers
(oracle/clik_oracle.py ExprEvaluator), the generator with symbolic derivatives
(casclik_amd/autodiff.py): two independent routes to ``cs.jacobian``
(reference: casclik/constraints.py:67-73)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import sym as cs, skills
from casclik_amd.lowering import lower_skill, OUT_EXTERN, OUT_AFFINE
from oracle import clik_oracle
from extern_skills import (double_pendulum_skill, mixed_frame_skill, ops_inputs, ops_skill,
                           random_expression as _random_expression)

HARNESS = r"""
#include <cmath>
#define __device__
#define __forceinline__ inline
template <int N> struct Kin { double p[3]; double R[9]; double Jv[3][N]; double Jw[3][N]; double o[3]; double M[9]; double tr; };
template <int TI> struct ExternTask;
static inline void sincos_joint(double x, double& s, double& c) { s = std::sin(x); c = std::cos(x); }
%(extern)s
template <int TI, int N, int M>
static void run(const double* z, const double* ys, const double* tv, const double* kin, double* e, double* J, double* Jt)
{
    double zz[N], ee[M], JJ[M][N], tt[M];
    Kin<N> K;
    for (int i = 0; i < N; ++i) zz[i] = z[i];
    for (int i = 0; i < 3; ++i) K.p[i] = kin[i];
    for (int i = 0; i < 9; ++i) K.R[i] = kin[3 + i];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < N; ++j) { K.Jv[i][j] = kin[12 + i * N + j]; K.Jw[i][j] = kin[12 + 3 * N + i * N + j]; }
    ExternTask<TI>::template eval<N, M>(zz, ys, tv, K, ee, JJ, tt);
    for (int i = 0; i < M; ++i) { e[i] = ee[i]; Jt[i] = tt[i]; for (int j = 0; j < N; ++j) J[i * N + j] = JJ[i][j]; }
}
extern "C" void run_task(int ti, const double* z, const double* ys, const double* tv, const double* kin, double* e, double* J, double* Jt)
{
    switch (ti) {
%(cases)s
    }
}
"""


def _compile(desc, tmp_path):
    cases = "".join("    case %d: run<%d, %d, %d>(z, ys, tv, kin, e, J, Jt); break;\n"
                    % (ti, ti, desc.n_state, desc.tasks[ti]["m"]) for ti in sorted(desc.extern_code))
    _compile.count += 1               # (a fresh name per build: dlopen caches by path)
    src = tmp_path / ("gen%d.cpp" % _compile.count)
    src.write_text(HARNESS % {"extern": desc.extern_source(), "cases": cases})
    so = tmp_path / ("gen%d.so" % _compile.count)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    lib.run_task.argtypes = [C.c_int] + [dp] * 7
    return lib


_compile.count = 0


def _kin_numeric(fk, q, n_state):
    """p, R, Jv, Jw of the tool frame at q (finite differences are not needed: the angular columns
    follow from dR/dq_s R^T = skew(w_s)); Jacobian columns padded to the state width."""
    n = len(q)
    qs = cs.MX.sym("qk", n)
    T = fk["T_fk"](qs)
    spec = cc.SkillSpecification("k", cs.MX.sym("tk"), qs, constraints=[cc.EqualityConstraint("p", T[:3, 3])])
    ev = clik_oracle.ExprEvaluator(spec, 0.0, np.asarray(q, dtype=float)[None, :], None)
    p, _, Jv = ev.vector(T[:3, 3])
    cols, dcols = [], []
    for c in range(3):
        v, _, d = ev.vector(T[:3, c])
        cols.append(v[0])
        dcols.append(d[0])
    R = np.stack(cols, axis=1)                      # R[:, c]
    Jw = np.zeros((3, n))
    for s in range(n):
        dR = np.stack([dcols[c][:, s] for c in range(3)], axis=1)
        W = dR @ R.T
        Jw[:, s] = [W[2, 1], W[0, 2], W[1, 0]]
    pad = np.zeros((3, n_state - n))
    return np.concatenate([p[0], R.reshape(-1), np.hstack([Jv[0], pad]).reshape(-1), np.hstack([Jw, pad]).reshape(-1)])


def _check(spec, desc, lib, t, Z, Y, fk=None, tol=1e-12):
    tv = np.ascontiguousarray(desc.time_terms(t)) if desc.n_tslots else np.zeros(1)
    dp = C.POINTER(C.c_double)
    n = desc.n_state
    ev = clik_oracle.ExprEvaluator(spec, t, Z, Y)
    for ti in sorted(desc.extern_code):
        cn = spec.constraints[ti]
        m = desc.tasks[ti]["m"]
        e_ref, jt_ref, j_ref = ev.vector(cn.expression)
        for b in range(Z.shape[0]):
            kin = _kin_numeric(fk, Z[b, :desc.n_q], n) if fk is not None else np.zeros(12 + 6 * n)
            z = np.ascontiguousarray(Z[b])
            ys = np.ascontiguousarray(Y[b]) if Y is not None else np.zeros(1)
            e, J, Jt = np.zeros(m), np.zeros(m * n), np.zeros(m)
            lib.run_task(ti, *[a.ctypes.data_as(dp) for a in (z, ys, tv, kin, e, J, Jt)])
            scale = 1.0 + np.abs(j_ref[b]).max()
            assert np.abs(e - e_ref[b]).max() <= tol * (1 + np.abs(e_ref[b]).max()), (cn.label, "value")
            assert np.abs(J.reshape(m, n) - j_ref[b]).max() <= tol * scale, (cn.label, "jacobian")
            assert np.abs(Jt - jt_ref[b]).max() <= tol * (1 + np.abs(jt_ref[b]).max()), (cn.label, "time derivative")


def test_double_pendulum_constraints_become_generated_code(tmp_path):
    rng = np.random.default_rng(0)
    for track in (False, True):
        spec = double_pendulum_skill(track)
        d = lower_skill(spec)
        kinds = [t["out_kind"][0] for t in d.tasks]
        assert kinds == [OUT_EXTERN, OUT_AFFINE, OUT_EXTERN, OUT_EXTERN]
        assert d.n_tslots == (4 if track else 0)          # target value and rate, per coordinate
        assert not d.uses_fk and not d.joints
        lib = _compile(d, tmp_path)
        _check(spec, d, lib, 1.7, rng.uniform(-3.0, 3.0, size=(16, 2)), None)


def test_generated_code_with_tool_frame_time_input_and_virtual_terms(tmp_path):
    fk = skills.iiwa()
    spec = mixed_frame_skill(fk)
    d = lower_skill(spec)
    assert [tk["out_kind"][0] for tk in d.tasks] == [OUT_EXTERN, OUT_EXTERN, OUT_AFFINE]
    assert d.uses_fk and len(d.joints) > 0
    lib = _compile(d, tmp_path)
    rng = np.random.default_rng(1)
    Z = np.concatenate([rng.uniform(-1.5, 1.5, size=(8, 7)), rng.uniform(-1, 1, size=(8, 1))], axis=1)
    _check(spec, d, lib, 0.8, Z, rng.uniform(-1, 1, size=(8, 3)), fk=fk, tol=1e-11)


def test_generated_code_of_the_operations_no_other_skill_emits(tmp_path):
    """tan, log, every form of pow, sign, fabs, fmax, fmin, the inverse trigonometric functions, tanh and if_else on
    `<=` and on a logic_and: the generated bodies against the oracle's dual numbers, away from every switch"""
    spec = ops_skill()
    d = lower_skill(spec)
    assert [tk["out_kind"][0] for tk in d.tasks] == [OUT_EXTERN, OUT_EXTERN]
    assert d.n_tslots > 0 and not d.uses_fk and not d.joints         # (sin(0.5 t), 0.3 t and their rates)
    assert sorted(int(tk["m"]) for tk in d.tasks) == [4, 6] and d.n_state == 4
    text = d.extern_source()
    for call in ("tan(", "log(", "pow(", "__builtin_powi(", "sqrt(", "asin(", "acos(", "atan(", "atan2(", "tanh(", "fabs(",
                 "fmax(", "fmin(", " <= ", " < ", " != ", "> 0.0) - ("):
        assert call in text, call
    lib = _compile(d, tmp_path)
    for t in (0.0, 1.3):
        Q, Y = ops_inputs(24, 31, t=t)
        _check(spec, d, lib, t, Q, Y, tol=1e-11)


def test_what_generated_code_cannot_express_is_refused():
    fk = skills.iiwa()
    t, q, dq, y = cs.MX.sym("t"), cs.MX.sym("q", 7), cs.MX.sym("dq", 7), cs.MX.sym("y", 4)
    T = fk["T_fk"](q)
    with pytest.raises(NotImplementedError, match="velocity variables"):
        lower_skill(cc.SkillSpecification("s", t, q, dq, constraints=[cc.EqualityConstraint("v", dq[0] * q[0])]))
    # more constraints than a shape-specialised kernel carries: generated code has nowhere to live
    many = [cc.EqualityConstraint("a%d" % i, q[i % 7] + 0.1 * i, priority=i) for i in range(8)]
    many.append(cc.EqualityConstraint("prod", q[0] * q[1], priority=9))
    with pytest.raises(NotImplementedError, match="generated device code"):
        lower_skill(cc.SkillSpecification("s", t, q, constraints=many))


def two_frames_skill(iiwa, ur5):
    """what the device path keeps as atoms (one chain, one orientation target) and what it writes out: a second chain
    (another robot's tool in the same skill), the same chain on other arguments, a second orientation target, an
    orientation error inside a product"""
    t, q, p2, y = cs.MX.sym("t"), cs.MX.sym("q", 7), cs.MX.sym("p2", 2), cs.MX.sym("y", 8)
    T = iiwa["T_fk"](q)                                   # the primary chain instance
    qb = cs.vertcat(q[0], q[1], q[2], q[3], q[4], q[5])
    Tb = ur5["T_fk"](qb)                                  # a second chain driven by six of the joints
    Tc = iiwa["T_fk"](cs.vertcat(q[6], q[5], q[4], q[3], q[2], q[1], q[0]))      # the first chain, other arguments
    e1 = cs.orientation_error(T[:3, :3], y[:4])           # the primary orientation target
    e2 = cs.orientation_error(T[:3, :3], y[4:8])          # a second target
    e3 = cs.orientation_error(Tb[:3, :3], cs.vertcat(0.0, 0.0, 0.6, 0.8))        # of the second chain
    cn = [cc.EqualityConstraint("pose", cs.vertcat(T[:3, 3] - 0.3, e1), gain=2.0, priority=0, constraint_type="soft"),
          cc.EqualityConstraint("second_tool", Tb[:3, 3] - cs.vertcat(0.2, 0.1, 0.4), gain=1.0, priority=1,
                                constraint_type="soft"),
          cc.EqualityConstraint("second_target", cs.vertcat(e2, e3[2]), gain=1.5, priority=2, constraint_type="soft"),
          cc.SetConstraint("mixed", cs.vertcat(e1[0] * q[0] + Tc[2, 3], cs.dot(Tb[:3, 3] - T[:3, 3], Tb[:3, 3] - T[:3, 3])),
                           set_min=cs.vertcat(-0.5, 0.01), set_max=cs.vertcat(0.5, 4.0), gain=1.0, priority=3,
                           constraint_type="soft")]
    return cc.SkillSpecification("two_frames", t, q, input_var=y, constraints=cn)


def test_second_chain_and_second_orientation_target_are_written_out(tmp_path):
    """casclik takes any expression (constraints.py:21-24); the kernels keep one chain and one orientation target as
    atoms, expand.py writes the others out in sin / cos, and the generated code equals the oracle's dual numbers
    evaluated on the ORIGINAL atoms (an independent route: oracle/clik_oracle.py differentiates every chain by its
    own forward-mode kinematics)."""
    iiwa, ur5 = skills.iiwa(), skills.ur5()
    spec = two_frames_skill(iiwa, ur5)
    d = lower_skill(spec)
    assert [tk["out_kind"][0] for tk in d.tasks] == [OUT_AFFINE, OUT_EXTERN, OUT_EXTERN, OUT_EXTERN]
    assert d.quat_src == 2 and list(d.quat_yi) == [0, 1, 2, 3] and len(d.joints) == len(iiwa["chain"].joints)
    lib = _compile(d, tmp_path)
    rng = np.random.default_rng(5)
    Z = rng.uniform(-1.5, 1.5, size=(6, 7))
    Y = rng.normal(size=(6, 8))
    Y[:, :4] /= np.linalg.norm(Y[:, :4], axis=1, keepdims=True)
    Y[:, 4:] /= np.linalg.norm(Y[:, 4:], axis=1, keepdims=True)
    _check(spec, d, lib, 0.3, Z, Y, fk=iiwa, tol=1e-11)


def test_random_expression_trees(tmp_path):
    """Property test of the generator: random expression trees over robot, virtual, input and time
    variables (and tool-frame entries), generated code against the oracle's dual numbers."""
    fk = skills.ur5()
    rng = np.random.default_rng(2024)
    for trial in range(24):
        t, q, x, y = cs.MX.sym("t"), cs.MX.sym("q", 6), cs.MX.sym("x", 2), cs.MX.sym("y", 2)
        T = fk["T_fk"](q)
        leaves = [q[i] for i in range(6)] + [x[0], x[1], y[0], y[1], t, cs.sin(0.3 * t)]
        if trial % 2 == 0:
            leaves += [T[0, 3], T[1, 3], T[2, 3], T[0, 0], T[1, 2], T[2, 1]]
        rows = []
        while len(rows) < 3:
            e = _random_expression(rng, leaves, 4, angles=trial >= 16)       # (the last eight with atan2 / asin / ... / fmin)
            if isinstance(e, cs.MX) and not e.is_constant():
                rows.append(e)
        cn = [cc.EqualityConstraint("rand", cs.vertcat(*rows), gain=1.0),
              cc.EqualityConstraint("anchor", q - 0.1, priority=5)]
        spec = cc.SkillSpecification("rand%d" % trial, t, q, virtual_var=x, input_var=y, constraints=cn)
        d = lower_skill(spec)
        if 0 not in d.extern_code:
            continue                                   # (the draw happened to be affine)
        lib = _compile(d, tmp_path)
        Z = np.concatenate([rng.uniform(-1.2, 1.2, size=(6, 6)), rng.uniform(-1, 1, size=(6, 2))], axis=1)
        _check(spec, d, lib, 0.9, Z, rng.uniform(-1, 1, size=(6, 2)), fk=fk if d.uses_fk else None, tol=1e-10)
