"""GPU: ``converge_batch`` - a rollout whose instances stop on their own (clik_converge.hpp) - and ``ik_batch`` on top of
it, both controllers.  Yardsticks: the records of the recording rollout (``rollout_batch(..., record_every=1)``, which
never stops) with the oracle's constraint values and the stop rule applied in numpy; a host loop on the oracle alone; and
the properties the rule states (every status, the edges, the same bits in every batch)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import jit, skills
from casclik_amd import sym as cs
from casclik_amd.controllers.base_controller import select_seeds

import converge_cases as K
import host_loops as H
from test_gpu_constraint_summary import TOL
from test_gpu_rollout_record import Q_TOL, V_TOL

pytestmark = pytest.mark.gpu

DT = K.DT
_made, _refs = {}, {}


def _ctrl(name, iiwa_fk, ur5_fk):
    if name not in _made:
        spec, ctrl, qp = K.make(name, iiwa_fk, ur5_fk)
        ctrl.setup_problem_functions()
        ctrl.setup_solver()
        _made[name] = (spec, ctrl, qp)
    return _made[name]


def _waves(ctrl):
    """waves per block of the controller's converging rollout, as the loaded unit states them"""
    ctrl._require_kernel("converge")
    info = jit._load(os.path.join(jit.CACHE, "clik_shape_%s.so" % ctrl._kernels["converge"])).clik_jit_converge_info
    info.restype, info.argtypes = C.c_longlong, [C.c_int]
    return int(info(4))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _quiet_nan(a):
    """every component a quiet NaN, by bits"""
    hi = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) >> np.uint64(32)
    return bool(((hi & np.uint64(0x7ff80000)) == np.uint64(0x7ff80000)).all())


def _unpack(res, qp, has_x):
    """converge_batch's result as a dict"""
    if has_x:
        q, x, dq, dx, flag, info = res
    else:
        (q, dq, flag, info), x, dx = res, None, None
    return dict(q=q, x=x, dq=dq, dx=dx, flag=flag, **info)


def _reference(name, iiwa_fk, ur5_fk):
    """the recording rollout of the case over max_ticks ticks at K.B_ALL instances, the oracle's values at its max_ticks +
    1 states and the stop rule on them - computed once, never changed"""
    if name in _refs:
        return _refs[name]
    spec, ctrl, qp = _ctrl(name, iiwa_fk, ur5_fk)
    case = K.CASES[name]
    n = case["max_ticks"]
    Q, X, Y = K.inputs(name, iiwa_fk)
    rec = ctrl.rollout_batch(np.zeros(n), Q, input_var=Y, virtual_var=X, dt=DT, record_every=1)[-1]
    states = np.concatenate([Q[None], rec["q"]])
    xs = None if X is None else np.concatenate([X[None], rec["x"]])
    orc = K.oracle_values(spec, 0.0, states, xs, Y)
    tol = K.tolerances(spec, case["tol"])
    ticks, status, residual, sure = K.stop_rule(*orc, tol, n)
    # the inputs are worth the run: the instances stop at many different ticks, some never
    assert len(np.unique(ticks)) >= 8 and (status == 0).any() and (status == 1).any(), np.bincount(ticks)
    assert (~sure).sum() <= 0.01 * sure.size
    assert np.abs(rec["dq"]).max() < 20.0       # (no trajectory runs through a singularity: a plain contraction each)
    if qp:
        assert (rec["status"] == 0).all()
    _refs[name] = dict(Q=Q, X=X, Y=Y, tol=tol, n=n, rec=rec, states=states, xs=xs, dist=K.distances(*orc), ticks=ticks,
                       status=status, sure=sure)
    return _refs[name]


# ---- 1: against the recording rollout and the oracle's values -----------------------------------------------------------
@pytest.mark.parametrize("name", ["pose", "stack", "qp", "virtual"])
def test_stops_where_the_recorded_rollout_meets_the_tolerance(iiwa_fk, ur5_fk, name):
    spec, ctrl, qp = _ctrl(name, iiwa_fk, ur5_fk)
    ref = _reference(name, iiwa_fk, ur5_fk)
    rec, n = ref["rec"], ref["n"]
    left_out = [0, 0]
    batches = sorted({1, 63, 64, 65, 64 * _waves(ctrl) + 1})
    assert batches[-1] <= K.B_ALL
    for B in batches:
        cut = lambda A: None if A is None else np.ascontiguousarray(A[:B])          # noqa: E731
        got = _unpack(ctrl.converge_batch(cut(ref["Q"]), cut(ref["Y"]), tol=ref["tol"], max_ticks=n, dt=DT,
                                          virtual_var=cut(ref["X"])), qp, ref["X"] is not None)
        assert got["ticks"].dtype == np.int32 and got["status"].dtype == np.int32 and got["ticks"].shape == (B,)
        assert got["residual"].shape == (B, ref["tol"].size) and got["residual"].dtype == np.float64
        sure = ref["sure"][:B]
        left_out[0] += int((~sure).sum())
        left_out[1] += B
        assert np.array_equal(got["ticks"][sure], ref["ticks"][:B][sure]), (name, B)
        assert np.array_equal(got["status"][sure], ref["status"][:B][sure]), (name, B)
        assert set(np.unique(got["status"])) <= {0, 1}
        # the floats at the tick the launch itself stopped at (the reference's own, wherever the oracle decides it)
        r, b = got["ticks"].astype(int), np.arange(B)
        assert (r >= 0).all() and (r <= n).all()
        last = np.maximum(r - 1, 0)
        moved = (r > 0)[:, None]
        eq = np.abs(got["q"] - ref["states"][r, b]).max()
        ev = np.abs(got["dq"] - np.where(moved, rec["dq"][last, b], 0.0)).max()
        # (the residual is that of the RETURNED state: the oracle's values there, not at the record's state, which may
        # differ from it by Q_TOL - the rows q - q_mid of the stack differ by as much)
        at = K.oracle_values(spec, 0.0, got["q"][None], None if got["x"] is None else got["x"][None], cut(ref["Y"]))
        er = np.abs(got["residual"] - K.distances(*at)[0]).max()
        print("%s B=%d: |q| %.3e |dq| %.3e |residual| %.3e, ticks %d .. %d" % (name, B, eq, ev, er, r.min(), r.max()))
        assert eq < Q_TOL and ev < V_TOL and er < TOL
        flag = rec["status" if qp else "mode"]
        assert np.array_equal(got["flag"], np.where(r > 0, flag[last, b], 0 if qp else -1))
        if ref["X"] is not None:
            assert np.abs(got["x"] - ref["xs"][r, b]).max() < Q_TOL
            assert np.abs(got["dx"] - np.where(moved, rec["dx"][last, b], 0.0)).max() < V_TOL
    print("%s: %d of %d instances left out of the integer comparisons (oracle margin below 4e-12)" % (name, *left_out))
    assert left_out[0] <= 0.01 * left_out[1], left_out


# ---- 2: against a host loop that involves no device code ------------------------------------------------------------------
def test_a_host_loop_on_the_oracle_stops_at_the_same_ticks(iiwa_fk, ur5_fk):
    """The oracle's state drifts from the device's by up to Q_TOL, so its constraint values - and the launch's residual -
    by up to ||J||_inf Q_TOL < 1e-8 (seven joints, a reach below 1.3 m); an instance that comes that close to a tolerance
    is left out of the integer comparisons."""
    spec, ctrl, _ = _ctrl("pose", iiwa_fk, ur5_fk)
    case = K.CASES["pose"]
    B, n, margin = 65, case["max_ticks"], 1e-8
    Q, _, Y = K.inputs("pose", iiwa_fk, B, seed=4)
    tol = K.tolerances(spec, case["tol"])
    hq, hdq, hticks, hstatus, hres, sure = H.converge_loop(spec, ctrl.options, Q, Y, tol, n, margin=margin)
    assert len(np.unique(hticks)) >= 8 and (hstatus == 0).any() and (hstatus == 1).any()
    got = _unpack(ctrl.converge_batch(Q, Y, tol=tol, max_ticks=n, dt=DT), False, False)
    print("host loop: %d of %d left out; |q| %.3e |dq| %.3e |residual| %.3e" % (
        (~sure).sum(), B, np.abs(got["q"] - hq)[sure].max(), np.abs(got["dq"] - hdq)[sure].max(),
        np.abs(got["residual"] - hres)[sure].max()))
    assert (~sure).sum() <= 0.01 * B
    assert np.array_equal(got["ticks"][sure], hticks[sure]) and np.array_equal(got["status"][sure], hstatus[sure])
    assert np.abs(got["q"] - hq)[sure].max() < Q_TOL and np.abs(got["dq"] - hdq)[sure].max() < V_TOL
    assert np.abs(got["residual"] - hres)[sure].max() < margin


# ---- 3: every status ------------------------------------------------------------------------------------------------------
def _blocked_skill():
    """a joint asked to go to 1.0 and held at 0.5 by its limit: a target that cannot be reached"""
    t, q = cs.MX.sym("t"), cs.MX.sym("q", 2)
    cons = [cc.SetConstraint("limit", q[0], set_min=-0.5, set_max=0.5, gain=10.0, priority=0),
            cc.EqualityConstraint("goal", q - np.array([1.0, 0.25]), gain=10.0, constraint_type="soft", priority=1)]
    return cc.SkillSpecification("blocked", t, q, constraints=cons)


def test_a_target_that_cannot_be_reached_stalls_or_runs_out_of_ticks():
    ctrl = cc.PseudoInverseController(skill_spec=_blocked_skill())
    ctrl.setup_problem_functions()
    ctrl.setup_solver()
    rows = ctrl.constraint_rows()
    tol = np.zeros(3)
    tol[rows["limit"]], tol[rows["goal"]] = 1e-6, 1e-6
    Q = np.random.default_rng(1).uniform(-0.3, 0.3, size=(65, 2))
    q, dq, mode, info = ctrl.converge_batch(Q, tol=tol, max_ticks=120, dt=DT, min_step=1e-6)
    print("stalled after", np.bincount(info["ticks"]))
    assert (info["status"] == 2).all() and (info["ticks"] > 0).all() and (info["ticks"] < 120).all()
    # (the free joint has arrived; the blocked one stands at or beyond its limit, as far from its goal as it ever gets)
    assert np.abs(q[:, 1] - 0.25).max() < 1e-3 and (q[:, 0] >= 0.5 - 1e-9).all() and (q[:, 0] < 1.0).all()
    assert (info["residual"][:, rows["goal"]].max(axis=1) > 0.2).all()
    q1, _, _, info1 = ctrl.converge_batch(Q, tol=tol, max_ticks=120, dt=DT)
    assert (info1["status"] == 1).all() and (info1["ticks"] == 120).all()
    # a stalled instance has not moved since its last integrated tick: the run without min_step passes through that state
    q2, _, _, info2 = ctrl.converge_batch(Q, tol=tol, max_ticks=int(info["ticks"].max()), dt=DT)
    same = info["ticks"] == info["ticks"].max()
    assert same.any() and _same_bits(q[same], q2[same])


def test_an_infeasible_qp_stops_the_instance_where_it_is():
    """the skill of tests/test_gpu_qp.py::test_qp_infeasible_is_reported: two hard rows that contradict each other"""
    t, q = cs.MX.sym("t"), cs.MX.sym("q", 7)
    cons = [cc.VelocitySetConstraint("a", q[0], set_min=1.0, set_max=2.0, priority=0),
            cc.VelocitySetConstraint("b", q[0], set_min=-2.0, set_max=-1.0, priority=1)]
    ctrl = cc.ReactiveQPController(skill_spec=cc.SkillSpecification("bad", t, q, constraints=cons))
    ctrl.setup_problem_functions()
    ctrl.setup_solver()
    Q = np.full((3, 7), 0.5)
    assert (ctrl.solve_batch(0.0, Q)[3] == 2).all()
    q, dq, status, info = ctrl.converge_batch(Q, tol=1e-6, max_ticks=5, dt=DT)
    assert (info["status"] == 3).all() and (info["ticks"] == 0).all() and (status == 2).all()
    assert _same_bits(q, Q) and (dq == 0.0).all() and np.abs(info["residual"] - 0.5).max() < TOL
    # a row that is within its tolerance at once never reaches the solve
    assert (ctrl.converge_batch(Q, tol=np.inf, max_ticks=5, dt=DT)[3]["status"] == 0).all()


@pytest.mark.parametrize("name", ["pose", "qp"])
@pytest.mark.parametrize("where", ["q", "target"])
def test_a_nan_in_one_instance_marks_that_instance_and_no_other(iiwa_fk, ur5_fk, name, where):
    spec, ctrl, qp = _ctrl(name, iiwa_fk, ur5_fk)
    ref = _reference(name, iiwa_fk, ur5_fk)
    B, bad = 65, 40
    Q, Y = ref["Q"][:B].copy(), ref["Y"][:B].copy()
    call = lambda q, y: _unpack(ctrl.converge_batch(q, y, tol=ref["tol"], max_ticks=ref["n"], dt=DT), qp, False)    # noqa: E731
    clean = call(Q, Y)
    if where == "q":
        Q[bad, 3] = np.nan
    else:
        Y[bad, 1] = np.nan
    poisoned = call(Q, Y)
    assert poisoned["status"][bad] == 4 and poisoned["ticks"][bad] == 0
    for key in ("q", "dq", "residual"):
        assert _quiet_nan(poisoned[key][bad]), (key, poisoned[key][bad])
    keep = np.arange(B) != bad
    for key in ("q", "dq", "flag", "ticks", "status", "residual"):
        assert _same_bits(np.ascontiguousarray(poisoned[key][keep]), np.ascontiguousarray(clean[key][keep])), key
        assert not np.isnan(clean[key].astype(float)).any(), key


# ---- 4: edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "qp"])
def test_edges_of_the_rule(iiwa_fk, ur5_fk, name):
    spec, ctrl, qp = _ctrl(name, iiwa_fk, ur5_fk)
    ref = _reference(name, iiwa_fk, ur5_fk)
    B = 65
    Q, Y, tol = ref["Q"][:B], ref["Y"][:B], ref["tol"]
    # no row can block: nothing runs
    q, dq, flag, info = ctrl.converge_batch(Q, Y, tol=np.inf, max_ticks=9, dt=DT)
    assert (info["ticks"] == 0).all() and (info["status"] == 0).all() and _same_bits(q, Q) and (dq == 0.0).all()
    # no tick allowed: the residual is that of the input
    q, dq, flag, info = ctrl.converge_batch(Q, Y, tol=tol, max_ticks=0, dt=DT)
    e = ctrl.constraint_values_batch(0.0, Q, input_var=Y)
    _, lo, hi, is_set = K.oracle_values(spec, 0.0, Q[None], None, Y)
    want = K.distances(e, lo[0], hi[0], is_set)
    assert (info["ticks"] == 0).all() and _same_bits(q, Q) and np.abs(info["residual"] - want).max() < TOL
    assert np.array_equal(info["status"], np.where((want <= tol).all(axis=1), 0, 1))
    # a row that never meets its tolerance blocks until its tolerance is inf
    rows = ctrl.constraint_rows()
    hard = tol.copy()
    hard[rows["joint_centering" if name == "stack" else "joint_speed_limits"]] = 1e-9
    blocked = ctrl.converge_batch(Q, Y, tol=hard, max_ticks=ref["n"], dt=DT)[3]
    free = ctrl.converge_batch(Q, Y, tol=tol, max_ticks=ref["n"], dt=DT)[3]
    assert (blocked["status"] == 1).all() and (blocked["ticks"] == ref["n"]).all()
    assert (free["status"] == 0).sum() > B // 2


# ---- 5: the same bits on every call and in every batch ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "qp"])
def test_same_bits_every_call_alone_and_in_a_batch(iiwa_fk, ur5_fk, name):
    spec, ctrl, qp = _ctrl(name, iiwa_fk, ur5_fk)
    ref = _reference(name, iiwa_fk, ur5_fk)
    B = 130
    Q, Y = ref["Q"][:B], ref["Y"][:B]
    call = lambda q, y: _unpack(ctrl.converge_batch(q, y, tol=ref["tol"], max_ticks=ref["n"], dt=DT), qp, False)    # noqa: E731
    one, two = call(Q, Y), call(Q, Y)
    keys = ("q", "dq", "flag", "ticks", "status", "residual")
    for key in keys:
        assert _same_bits(one[key], two[key]), key
    for b in (0, 1, 17, 62, 63, 64, 65, 100, 127, 128, 129):
        alone = call(Q[b:b + 1], Y[b:b + 1])
        for key in keys:
            assert _same_bits(np.ascontiguousarray(one[key][b:b + 1]), alone[key]), (key, b)


# ---- 6: ik_batch ----------------------------------------------------------------------------------------------------------
def test_ik_batch_is_select_seeds_on_one_launch(iiwa_fk, ur5_fk):
    import torch
    spec, ctrl, _ = _ctrl("pose", iiwa_fk, ur5_fk)
    Y, seeds, tol, n = K.ik_inputs(iiwa_fk)
    T, S = Y.shape[0], seeds.shape[0]
    assert (T, S) == (5, 13)
    kw = dict(tol=tol, max_ticks=n, dt=DT)
    q, info = ctrl.ik_batch(Y, seeds, **kw)
    Q0 = np.broadcast_to(seeds[None], (T, S, 7)).reshape(T * S, 7)
    Ys = np.repeat(Y, S, axis=0)
    pq, _, _, pinfo = ctrl.converge_batch(Q0, Ys, **kw)
    ok = (pinfo["status"] == 0).reshape(T, S)
    print("targets reached from", ok.sum(axis=1), "of", S, "seeds")
    assert ((ok.sum(axis=1) > 0) & (ok.sum(axis=1) < S)).any()
    full_tol = K.tolerances(spec, {"tool_pose": tol})
    pick = select_seeds(*(torch.from_numpy(pinfo[k]) for k in ("ticks", "status", "residual")), full_tol, S).numpy()
    assert np.array_equal(pick, K.select_seeds_loop(pinfo["ticks"], pinfo["status"], pinfo["residual"], full_tol, S))
    at = np.arange(T) * S + pick
    assert info["seed"].dtype == np.int32 and np.array_equal(info["seed"], pick)
    assert _same_bits(q, pq[at])
    for key in ("ticks", "status", "residual"):
        assert _same_bits(info[key], np.ascontiguousarray(pinfo[key][at])), key
    # seeds per target, device tensors in and out
    dev = ctrl._device
    seeds3 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(seeds[None], (T, S, 7)))).to(dev)
    qd, infod = ctrl.ik_batch(torch.from_numpy(Y).to(dev), seeds3, **kw)
    assert isinstance(qd, torch.Tensor) and qd.device == dev and _same_bits(qd.cpu().numpy(), q)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in infod.values())
    assert np.array_equal(infod["seed"].cpu().numpy(), pick)


# ---- 7: containers and refusals -------------------------------------------------------------------------------------------
def test_containers_and_refusals(iiwa_fk, ur5_fk, monkeypatch):
    import torch
    spec, ctrl, _ = _ctrl("stack", iiwa_fk, ur5_fk)
    ref = _reference("stack", iiwa_fk, ur5_fk)
    dev = ctrl._device
    Q, Y, tol = ref["Q"][:65], ref["Y"][:65], ref["tol"]
    host = ctrl.converge_batch(Q, Y, tol=tol, max_ticks=5, dt=DT)
    res = ctrl.converge_batch(torch.from_numpy(Q).to(dev), torch.from_numpy(Y).to(dev), tol=torch.from_numpy(tol),
                              max_ticks=5, dt=DT)
    assert len(host) == len(res) == 4
    for h, d in zip(host[:3], res[:3]):
        assert isinstance(h, np.ndarray) and isinstance(d, torch.Tensor) and d.device == dev and _same_bits(h, d.cpu().numpy())
    for key, h in host[3].items():
        assert isinstance(h, np.ndarray) and _same_bits(h, res[3][key].cpu().numpy()), key
    for bad in (-1e-3, float("nan"), np.full(tol.size - 1, 1e-3), np.where(np.arange(tol.size) == 3, -1.0, 1e-3)):
        with pytest.raises(ValueError, match="tol"):
            ctrl.converge_batch(Q, Y, tol=bad)
    with pytest.raises(ValueError, match="max_ticks"):
        ctrl.converge_batch(Q, Y, max_ticks=-1)
    with pytest.raises(ValueError, match="targets are fixed"):
        ctrl.converge_batch(Q, np.broadcast_to(Y[None], (3,) + Y.shape))
    # a pinv skill with more SetConstraints than a recording rollout is instantiated for (six: the comparison notebook's)
    from extern_skills import dual_quaternion_skill
    many = cc.PseudoInverseController(skill_spec=dual_quaternion_skill(ur5_fk, "Q_dist2", for_pinv=True))
    many.setup_problem_functions()
    many.setup_solver()
    assert sum(1 for t in many.descriptor.tasks if t["cls"] == 1) > jit.REC_MAX_SETS
    with pytest.raises(NotImplementedError, match="instantiated"):
        many.converge_batch(np.zeros((3, 6)), tol=1e-3, max_ticks=2)
    # a handle served only by the built-in dynamic kernels
    monkeypatch.setenv("CLIK_FORCE_DYNAMIC", "1")
    for dyn in (cc.PseudoInverseController(skill_spec=skills.stack_skill(iiwa_fk), options=dict(skills.STACK_OPTIONS)),
                cc.ReactiveQPController(skill_spec=skills.qp_skill(iiwa_fk))):
        dyn.setup_problem_functions()
        dyn.setup_solver()
        with pytest.raises(NotImplementedError, match="instantiated"):
            dyn.converge_batch(Q, Y, tol=1e-3, max_ticks=2)


_NO_JIT = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import casclik_amd as cc
from casclik_amd import skills
fk = skills.iiwa()
ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
ctrl.setup_problem_functions()
Q, Y = skills.synthetic_inputs(fk, 5, seed=0)
try:
    ctrl.converge_batch(Q, Y, tol=1e-3, max_ticks=2)
except NotImplementedError as exc:
    assert "instantiated" in str(exc), exc
    print("REFUSED")
"""


def test_without_an_instantiated_kernel_the_call_is_refused():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CLIK_JIT="0")
    out = subprocess.run([sys.executable, "-c", _NO_JIT % (root, os.path.join(root, "tests"))], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0 and b"REFUSED" in out.stdout, out.stdout.decode()[-2000:]
