"""GPU: rollouts that record their trajectory (``record_every``) and follow one target per tick (``input_var
[n_ticks, B, n_y]``), both controllers, every instantiated rollout kernel.  The yardstick is the host loop of all
rollout tests (tests/host_loops.py::rollout_loop: ``solve_batch`` -> ``np.clip`` -> ``q += dq * dt``) with the
tolerances of tests/test_gpu_pinv.py::test_rollout_matches_host_loop and tests/test_gpu_qp.py::
test_qp_rollout_matches_host_loop: |q| < 1e-9, |dq| and |slack| < 1e-7, modes equal, status 0."""
import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import skills
from casclik_amd import sym as cs

from host_loops import controller_tick, rollout_loop
from test_gpu_branches import _path_following_skill
from time_skills import UR5_HOME

pytestmark = pytest.mark.gpu

Q_TOL, V_TOL = 1e-9, 1e-7
N_TICKS = 11


def _point_skill(fk):
    """the five-set skill of tests/test_gpu_pinv.py::test_skills_without_aot_shape (32 modes, image-reading lane kernel)"""
    t, q = cs.MX.sym("t"), cs.MX.sym("q", 6)
    p = fk["T_fk"](q)[:3, 3]
    lo, hi = np.array(fk["lower"]), np.array(fk["upper"])
    cons = [cc.EqualityConstraint("dist", cs.norm_2(np.array([0.5, 0.5, 0.5]) - p), gain=50.0,
                                  constraint_type="soft", priority=6)]
    for i in range(5):
        cons.append(cc.SetConstraint("limit_q_%d" % i, q[i], set_min=0.3 * lo[i], set_max=0.3 * hi[i], priority=i))
    return cc.SkillSpecification("point", t, q, constraints=cons)


# family -> (controller class, dt, max_speed, variant a rollout of 100 instances must be served by or None)
FAMILIES = ["stack_values", "stack_image", "pose", "point", "virtual", "qp_box", "qp_walls"]
_made = {}


def _family(name, iiwa_fk, ur5_fk, monkeypatch):
    """(controller, is_qp, dt, max_speed, inputs(B) -> (Q, X, Y)) of a kernel family, made once per session"""
    if name in _made:
        return _made[name]
    qp = name.startswith("qp")
    if name == "stack_image":
        monkeypatch.setenv("CLIK_JIT_VALUES", "0")
    if name in ("stack_values", "stack_image"):
        spec, opts, fk, dt, vmax = skills.stack_skill(iiwa_fk), dict(skills.STACK_OPTIONS), iiwa_fk, 0.008, np.pi / 5
    elif name == "pose":
        spec, opts, fk, dt, vmax = skills.pose_skill(iiwa_fk), None, iiwa_fk, 0.008, np.pi / 5
    elif name == "qp_box":
        spec, opts, fk, dt, vmax = skills.qp_skill(iiwa_fk), None, iiwa_fk, 0.008, 1.0
    elif name == "point":
        spec, opts, fk, dt, vmax = _point_skill(ur5_fk), None, ur5_fk, 0.008, 0.4
    elif name == "virtual":
        spec, opts, fk, dt, vmax = _path_following_skill(ur5_fk), None, ur5_fk, 0.01, 0.4
    else:
        from extern_skills import moe_box_skill
        spec, _ = moe_box_skill(ur5_fk, soft_walls=False)       # (hard walls: general rows, the image-reading QP rollout)
        opts, fk, dt, vmax = None, ur5_fk, 0.008, 0.4
    ctrl = (cc.ReactiveQPController if qp else cc.PseudoInverseController)(skill_spec=spec, options=opts)
    ctrl.setup_problem_functions()
    ctrl.setup_solver()

    def inputs(B):
        if fk is iiwa_fk:
            Q, Y = skills.synthetic_inputs(iiwa_fk, B, seed=13, distribution="mixed")
            return Q, None, Y
        rng = np.random.default_rng(5)
        if name == "point":
            lo, hi = np.array(fk["lower"]), np.array(fk["upper"])
            return rng.uniform(0.35 * lo, 0.35 * hi, size=(B, 6)), None, None
        if name == "virtual":
            return UR5_HOME + rng.normal(scale=0.2, size=(B, 6)), rng.uniform(0.0, 0.9, size=(B, 1)), None
        return UR5_HOME + rng.normal(scale=0.02, size=(B, 6)), None, None      # (well inside the walls: status 0)

    _made[name] = (ctrl, qp, dt, vmax, inputs)
    return _made[name]


def _check_records(rec, host, k, qp, label):
    """entry r of every record against the host loop's tick (r + 1) * k (counted from 1)"""
    R = len(host) // k
    flag_name = "status" if qp else "mode"
    assert rec["q"].shape[0] == R and rec["dq"].shape[0] == R and rec[flag_name].shape[0] == R
    for r in range(R):
        h = host[(r + 1) * k - 1]
        eq, ev = np.abs(rec["q"][r] - h["q"]).max(), np.abs(rec["dq"][r] - h["dq"]).max()
        print("%s k=%d record %d: |q| %.3e |dq| %.3e" % (label, k, r, eq, ev))
        assert eq < Q_TOL and ev < V_TOL
        assert np.array_equal(rec[flag_name][r], h["flag"])
        if qp:
            assert (rec["status"][r] == 0).all()
        if h["x"] is not None:
            assert np.abs(rec["x"][r] - h["x"]).max() < Q_TOL and np.abs(rec["dx"][r] - h["dx"]).max() < V_TOL
        else:
            assert "x" not in rec and "dx" not in rec
        if h["slack"] is not None and h["slack"].size:
            es = np.abs(rec["slack"][r] - h["slack"]).max()
            print("%s k=%d record %d: |slack| %.3e" % (label, k, r, es))
            assert es < V_TOL
        else:
            assert "slack" not in rec


@pytest.mark.parametrize("B", [100, 1])
@pytest.mark.parametrize("family", FAMILIES)
def test_records_equal_the_host_loop_at_every_recorded_tick(iiwa_fk, ur5_fk, monkeypatch, family, B):
    """B = 100: a partial wave and a partial 64-instance team block, two blocks; B = 1.  Eleven ticks with a record every
    tick, every fourth (two records, three unrecorded trailing ticks) and every twelfth (no record: the final results
    are those of the unrecorded call)."""
    ctrl, qp, dt, vmax, inputs = _family(family, iiwa_fk, ur5_fk, monkeypatch)
    Q, X, Y = inputs(B)
    times = dt * np.arange(N_TICKS)
    host = rollout_loop(controller_tick(ctrl, qp), qp, times, Q, X, lambda i: Y, dt, vmax)
    plain = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, virtual_var=X)
    for k in (1, 4, 12):
        res = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, virtual_var=X, record_every=k)
        assert len(res) == len(plain) + 1 and isinstance(res[-1], dict)
        rec = res[-1]
        assert all(isinstance(v, np.ndarray) for v in rec.values())       # (the caller's container type)
        _check_records(rec, host, k, qp, "%s B=%d" % (family, B))
        assert rec["q"].shape == (N_TICKS // k, B, Q.shape[1])
        # the end of the launch is what it was
        assert np.abs(res[0] - host[-1]["q"]).max() < Q_TOL
        for a, b in zip(res[:-1], plain):
            assert (a is None and b is None) or np.allclose(a, b, rtol=0, atol=Q_TOL if a.dtype.kind == "f" else 0)
    if family.startswith("stack") and B == 100:
        modes = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, record_every=1)[-1]["mode"]
        assert set(np.unique(modes)) == {0, 1}          # (the mode store is exercised with both values)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_last_record_is_the_launch_s_own_result_bitwise(iiwa_fk, ur5_fk, monkeypatch, family):
    """twelve ticks, a record every fourth: the last record and the final results come from the same registers; and
    without records and with a 2-D input_var the call is today's - same tuple, same bits from call to call"""
    ctrl, qp, dt, vmax, inputs = _family(family, iiwa_fk, ur5_fk, monkeypatch)
    Q, X, Y = inputs(100)
    times = dt * np.arange(12)
    res = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, virtual_var=X, record_every=4)
    rec = res[-1]
    assert rec["q"].shape[0] == 3
    if X is None:
        finals = {"q": res[0], "dq": res[1], ("status" if qp else "mode"): res[3 if qp else 2]}
        if qp and res[2] is not None:
            finals["slack"] = res[2]
    else:
        finals = {"q": res[0], "x": res[1], "dq": res[2], "dx": res[3], ("status" if qp else "mode"): res[-2]}
    assert set(finals) == set(rec)
    for name, val in finals.items():
        assert np.array_equal(rec[name][-1], val, equal_nan=val.dtype.kind == "f"), name
    a = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, virtual_var=X, record_every=None)
    b = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, virtual_var=X)
    assert len(a) == len(b) == len(res) - 1
    assert len(a) == ((4 if X is None else 6) if qp else (3 if X is None else 5))
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v, equal_nan=u.dtype.kind == "f")


def _moving(Y, n_ticks):
    """the moving target of bench.py's hot QP: a millimetre per tick in position"""
    Y3 = np.repeat(Y[None], n_ticks, axis=0)
    Y3[:, :, :3] += 1e-3 * np.arange(n_ticks)[:, None, None]
    return Y3


@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("family", ["stack_values", "qp_box"])
def test_per_tick_target_matches_the_host_loop(iiwa_fk, ur5_fk, monkeypatch, family, method):
    """tick i reads record i of input_var [n_ticks, B, n_y] (Runge-Kutta: all four stages of the tick), against the
    host loop that passes that record at tick i; records taken along the way are checked too"""
    ctrl, qp, dt, vmax, inputs = _family(family, iiwa_fk, ur5_fk, monkeypatch)
    Q, X, Y = inputs(100)
    n = 7
    times = dt * np.arange(n)
    Y3 = _moving(Y, n)
    host = rollout_loop(controller_tick(ctrl, qp), qp, times, Q, X, lambda i: Y3[i], dt, vmax, rk4=method == "rk4")
    res = ctrl.rollout_batch(times, Q, input_var=Y3, dt=dt, max_speed=vmax, method=method, record_every=3)
    assert len(res) == (5 if qp else 4)
    eq, ev = np.abs(res[0] - host[-1]["q"]).max(), np.abs(res[1] - host[-1]["dq"]).max()
    print("%s %s: |q| %.3e |dq| %.3e" % (family, method, eq, ev))
    assert eq < Q_TOL and ev < V_TOL
    if qp:
        assert (res[3] == 0).all() and np.abs(res[2] - host[-1]["slack"]).max() < V_TOL
    else:
        assert np.array_equal(res[2], host[-1]["flag"])
    _check_records(res[-1], host, 3, qp, "%s %s moving" % (family, method))
    # the target did move the result: against the standing one the state differs by far more than the tolerance
    still = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, method=method)
    assert np.abs(still[0] - res[0]).max() > 1e3 * Q_TOL
    # ... and a standing target given per tick is the 2-D call
    same = ctrl.rollout_batch(times, Q, input_var=np.repeat(Y[None], n, axis=0), dt=dt, max_speed=vmax, method=method)
    assert len(same) == len(still)
    assert np.abs(same[0] - still[0]).max() < Q_TOL and np.abs(same[1] - still[1]).max() < V_TOL
    assert np.array_equal(same[-1], still[-1])


def test_device_tensors_in_and_record_out(iiwa_fk, ur5_fk, monkeypatch):
    """tensors in, tensors out; ``record_out`` tensors are written in place and validated"""
    import torch
    ctrl, qp, dt, vmax, inputs = _family("stack_values", iiwa_fk, ur5_fk, monkeypatch)
    Q, _, Y = inputs(100)
    times = dt * np.arange(8)
    ref = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, record_every=2)[-1]
    mine = torch.full((4, 100, 7), np.nan, dtype=torch.float64, device="cuda")
    res = ctrl.rollout_batch(times, torch.from_numpy(Q).cuda(), input_var=torch.from_numpy(_moving(Y, 8) * 0 + Y).cuda(),
                             dt=dt, max_speed=vmax, record_every=2, record_out={"q": mine})
    rec = res[-1]
    assert rec["q"] is mine and all(isinstance(v, torch.Tensor) and v.is_cuda for v in rec.values())
    assert np.array_equal(mine.cpu().numpy(), ref["q"]) and np.array_equal(rec["mode"].cpu().numpy(), ref["mode"])
    with pytest.raises(ValueError, match="shape"):
        ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, record_every=2, record_out={"q": mine[:3]})
    with pytest.raises(ValueError, match="no field"):
        ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, record_every=2, record_out={"slack": mine})


@pytest.mark.parametrize("kind", ["pinv", "qp"])
def test_refusals(iiwa_fk, monkeypatch, kind):
    Q, Y = skills.synthetic_inputs(iiwa_fk, 8, seed=15)
    times = np.zeros(3)
    if kind == "pinv":
        ok = cc.PseudoInverseController(skill_spec=skills.stack_skill(iiwa_fk), options=dict(skills.STACK_OPTIONS))
    else:
        ok = cc.ReactiveQPController(skill_spec=skills.qp_skill(iiwa_fk))
    ok.setup_problem_functions()
    ok.setup_solver()
    with pytest.raises(ValueError, match="records"):
        ok.rollout_batch(times, Q, input_var=np.repeat(Y[None], 4, axis=0))       # (four records, three ticks)
    with pytest.raises(ValueError, match="record_every"):
        ok.rollout_batch(times, Q, input_var=Y, record_every=0)
    # a handle served only by the built-in dynamic kernel: refused, not chunked
    monkeypatch.setenv("CLIK_FORCE_DYNAMIC", "1")
    if kind == "pinv":
        dyn = cc.PseudoInverseController(skill_spec=skills.stack_skill(iiwa_fk), options=dict(skills.STACK_OPTIONS))
    else:
        dyn = cc.ReactiveQPController(skill_spec=skills.qp_skill(iiwa_fk))
    dyn.setup_problem_functions()
    dyn.setup_solver()
    with pytest.raises(Exception, match="shape-specialised"):
        dyn.rollout_batch(times, Q, input_var=Y, record_every=1)
    with pytest.raises(Exception, match="shape-specialised"):
        dyn.rollout_batch(times, Q, input_var=np.repeat(Y[None], 3, axis=0))
