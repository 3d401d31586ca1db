"""GPU: ``constraint_values_batch`` - e, J = d e / d (q, x) and d e / d t of every constraint of a skill over a batch or a
whole trajectory of states, from the kernel of clik_monitor.hpp - against the oracle's expression evaluator
(``ExprEvaluator.vector``), for both controllers.

Tolerances: the ones tests/test_gpu_qp.py holds the same quantities to - device Jacobian rows max |d| < 1e-12, and 1e-12
for the unscaled e and e_t; every fixture here is O(1) (max |ref| below 4; below 15 for the `ops` skill, whose rows add
up to three library functions), none is scaled."""
import os
import subprocess
import sys

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import skills
from oracle import clik_oracle

import notebook_figures as cf
import time_skills
from extern_skills import double_pendulum_skill, dual_quaternion_skill, mixed_frame_skill, ops_inputs, ops_skill
from test_figure_pins import PIXELS

pytestmark = pytest.mark.gpu

TOL = 1e-12
BATCHES = (1, 63, 65, 257)      # a lone row, both sides of a wave, one past a 256-lane block
NAMES = ["pose", "stack", "qp", "dual_quaternion", "pendulum", "tracking", "tracking_qp", "mixed"]


def _make(name, iiwa_fk, ur5_fk, **options):
    """(spec, controller, set up) of a fixture"""
    if name == "pose":
        spec, ctrl = skills.pose_skill(iiwa_fk), None
    elif name == "stack":
        spec = skills.stack_skill(iiwa_fk)
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict(skills.STACK_OPTIONS, **options))
    elif name == "qp":
        spec = skills.qp_skill(iiwa_fk)
        ctrl = cc.ReactiveQPController(skill_spec=spec, options=dict(options))
    elif name == "dual_quaternion":
        spec = dual_quaternion_skill(ur5_fk)                    # (the 8-row deviation as generated code)
        ctrl = cc.ReactiveQPController(skill_spec=spec, options=dict(options))
    elif name == "pendulum":
        spec = double_pendulum_skill(track=True)
        ctrl = cc.ReactiveQPController(skill_spec=spec, robot_var_weights=[1.0, 1.0], options=dict(options))
    elif name == "tracking":
        spec, ctrl = time_skills.tracking_spec(ur5_fk), None    # (time slots: e_t != 0)
    elif name == "tracking_qp":
        spec = time_skills.track_qp_spec(ur5_fk)
        ctrl = cc.ReactiveQPController(skill_spec=spec, options=dict(options))
    elif name == "ops":
        spec = ops_skill()          # (the operations no other skill emits, no kinematics: generated code throughout)
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict({"multidim_sets": True}, **options))
    elif name == "ops_qp":
        spec = ops_skill()
        ctrl = cc.ReactiveQPController(skill_spec=spec, options=dict(options))
    else:
        spec = mixed_frame_skill(iiwa_fk)                       # (a virtual variable: J has n_q + n_x columns)
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict({"multidim_sets": False}, **options))
    if ctrl is None:
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict(options))
    ctrl.setup_problem_functions()
    if isinstance(ctrl, cc.ReactiveQPController):
        ctrl.setup_solver()
    return spec, ctrl


def _inputs(name, B, iiwa_fk, seed=0):
    """(Q, X | None, Y | None) of a fixture, away from anything singular"""
    rng = np.random.default_rng(100 + seed)
    if name in ("pose", "stack", "qp"):
        Q, Y = skills.synthetic_inputs(iiwa_fk, B, seed=seed, distribution="mixed")
        return Q, None, Y
    if name == "mixed":
        Q, _ = skills.synthetic_inputs(iiwa_fk, B, seed=seed)
        return Q, rng.uniform(-1.0, 1.0, size=(B, 1)), rng.uniform(-1.0, 1.0, size=(B, 3))
    if name == "pendulum":
        return np.stack([rng.uniform(0.2, 2.9, B), rng.uniform(-1.5, 1.5, B)], axis=1), None, None
    return time_skills.UR5_HOME + rng.normal(scale=0.3, size=(B, 6)), None, None


def _oracle(spec, ctrl, t, Q, X=None, Y=None):
    """(e [B, M_tot], J [B, M_tot, n], e_t [B, M_tot]) in the rows of ``ctrl.constraint_rows()``: one evaluator for the
    record, every constraint's expression through ``vector``"""
    Z = Q if X is None else np.hstack([Q, X])
    ev = clik_oracle.ExprEvaluator(spec, t, Z, Y)
    rows = ctrl.constraint_rows()
    m_tot = max(sl.stop for sl in rows.values())
    e, J, et = np.zeros((len(Q), m_tot)), np.zeros((len(Q), m_tot, Z.shape[1])), np.zeros((len(Q), m_tot))
    by_label = {c.label: c for c in spec.constraints}
    assert set(by_label) == set(rows)
    for label, sl in rows.items():
        e[:, sl], et[:, sl], J[:, sl] = ev.vector(by_label[label].expression)
    return e, J, et


def _close(name, what, got, ref):
    bound = TOL
    err = float(np.abs(got - ref).max())
    print("%s %s: max |dev - oracle| = %.3g (bound %.3g, max |ref| %.3g)" % (name, what, err, bound, np.abs(ref).max()))
    assert np.isfinite(got).all() and err < bound, (name, what, err, bound)


@pytest.fixture(scope="module")
def ctrls(iiwa_fk, ur5_fk):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _make(name, iiwa_fk, ur5_fk)
        return cache[name]
    return get


# ---- 1: values and Jacobians against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_values_and_jacobians_match_the_oracle(ctrls, iiwa_fk, name):
    spec, ctrl = ctrls(name)
    d = ctrl.descriptor
    t = 1.3
    Qa, Xa, Ya = _inputs(name, max(BATCHES), iiwa_fk)
    ref = _oracle(spec, ctrl, t, Qa, Xa, Ya)          # (one reference for all batch sizes: a row does not see its batch)
    m_tot = ref[0].shape[1]
    assert m_tot == sum(int(task["m"]) for task in d.tasks)
    for B in BATCHES:
        e, J, et = ctrl.constraint_values_batch(t, Qa[:B], virtual_var=None if Xa is None else Xa[:B],
                                                input_var=None if Ya is None else Ya[:B], jacobian=True)
        assert e.shape == (B, m_tot) and J.shape == (B, m_tot, d.n_q + d.n_x) and et.shape == (B, m_tot)
        _close(name, "e B=%d" % B, e, ref[0][:B])
        _close(name, "J B=%d" % B, J, ref[1][:B])
        _close(name, "e_t B=%d" % B, et, ref[2][:B])
    if name in ("tracking", "tracking_qp", "pendulum", "mixed"):
        assert np.abs(ref[2]).max() > 1e-3          # (these follow a trajectory in time)
    # the single-instance form returns what the notebooks' cnstr.eval(t, q) does
    first = ctrl.constraint_values_batch(t, Qa[:1], virtual_var=None if Xa is None else Xa[:1],
                                         input_var=None if Ya is None else Ya[:1])
    one = ctrl.constraint_values(t, Qa[0], None if Xa is None else Xa[0], None if Ya is None else Ya[0])
    assert list(one) == list(ctrl.constraint_rows())
    for label, sl in ctrl.constraint_rows().items():
        assert one[label].toarray().shape == (sl.stop - sl.start, 1)
        assert np.array_equal(one[label].toarray()[:, 0], first[0, sl])


@pytest.mark.parametrize("name", ["ops", "ops_qp"])
def test_generated_operations_match_the_oracle(ctrls, name):
    """tan, log, every form of pow, sign, fabs, fmax, fmin, asin, acos, atan, atan2, tanh and if_else on `<=` and on a
    logic_and as a skill's constraints: e, J and d e / d t against the oracle's dual numbers under the bound of this
    file, a batch and a trajectory, states away from every switch"""
    spec, ctrl = ctrls(name)
    stamps = np.array([0.4, 1.3, 2.9])
    recs = [ops_inputs(65, 40 + r, t=stamps[r]) for r in range(3)]
    Q3, Y3 = np.stack([r[0] for r in recs]), np.stack([r[1] for r in recs])
    refs = [_oracle(spec, ctrl, stamps[r], Q3[r], None, Y3[r]) for r in range(3)]
    assert refs[0][0].shape == (65, 10) and max(np.abs(a).max() for ref in refs for a in ref) < 15.0
    assert min(np.abs(ref[2]).max() for ref in refs) > 1e-2         # (the time terms move)
    for B in (1, 65):
        got = ctrl.constraint_values_batch(stamps[1], Q3[1][:B], input_var=Y3[1][:B], jacobian=True)
        assert got[0].shape == (B, 10) and got[1].shape == (B, 10, 4) and got[2].shape == (B, 10)
        for what, a, ref in zip(("e", "J", "e_t"), got, refs[1]):
            _close(name, "%s B=%d" % (what, B), a, ref[:B])
        traj = ctrl.constraint_values_batch(stamps, Q3[:, :B], input_var=Y3[:, :B], jacobian=True)
        for r in range(3):
            for what, a, ref in zip(("e", "J", "e_t"), traj, refs[r]):
                _close(name, "%s R=3 B=%d record %d" % (what, B, r), a[r], ref[:B])
        if B == 65:         # R = 1: the middle record as a trajectory of one
            single = ctrl.constraint_values_batch(stamps[1:2], Q3[1:2], input_var=Y3[1:2], jacobian=True)
            for a, b in zip(single, got):
                assert np.array_equal(a[0], b)


# ---- 2: trajectory shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "tracking", "mixed"])
def test_trajectory_shapes_equal_the_record_by_record_calls(ctrls, iiwa_fk, name):
    spec, ctrl = ctrls(name)
    R, B = 3, 65
    recs = [_inputs(name, B, iiwa_fk, seed=10 + r) for r in range(R)]
    Q3 = np.stack([r[0] for r in recs])
    X3 = None if recs[0][1] is None else np.stack([r[1] for r in recs])
    Y3 = None if recs[0][2] is None else np.stack([r[2] for r in recs])
    stamps = np.array([0.4, 1.7, 2.9])
    kw = lambda r, y: dict(virtual_var=None if X3 is None else X3[r], input_var=y, jacobian=True)      # noqa: E731
    # [R] stamps, one input block per record: record r is the 2-D call on robot_var[r] at stamp r, bit for bit
    got = ctrl.constraint_values_batch(stamps, Q3, virtual_var=X3, input_var=Y3, jacobian=True)
    assert got[0].shape[:2] == (R, B) and got[1].shape[:2] == (R, B) and got[2].shape[:2] == (R, B)
    for r in range(R):
        one = ctrl.constraint_values_batch(stamps[r], Q3[r], **kw(r, None if Y3 is None else Y3[r]))
        for a, b in zip(got, one):
            assert np.array_equal(a[r], b), (name, r)
        for k, a in enumerate(_oracle(spec, ctrl, stamps[r], Q3[r], None if X3 is None else X3[r],
                                      None if Y3 is None else Y3[r])):
            _close(name, "record %d output %d" % (r, k), got[k][r], a)
    # one stamp for all records; a [B, n_y] input block shared by all records
    Ys = None if Y3 is None else Y3[0]
    shared = ctrl.constraint_values_batch(1.7, Q3, virtual_var=X3, input_var=Ys, jacobian=True)
    for r in range(R):
        one = ctrl.constraint_values_batch(1.7, Q3[r], **kw(r, Ys))
        for a, b in zip(shared, one):
            assert np.array_equal(a[r], b), (name, r)
    # [B] stamps with a 2-D robot_var: one per instance, as solve_batch(times[B], ...)
    per_inst = np.linspace(0.0, 3.0, B)
    got = ctrl.constraint_values_batch(per_inst, Q3[0], **kw(0, Ys))
    for k, a in enumerate(_oracle(spec, ctrl, per_inst, Q3[0], None if X3 is None else X3[0], Ys)):
        _close(name, "per-instance stamps output %d" % k, got[k], a)
    for b in (0, 17, B - 1):
        one = ctrl.constraint_values_batch(per_inst[b], Q3[0][b:b + 1],
                                           virtual_var=None if X3 is None else X3[0][b:b + 1],
                                           input_var=None if Ys is None else Ys[b:b + 1], jacobian=True)
        for a, c in zip(got, one):
            assert np.array_equal(a[b:b + 1], c), (name, b)
    # mismatches are refused before anything is launched
    with pytest.raises(ValueError, match="time_var has 2 entries"):
        ctrl.constraint_values_batch(stamps[:2], Q3, virtual_var=X3, input_var=Y3)
    with pytest.raises(ValueError, match="time_var has 3 entries"):
        ctrl.constraint_values_batch(stamps, Q3[0], virtual_var=None if X3 is None else X3[0], input_var=Ys)
    if Y3 is not None:
        with pytest.raises(ValueError, match="input_var"):
            ctrl.constraint_values_batch(stamps, Q3, virtual_var=X3, input_var=Y3[:2])
    if X3 is not None:
        with pytest.raises(ValueError, match="virtual_var"):
            ctrl.constraint_values_batch(stamps, Q3, virtual_var=X3[0], input_var=Y3)


# ---- 3: optional outputs -------------------------------------------------------------------------------------------------
def test_optional_outputs_and_containers(ctrls, iiwa_fk):
    import torch
    spec, ctrl = ctrls("stack")
    Q, _, Y = _inputs("stack", 65, iiwa_fk, seed=3)
    e_only = ctrl.constraint_values_batch(0.0, Q, input_var=Y)
    e, J, et = ctrl.constraint_values_batch(0.0, Q, input_var=Y, jacobian=True)
    assert isinstance(e_only, np.ndarray) and isinstance(J, np.ndarray) and isinstance(et, np.ndarray)
    assert np.array_equal(e_only, e)
    dev = ctrl._device
    Qd, Yd = torch.from_numpy(Q).to(dev), torch.from_numpy(Y).to(dev)
    out = torch.full(e.shape, -7.0, dtype=torch.float64, device=dev)
    res = ctrl.constraint_values_batch(0.0, Qd, input_var=Yd, out=out)
    assert res is out and isinstance(res, torch.Tensor) and np.array_equal(out.cpu().numpy(), e)
    td = ctrl.constraint_values_batch(0.0, Qd, input_var=Yd, jacobian=True)
    assert all(isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float64 for t in td)
    assert np.array_equal(td[1].cpu().numpy(), J) and np.array_equal(td[2].cpu().numpy(), et)
    with pytest.raises(ValueError, match="out must have shape"):
        ctrl.constraint_values_batch(0.0, Qd, input_var=Yd, out=out[:-1])
    with pytest.raises(ValueError, match="input_var"):
        ctrl.constraint_values_batch(0.0, Qd)
    assert ctrl._lib.clik_pinv_n_constraint_rows(ctrl._handle) == e.shape[1]


# ---- 4: time_on_device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tracking", "tracking_qp"])
def test_time_on_device_table_gives_the_same_values(ctrls, iiwa_fk, ur5_fk, name):
    """the two calls differ in the time table only, which agrees to a few units in the last place
    (profiles/time_on_device.md): the same tolerance as against the oracle"""
    import torch
    spec, host = ctrls(name)
    _, on = _make(name, iiwa_fk, ur5_fk, time_on_device=True)
    R, B = 3, 65
    Q3 = np.stack([_inputs(name, B, iiwa_fk, seed=20 + r)[0] for r in range(R)])
    stamps = np.array([0.4, 1.7, 2.9])
    ref = host.constraint_values_batch(stamps, Q3, jacobian=True)
    dev = on._device
    got = on.constraint_values_batch(torch.from_numpy(stamps).to(dev), torch.from_numpy(Q3).to(dev), jacobian=True)
    assert all(isinstance(t, torch.Tensor) for t in got)
    for k, (a, b) in enumerate(zip(got, ref)):
        _close(name, "time_on_device output %d" % k, a.cpu().numpy(), b)
    per_inst = np.linspace(0.0, 3.0, B)
    ref = host.constraint_values_batch(per_inst, Q3[0], jacobian=True)
    got = on.constraint_values_batch(torch.from_numpy(per_inst).to(dev), torch.from_numpy(Q3[0]).to(dev), jacobian=True)
    for k, (a, b) in enumerate(zip(got, ref)):
        _close(name, "time_on_device per-instance output %d" % k, a.cpu().numpy(), b)
    _close(name, "time_on_device scalar stamp", on.constraint_values_batch(1.7, Q3[1]), host.constraint_values_batch(1.7, Q3[1]))


# ---- 5: tail and isolation -----------------------------------------------------------------------------------------------
def test_tail_is_masked_and_rows_are_isolated(ctrls, iiwa_fk):
    import torch
    spec, ctrl = ctrls("stack")
    d, dev = ctrl.descriptor, ctrl._device
    B = 65
    Q, _, Y = _inputs("stack", B, iiwa_fk, seed=5)
    Qd, Yd = torch.from_numpy(Q).to(dev), torch.from_numpy(Y).to(dev)
    clean = ctrl.constraint_values_batch(0.0, Qd, input_var=Yd, jacobian=True)
    m_tot, n = clean[0].shape[1], d.n_q + d.n_x
    # one guard row behind e and J, through the C entry point (the method allocates J itself)
    from casclik_amd.controllers.base_controller import current_stream, ptr
    sentinel = -12345.678
    E = torch.full((B + 1, m_tot), sentinel, dtype=torch.float64, device=dev)
    J = torch.full((B + 1, m_tot, n), sentinel, dtype=torch.float64, device=dev)
    Et = torch.full((B + 1, m_tot), sentinel, dtype=torch.float64, device=dev)
    ctrl._require_kernel("monitor")
    with torch.cuda.device(dev):
        rc = ctrl._lib.clik_pinv_constraint_values(ctrl._handle, 1, B, None, 0, 0, ptr(Qd), None, ptr(Yd), 0, ptr(E), ptr(J),
                                                   ptr(Et), current_stream(dev))
    assert rc == 0
    torch.cuda.synchronize(dev)
    for guarded, ref in ((E, clean[0]), (J, clean[1]), (Et, clean[2])):
        assert torch.equal(guarded[:B], ref)
        assert bool((guarded[B] == sentinel).all()), "the guard row behind the last instance was written"
    # a NaN in one instance's q: every other row is the clean run's, bit for bit (the poisoned row itself is whatever
    # the arithmetic gives - device code is built without NaN semantics)
    bad = 40
    Qn = Qd.clone()
    Qn[bad, 2] = float("nan")
    poisoned = ctrl.constraint_values_batch(0.0, Qn, input_var=Yd, jacobian=True)
    keep = torch.arange(B, device=dev) != bad
    for a, b in zip(poisoned, clean):
        assert torch.equal(a[keep], b[keep])


# ---- 6: the notebooks' loop, closed --------------------------------------------------------------------------------------
def test_closed_loop_error_curve_over_a_recorded_rollout(ctrls, iiwa_fk):
    spec, ctrl = ctrls("stack")
    B, n_ticks, dt = 65, 32, 0.01
    Q, _, Y = _inputs("stack", B, iiwa_fk, seed=6)
    times = dt * np.arange(n_ticks)
    rec = ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, record_every=1)[-1]
    assert rec["q"].shape == (n_ticks, B, ctrl.descriptor.n_q)
    e = ctrl.constraint_values_batch(times, rec["q"], input_var=Y)
    rows = ctrl.constraint_rows()
    assert e.shape == (n_ticks, B, max(sl.stop for sl in rows.values()))
    for r in (0, 13, n_ticks - 1):
        _close("stack", "closed loop record %d" % r, e[r], _oracle(spec, ctrl, times[r], rec["q"][r], None, Y)[0])
    # the pose task converges along the rollout: over the batch, and instance by instance except where a joint limit takes
    # over.  The ORACLE's closed loop on these inputs (clik_oracle.pinv_solve_batch, 32 Euler ticks of 0.01) ends further
    # from the target than its first record for exactly two of the 65 instances: 32 (pose error norm 0.99588 -> 1.17150,
    # joint-limit mode from tick 3 on) and 52 (0.76106 -> 1.38574, the limit active in ticks 16 and 17); the closest
    # other one (41) shrinks by a factor 0.9999996, the next by 0.983; 8 instances stay in mode 0 throughout.  The device loop follows the oracle's to 1e-12.
    pose = rows["tool_pose"]
    first, last = np.linalg.norm(e[0][:, pose], axis=1), np.linalg.norm(e[-1][:, pose], axis=1)
    assert np.linalg.norm(last) < np.linalg.norm(first), (np.linalg.norm(first), np.linalg.norm(last))
    # (instance 41 is the factor-0.9999996 one: its sign is inside what the rollout's velocities differ from the oracle's by)
    grown = set(np.nonzero(last >= first)[0].tolist())
    assert {32, 52} <= grown <= {32, 41, 52}, (grown, first, last)
    free = (rec["mode"] == 0).all(axis=0)
    assert free.sum() >= 6 and (last[free] < first[free]).all(), (free.sum(), first[free], last[free])


# ---- 7: a stored figure through the new path -----------------------------------------------------------------------------
def test_error_decay_figure_from_the_device_values(ur5_fk):
    """ur5_dual_quaternion_vs_transformation_matrix.ipynb cells 24-27: the loop of
    test_hip_qp_reproduces_the_error_decay_of_the_frame_figures, its error curve evaluated afterwards in ONE
    [R, 1, 6] call on the states it went through"""
    spec, _, error_norm = cf.frame_error_skill(ur5_fk, "Q_dist1", "qp")
    ctrl = cc.ReactiveQPController(skill_spec=spec)
    ctrl.setup_problem_functions()
    ctrl.setup_solver()
    ctrl.setup_initial_problem_solver()
    state = {"slack": ctrl.solve_initial_problem(0, cf.UR5_HOME)[-1]}

    def solve(t, q):
        res = ctrl.solve(t, q, warmstart_slack_var=state["slack"])
        if res[-1] is not None:
            state["slack"] = res[-1].toarray()[:, 0]
        return res[0].toarray()[:, 0]
    t_sim, log_e, q_sim = cf.simulate_frame_error(error_norm, solve, return_q=True)
    e = ctrl.constraint_values_batch(0.0, q_sim[:, None, :])
    assert e.shape[:2] == (len(q_sim), 1)
    rows = [sl for sl in ctrl.constraint_rows().values() if sl.stop - sl.start == 8]
    assert len(rows) == 1
    dev_log_e = np.log10(np.linalg.norm(e[:, 0, rows[0]], axis=1))
    worst, n = cf.deviation_in_pixels("ur5_qdist1_e", "qp", t_sim, dev_log_e, above=-13.0)
    print("figure ur5_qdist1_e from the device values: worst %.3f px over %d points" % (worst, n))
    assert n >= 25 and worst < PIXELS, (worst, n)


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------
def test_a_skill_beyond_the_shape_specialised_family_is_refused(iiwa_fk):
    """more constraints than a ShapeDesc holds: the built-in dynamic kernel serves the ticks, nothing serves the read-out"""
    from casclik_amd import sym as cs
    t, q = cs.MX.sym("t"), cs.MX.sym("q", 7)
    cons = [cc.EqualityConstraint("c%d" % i, q[i % 7] - 0.1 * i, gain=1.0, priority=i, constraint_type="soft")
            for i in range(9)]
    ctrl = cc.PseudoInverseController(skill_spec=cc.SkillSpecification("nine", t, q, constraints=cons))
    ctrl.setup_problem_functions()
    assert ctrl.kernel_name == "dynamic"
    assert list(ctrl.constraint_rows().items())[-1] == ("c8", slice(8, 9))
    with pytest.raises(NotImplementedError, match="instantiated"):
        ctrl.constraint_values_batch(0.0, np.zeros((3, 7)))


_FORCED = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import casclik_amd as cc
from casclik_amd import skills
fk = skills.iiwa()
ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
ctrl.setup_problem_functions()
assert ctrl.kernel_name == "dynamic", ctrl.kernel_name
Q, Y = skills.synthetic_inputs(fk, 5, seed=0)
try:
    ctrl.constraint_values_batch(0.0, Q, input_var=Y)
except NotImplementedError as exc:
    assert "instantiated" in str(exc), exc
    print("REFUSED")
"""


def test_the_dynamic_fallback_is_refused():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CLIK_FORCE_DYNAMIC="1")
    out = subprocess.run([sys.executable, "-c", _FORCED % (root, os.path.join(root, "tests"))], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0 and b"REFUSED" in out.stdout, out.stdout.decode()[-2000:]
