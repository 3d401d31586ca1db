"""What the tests of ``converge_batch`` / ``ik_batch`` share and what needs no GPU: the fixtures' inputs, the stop rule of
include/clik.h in plain numpy, a host loop on the oracle, and ``select_seeds`` as a plain-Python loop."""
import numpy as np

import casclik_amd as cc
from casclik_amd import skills
from casclik_amd.controllers.base_controller import constraint_row_slices
from casclik_amd.lowering import lower_skill
from oracle import clik_oracle

MARGIN = 4e-12          # (tests/test_gpu_constraint_summary.py: an integer result decided by less is left out)
DT = 0.05               # with gain 10 the error halves per tick
B_ALL = 130             # every batch of the tests is a prefix of this one


def reach_inputs(fk, B, seed=3, lo_exp=-5.0, hi_exp=-1.2):
    """(Q, Y): start states inside 80 % of the joint range and the tool pose at a state near each of them - at a distance
    (a standard deviation per joint) spread over four decades, so that the instances need different numbers of ticks, and small enough (0.06 rad at most)
    that every trajectory is a plain contraction: two compilations of the same tick stay together on it"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(fk["lower"], float), np.asarray(fk["upper"], float)
    Q = rng.uniform(0.8 * lo, 0.8 * hi, size=(B, lo.size))
    near = Q + (10.0 ** rng.uniform(lo_exp, hi_exp, size=(B, 1))) * rng.normal(size=Q.shape)
    Y = np.zeros((B, 7))
    for b in range(B):
        T = fk["chain"].fk_numeric(near[b])
        Y[b, :3], Y[b, 3:] = T[:3, 3], skills.quat_from_matrix(T[:3, :3])
    return Q, Y


UR5_HOME = np.array([-50.0, -160.0, -110.0, -90.0, -90.0, 0.0]) * np.pi / 180.0


def path_skill(fk):
    """the path-following skill of tests/test_gpu_branches.py (one virtual variable) with gain 4 - with dt = 0.05 the
    error shrinks by a fifth per tick -, its line moved so that it passes through the tool's home position at s = 0.3, and
    the path parameter advancing slowly enough that the lag it causes (|d| * 0.001 / 4 = 6e-5) stays inside the tolerance"""
    from casclik_amd import sym as cs
    t, q, s = cs.MX.sym("t"), cs.MX.sym("q", 6), cs.MX.sym("s", 1)
    p = fk["T_fk"](q)[:3, 3]
    d = np.array([0.2, -0.1, 0.05])
    p0 = np.asarray(fk["chain"].fk_numeric(UR5_HOME), float)[:3, 3] - 0.3 * d
    cons = [cc.EqualityConstraint("follow", p - (p0 + d * s), gain=4.0, priority=1, constraint_type="soft"),
            cc.VelocityEqualityConstraint("progress", s, target=0.001, priority=0),
            cc.SetConstraint("s_range", s, set_min=0.0, set_max=1.0, priority=2)]
    return cc.SkillSpecification("path", t, q, virtual_var=s, constraints=cons)


# name -> what a case of test 1 runs with
CASES = {
    "pose": dict(max_ticks=11, tol={"tool_pose": 1e-5}),
    "stack": dict(max_ticks=24, tol={"tool_pose": 1e-4, "joint_centering": np.inf, "joint_limits": 1e-9}),
    "qp": dict(max_ticks=12, tol={"tool_pose": 1e-5, "joint_speed_limits": np.inf}),
    "virtual": dict(max_ticks=24, tol={"follow": 2e-4, "progress": np.inf, "s_range": 1e-9}),
}


def make(name, iiwa_fk, ur5_fk):
    """(spec, controller - not set up -, is_qp) of a case"""
    if name == "pose":
        spec = skills.pose_skill(iiwa_fk)
        return spec, cc.PseudoInverseController(skill_spec=spec), False
    if name == "stack":
        spec = skills.stack_skill(iiwa_fk)
        return spec, cc.PseudoInverseController(skill_spec=spec, options=dict(skills.STACK_OPTIONS)), False
    if name == "qp":
        spec = skills.qp_skill(iiwa_fk)
        return spec, cc.ReactiveQPController(skill_spec=spec), True
    spec = path_skill(ur5_fk)
    return spec, cc.PseudoInverseController(skill_spec=spec), False


def inputs(name, iiwa_fk, B=B_ALL, seed=3):
    """(Q, X | None, Y | None) of a case"""
    if name == "virtual":
        rng = np.random.default_rng(5)
        # (the tool starts at a distance from the path that differs from instance to instance: the path parameter is free)
        return UR5_HOME + (10.0 ** rng.uniform(-3.5, -0.7, size=(B, 1))) * rng.normal(size=(B, 6)), \
            np.full((B, 1), 0.3), None
    Q, Y = reach_inputs(iiwa_fk, B, seed)
    return Q, None, Y


def ik_inputs(fk, T=5, S=13):
    """(targets [T, 7], seeds [S, 7], tol, max_ticks) of the multi-seed test: poses near one state, and seeds at distances
    from that state spread over three decades - the near ones arrive within max_ticks, the far ones do not"""
    rng = np.random.default_rng(11)
    lo, hi = np.asarray(fk["lower"], float), np.asarray(fk["upper"], float)
    star = rng.uniform(0.5 * lo, 0.5 * hi)
    Y = np.zeros((T, 7))
    for k in range(T):
        M = fk["chain"].fk_numeric(star + 0.02 * rng.normal(size=7))
        Y[k, :3], Y[k, 3:] = M[:3, 3], skills.quat_from_matrix(M[:3, :3])
    seeds = star + (10.0 ** np.linspace(-2.5, 0.3, S))[:, None] * rng.normal(size=(S, 7))
    return Y, seeds, 1e-5, 12


def tolerances(spec, by_label):
    rows = constraint_row_slices(lower_skill(spec))
    tol = np.zeros(max(sl.stop for sl in rows.values()))
    for label, sl in rows.items():
        tol[sl] = by_label[label]
    return tol


def oracle_values(spec, t, Q, X=None, Y=None):
    """(e, set_min, set_max) [R, B, M_tot] and is_set [M_tot] of the records Q [R, B, n_q], all at time t, the target
    shared by the records: the oracle's own evaluation of every constraint expression (as ``_oracle`` of
    tests/test_gpu_constraint_summary.py)"""
    R, B = Q.shape[:2]
    flat = lambda A: None if A is None else A.reshape(R * B, -1)         # noqa: E731
    Z = flat(Q) if X is None else np.hstack([flat(Q), flat(X)])
    Yf = flat(None if Y is None else np.broadcast_to(Y, (R,) + Y.shape))
    ev = clik_oracle.ExprEvaluator(spec, np.full(R * B, float(t)), Z, Yf)
    rows = constraint_row_slices(lower_skill(spec))
    m_tot = max(sl.stop for sl in rows.values())
    e = np.zeros((R * B, m_tot))
    lo, hi = np.full((R * B, m_tot), -np.inf), np.full((R * B, m_tot), np.inf)
    is_set = np.zeros(m_tot, dtype=bool)
    views = clik_oracle.attribute_views(ev, spec.constraints)
    for c, view in zip(spec.constraints, views):
        sl = rows[c.label]
        e[:, sl] = ev.vector(c.expression)[0]
        if clik_oracle._cls(c) == "SetConstraint":
            is_set[sl] = True
            m = sl.stop - sl.start
            lo[:, sl] = np.stack([clik_oracle._num(v.set_min, m) for v in view])
            hi[:, sl] = np.stack([clik_oracle._num(v.set_max, m) for v in view])
    shape = (R, B, m_tot)
    return e.reshape(shape), lo.reshape(shape), hi.reshape(shape), is_set


def distances(e, lo, hi, is_set):
    with np.errstate(invalid="ignore"):
        return np.where(is_set, np.maximum(np.maximum(lo - e, e - hi), 0.0), np.abs(e))


def stop_rule(e, lo, hi, is_set, tol, max_ticks):
    """Steps 1 - 4 of the stop rule on the records r = 0 .. max_ticks of a rollout that never stops (e [max_ticks + 1, B,
    M_tot]): ``(ticks [B], status [B], residual [B, M_tot], sure [B])``; ``sure``: no row of the instance comes within
    MARGIN of its tolerance at any record up to its stop."""
    R, B, M = e.shape
    assert R == max_ticks + 1
    d = distances(e, lo, hi, is_set)
    with np.errstate(invalid="ignore"):
        met = (d <= tol).all(axis=2)
        close = (np.abs(d - tol) < MARGIN).any(axis=2)
    bad = ~np.isfinite(e).all(axis=2)
    ticks, status = np.full(B, max_ticks, dtype=np.int32), np.ones(B, dtype=np.int32)
    for b in range(B):
        for r in range(R):
            if bad[r, b] or met[r, b]:
                ticks[b], status[b] = r, 4 if bad[r, b] else 0
                break
    sure = np.array([not close[:ticks[b] + 1, b].any() for b in range(B)])
    return ticks, status, d[ticks, np.arange(B)], sure


def host_loop(spec, options, Q, Y, tol, max_ticks, dt=DT, max_speed=0.0, min_step=0.0, t=0.0, margin=MARGIN):
    """The whole rule, every instance on its own, no device code: the oracle's constraint values and
    ``clik_oracle.pinv_solve_batch`` per tick.  Returns ``(q, dq, ticks, status, residual, sure)``; ``sure``: no row of the
    instance came within ``margin`` of its tolerance."""
    B = Q.shape[0]
    q, dq = Q.copy(), np.zeros_like(Q)
    ticks, status = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    residual, sure = np.zeros((B, tol.size)), np.ones(B, dtype=bool)
    for r in range(max_ticks + 1):
        go = np.nonzero(status < 0)[0]
        if go.size == 0:
            break
        e, lo, hi, is_set = oracle_values(spec, t, q[None, go], None, None if Y is None else Y[go])
        d = distances(e, lo, hi, is_set)[0]
        residual[go] = d
        sure[go] &= ~(np.abs(d - tol) < margin).any(axis=1)
        bad = ~np.isfinite(e[0]).all(axis=1)
        with np.errstate(invalid="ignore"):
            met = (d <= tol).all(axis=1)
        st = np.where(bad, 4, np.where(met, 0, 1 if r == max_ticks else -1))
        status[go] = st
        ticks[go] = r
        go = go[st < 0]
        if go.size == 0:
            continue
        v = clik_oracle.pinv_solve_batch(spec, options, t, q[go], Y=None if Y is None else Y[go])[0][:, :Q.shape[1]]
        if max_speed > 0.0:
            v = np.clip(v, -max_speed, max_speed)
        stall = (min_step > 0.0) & (np.abs(v).max(axis=1) * dt <= min_step)
        status[go[stall]] = 2
        go, v = go[~stall], v[~stall]
        q[go] += v * dt
        dq[go] = v
    return q, dq, ticks, status, residual, sure


def select_seeds_loop(ticks, status, residual, tol, S):
    """``select_seeds`` as its description reads, one target and one seed at a time"""
    T = len(ticks) // S
    rows = [i for i in range(len(tol)) if np.isfinite(tol[i]) and tol[i] != 0.0]
    out = []
    for t in range(T):
        best, best_key = None, None
        for s in range(S):
            k = t * S + s
            if status[k] == 0:
                key = (0, float(ticks[k]))
            elif status[k] != 4:
                key = (1, max([residual[k][i] / tol[i] for i in rows], default=0.0))
            else:
                key = (2, 0.0)
            if best is None or key < best_key:      # (strictly: the lowest index among equals stays)
                best, best_key = s, key
        out.append(best)
    return np.asarray(out, dtype=np.int64)
