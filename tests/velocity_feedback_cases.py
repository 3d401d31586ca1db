"""What the tests of ``options["velocity_feedback"]`` share and what needs no GPU: the skills that read the last velocity
in ``input_var``, their maps, their inputs, and the host loops that rewrite the fed entries between ticks - of
``solve_batch`` calls (the yardstick) and of oracle calls (the independent one)."""
import numpy as np

import casclik_amd as cc
from casclik_amd import skills
from casclik_amd import sym as cs
from oracle import clik_oracle

import converge_cases as K

A_DT = 0.004                    # the QP skill's acceleration limit times dt: |dq_k - dq_{k-1}| <= A_DT per joint
DT = 0.008
N_TICKS = 11
FB_IIWA = tuple(range(7, 14))   # joint j's velocity is read in input_var[7 + j]; [0, 7) is the pose target
FB_PATH = (-1,) * 6 + (0,)      # the path parameter's rate in input_var[0], the joints feed nothing


def qp_skill(fk, a_dt=A_DT):
    """config 4 (skills.qp_skill) plus an acceleration limit around the last velocity, read in input_var[7:14]"""
    n = len(fk["joint_names"])
    t, q, dq, y = cs.MX.sym("t"), cs.MX.sym("q", n), cs.MX.sym("dq", n), cs.MX.sym("y", 7 + n)
    v_max = np.array(fk["velocity"])
    cons = [cc.EqualityConstraint(label="tool_pose", expression=skills._pose_expression(fk["T_fk"](q), y), gain=10.0,
                                  constraint_type="soft", priority=1),
            cc.VelocitySetConstraint(label="joint_speed_limits", expression=q, set_min=-v_max, set_max=v_max, priority=0),
            cc.VelocitySetConstraint("accel", q, set_min=y[7:7 + n] - a_dt, set_max=y[7:7 + n] + a_dt)]
    return cc.SkillSpecification(label="qp_accel", time_var=t, robot_var=q, robot_vel_var=dq, input_var=y, constraints=cons)


def pinv_skill(fk):
    """config 2 (skills.pose_skill) plus a pull towards the last velocity in the null space of the pose task"""
    n = len(fk["joint_names"])
    t, q, dq, y = cs.MX.sym("t"), cs.MX.sym("q", n), cs.MX.sym("dq", n), cs.MX.sym("y", 7 + n)
    cons = [cc.EqualityConstraint(label="tool_pose", expression=skills._pose_expression(fk["T_fk"](q), y), gain=10.0,
                                  constraint_type="soft", priority=1),
            cc.VelocityEqualityConstraint("smooth", q, target=y[7:7 + n], priority=2)]
    return cc.SkillSpecification(label="pose_smooth", time_var=t, robot_var=q, robot_vel_var=dq, input_var=y,
                                 constraints=cons)


def timed_skill(fk):
    """``pinv_skill`` with a target that sways in time (one time slot), for ``options["time_on_device"]``"""
    n = len(fk["joint_names"])
    t, q, dq, y = cs.MX.sym("t"), cs.MX.sym("q", n), cs.MX.sym("dq", n), cs.MX.sym("y", 7 + n)
    # (2 mm: the states stay where ``pinv_skill`` has them, well away from the singular configurations a larger sway -
    # 5 cm at gain 10 - drives some instances through, where two compilations of the same tick no longer stay together)
    sway = cs.vertcat(0.002 * cs.sin(3.0 * t), 0.0, 0.0, 0.0, 0.0, 0.0)
    cons = [cc.EqualityConstraint(label="tool_pose", expression=skills._pose_expression(fk["T_fk"](q), y) - sway, gain=10.0,
                                  constraint_type="soft", priority=1),
            cc.VelocityEqualityConstraint("smooth", q, target=y[7:7 + n], priority=2)]
    return cc.SkillSpecification(label="pose_smooth_t", time_var=t, robot_var=q, robot_vel_var=dq, input_var=y,
                                 constraints=cons)


def path_skill(fk):
    """converge_cases.path_skill (one virtual variable) extended by a VelocityEqualityConstraint on the path parameter
    whose target is fed from its own last rate, read in input_var[0]: ``ds_k = 0.5 ds_{k-1} + 0.002``.  It stands ahead
    of the skill's own "progress" at the same priority, so it decides the rate (behind it, it would change nothing a test
    can see), and the tool follows the point the parameter names: a launch that feeds nothing ends elsewhere in q and
    x."""
    base = K.path_skill(fk)
    y = cs.MX.sym("y", 1)
    ramp = cc.VelocityEqualityConstraint("ramp", base.virtual_var, target=0.5 * y[0] + 0.002, priority=0)
    return cc.SkillSpecification("path_fed", base.time_var, base.robot_var, virtual_var=base.virtual_var, input_var=y,
                                 constraints=[ramp] + list(base.constraints))


def make(name, iiwa_fk, ur5_fk):
    """(spec, controller with the option - not set up -, is_qp, map) of a case"""
    if name == "qp":
        spec = qp_skill(iiwa_fk)
        return spec, cc.ReactiveQPController(skill_spec=spec, options={"velocity_feedback": FB_IIWA}), True, FB_IIWA
    if name == "timed":
        spec = timed_skill(iiwa_fk)
        return spec, cc.PseudoInverseController(skill_spec=spec, options={"velocity_feedback": FB_IIWA,
                                                                          "time_on_device": True}), False, FB_IIWA
    if name == "pinv":
        spec = pinv_skill(iiwa_fk)
        return spec, cc.PseudoInverseController(skill_spec=spec, options={"velocity_feedback": FB_IIWA}), False, FB_IIWA
    spec = path_skill(ur5_fk)
    return spec, cc.PseudoInverseController(skill_spec=spec, options={"velocity_feedback": FB_PATH}), False, FB_PATH


def iiwa_inputs(fk, B=100):
    """(Q, Y [B, 14]) from converge_cases.reach_inputs: the pose targets, and zeros - at rest before the launch - in the
    fed entries"""
    Q, Y7 = K.reach_inputs(fk, B)
    return Q, np.hstack([Y7, np.zeros((B, 7))])


def path_inputs(B=100):
    Q, X, _ = K.inputs("virtual", None, B)
    return Q, X, np.zeros((B, 1))


def feed(Y, fb, v):
    """Y with the fed entries rewritten from the velocities v [B, n_q + n_x]"""
    Y = Y.copy()
    for j, k in enumerate(fb):
        if k >= 0:
            Y[:, k] = v[:, j]
    return Y


def host_loop(tick, times, Q, X, y_of, fb, dt, vmax=0.0, rk4=False):
    """The yardstick: one call of ``tick(t, q, x, y) -> (dq, dx | None, flag)`` per tick (rk4: per stage, all four with
    the tick's target), the fed entries of the target rewritten between ticks from the velocity the last tick was
    integrated with.  ``y_of(i)``: what the caller gives tick i; its fed entries count at tick 0 only.  Returns one dict
    per tick: the state after it, the velocity applied in it, the flag (QP: the worst status so far)."""
    q, x = Q.copy(), None if X is None else X.copy()
    nq = q.shape[1]
    clamp = (lambda d: np.clip(d, -vmax, vmax)) if vmax > 0.0 else (lambda d: d)
    out, v_last = [], None
    for i, tv in enumerate(times):
        y = y_of(i) if v_last is None else feed(y_of(i), fb, v_last)
        if not rk4:
            dq, dx, flag = tick(float(tv), q, x, y)
            dq = clamp(dq)
        else:
            z = q if x is None else np.hstack([q, x])
            flags = []

            def f(tt, zz):
                d, ddx, fl = tick(float(tt), zz[:, :nq], None if x is None else zz[:, nq:], y)
                flags.append(fl)
                d = clamp(d)
                return d if ddx is None else np.hstack([d, ddx])
            k1 = f(tv, z)
            k2 = f(tv + dt / 2, z + dt / 2 * k1)
            k3 = f(tv + dt / 2, z + dt / 2 * k2)
            k4 = f(tv + dt, z + dt * k3)
            v = (k1 + 2 * k2 + 2 * k3 + k4) / 6.0
            dq, dx = v[:, :nq], None if x is None else v[:, nq:]
            flag = flags[0]
        q = q + dq * dt
        if x is not None:
            x = x + dx * dt
        v_last = dq if dx is None else np.hstack([dq, dx])
        out.append({"q": q.copy(), "x": None if x is None else x.copy(), "dq": dq, "dx": dx, "flag": flag})
    return out


def controller_tick(ctrl, qp):
    """``tick`` of ``host_loop`` on a controller's ``solve_batch``"""
    def tick(t, q, x, y):
        res = ctrl.solve_batch(t, q, virtual_var=x, input_var=y)
        return (res[0], res[1], res[3]) if qp else (res[0], res[1], res[2])
    return tick


def oracle_tick(spec, qp, options=None):
    """``tick`` of ``host_loop`` on the oracle (skills without virtual variables)"""
    def tick(t, q, x, y):
        assert x is None
        if qp:
            dq, _, _, status = clik_oracle.qp_solve_batch(spec, t, q, Y=y)
            return dq[:, :q.shape[1]], None, status
        dq, mode = clik_oracle.pinv_solve_batch(spec, options or {}, t, q, Y=y)
        return dq[:, :q.shape[1]], None, mode
    return tick


def converge_host_loop(spec, Q, Y, fb, tol, max_ticks, dt=K.DT, pinv_fn=None):
    """converge_cases.host_loop extended by the feed: an instance's tick that is integrated rewrites its fed entries,
    a stopped instance keeps them.  ``pinv_fn``: the oracle's pseudo-inverse (None: its literal ``dpinv``).  Returns
    ``(q, dq, ticks, status, residual, sure)``."""
    B = Q.shape[0]
    q, dq, Y = Q.copy(), np.zeros_like(Q), Y.copy()
    ticks, status = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    residual, sure = np.zeros((B, tol.size)), np.ones(B, dtype=bool)
    for r in range(max_ticks + 1):
        go = np.nonzero(status < 0)[0]
        if go.size == 0:
            break
        e, lo, hi, is_set = K.oracle_values(spec, 0.0, q[None, go], None, Y[go])
        d = K.distances(e, lo, hi, is_set)[0]
        residual[go] = d
        sure[go] &= ~(np.abs(d - tol) < K.MARGIN).any(axis=1)
        bad = ~np.isfinite(e[0]).all(axis=1)
        with np.errstate(invalid="ignore"):
            met = (d <= tol).all(axis=1)
        st = np.where(bad, 4, np.where(met, 0, 1 if r == max_ticks else -1))
        status[go] = st
        ticks[go] = r
        go = go[st < 0]
        if go.size == 0:
            continue
        v = clik_oracle.pinv_solve_batch(spec, {}, 0.0, q[go], Y=Y[go], pinv_fn=pinv_fn)[0][:, :Q.shape[1]]
        q[go] += v * dt
        dq[go] = v
        Y[go] = feed(Y[go], fb, v)
    return q, dq, ticks, status, residual, sure
