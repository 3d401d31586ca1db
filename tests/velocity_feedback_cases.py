"""What the tests of ``options["velocity_feedback"]`` share and what needs no GPU: the skills that read the last velocity
in ``input_var``, their maps and their inputs.  The host loops that rewrite the fed entries between ticks are those of
tests/host_loops.py with the map given (``rollout_loop(..., fb=)``, ``converge_loop(..., fb=)``)."""
import numpy as np

import casclik_amd as cc
from casclik_amd import skills
from casclik_amd import sym as cs

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
