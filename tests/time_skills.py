"""Skills whose targets move in time, for the tests of the time slots' device code (test_time_codegen.py,
test_gpu_time_on_device.py), and the times they are evaluated at."""
import os
import sys

import numpy as np

import casclik_amd as cc
from casclik_amd import sym as cs

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))

# the times of the host comparison: zero, tiny, ordinary, negative, large (0.1 * 1e4 = 1000 rad stays inside the
# straight-line range of sincos_joint) and a rollout's stamps
TIMES = np.concatenate([[0.0, 1e-3, 3.0, 29.7, -12.5, 1e4], 3.0 + 0.05 * np.arange(40)])

# beyond it: 0.1 * 2e6 rad, where sincos_joint leaves its straight-line path for the library routine (the tracking skill
# alone is evaluated there)
TIMES_BEYOND_THE_FAST_RANGE = np.array([2.0e6, -2.0e6])

UR5_HOME = np.array([-50.0, -160.0, -110.0, -90.0, -90.0, 0.0]) * np.pi / 180.0


def _path(t):
    return cs.vertcat(0.5 * cs.sin(0.1 * t) * cs.sin(0.1 * t) + 0.2, 0.5 * cs.cos(0.1 * t) + 0.25 * cs.sin(0.1 * t),
                      0.5 * cs.sin(0.1 * t) * cs.cos(0.1 * t) + 0.1)


def tracking_spec(fk, n=6):
    """the `_tracking` skill of test_gpu_rollout.py: products of sin / cos of 0.1 t"""
    t = cs.MX.sym("t")
    q = cs.MX.sym("q", n)
    p = fk["T_fk"](q)[:3, 3]
    return cc.SkillSpecification("track", t, q, constraints=[
        cc.EqualityConstraint("move_point", p - _path(t), gain=0.5, constraint_type="soft")])


def track_qp_spec(fk):
    """the `track_qp` skill of test_gpu_rollout.py::test_per_instance_time_stamps_qp"""
    t = cs.MX.sym("t")
    q = cs.MX.sym("q", 6)
    p = fk["T_fk"](q)[:3, 3]
    return cc.SkillSpecification("track_qp", t, q, constraints=[
        cc.EqualityConstraint("move_point", p - _path(t), gain=0.5, constraint_type="soft"),
        cc.VelocitySetConstraint("speed", q, set_min=-0.4 * np.ones(6), set_max=0.4 * np.ones(6))])


def moe_spec(fk):
    """the Moe-2016 trajectory skill (ur5_moe2016_example2.ipynb) with its three wall sets"""
    import figure_skills
    return figure_skills.moe_skill("singular", cs, cc, fk["T_fk"])[0]


def mixed_spec(n=3):
    """joint-space targets built from pow with exponents 2 and 3, exp, a quotient of two time-only terms and an if_else
    on t (no kinematics: the skill is about its time slots)"""
    t = cs.MX.sym("t")
    q = cs.MX.sym("q", n)
    u = 0.1 * t
    target = cs.vertcat(u ** 2 + 0.01 * u ** 3,
                        cs.exp(-0.05 * t) + (1.0 + 0.2 * t) / (2.0 + cs.cos(0.3 * t)),
                        cs.if_else(t < 5.0, 0.3 * t, 1.5 + cs.sin(0.2 * t)))
    return cc.SkillSpecification("mixed_time", t, q, constraints=[
        cc.EqualityConstraint("follow", q - target[:n], gain=1.0, constraint_type="soft")])


def ops_time_spec():
    """joint-space targets built from the operations no other skill here puts into a time slot: tan(0.05 t) (its pole is
    at t = 31.4, beyond the rollouts' times), log(2 + t t), atan2, tanh, a fractional power (its base held at 1 for
    negative times by an fmax), and an if_else on t >= 5"""
    t = cs.MX.sym("t")
    q = cs.MX.sym("q", 4)
    target = cs.vertcat(0.1 * cs.tan(0.05 * t) + 0.01 * cs.log(2.0 + t * t),
                        cs.atan2(cs.sin(0.1 * t), 1.5 + cs.cos(0.1 * t)) + cs.tanh(0.2 * t - 1.0),
                        1e-3 * (1.0 + 0.1 * cs.fmax(t, 0.0)) ** 2.5,
                        cs.if_else(t >= 5.0, 0.3 + 0.1 * cs.tanh(0.1 * t), 0.06 * t))
    return cc.SkillSpecification("ops_time", t, q, constraints=[
        cc.EqualityConstraint("follow", q - target, gain=1.0, constraint_type="soft")])


def count_nodes(tree):
    """distinct nodes of a scalar tree"""
    seen = set()

    def walk(nd):
        if id(nd) in seen:
            return
        seen.add(id(nd))
        for a in getattr(nd, "args", ()) or ():
            walk(a)
    walk(tree)
    return len(seen)
