"""CPU: the two host yardsticks of tests/host_loops.py, with the oracle as the tick, against what the loops they replace
returned on the same inputs (tests/golden/host_loops/*.npz: inputs and results, recorded from those loops before they
were removed - bit for bit what ``host_loops`` gave then).  ``ticks``, ``status``, modes and flags exactly; states to
``Q_TOL``, velocities and slack to ``V_TOL``, the tolerances the GPU tests hold the device to against these loops, so that
another linear-algebra library under the oracle does not fail the test; a NaN equals a NaN at the same place."""
import os

import numpy as np
import pytest

from casclik_amd import skills

import converge_cases as K
import host_loops as H
import velocity_feedback_cases as V
from test_gpu_rollout_record import Q_TOL, V_TOL

R_TOL = 1e-8            # a residual moves by ||J||_inf Q_TOL at most (tests/test_gpu_converge.py, test 2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_loops")


def _close(got, ref, tol):
    """|got - ref| < tol, equal where they are not finite (NaN with NaN)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    fin = np.isfinite(ref)
    return got.shape == ref.shape and np.array_equal(got[~fin], ref[~fin], equal_nan=True) and \
        bool((np.abs(got[fin] - ref[fin]) < tol).all())


def _skill(name, iiwa_fk, ur5_fk):
    """(spec, options of its pseudo-inverse controller) of an input set of the fixtures"""
    if name == "feedback":
        return V.pinv_skill(iiwa_fk), {}
    spec, ctrl, _ = K.make(name, iiwa_fk, ur5_fk)
    return spec, ctrl.options


# case -> (input set, arguments of converge_loop, statuses the case is there for)
CONVERGE = {
    "pose_plain": ("pose", {}, {0, 1, 4}),
    "pose_stall": ("pose", dict(max_speed=0.05, min_step=1e-4), {1, 2, 4}),
    "pose_group4": ("pose", dict(group=4), {0, 1, 4, H.CANCELLED}),
    "stack_plain": ("stack", {}, {0, 1}),
    "feedback_fed": ("feedback", dict(fb=V.FB_IIWA), {0}),
}


@pytest.mark.parametrize("case", sorted(CONVERGE))
def test_converge_loop(iiwa_fk, ur5_fk, case):
    """``converge_cases`` "pose" (B = 16, one start state NaN) plain, clamped and stalling, and in groups of four; "stack"
    (SetConstraints); the feedback skill (B = 8, 20 ticks) with the feed"""
    g = np.load(os.path.join(GOLDEN, "converge.npz"))
    name, kw, statuses = CONVERGE[case]
    spec, options = _skill(name, iiwa_fk, ur5_fk)
    Q, Y, tol, n = (g["%s/%s" % (name, k)] for k in ("Q", "Y", "tol", "max_ticks"))
    ref = {k: g["%s/%s" % (case, k)] for k in ("q", "dq", "ticks", "status", "residual", "sure")}
    assert set(np.unique(ref["status"])) == statuses and ref["sure"].all() and np.isnan(Q).any() == (name == "pose")
    q, dq, ticks, status, residual, sure = H.converge_loop(spec, options, Q, Y, tol, int(n), **kw)
    print("%s: ticks %s status %s |q| %.3g |dq| %.3g" % (case, ticks, status, np.nanmax(np.abs(q - ref["q"])),
                                                          np.nanmax(np.abs(dq - ref["dq"]))))
    assert sure.all()
    assert np.array_equal(ticks, ref["ticks"]) and np.array_equal(status, ref["status"])        # (every instance)
    assert ticks.dtype == np.int32 and status.dtype == np.int32
    assert _close(q, ref["q"], Q_TOL) and _close(dq, ref["dq"], V_TOL) and _close(residual, ref["residual"], R_TOL)
    assert np.array_equal(Q, g[name + "/Q"], equal_nan=True) and np.array_equal(Y, g[name + "/Y"])      # (untouched)


# case -> (input set, is_qp, vmax, rk4, map)
ROLLOUT = {
    "pose_euler_free": ("pose", False, 0.0, False, None),
    "pose_euler_clamp": ("pose", False, 0.05, False, None),
    "pose_rk4_free": ("pose", False, 0.0, True, None),
    "pose_rk4_clamp": ("pose", False, 0.05, True, None),
    "feedback_euler_fed": ("feedback", False, 0.0, False, V.FB_IIWA),
    "qp_rk4_clamp": ("qp", True, 0.05, True, None),
}
DT, N_TICKS = 0.05, 5


@pytest.mark.parametrize("case", sorted(ROLLOUT))
def test_rollout_loop(iiwa_fk, ur5_fk, case):
    """B = 8, five ticks of dt = 0.05: the "pose" skill Euler and Runge-Kutta, free and clamped at 0.05; the feedback skill
    with the feed; ``skills.qp_skill`` Runge-Kutta, clamped"""
    g = np.load(os.path.join(GOLDEN, "rollout.npz"))
    name, qp, vmax, rk4, fb = ROLLOUT[case]
    spec = skills.qp_skill(iiwa_fk) if qp else _skill(name, iiwa_fk, ur5_fk)[0]
    Q, Y = g[name + "/Q"], g[name + "/Y"]
    host = H.rollout_loop(H.oracle_tick(spec, qp), qp, DT * np.arange(N_TICKS), Q, None, lambda i: Y, DT, vmax=vmax,
                          rk4=rk4, fb=fb)
    assert len(host) == N_TICKS and all(set(h) == {"q", "x", "dq", "dx", "slack", "flag"} for h in host)
    assert all(h["x"] is None and h["dx"] is None for h in host)
    for i, h in enumerate(host):
        assert np.array_equal(h["flag"], g[case + "/flag"][i]), i
        assert _close(h["q"], g[case + "/q"][i], Q_TOL) and _close(h["dq"], g[case + "/dq"][i], V_TOL), i
        if qp:
            assert _close(h["slack"], g[case + "/slack"][i], V_TOL), i
        else:
            assert h["slack"] is None
        if vmax > 0.0:
            assert np.abs(h["dq"]).max() <= vmax * (1.0 + 2.0 ** -50)    # (rk4: a mean of four clamped stages, rounded)
    if vmax > 0.0:
        assert any((np.abs(np.abs(h["dq"]) - vmax) < 1e-15).any() for h in host)        # (the clamp is reached)
    else:
        assert all(np.abs(h["dq"]).max() > 0.0 for h in host)           # (max_speed = 0 is "no clamp", not "no motion")
    if fb is not None:
        unfed = H.rollout_loop(H.oracle_tick(spec, qp), qp, DT * np.arange(N_TICKS), Q, None, lambda i: Y, DT)
        assert np.array_equal(unfed[0]["q"], host[0]["q"])              # (tick 0 reads what the caller gave)
        assert np.abs(unfed[-1]["q"] - host[-1]["q"]).max() > 1e3 * Q_TOL
