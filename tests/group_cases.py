"""What the tests of ``converge_batch(..., group=G)`` / ``ik_batch(..., first_hit=True)`` share and what needs no GPU: the
group rule of include/clik.h in plain numpy, applied to the ``(ticks, status)`` of a run without it, and the host loop of
``converge_cases`` with the rule added."""
import numpy as np

import converge_cases as K
from oracle import clik_oracle

CANCELLED = 5
GROUPS = (2, 4, 8, 16, 32, 64)

# (case of converge_cases.CASES, group size) of the grouped units the GPU tests run: the committed records hold each
GPU_UNITS = (("pose", 2), ("pose", 16), ("pose", 64), ("stack", 4), ("qp", 4), ("virtual", 8))


def group_rule(ticks, status, G):
    """``(ticks, status, first)`` of a launch with groups of ``G`` instances from the ``ticks`` and ``status`` ``[B]`` of the
    same launch without the rule (``B % G == 0``); ``first [B // G]`` is r*, the fewest ticks among a group's status-0
    instances, -1 for a group without one.  An instance is still active behind the test of tick r* - and stops there with
    status 5 - when it stopped at a later tick, or at r* itself by the solve (stalled 2, infeasible 3: the solve of tick r*
    comes behind the rule).  Everything else stays."""
    t = np.array(ticks, dtype=np.int64).reshape(-1, G)
    s = np.array(status, dtype=np.int64).reshape(-1, G)
    ok = s == 0
    has = ok.any(axis=1)
    first = np.where(has, np.where(ok, t, np.iinfo(np.int64).max).min(axis=1), -1)
    cut = has[:, None] & ((t > first[:, None]) | ((t == first[:, None]) & ((s == 2) | (s == 3))))
    t = np.where(cut, first[:, None], t)
    s = np.where(cut, CANCELLED, s)
    return t.reshape(-1).astype(np.int32), s.reshape(-1).astype(np.int32), first


def whole_groups(sure, G):
    """``sure`` of every instance of a group ANDed and spread over the group: one instance too close to a tolerance for the
    oracle to decide leaves its whole group out"""
    return np.repeat(np.asarray(sure, dtype=bool).reshape(-1, G).all(axis=1), G)


def host_loop(spec, options, Q, Y, tol, max_ticks, G, dt=K.DT, max_speed=0.0, min_step=0.0, t=0.0, margin=K.MARGIN):
    """``converge_cases.host_loop`` - every instance on its own, the oracle's constraint values and its solve, no device
    code - with the group rule behind the stop test of every tick.  Returns ``(q, dq, ticks, status, residual, sure)``."""
    B = Q.shape[0]
    assert B % G == 0
    q, dq = Q.copy(), np.zeros_like(Q)
    ticks, status = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    residual, sure = np.zeros((B, tol.size)), np.ones(B, dtype=bool)
    for r in range(max_ticks + 1):
        go = np.nonzero(status < 0)[0]
        if go.size == 0:
            break
        e, lo, hi, is_set = K.oracle_values(spec, t, q[None, go], None, None if Y is None else Y[go])
        d = K.distances(e, lo, hi, is_set)[0]
        residual[go] = d
        sure[go] &= ~(np.abs(d - tol) < margin).any(axis=1)
        bad = ~np.isfinite(e[0]).all(axis=1)
        with np.errstate(invalid="ignore"):
            met = (d <= tol).all(axis=1)
        status[go] = np.where(bad, 4, np.where(met, 0, 1 if r == max_ticks else -1))
        ticks[go] = r
        # the rule: whoever is still running next to an instance of its group that has arrived stops here
        won = np.repeat((status == 0).reshape(-1, G).any(axis=1), G)
        status[(status < 0) & won] = CANCELLED
        go = np.nonzero(status < 0)[0]
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


def first_hit_seeds(fk):
    """(targets [5, 7], seeds [13, 7], tol, max_ticks) of the ``first_hit`` test: the targets of ``converge_cases.ik_inputs``
    and seeds close enough to the state they were drawn around (at most 0.06 rad a joint) that every trajectory is a plain
    contraction - two compilations of the same tick stay together on it, which they need not on the far seeds of
    ``ik_inputs`` itself"""
    Y = K.ik_inputs(fk)[0]
    lo, hi = np.asarray(fk["lower"], float), np.asarray(fk["upper"], float)
    star = np.random.default_rng(11).uniform(0.5 * lo, 0.5 * hi)
    seeds = star + (10.0 ** np.linspace(-3.0, -1.2, 16))[::-1][:, None] * np.random.default_rng(12).normal(size=(16, 7))
    return Y, np.ascontiguousarray(seeds[:13]), 1e-5, 12
