"""What the tests of ``converge_batch(..., group=G)`` / ``ik_batch(..., first_hit=True)`` share and what needs no GPU: the
group rule of include/clik.h in plain numpy, applied to the ``(ticks, status)`` of a run without it.  The host loop with
the rule in it is ``host_loops.converge_loop(..., group=G)``."""
import numpy as np

import converge_cases as K
from host_loops import CANCELLED        # noqa: F401

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
