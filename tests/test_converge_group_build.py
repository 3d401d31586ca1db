"""CPU: the converging rollouts with the group rule (clik_converge.hpp under -DCLIK_CONVERGE_GROUP=G) - their units
cross-compiled for gfx950 without scratch, one kernel each; their tags; the committed records; what the host refuses; and
the property that makes ``ik_batch(first_hit=True)`` return what ``ik_batch()`` returns: ``select_seeds`` behind the rule
picks what it picks without it."""
import os

import numpy as np
import pytest

from casclik_amd import jit, skills
from casclik_amd.controllers.base_controller import converge_group_request, padded_seeds, select_seeds

import converge_cases as K
import group_cases as GC


def _unit(name):
    req = jit.unit_request(K.make(name, skills.iiwa(), skills.ur5())[1])
    assert req.eligible
    return req, jit.CONVERGE_UNITS["converge", req.kind]["template"]


def _tag(req, tmpl, defines):
    return jit._cache_tag(req.init, req.extern, False, list(defines) + jit._sched_key(jit.sched_strategy(tmpl, req.init)), tmpl)


def test_the_defines_of_a_group():
    assert jit.converge_group_defines(1) == ()
    assert jit.CONVERGE_GROUPS == GC.GROUPS
    for G in GC.GROUPS:
        assert jit.converge_group_defines(G) == ("-DCLIK_CONVERGE_GROUP=%d" % G,)
    for bad in (0, 3, 128, -2):
        with pytest.raises(ValueError, match="group"):
            jit.converge_group_defines(bad)
    # the grouped variants have no rows of their own in the tables
    assert sorted(jit.CONVERGE_UNITS) == [("converge", "pinv"), ("converge", "qp")]
    assert all(u["defines"] == () for u in jit.CONVERGE_UNITS.values())


@pytest.mark.parametrize("name,G", [("pose", 16), ("stack", 4), ("qp", 4)])
def test_grouped_rollout_compiles_for_gfx950_without_scratch(name, G):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req, tmpl = _unit(name)
    res = jit.unit_resources(jit.unit_text(tmpl, req.init, req.extern), req.init, extra=jit.converge_group_defines(G))
    kernel = "qp_converge_static_kernel" if req.kind == "qp" else "pinv_converge_static_kernel"
    assert len(res) == 1 and all(kernel in k for k in res), sorted(res)
    for k, r in res.items():
        assert r["ScratchSize"] == 0, (k, r)
        print(name, G, k[-50:], r)


def test_a_group_size_the_header_does_not_take_does_not_compile():
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    req, tmpl = _unit("pose")
    with pytest.raises(RuntimeError, match="CLIK_CONVERGE_GROUP is one of"):
        jit.unit_resources(jit.unit_text(tmpl, req.init, req.extern), req.init, extra=("-DCLIK_CONVERGE_GROUP=3",))


def test_tags_of_the_grouped_units():
    tags = {}
    for name, G in (("pose", 16), ("stack", 4), ("qp", 4), ("pose", 2), ("pose", 1), ("stack", 1), ("qp", 1)):
        req, tmpl = _unit(name)
        tags[name, G] = _tag(req, tmpl, jit.converge_group_defines(G))
    assert len(set(tags.values())) == len(tags), tags
    # the default unit is asked for as before: no define, the tag of a request without any
    for name in ("pose", "stack", "qp"):
        req, tmpl = _unit(name)
        assert tags[name, 1] == _tag(req, tmpl, ())
        assert jit._request_id(req.init, req.extern, False, list(jit.converge_group_defines(1)), tmpl) == \
            jit._request_id(req.init, req.extern, False, [], tmpl)


def test_the_committed_records_hold_the_grouped_units_of_the_gpu_tests():
    tags = set(jit.recorded_tags())
    for name, G in GC.GPU_UNITS:
        req, tmpl = _unit(name)
        flags = list(jit.converge_group_defines(G))
        rid = jit._request_id(req.init, req.extern, False, flags, tmpl)
        assert os.path.exists(os.path.join(jit.CONVERGE_RECORDS, "req_%s.json" % rid)), (name, G)
        assert _tag(req, tmpl, flags) in tags, (name, G)
    # ik_batch(first_hit=True) with 13 seeds: groups of 16 of the pose skill
    assert padded_seeds(13) == 16 and ("pose", 16) in GC.GPU_UNITS


def test_what_the_host_refuses():
    for G in (1,) + GC.GROUPS:
        assert converge_group_request(G, 3 * G) == G and converge_group_request(np.int32(G), G) == G
    for bad in (0, -1, 3, 6, 128, True, 2.0, "4", None):
        with pytest.raises(ValueError, match="group must be one of"):
            converge_group_request(bad, 64)
    for G, B in ((2, 3), (4, 6), (16, 65), (64, 65), (64, 32)):
        with pytest.raises(ValueError, match="whole groups"):
            converge_group_request(G, B)
    assert [padded_seeds(S) for S in (1, 2, 3, 4, 5, 8, 13, 16, 17, 33, 64)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 64, 64]
    for S in (65, 100):
        with pytest.raises(ValueError, match="at most 64 seeds"):
            padded_seeds(S)


def test_the_rule_on_a_case_worked_by_hand():
    #        group 0: the winner at 3 cuts 7 and 9 short, the one that stopped at 2 stays
    ticks = [3, 7, 2, 9,
             # group 1: nobody arrives - untouched
             5, 5, 0, 5,
             # group 2: a tie at 4; a stall AT 4 happened behind the test of tick 4: cancelled; max_ticks at 6: cancelled
             4, 4, 4, 6,
             # group 3: the winner arrives at 0: everyone else stops at 0, a NaN at 0 stays
             0, 0, 8, 1]
    status = [0, 0, 2, 1,
              1, 2, 4, 3,
              0, 0, 2, 1,
              0, 4, 0, 3]
    t, s, first = GC.group_rule(ticks, status, 4)
    assert first.tolist() == [3, -1, 4, 0]
    assert t.tolist() == [3, 3, 2, 3, 5, 5, 0, 5, 4, 4, 4, 4, 0, 0, 0, 0]
    assert s.tolist() == [0, 5, 2, 5, 1, 2, 4, 3, 0, 0, 5, 5, 0, 4, 5, 5]
    assert t.dtype == np.int32 and s.dtype == np.int32
    # groups of one: nothing happens
    t1, s1, _ = GC.group_rule(ticks, status, 1)
    assert t1.tolist() == ticks and s1.tolist() == status


def _synthetic(rng, T, S):
    ticks = rng.integers(0, 5, T * S).astype(np.int32)
    status = rng.choice([0, 0, 1, 1, 2, 3, 4], T * S).astype(np.int32)
    residual = np.round(rng.uniform(0, 3, (T * S, 4)), 0) * 1e-3
    residual[status == 4] = np.nan
    return ticks, status, residual


def _select(ticks, status, residual, tol, S):
    import torch
    return select_seeds(torch.from_numpy(ticks), torch.from_numpy(status), torch.from_numpy(residual), tol, S).numpy()


@pytest.mark.parametrize("G", [2, 4, 16])
def test_select_seeds_picks_the_same_seed_behind_the_rule(G):
    """random (ticks, status, residual) with many ties: the rule changes no pick and nothing of what is returned for it"""
    rng = np.random.default_rng(G)
    tol = np.array([1e-3, np.inf, 0.0, 1e-2])
    seen = [0, 0, 0]
    for trial in range(30):
        T = 9
        ticks, status, residual = _synthetic(rng, T, G)
        if trial % 3 == 0:
            status[:G] = rng.choice([1, 2, 3, 4], G)         # (a group without a winner in every third trial)
            residual[:G] = np.round(rng.uniform(0, 3, (G, 4)), 0) * 1e-3
            residual[:G][status[:G] == 4] = np.nan
        gt, gs, first = GC.group_rule(ticks, status, G)
        # (a cancelled lane's residual is that of an earlier state: anything; it is never read where it could decide)
        gres = np.where((gs == GC.CANCELLED)[:, None], rng.uniform(0, 1, residual.shape), residual)
        want = _select(ticks, status, residual, tol, G)
        got = _select(gt, gs, gres, tol, G)
        assert got.tolist() == want.tolist() == K.select_seeds_loop(gt, gs, gres, tol, G).tolist(), trial
        at = np.arange(T) * G + want
        assert np.array_equal(gt[at], ticks[at]) and np.array_equal(gs[at], status[at])
        assert np.array_equal(gres[at], residual[at], equal_nan=True)
        # what the rule states about the lanes it stops
        cut = gs == GC.CANCELLED
        assert np.array_equal(gt[cut], np.repeat(first, G)[cut]) and not cut[np.repeat(first < 0, G)].any()
        assert np.array_equal(gt[~cut], ticks[~cut]) and np.array_equal(gs[~cut], status[~cut])
        seen[0] += int((first >= 0).sum())
        seen[1] += int((first < 0).sum())
        seen[2] += int((((gs == 0) & (gt == np.repeat(first, G))).reshape(T, G).sum(axis=1) > 1).sum())
    assert min(seen) > 0, seen


@pytest.mark.parametrize("S", [3, 5, 13])
def test_padding_with_copies_of_seed_0_changes_no_pick(S):
    rng = np.random.default_rng(100 + S)
    tol = np.array([1e-3, np.inf, 0.0, 1e-2])
    P = padded_seeds(S)
    pad = lambda A: np.concatenate([A.reshape((-1, S) + A.shape[1:]),                                   # noqa: E731
                                    np.repeat(A.reshape((-1, S) + A.shape[1:])[:, :1], P - S, axis=1)],
                                   axis=1).reshape((-1,) + A.shape[1:])
    for trial in range(30):
        T = 9
        ticks, status, residual = _synthetic(rng, T, S)
        if trial % 2 == 0:
            status[:S] = 0          # (seed 0 among the winners, so its copies tie with it)
            ticks[:S] = 2
            residual[:S] = 0.0
        want = _select(ticks, status, residual, tol, S)
        gt, gs, _ = GC.group_rule(pad(ticks), pad(status), P)
        got = _select(gt, gs, pad(residual), tol, P)
        assert (got < S).all() and got.tolist() == want.tolist(), trial
        assert np.array_equal(gt[np.arange(T) * P + got], ticks[np.arange(T) * S + want])
        assert np.array_equal(gs[np.arange(T) * P + got], status[np.arange(T) * S + want])
