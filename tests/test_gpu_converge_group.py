"""GPU: ``converge_batch(..., group=G)`` - the group rule of clik_converge.hpp: an instance's first converged sibling stops
it - and ``ik_batch(..., first_hit=True)`` on top of it.  Yardsticks: test 1 of tests/test_gpu_converge.py (the recording
rollout, which never stops, with the oracle's constraint values and the stop rule in numpy) followed by the rule in numpy
(group_cases.group_rule); a host loop on the oracle alone with the rule in it; ``ik_batch()`` without ``first_hit``; and
the properties the rule states."""
import ctypes as C
import os

import numpy as np
import pytest

from casclik_amd import jit, skills

import converge_cases as K
import group_cases as GC
import host_loops as H
from test_gpu_constraint_summary import TOL
from test_gpu_converge import _ctrl, _quiet_nan, _reference, _same_bits, _unpack
from test_gpu_rollout_record import Q_TOL, V_TOL

pytestmark = pytest.mark.gpu

DT = K.DT
KEYS = ("q", "dq", "flag", "ticks", "status", "residual")


def _rule_holds(ticks, status, G):
    """what the rule states about a launch's own output: a status-5 instance has the fewest ticks among its group's
    status-0 instances, and a group without a status-0 instance has no status-5 instance"""
    t, s = ticks.reshape(-1, G).astype(np.int64), status.reshape(-1, G)
    ok, cut = s == 0, s == GC.CANCELLED
    first = np.where(ok, t, np.iinfo(np.int64).max).min(axis=1)
    assert not cut[~ok.any(axis=1)].any()
    assert (t[cut] == np.broadcast_to(first[:, None], t.shape)[cut]).all()
    # (nobody runs on behind the test at which a sibling arrived)
    assert (t[ok.any(axis=1)] <= first[ok.any(axis=1), None]).all()


def _info(tag):
    info = jit._load(os.path.join(jit.CACHE, "clik_shape_%s.so" % tag)).clik_jit_converge_info
    info.restype, info.argtypes = C.c_longlong, [C.c_int]
    return info


# ---- 1: against the recording rollout, the oracle's stop rule and the group rule in numpy ---------------------------------
@pytest.mark.parametrize("name,G", GC.GPU_UNITS)
def test_a_group_stops_at_its_first_arrival(iiwa_fk, ur5_fk, name, G):
    spec, ctrl, qp = _ctrl(name, iiwa_fk, ur5_fk)
    ref = _reference(name, iiwa_fk, ur5_fk)
    rec, n = ref["rec"], ref["n"]
    left_out, seen = [0, 0], [0, 0, 0]
    for B in sorted({G, 64, 128}):
        cut = lambda A: None if A is None else np.ascontiguousarray(A[:B])          # noqa: E731
        call = lambda **kw: _unpack(ctrl.converge_batch(cut(ref["Q"]), cut(ref["Y"]), tol=ref["tol"], max_ticks=n, dt=DT,    # noqa: E731
                                                        virtual_var=cut(ref["X"]), **kw), qp, ref["X"] is not None)
        got = call(group=G)
        assert got["ticks"].dtype == np.int32 and got["status"].dtype == np.int32 and got["ticks"].shape == (B,)
        assert got["residual"].shape == (B, ref["tol"].size) and got["residual"].dtype == np.float64
        want_t, want_s, first = GC.group_rule(ref["ticks"][:B], ref["status"][:B], G)
        sure = GC.whole_groups(ref["sure"][:B], G)
        left_out[0] += int((~sure).sum())
        left_out[1] += B
        assert np.array_equal(got["ticks"][sure], want_t[sure]), (name, G, B)
        assert np.array_equal(got["status"][sure], want_s[sure]), (name, G, B)
        assert set(np.unique(got["status"])) <= {0, 1, GC.CANCELLED}
        _rule_holds(got["ticks"], got["status"], G)
        seen[0] += int((first >= 0).sum())
        seen[1] += int((first < 0).sum())
        seen[2] += int((got["status"] == GC.CANCELLED).sum())
        # the floats at the tick the launch itself stopped at: a cancelled instance holds the state after r* ticks, the
        # velocity and mode of tick r* - 1 and the dist values of the test of tick r*
        r, b = got["ticks"].astype(int), np.arange(B)
        assert (r >= 0).all() and (r <= n).all()
        last = np.maximum(r - 1, 0)
        moved = (r > 0)[:, None]
        eq = np.abs(got["q"] - ref["states"][r, b]).max()
        ev = np.abs(got["dq"] - np.where(moved, rec["dq"][last, b], 0.0)).max()
        at = K.oracle_values(spec, 0.0, got["q"][None], None if got["x"] is None else got["x"][None], cut(ref["Y"]))
        er = np.abs(got["residual"] - K.distances(*at)[0]).max()
        # (another compilation of the same tick: are the bits those of the default unit wherever the rule changed nothing?)
        plain = call()
        same = (got["ticks"] == plain["ticks"]) & (got["status"] == plain["status"])
        bits = all(_same_bits(np.ascontiguousarray(got[k][same]), np.ascontiguousarray(plain[k][same])) for k in KEYS)
        print("%s G=%d B=%d: |q| %.3e |dq| %.3e |residual| %.3e, ticks %d .. %d (without the rule .. %d), %d cancelled; "
              "bits of the %d untouched instances equal to the default unit's: %s"
              % (name, G, B, eq, ev, er, r.min(), r.max(), plain["ticks"].max(), (got["status"] == GC.CANCELLED).sum(),
                 same.sum(), bits))
        assert eq < Q_TOL and ev < V_TOL and er < TOL
        flag = rec["status" if qp else "mode"]
        assert np.array_equal(got["flag"], np.where(r > 0, flag[last, b], 0 if qp else -1))
        if ref["X"] is not None:
            assert np.abs(got["x"] - ref["xs"][r, b]).max() < Q_TOL
            assert np.abs(got["dx"] - np.where(moved, rec["dx"][last, b], 0.0)).max() < V_TOL
    print("%s G=%d: %d groups with an arrival, %d without, %d instances cancelled; %d of %d instances left out of the "
          "integer comparisons" % (name, G, *seen, *left_out))
    assert seen[0] > 0 and seen[2] > 0          # (the inputs are worth the run)
    assert left_out[0] <= 0.01 * left_out[1], left_out
    # the default unit's tag is where it was; each loaded unit says which group it was compiled for
    assert _info(ctrl._kernels["converge"])(6) == 1 and _info(ctrl._converge_units[G][0])(6) == G
    assert ctrl._converge_units[G][0] != ctrl._kernels["converge"]


# ---- 2: against a host loop that involves no device code ------------------------------------------------------------------
def test_a_host_loop_with_the_rule_stops_at_the_same_ticks(iiwa_fk, ur5_fk):
    """as test 2 of tests/test_gpu_converge.py (the margin 1e-8 is derived there), an instance that comes that close to a
    tolerance leaving its whole group out"""
    spec, ctrl, _ = _ctrl("pose", iiwa_fk, ur5_fk)
    case = K.CASES["pose"]
    B, G, n, margin = 128, 2, case["max_ticks"], 1e-8
    Q, _, Y = K.inputs("pose", iiwa_fk, B, seed=4)
    tol = K.tolerances(spec, case["tol"])
    hq, hdq, hticks, hstatus, hres, sure = H.converge_loop(spec, ctrl.options, Q, Y, tol, n, margin=margin, group=G)
    sure = GC.whole_groups(sure, G)
    ok = (hstatus == 0).reshape(-1, G)
    ties = ok.all(axis=1) & (hticks.reshape(-1, G)[:, 0] == hticks.reshape(-1, G)[:, 1])
    print("host loop with G=2: %d groups with an arrival, %d without, %d ties, %d instances cancelled"
          % (ok.any(axis=1).sum(), (~ok.any(axis=1)).sum(), ties.sum(), (hstatus == GC.CANCELLED).sum()))
    assert ok.any(axis=1).any() and (~ok.any(axis=1)).any() and ties.any() and (hstatus == GC.CANCELLED).any()
    got = _unpack(ctrl.converge_batch(Q, Y, tol=tol, max_ticks=n, dt=DT, group=G), False, False)
    print("%d of %d left out; |q| %.3e |dq| %.3e |residual| %.3e" % (
        (~sure).sum(), B, np.abs(got["q"] - hq)[sure].max(), np.abs(got["dq"] - hdq)[sure].max(),
        np.abs(got["residual"] - hres)[sure].max()))
    assert (~sure).sum() <= 0.01 * B
    assert np.array_equal(got["ticks"][sure], hticks[sure]) and np.array_equal(got["status"][sure], hstatus[sure])
    assert np.abs(got["q"] - hq)[sure].max() < Q_TOL and np.abs(got["dq"] - hdq)[sure].max() < V_TOL
    assert np.abs(got["residual"] - hres)[sure].max() < margin


# ---- 3: ik_batch(first_hit=True) against ik_batch() -------------------------------------------------------------------------
def test_first_hit_returns_what_ik_batch_returns(iiwa_fk, ur5_fk):
    import torch
    spec, ctrl, _ = _ctrl("pose", iiwa_fk, ur5_fk)
    Y, seeds, tol, n = GC.first_hit_seeds(iiwa_fk)
    T, S = Y.shape[0], seeds.shape[0]
    assert (T, S) == (5, 13)
    kw = dict(tol=tol, max_ticks=n, dt=DT)
    q0, info0 = ctrl.ik_batch(Y, seeds, **kw)
    q1, info1 = ctrl.ik_batch(Y, seeds, first_hit=True, **kw)
    print("seed", info0["seed"], info1["seed"], "ticks", info0["ticks"], info1["ticks"], "status", info0["status"],
          info1["status"])
    # both paths of the rule: a target none of whose seeds arrives (nothing is cancelled) and targets with an arrival
    assert (info0["status"] != 0).any() and (info0["status"] == 0).any()
    for key in ("seed", "ticks", "status"):
        assert info1[key].dtype == np.int32 and np.array_equal(info0[key], info1[key]), key
    assert q1.shape == (T, 7) and info1["residual"].shape == info0["residual"].shape
    eq, er = np.abs(q1 - q0).max(), np.abs(info1["residual"] - info0["residual"]).max()
    print("first_hit against ik_batch(): |q| %.3e |residual| %.3e, same bits: %s" % (
        eq, er, _same_bits(q0, q1) and _same_bits(info0["residual"], info1["residual"])))
    assert eq < Q_TOL and er < TOL
    # the launch behind it: 16 lanes a target, the copies of seed 0 do what seed 0 does, and seeds were cut short
    P = 16
    padded = np.concatenate([seeds, np.repeat(seeds[:1], P - S, axis=0)])
    Q0 = np.ascontiguousarray(np.broadcast_to(padded[None], (T, P, 7)).reshape(T * P, 7))
    raw = _unpack(ctrl.converge_batch(Q0, np.repeat(Y, P, axis=0), group=P, **kw), False, False)
    _rule_holds(raw["ticks"], raw["status"], P)
    for key in KEYS:
        lanes = raw[key].reshape((T, P) + raw[key].shape[1:])
        for s in range(S, P):
            assert _same_bits(np.ascontiguousarray(lanes[:, s]), np.ascontiguousarray(lanes[:, 0])), (key, s)
    cancelled = (raw["status"] == GC.CANCELLED).reshape(T, P)
    print("cancelled seeds per target", cancelled.sum(axis=1))
    assert cancelled.any() and not cancelled[info0["status"] != 0].any()
    # seeds per target, device tensors in and out
    dev = ctrl._device
    seeds3 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(seeds[None], (T, S, 7)))).to(dev)
    qd, infod = ctrl.ik_batch(torch.from_numpy(Y).to(dev), seeds3, first_hit=True, **kw)
    assert isinstance(qd, torch.Tensor) and qd.device == dev and _same_bits(qd.cpu().numpy(), q1)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in infod.values())
    for key, v in info1.items():
        assert _same_bits(infod[key].cpu().numpy(), v), key
    # what the host refuses
    with pytest.raises(ValueError, match="at most 64 seeds"):
        ctrl.ik_batch(Y, np.zeros((65, 7)), first_hit=True, **kw)
    with pytest.raises(ValueError, match="do not pass group"):
        ctrl.ik_batch(Y, seeds, first_hit=True, group=16, **kw)


# ---- 4: properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,G", [("stack", 4), ("qp", 4)])
def test_same_bits_every_call_and_a_group_alone_or_in_a_batch(iiwa_fk, ur5_fk, name, G):
    spec, ctrl, qp = _ctrl(name, iiwa_fk, ur5_fk)
    ref = _reference(name, iiwa_fk, ur5_fk)
    B = 128
    Q, Y = ref["Q"][:B], ref["Y"][:B]
    call = lambda q, y, **kw: _unpack(ctrl.converge_batch(q, y, tol=ref["tol"], max_ticks=ref["n"], dt=DT, **kw), qp, False)    # noqa: E731
    one, two = call(Q, Y, group=G), call(Q, Y, group=G)
    assert (one["status"] == GC.CANCELLED).any()
    for key in KEYS:
        assert _same_bits(one[key], two[key]), key
    for g in (0, 1, 7, 15, 16, 17, 31):
        rows = slice(g * G, (g + 1) * G)
        alone = call(np.ascontiguousarray(Q[rows]), np.ascontiguousarray(Y[rows]), group=G)
        for key in KEYS:
            assert _same_bits(np.ascontiguousarray(one[key][rows]), alone[key]), (key, g)
    # group=1 is the call without it, also right behind a grouped call (the default unit is attached again)
    plain, single = call(Q, Y), call(Q, Y, group=1)
    assert not (plain["status"] == GC.CANCELLED).any()
    for key in KEYS:
        assert _same_bits(plain[key], single[key]), key
    three = call(Q, Y, group=G)
    for key in KEYS:
        assert _same_bits(one[key], three[key]), key


def test_a_nan_seed_cancels_nobody_and_is_not_cancelled(iiwa_fk, ur5_fk):
    spec, ctrl, _ = _ctrl("pose", iiwa_fk, ur5_fk)
    ref = _reference("pose", iiwa_fk, ur5_fk)
    B, G = 64, 16
    Q, Y = ref["Q"][:B].copy(), ref["Y"][:B].copy()
    call = lambda q, y, **kw: _unpack(ctrl.converge_batch(q, y, tol=ref["tol"], max_ticks=ref["n"], dt=DT, **kw), False, False)    # noqa: E731
    clean = call(Q, Y, group=G)
    # group 1: a NaN in the instance that runs longest there (so not the one whose arrival stops the others)
    bad = G + int(np.argmax(ref["ticks"][G:2 * G]))
    assert ref["ticks"][bad] > GC.group_rule(ref["ticks"][:B], ref["status"][:B], G)[2][1] >= 0
    # group 2: an instance that stands on its target - everyone else of the group is cancelled at tick 0 - and a NaN
    # next to it, which the test of tick 0 stops itself: it keeps status 4
    home, bad0 = 2 * G + 3, 2 * G + 9
    M = iiwa_fk["chain"].fk_numeric(Q[home])
    Y[home, :3], Y[home, 3:] = M[:3, 3], skills.quat_from_matrix(M[:3, :3])
    Q[bad, 3] = np.nan
    Y[bad0, 1] = np.nan
    got = call(Q, Y, group=G)
    _rule_holds(got["ticks"], got["status"], G)
    for b in (bad, bad0):
        assert got["status"][b] == 4 and got["ticks"][b] == 0
        for key in ("q", "dq", "residual"):
            assert _quiet_nan(got[key][b]), (key, got[key][b])
    # groups 0, 1 and 3 but for the NaN instance: the bits of the clean launch
    keep = np.ones(B, dtype=bool)
    keep[2 * G:3 * G] = False
    keep[bad] = False
    for key in KEYS:
        assert _same_bits(np.ascontiguousarray(got[key][keep]), np.ascontiguousarray(clean[key][keep])), key
        assert not np.isnan(clean[key].astype(float)).any(), key
    # group 2: the winner at tick 0, the NaN, and the others cancelled where they started (but for one that starts within
    # the tolerance itself, if there is one)
    rest = np.setdiff1d(np.arange(2 * G, 3 * G), [home, bad0])
    there = (ref["ticks"][rest] == 0) & (ref["status"][rest] == 0)
    assert got["status"][home] == 0 and got["ticks"][home] == 0 and (~there).sum() >= G // 2
    assert np.array_equal(got["status"][rest], np.where(there, 0, GC.CANCELLED)) and (got["ticks"][rest] == 0).all()
    assert _same_bits(np.ascontiguousarray(got["q"][rest]), np.ascontiguousarray(Q[rest])) and (got["dq"][rest] == 0.0).all()
    assert (got["flag"][rest] == -1).all() and (got["residual"][rest][~there].max(axis=1) > ref["tol"].max()).all()


def test_what_the_controller_refuses(iiwa_fk, ur5_fk):
    spec, ctrl, _ = _ctrl("pose", iiwa_fk, ur5_fk)
    ref = _reference("pose", iiwa_fk, ur5_fk)
    Q, Y = ref["Q"][:65], ref["Y"][:65]
    for bad in (0, 3, 128, True, 4.0):
        with pytest.raises(ValueError, match="group must be one of"):
            ctrl.converge_batch(Q[:64], Y[:64], tol=ref["tol"], max_ticks=2, dt=DT, group=bad)
    for G in (2, 16, 64):
        with pytest.raises(ValueError, match="whole groups"):
            ctrl.converge_batch(Q, Y, tol=ref["tol"], max_ticks=2, dt=DT, group=G)
