"""GPU: ``options["velocity_feedback"]`` - inside an on-device loop tick k + 1 reads, in the entries of ``input_var`` the
map names, the velocity tick k was integrated with (include/clik.h has the rule).  Both controllers, every loop that runs
in one launch: ``rollout_batch`` plain, recording, with a per-tick target, summarising, Euler and Runge-Kutta, and
``converge_batch``.

The yardstick is the host loop the launch replaces: one ``solve_batch`` call per tick (rk4: per stage) that rewrites the
fed entries between ticks (host_loops.rollout_loop with the map), with the tolerances of tests/test_gpu_rollout_record.py:
|q| < 1e-9, |dq| < 1e-7.  The skills are made so that the feed matters: on the oracle, feeding back against frozen entries
moves q by 1.8e-3 (QP skill: an acceleration limit around the last velocity) and 1.1e-3 (pinv skill: a null-space pull
towards it), so a launch that ignores the option misses Q_TOL by six orders of magnitude.  iiwa inputs from
``converge_cases.reach_inputs(fk, 100)``; B = 100 (two waves, one partial) and B = 1; 11 ticks; dt = 0.008."""
import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import jit, skills

import converge_cases as K
import host_loops as H
import velocity_feedback_cases as V
from test_gpu_constraint_summary import _check, _oracle, _reduce, _tolerances
from test_gpu_rollout_record import Q_TOL, V_TOL
from tolerances import LAST, pinv_close, qp_close

pytestmark = pytest.mark.gpu

DT, N = V.DT, V.N_TICKS
TIMES = DT * np.arange(N)
BATCHES = (100, 1)


@pytest.fixture(scope="module")
def cases(iiwa_fk, ur5_fk):
    made = {}

    def get(name):
        if name not in made:
            spec, ctrl, qp, fb = V.make(name, iiwa_fk, ur5_fk)
            ctrl.setup_problem_functions()
            ctrl.setup_solver()
            made[name] = (spec, ctrl, qp, fb)
        return made[name]
    return get


_HOST = {}


def _host(cases, iiwa_fk, name, method, B=100):
    """the host loop of a skill and method at B = 100, computed once and shared (B = 1 is its first instance: every
    instance is on its own)"""
    key = (name, method)
    if key not in _HOST:
        spec, ctrl, qp, fb = cases(name)
        Q, Y = V.iiwa_inputs(iiwa_fk, 100)
        _HOST[key] = H.rollout_loop(H.controller_tick(ctrl, qp), qp, TIMES, Q, None, lambda i: Y, DT, rk4=method == "rk4",
                                    fb=fb)
    return [{k: (None if v is None else v[:B]) for k, v in h.items()} for h in _HOST[key]]


def _unpack(res, qp, has_x=False):
    """(q, x, dq, dx, flag, rest) of what rollout_batch returns"""
    if has_x:
        q, x, dq, dx = res[:4]
        return q, x, dq, dx, res[5 if qp else 4], res[(6 if qp else 5):]
    q, dq = res[:2]
    return q, None, dq, None, res[3 if qp else 2], res[(4 if qp else 3):]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _against(host, k, rec, what):
    """entry r of the records against the host loop's tick (r + 1) * k, every instance"""
    R = len(host) // k
    assert rec["q"].shape[0] == R and rec["dq"].shape[0] == R
    for r in range(R):
        h = host[(r + 1) * k - 1]
        eq, ev = np.abs(rec["q"][r] - h["q"]).max(), np.abs(rec["dq"][r] - h["dq"]).max()
        print("%s record %d of every %d: |q| %.3g |dq| %.3g" % (what, r, k, eq, ev))
        assert eq < Q_TOL and ev < V_TOL, (what, k, r, eq, ev)
        if h["x"] is not None:
            assert np.abs(rec["x"][r] - h["x"]).max() < Q_TOL and np.abs(rec["dx"][r] - h["dx"]).max() < V_TOL, (what, k, r)


# ---- 1: the host loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("name", ["qp", "pinv"])
def test_launch_matches_the_host_loop_that_rewrites_the_fed_entries(cases, iiwa_fk, name, method):
    spec, ctrl, qp, fb = cases(name)
    for B in BATCHES:
        Q, Y = V.iiwa_inputs(iiwa_fk, 100)
        Q, Y = Q[:B], Y[:B]
        host = _host(cases, iiwa_fk, name, method, B)
        flag_name = "status" if qp else "mode"
        for k in (1, 4):
            res = ctrl.rollout_batch(TIMES, Q, input_var=Y, dt=DT, method=method, record_every=k)
            q, _, dq, _, flag, rest = _unpack(res, qp)
            rec = rest[-1]
            _against(host, k, rec, "%s %s B=%d" % (name, method, B))
            eq, ev = np.abs(q - host[-1]["q"]).max(), np.abs(dq - host[-1]["dq"]).max()
            print("%s %s B=%d final: |q| %.3g |dq| %.3g" % (name, method, B, eq, ev))
            assert eq < Q_TOL and ev < V_TOL
            if qp:
                assert (flag == 0).all() and (rec[flag_name] == 0).all()
                assert all((h["flag"] == 0).all() for h in host)
            elif method == "euler":
                for r in range(N // k):
                    assert np.array_equal(rec[flag_name][r], host[(r + 1) * k - 1]["flag"])
        # the plain launch - no record, no per-tick target - is fed as well
        plain = ctrl.rollout_batch(TIMES, Q, input_var=Y, dt=DT, method=method)
        assert np.abs(plain[0] - host[-1]["q"]).max() < Q_TOL and np.abs(plain[1] - host[-1]["dq"]).max() < V_TOL
        if qp and method == "euler":
            # on the launch's own output: the limit is reached, and never passed
            rec = ctrl.rollout_batch(TIMES, Q, input_var=Y, dt=DT, record_every=1)[-1]
            v = np.concatenate([Y[None, :, 7:], rec["dq"]])
            step = np.abs(np.diff(v, axis=0))
            print("QP B=%d: largest |dq_k - dq_{k-1}| - a_dt = %.3g, (tick, instance) pairs with a joint at the limit %.0f %%"
                  % (B, step.max() - V.A_DT, 100.0 * (np.abs(step - V.A_DT) < 1e-9).any(axis=2).mean()))
            if B == 100:
                # (61 % of the 100 instances reach the limit at some tick on the oracle; the first one - the batch of
                # one - starts 1e-4 rad from its target and never asks for that much)
                assert (np.abs(step - V.A_DT) < 1e-9).any()
            assert step.max() <= V.A_DT + V_TOL
            assert (rec["status"] == 0).all()


# ---- 2: an independent yardstick ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp", "pinv"])
def test_every_tick_is_the_oracle_s_at_the_fed_target(cases, iiwa_fk, name):
    """The oracle's loop, tick by tick at the launch's own states, so that every tick is held to the suite's own rule
    (tolerances.py: per instance max(FLOOR, FACTOR u kappa)) and nothing accumulates: tick k of the oracle starts from
    record k - 1 and reads record k - 1's velocity in the fed entries, as the rule says the launch does."""
    spec, ctrl, qp, fb = cases(name)
    Q, Y = V.iiwa_inputs(iiwa_fk, 100)
    res = ctrl.rollout_batch(TIMES, Q, input_var=Y, dt=DT, record_every=1)
    rec = res[-1]
    close = qp_close if qp else pinv_close
    tick = H.oracle_tick(spec, qp, {})
    q, y = Q, Y
    for k in range(N):
        ref, _, _, flag = tick(float(TIMES[k]), q, None, y)
        if qp:
            assert (flag == 0).all()
        ok = close(rec["dq"][k], ref)
        print("%s tick %d: %s" % (name, k, dict(LAST)))
        assert ok, (name, k, dict(LAST))
        assert np.abs(rec["q"][k] - (q + rec["dq"][k] * DT)).max() < 1e-15 * 8
        q, y = rec["q"][k], H.feed(Y, fb, rec["dq"][k])


# ---- 3: chunking ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("name", ["qp", "pinv"])
def test_a_launch_is_two_launches_whose_second_is_fed_the_first_one_s_velocity(cases, iiwa_fk, name, method):
    spec, ctrl, qp, fb = cases(name)
    Q, Y = V.iiwa_inputs(iiwa_fk, 100)
    kw = dict(dt=DT, method=method)
    whole = ctrl.rollout_batch(TIMES, Q, input_var=Y, **kw)
    first = ctrl.rollout_batch(TIMES[:4], Q, input_var=Y, **kw)
    second = ctrl.rollout_batch(TIMES[4:], first[0], input_var=H.feed(Y, fb, first[1]), **kw)
    if qp:
        # (the second launch's first tick is a cold solve, the whole launch's a hot one: the same minimiser to rounding)
        eq, ev = np.abs(whole[0] - second[0]).max(), np.abs(whole[1] - second[1]).max()
        print("QP %s 11 = 4 + 7: |q| %.3g |dq| %.3g" % (method, eq, ev))
        assert eq < Q_TOL and ev < V_TOL and (second[3] == 0).all()
    else:
        assert _same_bits(whole[0], second[0]) and _same_bits(whole[1], second[1])
        assert np.array_equal(whole[2], second[2])


# ---- 4: a moving target -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp", "pinv"])
def test_a_per_tick_target_keeps_its_other_entries_and_loses_the_fed_ones(cases, iiwa_fk, name):
    spec, ctrl, qp, fb = cases(name)
    Q, Y = V.iiwa_inputs(iiwa_fk, 100)
    rng = np.random.default_rng(17)
    Y3 = np.repeat(Y[None], N, axis=0)
    Y3[:, :, :3] += 0.002 * np.arange(N)[:, None, None] * rng.normal(size=(1, 100, 3))     # (the pose target drifts)
    Y3[1:, :, 7:] = rng.normal(scale=50.0, size=(N - 1, 100, 7))                           # (garbage where the feed goes)
    host = H.rollout_loop(H.controller_tick(ctrl, qp), qp, TIMES, Q, None, lambda i: Y3[i], DT, fb=fb)
    for B in BATCHES:
        res = ctrl.rollout_batch(TIMES, Q[:B], input_var=np.ascontiguousarray(Y3[:, :B]), dt=DT, record_every=1)
        hostB = [{k: (None if v is None else v[:B]) for k, v in h.items()} for h in host]
        _against(hostB, 1, res[-1], "%s moving target B=%d" % (name, B))
        assert np.abs(res[0] - hostB[-1]["q"]).max() < Q_TOL and np.abs(res[1] - hostB[-1]["dq"]).max() < V_TOL
    # the drift is seen: the same launch with the first record's target throughout ends elsewhere
    still = ctrl.rollout_batch(TIMES, Q, input_var=Y, dt=DT)
    assert np.abs(still[0] - host[-1]["q"]).max() > 1e-6


# ---- 5: a permutation of the instances ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp", "pinv"])
def test_a_permutation_of_the_instances_permutes_the_results(cases, iiwa_fk, name):
    spec, ctrl, qp, fb = cases(name)
    Q, Y = V.iiwa_inputs(iiwa_fk, 100)
    perm = np.random.default_rng(23).permutation(100)
    one = ctrl.rollout_batch(TIMES, Q, input_var=Y, dt=DT, record_every=1)
    two = ctrl.rollout_batch(TIMES, Q[perm], input_var=Y[perm], dt=DT, record_every=1)
    for a, b in zip(one[:-1], two[:-1]):
        if a is not None:
            assert _same_bits(np.ascontiguousarray(a[perm]), b)
    for key in one[-1]:
        assert _same_bits(np.ascontiguousarray(one[-1][key][:, perm]), two[-1][key]), key


# ---- 6: the summarising launch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "rk4"])
@pytest.mark.parametrize("name", ["qp", "pinv"])
def test_the_summary_is_of_the_trajectory_the_recording_launch_returns(cases, iiwa_fk, name, method):
    """One launch that summarises, records and feeds (the composing hook): its records are the recording launch's to the
    host loop's tolerances, and its summary is the numpy reduction of the oracle's values at its own records, the
    comparison and bounds of tests/test_gpu_rollout_summary.py.  Record r of the summary is what tick r acts on: the
    state before it and the target it reads, fed entries included."""
    spec, ctrl, qp, fb = cases(name)
    for B in BATCHES:
        Q, Y = V.iiwa_inputs(iiwa_fk, 100)
        Q, Y = Q[:B], Y[:B]
        kw = dict(input_var=Y, dt=DT, method=method, record_every=1)
        recd = ctrl.rollout_batch(TIMES, Q, **kw)
        first = ctrl.rollout_batch(TIMES, Q, summary=True, **kw)
        rec = first[-2]
        for key in ("q", "dq"):
            err = np.abs(rec[key] - recd[-1][key]).max()
            assert err < (Q_TOL if key == "q" else V_TOL), (key, err)
        Qs = np.concatenate([Q[None], rec["q"][:-1]])
        Ys = np.stack([Y] + [H.feed(Y, fb, rec["dq"][r]) for r in range(N - 1)])
        orc = _oracle(spec, TIMES, Qs, None, Ys)
        tol = _tolerances(*orc)
        res = ctrl.rollout_batch(TIMES, Q, summary=True, summary_tol=tol, **kw)
        for key in rec:
            assert _same_bits(res[-2][key], rec[key]), key
        ref, sure = _reduce(*orc, tol)
        left_out = [0, 0]
        _check(name, "%s B=%d fed" % (method, B), res[-1], ref, sure, N, left_out)
        assert left_out[0] <= 0.01 * left_out[1], left_out
        # and without records: the same summary, bit for bit
        bare = ctrl.rollout_batch(TIMES, Q, input_var=Y, dt=DT, method=method, summary=True, summary_tol=tol)
        for key in bare[-1]:
            assert _same_bits(bare[-1][key], res[-1][key]), key


# ---- 7: a virtual variable ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_the_rate_of_a_virtual_variable_is_fed(cases, method):
    spec, ctrl, qp, fb = cases("path")
    assert ctrl.descriptor.n_x == 1 and fb == V.FB_PATH
    Q, X, Y = V.path_inputs(100)
    host = H.rollout_loop(H.controller_tick(ctrl, False), False, TIMES, Q, X, lambda i: Y, DT, rk4=method == "rk4", fb=fb)
    # the feed is what the skill turns on: the parameter's rate follows ds_k = 0.5 ds_{k-1} + 0.002 from rest towards its
    # fixed point 0.004 (within 2^-11 of it after 11 ticks); with nothing fed it would stay at 0.002
    assert np.abs(host[0]["dx"] - 0.002).max() < 1e-6 and np.abs(host[-1]["dx"] - 0.004).max() < 1e-5
    for B in BATCHES:
        hostB = [{k: (None if v is None else v[:B]) for k, v in h.items()} for h in host]
        res = ctrl.rollout_batch(TIMES, Q[:B], input_var=Y[:B], virtual_var=X[:B], dt=DT, method=method, record_every=1)
        q, x, dq, dx, _, rest = _unpack(res, False, has_x=True)
        _against(hostB, 1, rest[-1], "path %s B=%d" % (method, B))
        assert np.abs(q - hostB[-1]["q"]).max() < Q_TOL and np.abs(x - hostB[-1]["x"]).max() < Q_TOL
        assert np.abs(dq - hostB[-1]["dq"]).max() < V_TOL and np.abs(dx - hostB[-1]["dx"]).max() < V_TOL


# ---- 7b: the times on the device -------------------------------------------------------------------------------------------------
def test_a_launch_with_the_times_on_the_device_is_fed(cases, iiwa_fk):
    """``time_on_device``: the launch goes through ``clik_pinv_rollout_batch_dev``, which hands a launch without records
    and per-tick targets to the plain kernels - with the option it must still be the lane kernel that feeds"""
    import torch
    spec, ctrl, qp, fb = cases("timed")
    assert ctrl._time_kernel is not None and ctrl.descriptor.n_tslots > 0
    Q, Y = V.iiwa_inputs(iiwa_fk, 100)
    times = 0.3 + TIMES
    host = H.rollout_loop(H.controller_tick(ctrl, False), False, times, Q, None, lambda i: Y, DT, fb=fb)
    frozen = H.rollout_loop(H.controller_tick(ctrl, False), False, times, Q, None, lambda i: Y, DT, fb=(-1,) * 7)
    assert np.abs(frozen[-1]["q"] - host[-1]["q"]).max() > 1e-6            # (the feed matters here too)
    for tv in (times, torch.from_numpy(times).to(ctrl._device)):
        plain = ctrl.rollout_batch(tv, Q, input_var=Y, dt=DT)
        assert np.abs(plain[0] - host[-1]["q"]).max() < Q_TOL and np.abs(plain[1] - host[-1]["dq"]).max() < V_TOL
        res = ctrl.rollout_batch(tv, Q, input_var=Y, dt=DT, record_every=1)
        _against(host, 1, res[-1], "timed")
        assert _same_bits(res[0], plain[0]) and _same_bits(res[1], plain[1])


# ---- 8: converge_batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_converge_batch_feeds_the_ticks_it_integrates(cases, iiwa_fk, group):
    """``ticks`` and ``status`` exactly, on every instance, against host_loops.converge_loop with the feed (the
    oracle; none of the 100 instances comes within MARGIN of its tolerance).  The state and the velocity at the stop are
    held to Q_TOL / V_TOL against the same loop with every pseudo-inverse taken through the SVD filter factors
    (exact_yardstick.dpinv_stable, the evaluation tolerances.py calls the stable one), and to Q_TOL / V_TOL plus the
    literal oracle's own distance from that evaluation against the literal loop.  That distance is no rounding here: the
    smoothing task behind the pose task is the one tolerances.py describes (noise of u * 1e8 in the velocity of a task
    behind the first equality on a redundant arm), and the feed keeps what a tick adds in the null space for all later
    ticks, so it grows with the square of the tick count: 1.8e-9 in q and 2.8e-9 in dq after up to 14 ticks of dt = 0.05
    (1.6e-13 and 2.6e-12 with nothing fed) - both loops on the CPU, no device result enters the bound.  Measured on the
    MI355X: the launch is 1.77e-9 from the literal loop in q."""
    from exact_yardstick import dpinv_stable
    spec, ctrl, qp, fb = cases("pinv")
    Q, Y = V.iiwa_inputs(iiwa_fk, 100)
    tol = K.tolerances(spec, {"tool_pose": 1e-5, "smooth": np.inf})
    hq, hdq, hticks, hstatus, hres, sure = H.converge_loop(spec, {}, Q, Y, tol, 60, fb=fb)
    print("host loop: ticks %d .. %d, status %s, sure %d of %d" % (hticks.min(), hticks.max(), np.bincount(hstatus),
                                                                   sure.sum(), sure.size))
    assert (hstatus == 0).all() and hticks.min() >= 1 and hticks.max() <= 14 and sure.all()
    sq, sdq, sticks, sstatus, _, _ = H.converge_loop(spec, {}, Q, Y, tol, 60, fb=fb, pinv_fn=dpinv_stable)
    assert np.array_equal(sticks, hticks) and np.array_equal(sstatus, hstatus)
    own_q, own_v = np.abs(hq - sq).max(), np.abs(hdq - sdq).max()
    print("the literal oracle's loop against its stable evaluation: |q| %.3g |dq| %.3g" % (own_q, own_v))
    assert own_q < 1e-8 and own_v < 1e-7          # (the yardstick still resolves what the test is about: 1.7e-2 in q)
    if group == 1:
        for B in BATCHES:
            q, dq, mode, info = ctrl.converge_batch(Q[:B], input_var=Y[:B], tol=tol, max_ticks=60, dt=K.DT)
            assert np.array_equal(info["ticks"], hticks[:B]) and np.array_equal(info["status"], hstatus[:B])
            eq, ev = np.abs(q - sq[:B]).max(), np.abs(dq - sdq[:B]).max()
            lq, lv = np.abs(q - hq[:B]).max(), np.abs(dq - hdq[:B]).max()
            print("converge B=%d: against the stable loop |q| %.3g |dq| %.3g, against the literal loop |q| %.3g |dq| %.3g"
                  % (B, eq, ev, lq, lv))
            assert eq < Q_TOL and ev < V_TOL
            assert lq < Q_TOL + own_q and lv < V_TOL + own_v
        # the feed is seen: frozen at rest, the smoothing task pulls the null-space motion to zero instead
        frozen = H.converge_loop(spec, {}, Q, Y, tol, 60, fb=(-1,) * 7)
        assert np.abs(frozen[0] - hq).max() > 1e-6
    else:
        # groups of four copies of an instance: the copies arrive together, so the rule cancels nobody and every copy is
        # the ungrouped launch's instance - with the feed compiled into the grouped kernel as well
        q, dq, mode, info = ctrl.converge_batch(np.repeat(Q, 4, axis=0), input_var=np.repeat(Y, 4, axis=0), tol=tol,
                                                max_ticks=60, dt=K.DT, group=4)
        assert np.array_equal(info["ticks"], np.repeat(hticks, 4)) and np.array_equal(info["status"], np.repeat(hstatus, 4))
        assert np.abs(q - np.repeat(sq, 4, axis=0)).max() < Q_TOL and np.abs(dq - np.repeat(sdq, 4, axis=0)).max() < V_TOL
        assert np.abs(q - np.repeat(hq, 4, axis=0)).max() < Q_TOL + own_q


# ---- 9: what is refused -------------------------------------------------------------------------------------------------------------
def test_refusals(cases, iiwa_fk, monkeypatch):
    import torch
    spec = V.pinv_skill(iiwa_fk)
    Q, Y = V.iiwa_inputs(iiwa_fk, 4)
    # the option itself, at set-up
    for bad, match in (((7, 8, 9), "must have 7 entries"), (tuple(range(8, 15)), r"in \[-1, 14\)"),
                       ((7, 7, 8, 9, 10, 11, 12), "twice"), ((7.0,) * 7, "must be an int"), (5, "sequence")):
        with pytest.raises(ValueError, match=match):
            cc.PseudoInverseController(skill_spec=spec, options={"velocity_feedback": bad}).setup_problem_functions()
    no_input = K.path_skill(skills.ur5())
    with pytest.raises(ValueError, match="input_var"):
        cc.PseudoInverseController(skill_spec=no_input, options={"velocity_feedback": (-1,) * 6 + (0,)}).setup_problem_functions()
    # a handle that only the built-in kernels serve (config 2 without run-time instantiation: its constraints need no
    # generated code, so the handle exists - and has no kernel that could carry a map)
    dyn = cc.PseudoInverseController(skill_spec=skills.pose_skill(iiwa_fk),
                                     options={"velocity_feedback": tuple(range(7)), "function_opts": {"jit": False}})
    dyn.setup_problem_functions()
    Y7 = Y[:, :7]
    assert dyn.solve_batch(0.0, Q, input_var=Y7)[0].shape == Q.shape        # (ticks are served, and unchanged)
    for call in (lambda: dyn.rollout_batch(TIMES, Q, input_var=Y7, dt=DT),
                 lambda: dyn.rollout_batch(TIMES, Q, input_var=Y7, dt=DT, summary=True),
                 lambda: dyn.converge_batch(Q, input_var=Y7, tol=np.inf, max_ticks=3)):
        with pytest.raises(NotImplementedError, match="velocity_feedback"):
            call()
    # the resident loop that keeps the state in the kernel
    ctrl = cases("pinv")[1]
    dev = ctrl._device
    with pytest.raises(NotImplementedError, match="resident"):
        ctrl.resident_start(torch.from_numpy(Q).to(dev), torch.from_numpy(Y).to(dev), 2, integrate_dt=DT)
    # a variant that would spill, or whose block is too large: at attach time, with the figure
    figures = {0: 0, 1: 24, 2: 1000, 3: 2000, 4: 1}

    class Unit(object):
        def __init__(self, fig):
            self.clik_jit_rec_info = lambda what: fig[what]
    monkeypatch.setattr(jit, "_load", lambda so: Unit(figures))
    with pytest.raises(NotImplementedError, match="24 bytes of scratch"):
        jit._rec_feedback_entry("unit.so", "clik_jit_rollout_rec")
    figures = {**figures, 1: 0, 3: 200000, 4: 0}
    monkeypatch.setattr(jit, "_load", lambda so: Unit(figures))
    with pytest.raises(NotImplementedError, match="200000 bytes of LDS"):
        jit._rec_feedback_entry("unit.so", "clik_jit_rollout_rec")
