"""GPU: ``rollout_batch(..., summary=True)`` - the constraint summaries of ``constraint_summary_batch`` computed inside the
rollout (clik_rollout_summary.hpp), with no record of the trajectory.  Record r of the summary is what tick r acts on: the
tick's time, the state it starts from, the target it reads.

The yardstick separates the summary from the tick: every launch also records (``record_every=1``, the same launch), and the
reference is the numpy reduction (``_reduce``) of the oracle's values (``_oracle``) at the launch's OWN states ``concat(q_0,
rec["q"][:-1])`` - the ticks themselves are held to their tolerance by the rollout suites.  Bounds as
tests/test_gpu_constraint_summary.py states them: floats 1e-12 (``rms``: 1e-12 + n u max|ref|), integers exact on the
rows the oracle decides by 4e-12, at most 1 % of the integer results left out (the count is printed).

Every call without ``summary=`` is what it was before; every call with it needs the summarising kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import skills

from test_gpu_constraint_summary import FLOATS, INTS, NAMES, TOL, _check, _inputs, _make, _oracle, _reduce, _tolerances
from test_gpu_rollout_record import Q_TOL, V_TOL, _family, _moving

pytestmark = pytest.mark.gpu

DT = 0.02
BATCHES = (1, 63, 65)           # a lone row, both sides of a wave
TICKS = (1, 2, 9)


@pytest.fixture(scope="module")
def ctrls(iiwa_fk, ur5_fk):
    cache = {}

    def get(name, **options):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            cache[key] = _make(name, iiwa_fk, ur5_fk, **options)
        return cache[key]
    return get


def _before(first, rec):
    """the state every tick of a recording launch starts from: ``concat(first, rec[:-1])``"""
    return None if first is None else np.concatenate([np.asarray(first)[None], rec[:-1]])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _near_targets(iiwa_fk, B):
    """the start states and reachable targets of test_gpu_constraint_summary.py::test_summary_of_a_recorded_rollout: the
    tool pose at a state 0.15 rad (a standard deviation per joint) from the start, the start clipped into 80 % of the
    joint range first"""
    Q, _, _ = _inputs("stack", B, iiwa_fk, seed=6)
    lo, hi = np.asarray(iiwa_fk["lower"], float), np.asarray(iiwa_fk["upper"], float)
    near = np.clip(Q, 0.8 * lo, 0.8 * hi) + np.random.default_rng(7).normal(scale=0.15, size=Q.shape)
    Y = np.zeros((B, 7))
    for b in range(B):
        T = iiwa_fk["chain"].fk_numeric(near[b])
        Y[b, :3], Y[b, 3:] = T[:3, 3], skills.quat_from_matrix(T[:3, :3])
    return Q, Y


# ---- 1: against the oracle -----------------------------------------------------------------------------------------------
CASES = [(name, "euler", False) for name in NAMES] + [("stack", "rk4", False), ("qp", "rk4", False),
                                                       ("tracking", "euler", True)]


@pytest.mark.parametrize("name,method,on_device", CASES)
def test_summaries_match_the_reductions_of_the_oracle(ctrls, iiwa_fk, ur5_fk, name, method, on_device):
    import torch
    spec, ctrl = ctrls(name, time_on_device=True) if on_device else ctrls(name)
    left_out = [0, 0]
    for B in BATCHES:
        Q0, X0, Y = _inputs(name, B, iiwa_fk, seed=6)
        for n in TICKS:
            times = DT * np.arange(n)
            tv = torch.from_numpy(times).to(ctrl._device) if on_device else times
            kw = dict(input_var=Y, virtual_var=X0, dt=DT, method=method, record_every=1, summary=True)
            # the launch's own states, from a first launch without a tolerance; the launch under test repeats it bit for bit
            first = ctrl.rollout_batch(tv, Q0, **kw)
            rec = first[-2]
            assert rec["q"].shape == (n, B, ctrl.descriptor.n_q)
            Qs, Xs = _before(Q0, rec["q"]), _before(X0, rec.get("x"))
            orc = _oracle(spec, times, Qs, Xs, Y)
            tol = _tolerances(*orc)
            res = ctrl.rollout_batch(tv, Q0, summary_tol=tol, **kw)
            assert len(res) == len(first)
            for key in rec:
                assert _same_bits(res[-2][key], rec[key]), key
            got = res[-1]
            assert sorted(got) == sorted(FLOATS + INTS) and all(v.shape == (B, len(tol)) for v in got.values())
            ref, sure = _reduce(*orc, tol)
            _check(name, "%s B=%d n=%d" % (method, B, n), got, ref, sure, n, left_out)
            # without a tolerance: the same values, and no settled_at
            assert sorted(first[-1]) == sorted(FLOATS + INTS[:2])
            for key in first[-1]:
                assert _same_bits(first[-1][key], got[key]), key
    print("%s %s: %d of %d integer results left out (oracle margin below 4e-12)" % (name, method, left_out[0], left_out[1]))
    assert left_out[0] <= 0.01 * left_out[1], left_out


# ---- 2: a loop that settles ----------------------------------------------------------------------------------------------
def test_a_loop_that_settles(ctrls, iiwa_fk):
    spec, ctrl = ctrls("stack")
    B, n = 65, 64
    Q, Y = _near_targets(iiwa_fk, B)
    times = DT * np.arange(n)
    res = ctrl.rollout_batch(times, Q, input_var=Y, dt=DT, summary=True, summary_tol=1e-3)
    assert len(res) == 4                                        # (q, dq, mode and the summary: no record)
    got = res[-1]
    rec = ctrl.rollout_batch(times, Q, input_var=Y, dt=DT, record_every=1)[-1]     # (a second launch, without summary)
    orc = _oracle(spec, times, _before(Q, rec["q"]), None, Y)
    ref, sure = _reduce(*orc, np.full(orc[0].shape[2], 1e-3))
    left_out = [0, 0]
    _check("stack", "settling loop", got, ref, sure, n, left_out)
    print("settling loop: %d of %d integer results left out" % tuple(left_out))
    assert left_out[0] <= 0.01 * left_out[1], left_out
    rows = ctrl.constraint_rows()
    pose, limits = rows["tool_pose"], rows["joint_limits"]
    inside = ((got["settled_at"][:, pose] > 0) & (got["settled_at"][:, pose] < n)).all(axis=1)
    print("pose rows settle strictly inside the rollout for %d of %d instances" % (inside.sum(), B))
    assert inside.sum() > B // 2, inside.sum()
    assert (got["viol_count"][:, limits] > 0).any() and (got["viol_count"][:, limits] == 0).any()


# ---- 3: nothing else moves -----------------------------------------------------------------------------------------------
def _close(a, b, tol):
    """floats: NaN where the other has NaN (an infeasible QP instance) and within tol elsewhere; integers: identical"""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and (nan.all() or float(np.abs(a[~nan] - b[~nan]).max()) < tol)


@pytest.mark.parametrize("family", ["stack_values", "stack_image", "pose", "point", "virtual", "qp_box", "qp_walls"])
def test_the_rollout_s_own_results_do_not_move(iiwa_fk, ur5_fk, monkeypatch, family):
    ctrl, qp, dt, vmax, inputs = _family(family, iiwa_fk, ur5_fk, monkeypatch)
    Q, X, Y = inputs(100)
    times = dt * np.arange(11)
    if family == "point":
        # the five-set skill's plain rollouts are the built-in kernel's, which has no Runge-Kutta form: refused with a summary
        # as it is without one, so no summarising kernel runs that nothing can be compared with
        for kw in ({}, {"summary": True}):
            with pytest.raises(NotImplementedError, match="Runge-Kutta"):
                ctrl.rollout_batch(times, Q, input_var=Y, dt=dt, max_speed=vmax, method="rk4", **kw)
    for method in (("euler",) if family == "point" else ("euler", "rk4")):
        kw = dict(input_var=Y, dt=dt, max_speed=vmax, virtual_var=X, method=method, record_every=2)
        plain = ctrl.rollout_batch(times, Q, **kw)
        summed = ctrl.rollout_batch(times, Q, summary=True, summary_tol=1e-3, **kw)
        assert len(summed) == len(plain) + 1 and sorted(summed[-1]) == sorted(FLOATS + INTS)
        names = (("q", "x", "dq", "dx") if X is not None else ("q", "dq")) + (("slack", "status") if qp else ("mode",))
        assert len(names) == len(plain) - 1
        for key, a, b in zip(names, summed, plain):
            assert _close(a, b, Q_TOL if key in ("q", "x") else V_TOL), (family, method, key)
        assert set(summed[-2]) == set(plain[-1])
        for key, b in plain[-1].items():
            assert _close(summed[-2][key], b, Q_TOL if key in ("q", "x") else V_TOL), (family, method, "record", key)


# ---- 4: a per-tick target ------------------------------------------------------------------------------------------------
def test_a_moving_target_is_summarised_record_by_record(ctrls, iiwa_fk):
    spec, ctrl = ctrls("stack")
    B, n = 65, 9
    Q, _, Y = _inputs("stack", B, iiwa_fk, seed=6)
    Y3 = _moving(Y, n)
    times = DT * np.arange(n)
    kw = dict(dt=DT, record_every=1, summary=True, summary_tol=1e-2)
    res = ctrl.rollout_batch(times, Q, input_var=Y3, **kw)
    orc = _oracle(spec, times, _before(Q, res[-2]["q"]), None, Y3)
    ref, sure = _reduce(*orc, np.full(orc[0].shape[2], 1e-2))
    left_out = [0, 0]
    _check("stack", "moving target", res[-1], ref, sure, n, left_out)
    assert left_out[0] <= 0.01 * left_out[1], left_out
    still = ctrl.rollout_batch(times, Q, input_var=Y, **kw)[-1]
    pose = ctrl.constraint_rows()["tool_pose"]
    assert np.abs(still["rms"][:, pose] - res[-1]["rms"][:, pose]).max() > 1e3 * TOL


# ---- 5: determinism and independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "pendulum"])
def test_same_bits_every_call_and_in_every_batch(ctrls, iiwa_fk, name):
    spec, ctrl = ctrls(name)
    Q, X, Y = _inputs(name, 65, iiwa_fk, seed=6)
    times = DT * np.arange(9)
    cut = lambda A: None if A is None else np.ascontiguousarray(A[:63])        # noqa: E731
    call = lambda q, x, y: ctrl.rollout_batch(times, q, input_var=y, virtual_var=x, dt=DT, summary=True,     # noqa: E731
                                              summary_tol=1e-2)[-1]
    one, two, part = call(Q, X, Y), call(Q, X, Y), call(cut(Q), cut(X), cut(Y))
    for key in FLOATS + INTS:
        assert _same_bits(one[key], two[key]), key
        assert _same_bits(np.ascontiguousarray(one[key][:63]), part[key]), key


# ---- 6: containers and refusals ------------------------------------------------------------------------------------------
def test_containers_and_refusals(ctrls, iiwa_fk, monkeypatch):
    import torch
    spec, ctrl = ctrls("stack")
    dev = ctrl._device
    Q, _, Y = _inputs("stack", 65, iiwa_fk, seed=6)
    times = DT * np.arange(3)
    host = ctrl.rollout_batch(times, Q, input_var=Y, dt=DT, summary=True, summary_tol=1e-2)
    res = ctrl.rollout_batch(times, torch.from_numpy(Q).to(dev), input_var=torch.from_numpy(Y).to(dev), dt=DT, summary=True,
                             summary_tol=1e-2)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in res[-1].values())
    for key, v in host[-1].items():
        assert isinstance(v, np.ndarray) and _same_bits(v, res[-1][key].cpu().numpy()), key
    m = len(host[-1]["rms"][0])
    with pytest.raises(ValueError, match="summary=True"):
        ctrl.rollout_batch(times, Q, input_var=Y, dt=DT, summary_tol=1e-2)
    for bad in (-1e-3, float("nan"), np.full(m - 1, 1e-3), np.where(np.arange(m) == 3, -1.0, 1e-3)):
        with pytest.raises(ValueError, match="tol"):
            ctrl.rollout_batch(times, Q, input_var=Y, dt=DT, summary=True, summary_tol=bad)
    with pytest.raises(ValueError, match="at least one tick"):
        ctrl.rollout_batch(np.zeros(0), Q, input_var=Y, dt=DT, summary=True)
    assert len(ctrl.rollout_batch(np.zeros(0), Q, input_var=Y, dt=DT)) == 3        # (without summary: as before)
    # a handle served only by the built-in dynamic kernels: refused, no chunked or host fallback
    monkeypatch.setenv("CLIK_FORCE_DYNAMIC", "1")
    for dyn in (cc.PseudoInverseController(skill_spec=skills.stack_skill(iiwa_fk), options=dict(skills.STACK_OPTIONS)),
                cc.ReactiveQPController(skill_spec=skills.qp_skill(iiwa_fk))):
        dyn.setup_problem_functions()
        dyn.setup_solver()
        with pytest.raises(NotImplementedError, match="summarising rollout"):
            dyn.rollout_batch(times, Q, input_var=Y, dt=DT, summary=True)


_NO_JIT = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import casclik_amd as cc
from casclik_amd import skills
fk = skills.iiwa()
ctrl = cc.PseudoInverseController(skill_spec=skills.stack_skill(fk), options=dict(skills.STACK_OPTIONS))
ctrl.setup_problem_functions()
Q, Y = skills.synthetic_inputs(fk, 5, seed=0)
try:
    ctrl.rollout_batch(np.zeros(2), Q, input_var=Y, dt=0.02, summary=True)
except NotImplementedError as exc:
    assert "instantiated" in str(exc), exc
    print("REFUSED")
"""


def test_without_an_instantiated_kernel_the_call_is_refused():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CLIK_JIT="0")
    out = subprocess.run([sys.executable, "-c", _NO_JIT % (root, os.path.join(root, "tests"))], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0 and b"REFUSED" in out.stdout, out.stdout.decode()[-2000:]


# ---- 7: a poisoned instance ----------------------------------------------------------------------------------------------
def test_a_nan_in_one_instance_marks_that_instance_and_no_other(ctrls, iiwa_fk):
    import torch
    spec, ctrl = ctrls("stack")
    dev = ctrl._device
    B, bad = 65, 40
    Q, _, Y = _inputs("stack", B, iiwa_fk, seed=6)
    times = DT * np.arange(9)
    Qd, Yd = torch.from_numpy(Q).to(dev), torch.from_numpy(Y).to(dev)
    call = lambda q: ctrl.rollout_batch(times, q, input_var=Yd, dt=DT, summary=True, summary_tol=1e-2)[-1]      # noqa: E731
    clean = call(Qd)
    Qn = Qd.clone()
    Qn[bad, :] = float("nan")
    poisoned = call(Qn)
    keep = torch.arange(B, device=dev) != bad
    for key in FLOATS + INTS:
        assert _same_bits(poisoned[key][keep].cpu().numpy(), clean[key][keep].cpu().numpy()), key
        assert not bool(torch.isnan(clean[key].double()).any()), key
    limits = ctrl.constraint_rows()["joint_limits"]
    assert bool(torch.isnan(poisoned["abs_max"][bad, limits]).all()), poisoned["abs_max"][bad]


# ---- 8: every on-demand kernel is built once -----------------------------------------------------------------------------
def _unit_of(template):
    """which entry of ``jit.UNITS`` a translation unit is (its second, value-specialised object counts as the entry's)"""
    from casclik_amd import jit
    for (what, _), unit in jit.UNITS.items():
        for u in (unit, unit["values"]):
            if u and any('extern "C" hipError_t %s(' % s in (template or "") for s in u["symbols"]):
                return what
    return None


@pytest.mark.parametrize("name", ["stack", "qp"])
def test_every_on_demand_kernel_is_asked_for_once(iiwa_fk, ur5_fk, monkeypatch, name):
    """A recording rollout, a summarising one, the constraint values and their summaries, each twice on a fresh
    controller, B = 3 (a partial wave), 2 ticks: the first round asks ``jit.build_shape_library`` for each kind of unit
    exactly once (the recording rollouts for two objects where a value-specialised kernel serves the handle), the second
    round for none, and returns the first round's bits."""
    from casclik_amd import jit
    spec, ctrl = _make(name, iiwa_fk, ur5_fk)
    asked = []
    build = jit.build_shape_library

    def counting(init, verbose=False, template=None, defines=(), extern=""):
        asked.append(_unit_of(template))
        return build(init, verbose, template=template, defines=defines, extern=extern)
    monkeypatch.setattr(jit, "build_shape_library", counting)
    B, n = 3, 2
    Q, _, Y = _inputs(name, B, iiwa_fk, seed=6)
    times = DT * np.arange(n)

    def one_round():
        rec = ctrl.rollout_batch(times, Q, input_var=Y, dt=DT, record_every=1)
        summed = ctrl.rollout_batch(times, Q, input_var=Y, dt=DT, summary=True)
        values = ctrl.constraint_values_batch(times, rec[-1]["q"], input_var=Y)
        summary = ctrl.constraint_summary_batch(times, rec[-1]["q"], input_var=Y)
        flat = list(rec[:-1]) + list(summed[:-1]) + [values]
        for d in (rec[-1], summed[-1], summary):
            flat += [d[key] for key in sorted(d)]
        return flat
    first = one_round()
    want = {"rec": 2 if ctrl.value_kernel else 1, "rollsum": 1, "monitor": 1, "summary": 1}
    assert {what: asked.count(what) for what in set(asked)} == want, asked
    del asked[:]
    second = one_round()
    assert asked == []
    assert len(first) == len(second) and len(first) > 12
    for a, b in zip(first, second):
        assert _same_bits(a, b)
