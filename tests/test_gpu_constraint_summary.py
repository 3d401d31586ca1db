"""GPU: ``constraint_summary_batch`` - per instance and constraint row what e did over a trajectory (largest magnitude and
where, last value, rms, SetConstraint violations, settling), reduced inside the kernels of clik_summary.hpp - against
numpy reductions of the oracle's per-record values (``ExprEvaluator.vector``, bounds from ``attribute_views``), for both
controllers.

Tolerances.  ``abs_max``, ``last``, ``viol_max``: the 1e-12 tests/test_gpu_constraint_values.py holds e to (a maximum or a
clipped difference of values each within 1e-12 is within 1e-12).  ``rms``: 1e-12 + R u max|ref|, u = 2^-53 (the summation
rounding on top).  The integer outputs are compared exactly where the ORACLE's own decision margin is at least 4e-12 (the
two largest |e| of a row apart by that much, no record's d that close to tol, no violation that close to 0); the other
rows are left out, at most 1 % of them - with the seeds below the oracle leaves out none (printed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import jit, skills
from casclik_amd.controllers.base_controller import constraint_row_slices
from casclik_amd.lowering import lower_skill
from oracle import clik_oracle

import time_skills
from extern_skills import double_pendulum_skill, mixed_frame_skill
from test_gpu_attr import _stack as breathing_stack, _states as breathing_states

pytestmark = pytest.mark.gpu

TOL = 1e-12
U = 2.0 ** -53
MARGIN = 4e-12
BATCHES = (1, 63, 65, 257)      # a lone row, both sides of a wave, one past a 256-lane block
NAMES = ["stack", "qp", "tracking", "mixed", "pendulum", "attr"]
FLOATS = ("abs_max", "last", "rms", "viol_max")
INTS = ("abs_max_at", "viol_count", "settled_at")
DT = 0.3                        # seconds between the records' time stamps


def _chunk(B):
    """the chunk length the implementation picks for the short trajectories of these tests"""
    c = jit.summary_chunk_length(1, B)
    assert jit.summary_chunk_length(2 * c + 3, B) == c          # (every R below is cut into chunks of c)
    return c


def _records(B):
    c = _chunk(B)
    return (1, 2, c - 1, c, c + 1, 2 * c + 3)


def _spec(name, iiwa_fk, ur5_fk):
    if name == "stack":
        return skills.stack_skill(iiwa_fk)
    if name == "qp":
        return skills.qp_skill(iiwa_fk)
    if name == "pendulum":
        return double_pendulum_skill(track=True)
    if name == "tracking":
        return time_skills.tracking_spec(ur5_fk)                # (time slots: e depends on the record's stamp)
    if name == "attr":
        return breathing_stack(iiwa_fk, 7)[0]                   # (set bounds that are expressions of t: attr_ext)
    return mixed_frame_skill(iiwa_fk)                           # (a virtual variable)


def _make(name, iiwa_fk, ur5_fk, **options):
    """(spec, controller, set up) of a fixture"""
    spec = _spec(name, iiwa_fk, ur5_fk)
    if name == "stack":
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict(skills.STACK_OPTIONS, **options))
    elif name == "qp":
        ctrl = cc.ReactiveQPController(skill_spec=spec, options=dict(options))
    elif name == "pendulum":
        ctrl = cc.ReactiveQPController(skill_spec=spec, robot_var_weights=[1.0, 1.0], options=dict(options))
    elif name == "tracking":
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict(options))
    elif name == "attr":
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict({"multidim_sets": True}, **options))
    else:
        ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict({"multidim_sets": False}, **options))
    ctrl.setup_problem_functions()
    if isinstance(ctrl, cc.ReactiveQPController):
        ctrl.setup_solver()
    return spec, ctrl


def _inputs(name, B, iiwa_fk, seed=0):
    """(Q, X | None, Y | None) of a fixture, away from anything singular"""
    rng = np.random.default_rng(100 + seed)
    if name in ("stack", "qp"):
        Q, Y = skills.synthetic_inputs(iiwa_fk, B, seed=seed, distribution="mixed")
        return Q, None, Y
    if name == "mixed":
        Q, _ = skills.synthetic_inputs(iiwa_fk, B, seed=seed)
        return Q, rng.uniform(-1.0, 1.0, size=(B, 1)), rng.uniform(-1.0, 1.0, size=(B, 3))
    if name == "pendulum":
        return np.stack([rng.uniform(0.2, 2.9, B), rng.uniform(-1.5, 1.5, B)], axis=1), None, None
    if name == "attr":
        return breathing_states(np.asarray(iiwa_fk["lower"], float), np.asarray(iiwa_fk["upper"], float), B, 100 + seed), None, None
    return time_skills.UR5_HOME + rng.normal(scale=0.3, size=(B, 6)), None, None


def _trajectory(name, R, B, iiwa_fk, seed=0):
    """(times [R], Q [R, B, n_q], X | None, Y | None): every record a batch of random states of its own"""
    recs = [_inputs(name, B, iiwa_fk, seed=seed + 7 * r) for r in range(R)]
    stack = lambda k: None if recs[0][k] is None else np.stack([r[k] for r in recs])        # noqa: E731
    return DT * np.arange(R), stack(0), stack(1), stack(2)


def _oracle(spec, times, Q, X=None, Y=None):
    """(e, set_min, set_max) [R, B, M_tot] and is_set [M_tot] in the rows of ``constraint_rows()``: ONE evaluator for all
    records (the record's stamp per row), every constraint's expression through ``vector``, the bounds of the
    SetConstraints as each row sees them (``attribute_views``; -inf / +inf on the rows of every other class)"""
    R, B = Q.shape[:2]
    flat = lambda A: None if A is None else A.reshape(R * B, -1)         # noqa: E731
    Z = flat(Q) if X is None else np.hstack([flat(Q), flat(X)])
    Yf = flat(Y if Y is None or Y.ndim == 3 else np.broadcast_to(Y, (R,) + Y.shape))
    ev = clik_oracle.ExprEvaluator(spec, np.repeat(np.asarray(times, dtype=float), B), Z, Yf)
    rows = constraint_row_slices(lower_skill(spec))
    m_tot = max(sl.stop for sl in rows.values())
    e = np.zeros((R * B, m_tot))
    lo, hi = np.full((R * B, m_tot), -np.inf), np.full((R * B, m_tot), np.inf)
    is_set = np.zeros(m_tot, dtype=bool)
    views = clik_oracle.attribute_views(ev, spec.constraints)
    for c, view in zip(spec.constraints, views):
        sl = rows[c.label]
        e[:, sl] = ev.vector(c.expression)[0]
        if clik_oracle._cls(c) == "SetConstraint":
            is_set[sl] = True
            m = sl.stop - sl.start
            lo[:, sl] = np.stack([clik_oracle._num(v.set_min, m) for v in view])
            hi[:, sl] = np.stack([clik_oracle._num(v.set_max, m) for v in view])
    shape = (R, B, m_tot)
    return e.reshape(shape), lo.reshape(shape), hi.reshape(shape), is_set


def _tolerances(e, lo, hi, is_set):
    """one tolerance per row, from the reference values alone: near the middle of what the row's d takes, rounded to two
    digits so that no record sits on it; the same for every shape of a fixture"""
    a = np.abs(e)
    v = np.maximum(np.maximum(lo - e, e - hi), 0.0)
    d = np.where(is_set, v, a).reshape(-1, e.shape[2])
    tol = np.empty(e.shape[2])
    for i in range(e.shape[2]):
        pos = d[:, i][d[:, i] > 0.0]
        tol[i] = float("%.2g" % np.quantile(pos, 0.7)) if pos.size else 0.05
    return tol


def _reduce(e, lo, hi, is_set, tol):
    """the summary of e [R, B, M] by plain numpy reductions, and per (instance, row) whether each integer output is
    decided by a margin of at least MARGIN"""
    R = e.shape[0]
    a = np.abs(e)
    raw = np.maximum(lo - e, e - hi)
    v = np.where(is_set, np.maximum(raw, 0.0), 0.0)
    d = np.where(is_set, v, a)
    uns = d > tol
    any_uns = uns.any(axis=0)
    last_uns = R - 1 - np.argmax(uns[::-1], axis=0)
    ref = {"abs_max": a.max(axis=0), "abs_max_at": a.argmax(axis=0).astype(np.int32), "last": e[-1],
           "rms": np.sqrt((e * e).mean(axis=0)), "viol_max": v.max(axis=0),
           "viol_count": (v > 0.0).sum(axis=0).astype(np.int32),
           "settled_at": np.where(any_uns, last_uns + 1, 0).astype(np.int32)}
    srt = np.sort(a, axis=0)
    sure = {"abs_max_at": (srt[-1] - srt[-2] >= MARGIN) if R > 1 else np.ones(e.shape[1:], dtype=bool),
            "viol_count": ~(is_set & (np.abs(raw) < MARGIN)).any(axis=0),
            "settled_at": ~(np.abs(d - tol) < MARGIN).any(axis=0)}
    return ref, sure


def _check(name, what, got, ref, sure, R, left_out):
    """floats within their bounds; integers exactly on the rows the oracle decides by a margin"""
    for key in FLOATS:
        bound = TOL + (R * U * np.abs(ref[key]).max() if key == "rms" else 0.0)
        err = float(np.abs(got[key] - ref[key]).max())
        print("%s %s %s: max |dev - ref| = %.3g (bound %.3g, max |ref| %.3g)" % (name, what, key, err, bound,
                                                                                 np.abs(ref[key]).max()))
        assert got[key].dtype == np.float64 and np.isfinite(got[key]).all() and err < bound, (name, what, key, err, bound)
    for key in INTS:
        if key not in ref or (key == "settled_at" and key not in got):
            continue
        assert got[key].dtype == np.int32 and got[key].shape == ref[key].shape, (name, what, key)
        keep = sure[key]
        left_out[0] += int((~keep).sum())
        left_out[1] += keep.size
        assert np.array_equal(got[key][keep], ref[key][keep]), (name, what, key, np.nonzero(got[key] != ref[key]))


_REFERENCES = {}


def reference(name, iiwa_fk, ur5_fk):
    """(spec, trajectory, oracle values, tol) of a fixture at the largest shape the tests use: computed once, shared by
    every test, never changed (the smaller shapes are its leading records and instances)"""
    if name not in _REFERENCES:
        spec = _spec(name, iiwa_fk, ur5_fk)
        B = max(BATCHES)
        traj = _trajectory(name, max(_records(B)), B, iiwa_fk)
        orc = _oracle(spec, *traj)
        _REFERENCES[name] = (spec, traj, orc, _tolerances(*orc))
    return _REFERENCES[name]


def _cut(traj, orc, R, B):
    times, Q, X, Y = traj
    cut = lambda A: None if A is None else np.ascontiguousarray(A[:R, :B])      # noqa: E731
    return (times[:R], cut(Q), cut(X), cut(Y)), tuple(A[:R, :B] for A in orc[:3]) + (orc[3],)


@pytest.fixture(scope="module")
def ctrls(iiwa_fk, ur5_fk):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _make(name, iiwa_fk, ur5_fk)
        return cache[name]
    return get


# ---- 1: against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_summaries_match_the_reductions_of_the_oracle(ctrls, iiwa_fk, ur5_fk, name):
    spec, ctrl = ctrls(name)
    _, traj, orc, tol = reference(name, iiwa_fk, ur5_fk)
    assert list(constraint_row_slices(lower_skill(spec))) == list(ctrl.constraint_rows())
    left_out = [0, 0]
    counts, settled = [], []
    for B in BATCHES:
        for R in _records(B):
            (times, Q, X, Y), cut = _cut(traj, orc, R, B)
            ref, sure = _reduce(*cut, tol)
            got = ctrl.constraint_summary_batch(times, Q, virtual_var=X, input_var=Y, tol=tol)
            assert sorted(got) == sorted(FLOATS + INTS) and all(v.shape == (B, len(tol)) for v in got.values())
            _check(name, "B=%d R=%d" % (B, R), got, ref, sure, R, left_out)
            counts.append(ref["viol_count"][:, orc[3]])
            settled.append((ref["settled_at"] == 0).any() + 2 * (ref["settled_at"] == R).any()
                           + 4 * ((ref["settled_at"] > 0) & (ref["settled_at"] < R)).any())
    print("%s: %d of %d integer results left out (oracle margin below %.0e)" % (name, left_out[0], left_out[1], MARGIN))
    assert left_out[0] <= 0.01 * left_out[1], left_out
    # the inputs are not one-sided
    assert np.bitwise_or.reduce(settled) == 7, settled
    if orc[3].any():
        every = np.concatenate([c.reshape(-1) for c in counts])
        assert (every == 0).any() and (every > 0).any()
    else:
        assert name in ("qp", "tracking")           # (no SetConstraint: a VelocitySetConstraint bounds a velocity)


# ---- 2: a real record ----------------------------------------------------------------------------------------------------
def test_summary_of_a_recorded_rollout(ctrls, iiwa_fk):
    import torch
    spec, ctrl = ctrls("stack")
    dev = ctrl._device
    B, n_ticks, dt = 65, 64, 0.02
    # targets a loop of 64 ticks can reach: the tool pose at a state 0.15 rad (a standard deviation per joint) from the
    # start, the start clipped into 80 % of the joint range first.  (The far targets of `synthetic_inputs` are not reached
    # in 64 ticks by more than half of the instances.)  The ORACLE's closed loop on these inputs - 64 Euler ticks of
    # clik_oracle.pinv_solve_batch - settles all six pose rows strictly inside the record for 59 of the 65 instances, 5
    # have a row that is still outside at the end, 15 joint-limit rows are violated at some record.
    Q, _, _ = _inputs("stack", B, iiwa_fk, seed=6)
    lo, hi = np.asarray(iiwa_fk["lower"], float), np.asarray(iiwa_fk["upper"], float)
    near = np.clip(Q, 0.8 * lo, 0.8 * hi) + np.random.default_rng(7).normal(scale=0.15, size=Q.shape)
    Y = np.zeros((B, 7))
    for b in range(B):
        T = iiwa_fk["chain"].fk_numeric(near[b])
        Y[b, :3], Y[b, 3:] = T[:3, 3], skills.quat_from_matrix(T[:3, :3])
    times = torch.from_numpy(dt * np.arange(n_ticks)).to(dev)
    Qd, Yd = torch.from_numpy(Q).to(dev), torch.from_numpy(Y).to(dev)
    rec = ctrl.rollout_batch(times.cpu().numpy(), Qd, input_var=Yd, dt=dt, record_every=1)[-1]
    assert rec["q"].shape == (n_ticks, B, ctrl.descriptor.n_q) and rec["q"].device == dev
    got = ctrl.constraint_summary_batch(times, rec["q"], input_var=Yd, tol=1e-3)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values())
    got = {k: v.cpu().numpy() for k, v in got.items()}
    orc = _oracle(spec, times.cpu().numpy(), rec["q"].cpu().numpy(), None, Y)
    ref, sure = _reduce(*orc, np.full(orc[0].shape[2], 1e-3))
    left_out = [0, 0]
    _check("stack", "recorded rollout", got, ref, sure, n_ticks, left_out)
    print("recorded rollout: %d of %d integer results left out" % tuple(left_out))
    assert left_out[0] <= 0.01 * left_out[1], left_out
    pose = ctrl.constraint_rows()["tool_pose"]
    inside = ((got["settled_at"][:, pose] > 0) & (got["settled_at"][:, pose] < n_ticks)).all(axis=1)
    print("pose rows settle strictly inside the record for %d of %d instances" % (inside.sum(), B))
    assert inside.sum() > B // 2, inside.sum()


# ---- 3: chunking is invisible --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES[:5])      # ("attr": its bounds are the kernel's own evaluation, held to the oracle in 1)
def test_chunks_reduce_to_what_the_stored_values_reduce_to(ctrls, iiwa_fk, ur5_fk, name):
    spec, ctrl = ctrls(name)
    _, traj, orc, tol = reference(name, iiwa_fk, ur5_fk)
    B = 65
    R = 2 * _chunk(B) + 3
    (times, Q, X, Y), cut = _cut(traj, orc, R, B)
    e = ctrl.constraint_values_batch(times, Q, virtual_var=X, input_var=Y)
    got = ctrl.constraint_summary_batch(times, Q, virtual_var=X, input_var=Y, tol=tol)
    # the device's own e, the oracle's bounds widened to the image's "no bound" (+-1e10, lowering.py) where infinite
    lo, hi = np.clip(cut[1], -1e10, None), np.clip(cut[2], None, 1e10)
    ref, _ = _reduce(e, lo, hi, cut[3], tol)
    for key in ("abs_max", "abs_max_at", "last", "viol_max", "viol_count", "settled_at"):
        assert np.array_equal(got[key], ref[key]), (name, key, np.abs(got[key] - ref[key]).max())
    bound = R * U * np.abs(ref["rms"]).max()
    err = np.abs(got["rms"] - ref["rms"]).max()
    print("%s rms: max |summary - reduction of the stored values| = %.3g (bound %.3g)" % (name, err, bound))
    assert err <= bound, (name, err, bound)


# ---- 4: determinism and independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "pendulum"])
def test_same_bits_every_call_and_in_every_batch(ctrls, iiwa_fk, ur5_fk, name):
    spec, ctrl = ctrls(name)
    _, traj, orc, tol = reference(name, iiwa_fk, ur5_fk)
    R = 2 * _chunk(257) + 3
    big, _ = _cut(traj, orc, R, 257)
    small, _ = _cut(traj, orc, R, 63)
    call = lambda t: ctrl.constraint_summary_batch(t[0], t[1], virtual_var=t[2], input_var=t[3], tol=tol)   # noqa: E731
    one, two, part = call(big), call(big), call(small)
    for key in FLOATS + INTS:
        assert np.array_equal(one[key].view(np.uint8), two[key].view(np.uint8)), key
        assert np.array_equal(one[key][:63].view(np.uint8), part[key].view(np.uint8)), key


# ---- 5: shapes and errors ------------------------------------------------------------------------------------------------
def test_shapes_containers_and_refusals(ctrls, iiwa_fk, ur5_fk):
    spec, ctrl = ctrls("stack")
    _, traj, orc, tol = reference("stack", iiwa_fk, ur5_fk)
    (times, Q, X, Y), _ = _cut(traj, orc, 3, 65)
    flat = ctrl.constraint_summary_batch(times[0], Q[0], input_var=Y[0], tol=tol)
    one = ctrl.constraint_summary_batch(times[:1], Q[:1], input_var=Y[:1], tol=tol)
    for key in FLOATS + INTS:
        assert isinstance(flat[key], np.ndarray) and np.array_equal(flat[key].view(np.uint8), one[key].view(np.uint8)), key
    assert (flat["abs_max_at"] == 0).all() and np.array_equal(flat["abs_max"], np.abs(flat["last"]))
    # one [B, n_y] block for all records, or one per record
    shared = ctrl.constraint_summary_batch(times, Q, input_var=Y[0])
    per_rec = ctrl.constraint_summary_batch(times, Q, input_var=np.ascontiguousarray(np.broadcast_to(Y[0], Y.shape)))
    assert "settled_at" not in shared and sorted(shared) == sorted(FLOATS + INTS[:2])
    for key in shared:
        assert np.array_equal(shared[key].view(np.uint8), per_rec[key].view(np.uint8)), key
    scalar = ctrl.constraint_summary_batch(times, Q, input_var=Y, tol=0.25)
    assert np.array_equal(scalar["settled_at"],
                          ctrl.constraint_summary_batch(times, Q, input_var=Y, tol=np.full(len(tol), 0.25))["settled_at"])
    for bad in (tol[:-1], -tol, np.where(np.arange(len(tol)) == 3, np.nan, tol), np.inf):
        with pytest.raises(ValueError, match="tol"):
            ctrl.constraint_summary_batch(times, Q, input_var=Y, tol=bad)
    with pytest.raises(ValueError, match="time_var has 2 entries"):
        ctrl.constraint_summary_batch(times[:2], Q, input_var=Y)
    with pytest.raises(ValueError, match="time_var has 3 entries"):
        ctrl.constraint_summary_batch(times, Q[0], input_var=Y[0])
    with pytest.raises(ValueError, match="input_var"):
        ctrl.constraint_summary_batch(times, Q)


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
    ctrl.constraint_summary_batch(0.0, Q, input_var=Y, tol=1e-3)
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


# ---- 6: a poisoned instance ----------------------------------------------------------------------------------------------
def test_a_nan_in_one_record_marks_that_instance_and_no_other(ctrls, iiwa_fk, ur5_fk):
    import torch
    spec, ctrl = ctrls("stack")
    dev = ctrl._device
    _, traj, orc, tol = reference("stack", iiwa_fk, ur5_fk)
    B = 65
    R = 2 * _chunk(B) + 3
    (times, Q, X, Y), _ = _cut(traj, orc, R, B)
    Qd, Yd = torch.from_numpy(Q).to(dev), torch.from_numpy(Y).to(dev)
    clean = ctrl.constraint_summary_batch(times, Qd, input_var=Yd, tol=tol)
    bad_rec, bad = _chunk(B) + 2, 40
    Qn = Qd.clone()
    Qn[bad_rec, bad, :] = float("nan")
    poisoned = ctrl.constraint_summary_batch(times, Qn, input_var=Yd, tol=tol)
    keep = torch.arange(B, device=dev) != bad
    for key in FLOATS + INTS:
        assert torch.equal(poisoned[key][keep], clean[key][keep]), key
    for key in FLOATS:
        assert bool(torch.isnan(poisoned[key][bad]).all()), (key, poisoned[key][bad])
