"""GPU: `DeviceFunction` - a cs.Function at every row of a batch or a recorded trajectory in one launch - against
`Function.__call__` under the derived tolerance of function_cases.py, at the wave and block tails, with every form of
broadcasting, in place over the records of a rollout, and with a poisoned row; the cases that hold every operation the
code generator emits, and sincos_joint alone, also against the exact value; selections at their ties and the infinite
results of finite inputs bit for bit."""
import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import sym as cs

import function_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dfn():
    made = {}

    def get(name):
        if name not in made:
            made[name] = cc.DeviceFunction(fc.get(name))
        return made[name]
    return get


def _args(name, R, B, three_d=True):
    """the leading [:R, :B] corner of the pool; ``three_d`` False: record 0 as a [B] batch"""
    return tuple(np.ascontiguousarray(a[:R, :B] if three_d else a[0, :B]) for a in fc.pool(name))


def _as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


# ---- parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_every_entry_matches_the_host_evaluator_under_the_derived_bound(dfn, name):
    f = dfn(name)
    assert f.scratch_bytes == 0
    vals, bnds = fc.reference(name)
    worst = 0.0
    for R, B in fc.shapes(name):
        for three_d in ((True, False) if R == 1 else (True,)):
            outs = _as_tuple(f(*_args(name, R, B, three_d)))
            lead = (R, B) if three_d else (B,)
            for got, want, bound, (s1, s2) in zip(outs, vals, bnds, f.output_sizes):
                assert isinstance(got, np.ndarray)
                assert got.shape == lead + (() if s1 * s2 == 1 else (s1,) if s2 == 1 else (s1, s2))
                ratio = fc.worst_ratio(got, want[:R, :B], bound[:R, :B])
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, R, B, ratio)
    print("%s: worst |device - host| in units of 2 (bound + bound): %.3g" % (name, worst))


def _ulp(x):
    """the spacing of the doubles at |x|, normal or not"""
    return np.maximum(np.spacing(np.abs(x)), 2.0 ** -1074)


@pytest.mark.parametrize("name", fc.EXACT)
def test_every_entry_is_within_twice_the_running_bound_of_the_exact_value(dfn, name):
    """|device - exact| <= 2 running_bound, entry by entry, against the same DAG at 40 digits: the rule the host
    evaluator is held to in test_function_codegen.py, for the device alone"""
    f = dfn(name)
    _, bnds = fc.reference(name)
    his, los = fc.exact_reference(name)
    R, B = fc.lead(name)
    full = _as_tuple(f(*_args(name, R, B)))
    worst = 0.0
    for k, (got, hi, lo, bound) in enumerate(zip(full, his, los, bnds)):
        ratio = fc.worst_exact_ratio(got, hi, lo, bound)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, k, ratio)
    # the smaller shapes give the bits of the full one, row by row (so they are within the rule as well)
    for R_, B_ in fc.shapes(name):
        for got, whole in zip(_as_tuple(f(*_args(name, R_, B_))), full):
            assert got.tobytes() == np.ascontiguousarray(whole[:R_, :B_]).tobytes(), (name, R_, B_)
    print("%s: worst |device - exact| in units of 2 bound: %.3g" % (name, worst))
    if name == "trig":
        # sincos_joint itself, in units in the last place of the exact value: its straight-line path (|x| <= 1e5) and
        # the library path beyond
        x = fc.pool(name)[0]
        err = np.abs((his[0] - full[0].reshape(his[0].shape)) + los[0]) / _ulp(his[0])
        fast = np.abs(x) <= 1e5
        assert fast.sum() > 1300 and (~fast).sum() == 16
        for what, sel in (("fast", fast), ("library", ~fast)):
            print("trig: sincos_joint, %s path: worst error %.3f ulp (sin), %.3f ulp (cos) over %d arguments"
                  % (what, err[sel][:, 0, 0].max(), err[sel][:, 1, 0].max(), sel.sum()))


def test_selections_at_their_ties_match_the_written_out_rules_bit_for_bit(dfn):
    f = dfn("ties")
    vals, _ = fc.reference("ties")
    R, B = fc.lead("ties")
    outs = _as_tuple(f(*_args("ties", R, B)))
    for got, want, (s1, s2) in zip(outs, vals, f.output_sizes):
        assert got.reshape(want.shape).tobytes() == want.tobytes()
    for r, b in [(0, 0), (0, 1), (0, 2), (1, 63), (2, 256)]:
        for got, want in zip(outs, fc.ties_expected(fc.point("ties", r, b))):
            assert got[r, b].reshape(want.shape).tobytes() == want.tobytes(), (r, b)


def test_finite_inputs_with_infinite_or_exact_results_give_the_hosts_bits(dfn):
    """log(0), exp(+-800), 1 / 0, tanh(+-1e3), 0 ** -1: -inf, inf or 0, inf, +-1, inf - and the exact results at 1, 0,
    2, 0, 4.  (Nothing is promised for a NaN result: the device code is built with -fno-honor-nans.)"""
    f = dfn("edges")
    got = f(fc.EDGE_POINTS)
    assert got.shape == (3, 5) and got.tobytes() == fc.EDGE_VALUES.tobytes(), got
    host = np.stack([fc.host_call(fc.get("edges"), (p,))[0][:, 0] for p in fc.EDGE_POINTS])
    assert got.tobytes() == host.tobytes()


# ---- broadcasting ----------------------------------------------------------------------------------------------------------
def test_every_form_of_an_argument_equals_the_expanded_call_bit_for_bit(dfn):
    import torch
    f = dfn("manip")
    R, B = 3, 65
    t_pool, q_pool = fc.pool("manip")
    q = np.ascontiguousarray(q_pool[:R, :B])
    t_rec = np.ascontiguousarray(t_pool[:R, 0])
    # a Python float
    full = f(np.full((R, B), 0.75), q)
    for a, b in zip(f(0.75, q), full):
        assert a.tobytes() == b.tobytes()
    # [R]: one per record; also as [R, 1]
    full = f(np.ascontiguousarray(np.broadcast_to(t_rec[:, None], (R, B))), q)
    for form in (t_rec, t_rec[:, None]):
        for a, b in zip(f(form, q), full):
            assert a.tobytes() == b.tobytes()
    # [R, B] is the expanded call itself: the time is not read, so every form gives the same p, J and cost
    for a, b in zip(f(np.ascontiguousarray(t_pool[:R, :B]), q), full):
        assert a.tobytes() == b.tobytes()
    # a 2-D q with t as [B]: one record
    one = f(np.ascontiguousarray(t_pool[0, :B]), q[0])
    for a, b in zip(one, full):
        assert a.shape == b.shape[1:] and a.tobytes() == b[0].tobytes()
    # a [B] block of q shared by all records, and one q for all rows
    shared = f(t_rec[:, None], q[1])
    for a, b in zip(shared, f(t_rec, np.ascontiguousarray(np.broadcast_to(q[1], (R, B, 6))))):
        assert a.tobytes() == b.tobytes()
    single = f(np.zeros(B), q[2, 7])
    assert single[0].shape == (B, 3) and (single[0] == full[0][2, 7]).all() and (single[2] == full[2][2, 7]).all()
    # a function that READS its per-record and shared inputs: wide's s as [R], M shared, against the expanded call
    w = dfn("wide")
    a_, M_, s_ = (np.ascontiguousarray(v[:R, :B]) for v in fc.pool("wide"))
    got = w(a_, M_[0, 0], s_[:, 0])
    want = w(a_, np.ascontiguousarray(np.broadcast_to(M_[0, 0], (R, B, 3, 2))),
             np.ascontiguousarray(np.broadcast_to(s_[:, :1], (R, B))))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match="argument 1 of manip"):
        f(0.0, np.zeros((R, B, 5)))
    with pytest.raises(TypeError):
        f(q)
    del torch


# ---- determinism and containers --------------------------------------------------------------------------------------------
def test_determinism_halves_containers_out_and_the_empty_batch(dfn):
    import torch
    f = dfn("tool")
    dev = f._device
    R, B = 3, 257
    q, = _args("tool", R, B)
    a = f(q)
    b = f(q)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # a row's result does not depend on its lane: the two halves of a batch, concatenated, are the whole
    h = 100
    lo, hi = f(np.ascontiguousarray(q[:, :h])), f(np.ascontiguousarray(q[:, h:]))
    for whole, x, y in zip(a, lo, hi):
        assert np.concatenate([x, y], axis=1).tobytes() == whole.tobytes()
    # tensor in, tensor out, on the same device; a contiguous float64 tensor is read in place
    qd = torch.from_numpy(q).to(dev)
    td = f(qd)
    assert all(isinstance(x, torch.Tensor) and x.device == dev and x.dtype == torch.float64 for x in td)
    assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(td, a))
    assert torch.equal(qd.cpu(), torch.from_numpy(q))
    # out= is filled in place and returned
    outs = (torch.full((R, B, 4, 4), -7.0, dtype=torch.float64, device=dev),
            torch.full((R, B, 3), -7.0, dtype=torch.float64, device=dev))
    back = f(qd, out=outs)
    assert back[0] is outs[0] and back[1] is outs[1]
    assert torch.equal(outs[0], td[0]) and torch.equal(outs[1], td[1])
    with pytest.raises(ValueError, match=r"out\[1\] of tool must have shape"):
        f(qd, out=(outs[0], outs[1][:, :, :2]))
    with pytest.raises(ValueError, match="must hold 2 tensor"):
        f(qd, out=outs[0])
    # mixed arguments give tensors
    m = dfn("manip")
    assert all(isinstance(x, torch.Tensor) for x in m(0.0, qd))
    # an empty batch: empty arrays of the right shape, no launch
    e = f(np.zeros((0, 6)))
    assert e[0].shape == (0, 4, 4) and e[1].shape == (0, 3)
    e = f(torch.zeros((R, 0, 6), dtype=torch.float64, device=dev))
    assert tuple(e[0].shape) == (R, 0, 4, 4) and tuple(e[1].shape) == (R, 0, 3)
    # the shorthand builds the same kernel
    assert fc.get("tool").on_device().kernel_name == f.kernel_name


# ---- trajectory use --------------------------------------------------------------------------------------------------------
def _point_skill(fk):
    """the five-set UR5 skill of tests/test_gpu_rollout_record.py (its recording rollout is among the recorded
    instantiations)"""
    t, q = cs.MX.sym("t"), cs.MX.sym("q", 6)
    p = fk["T_fk"](q)[:3, 3]
    lo, hi = np.array(fk["lower"]), np.array(fk["upper"])
    cons = [cc.EqualityConstraint("dist", cs.norm_2(np.array([0.5, 0.5, 0.5]) - p), gain=50.0,
                                  constraint_type="soft", priority=6)]
    for i in range(5):
        cons.append(cc.SetConstraint("limit_q_%d" % i, q[i], set_min=0.3 * lo[i], set_max=0.3 * hi[i], priority=i))
    return cc.SkillSpecification("point", t, q, constraints=cons)


def test_the_records_of_a_rollout_go_in_as_they_are(dfn, ur5_fk):
    import torch
    f = dfn("tool")
    ctrl = cc.PseudoInverseController(skill_spec=_point_skill(ur5_fk))
    ctrl.setup_problem_functions()
    ctrl.setup_solver()
    B, n_ticks, dt = 65, 32, 0.008
    lo, hi = np.array(ur5_fk["lower"]), np.array(ur5_fk["upper"])
    Q = torch.from_numpy(np.random.default_rng(5).uniform(0.35 * lo, 0.35 * hi, size=(B, 6))).to(f._device)
    rec = ctrl.rollout_batch(dt * np.arange(n_ticks), Q, dt=dt, max_speed=0.4, record_every=1)[-1]
    q = rec["q"]
    assert isinstance(q, torch.Tensor) and tuple(q.shape) == (n_ticks, B, 6) and q.is_contiguous()
    before = q.clone()
    T, p = f(q)
    assert tuple(T.shape) == (n_ticks, B, 4, 4) and tuple(p.shape) == (n_ticks, B, 3)
    assert torch.equal(q, before)
    for r in range(n_ticks):
        Tr, pr = f(q[r])
        assert torch.equal(Tr, T[r]) and torch.equal(pr, p[r])
    assert torch.equal(T[..., :3, 3], p)
    qh, Th, ph = q.cpu().numpy(), T.cpu().numpy(), p.cpu().numpy()
    fn = fc.get("tool")
    for r, b in [(0, 0), (13, 64), (n_ticks - 1, 31)]:
        want, bound = fc.host_call(fn, (qh[r, b],)), fc.running_bound(fn, (qh[r, b],))
        assert fc.worst_ratio(Th[r, b], want[0], bound[0]) <= 1.0
        assert fc.worst_ratio(ph[r, b], want[1], bound[1]) <= 1.0
    assert np.abs(ph[-1] - ph[0]).max() > 1e-3          # (the tool moved: the records are not one state 32 times)


# ---- isolation of a bad row ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tool", "manip"])
def test_a_nan_row_leaves_every_other_row_alone(dfn, name):
    f = dfn(name)
    B, bad = 65, 40
    args = list(_args(name, 1, B, three_d=False))
    clean = _as_tuple(f(*args))
    q = args[-1].copy()
    q[bad, 2] = np.nan
    poisoned = _as_tuple(f(*(args[:-1] + [q])))
    keep = np.arange(B) != bad
    for a, b in zip(poisoned, clean):
        assert a[keep].tobytes() == b[keep].tobytes()
