"""The stable evaluation of the oracle's pseudo-inverse (tests/exact_yardstick.py::dpinv_stable) deserves to be the
yardstick of tests/test_gpu_structural_parity.py: on the first 64 instances of every batch that file uses it agrees
with the 50-digit evaluation of the literal formula to an eighth of the structural bound, while the literal fp64
oracle misses that bound on most of the 7-DoF stack.  No GPU."""
import functools

import numpy as np
import pytest

import exact_yardstick as ey
from tolerances import (FACTOR, FLOOR, ILL_POSED, LAST, MAX_LEFT_OUT, U, kappa_structural, pinv_close,
                        pinv_close_structural, rel_err, rtol_from_cond)

ROWS = 64
ALL_CASES = ey.PARITY_CASES + [ey.NEAR_SINGULAR]


@functools.lru_cache(maxsize=None)
def _solved(case, which):
    # (computed once per case and evaluation, shared by the tests below and never written to)
    fn = {"stable": ey.dpinv_stable, "exact": ey.dpinv_exact, "literal": None}[which]
    out = ey.solve(case, fn, ROWS)
    for arrays in out:
        for a in arrays:
            a.setflags(write=False)
    return out


def test_default_call_is_the_literal_path_bit_for_bit():
    """`pinv_fn=None` must leave `pinv_solve_batch` what bench.py, smoke() and every earlier test compare against: the
    same bits as handing it `dpinv` itself, and as the literal formula (pseudo_inverse.py:92-105) restated here."""
    from oracle import clik_oracle

    def frozen(J, opt, cond=None):
        rows, cols = J.shape
        assert opt["pinv_method"] == "damped"
        lam = opt["damping_factor"]
        inner = J.dot(J.T) + lam * np.eye(rows) if cols >= rows else J.T.dot(J) + lam * np.eye(cols)
        if cond is not None:
            w = np.linalg.eigvalsh(inner)
            cond[0] += float(abs(w[-1]) / abs(w[0]))
        return np.linalg.solve(inner, J).T if cols >= rows else np.linalg.solve(inner, J.T)
    spec, opts, stamps, Q, Y = ey.STACK_CASES["iiwa", "mixed"].build()
    got = []
    for fn in (None, clik_oracle.dpinv, frozen):
        kappa, margin = np.ones(ROWS), np.full(ROWS, np.inf)
        kw = {} if fn is None else {"pinv_fn": fn}
        dq, mode = clik_oracle.pinv_solve_batch(spec, opts, stamps[0], Q[:ROWS], Y=Y[:ROWS], cond_out=kappa,
                                                margins_out=margin, **kw)
        got.append((dq, mode, kappa, margin))
    assert set(np.unique(got[0][1])) == {0, 1}
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert a.tobytes() == b.tobytes()
    # and the bookkeeping of the old rule still finds the default call's condition numbers
    assert clik_oracle.condition_of(got[2][0]) is not None and pinv_close(got[2][0], got[2][0])


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_stable_evaluation_against_the_exact_one(case):
    """same modes; err <= (1 / 8) max(FLOOR, FACTOR u kappa_r) on every posed instance; at most MAX_LEFT_OUT left out"""
    for (ds, ms, ks, _), (de, me, ke, _) in zip(_solved(case, "stable"), _solved(case, "exact")):
        assert np.array_equal(ms, me)
        assert np.array_equal(ks, ke)                 # (both report kappa_r)
        tol = rtol_from_cond(ks)
        posed = tol < ILL_POSED
        assert (~posed).sum() <= MAX_LEFT_OUT * len(tol), (case, int((~posed).sum()))
        err = rel_err(ds, de)
        print("%s: kappa_r median %.1e max %.1e, share at the floor %.2f, worst err %.1e = %.4f of the bound" % (
            case, np.median(ks), ks.max(), (tol <= FLOOR).mean(), err[posed].max(), (err / tol)[posed].max()))
        assert (err[posed] <= tol[posed] / 8.0).all(), (case, float((err / tol)[posed].max()))
        assert pinv_close_structural(ds, de, ks) and LAST["rule"] == "kappa_r" and LAST["left_out"] == int((~posed).sum())


def test_literal_oracle_misses_the_structural_bound_on_the_redundant_arm():
    """why the literal oracle cannot be the yardstick: on the 7-DoF stack its own distance from the exact answer exceeds
    max(FLOOR, FACTOR u kappa_r) on at least half of the instances (its Gram matrix of [J; J] has an eigenvalue lam for
    every configuration); on the 6-DoF arm, where the old and the new bound coincide, it stays within."""
    beyond, count = 0, 0
    for (robot, dist), case in ey.STACK_CASES.items():
        (dl, ml, kl, _), (de, me, kr, _) = _solved(case, "literal")[0], _solved(case, "exact")[0]
        assert np.array_equal(ml, me)
        tol, old = rtol_from_cond(kr), rtol_from_cond(kl)
        err = rel_err(dl, de)
        print("%s: literal against exact worst err %.1e = %.1f of the structural bound (median %.1e), %.3f of the old "
              "one (median %.1e); beyond the structural bound: %d of %d" % (
                  case, err.max(), (err / tol).max(), np.median(tol), (err / old).max(), np.median(old),
                  (err > tol).sum(), len(err)))
        assert (err <= old).all()                  # (the old rule does cover the literal oracle's own noise)
        if robot == "iiwa":
            beyond, count = beyond + int((err > tol).sum()), count + len(err)
        else:
            assert (err <= tol).all()
    assert 2 * beyond >= count, (beyond, count)


def test_kappa_structural_ignores_what_the_stack_makes_zero():
    rng = np.random.default_rng(0)
    J = rng.normal(size=(6, 7))
    s = np.linalg.svd(J, compute_uv=False)
    lam = 1e-7
    assert np.isclose(kappa_structural(J, lam), (s[0] ** 2 + lam) / (s[-1] ** 2 + lam), rtol=1e-12)
    # [J; J]: twelve rows of rank six - the literal Gram matrix has condition (2 s1^2 + lam) / lam
    assert np.isclose(kappa_structural(np.vstack([J, J]), lam), (2 * s[0] ** 2 + lam) / (2 * s[-1] ** 2 + lam), rtol=1e-9)
    S = np.diag([1.0, 0, 0, 1, 0, 0, 0])
    assert kappa_structural(S, lam) == 1.0 and kappa_structural(np.zeros((3, 7)), lam) == 1.0
    assert kappa_structural(np.full((2, 2), np.nan), lam) == float("inf")
    # a genuinely small singular value (above 1e-8 s1) counts
    D = np.diag([1.0, 1e-5])
    assert np.isclose(kappa_structural(D, lam), (1 + lam) / (1e-10 + lam))


def test_structural_rule_keeps_the_old_rules_body():
    """same FACTOR / FLOOR / ILL_POSED / MAX_LEFT_OUT, the NaN rule and the LAST bookkeeping"""
    ref = np.ones((8, 3))
    kr = np.full(8, 1e3)
    assert pinv_close_structural(ref + 0.9 * FLOOR * 2, ref, kr) and LAST == dict(rule="kappa_r", checked=8, left_out=0,
                                                                                  worst=LAST["worst"])
    assert not pinv_close_structural(ref + 1.1 * FLOOR * 2, ref, kr)
    kr[0] = 1e6                 # (bound FACTOR u 1e6 = 8.9e-10 for that instance only)
    a = ref.copy()
    a[0] += 1.5e-9
    assert pinv_close_structural(a, ref, kr)
    a[1] += 1.5e-9
    assert not pinv_close_structural(a, ref, kr)
    assert np.isclose(rtol_from_cond(kr)[0], FACTOR * U * 1e6)
    kr[:] = 1e3
    kr[:2] = 1e16               # two of eight ill-posed: left out, counted
    assert pinv_close_structural(a, ref, kr) and LAST["left_out"] == 2 and LAST["checked"] == 6
    kr[:3] = 1e16               # three of eight: more than MAX_LEFT_OUT
    assert not pinv_close_structural(ref, ref, kr)
    kr[:] = 1e3
    b = ref.copy()
    b[5, 1] = np.nan
    assert not pinv_close_structural(b, ref, kr) and LAST["rule"] == "nan"
    rows = np.ones(8, dtype=bool)
    rows[5] = False
    assert pinv_close_structural(b, ref, kr, rows=rows) and LAST["checked"] == 7
    with pytest.raises(AssertionError):
        pinv_close_structural(ref, ref, None)
