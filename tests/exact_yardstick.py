"""Two more evaluations of the oracle's damped pseudo-inverse, for `clik_oracle.pinv_solve_batch(..., pinv_fn=)`, and
the skills and batches the structural-parity tests run them on (tests/test_exact_yardstick.py on the CPU,
tests/test_gpu_structural_parity.py on the device).  TEST INFRASTRUCTURE ONLY.

  dpinv_stable   V diag(s / (s^2 + lam)) U' from the SVD of J: the same function of J as the literal
                 J'(JJ' + lam I)^-1, without forming the Gram matrix whose structural zeros the damping lifts to lam
                 (condition 1e8 at the default damping, whatever the configuration).  The yardstick for ARITHMETIC.
  dpinv_exact    the literal formula in 50-digit mpmath from the fp64 matrix, rounded once.  What the stable one is
                 held to (tests/test_exact_yardstick.py); too slow for anything else.

Both add `tolerances.kappa_structural(J, lam)` to `cond`, so `cond_out` of a solve with either is kappa_r, the bound
of `tolerances.pinv_close_structural`."""
import numpy as np

from tolerances import kappa_structural

DIGITS = 50


def dpinv_stable(J, opt, cond=None):
    """drop-in for `clik_oracle.dpinv`.  pinv_method "standard" keeps the literal form (undamped and rank-deficient
    has no answer to be stable about) and the literal condition number."""
    from oracle import clik_oracle
    if opt["pinv_method"] == "standard":
        return clik_oracle.dpinv(J, opt, cond)
    lam = opt["damping_factor"]
    if cond is not None:
        cond[0] += kappa_structural(J, lam)
    if not np.isfinite(J).all():
        return np.full(J.shape[::-1], np.nan)       # (a poisoned instance, as the literal solve answers it)
    Us, s, Vt = np.linalg.svd(J, full_matrices=False)
    return (Vt.T * (s / (s * s + lam))).dot(Us.T)


_EXACT = {}          # (shape, bytes of J, lam) -> (pinv, kappa_r): one stack hands the same J to dpinv three times


def dpinv_exact(J, opt, cond=None):
    """drop-in for `clik_oracle.dpinv`: J'(JJ' + lam I)^-1 for a wide or square J, (J'J + lam I)^-1 J' for a tall one
    (pseudo_inverse.py:92-105), every operation at DIGITS decimal digits, the result rounded to fp64 once.  lam = 0 for
    pinv_method "standard" (mpmath raises on a singular Gram matrix)."""
    import mpmath as mp
    J = np.ascontiguousarray(J, dtype=float)
    lam = 0.0 if opt["pinv_method"] == "standard" else float(opt["damping_factor"])
    key = (J.shape, J.tobytes(), lam)
    if key not in _EXACT:
        rows, cols = J.shape
        with mp.workdps(DIGITS):
            M = mp.matrix(J.tolist())
            if cols >= rows:
                P = M.T * mp.inverse(M * M.T + mp.mpf(lam) * mp.eye(rows))
            else:
                P = mp.inverse(M.T * M + mp.mpf(lam) * mp.eye(cols)) * M.T
            out = np.array([[float(P[i, j]) for j in range(P.cols)] for i in range(P.rows)])
        if len(_EXACT) > 4096:
            _EXACT.clear()
        _EXACT[key] = (out, kappa_structural(J, lam))
    out, kr = _EXACT[key]
    if cond is not None:
        cond[0] += kr
    return out.copy()


def solve(case, pinv_fn, rows=None):
    """the oracle's algorithm on a case's batch (or its first `rows` instances) with `pinv_fn` (None: the literal
    `dpinv`) at every time stamp of the case -> list of (dq [B, n], mode [B], cond_out [B], margin [B])"""
    from oracle import clik_oracle
    spec, opts, stamps, Q, Y = case.build()
    Q = Q[:rows]
    Y = None if Y is None else Y[:rows]
    out = []
    for t in stamps:
        kappa, margin = np.ones(len(Q)), np.full(len(Q), np.inf)
        dq, mode = clik_oracle.pinv_solve_batch(spec, opts, t, Q, Y=Y, cond_out=kappa, margins_out=margin,
                                                pinv_fn=pinv_fn)
        out.append((dq, mode, kappa, margin))
    return out


# ---- the skills and batches of the structural-parity tests ---------------------------------------------------------
B_TICK = 257            # seventeen team waves (sixteen instances each), four lane waves and a tail


class Case(object):
    """`build()` -> (spec, options, time stamps, Q, Y | None); built once, on first use"""

    def __init__(self, name, make):
        self.name, self._make, self._built = name, make, None

    def build(self):
        if self._built is None:
            self._built = self._make()
        return self._built

    def __repr__(self):
        return self.name


def _fk(robot):
    from casclik_amd import skills
    return skills.iiwa() if robot == "iiwa" else skills.ur5()


def _stack(robot, dist):
    from casclik_amd import skills
    fk = _fk(robot)
    Q, Y = skills.synthetic_inputs(fk, B_TICK, seed=3, distribution=dist)
    return skills.stack_skill(fk), dict(skills.STACK_OPTIONS), (0.0,), Q, Y


def _family(gain_matrix, one_sided, feedforward):
    """the members of tests/test_gpu_team.py::test_team_kernel_family_members, at the later of its two time stamps"""
    from casclik_amd import skills
    from test_gpu_team import _custom_stack
    fk = _fk("iiwa")
    Q, Y = skills.synthetic_inputs(fk, B_TICK, seed=21, distribution="mixed")
    return _custom_stack(fk, gain_matrix, one_sided), dict(skills.STACK_OPTIONS, feedforward=feedforward), (0.7,), Q, Y


def _twenty():
    """the pinv stack of tests/test_gpu_qp.py::test_twenty_constraints_in_one_skill: two 1-D sets, a position task and
    seventeen more equalities and velocity targets behind each other, its batch of 96"""
    import casclik_amd as cc
    from casclik_amd import skills, sym as cs
    fk = _fk("iiwa")
    t, q, y = cs.MX.sym("t"), cs.MX.sym("q", 7), cs.MX.sym("y", 3)
    T = fk["T_fk"](q)
    lo, hi = np.array(fk["lower"]), np.array(fk["upper"])
    cons = [cc.SetConstraint(label="limit_q%d" % j, expression=q[j], set_min=0.5 * lo[j], set_max=0.5 * hi[j], priority=j)
            for j in range(2)]
    cons.append(cc.EqualityConstraint(label="position", expression=T[:3, 3] - y, gain=3.0, constraint_type="soft", priority=10))
    cons += [cc.EqualityConstraint(label="rest_q%d" % j, expression=q[j] - 0.1 * (j + 1), gain=0.3 + 0.1 * j,
                                   constraint_type="soft", priority=20 + j) for j in range(7)]
    cons += [cc.VelocityEqualityConstraint(label="drift_q%d" % j, expression=q[j], target=0.01 * (j - 3),
                                           constraint_type="soft", priority=40 + j) for j in range(7)]
    cons += [cc.EqualityConstraint(label="pair_%d" % j, expression=q[j] + q[j + 1], gain=0.2, constraint_type="soft",
                                   priority=60 + j) for j in range(3)]
    Q, Y7 = skills.synthetic_inputs(fk, 96, seed=12, distribution="mixed")
    return cc.SkillSpecification("twenty", t, q, input_var=y, constraints=cons), None, (0.3,), Q, Y7[:, :3]


def _tall():
    """tests/test_gpu_branches.py::test_tall_first_equality_is_processed_twice: an 8 x 6 first equality on the UR5 and a
    joint-space task behind it (projected through [J; J]), damping 1e-4"""
    import casclik_amd as cc
    from casclik_amd import skills, sym as cs
    fk = _fk("ur5")
    t, q = cs.MX.sym("t"), cs.MX.sym("q", 6)
    T = fk["T_fk"](q)
    frame = cc.EqualityConstraint("frame", cs.vertcat(T[:3, 3] - np.array([0.4, 0.1, 0.4]),
                                                      T[:3, 0] - np.array([0.0, 1.0, 0.0]),
                                                      T[:2, 1] - np.array([1.0, 0.0])), gain=4.0, priority=0)
    rest = cc.EqualityConstraint("rest", q - np.array([0.0, -1.2, 1.0, -1.0, 0.3, 0.0]), gain=0.3, priority=1)
    Q, _ = skills.synthetic_inputs(fk, B_TICK, seed=6)
    return cc.SkillSpecification("tall", t, q, constraints=[frame, rest]), {"damping_factor": 1e-4}, (0.0,), 0.3 * Q, None


def _near_singular():
    """the batch of tests/test_gpu_team.py::test_team_kernel_near_singular: every joint of the iiwa within 1e-5 of zero"""
    from casclik_amd import skills
    fk = _fk("iiwa")
    Q = np.random.default_rng(8).normal(0.0, 1e-5, size=(128, 7))
    _, Y = skills.synthetic_inputs(fk, 128, seed=2)
    return skills.stack_skill(fk), dict(skills.STACK_OPTIONS), (0.0,), Q, Y


STACK_CASES = {(robot, dist): Case("stack-%s-%s" % (robot, dist), lambda r=robot, d=dist: _stack(r, d))
               for robot in ("iiwa", "ur5") for dist in ("interior", "mixed")}
FAMILY_CASES = {(g, o, f): Case("family-%s-%s-%s" % ("matrixgain" if g else "scalargain", "onesided" if o else "twosided",
                                                      "ff" if f else "noff"), lambda g=g, o=o, f=f: _family(g, o, f))
                for g in (False, True) for o in (False, True) for f in (True, False)}
TWENTY = Case("twenty-constraints", _twenty)
TALL = Case("tall-first-equality", _tall)
NEAR_SINGULAR = Case("stack-iiwa-near-singular", _near_singular)
# the cases the new rule must HOLD on (the near-singular batch only has to be posed and no looser than the old rule)
PARITY_CASES = list(STACK_CASES.values()) + list(FAMILY_CASES.values()) + [TWENTY, TALL]
