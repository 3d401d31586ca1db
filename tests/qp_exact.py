"""The exact yardstick of the QP path, and the weakly active cases it alone can judge.  TEST INFRASTRUCTURE ONLY
(tests/test_qp_exact_yardstick.py on the CPU, tests/test_gpu_qp_exact_parity.py on the device).

  qp_exact           the unique minimiser of  min 1/2 x'Hx  s.t.  lb <= A x <= ub  (H = diag(hd) > 0) at DIGITS decimal
                     digits, rounded to fp64 once, with its working set and multipliers.  An active-set polish of the
                     literal oracle's answer; what it returns carries the optimality certificate (primal feasibility
                     and multiplier signs at DIGITS digits), or it raises.
  kappa_qp_active    cond+(Aa H^-1 Aa') of the returned working set: the condition of the system every solver's algebra
                     reduces to, WITHOUT the cond(H) factor of `clik_oracle.qp_condition` (diagonal scaling, which limits
                     no correct solver).  The bound of `tolerances.qp_close_exact`.
  weak_bound_cases   instances whose minimiser has one state within |ds| of its bound, on either side: what no random
                     batch reaches and every threshold-stopped solver (the kernels' and the literal oracle's) gets wrong
                     by its threshold over the smallest curvature.  The minimiser is continuous across such a point, so
                     the exact reference is well defined there."""
import numpy as np

DIGITS = 50
VIOLATION = 1e-40         # anything beyond this is a violation / a wrong sign / a dependent row, at DIGITS digits
START_TOL = 1e-8          # rows the starting point has within this (relative to max(1, |bound|)) of a bound start active
OFFSETS = (-1e-5, -1e-7, -1e-9, -1e-11, 0.0, 1e-11, 1e-9, 1e-7, 1e-5)


def _mp():
    import mpmath
    return mpmath


def _solve_working_set(mp, hinv, Am, rows, bounds):
    """x = H^-1 Aa' lam,  S lam = b_a  for the independent rows in `rows` -> (x, lam by row, rows kept).  Rows dependent on
    the ones before them in the H^-1 inner product (tested at DIGITS digits) are dropped."""
    nv = len(hinv)
    kept, basis = [], []            # (basis: the rows orthogonalised in the H^-1 inner product, with their squared norms)
    for i in rows:
        v = [Am[i][j] for j in range(nv)]
        n0 = mp.fsum(v[j] * v[j] * hinv[j] for j in range(nv))
        for w, nw in basis:
            c = mp.fsum(v[j] * w[j] * hinv[j] for j in range(nv)) / nw
            v = [v[j] - c * w[j] for j in range(nv)]
        n1 = mp.fsum(v[j] * v[j] * hinv[j] for j in range(nv))
        if n0 == 0 or n1 <= mp.mpf(VIOLATION) * n0:
            continue
        basis.append((v, n1))
        kept.append(i)
    x = [mp.mpf(0)] * nv
    lam = {}
    if kept:
        k = len(kept)
        S = mp.matrix(k, k)
        for a in range(k):
            for b in range(a + 1):
                S[a, b] = S[b, a] = mp.fsum(Am[kept[a]][j] * hinv[j] * Am[kept[b]][j] for j in range(nv))
        sol = mp.lu_solve(S, mp.matrix([bounds[i] for i in kept]))
        lam = {i: sol[a] for a, i in enumerate(kept)}
        x = [hinv[j] * mp.fsum(Am[i][j] * lam[i] for i in kept) for j in range(nv)]
    return x, lam, kept


def qp_exact(hd, A, lb, ub, x0, full=False):
    """-> (x [nv], W: sorted row indices of the working set, lam [nc]: signed multipliers, H x = A' lam, >= 0 on a lower
    bound and <= 0 on an upper one).  `x0`: the literal oracle's answer (any point does; it only seeds the working set).
    `full`: also the number of passes the polish needed and x, lam as mpmath numbers."""
    mp = _mp()
    hd, A, lb, ub = (np.asarray(v, dtype=float) for v in (hd, A, lb, ub))
    nc, nv = A.shape
    with mp.workdps(DIGITS):
        hinv = [1 / mp.mpf(float(h)) for h in hd]
        Am = [[mp.mpf(float(A[i, j])) for j in range(nv)] for i in range(nc)]
        eq = [i for i in range(nc) if not ub[i] - lb[i] > 0.0]
        side = {i: 0 for i in eq}                       # row -> -1 lower bound, +1 upper bound, 0 equality
        Ax0 = A.dot(np.asarray(x0, dtype=float))
        for i in range(nc):
            if i in side:
                continue
            if np.isfinite(lb[i]) and abs(Ax0[i] - lb[i]) <= START_TOL * max(1.0, abs(lb[i])):
                side[i] = -1
            elif np.isfinite(ub[i]) and abs(Ax0[i] - ub[i]) <= START_TOL * max(1.0, abs(ub[i])):
                side[i] = +1

        def bound_of(i, s):
            return mp.mpf(float(0.5 * (lb[i] + ub[i]) if s == 0 else (lb[i] if s < 0 else ub[i])))

        tiny = mp.mpf(VIOLATION)
        for passes in range(4 * nc + 1):
            rows = eq + sorted(i for i in side if side[i] != 0)
            x, lam, kept = _solve_working_set(mp, hinv, Am, rows, {i: bound_of(i, side[i]) for i in rows})
            for i in rows:
                if i not in lam and side[i] != 0:
                    del side[i]                          # (dependent: the rows before it decide)
            # the multiplier with the wrong sign by the most leaves
            worst, out = tiny, None
            for i in kept:
                wrong = lam[i] * side[i]                 # (lower bound: lam < 0 is wrong; upper bound: lam > 0)
                if side[i] != 0 and wrong > worst:
                    worst, out = wrong, i
            if out is not None:
                del side[out]
                continue
            # otherwise the most violated row joins
            worst, add = tiny, None
            for i in range(nc):
                ax = mp.fsum(Am[i][j] * x[j] for j in range(nv))
                if i in side and i in lam:
                    continue
                for s, b in ((-1, lb[i]), (+1, ub[i])):
                    if not np.isfinite(b):
                        continue
                    v = (mp.mpf(float(b)) - ax) * (-s) / max(1.0, abs(float(b)))
                    if v > worst:
                        worst, add = v, (i, s)
            if add is not None:
                if add[0] in side:
                    raise ArithmeticError("qp_exact: row %d is violated and depends on the working set: no minimiser" % add[0])
                side[add[0]] = add[1]
                continue
            W = np.array(sorted(lam), dtype=int)
            lam_out = np.zeros(nc)
            for i in kept:
                lam_out[i] = float(lam[i])
            out = (np.array([float(v) for v in x]), W, lam_out)
            return out + (passes, x, lam) if full else out
    raise ArithmeticError("qp_exact: no certificate within %d passes" % (4 * nc))


def kappa_qp_active(hd, A, W):
    """cond+(Aa H^-1 Aa') over the rows W, singular values below 1e-12 of the largest cut as `clik_oracle.qp_condition`
    cuts them; an empty working set gives 1"""
    W = np.asarray(W, dtype=int)
    if W.size == 0:
        return 1.0
    hd, Aa = np.asarray(hd, dtype=float), np.asarray(A, dtype=float)[W]
    sv = np.linalg.svd((Aa / hd[None, :]).dot(Aa.T), compute_uv=False)
    sv = sv[sv > 1e-12 * sv[0]]
    return float(sv[0] / sv[-1])


class Solved(object):
    """one batch through the literal oracle and the exact polish: `x` [B, nv] exact (NaN where the oracle reports
    infeasible or poisoned data), `dq`, `slack`, `kappa_s` [B], `status` (the oracle's), `W`, `lam`, `passes` per
    instance, `oracle_x`, `kappa` (the oracle's own, with the cond(H) factor), and the problem data"""

    def __init__(self, spec, t, Q, Y=None, weights=None, only=None):
        """`only`: the instances to polish and compare (the others keep the oracle's status and count as not `ok`)"""
        from oracle import clik_oracle
        self.hd, self.A, self.lb, self.ub = clik_oracle.qp_data_batch(spec, t, Q, Y=Y, weights=weights)
        B = len(self.hd)
        self.kappa = np.ones(B)
        odq, odx, oslack, self.status = clik_oracle.qp_solve_batch(spec, t, Q, Y=Y, weights=weights, cond_out=self.kappa)
        self.oracle_x = np.hstack([v for v in (odq, odx, oslack) if v is not None])
        self.x = np.full_like(self.oracle_x, np.nan)
        self.kappa_s, self.W, self.lam, self.passes = np.ones(B), [None] * B, [None] * B, np.zeros(B, dtype=int)
        chosen = np.ones(B, dtype=bool) if only is None else np.isin(np.arange(B), only)
        for b in np.nonzero((self.status == 0) & chosen)[0]:
            self.x[b], self.W[b], self.lam[b], self.passes[b] = qp_exact(
                self.hd[b], self.A[b], self.lb[b], self.ub[b], self.oracle_x[b], full=True)[:4]
            self.kappa_s[b] = kappa_qp_active(self.hd[b], self.A[b], self.W[b])
        nq = spec.n_robot_var
        nvirt = spec.n_virtual_var if spec.virtual_var is not None else 0
        self.dq, self.slack = self.x[:, :nq], self.x[:, nq + nvirt:]
        self.oracle_dq, self.oracle_slack = self.oracle_x[:, :nq], self.oracle_x[:, nq + nvirt:]
        for a in (self.x, self.kappa_s, self.kappa, self.status, self.oracle_x, self.hd, self.A, self.lb, self.ub):
            a.setflags(write=False)
        self.ok = (self.status == 0) & chosen


# ---- weakly active bounds ------------------------------------------------------------------------------------------
def state_rows(A, a):
    """the rows of one instance's A that bound the state `a` alone (a single entry, 1, in column a)"""
    unit = (A[:, a] == 1.0) & (np.count_nonzero(A, axis=1) == 1)
    return np.nonzero(unit)[0]


def _meeting_step(solve_free, bound, sign, reach, steps=44):
    """bisect for the step s in (0, reach] at which sign * (x_a(s) - bound) changes from negative to non-negative,
    x_a(s) = solve_free(s) the state of the QP WITHOUT the state's own bounds; None when it does not within `reach`"""
    lo = 0.0
    for hi in (0.25 * reach, 0.5 * reach, reach):
        xa = solve_free(hi)
        if xa is None:
            return None
        if sign * (xa - bound) >= 0.0:
            break
        lo = hi
    else:
        return None
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        xa = solve_free(mid)
        if xa is None:
            return None
        if sign * (xa - bound) >= 0.0:
            hi = mid
        else:
            lo = mid
    return hi


def weak_bound_cases(spec, fk, Q, Y, offsets=OFFSETS, t=0.0, reach=0.2, skip_states=(), limit=None):
    """For a skill whose soft task is affine in the target Y[:, :3] (the position part of `skills.qp_skill`'s pose, the
    whole input of the box-stack skills).  Per base instance: the free state a with the largest |x_a| / v_max,a (v_max
    from `fk`), not in `skip_states`; the target walked along +x, -x, +y, -y, +z, -z (the first that works) up to `reach`;
    the step s0 at which the state meets its bound, bisected on the QP without that state's bounds; one instance per
    offset at s0 + ds.  Negative ds leaves the bound inactive by a few |ds|, positive ds activates it with a multiplier of
    that order.  -> (Qw, Yw, info): the instances case-major (len(offsets) rows per case), info per row = (base index,
    state, +1 upper / -1 lower bound, bounding row, ds); `limit`: stop after that many cases."""
    from oracle import clik_oracle
    Q, Y = np.atleast_2d(np.asarray(Q, dtype=float)), np.atleast_2d(np.asarray(Y, dtype=float))
    vmax = np.asarray(fk["velocity"], dtype=float)
    base = clik_oracle.qp_solve_batch(spec, t, Q, Y=Y)
    hd, A, lb, ub = clik_oracle.qp_data_batch(spec, t, Q, Y=Y)
    nq = spec.n_robot_var
    Qw, Yw, info = [], [], []
    for b in range(len(Q)):
        if limit is not None and len(info) >= limit * len(offsets):
            break
        if base[3][b] != 0:
            continue
        x = base[0][b]
        # the state's own bounds: the tightest of the rows that bound it alone
        box = []
        for a in range(nq):
            rows = state_rows(A[b], a)
            box.append(None if rows.size == 0 else
                       (rows[np.argmax(lb[b, rows])], rows[np.argmin(ub[b, rows])], lb[b, rows].max(), ub[b, rows].min()))
        # (free: strictly inside its bounds, with a real bound - not the reference's 1e10 "none" - on the side it moves to)
        free = [a for a in range(nq) if a not in skip_states and box[a] is not None and box[a][2] < box[a][3]
                and box[a][2] + START_TOL < x[a] < box[a][3] - START_TOL
                and abs(box[a][3] if x[a] >= 0.0 else box[a][2]) < 1e9]
        if not free:
            continue
        a = max(free, key=lambda j: abs(x[j]) / vmax[j])
        sign = 1.0 if x[a] >= 0.0 else -1.0
        row, bound = (box[a][1], box[a][3]) if sign > 0 else (box[a][0], box[a][2])
        rows_a = state_rows(A[b], a)
        found = None
        for axis in range(3):
            for direction in (1.0, -1.0):

                def target(s, axis=axis, direction=direction):
                    y = Y[b].copy()
                    y[axis] += direction * s
                    return y

                def solve_free(s):
                    h1, A1, l1, u1 = clik_oracle.qp_data_batch(spec, t, Q[b:b + 1], Y=target(s)[None])
                    l1[0, rows_a], u1[0, rows_a] = -np.inf, np.inf
                    try:
                        return clik_oracle.qp_solve_dense(h1[0], A1[0], l1[0], u1[0])[a]
                    except clik_oracle.QPInfeasible:
                        return None

                s0 = _meeting_step(solve_free, bound, sign, reach)
                if s0 is None:
                    continue
                # a transversal crossing, and every offset's full problem has a minimiser
                below, above = solve_free(s0 + min(offsets)), solve_free(s0 + max(offsets))
                if below is None or above is None or not (sign * (below - bound) < 0.0 < sign * (above - bound)):
                    continue
                ys = np.stack([target(s0 + ds) for ds in offsets])
                if (clik_oracle.qp_solve_batch(spec, t, np.repeat(Q[b:b + 1], len(offsets), axis=0), Y=ys)[3] != 0).any():
                    continue
                found = ys
                break
            if found is not None:
                break
        if found is None:
            continue
        for ds, y in zip(offsets, found):
            Qw.append(Q[b])
            Yw.append(y)
            info.append((b, a, int(sign), int(row), ds))
    return np.array(Qw), np.array(Yw), info


def hold_hint(word, state, sign):
    """the box family's hot word (lower bounds in bits 0..15, upper bounds in bits 16..31, one bit per state) with the
    state HELD at the bound in question"""
    word = int(word) & 0xffffffff
    word |= 1 << (state if sign < 0 else 16 + state)
    if sign > 0:
        word &= ~(1 << state)                           # (a lower-bound bit would win over the upper one)
    return word - (1 << 32) if word >= (1 << 31) else word


# ---- the skills and batches of the exact-parity tests ---------------------------------------------------------------
B_TICK = 130            # two waves and a ragged tail of two: three blocks of the four-strategy kernel, the last nearly empty


def box_move_skill(fk):
    """the skill of tests/test_gpu_qp.py::test_qp_value_specialised_kernel_outside_the_box_family: a hard tool-position
    box (general rows), a soft move, hard speed limits on the UR5 -> (spec, home)"""
    import casclik_amd as cc
    from casclik_amd import sym as cs
    from time_skills import UR5_HOME as home
    t, q = cs.MX.sym("t"), cs.MX.sym("q", 6)
    p = fk["T_fk"](q)[:3, 3]
    p_home = fk["chain"].fk_numeric(home)[:3, 3]
    cons = [cc.SetConstraint("box_%d" % i, p[i], set_min=p_home[i] - 0.15, set_max=p_home[i] + 0.15, priority=i, gain=50.0)
            for i in range(3)]
    cons.append(cc.EqualityConstraint("move", p - (p_home + np.array([0.3, 0.0, 0.1])), priority=10, constraint_type="soft",
                                      gain=1.0))
    cons.append(cc.VelocitySetConstraint("speed", q, set_min=-0.6 * np.ones(6), set_max=0.6 * np.ones(6), priority=0))
    return cc.SkillSpecification("box_move", t, q, constraints=cons), home


def edge_skill(fk, case):
    """the "one_sided" and "pinned_state" skills of tests/test_gpu_qp.py::test_box_family_solver_edge_cases"""
    import casclik_amd as cc
    from casclik_amd import sym as cs
    from test_gpu_qp import _box_stack
    if case == "one_sided":
        return _box_stack(fk, 7, dict(set_min=np.asarray(fk["lower"], float), gain=2.0), speed=None)
    assert case == "pinned_state", case
    pin_lo, pin_hi = -0.8 * np.ones(7), 0.8 * np.ones(7)
    pin_lo[3] = pin_hi[3] = 0.25
    t, q, y = cs.MX.sym("t"), cs.MX.sym("q", 7), cs.MX.sym("y", 3)
    return cc.SkillSpecification("pinned", t, q, input_var=y, constraints=[
        cc.EqualityConstraint("tool_position", fk["T_fk"](q)[:3, 3] - y, gain=3.0, constraint_type="soft", priority=1),
        cc.VelocitySetConstraint("speed", q, set_min=pin_lo, set_max=pin_hi, priority=0)])


class QpCase(object):
    """`build()` -> (spec, t, Q, Y | None); `solved()` -> the batch through the oracle and the exact polish; `info`: per
    row of a weakly-active batch (base index, state, side, row, ds), None for a filler row.  Built once, on first use."""

    def __init__(self, name, make, only=None):
        self.name, self._make, self._built, self._solved, self.info, self.only = name, make, None, None, None, only

    def build(self):
        if self._built is None:
            built = self._make()
            self._built, self.info = built[:4], (built[4] if len(built) > 4 else None)
            for a in self._built[2:]:
                if a is not None:
                    a.setflags(write=False)
        return self._built

    def solved(self):
        if self._solved is None:
            spec, t, Q, Y = self.build()
            self._solved = Solved(spec, t, Q, Y, only=self.only)
        return self._solved

    def __repr__(self):
        return self.name


def _config4(dist):
    from casclik_amd import skills
    fk = skills.iiwa()
    Q, Y = skills.synthetic_inputs(fk, B_TICK, seed=3, distribution=dist)
    return skills.qp_skill(fk), 0.0, Q, Y


def _moe(soft_walls):
    from casclik_amd import skills
    from extern_skills import moe_box_skill
    spec, home = moe_box_skill(skills.ur5(), soft_walls=soft_walls)
    return spec, 3.0, home + np.random.default_rng(11).normal(scale=0.12, size=(B_TICK, 6)), None


def _box_move():
    from casclik_amd import skills
    spec, home = box_move_skill(skills.ur5())
    return spec, 0.0, home + np.random.default_rng(8).normal(scale=0.06, size=(B_TICK, 6)), None


def _many_rows():
    from casclik_amd import skills
    from test_gpu_qp import many_rows_skill
    fk = skills.iiwa()
    Q, Y = skills.synthetic_inputs(fk, B_TICK, seed=8, distribution="interior")
    return many_rows_skill(fk), 0.0, Q, Y


N_WEAK = 14             # cases per weakly-active batch: 14 x 9 offsets = 126 rows, and four filler rows to B_TICK
N_WEAK_EDGE = 8         # ... at least, on the edge skills (fewer of their instances reach a bound within the walk)
N_BASE = 48             # base instances the construction may draw from


def _pad_weak(Qw, Yw, info, Q, Y):
    fill = np.arange(B_TICK - len(info)) % len(Q)
    return np.vstack([Qw, Q[fill]]), np.vstack([Yw, Y[fill]]), list(info) + [None] * len(fill)


def _weak_config4():
    from casclik_amd import skills
    fk = skills.iiwa()
    spec = skills.qp_skill(fk)
    Q, Y = skills.synthetic_inputs(fk, N_BASE, seed=3, distribution="interior")
    Qw, Yw, info = _pad_weak(*weak_bound_cases(spec, fk, Q, Y, limit=N_WEAK), Q, Y)
    return spec, 0.0, Qw, Yw, info


def _weak_edge(case):
    from casclik_amd import skills
    fk = skills.iiwa()
    spec = edge_skill(fk, case)
    Q, Y = skills.synthetic_inputs(fk, N_BASE, seed=31, distribution="mixed")
    Y = Y[:, :3].copy()
    Qw, Yw, info = _pad_weak(*weak_bound_cases(spec, fk, Q, Y, limit=N_WEAK,
                                               skip_states=(3,) if case == "pinned_state" else ()), Q, Y)
    return spec, 0.0, Qw, Yw, info


CONFIG4 = {dist: QpCase("config4-%s" % dist, lambda d=dist: _config4(d)) for dist in ("interior", "mixed")}
MOE = {soft: QpCase("moe-%s-walls" % ("soft" if soft else "hard"), lambda s=soft: _moe(s)) for soft in (False, True)}
BOX_MOVE = QpCase("box-move", _box_move)
MANY_ROWS = QpCase("thirty-rows", _many_rows)
WEAK_CONFIG4 = QpCase("config4-weak", _weak_config4)
WEAK_EDGE = {case: QpCase("%s-weak" % case, lambda c=case: _weak_edge(c)) for case in ("pinned_state", "one_sided")}
RANDOM_CASES = list(CONFIG4.values()) + list(MOE.values()) + [BOX_MOVE]


# one-dimensional weak cases on a wall row of the Moe-2016 skill: the wall's set_max is a number of the skill, so every
# offset is a skill (and a controller) of its own.  Offsets in units of the row's bound: negative leaves the wall
# inactive by |ds|, positive activates it by ds.
WALL_OFFSETS = (-1e-6, -1e-9, 0.0, 1e-9, 1e-6)
WALL_ROWS = np.arange(B_TICK - 10, B_TICK)      # the rows compared: the ragged tail and the end of the wave before it


def _wall_skill(soft_walls, wall=None, set_max=None):
    from casclik_amd import skills
    from extern_skills import moe_box_skill
    spec, home = moe_box_skill(skills.ur5(), soft_walls=soft_walls)
    if wall is not None:
        _wall_constraint(spec, wall).set_max = set_max
    return spec, home


def _wall_constraint(spec, wall):
    c, = [c for c in spec.constraints if c.label == "colav_%d" % wall]
    return c


_WALL_BASE = {}


def _wall_base(soft_walls):
    """-> (Q with the base instance moved to the last row, wall, its row of A, set_max at which the wall's upper bound
    meets the minimiser of the QP without it): the first instance of the wall batch and wall that admit one"""
    from oracle import clik_oracle
    if soft_walls in _WALL_BASE:
        return _WALL_BASE[soft_walls]
    spec, home = _wall_skill(soft_walls)
    Q = _moe(soft_walls)[2]
    hd, A, lb, ub = clik_oracle.qp_data_batch(spec, 3.0, Q)
    status = clik_oracle.qp_solve_batch(spec, 3.0, Q)[3]
    for b in np.nonzero(status == 0)[0]:
        for wall in range(3):
            c = _wall_constraint(spec, wall)
            moved = clik_oracle.qp_data_batch(_wall_skill(soft_walls, wall, c.set_max + 1e-3)[0], 3.0, Q[b:b + 1])[3][0]
            row = np.nonzero(moved != ub[b])[0]
            assert row.size == 1
            row, gain = int(row[0]), (moved[row[0]] - ub[b, row[0]]) / 1e-3
            u1 = ub[b].copy()
            u1[row] = np.inf
            try:
                free = clik_oracle.qp_solve_dense(hd[b], A[b], lb[b], u1)
            except clik_oracle.QPInfeasible:
                continue
            meet = c.set_max + (A[b, row].dot(free) - ub[b, row]) / gain
            # (the wall stays a wall: an interval of at least 5 cm, moved by less than its half-width; and it is the
            # upper bound that the row meets while it moves towards it)
            if not (c.set_min + 0.05 < meet < c.set_max + 0.15) or A[b, row].dot(free) <= lb[b, row] + 1e-3:
                continue
            order = np.concatenate([np.delete(np.arange(len(Q)), b), [b]])
            _WALL_BASE[soft_walls] = (Q[order], wall, row, meet, gain)
            return _WALL_BASE[soft_walls]
    raise AssertionError("no instance of the wall batch meets a wall")


def _wall_weak(soft_walls, ds):
    Q, wall, row, meet, gain = _wall_base(soft_walls)
    spec, _ = _wall_skill(soft_walls, wall, meet - ds / gain)
    return spec, 3.0, Q, None, [None] * (len(Q) - 1) + [(len(Q) - 1, None, +1, row, ds)]


WALL_WEAK = {(soft, ds): QpCase("moe-%s-walls-weak%+.0e" % ("soft" if soft else "hard", ds),
                                lambda s=soft, d=ds: _wall_weak(s, d), only=WALL_ROWS)
             for soft in (False, True) for ds in WALL_OFFSETS}


def weak_gaps(case):
    """per constructed row of a weakly-active case: (ds, the exact minimiser's signed gap of the state to its bound -
    negative: inside -, the bound's multiplier)"""
    sol = case.solved()
    out = []
    for k, row in enumerate(case.info):
        if row is None:
            continue
        _, a, sign, r, ds = row
        bound = sol.ub[k, r] if sign > 0 else sol.lb[k, r]
        out.append((ds, sign * (sol.x[k, a] - bound), sol.lam[k][r]))
    return out


# ---- the box solver's stopping rule, restated (for the test that the rule has teeth) --------------------------------
BOX_RELEASE_TOL = 1e-9      # what `qp_box_pas` kept a held state held on, relative to max(1, |g_a|), before it was held to this


def box_reduction(hd, A, lb, ub, nq):
    """the box family's problem in the velocities alone: the soft equalities  J dq - s = b  folded into
    f(z) = 1/2 z'P z - g'z,  P = Hq + J' Hs J,  g = J' Hs b,  and the rows that bound one state -> (P, g, J, b)"""
    soft = np.nonzero(np.count_nonzero(A[:, nq:], axis=1) == 1)[0]
    assert (lb[soft] == ub[soft]).all() and len(soft) == A.shape[1] - nq
    J, b = np.zeros((A.shape[1] - nq, nq)), np.zeros(A.shape[1] - nq)
    for r in soft:
        k = int(np.nonzero(A[r, nq:])[0][0])
        assert A[r, nq + k] == -1.0
        J[k], b[k] = A[r, :nq], lb[r]
    hs = hd[nq:]
    return np.diag(hd[:nq]) + (J.T * hs).dot(J), (J.T * hs).dot(b), J, b


def held_face_minimum(P, g, J, b, z_star, lo, hi, a, bound):
    """the minimiser of f on the face that holds the states `z_star` has on a bound AND the state `a` at `bound`
    -> [z, s]; the gradient there"""
    n = len(g)
    z = z_star.copy()
    held = (z_star <= lo) | (z_star >= hi)
    held[a], z[a] = True, bound
    f = ~held
    z[f] = np.linalg.solve(P[np.ix_(f, f)], g[f] - P[np.ix_(f, held)].dot(z[held]))
    return np.concatenate([z, J.dot(z) - b]), P.dot(z) - g
