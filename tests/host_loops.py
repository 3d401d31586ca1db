"""The host yardsticks of the on-device loops, written once and needing no GPU: the fixed-length loop ``rollout_batch``
is held to (``rollout_loop``), the run-until-converged loop ``converge_batch`` / ``ik_batch`` are held to
(``converge_loop``), the ticks they run on (a controller's ``solve_batch``, the oracle), and the stop rule of
include/clik.h in plain numpy.  tests/test_host_loops.py pins both loops on the CPU."""
import numpy as np

from casclik_amd.controllers.base_controller import constraint_row_slices
from casclik_amd.lowering import lower_skill
from oracle import clik_oracle

MARGIN = 4e-12          # (tests/test_gpu_constraint_summary.py: an integer result decided by less is left out)
DT = 0.05               # with gain 10 the error halves per tick
CANCELLED = 5           # status of an instance stopped by the group rule


# ---- the ticks ----------------------------------------------------------------------------------------------------------
def controller_tick(ctrl, qp):
    """``tick`` of ``rollout_loop`` on a controller's ``solve_batch``"""
    def tick(t, q, x, y):
        res = ctrl.solve_batch(t, q, virtual_var=x, input_var=y)
        return (res[0], res[1], res[2], res[3]) if qp else (res[0], res[1], None, res[2])
    return tick


def oracle_tick(spec, qp, options=None, **solve_kwargs):
    """``tick`` of ``rollout_loop`` on the oracle; ``solve_kwargs`` go to its solve (the QP's ``weights``, ``pinv_fn``)"""
    def tick(t, q, x, y):
        nq = q.shape[1]
        if qp:
            dq, dx, slack, status = clik_oracle.qp_solve_batch(spec, t, q, X=x, Y=y, **solve_kwargs)
            return dq[:, :nq], dx, slack, status
        dz, mode = clik_oracle.pinv_solve_batch(spec, options, t, q, X=x, Y=y, **solve_kwargs)
        return dz[:, :nq], None if x is None else dz[:, nq:], None, mode
    return tick


def feed(Y, fb, v):
    """Y with the fed entries rewritten from the velocities v [B, n_q + n_x] (``options["velocity_feedback"]``: entry j
    of the map names where velocity j is read, -1 for a velocity that is fed nowhere)"""
    Y = Y.copy()
    for j, k in enumerate(fb):
        if k >= 0:
            Y[:, k] = v[:, j]
    return Y


# ---- the fixed-length loop ----------------------------------------------------------------------------------------------
def rollout_loop(tick, qp, times, Q, X, y_of, dt, vmax=0.0, rk4=False, fb=None):
    """The yardstick of ``rollout_batch``: one call of ``tick(t, q, x, y) -> (dq, dx | None, slack | None, flag)`` per tick
    (``rk4``: per stage), ``y_of(i)`` the target the caller gives tick i.  Returns one dict per tick: the state after it
    (``q``, ``x``), the velocity it was integrated with (``dq``, ``dx``), ``slack`` and ``flag``.  The rules are the API's:

    - Clamp: the robot velocities only, and only for ``vmax > 0`` (0 is "no clamp"); with ``rk4`` every stage is clamped.
      The virtual variables are never clamped.
    - Runge-Kutta: the classical scheme of casclik_amd/integration_methods.py:17-23, all four stages with the tick's
      target ``y_of(i)``; ``dq`` / ``dx`` are the combined rate, ``slack`` is the last stage's.
    - Flag: the pseudo-inverse's is the mode of the tick's first stage; the QP's (``qp``) is the status, the maximum over
      the stages and then the worst so far across the ticks.
    - Feed: with the map ``fb``, ``feed(y, fb, v_last)`` rewrites the fed entries of the target from the velocity the
      tick before was integrated with; tick 0 reads what the caller gave.
    - Integration: ``q + dq * dt``, and ``x + dx * dt`` when there are virtual variables."""
    q, x = Q.copy(), None if X is None else X.copy()
    nq = q.shape[1]
    clamp = (lambda d: np.clip(d, -vmax, vmax)) if vmax > 0.0 else (lambda d: d)
    out, v_last = [], None
    for i, tv in enumerate(times):
        y = y_of(i) if fb is None or v_last is None else feed(y_of(i), fb, v_last)
        if not rk4:
            dq, dx, sl, flag = tick(float(tv), q, x, y)
            dq = clamp(dq)
        else:
            z = q if x is None else np.hstack([q, x])
            flags, sls = [], []

            def f(tt, zz):
                d, ddx, s_, fl = tick(float(tt), zz[:, :nq], None if x is None else zz[:, nq:], y)
                flags.append(fl)
                sls.append(s_)
                d = clamp(d)
                return d if ddx is None else np.hstack([d, ddx])
            k1 = f(tv, z)
            k2 = f(tv + dt / 2, z + dt / 2 * k1)
            k3 = f(tv + dt / 2, z + dt / 2 * k2)
            k4 = f(tv + dt, z + dt * k3)
            v = (k1 + 2 * k2 + 2 * k3 + k4) / 6.0
            dq, dx = v[:, :nq], None if x is None else v[:, nq:]
            sl = sls[-1]
            flag = np.maximum.reduce(flags) if qp else flags[0]
        q = q + dq * dt
        if x is not None:
            x = x + dx * dt
        if qp and out:
            flag = np.maximum(flag, out[-1]["flag"])
        v_last = dq if dx is None else np.hstack([dq, dx])
        out.append({"q": q.copy(), "x": None if x is None else x.copy(), "dq": dq, "dx": dx, "slack": sl, "flag": flag})
    return out


# ---- the stop rule ------------------------------------------------------------------------------------------------------
def oracle_values(spec, t, Q, X=None, Y=None):
    """(e, set_min, set_max) [R, B, M_tot] and is_set [M_tot] of the records Q [R, B, n_q], all at time t, the target
    shared by the records: the oracle's own evaluation of every constraint expression (as ``_oracle`` of
    tests/test_gpu_constraint_summary.py)"""
    R, B = Q.shape[:2]
    flat = lambda A: None if A is None else A.reshape(R * B, -1)         # noqa: E731
    Z = flat(Q) if X is None else np.hstack([flat(Q), flat(X)])
    Yf = flat(None if Y is None else np.broadcast_to(Y, (R,) + Y.shape))
    ev = clik_oracle.ExprEvaluator(spec, np.full(R * B, float(t)), Z, Yf)
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


def distances(e, lo, hi, is_set):
    with np.errstate(invalid="ignore"):
        return np.where(is_set, np.maximum(np.maximum(lo - e, e - hi), 0.0), np.abs(e))


def stop_rule(e, lo, hi, is_set, tol, max_ticks):
    """Steps 1 - 4 of the stop rule on the records r = 0 .. max_ticks of a rollout that never stops (e [max_ticks + 1, B,
    M_tot]): ``(ticks [B], status [B], residual [B, M_tot], sure [B])``; ``sure``: no row of the instance comes within
    MARGIN of its tolerance at any record up to its stop."""
    R, B, M = e.shape
    assert R == max_ticks + 1
    d = distances(e, lo, hi, is_set)
    with np.errstate(invalid="ignore"):
        met = (d <= tol).all(axis=2)
        close = (np.abs(d - tol) < MARGIN).any(axis=2)
    bad = ~np.isfinite(e).all(axis=2)
    ticks, status = np.full(B, max_ticks, dtype=np.int32), np.ones(B, dtype=np.int32)
    for b in range(B):
        for r in range(R):
            if bad[r, b] or met[r, b]:
                ticks[b], status[b] = r, 4 if bad[r, b] else 0
                break
    sure = np.array([not close[:ticks[b] + 1, b].any() for b in range(B)])
    return ticks, status, d[ticks, np.arange(B)], sure


# ---- the run-until-converged loop ---------------------------------------------------------------------------------------
def converge_loop(spec, options, Q, Y, tol, max_ticks, dt=DT, max_speed=0.0, min_step=0.0, t=0.0, margin=MARGIN, group=1,
                  fb=None, pinv_fn=None):
    """The yardstick of ``converge_batch``: the whole rule, every instance on its own, no device code - the oracle's
    constraint values and ``clik_oracle.pinv_solve_batch`` (``pinv_fn``: its pseudo-inverse, None for its literal
    ``dpinv``) per tick.  Returns ``(q, dq, ticks, status, residual, sure)``; ``sure``: no row of the instance came within
    ``margin`` of its tolerance.  A tick, on the instances still running:

    1. the stop test on the oracle's constraint values: status 4 (a value that is not finite), then 0 (every row within
       its tolerance), then 1 at ``max_ticks``;
    2. the group rule, for ``group > 1``: whoever is still running next to an instance of its group that has arrived
       stops with status 5;
    3. the oracle's solve;
    4. the clamp, for ``max_speed > 0``;
    5. the stall test, for ``min_step > 0``: status 2 where the largest step would be ``min_step`` or less;
    6. the Euler step ``q + v * dt``;
    7. with the map ``fb``, the feed of v into those instances' rows of a copy of ``Y``.

    A stopped instance keeps its state and its fed entries."""
    B, nq = Q.shape
    assert B % group == 0
    q, dq, Y = Q.copy(), np.zeros_like(Q), None if Y is None else Y.copy()
    ticks, status = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    residual, sure = np.zeros((B, tol.size)), np.ones(B, dtype=bool)
    for r in range(max_ticks + 1):
        go = np.nonzero(status < 0)[0]
        if go.size == 0:
            break
        e, lo, hi, is_set = oracle_values(spec, t, q[None, go], None, None if Y is None else Y[go])
        d = distances(e, lo, hi, is_set)[0]
        residual[go] = d
        sure[go] &= ~(np.abs(d - tol) < margin).any(axis=1)
        bad = ~np.isfinite(e[0]).all(axis=1)
        with np.errstate(invalid="ignore"):
            met = (d <= tol).all(axis=1)
        status[go] = np.where(bad, 4, np.where(met, 0, 1 if r == max_ticks else -1))
        ticks[go] = r
        if group > 1:
            won = np.repeat((status == 0).reshape(-1, group).any(axis=1), group)
            status[(status < 0) & won] = CANCELLED
        go = np.nonzero(status < 0)[0]
        if go.size == 0:
            continue
        v = clik_oracle.pinv_solve_batch(spec, options, t, q[go], Y=None if Y is None else Y[go], pinv_fn=pinv_fn)[0][:, :nq]
        if max_speed > 0.0:
            v = np.clip(v, -max_speed, max_speed)
        stall = (min_step > 0.0) & (np.abs(v).max(axis=1) * dt <= min_step)
        status[go[stall]] = 2
        go, v = go[~stall], v[~stall]
        q[go] += v * dt
        dq[go] = v
        if fb is not None:
            Y[go] = feed(Y[go], fb, v)
    return q, dq, ticks, status, residual, sure
