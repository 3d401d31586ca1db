"""The functions, test points and tolerance of the DeviceFunction tests (test_function_codegen.py, CPU;
test_gpu_function_batch.py, GPU).

Four functions: ``tool`` (the UR5's tool frame and tool position: 'fk' expansion, a matrix output), ``manip`` (the
quantities of cell 4 of ur5_moe2016_example2.ipynb - tool position, its Jacobian and the manipulability cost - in this
project's own words: 'fk_d' expansion, three outputs, an input nothing reads), ``pend`` (the double pendulum's tip and a column that goes through atan2, sqrt, fmin, fabs, a cube,
if_else, exp and tanh) and ``wide`` (a 14-column, a 3 x 2 matrix and a 1-entry input: index mapping, even and odd
widths).

The test points are one pool per function, ``[R_MAX, B_MAX, ...]`` from a fixed seed; every shape a test uses is the
leading ``[:R, :B]`` corner of it, so the host reference is computed once.

The tolerance is derived, not measured (``running_bound``): a forward first-order running error bound over the DAG the
device evaluates (the function's outputs with the kinematics atoms written out), from the host evaluator's node values.
With u = 2^-53, a node v = f(a, b) carries

    bound(v) = local(v) + |df/da| bound(a) + |df/db| bound(b)

where local(v) = u |v| for + - * / sqrt (correctly rounded: half a unit in the last place), 0 for negation, fabs, the
selections (fmin, fmax, if_else, sign, comparisons: ``assert_no_switch_nearby`` keeps every test point 1e-6 away from a
switch) and 4 u max(|v|, tiny) = 2 ulp for sin cos exp log tan atan atan2 asin acos tanh pow.  2 ulp is the one figure used
for all of them: the largest error the ROCm documentation of the HIP math API states for these double-precision device
functions.  That documentation is not shipped next to the compiler, so the figure is restated here, not read; the
kernels' own ``sincos_joint`` is held to the same figure by the FK parity tests.  An integer power n is n - 1 rounded
products on the device (``__builtin_powi``): local max(4, |n|) u |v|.  Fused multiply-adds only remove roundings.

An output entry passes when |dev - host| <= 2 (bound_dev + bound_host): both sides get the same bound (the host's libm
is at least as accurate as assumed, and its numpy forward kinematics multiplies the same matrices in the same order as
the written-out chain), and the factor 2 covers the truncation of the bound to first order.  ``exact_eval`` (mpmath, 40
digits) checks the reference side alone against the rule: |host - exact| <= 2 bound.
"""
import functools
import math

import numpy as np

from casclik_amd import expand, skills
from casclik_amd import sym as cs

U = 2.0 ** -53
TINY = 2.0 ** -1022
NAMES = ["tool", "manip", "pend", "wide"]
R_MAX, B_MAX = 3, 257
SHAPES = [(R, B) for R in (1, 3) for B in (1, 63, 64, 65, 257)]
SWITCH_MARGIN = 1e-6
_LIBM = ("sin", "cos", "exp", "log", "tan", "atan", "atan2", "asin", "acos", "tanh")


@functools.lru_cache(maxsize=None)
def ur5_fk():
    return skills.ur5()


def ur5_chain():
    return ur5_fk()["chain"]


def make(name):
    """a NEW ``cs.Function`` (new symbols, new nodes) of the named case"""
    if name == "tool":
        q = cs.MX.sym("q", 6)
        T = ur5_fk()["T_fk"](q)
        return cs.Function("tool", [q], [T, T[:3, 3]])
    if name == "manip":
        # the manipulability function of the Moe-2016 example: tool position, its Jacobian, and the cost
        # 1e3 |q|^2 - det(J J'), the Gram determinant expanded along its first row
        t, q = cs.MX.sym("t"), cs.MX.sym("q", 6)
        p = ur5_fk()["T_fk"](q)[:3, 3]
        J = cs.jacobian(p, q)
        G = cs.mtimes(J, J.T)
        det = (G[0, 0] * (G[1, 1] * G[2, 2] - G[1, 2] * G[2, 1]) - G[0, 1] * (G[1, 0] * G[2, 2] - G[1, 2] * G[2, 0])
               + G[0, 2] * (G[1, 0] * G[2, 1] - G[1, 1] * G[2, 0]))
        return cs.Function("manip", [t, q], [p, J, 1e3 * cs.dot(q, q) - det])
    if name == "pend":
        l_1, l_2 = 1.0, 0.75
        q, y = cs.MX.sym("q", 2), cs.MX.sym("y", 2)
        p = cs.vertcat(l_1 * cs.cos(q[0]) + l_2 * cs.cos(q[0] + q[1]), l_1 * cs.sin(q[0]) + l_2 * cs.sin(q[0] + q[1]))
        d = p - y
        col = cs.vertcat(cs.atan2(d[1], d[0]), cs.sqrt(d[0] * d[0] + d[1] * d[1]), cs.fmin(p[0], y[0]), cs.fabs(p[1]),
                         d[0] ** 3, cs.if_else(p[0] < y[1], cs.exp(d[0]), cs.tanh(d[1])), cs.exp(-cs.dot(d, d)),
                         cs.tanh(p[0] * y[1]))
        return cs.Function("pend", [q, y], [p, col])
    if name == "wide":
        a, M, s = cs.MX.sym("a", 14), cs.MX.sym("M", 3, 2), cs.MX.sym("s")
        col = cs.vertcat(*[a[i] * s + M[i % 3, (i // 3) % 2] * cs.sin(a[i]) for i in range(14)])
        acc = s * a[13]
        for i in range(3):
            for j in range(2):
                acc = acc + (1.0 + i + 3.0 * j) * M[i, j]
        return cs.Function("wide", [a, M, s], [col, acc])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def get(name):
    return make(name)


@functools.lru_cache(maxsize=None)
def pool(name):
    """the test points of a case: one array per input, ``[R_MAX, B_MAX, *value dims]`` (a 1-entry input: ``[R_MAX,
    B_MAX]``), fixed seed"""
    rng = np.random.default_rng({"tool": 11, "manip": 12, "pend": 13, "wide": 14}[name])
    lead = (R_MAX, B_MAX)
    if name == "tool":
        return (rng.uniform(-2.8, 2.8, lead + (6,)),)
    if name == "manip":
        return (rng.uniform(0.0, 80.0, lead), rng.uniform(-2.8, 2.8, lead + (6,)))
    if name == "pend":
        return (rng.uniform(-3.0, 3.0, lead + (2,)), rng.uniform(-1.5, 1.5, lead + (2,)))
    return (rng.uniform(-2.0, 2.0, lead + (14,)), rng.uniform(-1.0, 1.0, lead + (3, 2)), rng.uniform(0.5, 2.0, lead))


def point(name, r, b):
    """the arguments of ``Function.__call__`` at row (r, b) of the pool"""
    return tuple(a[r, b] for a in pool(name))


def host_call(fn, args):
    """``Function.__call__`` as a list of ``[size1, size2]`` arrays"""
    out = fn(*args)
    out = out if isinstance(out, tuple) else (out,)
    return [np.asarray(o.toarray(), dtype=float) for o in out]


_EXPANDED = {}


def expanded(fn):
    """the outputs of ``fn`` as the device evaluates them: object arrays of Scalars, kinematics atoms written out"""
    hit = _EXPANDED.get(id(fn))
    if hit is None or hit[0] is not fn:
        memo = {}
        outs = []
        for mx in fn._outputs:
            arr = cs._as_array(mx)
            out = np.empty(arr.shape, dtype=object)
            for idx in np.ndindex(arr.shape):
                out[idx] = expand.rewrite(arr[idx], lambda n: False, lambda n: False, memo, expand_fk_d=True)
            outs.append(out)
        hit = _EXPANDED[id(fn)] = (fn, outs, memo)
    return hit[1]


def env_of(fn, args, conv=float):
    env = {}
    for sym_in, val in zip(fn._inputs, args):
        flat = np.asarray(val, dtype=float).T.reshape(-1)       # (column-major: the numbering of MX.sym)
        for k, s in enumerate(cs._as_array(sym_in).T.reshape(-1)):
            env.setdefault(id(s.family), {})[s.index] = conv(flat[k])
    return env


def _walk(nodes):
    """the DAG below ``nodes`` in evaluation order (arguments first), each node once"""
    order, seen = [], set()
    stack = [(n, False) for n in reversed(nodes)]
    while stack:
        n, done = stack.pop()
        if done:
            order.append(n)
            continue
        if id(n) in seen:
            continue
        seen.add(id(n))
        stack.append((n, True))
        stack.extend((a, False) for a in reversed(n.args))
    return order


_ORDER = {}


def _order(fn):
    hit = _ORDER.get(id(fn))
    if hit is None or hit[0] is not fn:
        hit = _ORDER[id(fn)] = (fn, _walk([n for out in expanded(fn) for n in out.flat]))
    return hit[1]


def _node_values(fn, args):
    """{id(node): host float64 value} of the expanded DAG at one point: the memo of ``sym._eval_scalar``"""
    env, memo = env_of(fn, args), {}
    for out in expanded(fn):
        for n in out.flat:
            cs._eval_scalar(n, env, memo)
    return memo


def running_bound(fn, args):
    """The first-order running error bound of every output entry at one point (module text): a list of ``[size1,
    size2]`` arrays.  A device result passes at 2 (bound + bound) = 4 bound, the host's float64 result at 2 bound."""
    val = _node_values(fn, args)
    err = {}
    for n in _order(fn):
        op, v = n.op, val[id(n)]
        a = [val[id(x)] for x in n.args]
        e = [err[id(x)] for x in n.args]
        if op in ("const", "sym"):
            b = 0.0
        elif op in ("add", "sub"):
            b = U * abs(v) + e[0] + e[1]
        elif op == "mul":
            b = U * abs(v) + abs(a[1]) * e[0] + abs(a[0]) * e[1]
        elif op == "div":
            b = U * abs(v) + e[0] / abs(a[1]) + abs(a[0]) / (a[1] * a[1]) * e[1]
        elif op == "neg" or op == "fabs":
            b = e[0]
        elif op == "sqrt":
            b = U * abs(v) + e[0] / (2.0 * abs(v))
        elif op in _LIBM:
            local = 4.0 * U * max(abs(v), TINY)
            if op == "sin":
                b = local + abs(math.cos(a[0])) * e[0]
            elif op == "cos":
                b = local + abs(math.sin(a[0])) * e[0]
            elif op == "tan":
                b = local + (1.0 + v * v) * e[0]
            elif op == "exp":
                b = local + abs(v) * e[0]
            elif op == "log":
                b = local + e[0] / abs(a[0])
            elif op == "atan":
                b = local + e[0] / (1.0 + a[0] * a[0])
            elif op in ("asin", "acos"):
                b = local + e[0] / math.sqrt(1.0 - a[0] * a[0])
            elif op == "tanh":
                b = local + (1.0 - v * v) * e[0]
            else:       # atan2(y, x)
                b = local + (abs(a[1]) * e[0] + abs(a[0]) * e[1]) / (a[0] * a[0] + a[1] * a[1])
        elif op == "pow":
            expo = n.args[1]
            rounds = max(4.0, abs(expo.value)) if expo.is_const() and float(expo.value).is_integer() else 4.0
            b = rounds * U * max(abs(v), TINY) + abs(a[1] * a[0] ** (a[1] - 1.0)) * e[0]
            if not expo.is_const():
                b += abs(v * math.log(a[0])) * e[1]
        elif op == "norm2":
            b = (len(a) + 1.0) * U * abs(v) + sum(abs(x) * ex for x, ex in zip(a, e)) / abs(v)
        elif op in ("fmin", "fmax"):
            first = (a[0] <= a[1]) if op == "fmin" else (a[0] >= a[1])
            b = e[0] if first else e[1]
        elif op == "if_else":
            b = e[1] if a[0] != 0.0 else e[2]
        elif op == "sign" or op.startswith("cmp_"):
            b = 0.0
        else:
            raise NotImplementedError("running_bound: operation '%s'" % op)
        err[id(n)] = b
    return [np.array([[err[id(out[i, j])] for j in range(out.shape[1])] for i in range(out.shape[0])])
            for out in expanded(fn)]


def assert_no_switch_nearby(fn, args, margin=SWITCH_MARGIN):
    """no comparison, if_else, fmin, fmax, fabs or sign of the expanded DAG is within ``margin`` of switching"""
    val = _node_values(fn, args)
    for n in _order(fn):
        a = [val[id(x)] for x in n.args]
        if n.op.startswith("cmp_") or n.op in ("fmin", "fmax"):
            assert abs(a[0] - a[1]) > margin, (n.op, a)
        elif n.op in ("fabs", "sign"):
            assert abs(a[0]) > margin, (n.op, a)
        elif n.op == "if_else" and not n.args[0].op.startswith("cmp_"):
            assert abs(a[0]) > margin, (n.op, a)


def exact_eval(fn, args, digits=40):
    """the expanded DAG at one point in ``digits``-digit arithmetic (mpmath): a list of ``[size1, size2]`` object
    arrays of mpf.  The inputs and the constants are the float64 numbers, exactly."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = digits
    f1 = {"sin": mp.sin, "cos": mp.cos, "tan": mp.tan, "exp": mp.exp, "log": mp.log, "atan": mp.atan, "asin": mp.asin,
          "acos": mp.acos, "tanh": mp.tanh, "sqrt": mp.sqrt, "fabs": abs, "neg": lambda x: -x,
          "sign": lambda x: mp.mpf((x > 0) - (x < 0))}
    env = env_of(fn, args, conv=mp.mpf)
    val = {}
    for n in _order(fn):
        op = n.op
        a = [val[id(x)] for x in n.args]
        if op == "const":
            v = mp.mpf(n.value)
        elif op == "sym":
            v = env[id(n.family)][n.index]
        elif op in f1:
            v = f1[op](a[0])
        elif op == "add":
            v = a[0] + a[1]
        elif op == "sub":
            v = a[0] - a[1]
        elif op == "mul":
            v = a[0] * a[1]
        elif op == "div":
            v = a[0] / a[1]
        elif op == "pow":
            v = mp.power(a[0], a[1])
        elif op == "atan2":
            v = mp.atan2(a[0], a[1])
        elif op == "fmin":
            v = min(a[0], a[1])
        elif op == "fmax":
            v = max(a[0], a[1])
        elif op == "norm2":
            v = mp.sqrt(sum(x * x for x in a))
        elif op == "cmp_lt":
            v = mp.mpf(a[0] < a[1])
        elif op == "cmp_le":
            v = mp.mpf(a[0] <= a[1])
        elif op == "cmp_eq":
            v = mp.mpf(a[0] == a[1])
        elif op == "cmp_ne":
            v = mp.mpf(a[0] != a[1])
        elif op == "if_else":
            v = a[1] if a[0] != 0 else a[2]
        else:
            raise NotImplementedError("exact_eval: operation '%s'" % op)
        val[id(n)] = v
    outs = []
    for out in expanded(fn):
        o = np.empty(out.shape, dtype=object)
        for idx in np.ndindex(out.shape):
            o[idx] = val[id(out[idx])]
        outs.append(o)
    return outs


@functools.lru_cache(maxsize=None)
def reference(name):
    """(values, bounds) of a case over its whole pool, computed once and never changed: per output an array ``[R_MAX,
    B_MAX, size1, size2]`` of ``Function.__call__`` results and one of ``running_bound``.  Every point is checked to be
    away from a switch."""
    fn = get(name)
    vals = [np.empty((R_MAX, B_MAX) + mx.shape) for mx in fn._outputs]
    bnds = [np.empty((R_MAX, B_MAX) + mx.shape) for mx in fn._outputs]
    for r in range(R_MAX):
        for b in range(B_MAX):
            args = point(name, r, b)
            assert_no_switch_nearby(fn, args)
            for k, (v, e) in enumerate(zip(host_call(fn, args), running_bound(fn, args))):
                vals[k][r, b] = v
                bnds[k][r, b] = e
    for a in vals + bnds:
        a.setflags(write=False)
    return vals, bnds


def worst_ratio(got, want, bound):
    """max over entries of |got - want| / (2 (bound + bound)); every entry must be finite on both sides.  ``got`` may
    have the call's output shape (``[..., size1]`` for a column, ``[...]`` for a scalar)."""
    got = np.asarray(got, dtype=float).reshape(np.shape(want))
    assert np.isfinite(got).all() and np.isfinite(want).all()
    tol = 2.0 * (bound + bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0.0, np.abs(got - want) / np.where(tol > 0.0, tol, 1.0),
                         np.where(got == want, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0
