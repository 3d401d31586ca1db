"""The functions, test points and tolerance of the DeviceFunction tests (test_function_codegen.py, CPU;
test_gpu_function_batch.py, GPU).

Four functions: ``tool`` (the UR5's tool frame and tool position: 'fk' expansion, a matrix output), ``manip`` (the
quantities of cell 4 of ur5_moe2016_example2.ipynb - tool position, its Jacobian and the manipulability cost - in this
project's own words: 'fk_d' expansion, three outputs, an input nothing reads), ``pend`` (the double pendulum's tip and a column that goes through atan2, sqrt, fmin, fabs, a cube,
if_else, exp and tanh) and ``wide`` (a 14-column, a 3 x 2 matrix and a 1-entry input: index mapping, even and odd
widths).

Five more hold what those four never emit.  ``ops_pow``, ``ops_libm`` and ``ops_sel`` together hold every operation
``codegen.TaskEmitter._op`` emits - tan, log, pow with exponent 2, 0.5, 5, -3, 2.5, a variable exponent and a constant
base, sign, fabs, fmax, fmin, asin, acos, atan, atan2, tanh, exp, sqrt, division, negation, norm_2, if_else on each of the
four comparisons, on logic_and / logic_or / logic_not and on a product - each as a value column and its Jacobians with
respect to both inputs (three functions: inputs together and the widest output stay below DeviceFunction's 80 entries).
``trig`` is ``[sin x, cos x]``, that is ``sincos_joint`` alone, on a pool of its own: 0, +-5e-324, +-1e-310, +-1e-300,
+-1e-8, the nearest double to k pi / 2 and both its neighbours for k = 1 ... 64 and 111 further k up to 63661, +-1e5 (the last
argument of the straight-line path), the next double, 1e5 + 1, 1e6, 1e9, 1e15, 2^53, 1e22 and 1e300, each with both signs,
the rest uniform in +-pi and in +-1e5.  ``ties`` holds pure selections AT their switches - fmin / fmax of equal inputs
and of neighbouring doubles with their derivatives, sign and the derivative of fabs at +0.0, the four comparisons on
equal inputs, if_else on 0.0 and 0.3: it bypasses the switch-margin check, every bound of it is 0, and it is compared
bit for bit, also with its outputs written out by hand (``ties_expected``).  There is no negative zero in it: device code
is built with -fno-signed-zeros.  (``edges``, not among ``NAMES``: finite inputs with infinite or exact results.)

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
digits) checks the reference side alone against the rule: |host - exact| <= 2 bound.  The cases of ``EXACT`` (``ops_*``,
``trig``) hold the DEVICE to that rule as well, |device - exact| <= 2 bound, the exact values computed once per case
(``exact_reference``).  Measured on one MI355X (profiles/function_batch.md): worst ratio 0.492 / 0.386 / 0.497 for
``ops_pow`` / ``ops_libm`` / ``ops_sel`` and 0.198 for ``trig`` (sincos_joint: 0.91 ulp for sin and 0.93 ulp for cos up to
1e5 rad, 0.43 and 0.52 ulp on the library path beyond), so no operation's local term (``LOCAL_ULP``) was raised above the
2 ulp.
"""
import functools
import math

import numpy as np

from casclik_amd import expand, skills
from casclik_amd import sym as cs

U = 2.0 ** -53
TINY = 2.0 ** -1022
OPS = ["ops_pow", "ops_libm", "ops_sel"]
NAMES = ["tool", "manip", "pend", "wide"] + OPS + ["trig", "ties"]
EXACT = OPS + ["trig"]                  # held to |device - exact| <= 2 bound as well
R_MAX, B_MAX = 3, 257
SHAPES = [(R, B) for R in (1, 3) for B in (1, 63, 64, 65, 257)]
# the one case whose pool is not [R_MAX, B_MAX]: the listed points of `trig` alone are more than 3 x 257
_LEAD = {"trig": (3, 449)}
SWITCH_MARGIN = 1e-6
_LIBM = ("sin", "cos", "exp", "log", "tan", "atan", "atan2", "asin", "acos", "tanh")
# the local term of a library function and of pow with a non-integer exponent, in ulp (module text)
LOCAL_ULP = dict.fromkeys(_LIBM + ("pow",), 2.0)


def lead(name):
    """(R, B) of a case's pool"""
    return _LEAD.get(name, (R_MAX, B_MAX))


def shapes(name):
    """the (R, B) corners of its pool a case is run at: SHAPES, ending at the pool's own B"""
    return [(R, B) for R in (1, 3) for B in sorted({1, 63, 64, 65, lead(name)[1]})]


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
    if name in OPS:
        # a: 4 entries of either sign, 0.15 <= |a_i| <= 2; b: 3 entries in [0.3, 1.7] (`pool`).  Arguments of log and
        # sqrt and the bases of non-integer powers are >= 0.3, asin / acos see +-0.9 at most, tan +-1.4.
        a, b = cs.MX.sym("a", 4), cs.MX.sym("b", 3)
        if name == "ops_pow":
            rows = [cs.tan(0.7 * a[0]), cs.log(b[0] + b[1] * b[1]), b[0] ** b[1], b[1] ** 2.5, b[2] ** -3,
                    (2.5 + a[1]) ** 0.5, a[0] ** 5, 2.0 ** a[2], cs.sign(a[3]) * a[0], cs.fabs(a[2] * a[3]),
                    cs.fmax(a[0], a[1] * b[0]), cs.fmin(a[2], a[3]), (b[0] + a[3] * a[3]) ** 2,
                    (b[1] + 0.5) ** (a[1] * b[2])]
        elif name == "ops_libm":
            rows = [cs.asin(0.45 * a[0]), cs.acos(0.45 * a[1]), cs.atan(a[2] * b[2]), cs.atan2(a[3], a[0]),
                    cs.tanh(a[1] - b[1]), cs.exp(-a[2] * a[2]), cs.sqrt(b[0] + a[3] * a[3]), a[0] / (b[1] + a[1] * a[1]),
                    -a[3] * cs.cos(a[0]), cs.sin(a[1] * b[1]) * b[2], cs.norm_2(cs.vertcat(a[0], a[1], b[2])),
                    cs.log(b[2]) * cs.tan(0.3 * a[1])]
        else:
            rows = [cs.if_else(a[0] <= a[1], a[2] * b[0], cs.sin(a[3])),
                    cs.if_else(cs.logic_and(a[0] < a[2], a[1] != a[3]), cs.log(b[2]), cs.tan(0.3 * a[1])),
                    cs.if_else(a[2] == a[3], 1.0, b[0] * a[2]),
                    cs.if_else(cs.logic_or(a[0] > 0.0, cs.logic_not(a[1] >= 0.0)), a[0] * a[1], b[1]),
                    cs.if_else(a[0] < a[2], cs.exp(a[1]), b[1] * b[2]),
                    cs.if_else(a[1] != a[3], a[0] * b[2], cs.cos(a[2])),
                    cs.if_else(a[1] * b[0], a[2] / b[1], a[3]),             # (a condition that is no comparison)
                    cs.if_else(cs.logic_not(a[2] < a[3]), cs.fmin(a[0], b[0]), cs.fmax(a[1] * a[1], b[1]))]
        col = cs.vertcat(*rows)
        return cs.Function(name, [a, b], [col, cs.jacobian(col, a), cs.jacobian(col, b)])
    if name == "trig":
        x = cs.MX.sym("x")
        return cs.Function("trig", [x], [cs.vertcat(cs.sin(x), cs.cos(x))])
    if name == "ties":
        x, z, w, c = cs.MX.sym("x", 2), cs.MX.sym("z"), cs.MX.sym("w", 2), cs.MX.sym("c", 2)
        col = cs.vertcat(cs.fmin(x[0], x[1]), cs.fmax(x[0], x[1]), cs.sign(z), cs.if_else(x[0] <= x[1], w[0], w[1]),
                         cs.if_else(x[0] == x[1], w[0], w[1]), cs.if_else(x[0] != x[1], w[0], w[1]),
                         cs.if_else(x[0] < x[1], w[0], w[1]), cs.if_else(c[0], w[0], w[1]), cs.if_else(c[1], w[0], w[1]))
        return cs.Function("ties", [x, z, w, c], [col, cs.jacobian(col[:2], x), cs.jacobian(cs.fabs(z), z)])
    if name == "edges":
        # (not among NAMES: finite inputs whose results are infinite or exact - no bound applies, compared by bits)
        x = cs.MX.sym("x", 5)
        return cs.Function("edges", [x], [cs.vertcat(cs.log(x[0]), cs.exp(x[1]), 1.0 / x[2], cs.tanh(x[3]), x[4] ** -1)])
    raise KeyError(name)


EDGE_POINTS = np.array([[0.0, 800.0, 0.0, 1e3, 0.0], [1.0, 0.0, 2.0, 0.0, 4.0], [0.0, -800.0, 0.0, -1e3, 0.0]])
EDGE_VALUES = np.array([[-np.inf, np.inf, np.inf, 1.0, np.inf], [0.0, 1.0, 0.5, 0.0, 0.25],
                        [-np.inf, 0.0, np.inf, -1.0, np.inf]])


def ties_expected(args):
    """the outputs of ``ties`` at one point, written out by hand: CasADi's rules (fmin / fmax give the FIRST argument's
    derivative where it is the one taken, ties included; sign(0) = 0 and so is the derivative of fabs there; a
    condition counts as true when it is not 0)"""
    x, z, w, c = (np.asarray(v, dtype=float).reshape(-1) for v in args)
    assert z[0] == 0.0

    def pick(cond):
        return w[0] if cond else w[1]
    le, ge = x[0] <= x[1], x[0] >= x[1]
    col = [x[0] if le else x[1], x[0] if ge else x[1], 0.0, pick(le), pick(x[0] == x[1]), pick(x[0] != x[1]),
           pick(x[0] < x[1]), pick(c[0] != 0.0), pick(c[1] != 0.0)]
    return [np.array(col).reshape(-1, 1), np.array([[float(le), float(not le)], [float(ge), float(not ge)]]),
            np.zeros((1, 1))]


def _trig_points():
    """the listed arguments of ``trig`` (module text)"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 60
    inf = float("inf")
    pts = [5e-324, 1e-310, 1e-300, 1e-8]
    ks = sorted(set(range(1, 65)) | {int(round(k)) for k in np.geomspace(65.0, 63661.0, 110)} | {63660, 63661})
    for k in ks:
        m = float(mp.mpf(k) * mp.pi / 2)                      # (the nearest double to k pi / 2)
        pts += [m, float(np.nextafter(m, inf)), float(np.nextafter(m, -inf))]
    pts += [1e5, float(np.nextafter(1e5, inf)), 1e5 + 1.0, 1e6, 1e9, 1e15, 2.0 ** 53, 1e22, 1e300]
    return np.array([0.0] + pts + [-p for p in pts])


@functools.lru_cache(maxsize=None)
def get(name):
    return make(name)


@functools.lru_cache(maxsize=None)
def pool(name):
    """the test points of a case: one array per input, ``[*lead(name), *value dims]`` (a 1-entry input:
    ``[*lead(name)]``), fixed seed"""
    rng = np.random.default_rng({"tool": 11, "manip": 12, "pend": 13, "wide": 14, "ops_pow": 15, "ops_libm": 16,
                                 "ops_sel": 17, "trig": 18, "ties": 19}[name])
    shape = lead(name)
    if name in OPS:
        return (rng.uniform(0.15, 2.0, shape + (4,)) * rng.choice([-1.0, 1.0], shape + (4,)),
                rng.uniform(0.3, 1.7, shape + (3,)))
    if name == "trig":
        # the listed points, the rest half uniform in +-pi and half in +-1e5, in an order that gives every corner of
        # the pool some of each
        pts = _trig_points()
        rest = shape[0] * shape[1] - len(pts)
        assert rest >= 200, rest
        x = np.concatenate([pts, rng.uniform(-math.pi, math.pi, rest // 2), rng.uniform(-1e5, 1e5, rest - rest // 2)])
        return (rng.permutation(x).reshape(shape),)
    if name == "ties":
        # x_1 is x_0 (instance 0, 3, ...), the next double above it (1, 4, ...) or below it (2, 5, ...)
        x0 = rng.uniform(-2.0, 2.0, shape)
        step = np.array([0.0, np.inf, -np.inf])[np.arange(shape[1]) % 3]
        x1 = np.where(step == 0.0, x0, np.nextafter(x0, step))
        return (np.stack([x0, x1], axis=-1), np.zeros(shape), rng.uniform(-2.0, 2.0, shape + (2,)),
                np.broadcast_to(np.array([0.0, 0.3]), shape + (2,)).copy())
    if name == "tool":
        return (rng.uniform(-2.8, 2.8, shape + (6,)),)
    if name == "manip":
        return (rng.uniform(0.0, 80.0, shape), rng.uniform(-2.8, 2.8, shape + (6,)))
    if name == "pend":
        return (rng.uniform(-3.0, 3.0, shape + (2,)), rng.uniform(-1.5, 1.5, shape + (2,)))
    return (rng.uniform(-2.0, 2.0, shape + (14,)), rng.uniform(-1.0, 1.0, shape + (3, 2)), rng.uniform(0.5, 2.0, shape))


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
            local = 2.0 * LOCAL_ULP[op] * U * max(abs(v), TINY)
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
            rounds = 2.0 * LOCAL_ULP["pow"]
            if expo.is_const() and float(expo.value).is_integer():
                rounds = max(4.0, abs(expo.value))
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


def _is_truth_value(n):
    """a node that is 0 or 1 (or a count of such) EXACTLY on both sides: a comparison, the constants 0 and 1, sums and
    products of these - what logic_and / logic_or / logic_not build and compare with 0.0"""
    return (n.op.startswith("cmp_") or (n.op == "const" and n.value in (0.0, 1.0))
            or (n.op in ("add", "mul") and all(_is_truth_value(x) for x in n.args)))


def assert_no_switch_nearby(fn, args, margin=SWITCH_MARGIN):
    """no comparison, if_else, fmin, fmax, fabs or sign of the expanded DAG is within ``margin`` of switching; a
    comparison among truth values cannot switch by rounding and is left alone"""
    val = _node_values(fn, args)
    for n in _order(fn):
        a = [val[id(x)] for x in n.args]
        if n.op.startswith("cmp_") or n.op in ("fmin", "fmax"):
            if n.op.startswith("cmp_") and all(_is_truth_value(x) for x in n.args):
                continue
            assert abs(a[0] - a[1]) > margin, (n.op, a)
        elif n.op in ("fabs", "sign"):
            assert abs(a[0]) > margin, (n.op, a)
        elif n.op == "if_else" and not _is_truth_value(n.args[0]):
            assert abs(a[0]) > margin, (n.op, a)


def exact_eval(fn, args, digits=40, shift=None):
    """the expanded DAG at one point in ``digits``-digit arithmetic (mpmath): a list of ``[size1, size2]`` object
    arrays of mpf.  The inputs and the constants are the float64 numbers, exactly; ``shift`` = (input, entry, h) moves
    one entry of one input (numbered as ``MX.sym`` numbers them) by the mpf ``h``."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = digits
    f1 = {"sin": mp.sin, "cos": mp.cos, "tan": mp.tan, "exp": mp.exp, "log": mp.log, "atan": mp.atan, "asin": mp.asin,
          "acos": mp.acos, "tanh": mp.tanh, "sqrt": mp.sqrt, "fabs": abs, "neg": lambda x: -x,
          "sign": lambda x: mp.mpf((x > 0) - (x < 0))}
    env = env_of(fn, args, conv=mp.mpf)
    if shift is not None:
        fam = cs._as_array(fn._inputs[shift[0]]).T.reshape(-1)[shift[1]]
        env[id(fam.family)][fam.index] += shift[2]
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


def central_difference(fn, args, k, j, digits=80, h="1e-25"):
    """d (first output of ``fn``, a column) / d (entry ``j`` of input ``k``) at one point by central differences in
    ``digits``-digit arithmetic: a list of mpf.  Nothing of autodiff.py takes part."""
    import mpmath
    h = mpmath.mpf(h)
    up = exact_eval(fn, args, digits, (k, j, h))[0]
    down = exact_eval(fn, args, digits, (k, j, -h))[0]
    mp = mpmath.mp.clone()
    mp.dps = digits
    return [mp.fdiv(mp.fsub(up[i, 0], down[i, 0]), 2 * h) for i in range(up.shape[0])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(values, bounds) of a case over its whole pool, computed once and never changed: per output an array ``[R_MAX,
    B_MAX, size1, size2]`` of ``Function.__call__`` results and one of ``running_bound``.  Every point is checked to be
    away from a switch."""
    fn = get(name)
    vals = [np.empty(lead(name) + mx.shape) for mx in fn._outputs]
    bnds = [np.empty(lead(name) + mx.shape) for mx in fn._outputs]
    for r in range(lead(name)[0]):
        for b in range(lead(name)[1]):
            args = point(name, r, b)
            if name != "ties":          # (pure selections AT their switches: exact on both sides, compared by bits)
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


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    """``exact_eval`` of a case over its whole pool, computed once: per output two float64 arrays ``[R, B, size1,
    size2]``, the exact value rounded to a double and the rest of it rounded to a double (together 106 bits, far below
    any bound here)"""
    fn = get(name)
    his = [np.empty(lead(name) + mx.shape) for mx in fn._outputs]
    los = [np.empty(lead(name) + mx.shape) for mx in fn._outputs]
    for r in range(lead(name)[0]):
        for b in range(lead(name)[1]):
            for k, ex in enumerate(exact_eval(fn, point(name, r, b))):
                for idx in np.ndindex(ex.shape):
                    h = float(ex[idx])
                    his[k][(r, b) + idx] = h
                    los[k][(r, b) + idx] = float(ex[idx] - h)
    for a in his + los:
        a.setflags(write=False)
    return his, los


def worst_exact_ratio(got, hi, lo, bound):
    """max over entries of |got - exact| / (2 bound), exact = hi + lo (``exact_reference``): the rule of the module
    text for one side alone.  An entry whose bound is 0 must be exact."""
    got = np.asarray(got, dtype=float).reshape(np.shape(hi))
    assert np.isfinite(got).all()
    err = np.abs((hi - got) + lo)           # (hi - got is exact where got is within a factor 2 of hi)
    tol = 2.0 * bound
    ratio = np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), np.where(err == 0.0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0
