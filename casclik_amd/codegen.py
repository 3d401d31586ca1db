"""Device code for constraint expressions outside the affine-in-features family.

The reference differentiates every constraint expression with CasADi
(``cs.jacobian``, casclik/constraints.py:67-73) and JIT-compiles the resulting
function per controller (casclik/controllers/pseudo_inverse.py:476-483,
reactive_qp.py:262-298).  Most skills lower to the device task table
(lowering.py) and run hand-written row code; a constraint that does not - products
or trigonometric functions of the state (``l*cos(q[0]+q[1])`` of
double_pendulum_2D_comparison_of_controllers.ipynb cell 4), functions of the tool
frame other than its entries and norms - is kept as an expression graph.  This
module turns such a constraint into one straight-line ``__device__`` function

    ExternTask<TI>::eval(z, ys, tv, K, e, J, Jt)

(value, state Jacobian and partial time derivative; clik_pinv_static.hpp) from the
scalar DAG and its symbolic derivatives (autodiff.py), with common sub-expressions
shared.  Time-only sub-expressions stay on the host as time slots (``tv``), like in
the row table.  The kernel templates around it are the hand-written ones; jit.py
compiles both for the skill.

The time slots themselves have device code too, on request (``emit_time_slots``; the
controllers' option ``time_on_device``): one straight-line function that fills ``tv``
from a time, for the kernel of clik_time.hpp.
"""
from __future__ import annotations

import math

from . import autodiff

_UNARY_C = {"tan": "tan", "sqrt": "sqrt", "exp": "exp", "log": "log",
            "fabs": "fabs", "asin": "asin", "acos": "acos", "atan": "atan", "tanh": "tanh"}
_BINARY_C = {"atan2": "atan2", "fmin": "fmin", "fmax": "fmax"}
_INFIX = {"add": "+", "sub": "-", "mul": "*", "div": "/"}


def _lit(v):
    v = float(v)
    if math.isinf(v):
        return "(-__builtin_inf())" if v < 0 else "__builtin_inf()"
    if math.isnan(v):
        return "__builtin_nan(\"\")"
    r = repr(v)
    return "(%s)" % r if v < 0 else r


class TaskEmitter(object):
    """Emits the body of one ExternTask<TI>::eval.  ``low`` is the skill's
    lowering._Lowerer (symbol families, chain bookkeeping, time slots)."""

    def __init__(self, low):
        self.low = low
        self.lines = []
        self._by_id = {}
        self._by_key = {}
        self._tslot_by_repr = {}
        self.uses_fk = False
        self._keep = []          # derivative trees must outlive the id()-keyed memo

    # -- leaves -------------------------------------------------------------
    def _sym(self, node):
        low = self.low
        fam = node.family
        if fam is low.fam_q:
            return "z[%d]" % node.index
        if fam is low.fam_x and fam is not None:
            return "z[%d]" % (low.desc.n_q + node.index)
        if fam is low.fam_y and fam is not None:
            return "ys[%d]" % node.index
        if fam is low.fam_dq or fam is low.fam_dx:
            raise NotImplementedError("constraint expressions must not contain velocity variables")
        raise NotImplementedError("symbol '%s' is not a variable of the skill specification" % node.name)

    def _time_slot(self, node):
        key = repr(node)
        if key not in self._tslot_by_repr:
            self._tslot_by_repr[key] = self.low._tslot(node)
        return "tv[%d]" % self._tslot_by_repr[key]

    def _temp(self, key, expr):
        if key in self._by_key:
            return self._by_key[key]
        name = "v%d" % len(self.lines)
        self.lines.append("const double %s = %s;" % (name, expr))
        self._by_key[key] = name
        return name

    # -- nodes --------------------------------------------------------------
    def ref(self, node):
        nid = id(node)
        if nid not in self._by_id:
            self._by_id[nid] = self._ref(node)
        return self._by_id[nid]

    def _ref(self, node):
        op = node.op
        low = self.low
        if op == "const":
            return _lit(node.value)
        if low._time_only(node):
            return self._time_slot(node)
        if op == "sym":
            return self._sym(node)
        if op == "fk":
            low._use_chain(node)
            self.uses_fk = True
            _, i, j = node.aux
            return "K.p[%d]" % i if j == 3 else "K.R[%d]" % (3 * i + j)
        if op == "fk_d":
            low._use_chain(node)
            self.uses_fk = True
            _, i, j, k = node.aux
            s = low._chain_state_index[k]
            if j == 3:
                return "K.Jv[%d][%d]" % (i, s)
            a, b = (i + 1) % 3, (i + 2) % 3
            # d R[:, j] / d z_s = w_s x R[:, j]
            expr = "K.Jw[%d][%d] * K.R[%d] - K.Jw[%d][%d] * K.R[%d]" % (a, s, 3 * b + j, b, s, 3 * a + j)
            return self._temp(("fk_d", i, j, s), expr)
        if op == "ori_err":
            raise NotImplementedError("orientation_error inside a non-affine constraint expression")
        return self._op(node)

    def _op(self, node):
        """an operation node (no leaf, no kinematics atom): one memoised temporary over its arguments' references"""
        op = node.op
        args = [self.ref(a) for a in node.args]
        if op in ("sin", "cos"):
            # one evaluation serves both (a Jacobian needs the other one anyway); sincos_joint is the
            # kernels' own routine (straight-line up to 1e5 rad, library fallback beyond)
            key = ("sincos", args[0])
            if key not in self._by_key:
                k = len(self.lines)
                self.lines.append("double s%d, c%d; sincos_joint(%s, s%d, c%d);" % (k, k, args[0], k, k))
                self._by_key[key] = ("s%d" % k, "c%d" % k)
            return self._by_key[key][0 if op == "sin" else 1]
        if op in _INFIX:
            expr = "%s %s %s" % (args[0], _INFIX[op], args[1])
        elif op == "neg":
            expr = "-%s" % args[0]
        elif op in _UNARY_C:
            expr = "%s(%s)" % (_UNARY_C[op], args[0])
        elif op in _BINARY_C:
            expr = "%s(%s, %s)" % (_BINARY_C[op], args[0], args[1])
        elif op == "sign":
            expr = "(double)((%s > 0.0) - (%s < 0.0))" % (args[0], args[0])
        elif op == "pow":
            b = node.args[1]
            if b.is_const() and b.value == 2.0:
                expr = "%s * %s" % (args[0], args[0])
            elif b.is_const() and b.value == 1.0:
                return args[0]
            elif b.is_const() and b.value == 0.5:
                expr = "sqrt(%s)" % args[0]
            elif b.is_const() and float(b.value).is_integer() and abs(b.value) <= 64:
                expr = "__builtin_powi(%s, %d)" % (args[0], int(b.value))
            else:
                expr = "pow(%s, %s)" % (args[0], args[1])
        elif op == "norm2":
            expr = "sqrt(%s)" % " + ".join("%s * %s" % (a, a) for a in args)
        elif op == "cmp_lt":
            expr = "(%s < %s ? 1.0 : 0.0)" % (args[0], args[1])
        elif op == "cmp_le":
            expr = "(%s <= %s ? 1.0 : 0.0)" % (args[0], args[1])
        elif op == "cmp_eq":
            expr = "(%s == %s ? 1.0 : 0.0)" % (args[0], args[1])
        elif op == "cmp_ne":
            expr = "(%s != %s ? 1.0 : 0.0)" % (args[0], args[1])
        elif op == "if_else":
            expr = "(%s != 0.0 ? %s : %s)" % (args[0], args[1], args[2])
        else:
            raise NotImplementedError("no device code for operation '%s'" % op)
        return self._temp((op,) + tuple(args), expr)

    # -- attributes given as expressions ---------------------------------------
    def emit_attr(self, ti, nodes):
        """C++ source of ``template <> struct ExternAttr<ti>``: ``nodes`` are the Scalar nodes of the task's
        attribute slice in its layout order (clik_pinv_static.hpp: [gain | set_min | set_max | target], present
        parts only).  Values only - the reference never differentiates a gain or a bound
        (casclik/constraints.py:67-73 takes the Jacobian of ``expression``)."""
        n = self.low.desc.n_state
        out = ["a[%d] = %s;" % (k, self.ref(node)) for k, node in enumerate(nodes)]
        body = "\n        ".join(self.lines + out)
        return ("template <>\n"
                "struct ExternAttr<%d> {\n"
                "    template <int N>\n"
                "    __device__ __forceinline__ static void eval(const double (&z)[N], const double* ys, const double* tv,\n"
                "                                                const Kin<N>& K, double* a)\n"
                "    {\n"
                "        static_assert(N == %d, \"generated for another skill structure\");\n"
                "        (void)z; (void)ys; (void)tv; (void)K;\n"
                "        %s\n"
                "    }\n"
                "};\n" % (ti, n, body))

    # -- one constraint -------------------------------------------------------
    def emit_task(self, ti, nodes):
        """C++ source of ``template <> struct ExternTask<ti>`` for the column
        of Scalar nodes ``nodes``."""
        low = self.low
        n = low.desc.n_state
        keys = []
        for j in range(n):
            if j < low.desc.n_q:
                keys.append((id(low.fam_q), j))
            else:
                keys.append((id(low.fam_x), j - low.desc.n_q))
        tkey = (id(low.fam_t), 0) if low.fam_t is not None else None
        out = []
        memos = [dict() for _ in range(n + 1)]
        for i, node in enumerate(nodes):
            out.append("e[%d] = %s;" % (i, self.ref(node)))
            for j in range(n):
                d = autodiff.diff_scalar(node, keys[j], memos[j])
                self._keep.append(d)
                out.append("J[%d][%d] = %s;" % (i, j, self.ref(d)))
            if tkey is None:
                out.append("Jt[%d] = 0.0;" % i)
            else:
                d = autodiff.diff_scalar(node, tkey, memos[n])
                self._keep.append(d)
                out.append("Jt[%d] = %s;" % (i, self.ref(d)))
        body = "\n        ".join(self.lines + out)
        return ("template <>\n"
                "struct ExternTask<%d> {\n"
                "    template <int N, int M>\n"
                "    __device__ __forceinline__ static void eval(const double (&z)[N], const double* ys, const double* tv,\n"
                "                                                const Kin<N>& K, double (&e)[M], double (&J)[M][N],\n"
                "                                                double (&Jt)[M])\n"
                "    {\n"
                "        static_assert(N == %d && M == %d, \"generated for another skill structure\");\n"
                "        (void)ys; (void)tv; (void)K;\n"
                "        %s\n"
                "    }\n"
                "};\n" % (ti, n, len(nodes), body))


class _TimeEmitter(TaskEmitter):
    """Node emission of TaskEmitter for trees over time alone: the time symbol is the one leaf beside constants."""

    def __init__(self, time_family):
        TaskEmitter.__init__(self, None)
        self.time_family = time_family

    def _ref(self, node):
        op = node.op
        if op == "const":
            return _lit(node.value)
        if op == "sym":
            if node.family is not None and node.family is self.time_family:
                return "t"
            raise NotImplementedError("symbol '%s' in a time slot is not the time variable" % node.name)
        if op in ("fk", "fk_d", "ori_err"):
            raise NotImplementedError("no device code for operation '%s' in a time slot" % op)
        return self._op(node)


def emit_time_slots(low_or_desc):
    """C++ source of ``struct TimeSlots`` for a lowered skill (its lowering._Lowerer or its SkillDescriptor): one
    straight-line function

        TimeSlots::eval(double t, double* tv)

    that writes ``tv[k]``, the value of time slot k, and ``tv[n_tslots + k]``, its time derivative - the layout of
    ``SkillDescriptor.time_terms`` and of the kernels' TickArgs - with common sub-expressions shared across slots and
    across values and derivatives.  ``sin`` / ``cos`` go through ``sincos_joint``, which the includer supplies
    (clik_device.hpp on the device; the text is host C++ as well once ``__device__``, ``__forceinline__`` and
    ``sincos_joint`` are defined).  A skill without time slots gives an empty body."""
    desc = getattr(low_or_desc, "desc", low_or_desc)
    n = desc.n_tslots
    em = _TimeEmitter(desc.time_family)
    out = []
    for k, (val, der) in enumerate(desc.tslots):
        out.append("tv[%d] = %s;" % (k, em.ref(val)))
        out.append("tv[%d] = %s;" % (n + k, em.ref(der)))
    body = "\n        ".join(em.lines + out)
    return ("struct TimeSlots {\n"
            "    static constexpr int n_tslots = %d;\n"
            "    __device__ __forceinline__ static void eval(double t, double* tv)\n"
            "    {\n"
            "        (void)t; (void)tv;\n"
            "        %s\n"
            "    }\n"
            "};\n" % (n, body))


class _FunctionEmitter(TaskEmitter):
    """Node emission of TaskEmitter for the outputs of a ``sym.Function``: a symbol of input k is a read of the lane's
    row of that input, ``x[...]``; there is no skill, so no time slot and no kernel-side kinematics."""

    def __init__(self, leaves, name):
        TaskEmitter.__init__(self, None)
        self.leaves = leaves        # (id(family), index) -> "x[...]"
        self.fn_name = name

    def _ref(self, node):
        op = node.op
        if op == "const":
            return _lit(node.value)
        if op == "sym":
            ref = self.leaves.get((id(node.family), node.index))
            if ref is None:
                raise NotImplementedError("symbol '%s' is not an input of the function '%s'" % (node.name, self.fn_name))
            return ref
        if op in ("fk", "fk_d", "ori_err"):        # (written out before emission, see emit_function)
            raise NotImplementedError("no device code for operation '%s' in a function" % op)
        return self._op(node)


def _expand_all(node):
    """keep_fk / keep_ori of expand.rewrite: no atom is kept"""
    return False


def function_layout(fn):
    """(inputs, outputs) of a ``sym.Function`` as lists of (size1, size2, offset): where each input's row begins in the
    lane's flat input array ``x`` and each output's row in ``y``.  Rows are row-major (entry (i, j) of an
    ``size1 x size2`` matrix at ``offset + i * size2 + j``, numpy order)."""
    ins, outs, off = [], [], 0
    for mx in fn._inputs:
        ins.append((mx.size1(), mx.size2(), off))
        off += mx.numel()
    off = 0
    for mx in fn._outputs:
        outs.append((mx.size1(), mx.size2(), off))
        off += mx.numel()
    return ins, outs


def emit_function(fn):
    """C++ source of ``struct BatchFn`` for a ``sym.Function``: compile-time input / output counts, widths and offsets
    and one straight-line function

        BatchFn::eval(const double (&x)[n_x], double (&y)[n_y])

    that reads the lane's input rows from ``x`` (input k at ``in_off[k]``, ``in_w[k]`` doubles) and writes every entry
    of every output into ``y`` (output k at ``out_off[k]``) exactly once, reading none of them back.  Rows are row-major
    (``function_layout``): the symbols of a matrix input are numbered down the columns (``MX.sym``), its memory runs
    along the rows, and the emitter maps the one to the other.  Common sub-expressions are shared across all outputs;
    ``sin`` / ``cos`` go through ``sincos_joint``, one pair per argument, which the includer supplies (as for
    ``emit_time_slots``).  The kinematics atoms are written out first - there is no kernel-side forward kinematics or
    skill image here - 'fk' and 'ori_err' as for any expression outside the row table, 'fk_d' (what ``cs.jacobian`` of
    a tool position leaves in an output) by ``expand.fk_d_entry``.  NotImplementedError for a symbol that is not one
    of the function's inputs and for an operation without device code."""
    from . import expand
    from . import sym as cs
    ins, outs = function_layout(fn)
    if not ins or not outs or any(a * b == 0 for a, b, _ in ins + outs):
        raise NotImplementedError("function '%s': no device code for a function without inputs or outputs, or with "
                                  "an empty one" % fn.name)
    leaves = {}
    for mx, (s1, s2, off) in zip(fn._inputs, ins):
        arr = cs._as_array(mx)
        for i in range(s1):
            for j in range(s2):
                leaves[(id(arr[i, j].family), arr[i, j].index)] = "x[%d]" % (off + i * s2 + j)
    em = _FunctionEmitter(leaves, fn.name)
    memo, stores = {}, []
    for mx, (s1, s2, off) in zip(fn._outputs, outs):
        arr = cs._as_array(mx)
        for i in range(s1):
            for j in range(s2):
                node = expand.rewrite(arr[i, j], _expand_all, _expand_all, memo, expand_fk_d=True)
                em._keep.append(node)
                stores.append("y[%d] = %s;" % (off + i * s2 + j, em.ref(node)))
    body = "\n        ".join(em.lines + stores)

    def arr_of(vals):
        return "{%s}" % ", ".join(str(v) for v in vals)
    return ("struct BatchFn {\n"
            "    static constexpr int n_in = %d, n_out = %d, n_x = %d, n_y = %d;\n"
            "    static constexpr int in_w[%d] = %s;\n"
            "    static constexpr int in_off[%d] = %s;\n"
            "    static constexpr int out_w[%d] = %s;\n"
            "    static constexpr int out_off[%d] = %s;\n"
            "    __device__ __forceinline__ static void eval(const double (&x)[%d], double (&y)[%d])\n"
            "    {\n"
            "        (void)x;\n"
            "        %s\n"
            "    }\n"
            "};\n" % (len(ins), len(outs), sum(a * b for a, b, _ in ins), sum(a * b for a, b, _ in outs),
                      len(ins), arr_of(a * b for a, b, _ in ins), len(ins), arr_of(o for _, _, o in ins),
                      len(outs), arr_of(a * b for a, b, _ in outs), len(outs), arr_of(o for _, _, o in outs),
                      sum(a * b for a, b, _ in ins), sum(a * b for a, b, _ in outs), body))
