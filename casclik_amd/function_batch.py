"""A ``cs.Function`` evaluated on the device, over a batch or a recorded trajectory, in one launch.

The reference's notebooks compute every user function of the state - the tool position, the tool frame, the
manipulability cost - once per simulated tick on the host (ur5_moe2016_example2.ipynb, cell 12), through CasADi's
compiled ``Function``.  ``sym.Function.__call__`` here is a
scalar tree walk per call; ``DeviceFunction`` is the compiled form: the function's outputs as one straight-line device
function (codegen.emit_function) inside the kernel of csrc/clik_function.hpp, one lane per (record, instance) row.
Inputs and outputs are device tensors, so ``rec["q"]`` of a recording rollout goes in as it is.

    curves = cs.Function("curves", [t, q], [T_fk(q)[:3, 3], J_p, manipulability_cost])
    dfn  = cc.DeviceFunction(curves)          # or curves.on_device()
    p, Jp, man = dfn(times, rec["q"])         # times [R], rec["q"] [R, B, 6]  ->  [R, B, 3], [R, B, 3, 6], [R, B]

There is no host fallback: where the kernel cannot be had, construction raises NotImplementedError.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

from . import jit

SHARED, PER_RECORD, PER_INSTANCE, FULL = "shared", "per_record", "per_instance", "full"


def _strides(kind, B, w):
    return {SHARED: (0, 0), PER_RECORD: (w, 0), PER_INSTANCE: (0, w), FULL: (B * w, w)}[kind]


def plan_arguments(input_sizes, arg_shapes, names=None):
    """How the arguments of one ``DeviceFunction`` call map onto the kernel's rows; a pure function of shapes.

    ``input_sizes``: ``(size1, size2)`` of every input; ``arg_shapes``: the shape of every argument.  Returns
    ``(lead, plans)``: ``lead`` is ``(B,)`` or ``(R, B)``, taken from the argument of highest rank; ``plans[k]`` is
    ``(kind, rec_stride, inst_stride)`` of argument k, strides in doubles, ``kind`` one of ``"shared"`` (0 / 0),
    ``"per_record"`` (w / 0), ``"per_instance"`` (0 / w) and ``"full"`` (B w / w).

    Argument k ends in its value dimensions - ``(size1,)`` for a column, ``(size1, size2)`` for a matrix, numpy order;
    none or ``(1,)`` for a 1-entry input - behind one of the fronts ``()`` (one value for all rows), ``(B,)``,
    ``(R, B)`` and ``(R, 1)`` (one per record).  A 1-entry input reads its shape as front: 0-D or ``(1,)`` one value
    for all rows; 1-D one per record when the lead is ``(R, B)`` and one per instance when it is ``(B,)`` (as
    ``constraint_values_batch`` reads its times); 2-D ``(R, B)`` or ``(R, 1)``; 3-D ``(R, B, 1)`` or ``(R, 1, 1)``.
    When no argument has a front, the lead is ``(1,)``.  Anything else raises ValueError naming the argument and the
    shapes."""
    n = len(input_sizes)
    if len(arg_shapes) != n:
        raise TypeError("expected %d argument(s), got %d" % (n, len(arg_shapes)))
    names = list(names) if names is not None else ["argument %d" % k for k in range(n)]

    def bad(k, why):
        s1, s2 = input_sizes[k]
        raise ValueError("%s (an input of %d x %d) has shape %s: %s" % (names[k], s1, s2, tuple(arg_shapes[k]), why))

    fronts = []
    for k, ((s1, s2), shape) in enumerate(zip(input_sizes, arg_shapes)):
        shape = tuple(int(v) for v in shape)
        if s1 * s2 == 1:
            if len(shape) == 3:
                if shape[2] != 1:
                    bad(k, "a 3-D argument of a 1-entry input is [R, B, 1]")
                shape = shape[:2]
            elif len(shape) > 3:
                bad(k, "too many dimensions")
            elif shape == (1,):
                shape = ()
            fronts.append(shape)
            continue
        value = (s1,) if s2 == 1 else (s1, s2)
        if len(shape) < len(value) or shape[len(shape) - len(value):] != value:
            bad(k, "it must end in %s" % (value,))
        front = shape[:len(shape) - len(value)]
        if len(front) > 2:
            bad(k, "in front of %s there may be (), (B,), (R, B) or (R, 1)" % (value,))
        fronts.append(front)
    rank = max([len(f) for f in fronts] + [1])
    if rank == 2:
        twos = [(k, f) for k, f in enumerate(fronts) if len(f) == 2]
        R = twos[0][1][0]
        # (a [B] block of rows shared by all records counts: times as [R, 1] next to a 2-D q)
        B = max([f[1] for _, f in twos] + [f[0] for k, f in enumerate(fronts)
                                            if len(f) == 1 and input_sizes[k][0] * input_sizes[k][1] > 1])
        lead = (R, B)
    else:
        ones = [f[0] for f in fronts if len(f) == 1]
        B = ones[0] if ones else 1
        lead = (B,)
    plans = []
    for k, front in enumerate(fronts):
        w = input_sizes[k][0] * input_sizes[k][1]
        if len(front) == 0:
            kind = SHARED
        elif rank == 2 and len(front) == 2:
            if front[0] != lead[0]:
                bad(k, "the call has %d record(s) (lead shape %s)" % (lead[0], lead))
            if front[1] == B and B != 1:
                kind = FULL
            elif front[1] == 1:
                kind = PER_RECORD
            else:
                bad(k, "the call has %d instance(s) per record (lead shape %s)" % (B, lead))
        elif rank == 2:         # a 1-D front under an (R, B) lead
            if w == 1:
                if front[0] != lead[0]:
                    bad(k, "a 1-D argument of a 1-entry input is one value per record, and the call has %d (lead "
                           "shape %s)" % (lead[0], lead))
                kind = PER_RECORD
            else:
                if front[0] != B:
                    bad(k, "the call has %d instance(s) per record (lead shape %s)" % (B, lead))
                kind = PER_INSTANCE
        else:
            if front[0] != B:
                bad(k, "the call has %d instance(s) (lead shape %s)" % (B, lead))
            kind = PER_INSTANCE
        plans.append((kind,) + _strides(kind, B, w))
    return lead, plans


def output_shape(lead, size1, size2):
    """``[*lead]`` for a scalar output, ``[*lead, size1]`` for a column, ``[*lead, size1, size2]`` in general"""
    if size1 * size2 == 1:
        return tuple(lead)
    return tuple(lead) + ((size1,) if size2 == 1 else (size1, size2))


class DeviceFunction(object):
    """The device form of a ``sym.Function`` (see the module text).  Construction generates, compiles and loads the
    kernel - cached under ``casclik_amd/_jit``, recorded with ``CLIK_JIT_RECORD`` and replayed by
    ``jit.prebuild_recorded()`` like every other instantiation - and raises NotImplementedError when it cannot be had:
    ``CLIK_JIT=0``, no compiler and nothing cached, an operation without device code, a symbol that is not an input, a
    function too wide for the kernel's LDS."""

    def __init__(self, fn, device=None):
        from . import codegen
        self.function = fn
        self.name = fn.name
        ins, outs = codegen.function_layout(fn)
        self.input_sizes = [(a, b) for a, b, _ in ins]
        self.output_sizes = [(a, b) for a, b, _ in outs]
        slots = max([sum(a * b for a, b in self.input_sizes)] + [a * b for a, b in self.output_sizes])
        if slots > jit.FUNCTION_WAVE_SLOTS:
            raise NotImplementedError(
                "function '%s': its inputs together have %d entries and its widest output %d; the kernel stages them "
                "through LDS, %d bytes per block of 256 rows, which holds %d entries per row at most (every input "
                "counts, also one a call passes as a shared or per-record value: the kernel is built before the calls)"
                % (fn.name, sum(a * b for a, b in self.input_sizes), max(a * b for a, b in self.output_sizes),
                   jit.FUNCTION_LDS_BYTES, jit.FUNCTION_WAVE_SLOTS))
        if os.environ.get("CLIK_JIT", "1") == "0":
            raise NotImplementedError("function '%s' needs a run-time instantiated kernel and CLIK_JIT=0 forbids "
                                      "instantiating one; there is no host fallback" % fn.name)
        so, tag = jit.build_function_library(fn)
        if so is None:
            raise NotImplementedError(
                "no kernel could be instantiated for the function '%s': hipcc is missing and nothing is cached under "
                "%s (kernel %s)" % (fn.name, jit.CACHE, tag))
        self.kernel_name = "jit_" + tag
        self._device = None
        self._requested_device = device
        from . import _capi
        _capi._preload_hip_runtime()        # (the object is linked without the HIP runtime, like the main library)
        self._lib = jit._load(so)
        self._launch = self._lib.clik_jit_function_batch
        self._launch.restype = C.c_int
        self._launch.argtypes = [C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        info = self._lib.clik_jit_function_info
        info.restype, info.argtypes = C.c_int, [C.c_int, C.c_int]
        got = ([info(2, k) for k in range(info(0, 0))], [info(3, k) for k in range(info(1, 0))])
        want = ([a * b for a, b in self.input_sizes], [a * b for a, b in self.output_sizes])
        if got != want:
            raise RuntimeError("the cached kernel %s was generated for other widths (%s, function: %s)"
                               % (self.kernel_name, got, want))
        self.lds_bytes = info(4, 0)
        self.scratch_bytes = None
        import torch
        if device is not None or torch.cuda.is_available():
            self._bind_device()

    def _bind_device(self):
        """the device the launches go to, resolved once; asks the runtime whether the kernel spills"""
        from .controllers.base_controller import device_of
        import torch
        self._device = device_of(self._requested_device)
        with torch.cuda.device(self._device):
            scratch = self._lib.clik_jit_function_scratch
            scratch.restype = C.c_int
            self.scratch_bytes = scratch()
        if self.scratch_bytes and self.scratch_bytes > 0:
            warnings.warn("function '%s': the kernel spills %d bytes per row to scratch memory; it runs, slower than "
                          "a function that fits the registers" % (self.name, self.scratch_bytes))

    def __repr__(self):
        return "DeviceFunction(%s, %s)" % (self.name, self.kernel_name)

    def __call__(self, *args, **kw):
        out = kw.pop("out", None)
        if kw:
            raise TypeError("unexpected keyword argument(s) %s" % sorted(kw))
        if len(args) != len(self.input_sizes):
            raise TypeError("%s expects %d arguments" % (self.name, len(self.input_sizes)))
        import torch
        from .controllers.base_controller import check_out_tensor
        if self._device is None:
            self._bind_device()
        dev = self._device
        names = ["argument %d of %s" % (k, self.name) for k in range(len(args))]
        vals, all_np = [], True
        for a in args:
            if isinstance(a, torch.Tensor):
                all_np = False
                vals.append(a)
            else:
                if hasattr(a, "toarray"):
                    a = a.toarray()
                vals.append(np.asarray(a, dtype=np.float64))
        lead, plans = plan_arguments(self.input_sizes, [tuple(v.shape) for v in vals], names)
        # a contiguous float64 tensor on the device is read in place; anything else becomes one
        tens = [v.to(device=dev, dtype=torch.float64).contiguous() if isinstance(v, torch.Tensor)
                else torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in vals]
        shapes = [output_shape(lead, a, b) for a, b in self.output_sizes]
        if out is None:
            outs = [torch.empty(s, dtype=torch.float64, device=dev) for s in shapes]
        else:
            outs = [out] if isinstance(out, torch.Tensor) else list(out)
            if len(outs) != len(shapes):
                raise ValueError("out must hold %d tensor(s), one per output of %s" % (len(shapes), self.name))
            for k, (t, s) in enumerate(zip(outs, shapes)):
                if t is None:
                    raise ValueError("out[%d] of %s is None" % (k, self.name))
                check_out_tensor(t, s, "float64", dev, "out[%d] of %s" % (k, self.name))
        R, B = (lead[0], lead[1]) if len(lead) == 2 else (1, lead[0])
        if R * B > 0:
            n_in, n_out = len(tens), len(outs)
            in_p = (C.c_void_p * n_in)(*[t.data_ptr() for t in tens])
            rs = (C.c_longlong * n_in)(*[p[1] for p in plans])
            is_ = (C.c_longlong * n_in)(*[p[2] for p in plans])
            out_p = (C.c_void_p * n_out)(*[t.data_ptr() for t in outs])
            with torch.cuda.device(dev):
                rc = self._launch(R, B, in_p, rs, is_, out_p, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if rc != 0:
                raise RuntimeError("%s: the launch of %s failed (hipError_t %d)" % (self.name, self.kernel_name, rc))
        if all_np:
            outs = [t.cpu().numpy() for t in outs]
        return outs[0] if len(outs) == 1 else tuple(outs)
