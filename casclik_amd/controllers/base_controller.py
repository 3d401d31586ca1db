"""Shared plumbing of the device controllers.

``BaseController`` keeps the reference's ``controller_type<label>`` repr
(reference: casclik/controllers/base_controller.py:1-6) and carries everything
of a device controller that is not controller mathematics: the handle's
lifetime, set-up, batch marshalling, per-instance time, rollout times, resident
ticks and the staging of ``solve()``.  The helpers move batches between numpy /
torch and the device pointers the C ABI takes; torch is used purely as the
device allocator and stream provider.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

from .. import _capi
from ..lowering import lower_skill


def _torch():
    import torch
    return torch


def device_of(device=None):
    torch = _torch()
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError(
                "casclik_amd controllers run on an AMD GPU through the HIP "
                "library; no GPU is visible and there is no CPU fallback.")
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        # ("cuda" without an index never compares equal to a tensor's "cuda:0": resolve it once, here)
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def check_out_tensor(t, shape, dtype_name, device, what):
    """An output tensor the kernels write through ``data_ptr()``: it must be exactly what they assume -
    a contiguous torch tensor of that shape and dtype on the controller's device - or the launch would write
    out of bounds / garbage instead of raising."""
    torch = _torch()
    if t is None:
        return
    want = getattr(torch, dtype_name)
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor on %s" % (what, device))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
    if t.dtype != want:
        raise ValueError("%s must be %s, got %s" % (what, want, t.dtype))
    if t.device != torch.device(device):
        raise ValueError("%s lives on %s, the controller on %s" % (what, t.device, device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)


def to_device_matrix(val, width, device, what, batch=None):
    """numpy / list / DM / torch -> contiguous float64 [B, width] tensor on
    ``device``; returns (tensor, was_numpy)."""
    torch = _torch()
    if val is None:
        return None, True
    if isinstance(val, torch.Tensor):
        t = val
        if t.dim() == 1:
            t = t.reshape(1, -1) if width != 1 or t.numel() == 1 else t.reshape(-1, 1)
        t = t.to(device=device, dtype=torch.float64).contiguous()
        was_numpy = False
    else:
        if hasattr(val, "toarray"):
            val = val.toarray()
        arr = np.asarray(val, dtype=np.float64)
        if arr.ndim == 0:
            arr = arr.reshape(1, 1)
        elif arr.ndim == 1:
            arr = arr.reshape(1, -1) if arr.size == width else arr.reshape(-1, width)
        elif arr.ndim == 2 and arr.shape[1] != width and arr.shape[0] == width and arr.shape[1] == 1:
            arr = arr.T
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        was_numpy = True
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError("%s must have %d columns, got shape %s"
                         % (what, width, tuple(t.shape)))
    if batch is not None and t.shape[0] != batch:
        raise ValueError("%s has %d rows, expected %d" % (what, t.shape[0], batch))
    return t, was_numpy


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream(device):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def free_stream(device, tries=12, wait_s=0.25):
    """A stream whose work makes progress WHILE a resident kernel holds its own stream's hardware queue.  The runtime
    multiplexes streams onto a few hardware queues (round-robin by creation order, per priority): a producer stream that
    lands on the resident kernel's queue waits until the kernel leaves - by its watchdog, seconds later.  Which queue a new
    stream gets depends on how many streams the process created before, so asking for "another priority" is not enough
    (seen in the GPU suite: the same test passed or stalled with the number of streams earlier tests had made).  This
    tries candidate streams of both priorities with a one-word kernel and returns the first on which it completes within
    ``wait_s``; RuntimeError if none does."""
    import time
    torch = _torch()
    dev = device_of(device)
    probe = torch.zeros(1, dtype=torch.int32, device=dev)
    kept = []       # (stalled candidates stay alive until we return: a freed stream's queue slot would be handed out again)
    for k in range(tries):
        s = torch.cuda.Stream(device=dev, priority=-1 if k % 2 == 0 else 0)
        with torch.cuda.stream(s):
            probe.add_(1)
        t0 = time.time()
        while time.time() - t0 < wait_s:
            if s.query():
                return s
            time.sleep(0.002)
        kept.append(s)
    raise RuntimeError("no stream makes progress beside the resident kernel (%d candidates tried): is another kernel "
                       "occupying the device?" % tries)


class ResidentWatchdog(RuntimeError):
    """A resident run ended by its watchdog (``ticket[32] == 2``): some wave used up the poll budget waiting for a ticket."""


def resident_wait(run):
    """Wait for a resident run (the dict ``resident_start`` returned) to leave and say how: returns the number of ticks
    every wave finished; raises ``ResidentWatchdog`` when the kernel left by its watchdog instead (nobody published the
    next ticket within ``timeout_s`` - typically a feeder whose stream shares the kernel's hardware queue, see
    ``free_stream``).  ``ticket[32] == 1`` (the caller asked it to stop) is not an error."""
    run["stream"].synchronize()
    tk = run["ticket"].cpu()
    stop, ticks_done = int(tk[32]), int(tk[49])
    if stop == 2:
        raise ResidentWatchdog(
            "resident kernel left by its watchdog after %d tick(s): wave %d used up its budget of %d polls waiting for ticket "
            "%d (in_seq = %d).  Is the producer on a stream that makes progress beside the kernel (resident_feed_stream())?"
            % (ticks_done, int(tk[54]), (int(tk[50]) & 0xffffffff) | ((int(tk[51]) & 0xffffffff) << 32), ticks_done + 1,
               int(tk[0])))
    return ticks_done


class SingleSlot(object):
    """Persistent staging for the single-instance ``solve()`` call (B = 1): one pinned host
    buffer each way that the kernel reads and writes in place (pinned host memory is mapped into
    the device's address space on ROCm, same pointer), so a call is one launch and one stream
    synchronisation - no copy commands.  ``CLIK_SOLVE_STAGED=1`` restores the staged variant
    (pinned -> device copy, launch, device -> pinned copy)."""

    def __init__(self, device, n_in, n_out, n_int):
        torch = _torch()
        self.device = device
        self.zero_copy = os.environ.get("CLIK_SOLVE_STAGED", "0") != "1"
        self.h_in = torch.empty((max(n_in, 1),), dtype=torch.float64).pin_memory()
        self.d_in = torch.empty((max(n_in, 1),), dtype=torch.float64, device=device)
        # outputs: n_out doubles followed by n_int int32 (padded to 8 bytes)
        self.n_out, self.n_int = n_out, n_int
        nbytes = 8 * n_out + 8 * ((n_int + 1) // 2)
        self.d_out = torch.zeros((max(nbytes, 8),), dtype=torch.uint8, device=device)
        self.h_out = torch.zeros((max(nbytes, 8),), dtype=torch.uint8).pin_memory()
        self.in_np = self.h_in.numpy()
        out_np = self.h_out.numpy()
        self.out_f = out_np[:8 * n_out].view(np.float64)
        self.out_i = out_np[8 * n_out:8 * n_out + 4 * n_int].view(np.int32)
        # one device in the process: no device-guard context around the call (it costs ~3 us)
        import contextlib
        self._single_device = torch.cuda.device_count() == 1
        self._no_guard = contextlib.nullcontext()
        self._stream = None
        self.d_in_ptr = self.h_in.data_ptr() if self.zero_copy else self.d_in.data_ptr()
        self.d_out_ptr = self.h_out.data_ptr() if self.zero_copy else self.d_out.data_ptr()

    def in_ptr(self, offset_doubles):
        return C.c_void_p(self.d_in_ptr + 8 * offset_doubles)

    def out_ptr(self, offset_doubles):
        return C.c_void_p(self.d_out_ptr + 8 * offset_doubles)

    def int_ptr(self, index=0):
        return C.c_void_p(self.d_out_ptr + 8 * self.n_out + 4 * index)

    def guard(self):
        """Device context for the call (a no-op when the process has one device)."""
        return self._no_guard if self._single_device else _torch().cuda.device(self.device)

    def begin(self):
        """Stream of this call (torch's current stream, looked up once) as a launch argument."""
        self._stream = _torch().cuda.current_stream(self.device)
        if not self.zero_copy:
            self.d_in.copy_(self.h_in, non_blocking=True)
        return C.c_void_p(self._stream.cuda_stream)

    def upload(self):
        if not self.zero_copy:
            self.d_in.copy_(self.h_in, non_blocking=True)

    def download(self):
        torch = _torch()
        if not self.zero_copy:
            self.h_out.copy_(self.d_out, non_blocking=True)
        st = self._stream if self._stream is not None else torch.cuda.current_stream(self.device)
        self._stream = None
        st.synchronize()


def scalar_of(v):
    if hasattr(v, "toarray"):
        v = v.toarray()
    return np.asarray(v, dtype=float).reshape(-1)[0]


def flat_vector(v, n, what):
    if hasattr(v, "toarray"):
        v = v.toarray()
    arr = np.asarray(v, dtype=np.float64).reshape(-1)
    if arr.size != n:
        raise ValueError("%s must have %d entries, got %d" % (what, n, arr.size))
    return arr


def rollout_records(n_ticks, record_every):
    """Number of records ``R = n_ticks // record_every`` of a recording rollout (record r is taken after tick
    ``(r + 1) * record_every``, counted from 1; ticks after the last multiple are not recorded; ``record_every >
    n_ticks`` gives none); ``None`` when ``record_every`` is None (recording off).  ValueError unless an int >= 1."""
    if record_every is None:
        return None
    if isinstance(record_every, bool) or not isinstance(record_every, (int, np.integer)) or record_every < 1:
        raise ValueError("record_every must be an int >= 1 or None, got %r" % (record_every,))
    return int(n_ticks) // int(record_every)


def ring_depth_request(ring_depth):
    """``ring_depth`` of ``resident_start`` as an int: 1 for plain ``[B, n]`` tensors, D > 1 for rings ``[D, B, n]``.
    ValueError below 1."""
    D = int(ring_depth)
    if D < 1:
        raise ValueError("ring_depth must be at least 1")
    return D


def per_tick_input(input_var, n_ticks, n_y):
    """Is ``input_var`` one target per tick?  True for a ``[n_ticks, B, n_y]`` array or tensor (tick i reads record
    i); False for what a rollout took before (``[B, n_y]``, a vector, None).  ValueError for a 3-D ``input_var`` whose
    first dimension is not ``n_ticks`` or whose last is not ``n_y``."""
    if input_var is None or hasattr(input_var, "toarray"):
        return False
    shape = tuple(input_var.shape) if hasattr(input_var, "shape") else np.shape(input_var)
    if len(shape) != 3:
        return False
    if shape[0] != n_ticks:
        raise ValueError("input_var [n_ticks, B, n_y] has %d records, the rollout %d ticks" % (shape[0], n_ticks))
    if shape[2] != n_y:
        raise ValueError("input_var must have %d columns, got shape %s" % (n_y, shape))
    return True


def rollout_stage_times(time_vars, dt, method):
    """The times at which a rollout evaluates its time slots, as the host computes them: ``time_vars`` itself for
    ``method="euler"``; for ``"rk4"`` tick-major, stage-minor ``t, t + 0.5 * dt, t + 0.5 * dt, t + dt`` - one rounded
    add each (``0.5 * dt`` is exact), the identity the device's time kernel keeps bit for bit (clik_time.hpp).
    ValueError for any other method."""
    if method not in ("euler", "rk4"):
        raise ValueError("method must be 'euler' or 'rk4'")
    times = np.asarray(time_vars, dtype=float).reshape(-1)
    if method == "rk4":
        return np.stack([times, times + 0.5 * dt, times + 0.5 * dt, times + dt], axis=1).reshape(-1)
    return times


def record_layout(fields, R, B):
    """``{name: (shape, dtype name)}`` of the records of a rollout: ``fields`` is a list of ``(name, width, dtype
    name)``; width 0 leaves the field out, width None makes it ``[R, B]`` (one number per instance), any other
    ``[R, B, width]``."""
    out = {}
    for name, width, dtype in fields:
        if width == 0:
            continue
        out[name] = ((R, B) if width is None else (R, B, int(width)), dtype)
    return out


def constraint_row_slices(descriptor):
    """``label -> slice`` into the ``M_tot`` rows of ``constraint_values_batch``, in skill order: the rows of a
    lowered skill's constraints one after the other (the Velocity*Constraints included)."""
    from collections import OrderedDict
    out, r = OrderedDict(), 0
    for task in descriptor.tasks:
        out[task["label"]] = slice(r, r + int(task["m"]))
        r += int(task["m"])
    return out


def summary_tolerances(tol, m_tot):
    """``tol`` of ``constraint_summary_batch`` as ``[m_tot]`` float64 (None stays None): a scalar for all rows or one
    value per row, finite and >= 0.  ValueError otherwise."""
    if tol is None:
        return None
    arr = np.asarray(tol.detach().cpu().numpy() if hasattr(tol, "detach") else tol, dtype=np.float64)
    if arr.ndim == 0:
        arr = np.full(m_tot, float(arr))
    arr = arr.reshape(-1)
    if arr.size != m_tot:
        raise ValueError("tol has %d entries, the skill %d constraint rows" % (arr.size, m_tot))
    if not (np.isfinite(arr).all() and (arr >= 0.0).all()):
        raise ValueError("tol must be finite and >= 0")
    return np.ascontiguousarray(arr)


def rollout_summary_request(summary, summary_tol, n_ticks, m_tot):
    """What ``rollout_batch(..., summary=, summary_tol=)`` asks for, checked on the host: ``(False, None)`` without
    ``summary``, else ``(True, tol)`` with ``tol`` as ``summary_tolerances`` returns it (``[m_tot]`` float64 or None).
    ValueError for a ``summary_tol`` without ``summary=True``, for a summary of no tick at all, and for what
    ``summary_tolerances`` refuses (wrong length, negative, non-finite)."""
    if not summary:
        if summary_tol is not None:
            raise ValueError("summary_tol needs summary=True")
        return False, None
    if int(n_ticks) < 1:
        raise ValueError("summary=True needs at least one tick: a summary of no record does not exist")
    return True, summary_tolerances(summary_tol, m_tot)


def converge_tolerances(tol, m_tot):
    """``tol`` of ``converge_batch`` as ``[m_tot]`` float64: a scalar for all rows or one value per row, each >= 0;
    ``+inf`` is allowed (the row cannot block).  ValueError for a wrong length, a negative entry and NaN."""
    arr = np.asarray(tol.detach().cpu().numpy() if hasattr(tol, "detach") else tol, dtype=np.float64)
    if arr.ndim == 0:
        arr = np.full(m_tot, float(arr))
    arr = arr.reshape(-1)
    if arr.size != m_tot:
        raise ValueError("tol has %d entries, the skill %d constraint rows" % (arr.size, m_tot))
    if np.isnan(arr).any() or (arr < 0.0).any():
        raise ValueError("tol must be >= 0 (+inf allowed), not NaN")
    return np.ascontiguousarray(arr)


def converge_request(tol, max_ticks, min_step, input_var, m_tot):
    """What ``converge_batch`` asks for, checked on the host: ``(tol [m_tot] float64, max_ticks)``.  ValueError for a bad
    ``tol`` (``converge_tolerances``), ``max_ticks < 0``, a negative or NaN ``min_step`` and a 3-D ``input_var``: the
    target of a converging rollout is fixed."""
    shape = tuple(input_var.shape) if hasattr(input_var, "shape") and not hasattr(input_var, "toarray") else ()
    if len(shape) >= 3:
        raise ValueError("input_var must be [B, n_y]: targets are fixed here, one per instance for the whole launch "
                         "(rollout_batch follows a target per tick), got shape %s" % (shape,))
    if isinstance(max_ticks, bool) or not isinstance(max_ticks, (int, np.integer)) or max_ticks < 0:
        raise ValueError("max_ticks must be an int >= 0, got %r" % (max_ticks,))
    if not float(min_step) >= 0.0:
        raise ValueError("min_step must be >= 0, got %r" % (min_step,))
    return converge_tolerances(tol, m_tot), int(max_ticks)


def converge_group_request(group, B):
    """``group`` of ``converge_batch`` as an int, checked on the host.  ValueError for anything but an int among 1, 2, 4,
    8, 16, 32, 64 (bools and floats are refused as for ``max_ticks``) and for a batch of ``B`` instances that is not
    whole groups."""
    if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or int(group) not in (1, 2, 4, 8, 16, 32, 64):
        raise ValueError("group must be one of 1, 2, 4, 8, 16, 32, 64, got %r" % (group,))
    if int(B) % int(group) != 0:
        raise ValueError("group=%d: the batch must be whole groups, got %d instances" % (group, B))
    return int(group)


def velocity_feedback_request(fb, n_q, n_x, n_y):
    """``options["velocity_feedback"]`` checked against a lowered skill (``n_q`` robot, ``n_x`` virtual variables, ``n_y``
    entries of ``input_var``): the map as a tuple of ints, one per state - robot variables first -, entry j the index
    into ``input_var`` that the next tick of an on-device loop reads the velocity of state j in, -1 for none.  None for no
    option (None) and for a map that feeds nothing.  ValueError for a skill without ``input_var``, a wrong length, an
    entry that is no int in ``[-1, n_y)`` and an ``input_var`` index named twice.  No device is needed."""
    if fb is None:
        return None
    try:
        entries = list(fb.tolist() if hasattr(fb, "tolist") else fb)
    except TypeError:
        raise ValueError("options['velocity_feedback'] must be a sequence of ints, got %r" % (fb,))
    if n_y <= 0:
        raise ValueError("options['velocity_feedback'] needs a skill with input_var: the velocities are fed into it")
    if len(entries) != n_q + n_x:
        raise ValueError("options['velocity_feedback'] must have %d entries (%d robot and %d virtual variables), got %d"
                         % (n_q + n_x, n_q, n_x, len(entries)))
    for j, k in enumerate(entries):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not -1 <= int(k) < n_y:
            raise ValueError("options['velocity_feedback'][%d] must be an int in [-1, %d), got %r" % (j, n_y, k))
    entries = tuple(int(k) for k in entries)
    named = [k for k in entries if k >= 0]
    if len(set(named)) != len(named):
        raise ValueError("options['velocity_feedback'] names input_var[%d] twice"
                         % next(k for k in named if named.count(k) > 1))
    return entries if named else None


def padded_seeds(S):
    """Seeds per target of an ``ik_batch(first_hit=True)`` launch: ``S`` padded to the next power of two, the size of a
    group of lanes.  ValueError for ``S > 64``: a group does not span two waves."""
    S = int(S)
    if S > 64:
        raise ValueError("first_hit serves at most 64 seeds per target (a target's seeds share a wave), got %d" % S)
    return 1 << (S - 1).bit_length() if S > 1 else 1


def select_seeds(ticks, status, residual, tol, S):
    """Which of its ``S`` seeds serves each target of an ``ik_batch`` launch: a pure function of torch tensors, on any
    device.  ``ticks``, ``status`` ``[T * S]`` and ``residual`` ``[T * S, M_tot]`` are ``converge_batch``'s info of
    instance ``t * S + s``, ``tol`` ``[M_tot]``.  Returns the seed index ``[T]`` (int64).  Among a target's seeds with
    status 0 the fewest ticks wins, then the lowest index.  If none has status 0, the seed whose ``max_i residual_i /
    tol_i`` over the rows with a finite, non-zero ``tol_i`` is smallest wins (then the lowest index); a seed with status 4
    is chosen only when all of the target's seeds have it."""
    torch = _torch()
    S = int(S)
    T = ticks.numel() // S
    ticks, status = ticks.reshape(T, S), status.reshape(T, S)
    tol = torch.as_tensor(tol, dtype=torch.float64, device=residual.device).reshape(-1)
    rows = torch.isfinite(tol) & (tol != 0.0)
    if bool(rows.any()):
        score = (residual.reshape(T, S, -1)[:, :, rows] / tol[rows]).amax(dim=2)
    else:
        score = torch.zeros((T, S), dtype=torch.float64, device=residual.device)
    cls = torch.where(status == 0, 0, torch.where(status == 4, 2, 1))
    best = cls.amin(dim=1, keepdim=True)
    key = torch.where(best == 0, ticks.to(torch.float64), torch.where(best == 1, score, torch.zeros_like(score)))
    inf = torch.full_like(key, float("inf"))
    key = torch.where(cls == best, key, inf)
    hit = (cls == best) & (key == key.amin(dim=1, keepdim=True))
    idx = torch.arange(S, device=ticks.device).expand(T, S)
    return torch.where(hit, idx, torch.full_like(idx, S)).amin(dim=1)


def trajectory_rows(val, width, what, lead=None):
    """``val`` as ``(tensor-or-array [R, B, width], ndim)``: a ``[B, width]`` matrix (or what ``to_device_matrix`` takes
    for one) is one record, ``ndim`` 2; a ``[R, B, width]`` array or tensor stays as it is, ``ndim`` 3.  ``lead``: the
    ``(R, B)`` it must have.  ValueError otherwise."""
    shape = tuple(val.shape) if hasattr(val, "shape") and not hasattr(val, "toarray") else None
    if shape is not None and len(shape) == 3:
        if shape[2] != width:
            raise ValueError("%s must have %d columns, got shape %s" % (what, width, shape))
        if lead is not None and shape[:2] != tuple(lead):
            raise ValueError("%s [R, B, %d] has shape %s, robot_var %d record(s) of %d instance(s)"
                             % (what, width, shape, lead[0], lead[1]))
        return val, 3
    if shape is not None and len(shape) > 3:
        raise ValueError("%s must be [B, %d] or [R, B, %d], got shape %s" % (what, width, width, shape))
    return val, 2


class BaseController(object):
    """What a device controller is apart from its mathematics.  A controller class names the C entry points that make
    and free its handle (``_create_fn`` / ``_destroy_fn``), returns their options structure from ``_c_options(descriptor)``, says
    in ``_slot_results()`` how many doubles and int32 its ``solve()`` brings back, names its tick entry points
    (``_tick_fn`` / ``_tick_t_fn``) and the outputs behind the velocities (``_rollout_tail``), and has ``skill_spec`` and
    ``options``; ``_create_handle()`` then gives it ``_lib``, ``_handle``, ``_device`` and ``descriptor``, which every
    other helper here works from."""
    controller_type = "BaseController"
    _create_fn = _destroy_fn = None
    _kind = None                # "pinv" | "qp": whose clik_<kind>_* entry points and jit.UNITS entries the handle takes
    # what a rollout returns after dX and records after dx: (name, descriptor attribute of its width | None: one number per
    # instance, dtype name); a width of 0 leaves the output out (None in the result, no record)
    _rollout_tail = ()
    _kernels = {}               # on-demand kernels asked for so far, what -> cache tag | False (``_create_handle`` resets it)
    # the converging rollouts loaded so far, group -> (cache tag, attach function, its arguments) | False, and the group of
    # the one attached (``_require_converge_kernel``; ``_create_handle`` resets both)
    _converge_units = {}
    _converge_group = None
    _feedback = None            # options["velocity_feedback"] as ``velocity_feedback_request`` returns it (set-up)

    def __repr__(self):
        return self.controller_type + "<" + self.skill_spec.label + ">"

    # -- handle lifetime ----------------------------------------------------------------------------------------
    def __del__(self):
        self._release()

    def _release(self):
        if getattr(self, "_handle", None) is not None and self._lib is not None:
            try:
                getattr(self._lib, self._destroy_fn)(self._handle)
            except Exception:
                pass
            self._handle = None
        self._slot = None

    def _require_handle(self):
        if self._handle is None:
            raise RuntimeError("call setup_problem_functions() / setup_solver() first")

    # -- set-up -------------------------------------------------------------------------------------------------
    def _create_handle(self):
        """Lower the skill and create its handle on the controller's device (``options["device"]``, by default the
        current one).  Returns the C descriptor and options, which the ``jit.attach*`` calls take as well."""
        self._release()
        self._lib = _capi.load_library()
        self.descriptor = lower_skill(self.skill_spec)
        self._setup_velocity_feedback()     # (checked before anything is made on the device)
        cdesc = _capi.desc_to_c(self.descriptor)
        copts = self._c_options(self.descriptor)
        self._device = device_of(self.options.get("device"))
        handle = C.c_void_p()
        with _torch().cuda.device(self._device):
            rc = getattr(self._lib, self._create_fn)(C.byref(cdesc), C.byref(copts), C.byref(handle))
        _capi.check(self._lib, rc)
        self._handle = handle
        self._setup_c = (cdesc, copts)      # (the on-demand kernels are instantiated later, at their first use)
        self._kernels = {}
        self._converge_units, self._converge_group = {}, None
        return cdesc, copts

    def _want_jit(self):
        """May kernels be instantiated for this skill at set-up (the reference JIT-compiles at this point too,
        function_opts["jit"])?  ``CLIK_JIT=0`` and ``CLIK_FORCE_DYNAMIC=1`` say no for the whole process."""
        fopts = self.options.get("function_opts") or {}
        return fopts.get("jit", True) and os.environ.get("CLIK_JIT", "1") != "0" \
            and os.environ.get("CLIK_FORCE_DYNAMIC", "0") != "1"

    def _attach_or_warn(self, attach, instead, limit):
        """One ``jit.attach*`` call on the controller's device.  A failed instantiation is not fatal when another
        kernel serves the skill: warn (``instead`` says which one runs, then the first ``limit`` characters of the
        compiler's message) and return None - still the GPU path; skills only instantiated kernels can serve are
        refused afterwards (``_require_generated_code_kernel``)."""
        with _torch().cuda.device(self._device):
            try:
                return attach()
            except RuntimeError as exc:
                warnings.warn("%s: %s" % (instead, str(exc)[:limit]))
                return None

    def _setup_shape_kernel(self, attach):
        """``kernel_name`` of the handle; where no ahead-of-time shape serves the skill ("dynamic" / "none") and kernels
        may be instantiated, ``attach()`` - the controller's ``jit.attach*`` call - instantiates one for its structure
        (the reference JIT-compiles its functions at this point too)."""
        self.kernel_name = getattr(self._lib, "clik_%s_kernel_name" % self._kind)(self._handle).decode()
        if self.kernel_name in ("dynamic", "none") and self._want_jit():
            name = self._attach_or_warn(
                attach, "run-time kernel instantiation failed, using the built-in dynamic-shape kernel", 400)
            if name:
                self.kernel_name = name

    def _setup_value_kernel(self, wanted, attach, instead):
        """``value_kernel``: the tag of the kernel with the skill's own numbers compiled in - one more hipcc run at set-up,
        ``attach()`` - when the controller's rule says it is ``wanted`` and kernels may be instantiated; else None."""
        self.value_kernel = None
        if wanted and self._want_jit():
            self.value_kernel = self._attach_or_warn(attach, instead, 300)

    def _require_generated_code_kernel(self):
        """Constraints outside the row-table family exist only as generated code inside a run-time instantiated
        kernel; there is no other path (and no CPU fallback)."""
        d = self.descriptor
        if d.extern_code and not self.kernel_name.startswith("jit_"):
            raise NotImplementedError(
                "the skill has constraint expressions that need generated device code (%s), but no "
                "kernel could be instantiated for it (jit disabled, hipcc missing, or the skill is "
                "outside the shape-specialised family)" % ", ".join(
                    repr(d.tasks[k]["label"]) for k in sorted(d.extern_code)))

    # -- time slots on the device -------------------------------------------------------------------------------
    def _setup_time_kernel(self):
        """``options["time_on_device"]`` (default False), read at set-up: the skill's time slots as generated device
        code (codegen.emit_time_slots) in a kernel of their own, attached to the handle.  Rollouts and per-instance-time
        ticks then fill their time-term tables on the device from the times (``time_terms_batch``) instead of walking
        the slot trees on the host once per time stamp.  A skill without time slots builds nothing and behaves as
        without the option.  NotImplementedError when the kernel cannot be had (no compiler and nothing cached,
        ``function_opts["jit"]`` false): there is no silent return to the host path."""
        self._kernels.pop("time", None)
        if not self.options.get("time_on_device", False) or self.descriptor.n_tslots == 0:
            return
        tag = None
        if self._want_jit():
            from .. import codegen, jit
            tag = self._attach_or_warn(
                lambda: jit.attach_unit(self._lib, self._handle, self._kind, "time", None, None,
                                        extern=codegen.emit_time_slots(self.descriptor)),
                "the time kernel could not be built", 400)
        if not tag:
            raise NotImplementedError(
                "options['time_on_device'] is set, but no time kernel could be instantiated for the skill's %d time "
                "slot(s) (jit disabled, or hipcc missing and nothing cached)" % self.descriptor.n_tslots)
        self._kernels["time"] = tag

    # -- velocity feedback --------------------------------------------------------------------------------------
    def _setup_velocity_feedback(self):
        """``options["velocity_feedback"] = fb`` (default None), read at set-up and checked there
        (``velocity_feedback_request``): ``fb[j]`` is the index into ``input_var`` in which tick k + 1 of an on-device
        loop - ``rollout_batch`` in all its forms, ``converge_batch``, ``ik_batch`` - reads the velocity of state j
        (robot variables, then virtual ones) that tick k was integrated with; tick 0 reads what the caller gave.  The map
        is compiled into variants of the lane-per-instance kernels, built at their first use; ``solve_batch``,
        ``solve`` and the resident ticks fed by a producer do not change."""
        d = self.descriptor
        self._feedback = velocity_feedback_request(self.options.get("velocity_feedback"), d.n_q, d.n_x, d.n_y)

    def _feedback_defines(self):
        from .. import jit
        return jit.velocity_feedback_defines(self._feedback)

    def _require_feedback_served(self, tag, what):
        """With the velocity feedback a launch has no other kernel to run on: refuse here, saying so."""
        if self._feedback is not None and not tag:
            raise NotImplementedError(
                "options['velocity_feedback'] is set, but no %s with the feedback compiled in could be instantiated for "
                "this skill: only the built-in kernels serve this handle (jit disabled, hipcc missing and nothing cached, "
                "or a skill outside the shape-specialised family), and they feed nothing back" % what)

    @property
    def _time_kernel(self):
        """cache tag of the attached time kernel (``options["time_on_device"]``), or None"""
        return self._kernels.get("time")

    def _require_kernel(self, what):
        """An on-demand kernel of this controller's skill (``jit.UNITS``: "rec" the recording / per-tick-target rollouts,
        "monitor" the constraint values, "summary" the constraint summaries, "rollsum" the summarising rollout; ``jit.CONVERGE_UNITS``: "converge" the rollout
        that runs until each instance has converged),
        instantiated and attached at its first use and cached like every other instantiation.  Where no kernel may be
        instantiated (``_want_jit``) or none can be - a skill outside the shape-specialised family - nothing is attached
        and the library refuses the call (NotImplementedError): there is no chunked or host fallback.  A skill whose
        summary or summarising rollout does not fit the LDS of a compute unit, or would spill, is refused here with the
        figure."""
        if what == "converge":
            return self._require_converge_kernel(1)     # (the one unit with variants: which of them is attached matters)
        if self._kernels.get(what) is None and self._want_jit():
            from .. import jit
            cdesc, copts = self._setup_c
            with _torch().cuda.device(self._device):
                # (the rollouts of a controller with the velocity feedback are the variants with its map compiled in)
                tag = jit.attach_unit(self._lib, self._handle, self._kind, what, cdesc, copts,
                                      extern=self.descriptor.extern_source(), values=bool(self.value_kernel),
                                      defines=self._feedback_defines() if what in ("rec", "rollsum") else ())
            self._kernels[what] = tag or False
        if what in ("rec", "rollsum"):
            self._require_feedback_served(self._kernels.get(what), "rollout")

    def _require_converge_kernel(self, group=1):
        """The converging rollout with the group rule for groups of ``group`` lanes (1: the default unit, whose tag
        ``_kernels["converge"]`` is) attached to the handle: loaded at its first use as ``_require_kernel`` does it,
        kept, and attached again whenever the last call used another.  A variant that cannot be had detaches what is
        attached, so the library refuses the call (NotImplementedError) and no other variant runs in its place."""
        if not self._want_jit():
            self._require_feedback_served(None, "converging rollout")
        if self._converge_group == group or not self._want_jit():   # (what the last call used: nothing to do)
            return
        from .. import jit
        unit = self._converge_units.get(group)
        with _torch().cuda.device(self._device):
            if unit is None:
                cdesc, copts = self._setup_c
                unit = jit.load_unit(self._lib, self._handle, self._kind, "converge", cdesc, copts,
                                     extern=self.descriptor.extern_source(), values=bool(self.value_kernel),
                                     defines=jit.converge_group_defines(group) + self._feedback_defines()) or False
                self._converge_units[group] = unit
                if group == 1:
                    self._kernels["converge"] = unit[0] if unit else False
            if self._converge_group != group:
                attach = jit.CONVERGE_UNITS["converge", self._kind]["attach"]
                _capi.check(self._lib, getattr(self._lib, attach)(self._handle, *(unit[2] if unit else [None])))
                self._converge_group = group
        self._require_feedback_served(unit, "converging rollout")

    def _device_times(self, time_vars):
        """times as a flat contiguous float64 tensor on the controller's device (one that already is, is used in
        place: no host synchronisation) and whether they came as a tensor"""
        torch = _torch()
        if isinstance(time_vars, torch.Tensor):
            return time_vars.to(device=self._device, dtype=torch.float64).reshape(-1).contiguous(), True
        arr = np.ascontiguousarray(np.asarray(time_vars, dtype=np.float64).reshape(-1))
        return torch.from_numpy(arr).to(self._device), False

    def time_terms_batch(self, times, dt=0.0, method="euler"):
        """The time terms of the skill at ``times`` (N of them), computed on the device: ``[N * stages, 2 * n_tslots]``,
        row ``i * stages + s`` what ``descriptor.time_terms`` gives at the time of stage s of tick i - ``stages`` is 1
        for ``method="euler"`` (the time itself) and 4 for ``"rk4"`` (t, t + dt/2, t + dt/2, t + dt).  A device tensor
        when ``times`` is a tensor, numpy otherwise.  Needs ``options["time_on_device"]`` (NotImplementedError
        otherwise).  A row of a non-finite time holds whatever the arithmetic gives."""
        if method not in ("euler", "rk4"):
            raise ValueError("method must be 'euler' or 'rk4'")
        if not self.options.get("time_on_device", False):
            raise NotImplementedError("time_terms_batch needs options['time_on_device'] = True at set-up")
        self._require_handle()
        torch = _torch()
        dev, n_ts = self._device, self.descriptor.n_tslots
        stages = 4 if method == "rk4" else 1
        T, was_tensor = self._device_times(times)
        out = torch.empty((T.numel() * stages, 2 * n_ts), dtype=torch.float64, device=dev)
        if n_ts and T.numel():
            with torch.cuda.device(dev):
                rc = getattr(self._lib, "clik_%s_time_terms" % self._kind)(
                    self._handle, T.numel(), ptr(T), stages, float(dt), ptr(out), current_stream(dev))
            _capi.check(self._lib, rc)
        return out if was_tensor else out.cpu().numpy()

    # -- batches in and out -------------------------------------------------------------------------------------
    def _batch_inputs(self, robot_var, virtual_var=None, input_var=None, clone=False):
        """The inputs of a batch call as contiguous float64 tensors on the controller's device: ``Q [B, n_q]``,
        ``X [B, n_x] | None``, ``Y [B, n_y] | None``, the batch size (``robot_var``'s) and whether ``robot_var`` came as
        numpy (the container type of what the call returns).  Tensors that already are what the kernels read are used
        in place; ``clone`` copies those of ``Q`` and ``X`` (a rollout overwrites them with the final state)."""
        d, dev = self.descriptor, self._device
        Q, was_np = to_device_matrix(robot_var, d.n_q, dev, "robot_var")
        B = Q.shape[0]
        X = Y = None
        x_np = True
        if d.n_x > 0:
            if virtual_var is None:
                raise ValueError("skill has virtual_var: pass virtual_var")
            X, x_np = to_device_matrix(virtual_var, d.n_x, dev, "virtual_var", B)
        if d.n_y > 0:
            if input_var is None:
                raise ValueError("skill has input_var: pass input_var")
            Y, _ = to_device_matrix(input_var, d.n_y, dev, "input_var", B)
        if clone:
            Q = Q if was_np else Q.clone()
            X = X if x_np else X.clone()
        return Q, X, Y, B, was_np

    @staticmethod
    def _to_caller(outs, was_np):
        """A tuple of result tensors (or None) in the container type the inputs came in."""
        return tuple(None if o is None else o.cpu().numpy() for o in outs) if was_np else outs

    # -- per-instance time --------------------------------------------------------------------------------------
    def _instance_times(self, time_var, B):
        """``time_var`` of a batch tick -> ``(t, T, stamps)``.  One stamp for the batch: ``(t, None, None)``.  One per
        instance (robots at different phases of a trajectory): the time-only sub-expressions are evaluated on the host
        per distinct stamp and travel as the device tensor ``T [B, 2 * n_tslots]`` of the ``*_solve_batch_t`` entry
        points; ``stamps = (uniq, inverse)`` serves ``_solve_per_stamp``.  A skill without time slots gives the same
        tick at every stamp: ``(first stamp, None, None)``, the ordinary launch."""
        if self._time_kernel is not None and self.kernel_name not in ("dynamic", "none"):
            # time_on_device: T from the time kernel, in the instances' order - no sorting of the stamps, no tree-walk,
            # and a device tensor of times is read in place.  (A skill on the dynamic fallback kernel keeps the host
            # path below: `_solve_per_stamp` groups by stamp on the host and has no per-instance-time variant.)
            is_tensor = isinstance(time_var, _torch().Tensor)
            n = time_var.numel() if is_tensor else np.size(time_var)
            if is_tensor and n == 1:
                return float(time_var.reshape(-1)[0]), None, None
            if n > 1 and (is_tensor or np.ndim(time_var) > 0):
                if n != B:
                    raise ValueError("time_var has %d entries, the batch %d instances" % (n, B))
                return 0.0, self.time_terms_batch(self._device_times(time_var)[0]), None
        if not (np.ndim(time_var) > 0 and np.size(time_var) > 1):
            return (float(np.asarray(time_var).reshape(-1)[0]) if np.ndim(time_var) > 0 else time_var), None, None
        d = self.descriptor
        times = np.asarray(time_var, dtype=float).reshape(-1)
        if times.size != B:
            raise ValueError("time_var has %d entries, the batch %d instances" % (times.size, B))
        if d.n_tslots == 0:
            return float(times[0]), None, None
        uniq, inverse = np.unique(times, return_inverse=True)
        terms = np.stack([d.time_terms(float(tv)) for tv in uniq])
        T = _torch().from_numpy(np.ascontiguousarray(terms[inverse])).to(self._device)
        return float(times[0]), T, (uniq, inverse)

    def _solve_per_stamp(self, stamps, solve_one, ins, outs):
        """Per-instance time for a skill on the dynamic fallback kernel, which has no per-instance-time variant
        (``CLIK_EUNSUPPORTED``): the batch grouped by distinct time stamp, one launch per group.  ``solve_one(t, *rows
        of ins)`` is the controller's own single-stamp call; its results land in the same rows of ``outs`` (None
        entries on either side are skipped)."""
        torch = _torch()
        uniq, inverse = stamps
        for k, tv in enumerate(uniq):
            rows = torch.from_numpy(np.nonzero(inverse == k)[0]).to(self._device)
            res = solve_one(float(tv), *[None if t is None else t.index_select(0, rows) for t in ins])
            for o, r in zip(outs, res):
                if o is not None:
                    o.index_copy_(0, rows, r)

    # -- outputs of a batch -------------------------------------------------------------------------------------
    def _tail(self):
        """``_rollout_tail`` with this skill's widths: ``[(name, width | None: one number per instance, dtype name)]``"""
        d = self.descriptor
        return [(name, None if width is None else getattr(d, width), dtype) for name, width, dtype in self._rollout_tail]

    def _batch_outputs(self, B, lead=(), given=None, skip=(), init=False):
        """``[dQ, dX, *tail]`` of a batch of ``B`` instances on the controller's device: the velocities ``[B, n_q]`` and
        ``[B, n_x]``, then what ``_rollout_tail`` names, in its order; None for a width of 0 and for a name in ``skip``.
        ``lead``: the leading dimensions of a ring, ``(D,)``.  ``given``: the caller's own tensors, ``{"out": ..., tail
        name: ...}`` (None: not given) - checked as ``out`` / ``<name>_out`` (``check_out_tensor``) and used in place as
        they are.  New tensors are uninitialised, or with ``init`` zeros and, the int32 ones, -1: no tick wrote there."""
        torch = _torch()
        d, dev = self.descriptor, self._device
        given = given or {}
        outs = []
        for name, width, dtype in [("out", d.n_q, "float64"), ("dx", d.n_x, "float64")] + self._tail():
            shape = tuple(lead) + ((B,) if width is None else (B, width))
            t = given.get(name)
            if t is not None:
                check_out_tensor(t, shape, dtype, dev, "out" if name == "out" else name + "_out")
            elif width != 0 and name not in skip:
                if init:
                    t = torch.full(shape, -1 if dtype == "int32" else 0.0, dtype=getattr(torch, dtype), device=dev)
                else:
                    t = torch.empty(shape, dtype=getattr(torch, dtype), device=dev)
            outs.append(t)
        return outs

    # -- ticks --------------------------------------------------------------------------------------------------
    # Every tick entry point takes (handle, B, time terms, q, x, y, dq, dx, *tail, *extra, stream): the controller
    # names the entry for one stamp per batch and the one for a stamp per instance, and what ``extra`` is.
    _tick_fn = _tick_t_fn = None

    def _tick_batch(self, time_var, robot_var, virtual_var, input_var, again, given=None, skip=(), extra=None):
        """One tick of a batch, the body of ``solve_batch``: marshal the inputs (``_batch_inputs``), the time
        (``_instance_times``) and the outputs (``_batch_outputs`` of ``given`` and ``skip``), launch ``_tick_fn`` or -
        a stamp per instance - ``_tick_t_fn`` on torch's current stream, and return ``(dQ, dX, *tail)`` in the caller's
        container.  ``extra(B)`` returns the controller's extra launch arguments and the tensors they carry, ``(args,
        carried)``.  A skill on the dynamic fallback kernel has no per-instance-time variant (``CLIK_EUNSUPPORTED``): one
        launch per distinct stamp (``_solve_per_stamp``) of ``again(t, Q, X, Y, *carried)``, the controller's own
        single-stamp call, which returns the outputs followed by the carried rows."""
        self._require_handle()
        torch = _torch()
        d, dev = self.descriptor, self._device
        Q, X, Y, B, was_np = self._batch_inputs(robot_var, virtual_var, input_var)
        time_var, T, stamps = self._instance_times(time_var, B)
        outs = tuple(self._batch_outputs(B, given=given, skip=skip))
        args, carried = extra(B) if extra else ((), ())
        with torch.cuda.device(dev):
            if T is not None:
                fn, tt = getattr(self._lib, self._tick_t_fn), ptr(T)
            else:
                fn, (_, tt) = getattr(self._lib, self._tick_fn), _capi.tterms_arg(d.time_terms(time_var))
            rc = fn(self._handle, B, tt, ptr(Q), ptr(X), ptr(Y), *map(ptr, outs), *args, current_stream(dev))
        if T is not None and stamps is not None and rc == _capi.CLIK_EUNSUPPORTED:
            self._solve_per_stamp(stamps, again, (Q, X, Y) + carried, outs + carried)
            rc = 0
        _capi.check(self._lib, rc)
        return self._to_caller(outs, was_np)

    def _bind_tick(self, robot_var, input_var, virtual_var, given=None, extra=None):
        """The body of ``bind_batch``: marshal once, return ``tick(time_var=0.0, stream_handle=None)`` - per call the
        time terms (unless the skill has no time slots), the stream, ONE launch of ``_tick_fn`` and a status check.
        ``extra(B)`` returns ``(first, later, carried)``: the controller's extra launch arguments of the first call and of
        every later one - and of the first as well once ``tick.primed`` is set - and the tensors they carry.
        ``tick.tensors`` holds everything the launch reads and writes (``Q, X, Y, dQ, dX, *tail, *carried``),
        ``tick.out`` the velocities and ``tick.<name>`` each output of ``_rollout_tail``."""
        self._require_handle()
        d, dev = self.descriptor, self._device
        Q, X, Y, B, _ = self._batch_inputs(robot_var, virtual_var, input_var)
        outs = self._batch_outputs(B, given=given)
        first, later, carried = extra(B) if extra else ((), (), ())
        fn, handle, lib = getattr(self._lib, self._tick_fn), self._handle, self._lib
        args = tuple(map(ptr, (Q, X, Y, *outs)))
        static_tt = _capi.tterms_arg(np.zeros(0)) if d.n_tslots == 0 else None
        ticked = [extra is None]        # (without extra arguments there is no first call to tell from the others)

        def tick(time_var=0.0, stream_handle=None):
            tt, ttp = static_tt if static_tt is not None else _capi.tterms_arg(d.time_terms(time_var))
            sh = stream_handle if stream_handle is not None else current_stream(dev)
            rc = fn(handle, B, ttp, *args, *(later if ticked[0] or tick.primed else first), sh)
            ticked[0] = True
            if rc != 0:
                _capi.check(lib, rc)

        if extra is not None:
            tick.primed = False
        tick.tensors = (Q, X, Y, *outs) + tuple(carried)
        tick.out = outs[0]
        for (name, _, _), t in zip(self._rollout_tail, outs[2:]):
            setattr(tick, name, t)
        return tick

    # -- rollouts -----------------------------------------------------------------------------------------------
    def _rollout_times(self, time_vars, dt, method):
        """``(n_ticks, stages, tterms)`` of a rollout: ``stages`` is 1 for ``method="rk4"`` (the right-hand side at t,
        t + dt/2, t + dt/2, t + dt of every tick), 0 for ``"euler"`` (at t); ``tterms`` the ``_capi.tterms_arg`` pair
        of the time terms of all stage times, one after the other."""
        d = self.descriptor
        stage_times = rollout_stage_times(time_vars, dt, method)
        tt = np.concatenate([d.time_terms(t) for t in stage_times]) if d.n_tslots else np.zeros(0)
        return int(np.size(time_vars)), 1 if method == "rk4" else 0, _capi.tterms_arg(tt)

    def _rollout_times_dev(self, time_vars, method):
        """``(n_ticks, stages, T)`` of a rollout with ``time_on_device``: ``T`` the tick times as a device tensor, from
        which ``clik_*_rollout_batch_dev`` fills the time terms of all stage times itself (a tensor on the controller's
        device is used in place); ``stages`` as ``_rollout_times``."""
        if method not in ("euler", "rk4"):
            raise ValueError("method must be 'euler' or 'rk4'")
        T = self._device_times(time_vars)[0]
        return int(T.numel()), 1 if method == "rk4" else 0, T

    def _rollout_io(self, robot_var, virtual_var, input_var, n_ticks, record_every, record_out, fields):
        """The marshalling of a rollout: ``(Q, X, Y, B, was_np, y_per_tick, rec)``.  ``Q`` / ``X`` are copies the
        launch overwrites with the final state.  ``input_var`` may be ``[n_ticks, B, n_y]`` - one target per tick,
        ``y_per_tick`` is then 1 and ``Y`` that whole tensor - or what it was before.  ``rec``: None without
        ``record_every``, else the dict of ``[R, B, .]`` record tensors (``record_layout`` of ``fields``) on the device -
        those of ``record_out`` (validated with ``check_out_tensor``; every key must be a field) and new ones for the
        rest."""
        torch = _torch()
        d, dev = self.descriptor, self._device
        R = rollout_records(n_ticks, record_every)
        y_per_tick = 1 if d.n_y > 0 and per_tick_input(input_var, n_ticks, d.n_y) else 0
        Y3 = None
        if y_per_tick:
            if isinstance(input_var, torch.Tensor):
                Y3 = input_var.to(device=dev, dtype=torch.float64).contiguous()
            else:
                Y3 = torch.from_numpy(np.ascontiguousarray(np.asarray(input_var, dtype=np.float64))).to(dev)
            input_var = Y3[0] if n_ticks > 0 else None
        Q, X, Y, B, was_np = self._batch_inputs(robot_var, virtual_var, input_var, clone=True)
        if Y3 is not None:
            Y = Y3
        rec = None
        if R is not None:
            rec = {}
            given = dict(record_out or {})
            for name, (shape, dtype) in record_layout(fields, R, B).items():
                t = given.pop(name, None)
                check_out_tensor(t, shape, dtype, dev, "record_out[%r]" % name)
                rec[name] = t if t is not None else torch.empty(shape, dtype=getattr(torch, dtype), device=dev)
            if given:
                raise ValueError("record_out has no field(s) %s for this skill" % ", ".join(sorted(map(repr, given))))
        elif record_out:
            raise ValueError("record_out needs record_every")
        return Q, X, Y, B, was_np, y_per_tick, rec

    def _rollout_result(self, outs, rec, was_np, summ=None):
        """What a rollout returns: ``outs`` in the caller's container type, then - when recording - the dict of records
        and - with ``summary=True`` - the dict of summaries, each as one more, last element."""
        res = tuple(self._to_caller(outs, was_np))
        for extra in (rec, summ):
            if extra is not None:
                res += ({k: (v.cpu().numpy() if was_np else v) for k, v in extra.items()},)
        return res

    def _summary_out(self, tol, B):
        """``(tol on the device | None, dict of the [B, M_tot] output tensors)`` of ``constraint_summary_batch`` and of a
        summarising rollout; ``tol`` as ``summary_tolerances`` returns it (``settled_at`` only with a tolerance)."""
        torch = _torch()
        dev = self._device
        m_tot = sum(int(t["m"]) for t in self.descriptor.tasks)
        tol_dev = None if tol is None else torch.from_numpy(tol).to(dev)
        f64 = lambda: torch.empty((B, m_tot), dtype=torch.float64, device=dev)      # noqa: E731
        i32 = lambda: torch.empty((B, m_tot), dtype=torch.int32, device=dev)        # noqa: E731
        out = {"abs_max": f64(), "abs_max_at": i32(), "last": f64(), "rms": f64(), "viol_max": f64(), "viol_count": i32()}
        if tol_dev is not None:
            out["settled_at"] = i32()
        return tol_dev, out

    @staticmethod
    def _summary_ptrs(tol_dev, out):
        """tol and the seven outputs as ``clik_*_constraint_summary`` and ``clik_*_rollout_batch_sum`` take them"""
        return (ptr(tol_dev), ptr(out["abs_max"]), ptr(out["abs_max_at"]), ptr(out["last"]), ptr(out["rms"]),
                ptr(out["viol_max"]), ptr(out["viol_count"]), ptr(out.get("settled_at")))

    def rollout_batch(self, time_vars, robot_var, input_var=None, dt=0.008, max_speed=0.0, virtual_var=None,
                      method="euler", record_every=None, record_out=None, summary=False, summary_tol=None):
        """``len(time_vars)`` ticks of solve -> clamp(+-max_speed) -> integrate in one launch, the host loop of
        ur5_moe2016_example2.ipynb:537-545 (ReactiveQPController: the working set hot-started from tick to tick).
        ``method="euler"``: ``q += dq*dt``; ``method="rk4"``: classical Runge-Kutta with the controller as the right-hand
        side (casclik/integration_methods.py:17-23: k1..k4 at t, t+dt/2, t+dt/2, t+dt, each clamped).

        Returns ``(q_final, dq_last, mode_last)`` (PseudoInverseController) or ``(q_final, dq_last, slack_last | None,
        status [B])`` (ReactiveQPController: ``status`` is the worst status met so far, and an infeasible tick leaves the
        state where it was).  For a skill with virtual variables (path following, cart_on_track_1D...ipynb cell 60: pass
        ``virtual_var``) the path parameters are integrated alongside, unclamped, and the result is ``(q_final, x_final,
        dq_last, dx_last, mode_last)`` or ``(q_final, x_final, dq_last, dx_last, slack_last | None, status)``.

        Trajectory in: ``input_var`` may be ``[n_ticks, B, n_y]``, tick i then reads record i (``"rk4"``: all four
        stages of the tick).  Trajectory out: ``record_every=k`` appends one last element to the result, a dict of
        ``[n_ticks // k, B, .]`` arrays ``q``, ``dq`` (``x``, ``dx`` with virtual variables) and ``mode [R, B]``
        (ReactiveQPController: ``slack`` when the skill has slack, and ``status [R, B]``, the worst status up to and
        including that tick): entry r is what a launch ending at tick ``(r + 1) * k`` returns.  ``record_out``:
        preallocated device tensors for some of them.  Both need a kernel instantiated for the skill
        (NotImplementedError otherwise).

        Summary: ``summary=True`` appends one more, last element (behind the records when ``record_every`` is given as
        well): the dict ``constraint_summary_batch`` returns - ``abs_max``, ``abs_max_at``, ``last``, ``rms``,
        ``viol_max``, ``viol_count`` and, with ``summary_tol`` (a scalar or ``[M_tot]`` values, finite and >= 0),
        ``settled_at``; ``[B, M_tot]`` each, rows as ``constraint_rows()`` - computed inside the rollout, with no record
        of the trajectory.  Record r = 0 .. n_ticks - 1 is what tick r acts on: ``time_vars[r]``, the state the tick
        starts from (record 0: ``robot_var``) and the target it reads; with ``"rk4"`` the tick's first stage.  The state
        after the last tick is not a record (``constraint_values_batch`` on ``q_final`` gives its e); a tick of the
        ReactiveQPController that is infeasible leaves the state where it was, and the next record is that same state.
        It is what ``constraint_summary_batch(time_vars, concat(q_0, rec["q"][:-1]), ...)`` gives on the records of the
        same launch with ``record_every=1``, the same bits on every call and in every batch.  Such a launch uses the
        lane-per-instance kernel at every batch size.  ValueError for ``summary_tol`` without ``summary``, a bad
        ``summary_tol`` and an empty ``time_vars``; NotImplementedError when no kernel could be instantiated for the
        skill, when its block does not fit the LDS of a compute unit or when its kernel would spill.

        With ``options["time_on_device"]`` the launch goes through ``clik_*_rollout_batch_dev``: the time terms of all
        ticks and stages are computed on the device from ``time_vars``, which may be a tensor on the controller's
        device (used in place, no host synchronisation).

        With ``options["velocity_feedback"] = fb`` tick k + 1 reads in ``input_var[:, fb[j]]`` the velocity of state j
        that tick k was integrated with - what record k of ``record_every=1`` holds in ``dq`` / ``dx``: after the clamp,
        with ``"rk4"`` the combined rate, read by all four stages - and tick 0 what the caller gave; a NaN is fed like
        any other value.  With a 3-D ``input_var`` tick i takes its other entries from record i, and the fed entries of
        the records ``i >= 1`` are ignored.  A launch of ``n1 + n2`` ticks is a launch of ``n1`` followed by one of
        ``n2`` whose fed entries are the first one's ``dq`` / ``dx``.  Such a launch uses the lane-per-instance kernel
        at every batch size; NotImplementedError for a handle that only the built-in kernels serve."""
        self._require_handle()
        torch = _torch()
        d, dev = self.descriptor, self._device
        dev_times = self._time_kernel is not None
        if dev_times:
            n_ticks, stages, tt = self._rollout_times_dev(time_vars, method)
            ttp = ptr(tt)
        else:
            n_ticks, stages, (tt, ttp) = self._rollout_times(time_vars, dt, method)
        want_sum, tol = rollout_summary_request(summary, summary_tol, n_ticks, sum(int(t["m"]) for t in d.tasks))
        tail = self._tail()
        Q, X, Y, B, was_np, y_per_tick, rec = self._rollout_io(
            robot_var, virtual_var, input_var, n_ticks, record_every, record_out,
            [("q", d.n_q, "float64"), ("dq", d.n_q, "float64"), ("x", d.n_x, "float64"), ("dx", d.n_x, "float64")] + tail)
        dQ, dX, *last = self._batch_outputs(B)
        args = (self._handle, B, n_ticks, stages, float(dt), float(max_speed), ttp,
                ptr(Q), ptr(X), ptr(Y), ptr(dQ), ptr(dX), *map(ptr, last), current_stream(dev))
        # (without records or per-tick targets: 0, 0 and NULL for every record)
        r = rec or {}
        every = int(record_every or 0)
        if self._feedback is not None and dev_times and not every and not y_per_tick:
            # (clik_*_rollout_batch_dev hands a launch without records and per-tick targets to the plain kernels, which
            # feed nothing: ask for a record behind the last tick - none is written, and the recording lane kernel runs)
            every = n_ticks + 1
        rec_args = (y_per_tick, every) + tuple(
            ptr(r.get(name)) for name in ["q", "dq", "x", "dx"] + [name for name, _, _ in tail])
        entry = lambda suffix: getattr(self._lib, "clik_%s_rollout_batch_%s" % (self._kind, suffix))     # noqa: E731
        summ = None
        # (with the velocity feedback every launch is the recording lane kernel's, with or without records)
        plain = rec is None and not y_per_tick and self._feedback is None
        if want_sum:
            # (records, per-tick targets and the summary in ONE launch of the summarising lane kernel)
            tol_dev, summ = self._summary_out(tol, B)
            self._require_kernel("rollsum")
        elif not plain:
            self._require_kernel("rec")
        with torch.cuda.device(dev):
            if want_sum:
                # (here the host table and the device times are two arguments, and exactly one of them is given)
                rc = entry("sum")(*args[:6], None if dev_times else ttp, *args[7:], *rec_args,
                                  ttp if dev_times else None, *self._summary_ptrs(tol_dev, summ))
            elif plain and not dev_times:
                rc = entry("m")(*args)
            else:
                rc = entry("dev" if dev_times else "rec")(*args, *rec_args)
        _capi.check(self._lib, rc)
        outs = (Q, dQ, *last) if X is None else (Q, X, dQ, dX, *last)
        return self._rollout_result(outs, rec, was_np, summ)

    # -- constraint values over a trajectory --------------------------------------------------------------------
    def constraint_rows(self):
        """Ordered dict ``label -> slice`` into the ``M_tot`` rows ``constraint_values_batch`` returns: the rows of
        the skill's constraints in skill order.  Known after set-up (RuntimeError before), without a GPU call."""
        if getattr(self, "descriptor", None) is None or getattr(self, "_handle", None) is None:
            raise RuntimeError("call setup_problem_functions() / setup_solver() first")
        return constraint_row_slices(self.descriptor)

    def _trajectory_tensor(self, val, width, what, lead=None, shared=False):
        """``(T [R, B, width], ndim, was_np)`` of one argument of ``constraint_values_batch``: contiguous float64 on the
        controller's device; a tensor that already is that is used in place (the records of a rollout go in as they
        are).  A ``[B, width]`` matrix is one record (``T [1, B, width]``, ``ndim`` 2); with ``lead = (R, B)`` of
        ``robot_var`` and R > 1 it is accepted only where one block may serve all records (``shared``)."""
        torch = _torch()
        val, ndim = trajectory_rows(val, width, what, lead)
        if ndim == 2:
            t, was_np = to_device_matrix(val, width, self._device, what, None if lead is None else lead[1])
            if lead is not None and lead[0] != 1 and not shared:
                raise ValueError("%s must be [R, B, %d] like robot_var (%d records), got shape %s"
                                 % (what, width, lead[0], tuple(t.shape)))
            return t.unsqueeze(0), 2, was_np
        if isinstance(val, torch.Tensor):
            return val.to(device=self._device, dtype=torch.float64).contiguous(), 3, False
        return torch.from_numpy(np.ascontiguousarray(np.asarray(val, dtype=np.float64))).to(self._device), 3, True

    def _trajectory_inputs(self, robot_var, virtual_var, input_var):
        """What ``constraint_values_batch`` and ``constraint_summary_batch`` open with: ``(Q [R, B, n_q], X | None, Y |
        None, y_stride, R, B, ndim, was_np)`` - the states as ``_trajectory_tensor`` gives them, ``y_stride`` the record
        stride of ``Y`` (0: one block shared by all records), ``ndim`` and ``was_np`` those of ``robot_var``."""
        d = self.descriptor
        Q, ndim, was_np = self._trajectory_tensor(robot_var, d.n_q, "robot_var")
        R, B = int(Q.shape[0]), int(Q.shape[1])
        X = Y = None
        y_stride = 0
        if d.n_x > 0:
            if virtual_var is None:
                raise ValueError("skill has virtual_var: pass virtual_var")
            X = self._trajectory_tensor(virtual_var, d.n_x, "virtual_var", (R, B))[0]
        if d.n_y > 0:
            if input_var is None:
                raise ValueError("skill has input_var: pass input_var")
            Y, y_ndim, _ = self._trajectory_tensor(input_var, d.n_y, "input_var", (R, B), shared=True)
            y_stride = B * d.n_y if y_ndim == 3 else 0
        return Q, X, Y, y_stride, R, B, ndim, was_np

    def _monitor_time_table(self, time_var, R, B, ndim):
        """``(T | None, tt_rec_stride, tt_inst_stride)`` of a ``constraint_values_batch`` call: the device table of
        time terms and how row (r, b) finds its record in it.  One stamp: strides 0 / 0; ``[R]`` stamps with a 3-D
        ``robot_var``: one record each; ``[B]`` stamps with a 2-D ``robot_var``: one per instance.  The table comes from
        ``descriptor.time_terms`` per distinct stamp, uploaded once - or, with ``options["time_on_device"]``, from
        ``time_terms_batch`` (a device tensor of times is then read in place, nothing on the host)."""
        torch = _torch()
        d = self.descriptor
        is_tensor = isinstance(time_var, torch.Tensor)
        n = int(time_var.numel()) if is_tensor else int(np.size(time_var))
        if n == 0:
            raise ValueError("time_var is empty")
        many = n > 1
        if many:
            want = R if ndim == 3 else B
            if n != want:
                raise ValueError("time_var has %d entries, the trajectory %d %s" % (
                    n, want, "record(s) (robot_var [R, B, n_q])" if ndim == 3 else "instance(s) (robot_var [B, n_q])"))
        if d.n_tslots == 0:
            return None, 0, 0
        w = 2 * d.n_tslots
        if self._time_kernel is not None:
            T = self.time_terms_batch(self._device_times(time_var)[0])
        else:
            times = (time_var.detach().cpu().numpy() if is_tensor else np.asarray(time_var, dtype=float)).reshape(-1)
            uniq, inverse = np.unique(times.astype(float), return_inverse=True)
            terms = np.stack([d.time_terms(float(tv)) for tv in uniq])
            T = torch.from_numpy(np.ascontiguousarray(terms[inverse.reshape(-1)])).to(self._device)
        if not many:
            return T, 0, 0
        return (T, w, 0) if ndim == 3 else (T, 0, w)

    def constraint_values_batch(self, time_var, robot_var, virtual_var=None, input_var=None, jacobian=False, out=None):
        """The values of the skill's constraint expressions over a batch or a whole trajectory of states, in ONE launch
        of a kernel of its own: what the notebooks of the reference get from ``cnstr.eval(t, q)`` once per tick.

        ``robot_var``: ``[B, n_q]`` or ``[R, B, n_q]`` (numpy or device tensor; a contiguous float64 tensor on the
        controller's device is read in place, so ``rec["q"]`` of a recording rollout goes in directly);
        ``virtual_var``: the same leading shape; ``input_var``: ``[B, n_y]`` (shared by all records) or
        ``[R, B, n_y]``.  ``time_var``: one stamp, ``[R]`` stamps with a 3-D ``robot_var`` (one per record) or ``[B]``
        with a 2-D one (one per instance, as ``solve_batch``).  With ``options["time_on_device"]`` the time terms come
        from the time kernel and ``time_var`` may be a device tensor (no host synchronisation).

        Returns ``e [..., M_tot]``, or with ``jacobian=True`` ``(e, J [..., M_tot, n_q + n_x], e_t [..., M_tot])``:
        the rows of all constraints in skill order (``constraint_rows()``), the Velocity*Constraints included, ``J``
        the derivative with respect to (robot_var, virtual_var), ``e_t`` the partial derivative in time.  Numpy when
        ``robot_var`` is numpy, device tensors otherwise.  ``out``: a preallocated device tensor for ``e``, filled in place
        and returned - with a numpy ``robot_var`` it is still filled, and a numpy copy of it is returned.  The launch
        goes on torch's current stream.  NotImplementedError when no kernel could be instantiated for the skill."""
        self._require_handle()
        torch = _torch()
        d, dev = self.descriptor, self._device
        Q, X, Y, y_stride, R, B, ndim, was_np = self._trajectory_inputs(robot_var, virtual_var, input_var)
        T, tt_rec, tt_inst = self._monitor_time_table(time_var, R, B, ndim)
        m_tot, n = sum(int(t["m"]) for t in d.tasks), d.n_q + d.n_x
        lead = (R, B) if ndim == 3 else (B,)
        check_out_tensor(out, lead + (m_tot,), "float64", dev, "out")
        E = out if out is not None else torch.empty(lead + (m_tot,), dtype=torch.float64, device=dev)
        J = torch.empty(lead + (m_tot, n), dtype=torch.float64, device=dev) if jacobian else None
        Et = torch.empty(lead + (m_tot,), dtype=torch.float64, device=dev) if jacobian else None
        self._require_kernel("monitor")
        with torch.cuda.device(dev):
            rc = getattr(self._lib, "clik_%s_constraint_values" % self._kind)(
                self._handle, R, B, ptr(T), tt_rec, tt_inst, ptr(Q), ptr(X), ptr(Y), y_stride, ptr(E), ptr(J), ptr(Et),
                current_stream(dev))
        _capi.check(self._lib, rc)
        if not jacobian:
            return E.cpu().numpy() if was_np else E
        return self._to_caller((E, J, Et), was_np)

    def constraint_values(self, time_var, robot_var, virtual_var=None, input_var=None):
        """One instance, the reference's argument order: dict ``label -> DM [m, 1]``, what the notebooks'
        ``cnstr.eval(t, q)`` returns for each constraint of the skill."""
        from .. import sym as cs
        self._require_handle()
        d = self.descriptor
        q = flat_vector(robot_var, d.n_q, "robot_var").reshape(1, -1)
        x = flat_vector(virtual_var, d.n_x, "virtual_var").reshape(1, -1) if d.n_x > 0 and virtual_var is not None else None
        y = flat_vector(input_var, d.n_y, "input_var").reshape(1, -1) if d.n_y > 0 and input_var is not None else None
        e = self.constraint_values_batch(float(scalar_of(time_var)), q, virtual_var=x, input_var=y)[0]
        return {label: cs.DM(e[sl].reshape(-1, 1)) for label, sl in self.constraint_rows().items()}

    # -- constraint summaries over a trajectory -----------------------------------------------------------------
    def constraint_summary_batch(self, time_var, robot_var, virtual_var=None, input_var=None, tol=None):
        """What the skill's constraint expressions did over a whole trajectory of states, per instance and per
        constraint row: the reduction over the record axis of what ``constraint_values_batch`` returns, done inside the
        kernel that evaluates the constraints - ``e [R, B, M_tot]`` is never stored.

        The arguments are those of ``constraint_values_batch``: ``robot_var`` ``[R, B, n_q]`` (or ``[B, n_q]``: one
        record), ``virtual_var`` the same leading shape, ``input_var`` ``[B, n_y]`` (shared by all records) or
        ``[R, B, n_y]``, ``time_var`` one stamp or ``[R]`` stamps (a device tensor with ``options["time_on_device"]``).
        Device tensors are read in place - ``rec["q"]`` of a recording rollout goes in directly - and the launch goes on
        torch's current stream.

        Returns a dict of ``[B, M_tot]`` arrays, rows as ``constraint_rows()``; numpy when ``robot_var`` is numpy,
        device tensors otherwise.  Over the records r = 0 .. R - 1:

        * ``abs_max`` (float64) max |e[r]|, ``abs_max_at`` (int32) the first r that attains it;
        * ``last`` e[R - 1]; ``rms`` sqrt(mean e[r]^2);
        * ``viol_max`` on the rows of a ``SetConstraint`` max over r of max(set_min - e, e - set_max, 0) and
          ``viol_count`` (int32) the number of records with a violation > 0 - with the bounds the ticks use, expressions
          evaluated at the record's own (t, q, x, y); an infinite bound is "no bound".  0 on the rows of every other
          class (the bounds of a ``VelocitySetConstraint`` apply to a velocity, not to e);
        * ``settled_at`` (int32), only with ``tol`` - a scalar or ``[M_tot]`` values, finite and >= 0 (ValueError
          otherwise): the smallest r such that d[r'] <= tol[row] for all r' >= r, R when the last record is outside; d
          is the violation on ``SetConstraint`` rows and |e| on the others.

        The record axis is reduced in chunks of ``summary_chunk_length(R, B)`` records, combined in order: the result
        is the same bits on every call and for an instance whatever batch it is part of.  A row whose e is non-finite
        at any record reports NaN in ``abs_max``, ``last``, ``rms`` and ``viol_max``; its three integer outputs are
        unspecified; no other instance changes.  NotImplementedError when no kernel could be instantiated for the
        skill: there is no host fallback."""
        self._require_handle()
        torch = _torch()
        dev = self._device
        Q, X, Y, y_stride, R, B, _, was_np = self._trajectory_inputs(robot_var, virtual_var, input_var)
        # (one stamp, or one per record: a [B, n_q] robot_var is one record, not B stamps as in constraint_values_batch)
        T, tt_rec, tt_inst = self._monitor_time_table(time_var, R, B, 3)
        tol_dev, out = self._summary_out(summary_tolerances(tol, sum(int(t["m"]) for t in self.descriptor.tasks)), B)
        self._require_kernel("summary")
        with torch.cuda.device(dev):
            n_work = int(getattr(self._lib, "clik_%s_summary_work_bytes" % self._kind)(self._handle, R, B))
            work = torch.empty(max(n_work, 8) // 8 + 1, dtype=torch.float64, device=dev)
            tol_ptr, *out_ptrs = self._summary_ptrs(tol_dev, out)
            rc = getattr(self._lib, "clik_%s_constraint_summary" % self._kind)(
                self._handle, R, B, ptr(T), tt_rec, tt_inst, ptr(Q), ptr(X), ptr(Y), y_stride, tol_ptr, ptr(work),
                work.numel() * 8, *out_ptrs, current_stream(dev))
        _capi.check(self._lib, rc)
        return {k: v.cpu().numpy() for k, v in out.items()} if was_np else out

    # -- rollouts that run until each instance has converged ------------------------------------------------------
    def converge_batch(self, robot_var, input_var=None, tol=1e-6, max_ticks=1000, dt=0.008, max_speed=0.0,
                       virtual_var=None, time_var=0.0, min_step=0.0, group=1):
        """Closed-loop inverse kinematics for a batch in ONE launch: every instance ticks (solve -> clamp(+-max_speed)
        -> ``q += dq * dt``, explicit Euler) with the time ``time_var`` and its target ``input_var [B, n_y]`` frozen,
        until it has converged or cannot go on; a wave of 64 instances leaves the loop when all of them have stopped.

        Before tick r = 0, 1, ... of an instance every constraint is evaluated at its state: ``dist_i = |e_i|``, on the
        rows of a ``SetConstraint`` the distance outside ``[set_min, set_max]`` (as ``viol_max`` of
        ``constraint_summary_batch``).  The instance stops with ``status``

        * 4 when some ``e_i`` is non-finite;
        * 0 when ``dist_i <= tol_i`` on every row - ``tol`` is a scalar or ``[M_tot]`` values >= 0, rows as
          ``constraint_rows()``; a row with ``tol_i = +inf`` cannot block (give that to the rows of velocity constraints
          and of lower-priority tasks that cannot be met);
        * 1 when r == ``max_ticks``;
        * 3 (ReactiveQPController) when the QP of tick r is infeasible, 2 when ``min_step > 0`` and ``max_j |dq_j| * dt
          <= min_step`` over the robot variables - the state stays as it was in both cases.

        ``group = G`` (2, 4, 8, 16, 32 or 64; ``B`` a multiple of it) adds the group rule: instances ``[g G, (g + 1) G)``
        are one group - the seeds of one target, say - and an instance that is still running behind the test of tick r
        stops there with ``status`` 5 and ``ticks = r`` once an instance of its group has stopped with status 0, at this
        test or an earlier one.  It keeps its state and the ``dist_i`` of that test.  An instance the test itself stops
        at r keeps the status above, and a group none of whose instances reaches status 0 runs as without the rule.
        So a group costs its wave the ticks of its first arrival, not of its slowest member.  The rule is compiled into
        a kernel of its own per ``G``, built at its first use like the default one.

        Returns ``(q, dq, mode, info)``, with virtual variables ``(q, x, dq, dx, mode, info)`` (ReactiveQPController: the
        worst QP status met in place of ``mode``): the state at the stop, the velocity and mode of the last tick that was
        integrated (zeros and -1 when there was none), and ``info = {"ticks": int32 [B], "status": int32 [B], "residual":
        float64 [B, M_tot]}`` - the number of ticks integrated, the status above and the ``dist_i`` of the returned
        state.  For status 4 every component of the instance's rows of ``q``, ``dq`` and ``residual`` is NaN; no other
        instance changes.  Numpy when ``robot_var`` is numpy, device tensors otherwise; the same bits on every call and
        in every batch (with ``group``: in every batch of whole groups).  ValueError for a bad ``tol`` (negative, NaN,
        wrong length), ``max_ticks < 0``, a 3-D ``input_var`` (targets are fixed here), a ``group`` outside 1, 2, 4, 8, 16,
        32, 64 and a ``B`` that is no multiple of it; NotImplementedError when no kernel could be instantiated for the skill,
        when its block does not fit the LDS of a compute unit or when its kernel would spill.

        With ``options["velocity_feedback"]`` a tick that is integrated feeds its velocity to the instance's next tick
        (``rollout_batch`` has the rule); a stopped instance keeps its entries, and a stalled or infeasible tick feeds
        nothing.  ``group`` combines freely with it."""
        self._require_handle()
        torch = _torch()
        d, dev = self.descriptor, self._device
        m_tot = sum(int(t["m"]) for t in d.tasks)
        tol_np, max_ticks = converge_request(tol, max_ticks, min_step, input_var, m_tot)
        Q, X, Y, B, was_np = self._batch_inputs(robot_var, virtual_var, input_var, clone=True)
        if B < 1:
            raise ValueError("converge_batch needs at least one instance")
        group = converge_group_request(group, B)
        # (of the tail only its last output, the one number per instance - the mode, the QP's worst status - is returned:
        # the entry takes it first and NULL for the others, the QP's slack)
        dQ, dX, *unused, mode = self._batch_outputs(B, skip=[name for name, _, _ in self._rollout_tail[:-1]])
        info = {"ticks": torch.empty((B,), dtype=torch.int32, device=dev),
                "status": torch.empty((B,), dtype=torch.int32, device=dev),
                "residual": torch.empty((B, m_tot), dtype=torch.float64, device=dev)}
        tol_dev = torch.from_numpy(tol_np).to(dev)
        tt, ttp = _capi.tterms_arg(d.time_terms(float(scalar_of(time_var))))
        self._require_converge_kernel(group)
        with torch.cuda.device(dev):
            rc = getattr(self._lib, "clik_%s_converge_batch" % self._kind)(
                self._handle, B, max_ticks, float(dt), float(max_speed), float(min_step), ttp, ptr(Q), ptr(X), ptr(Y),
                ptr(dQ), ptr(dX), ptr(mode), *map(ptr, unused), ptr(tol_dev), ptr(info["ticks"]), ptr(info["status"]),
                ptr(info["residual"]), current_stream(dev))
        _capi.check(self._lib, rc)
        outs = (Q, X, dQ, dX, mode) if d.n_x > 0 else (Q, dQ, mode)
        return self._rollout_result(outs, info, was_np)

    def ik_batch(self, input_var, seeds, first_hit=False, **converge_kwargs):
        """Multi-seed inverse kinematics: ``T`` targets ``input_var [T, n_y]``, each started from ``S`` seeds - ``seeds
        [S, n_q]`` shared by all targets or ``[T, S, n_q]`` - in ONE ``converge_batch`` launch of ``T * S`` instances
        (instance ``t * S + s``); ``converge_kwargs`` are its other arguments.  Returns ``(q [T, n_q], info)``: per
        target the state and ``converge_batch``'s info of the seed ``select_seeds`` picks, and ``info["seed"]`` (int32
        ``[T]``) which one that was.  Numpy when ``seeds`` is numpy, device tensors otherwise.  For skills without
        virtual variables (ValueError otherwise).

        ``first_hit=True``: a target's first converged seed stops its other seeds (``converge_batch``'s ``group``), so
        a target costs its wave the ticks of its best seed instead of ``max_ticks`` whenever one seed stalls.  The seeds
        are padded to the next power of two ``P`` with copies of seed 0 and the launch has ``T * P`` instances in groups
        of ``P``; at most 64 seeds (ValueError otherwise).  The seed picked and everything returned for it are what
        ``first_hit=False`` returns: the seeds ``select_seeds`` can pick stop before the rule touches them, a stopped
        seed (status 5) never wins against a converged one, and a copy of seed 0 ties with seed 0 and loses to its
        lower index.  (The grouped kernel is another compilation of the same tick: the same integers, floats that agree
        to rounding.)"""
        self._require_handle()
        torch = _torch()
        d, dev = self.descriptor, self._device
        if d.n_x > 0 or "virtual_var" in converge_kwargs:
            raise ValueError("ik_batch serves skills without virtual variables")
        if "robot_var" in converge_kwargs:
            raise ValueError("ik_batch starts from seeds, not from robot_var")
        if first_hit and "group" in converge_kwargs:
            raise ValueError("first_hit chooses the group itself (the padded number of seeds): do not pass group")
        was_np = not isinstance(seeds, torch.Tensor)
        sd = (seeds if not was_np else torch.from_numpy(np.ascontiguousarray(np.asarray(seeds, dtype=np.float64)))).to(
            device=dev, dtype=torch.float64)
        Y, _ = to_device_matrix(input_var, d.n_y, dev, "input_var")
        T = Y.shape[0]
        if sd.dim() == 2 and sd.shape[1] == d.n_q:
            sd = sd.unsqueeze(0).expand(T, -1, -1)
        if sd.dim() != 3 or sd.shape[0] != T or sd.shape[2] != d.n_q or sd.shape[1] < 1:
            raise ValueError("seeds must be [S, %d] or [%d, S, %d], got shape %s" % (d.n_q, T, d.n_q, tuple(sd.shape)))
        S = n_seeds = sd.shape[1]
        if first_hit:
            S = padded_seeds(n_seeds)
            if S > n_seeds:
                sd = torch.cat([sd, sd[:, :1].expand(T, S - n_seeds, d.n_q)], dim=1)
            converge_kwargs = dict(converge_kwargs, group=S)
        Q0 = sd.reshape(T * S, d.n_q).contiguous()
        Ys = Y.unsqueeze(1).expand(T, S, d.n_y).reshape(T * S, d.n_y).contiguous()
        tol = converge_kwargs.get("tol", 1e-6)
        q, _, _, info = self.converge_batch(Q0, Ys, **converge_kwargs)
        m_tot = info["residual"].shape[1]
        pick = select_seeds(info["ticks"], info["status"], info["residual"], converge_tolerances(tol, m_tot), S)
        if S > n_seeds:
            assert bool((pick < n_seeds).all()), "a copy of seed 0 was picked ahead of seed 0"
        at = torch.arange(T, device=dev) * S + pick
        out = {k: v.index_select(0, at) for k, v in info.items()}
        out["seed"] = pick.to(torch.int32)
        res = q.index_select(0, at)
        if was_np:
            return res.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}
        return res, out

    # -- resident ticks -----------------------------------------------------------------------------------------
    def _resident_inputs(self, robot_var, input_var, D):
        """``(Q, Y | None, B, lead)`` of a resident launch: ``robot_var`` / ``input_var`` are read in place by a kernel
        that stays, so each must be a contiguous float64 device tensor ``[B, n]``, with ``ring_depth`` D > 1 a ring
        ``[D, B, n]`` (``lead = (D,)``).  The batch size is ``robot_var``'s and ``input_var`` must have THAT many rows -
        the kernel reads ``y[row * n_y + ...]`` for every row of ``robot_var`` -; a tensor of the wrong rank is a
        ValueError, not an IndexError.  A skill without ``input_var`` ignores what is passed for it."""
        torch = _torch()
        d = self.descriptor
        B = None
        lead = (D,) if D > 1 else ()
        for name, tns, n in (("robot_var", robot_var, d.n_q), ("input_var", input_var, d.n_y)):
            if n == 0:
                continue
            if not isinstance(tns, torch.Tensor) or not tns.is_cuda or tns.dtype != torch.float64 or not tns.is_contiguous():
                raise ValueError("resident ticks: %s must be a contiguous float64 device tensor (read in place)" % name)
            if tns.dim() != len(lead) + 2:
                raise ValueError("resident ticks with ring_depth %d: %s must have %d dimensions %s, got shape %s"
                                 % (D, name, len(lead) + 2, "[D, B, n]" if D > 1 else "[B, n]", list(tns.shape)))
            if B is None:
                B = int(tns.shape[-2])
            want = lead + (B, n)
            if tuple(tns.shape) != tuple(want):
                raise ValueError("resident ticks with ring_depth %d: %s must have shape %s, got %s"
                                 % (D, name, list(want), list(tns.shape)))
        return robot_var, (input_var if d.n_y > 0 else None), B, lead

    def _resident_run(self, entry, robot_var, input_var, D, n_ticks, time_var, timeout_s, stream, publish_ahead,
                      given=None, extra=()):
        """The body of ``resident_start``: check the inputs (``_resident_inputs``), make the outputs - zeros, -1 for the
        int32 ones, or the caller's ``given`` as they are (``_batch_outputs``) -, set the run up (``_resident_setup``)
        and launch ``entry(handle, B, n_ticks, time terms, q, y, dq, *tail, ticket, done, *extra, timeout_s, stream)``.
        Returns the dict of the run: ``ticket``, ``done``, ``waves``, ``out``, each output of ``_rollout_tail`` under
        its name, ``stream`` and ``keep`` (what must outlive the kernel)."""
        Q, Y, B, lead = self._resident_inputs(robot_var, input_var, D)
        dQ, _, *tail = self._batch_outputs(B, lead, given, skip=("dx",), init=True)
        waves = getattr(self._lib, "clik_%s_resident_waves" % self._kind)(self._handle, B)
        ticket, done, stream, (tt, ttp) = self._resident_setup(waves, D, publish_ahead, stream, time_var)
        with _torch().cuda.device(self._device):
            rc = getattr(self._lib, entry)(self._handle, B, int(n_ticks), ttp, ptr(Q), ptr(Y), ptr(dQ), *map(ptr, tail),
                                           ptr(ticket), ptr(done), *extra, float(timeout_s),
                                           C.c_void_p(stream.cuda_stream))
        _capi.check(self._lib, rc)
        run = {"ticket": ticket, "done": done, "waves": waves, "out": dQ, "stream": stream, "keep": (Q, Y, tt)}
        run.update(zip((name for name, _, _ in self._rollout_tail), tail))
        return run

    def _resident_setup(self, waves, ring_depth, publish_ahead, stream, time_var):
        """What a resident launch needs beside its tensors: the ``ticket`` (64 int32 words: [0] in_seq, [16] ring
        depth, [32] stop, [48] waves, [49] ticks_done), one ``done`` slot per wave, the launch stream (a new one by
        default) and the time terms.  Returns once they, and the outputs the caller initialised on the current stream,
        are in place."""
        torch = _torch()
        dev = self._device
        ticket = torch.zeros(64, dtype=torch.int32, device=dev)
        ticket[16] = ring_depth if ring_depth > 1 else 0
        if publish_ahead:
            # tickets 1 .. publish_ahead are valid before the kernel starts (the inputs of those ticks are in place):
            # no producer has to run next to it - what a profiler that serialises kernels needs
            ticket[0] = int(publish_ahead)
        done = torch.zeros(max(waves, 1), dtype=torch.int32, device=dev)
        stream = stream if stream is not None else torch.cuda.Stream(device=dev)
        tterms = _capi.tterms_arg(self.descriptor.time_terms(time_var))
        torch.cuda.current_stream(dev).synchronize()       # (ticket / outputs are initialised before the kernel starts)
        return ticket, done, stream, tterms

    def resident_wait(self, run):
        """Wait for a resident run to leave; ticks finished, or ``ResidentWatchdog`` (``base_controller.resident_wait``)."""
        return resident_wait(run)

    def resident_feed_stream(self):
        """A stream for whoever feeds a resident run that is ALREADY launched (copies, producer kernels): one whose work
        makes progress beside the resident kernel (``base_controller.free_stream``; the runtime may have put a new stream
        onto the resident kernel's hardware queue, where it would wait for the kernel's watchdog)."""
        return free_stream(self._device)

    def resident_feed(self, run, n_ticks, closed_loop=False, timeout_s=2.0, stream=None):
        """The reference producer of resident ticks (clik_ticket_feed): one device thread that publishes tickets
        1 .. n_ticks on ``stream`` (by default one that makes progress beside the kernel, ``resident_feed_stream``),
        back to back or - ``closed_loop`` - each only after every wave has finished the previous tick."""
        dev = self._device
        stream = stream if stream is not None else free_stream(dev)
        with _torch().cuda.device(dev):
            rc = self._lib.clik_ticket_feed(ptr(run["ticket"]), ptr(run["done"]), int(n_ticks), 1 if closed_loop else 0,
                                            int(run["waves"]), float(timeout_s), C.c_void_p(stream.cuda_stream))
        _capi.check(self._lib, rc)
        return stream

    # -- solve() ------------------------------------------------------------------------------------------------
    def _stage_solve(self, robot_var, virtual_var, input_var):
        """The inputs of a single-instance ``solve()`` into the persistent ``SingleSlot`` (made at the first call, with
        room for the ``(doubles, int32)`` of results the controller's ``_slot_results()`` asks for): returns the slot
        and the pointers of q, x, y as the launch takes them (None for a block the skill does not have).  The
        reference forwards ``virtual_var`` / ``input_var`` only when they are used (pseudo_inverse.py:521-525); the
        device descriptor always carries the full vectors, so a missing one is zeros."""
        spec = self.skill_spec
        q = flat_vector(robot_var, spec.n_robot_var, "robot_var")
        x = y = None
        if spec.n_virtual_var > 0:
            x = flat_vector(virtual_var if virtual_var is not None
                            else np.zeros(spec.n_virtual_var), spec.n_virtual_var, "virtual_var")
        if spec.n_input_var > 0:
            y = flat_vector(input_var if input_var is not None
                            else np.zeros(spec.n_input_var), spec.n_input_var, "input_var")
        if self._handle is None:        # (inline: this runs on every solve())
            self._require_handle()
        d = self.descriptor
        nq, nx, ny = d.n_q, d.n_x, d.n_y
        slot = getattr(self, "_slot", None)
        if slot is None:
            slot = self._slot = SingleSlot(self._device, nq + nx + ny, *self._slot_results())
            # where the launch writes dq, dx and the tail, in that order: the doubles one after the other, then the int32
            ptrs, at, n_int = [], 0, 0
            for _, width, dtype in [("out", nq, "float64"), ("dx", nx, "float64")] + self._tail():
                if dtype == "int32":
                    ptrs.append(slot.int_ptr(n_int))
                    n_int += 1
                else:
                    ptrs.append(slot.out_ptr(at) if width else None)
                    at += width
            slot.result_ptrs = tuple(ptrs)
        slot.in_np[:nq] = q
        if nx:
            slot.in_np[nq:nq + nx] = x
        if ny:
            slot.in_np[nq + nx:nq + nx + ny] = y
        return slot, slot.in_ptr(0), slot.in_ptr(nq) if nx else None, slot.in_ptr(nq + nx) if ny else None

    def _solve_slot(self, time_var, robot_var, virtual_var, input_var, extra=None):
        """The launch of a single-instance ``solve()``: B = 1 through the persistent pinned / device staging (one copy
        each way), ``_tick_fn`` with the results written into the slot at ``slot.result_ptrs`` and the controller's
        extra launch arguments ``extra(slot)``.  Returns the slot once its results are on the host: the doubles in
        ``slot.out_f`` (dq, dx, then the tail's), the int32 in ``slot.out_i``."""
        slot, pq, px, py = self._stage_solve(robot_var, virtual_var, input_var)
        tt, ttp = _capi.tterms_arg(self.descriptor.time_terms(float(scalar_of(time_var))))
        with slot.guard():
            stream = slot.begin()
            rc = getattr(self._lib, self._tick_fn)(self._handle, 1, ttp, pq, px, py, *slot.result_ptrs,
                                                   *(extra(slot) if extra else ()), stream)
            _capi.check(self._lib, rc)
            slot.download()
        return slot
