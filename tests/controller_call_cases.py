"""The calls of the controllers' per-tick surface - ``solve_batch``, ``bind_batch``, ``resident_start`` and ``solve`` of
both controllers - whose answers are recorded on one commit and replayed on a later one: what an accepted call returns
(containers, shapes, dtypes, which tensors are the caller's own, integer results and the size of the float ones) and
what a refused call raises (type and message).

tools/record_controller_calls.py writes the recording to tests/golden/controller_calls.json, run on the commit BEFORE a
change of the Python controllers; tests/test_gpu_controller_calls.py replays the same list.  Every skill here is one an
existing GPU test sets up, so no kernel is instantiated that the suite does not already ask for."""
import contextlib
import os

import numpy as np

import casclik_amd as cc
from casclik_amd import skills
from casclik_amd import sym as cs

import time_skills

BATCHES = (1, 63, 64, 65)       # a wave boundary on either side
DROP = object()                 # (an argument a case leaves out)


def _path_skill(fk):
    """the path-following skill of test_gpu_branches.py: one virtual variable, no input_var"""
    t, q, s = cs.MX.sym("t"), cs.MX.sym("q", 6), cs.MX.sym("s", 1)
    p = fk["T_fk"](q)[:3, 3]
    p0, d = np.array([0.3, 0.1, 0.4]), np.array([0.2, -0.1, 0.05])
    cons = [cc.EqualityConstraint("follow", p - (p0 + d * s), gain=2.0, priority=1, constraint_type="soft"),
            cc.VelocityEqualityConstraint("progress", s, target=0.05, priority=0),
            cc.SetConstraint("s_range", s, set_min=0.0, set_max=1.0, priority=2)]
    return cc.SkillSpecification("path", t, q, virtual_var=s, constraints=cons)


PINV, QP = cc.PseudoInverseController, cc.ReactiveQPController
# name -> (class, skill, options, environment at set-up, robot); "unset" controllers are never set up
CONTROLLERS = {
    "pinv": (PINV, lambda e: skills.stack_skill(e.iiwa), dict(skills.STACK_OPTIONS), {}, "iiwa"),
    "pinv_fb": (PINV, lambda e: skills.stack_skill(e.iiwa),
                dict(skills.STACK_OPTIONS, velocity_feedback=[0, -1, -1, -1, -1, -1, -1]), {}, "iiwa"),
    "pinv_unset": (PINV, lambda e: skills.stack_skill(e.iiwa), dict(skills.STACK_OPTIONS), None, "iiwa"),
    "qp": (QP, lambda e: skills.qp_skill(e.iiwa), None, {}, "iiwa"),
    "qp_unset": (QP, lambda e: skills.qp_skill(e.iiwa), None, None, "iiwa"),
    "pinv_path": (PINV, lambda e: _path_skill(e.ur5), None, {}, "ur5"),
    "qp_path": (QP, lambda e: _path_skill(e.ur5), None, {}, "ur5"),
    "pinv_track": (PINV, lambda e: time_skills.tracking_spec(e.ur5), None, {}, "ur5"),
    "qp_track": (QP, lambda e: time_skills.track_qp_spec(e.ur5), None, {}, "ur5"),
    "pinv_track_dev": (PINV, lambda e: time_skills.tracking_spec(e.ur5), {"time_on_device": True}, {}, "ur5"),
    "qp_track_dev": (QP, lambda e: time_skills.track_qp_spec(e.ur5), {"time_on_device": True}, {}, "ur5"),
    "pinv_track_dyn": (PINV, lambda e: time_skills.tracking_spec(e.ur5), None, {"CLIK_FORCE_DYNAMIC": "1"}, "ur5"),
    "qp_track_dyn": (QP, lambda e: time_skills.track_qp_spec(e.ur5), None, {"CLIK_FORCE_DYNAMIC": "1"}, "ur5"),
}


@contextlib.contextmanager
def _environ(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Env(object):
    """the controllers of the cases, set up at their first use, and the inputs of a batch"""

    def __init__(self):
        import torch
        self.torch = torch
        self.iiwa, self.ur5 = skills.iiwa(), skills.ur5()
        self._ctrls = {}

    def ctrl(self, name):
        if name not in self._ctrls:
            cls, spec, options, env, _ = CONTROLLERS[name]
            ctrl = cls(skill_spec=spec(self), options=None if options is None else dict(options))
            if env is not None:
                with _environ(env):
                    ctrl.setup_problem_functions()
                    ctrl.setup_solver()
            self._ctrls[name] = ctrl
        return self._ctrls[name]

    def inputs(self, name, B, seed=0):
        """(Q, X | None, Y | None) as numpy"""
        if CONTROLLERS[name][4] == "iiwa":
            Q, Y = skills.synthetic_inputs(self.iiwa, B, seed=seed, distribution="mixed")
            return Q, None, Y
        rng = np.random.default_rng(seed)
        Q = time_skills.UR5_HOME + rng.normal(scale=0.1, size=(B, 6))
        return Q, (rng.uniform(0.1, 0.9, size=(B, 1)) if name.endswith("_path") else None), None

    def conv(self, a, kind):
        """an input in the container of the case: numpy, list, DM column (one instance), device tensor (used in place),
        float32 strided device tensor (converted)"""
        torch = self.torch
        if a is None or a is DROP:
            return a
        if kind == "numpy":
            return a
        if kind == "list":
            return a.tolist()
        if kind == "dm":
            return cs.DM(a[0])
        if kind == "tensor":
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()
        assert kind == "f32s", kind
        return torch.from_numpy(np.asarray(a, dtype=np.float32).T.copy()).cuda().T


def describe(v):
    """the structure of a returned value as JSON: container, shape, dtype; the entries of integer arrays and the sum of
    magnitudes (NaN left out, and counted) of float ones"""
    import torch
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (tuple, list)):
        return {"type": type(v).__name__, "items": [describe(x) for x in v]}
    if isinstance(v, dict):
        return {"type": "dict", "items": {str(k): describe(x) for k, x in sorted(v.items())}}
    if isinstance(v, torch.cuda.Stream):
        return {"type": "stream"}
    if isinstance(v, torch.Tensor):
        out = {"type": "tensor", "device": v.device.type, "dtype": str(v.dtype).replace("torch.", "")}
        arr = v.detach().cpu().numpy()
    elif isinstance(v, np.ndarray):
        out, arr = {"type": "ndarray", "dtype": str(v.dtype)}, v
    elif isinstance(v, cs.DM):
        out, arr = {"type": "DM"}, v.toarray()
    elif isinstance(v, np.generic):
        return describe(v.item())
    else:
        return {"type": type(v).__name__}
    out["shape"] = list(arr.shape)
    if arr.dtype.kind in "iu":
        out["values"] = arr.reshape(-1).tolist()
    else:
        out["abs_sum"] = float(np.nansum(np.abs(arr)))
        out["nan"] = int(np.isnan(arr).sum())
    return out


def _alias(t, named):
    """which of the caller's tensors ``t`` is (same memory), or None"""
    import torch
    if not isinstance(t, torch.Tensor):
        return None
    for name, c in named.items():
        if isinstance(c, torch.Tensor) and c.data_ptr() == t.data_ptr():
            return name
    return None


def _close(a, b):
    """float results equal to rounding (another start of the same minimiser), NaN rows alike"""
    a, b = (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x) for x in (a, b))
    return bool(np.array_equal(np.isnan(a), np.isnan(b))
                and (np.abs(np.nan_to_num(a) - np.nan_to_num(b)) <= 1e-8 * (1.0 + np.abs(np.nan_to_num(b)))).all())


def _value(v, env, B):
    return v(env, B) if callable(v) else v


def _batch_args(env, name, B, kind, seed, kw):
    """robot_var and the keyword arguments of a batch call: the skill's inputs in the container ``kind``, then what the
    case overrides (``DROP`` leaves an argument out, a callable is called with ``(env, B)``)"""
    Q, X, Y = env.inputs(name, B, seed)
    args = {"robot_var": env.conv(Q, kind)}
    if X is not None:
        args["virtual_var"] = env.conv(X, kind)
    if Y is not None:
        args["input_var"] = env.conv(Y, kind)
    args.update({k: _value(v, env, B) for k, v in kw.items()})
    return {k: v for k, v in args.items() if v is not DROP}


def solve_batch_case(name, B, kind="numpy", t=0.0, seed=0, cold=False, **kw):
    def fn(env):
        ctrl = env.ctrl(name)
        args = _batch_args(env, name, B, kind, seed, kw)
        res = ctrl.solve_batch(_value(t, env, B), args.pop("robot_var"), **args)
        env.torch.cuda.synchronize()
        out = {"result": describe(res), "aliases": [_alias(r, args) for r in res]}
        if "hot_set" in args:
            out["hot_set"] = describe(args["hot_set"])
        if cold:        # (the minimiser does not depend on the start: equal to a cold solve of the same batch)
            args.pop("hot_set", None), args.pop("use_hot", None)
            ref = ctrl.solve_batch(_value(t, env, B), env.conv(env.inputs(name, B, seed)[0], kind), **args)
            out["same_as_cold"] = all(r is None or _close(r, c) for r, c in zip(res, ref))
        return out
    return fn


def bind_batch_case(name, B, kind="tensor", times=(0.0,), seed=0, primed=False, cold=False, **kw):
    def fn(env):
        ctrl = env.ctrl(name)
        args = _batch_args(env, name, B, kind, seed, kw)
        Q = args.pop("robot_var")
        tick = ctrl.bind_batch(Q, **args)
        named = dict(args, robot_var=Q)
        out = {"attributes": sorted(vars(tick)), "tensors": [_alias(t, named) for t in tick.tensors]}
        if primed:
            tick.primed = True
        for tv in times:
            tick(tv)
        env.torch.cuda.synchronize()
        out["after"] = {k: describe(v) for k, v in sorted(vars(tick).items()) if k != "primed"}
        out["primed"] = getattr(tick, "primed", None)
        if cold:
            ref = ctrl.solve_batch(times[-1], Q, **{k: v for k, v in args.items() if k in ("virtual_var", "input_var")})
            out["same_as_cold"] = _close(tick.out, ref[0]) and bool((tick.status.cpu().numpy() == np.asarray(
                ref[3].cpu() if hasattr(ref[3], "cpu") else ref[3])).all())
        return out
    return fn


def resident_case(name, B, D=1, n_ticks=2, seed=0, one_d=False, **kw):
    """a resident run of ``n_ticks`` ticks whose tickets are all published before the launch (no producer), waited
    for; with ``n_ticks`` < D the last slots of the rings keep what they started with"""
    def fn(env):
        torch = env.torch
        ctrl = env.ctrl(name)
        Q, _, Y = env.inputs(name, B, seed)
        ring = (lambda a: np.stack([a] * D)) if D > 1 else (lambda a: a[0] if one_d else a)
        args = {"robot_var": env.conv(ring(Q), "tensor"), "input_var": None if Y is None else env.conv(ring(Y), "tensor")}
        args.update({k: _value(v, env, B) for k, v in kw.items()})
        lead = (D,) if D > 1 else ()
        given = {k: v for k, v in args.items() if isinstance(v, torch.Tensor)}
        torch.cuda.synchronize()
        run = ctrl.resident_start(args.pop("robot_var"), args.pop("input_var"), n_ticks, timeout_s=2.0,
                                  ring_depth=D, publish_ahead=n_ticks, **args)
        ticks = ctrl.resident_wait(run)
        torch.cuda.synchronize()
        out = {"keys": sorted(run), "ticks": ticks, "waves": run["waves"], "lead": list(lead),
               "outputs": {k: describe(v) for k, v in sorted(run.items()) if k not in ("ticket", "done", "keep", "stream", "waves")},
               "aliases": {k: _alias(v, given) for k, v in sorted(run.items()) if isinstance(v, torch.Tensor)},
               "ticket": describe(run["ticket"][[0, 16, 32, 48, 49]]), "done": describe(run["done"])}
        if n_ticks < D:
            out["untouched"] = {k: describe(v[n_ticks:]) for k, v in sorted(run.items())
                                if isinstance(v, torch.Tensor) and k not in ("ticket", "done")}
        return out
    return fn


def resident_refusal(name, B=64, D=1, **kw):
    """``resident_start`` with what the case overrides; it raises before anything is launched"""
    def fn(env):
        ctrl = env.ctrl(name)
        Q, _, Y = env.inputs(name, B, 0)
        ring = (lambda a: np.stack([a] * D)) if D > 1 else (lambda a: a)
        args = {"robot_var": env.conv(ring(Q), "tensor"), "input_var": None if Y is None else env.conv(ring(Y), "tensor"),
                "ring_depth": D}
        args.update({k: _value(v, env, B) for k, v in kw.items()})
        ctrl.resident_start(args.pop("robot_var"), args.pop("input_var"), 2, timeout_s=1.0, publish_ahead=2, **args)
        raise AssertionError("the call was accepted")
    return fn


def solve_case(name, kind="numpy", t=0.0, calls=1, seed=0, x=None):
    def fn(env):
        ctrl = env.ctrl(name)
        Q, X, Y = env.inputs(name, 4, seed)
        one = {"numpy": lambda a: a[0], "list": lambda a: a[0].tolist(), "dm": lambda a: cs.DM(a[0])}[kind]
        kw = {}
        if X is not None:
            kw["virtual_var"] = one(X if x is None else np.full_like(X, x))
        if Y is not None:
            kw["input_var"] = one(Y)
        for _ in range(calls):
            res = ctrl.solve(t, one(Q), **kw)
        out = {"result": describe(res)}
        for attr in ("current_mode", "_slot_calls"):
            if hasattr(ctrl, attr):
                out[attr] = describe(getattr(ctrl, attr))
        if hasattr(ctrl, "res"):
            out["res"] = describe(ctrl.res)
        return out
    return fn


# ---- tensors of the cases ------------------------------------------------------------------------------------------
def _dev(shape, dtype="float64", fill=None):
    def make(env, B):
        torch = env.torch
        shp = tuple(B if s == "B" else s for s in shape)
        if fill is None:
            return torch.empty(shp, dtype=getattr(torch, dtype), device="cuda")
        return torch.full(shp, fill, dtype=getattr(torch, dtype), device="cuda")
    return make


def _host(shape, dtype="float64"):
    return lambda env, B: env.torch.zeros(tuple(B if s == "B" else s for s in shape), dtype=getattr(env.torch, dtype))


def _strided(shape, dtype="float64"):
    """a transposed view: the right shape, not contiguous"""
    return lambda env, B: env.torch.zeros(tuple(B if s == "B" else s for s in shape)[::-1], dtype=getattr(env.torch, dtype),
                                          device="cuda").permute(*range(len(shape) - 1, -1, -1))


def _junk_sets(env, B):
    return env.torch.from_numpy(np.random.default_rng(1).integers(-2**31, 2**31 - 1, size=B).astype(np.int32)).cuda()


def _stamps(env, B):
    return np.array([0.0, 1.5, 4.0])[np.random.default_rng(12).integers(0, 3, size=B)]


def _stamps_dev(env, B):
    return env.torch.from_numpy(_stamps(env, B)).cuda()


def cases():
    """``[(id, group, function of the Env)]``: the function makes the call and returns the description of its answer"""
    out = []

    def add(cid, group, fn):
        assert cid not in [c[0] for c in out], cid
        out.append((cid, group, fn))

    # ---- solve_batch, accepted -------------------------------------------------------------------------------------
    for name in ("pinv", "qp"):
        for B in BATCHES:
            for kind in ("numpy", "tensor"):
                add("%s.solve_batch.B%d.%s" % (name, B, kind), name, solve_batch_case(name, B, kind))
        add("%s.solve_batch.list" % name, name, solve_batch_case(name, 1, "list"))
        add("%s.solve_batch.dm" % name, name, solve_batch_case(name, 1, "dm"))
        add("%s.solve_batch.f32_strided" % name, name, solve_batch_case(name, 65, "f32s"))
    add("pinv.solve_batch.out", "pinv", solve_batch_case("pinv", 65, "tensor", out=_dev(("B", 7))))
    add("pinv.solve_batch.out.numpy_inputs", "pinv", solve_batch_case("pinv", 63, "numpy", out=_dev(("B", 7))))
    add("pinv.solve_batch.no_mode", "pinv", solve_batch_case("pinv", 64, "tensor", return_mode=False))
    add("qp.solve_batch.no_status", "qp", solve_batch_case("qp", 64, "tensor", return_status=False))
    for use_hot in (True, False):
        add("qp.solve_batch.hot_set.use_hot_%s" % use_hot, "qp",
            solve_batch_case("qp", 65, "tensor", hot_set=_junk_sets, use_hot=use_hot, cold=True))
    for name in ("pinv_path", "qp_path"):
        for kind in ("numpy", "tensor"):
            add("%s.solve_batch.%s" % (name, kind), "virtual", solve_batch_case(name, 63, kind))
    for name in ("pinv_track", "qp_track"):
        add("%s.solve_batch.t_scalar" % name, "time", solve_batch_case(name, 65, t=1.5))
        add("%s.solve_batch.t_one_element" % name, "time", solve_batch_case(name, 65, t=np.array([1.5])))
        add("%s.solve_batch.t_per_instance" % name, "time", solve_batch_case(name, 65, t=_stamps))
        add("%s.solve_batch.t_wrong_length" % name, "time", solve_batch_case(name, 65, t=np.zeros(5)))
    for name in ("pinv_track_dev", "qp_track_dev"):
        add("%s.solve_batch.t_scalar" % name, "time", solve_batch_case(name, 65, "tensor", t=1.5))
        add("%s.solve_batch.t_per_instance" % name, "time", solve_batch_case(name, 65, t=_stamps))
        add("%s.solve_batch.t_device_tensor" % name, "time", solve_batch_case(name, 65, "tensor", t=_stamps_dev))
        add("%s.solve_batch.t_device_tensor_one" % name, "time",
            solve_batch_case(name, 65, "tensor", t=lambda env, B: env.torch.tensor([1.5], dtype=env.torch.float64, device="cuda")))
        add("%s.solve_batch.t_wrong_length" % name, "time",
            solve_batch_case(name, 65, "tensor", t=lambda env, B: _stamps_dev(env, 5)))
    # (a skill on the dynamic fallback kernel: one launch per distinct stamp, the QP's working sets through their rows)
    for kind in ("numpy", "tensor"):
        add("pinv_track_dyn.solve_batch.t_per_instance.%s" % kind, "dynamic", solve_batch_case("pinv_track_dyn", 65, kind, t=_stamps))
        add("qp_track_dyn.solve_batch.t_per_instance.%s" % kind, "dynamic", solve_batch_case("qp_track_dyn", 65, kind, t=_stamps))
    add("pinv_track_dyn.solve_batch.t_per_instance.no_mode", "dynamic",
        solve_batch_case("pinv_track_dyn", 65, t=_stamps, return_mode=False))
    add("pinv_track_dyn.solve_batch.t_per_instance.out", "dynamic",
        solve_batch_case("pinv_track_dyn", 65, "tensor", t=_stamps, out=_dev(("B", 6))))
    for use_hot in (True, False):
        add("qp_track_dyn.solve_batch.t_per_instance.hot_set.use_hot_%s" % use_hot, "dynamic",
            solve_batch_case("qp_track_dyn", 65, "tensor", t=_stamps, hot_set=_dev(("B",), "int32", 0), use_hot=use_hot,
                             cold=True))
    add("qp_track_dyn.solve_batch.t_per_instance.no_status", "dynamic",
        solve_batch_case("qp_track_dyn", 65, t=_stamps, return_status=False))

    # ---- bind_batch, accepted --------------------------------------------------------------------------------------
    for name in ("pinv", "qp"):
        for B in BATCHES:
            add("%s.bind_batch.B%d" % (name, B), name, bind_batch_case(name, B))
        add("%s.bind_batch.numpy" % name, name, bind_batch_case(name, 63, "numpy"))
        add("%s.bind_batch.f32_strided" % name, name, bind_batch_case(name, 65, "f32s"))
        add("%s.bind_batch.out" % name, name, bind_batch_case(name, 65, out=_dev(("B", 7))))
    add("pinv.bind_batch.mode_out", "pinv", bind_batch_case("pinv", 65, out=_dev(("B", 7)), mode_out=_dev(("B",), "int32")))
    add("qp.bind_batch.hot_start", "qp", bind_batch_case("qp", 65, times=(0.0, 0.0, 0.0), hot_start=True, cold=True))
    add("qp.bind_batch.hot_set", "qp", bind_batch_case("qp", 65, times=(0.0, 0.0), hot_set=_junk_sets, cold=True))
    add("qp.bind_batch.hot_set.primed", "qp", bind_batch_case("qp", 65, hot_set=_junk_sets, primed=True, cold=True))
    for name in ("pinv_path", "qp_path"):
        add("%s.bind_batch" % name, "virtual", bind_batch_case(name, 63))
    for name in ("pinv_track", "qp_track"):
        add("%s.bind_batch.times" % name, "time", bind_batch_case(name, 65, times=(0.0, 1.5)))

    def shared_sets(env):
        """two ticks bound with the SAME hot_set hand their working sets on: the second, primed, starts hot at once"""
        torch, ctrl = env.torch, env.ctrl("qp")
        hs = torch.zeros(65, dtype=torch.int32, device="cuda")
        res = {}
        for k, seed in enumerate((0, 0)):
            Q, _, Y = env.inputs("qp", 65, seed)
            Qd, Yd = env.conv(Q, "tensor"), env.conv(Y, "tensor")
            tick = ctrl.bind_batch(Qd, input_var=Yd, hot_set=hs)
            tick.primed = k > 0
            tick()
            torch.cuda.synchronize()
            ref = ctrl.solve_batch(0.0, Qd, input_var=Yd)
            res["tick%d" % k] = {"status": describe(tick.status), "hot_set_is_shared": tick.hot_set.data_ptr() == hs.data_ptr(),
                                 "same_as_cold": _close(tick.out, ref[0]), "sets": describe(hs)}
        return res
    add("qp.bind_batch.shared_hot_set", "qp", shared_sets)

    # ---- resident_start, accepted ----------------------------------------------------------------------------------
    for name in ("pinv", "qp"):
        for B in BATCHES:
            for D in (1, 2):
                add("%s.resident.B%d.D%d" % (name, B, D), name, resident_case(name, B, D))
        add("%s.resident.untouched_slot" % name, name, resident_case(name, 65, 2, n_ticks=1))
        add("%s.resident.one_dimensional" % name, name, resident_case(name, 1, one_d=True))
    add("pinv.resident.out", "pinv", resident_case("pinv", 65, 2, n_ticks=1, out=_dev((2, "B", 7), fill=7.0),
                                                   mode_out=_dev((2, "B"), "int32", 5)))
    add("pinv.resident.integrate", "pinv", resident_case("pinv", 64, integrate_dt=1e-3, max_speed=2.0))

    # ---- solve -----------------------------------------------------------------------------------------------------
    for name, group in (("pinv", "pinv"), ("qp", "qp"), ("pinv_path", "virtual"), ("qp_path", "virtual"),
                        ("pinv_track", "time"), ("qp_track", "time")):
        for kind in ("numpy", "list", "dm"):
            add("%s.solve.%s" % (name, kind), group, solve_case(name, kind, t=1.5, calls=2))
    add("pinv_track.solve.t_dm", "time", solve_case("pinv_track", t=cs.DM([1.5])))
    add("qp_path.solve.infeasible", "virtual", solve_case("qp_path", x=1.2))

    # ---- refused: inputs -------------------------------------------------------------------------------------------
    for method, make in (("solve_batch", solve_batch_case), ("bind_batch", bind_batch_case)):
        for name in ("pinv", "qp"):
            pre = "%s.%s.refused." % (name, method)
            add(pre + "missing_input_var", name, make(name, 64, "tensor", input_var=DROP))
            add(pre + "input_var_rows", name, make(name, 64, "tensor", input_var=_dev((63, 7), fill=0.0)))
            add(pre + "input_var_columns", name, make(name, 64, "tensor", input_var=_dev(("B", 6), fill=0.0)))
            add(pre + "robot_var_columns", name, make(name, 64, "numpy", robot_var=np.zeros((64, 6))))
            add(pre + "before_set_up", "unset", make(name + "_unset", 64, "numpy"))
        for name in ("pinv_path", "qp_path"):
            pre = "%s.%s.refused." % (name, method)
            add(pre + "missing_virtual_var", "virtual", make(name, 63, "numpy", virtual_var=DROP))
            add(pre + "virtual_var_rows", "virtual", make(name, 63, "numpy", virtual_var=np.zeros((62, 1))))
    # ---- refused: out / mode_out -----------------------------------------------------------------------------------
    bad_out = (("shape", _dev((63, 7))), ("dtype", _dev(("B", 7), "float32")), ("device", _host(("B", 7))),
               ("stride", _strided(("B", 7))), ("no_tensor", lambda env, B: np.zeros((B, 7))))
    for what, bad in bad_out:
        add("pinv.solve_batch.refused.out_%s" % what, "pinv", solve_batch_case("pinv", 64, "tensor", out=bad))
        add("pinv.bind_batch.refused.out_%s" % what, "pinv", bind_batch_case("pinv", 64, out=bad))
        add("qp.bind_batch.refused.out_%s" % what, "qp", bind_batch_case("qp", 64, out=bad))
    for what, bad in (("shape", _dev((63,), "int32")), ("dtype", _dev(("B",), "int64")), ("device", _host(("B",), "int32"))):
        add("pinv.bind_batch.refused.mode_out_%s" % what, "pinv", bind_batch_case("pinv", 64, mode_out=bad))
    # ---- refused: hot_set ------------------------------------------------------------------------------------------
    for what, bad in (("dtype", _dev(("B",), "int64", 0)), ("length", _dev((63,), "int32", 0)), ("host", _host(("B",), "int32"))):
        add("qp.solve_batch.refused.hot_set_%s" % what, "qp", solve_batch_case("qp", 64, "tensor", hot_set=bad))
        add("qp.bind_batch.refused.hot_set_%s" % what, "qp", bind_batch_case("qp", 64, hot_set=bad))
    add("qp.bind_batch.refused.hot_set_stride", "qp",
        bind_batch_case("qp", 64, hot_set=lambda env, B: env.torch.zeros(2 * B, dtype=env.torch.int32, device="cuda")[::2]))
    # ---- refused: resident -----------------------------------------------------------------------------------------
    for name in ("pinv", "qp"):
        pre = "%s.resident.refused." % name
        add(pre + "ring_depth_0", name, resident_refusal(name, ring_depth=0))
        add(pre + "before_set_up", "unset", resident_refusal(name + "_unset"))
        for D in (1, 2):
            lead = (D,) if D > 1 else ()
            for arg in ("robot_var", "input_var"):
                tpre = "%s.resident.refused.tensor.D%d.%s." % (name, D, arg)
                add(tpre + "host", name, resident_refusal(name, D=D, **{arg: _host(lead + ("B", 7))}))
                add(tpre + "float32", name, resident_refusal(name, D=D, **{arg: _dev(lead + ("B", 7), "float32", 0.0)}))
                add(tpre + "not_contiguous", name, resident_refusal(name, D=D, **{arg: _strided(lead + ("B", 7))}))
                add(tpre + "rank", name, resident_refusal(name, D=D, **{arg: _dev((1,) + lead + ("B", 7), fill=0.0)}))
                add(tpre + "columns", name, resident_refusal(name, D=D, **{arg: _dev(lead + ("B", 6), fill=0.0)}))
                add(tpre + "numpy", name, resident_refusal(name, D=D, **{arg: lambda env, B, lead=lead: np.zeros(
                    tuple(B if s == "B" else s for s in lead + ("B", 7)))}))
            add("%s.resident.refused.tensor.D%d.input_var.batch" % (name, D), name,
                resident_refusal(name, D=D, input_var=_dev(lead + (48, 7), fill=0.0)))
        add("%s.resident.refused.tensor.D2.robot_var.ring_depth" % name, name,
            resident_refusal(name, D=2, robot_var=_dev((3, "B", 7), fill=0.0)))
        add("%s.resident.refused.tensor.D2.input_var.ring_depth" % name, name,
            resident_refusal(name, D=2, input_var=_dev((3, "B", 7), fill=0.0)))
    add("qp.resident.refused.tensor.D1.input_var.one_dimensional", "qp",
        resident_refusal("qp", input_var=_dev((7,), fill=0.0)))
    add("qp_path.resident.refused.virtual_variables", "virtual", resident_refusal("qp_path", B=63))
    add("pinv_fb.resident.refused.velocity_feedback", "pinv", resident_refusal("pinv_fb", integrate_dt=1e-3))
    # ---- refused: solve --------------------------------------------------------------------------------------------
    for name in ("pinv", "qp"):
        add("%s.solve.refused.before_set_up" % name, "unset", solve_case(name + "_unset"))
    return out


GROUPS = ("pinv", "qp", "virtual", "time", "dynamic", "unset")


def shared_wording(cid):
    """PseudoInverseController.resident_start's refusals of its tensors take the wording the controllers share: the type
    of the exception is held, and the message must name the argument"""
    return cid.startswith("pinv.resident.refused.tensor.")


def run_case(env, fn):
    try:
        return {"returns": fn(env)}
    except Exception as exc:        # (what the call raises IS the answer)
        return {"raises": [type(exc).__name__, str(exc)]}
    finally:
        env.torch.cuda.synchronize()


def run_group(env, group):
    return {cid: run_case(env, fn) for cid, g, fn in cases() if g == group}
