"""A table of calls that the entry points of include/clik.h refuse before they launch anything, and what runs it.

tools/record_api_refusals.py wrote tests/golden/api_refusals.json from this table: {case id: [return code, clik_last_error
text]}; test_api_refusals.py (host-only handles, no GPU) and test_gpu_api_refusals.py (device handles) replay the table and
compare both exactly.  No case reaches a launch: every call has something wrong with it, or returns CLIK_OK early because
there is nothing to do (`ok` cases: B == 0, n_rec == 0).  The kernels "attached" here are stand-ins that say so when called.

Three skills: `pinv_y` - the tracking skill of time_skills.py with an input_var offset on its target (input_var and a time
slot); `pinv_x` - the path-following skill of converge_cases.py (one virtual variable); `qp` - skills.qp_skill (config 4, the
bound-constrained family).  B = 2, n_ticks = 2 throughout.

Three kinds of handle per skill: `host` (clik_*_create_host), `dev` (clik_*_create, nothing attached) and `full` (a device
handle with a stand-in for every attachable kernel the skill's family admits)."""
import ctypes as C

import casclik_amd as cc
from casclik_amd import _capi, skills
from casclik_amd import sym as cs
from casclik_amd.lowering import lower_skill

import converge_cases
import time_skills

SKILLS = ("pinv_y", "pinv_x", "qp")
B, N_TICKS = 2, 2


def _pinv_y_spec(fk):
    t, q, y = cs.MX.sym("t"), cs.MX.sym("q", 6), cs.MX.sym("y", 3)
    p = fk["T_fk"](q)[:3, 3]
    return cc.SkillSpecification("track_y", t, q, input_var=y, constraints=[
        cc.EqualityConstraint("move_point", p - time_skills._path(t) - y, gain=0.5, constraint_type="soft")])


def descriptors(iiwa_fk, ur5_fk):
    """{skill: (descriptor, options, n_x, n_y, n_tslots)} as ctypes structures"""
    out = {}
    for name, spec in (("pinv_y", _pinv_y_spec(ur5_fk)), ("pinv_x", converge_cases.path_skill(ur5_fk))):
        d = lower_skill(spec)
        opts = _capi.pinv_opts_to_c(cc.PseudoInverseController(skill_spec=spec).options)
        out[name] = (_capi.desc_to_c(d), opts, d.n_x, d.n_y, d.n_tslots)
    spec = skills.qp_skill(iiwa_fk)
    d = lower_skill(spec)
    opts = cc.ReactiveQPController(skill_spec=spec)._c_options(d)
    out["qp"] = (_capi.desc_to_c(d), opts, d.n_x, d.n_y, d.n_tslots)
    return out


# ---- the entry points' parameters, by name (include/clik.h) -------------------------------------------------------------
_SUM7 = "abs_max abs_max_at last rms viol_max viol_count settled_at"
_REC = "y_per_tick record_every rec_q rec_dq rec_x rec_dx"
_TRAJ = "h n_rec B tterms_dev tt_rec_stride tt_inst_stride q x y y_stride"
SIG = {
    "attach_kernel": "h fn fn2 name",
    "attach_value_kernel": "h fn fn2",
    "attach_resident_kernel": "h fn",
    "attach_rec_kernel": "h fn fn2",
    "attach_time_kernel": "h fn",
    "attach_monitor_kernel": "h fn",
    "attach_summary_kernel": "h fn work_fn",
    "attach_rollout_summary_kernel": "h fn",
    "attach_converge_kernel": "h fn",
    "image_words": "h words cap",
    "resident_waves": "h B",
    "time_terms": "h n_times times stages dt out stream",
    "constraint_values": _TRAJ + " e J et stream",
    "constraint_summary": _TRAJ + " tol work work_bytes " + _SUM7 + " stream",
    "pinv_resident_run": "h B n_ticks tterms q y dq mode ticket done timeout_s stream",
    "pinv_resident_run_state": "h B n_ticks tterms q y dq mode ticket done integrate_dt max_speed timeout_s stream",
    "pinv_solve_batch": "h B tterms q x y dq dx mode stream",
    "pinv_solve_batch_t": "h B t_inst q x y dq dx mode stream",
    "pinv_rollout_batch": "h B n_ticks dt max_speed tterms q y dq mode stream",
    "pinv_rollout_batch_x": "h B n_ticks dt max_speed tterms q x y dq dx mode stream",
    "pinv_rollout_batch_m": "h B n_ticks method dt max_speed tterms q x y dq dx mode stream",
    "pinv_rollout_batch_rec": "h B n_ticks method dt max_speed tterms q x y dq dx mode stream " + _REC + " rec_mode",
    "pinv_rollout_batch_dev": "h B n_ticks method dt max_speed times q x y dq dx mode stream " + _REC + " rec_mode",
    "pinv_rollout_batch_sum": "h B n_ticks method dt max_speed tterms q x y dq dx mode stream " + _REC + " rec_mode "
                              "times_alt tol " + _SUM7,
    "pinv_converge_batch": "h B max_ticks dt max_speed min_step tterms q x y dq dx mode tol ticks stop_status residual "
                           "stream",
    "qp_resident_run": "h B n_ticks tterms q y dq slack status ticket done timeout_s stream",
    "qp_solve_batch": "h B tterms q x y dq dx slack status stream",
    "qp_solve_batch_hot": "h B tterms q x y dq dx slack status hot_set use_hot stream",
    "qp_solve_batch_t": "h B t_inst q x y dq dx slack status hot_set use_hot stream",
    "qp_data_batch": "h B tterms q x y Hdiag A lbA ubA stream",
    "qp_rollout_batch": "h B n_ticks dt max_speed tterms q y dq slack status stream",
    "qp_rollout_batch_x": "h B n_ticks dt max_speed tterms q x y dq dx slack status stream",
    "qp_rollout_batch_m": "h B n_ticks method dt max_speed tterms q x y dq dx slack status stream",
    "qp_rollout_batch_rec": "h B n_ticks method dt max_speed tterms q x y dq dx slack status stream " + _REC
                            + " rec_slack rec_status",
    "qp_rollout_batch_dev": "h B n_ticks method dt max_speed times q x y dq dx slack status stream " + _REC
                            + " rec_slack rec_status",
    "qp_rollout_batch_sum": "h B n_ticks method dt max_speed tterms q x y dq dx slack status stream " + _REC
                            + " rec_slack rec_status times_alt tol " + _SUM7,
    "qp_converge_batch": "h B max_ticks dt max_speed min_step tterms q x y dq dx status slack tol ticks stop_status "
                         "residual stream",
}
# the entry points that both controllers have under the same parameter list
_SHARED = ("attach_kernel", "attach_value_kernel", "attach_resident_kernel", "attach_rec_kernel", "attach_time_kernel",
           "attach_monitor_kernel", "attach_summary_kernel", "attach_rollout_summary_kernel", "attach_converge_kernel",
           "image_words", "resident_waves", "time_terms", "constraint_values", "constraint_summary")
_NUMBERS = dict(B=B, n_ticks=N_TICKS, n_rec=2, n_times=2, max_ticks=2, method=0, stages=1, dt=0.01, max_speed=0.0,
                min_step=0.0, timeout_s=1.0, integrate_dt=0.01, y_per_tick=0, record_every=1, use_hot=0, tt_rec_stride=0,
                tt_inst_stride=0, y_stride=0, work_bytes=1 << 16, cap=1 << 16, name=b"stand_in", stream=None,
                times_alt=None)
STAND_IN_WORK_BYTES = 4096


def symbol(kind, fn):
    """entry point of controller `kind` ("pinv" | "qp") for a key of SIG"""
    return "clik_%s_%s" % (kind, fn) if fn in _SHARED else "clik_" + fn


def good_args(fn, kind, info, h, bufs):
    """a call of `fn` with nothing wrong with it, as {parameter: value} in the order of SIG"""
    _, _, n_x, n_y, n_tslots = info
    P = bufs["dev"]
    out = {}
    for name in SIG[fn].split():
        if name == "h":
            v = h
        elif name in _NUMBERS:
            v = _NUMBERS[name]
        elif name in ("fn", "fn2"):
            v = bufs["stand_in"]
        elif name == "work_fn":
            v = bufs["stand_in_work"]
        elif name == "words":
            v = bufs["words"]
        elif name == "tterms":          # (host)
            v = bufs["host"] if n_tslots else None
        elif name in ("tterms_dev", "times", "t_inst"):
            v = P if n_tslots else None
        elif name in ("x", "dx", "rec_x", "rec_dx"):
            v = P if n_x else None
        elif name == "y":
            v = P if n_y else None
        else:
            v = P
        out[name] = v
    return out


# ---- the table -----------------------------------------------------------------------------------------------------------
def _launch_cases(kind, skill, info):
    """(handle kind, fn, label, overrides, ok) for the entry points that take batch arguments"""
    _, _, n_x, n_y, n_ts = info
    out = []

    def add(hk, name, label, ok=False, **over):
        out.append((hk, name, label, over, ok))
    fns = [f for f in SIG if f.startswith(kind + "_")] + ["time_terms", "constraint_values", "constraint_summary"]
    for fn in fns:
        names = SIG[fn].split()
        add("host", fn, "null_handle", h=None)
        add("host", fn, "host_only")
        # (clik_*_constraint_values / _summary check their arguments before they ask for a device handle)
        for hk in ("dev", "full") + (("host",) if fn.startswith("constraint_") else ()):
            for size in ("B", "n_ticks", "n_rec", "n_times", "max_ticks"):
                if size in names:
                    add(hk, fn, "negative_" + size, **{size: -1})
            for size in ("B", "n_rec", "n_times"):
                # (nothing to do: CLIK_OK without a launch - where the entry point says so; the others refuse a zero)
                if size in names:
                    add(hk, fn, "zero_" + size, ok=fn not in ("pinv_resident_run", "pinv_resident_run_state", "qp_resident_run",
                                                               "pinv_converge_batch", "qp_converge_batch"), **{size: 0})
            if "method" in names:
                add(hk, fn, "unknown_method", method=7)
            if "stages" in names:
                add(hk, fn, "unknown_stages", stages=3)
            if "record_every" in names:
                add(hk, fn, "negative_record_every", record_every=-1)
            if "settled_at" in names:
                add(hk, fn, "tol_without_settled_at", settled_at=None)
                add(hk, fn, "settled_at_without_tol", tol=None)
            if "times_alt" in names and n_ts:
                add(hk, fn, "tterms_and_times", times_alt="dev")
                add(hk, fn, "neither_tterms_nor_times", tterms=None)
            if "timeout_s" in names:
                add(hk, fn, "timeout_zero", timeout_s=0.0)
                add(hk, fn, "timeout_beyond_60", timeout_s=61.0)
            if "integrate_dt" in names:
                add(hk, fn, "integrate_dt_zero", integrate_dt=0.0)
                add(hk, fn, "negative_max_speed", max_speed=-1.0)
            if "work_bytes" in names:
                add(hk, fn, "work_too_small", work_bytes=16)
                add(hk, fn, "negative_stride", y_stride=-1)
            if fn == "constraint_values":
                add(hk, fn, "nothing_to_compute", e=None, J=None, et=None)
        # every required pointer null in turn, on the handle that has the kernels (the checks behind the kernel-presence
        # checks are reached there only); `dev` answers the same calls with what is missing
        optional = {"stream", "mode", "slack", "status", "hot_set", "e", "J", "et", "rec_q", "rec_dq", "rec_x", "rec_dx",
                    "rec_mode", "rec_slack", "rec_status", "times_alt", "h"}
        for name in names:
            if name in _NUMBERS or name in optional:
                continue
            if name in ("x", "dx") and not n_x or name == "y" and not n_y:
                continue
            if (name in ("tterms", "tterms_dev", "times", "t_inst") or fn == "time_terms") and not n_ts:
                continue            # (nothing depends on time: not read, and clik_*_time_terms has nothing to do)
            add("full", fn, "null_" + name, **{name: None})
            # (wrong in two ways - no x or dx AND no kernel for a skill with virtual variables: the rollouts ask for x / dx
            # before they look for their kernel)
            if name in ("x", "dx"):
                add("dev", fn, "null_" + name, **{name: None})
        # nothing wrong with the call but that the kernel it needs was never attached (record_every = 1: the plain rollout
        # kernels cannot serve _dev either)
        if fn.split("_", 1)[-1] in ("rollout_batch_rec", "rollout_batch_dev", "rollout_batch_sum", "converge_batch",
                                     "resident_run", "resident_run_state") or fn.startswith("constraint_") \
                or (fn == "time_terms" and n_ts):
            add("dev", fn, "nothing_attached")
    return out


def _other_cases(kind, skill):
    out = []

    def add(hk, name, label, **over):
        out.append((hk, name, label, over, False))
    for fn in ("attach_kernel", "attach_value_kernel", "attach_resident_kernel", "attach_rec_kernel", "attach_time_kernel",
               "attach_monitor_kernel", "attach_summary_kernel", "attach_rollout_summary_kernel", "attach_converge_kernel",
               "image_words", "resident_waves"):
        add("host", fn, "null_handle", h=None)
    for fn in ("attach_kernel", "attach_rec_kernel", "attach_monitor_kernel", "attach_summary_kernel",
               "attach_rollout_summary_kernel", "attach_converge_kernel"):
        add("host", fn, "host_only")
    add("host", "attach_rec_kernel", "host_only_detach", fn=None, fn2=None)
    add("host", "attach_kernel", "null_solve_fn", fn=None)
    add("dev", "attach_kernel", "null_solve_fn", fn=None)
    add("dev", "attach_summary_kernel", "without_work_fn", work_fn=None)
    add("full", "attach_summary_kernel", "without_work_fn", work_fn=None)
    add("host", "attach_summary_kernel", "without_work_fn", work_fn=None)
    # (what a handle served by the built-in kernel answers, or one outside the kernel's family)
    if kind == "pinv":
        for fn in ("attach_rec_kernel", "attach_monitor_kernel", "attach_summary_kernel", "attach_rollout_summary_kernel",
                   "attach_converge_kernel"):
            add("dev", fn, "family")
    if skill == "pinv_x":
        add("host", "attach_value_kernel", "family")
        add("host", "attach_resident_kernel", "family")
    add("host", "image_words", "null_buffer", words=None)
    add("host", "image_words", "zero_cap", cap=0)
    add("host", "image_words", "small_cap", cap=1)
    add("host", "resident_waves", "zero_B", B=0)
    add("host", "resident_waves", "negative_B", B=-1)
    return out


def cases(infos):
    """[(case id, skill, handle kind, symbol, fn, overrides, ok)] - `infos` from descriptors()"""
    out = []
    for skill in SKILLS:
        kind = "qp" if skill == "qp" else "pinv"
        for hk, fn, label, over, ok in _launch_cases(kind, skill, infos[skill]) + _other_cases(kind, skill):
            out.append(("%s/%s/%s/%s" % (hk, skill, symbol(kind, fn), label), skill, hk, symbol(kind, fn), fn, over, ok))
    ids = [c[0] for c in out]
    assert len(ids) == len(set(ids))
    return out


# calls without a handle: (case id, symbol, arguments by position - "desc" / "opts" / "buf" / "out" are filled in per skill)
def free_cases():
    out = []
    for skill in SKILLS:
        kind = "qp" if skill == "qp" else "pinv"
        for create in ("create", "create_host"):
            sym = "clik_%s_%s" % (kind, create)
            out += [("free/%s/%s/null_out" % (skill, sym), skill, sym, ("desc", "opts", None)),
                    ("free/%s/%s/null_opts" % (skill, sym), skill, sym, ("desc", None, "out")),
                    ("free/%s/%s/null_desc" % (skill, sym), skill, sym, (None, "opts", "out")),
                    ("free/%s/%s/abi_version" % (skill, sym), skill, sym, ("desc_abi", "opts", "out"))]
        if kind == "pinv":
            sym = "clik_shape_describe"
            out += [("free/%s/%s/null_opts" % (skill, sym), skill, sym, ("desc", None, "buf", 1 << 16)),
                    ("free/%s/%s/null_buffer" % (skill, sym), skill, sym, ("desc", "opts", None, 1 << 16)),
                    ("free/%s/%s/zero_cap" % (skill, sym), skill, sym, ("desc", "opts", "buf", 0)),
                    ("free/%s/%s/small_cap" % (skill, sym), skill, sym, ("desc", "opts", "buf", 8)),
                    ("free/%s/%s/null_desc" % (skill, sym), skill, sym, (None, "opts", "buf", 1 << 16))]
        else:
            sym = "clik_qp_shape_describe"
            out += [("free/%s/%s/null_buffer" % (skill, sym), skill, sym, ("desc", None, 1 << 16)),
                    ("free/%s/%s/zero_cap" % (skill, sym), skill, sym, ("desc", "buf", 0)),
                    ("free/%s/%s/small_cap" % (skill, sym), skill, sym, ("desc", "buf", 8)),
                    ("free/%s/%s/null_desc" % (skill, sym), skill, sym, (None, "buf", 1 << 16))]
    P = "dev"
    out += [("free/clik_ticket_feed/null_ticket", None, "clik_ticket_feed", (None, P, 2, 0, 1, 1.0, None)),
            ("free/clik_ticket_feed/null_done", None, "clik_ticket_feed", (P, None, 2, 0, 1, 1.0, None)),
            ("free/clik_ticket_feed/zero_ticks", None, "clik_ticket_feed", (P, P, 0, 0, 1, 1.0, None)),
            ("free/clik_ticket_feed/zero_waves", None, "clik_ticket_feed", (P, P, 2, 0, 0, 1.0, None)),
            ("free/clik_ticket_feed/timeout_zero", None, "clik_ticket_feed", (P, P, 2, 0, 1, 0.0, None)),
            ("free/clik_ticket_feed/timeout_beyond_60", None, "clik_ticket_feed", (P, P, 2, 0, 1, 61.0, None))]
    return out


# ---- running it ----------------------------------------------------------------------------------------------------------
class Runner:
    """Creates the handles of one kind of machine (`device`: False - host-only handles alone) and runs cases on them.
    `dev_buffer` is the address of 1 MiB that every non-null device pointer of a call points at: device memory on a GPU
    machine - a case that slipped through to a launch would compute on it, not fault -, any memory without one."""

    def __init__(self, lib, iiwa_fk, ur5_fk, device, dev_buffer):
        self.lib = lib
        self.infos = descriptors(iiwa_fk, ur5_fk)
        self.called, self.unexpected = [], []

        def stand_in(*a):
            self.called.append("kernel")
            return 1

        def stand_in_work(n_rec, nb):
            return STAND_IN_WORK_BYTES
        self._keep = (C.CFUNCTYPE(C.c_int)(stand_in), C.CFUNCTYPE(C.c_ulonglong, C.c_longlong, C.c_longlong)(stand_in_work))
        self.bufs = {"dev": dev_buffer, "host": (C.c_double * 4096)(), "words": (C.c_uint64 * (1 << 16))(),
                     "stand_in": C.cast(self._keep[0], C.c_void_p), "stand_in_work": C.cast(self._keep[1], C.c_void_p)}
        self.handles, self.attached = {}, {}
        for skill in SKILLS:
            kind = "qp" if skill == "qp" else "pinv"
            for hk in ("host", "dev", "full") if device else ("host",):
                h = C.c_void_p()
                create = getattr(lib, "clik_%s_create%s" % (kind, "_host" if hk == "host" else ""))
                rc = create(C.byref(self.infos[skill][0]), C.byref(self.infos[skill][1]), C.byref(h))
                assert rc == 0, lib.clik_last_error()
                self.handles[(skill, hk)] = h
                if hk == "full":
                    self.attached[skill] = self._attach_all(kind, skill, h)

    def _attach_all(self, kind, skill, h):
        """a stand-in for every attachable kernel; {symbol: return code} - a skill outside a kernel's family is refused"""
        got = {}
        for fn in ("attach_kernel", "attach_rec_kernel", "attach_time_kernel", "attach_monitor_kernel",
                   "attach_summary_kernel", "attach_rollout_summary_kernel", "attach_converge_kernel",
                   "attach_resident_kernel"):
            args = good_args(fn, kind, self.infos[skill], h, self.bufs)
            rc = getattr(self.lib, symbol(kind, fn))(*args.values())
            got[symbol(kind, fn)] = [int(rc), self.lib.clik_last_error().decode() if rc != 0 else ""]
        return got

    def setup_results(self):
        """what attaching the stand-ins to the `full` handles answered, as cases"""
        return {"full/%s/setup/%s" % (skill, sym): res for skill, by_sym in self.attached.items()
                for sym, res in by_sym.items()}

    def describe_handles(self, handle_kinds=("dev", "full")):
        """{"describe/<handle kind>/<skill>": [image words, text]}: everything the library tells about the skill a handle
        holds - the words of its image (their count and SHA-256), the kernel that serves it at four batch sizes, its sizes
        and the ShapeDesc text of its descriptor.  (The DevSkill record on the device has no accessor: this is what stands
        in for comparing its bytes.)"""
        import hashlib
        lib, got = self.lib, {}
        for (skill, hk), h in self.handles.items():
            if hk not in handle_kinds:
                continue
            kind = "qp" if skill == "qp" else "pinv"
            n = getattr(lib, "clik_%s_image_words" % kind)(h, self.bufs["words"], len(self.bufs["words"]))
            assert n > 0, lib.clik_last_error()
            text = ["sha256=" + hashlib.sha256(bytes(memoryview(self.bufs["words"]))[:8 * n]).hexdigest(),
                    "kernel=" + getattr(lib, "clik_%s_kernel_name" % kind)(h).decode(),
                    "rows=%d" % getattr(lib, "clik_%s_n_constraint_rows" % kind)(h)]
            buf = C.create_string_buffer(1 << 16)
            desc, opts = self.infos[skill][:2]
            if kind == "pinv":
                text.append("variants=" + ",".join(lib.clik_pinv_kernel_variant(h, b).decode() for b in (1, 64, 16385, 1 << 20)))
                text.append("modes=%d" % lib.clik_pinv_n_modes(h))
                text.append("eligible=%d" % lib.clik_shape_describe(C.byref(desc), C.byref(opts), buf, len(buf)))
            else:
                text.append("variants=" + ",".join(lib.clik_qp_kernel_variant(h, b, hot).decode()
                                                   for b in (1, 64, 16385, 1 << 20) for hot in (0, 1)))
                text.append("vars=%d rows=%d box=%d workspace=%d" % (lib.clik_qp_n_vars(h), lib.clik_qp_n_rows(h),
                                                                       lib.clik_qp_is_box_family(h),
                                                                       lib.clik_qp_workspace_bytes(h)))
                text.append("eligible=%d" % lib.clik_qp_shape_describe(C.byref(desc), buf, len(buf)))
            text.append("shape=" + buf.value.decode())
            got["describe/%s/%s" % (hk, skill)] = [int(n), " ".join(text)]
        return got

    def close(self):
        for (skill, _), h in self.handles.items():
            assert getattr(self.lib, "clik_%s_destroy" % ("qp" if skill == "qp" else "pinv"))(h) == 0
        self.handles = {}

    def _result(self, rc):
        assert not self.called, "a case reached a kernel"
        return [int(rc), self.lib.clik_last_error().decode() if rc != 0 else ""]

    def run(self, case):
        _, skill, hk, sym, fn, over, ok = case
        kind = "qp" if skill == "qp" else "pinv"
        args = good_args(fn, kind, self.infos[skill], self.handles[(skill, hk)], self.bufs)
        for k, v in over.items():
            assert k in args, (case[0], k)
            args[k] = self.bufs["dev"] if v == "dev" else v
        rc = getattr(self.lib, sym)(*args.values())
        if (rc == 0) != ok:
            self.unexpected.append((case[0], rc))
        return self._result(rc)

    def run_free(self, case):
        _, skill, sym, args = case
        out = C.c_void_p()
        buf = C.create_string_buffer(1 << 16)
        stale = None
        if skill is not None:
            stale = type(self.infos[skill][0])()
            C.memmove(C.byref(stale), C.byref(self.infos[skill][0]), C.sizeof(stale))
            stale.abi_version = 99
        named = {"out": C.byref(out), "buf": buf, "dev": self.bufs["dev"]}
        if skill is not None:
            named.update(desc=C.byref(self.infos[skill][0]), opts=C.byref(self.infos[skill][1]), desc_abi=C.byref(stale))
        rc = getattr(self.lib, sym)(*[named[a] if isinstance(a, str) else a for a in args])
        assert rc < 0 and not out.value, (case[0], rc)
        return self._result(rc)

    def run_all(self, handle_kinds):
        """{case id: [code, text]} of the cases on these kinds of handle ("free": the calls without one)"""
        got = {}
        for case in cases(self.infos):
            if case[2] in handle_kinds:
                got[case[0]] = self.run(case)
        if "free" in handle_kinds:
            for case in free_cases():
                got[case[0]] = self.run_free(case)
        assert not self.unexpected, "refused where the table says CLIK_OK, or the reverse: %s" % self.unexpected
        return got
