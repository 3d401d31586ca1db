"""PseudoInverseController: set-based task-priority CLIK, batched on the GPU.

Same constructor, options, setup and ``solve`` surface as the reference class
(reference: casclik/controllers/pseudo_inverse.py:10-556); ``solve_batch`` and
``rollout_batch`` are the additions that expose the batch dimension.  Where the
reference builds and JIT-compiles one CasADi function per mode
(:259-483), ``setup_problem_functions`` lowers the skill to the flat device
descriptor and uploads it; ``solve`` launches the HIP kernel (B = 1) instead
of scanning modes in Python (:512-556).
"""
from __future__ import annotations

import os

import numpy as np

from .. import _capi
from .. import sym as cs
from ..lowering import DYN_MAX_M
from .base_controller import BaseController, ring_depth_request, _torch


class PseudoInverseController(BaseController):
    """Pseudo inverse controller (Moe's set-based task priority scheme).

    Args:
        skill_spec (SkillSpecification): skill specification
        options (dict): see ``options`` setter for keys and defaults
    """
    controller_type = "PseudoInverseController"
    options_info = """feedforward (bool, True), multidim_sets (bool, False),
    converge_final_set_to_max (bool, False), pinv_method ("damped"|"standard"),
    damping_factor (float, 1e-7), function_opts (dict, accepted and ignored:
    there is no CasADi JIT on this path), device (torch device, optional), time_on_device (bool, False: evaluate the
    skill's time slots with a generated device kernel - rollouts and per-instance-time ticks then take their times
    from the device, see ``time_terms_batch``)"""
    _create_fn, _destroy_fn = "clik_pinv_create", "clik_pinv_destroy"
    _kind = "pinv"
    _rollout_tail = (("mode", None, "int32"),)
    _tick_fn, _tick_t_fn = "clik_pinv_solve_batch", "clik_pinv_solve_batch_t"

    def __init__(self, skill_spec, options=None):
        self._handle = None
        self._lib = None
        self.skill_spec = skill_spec
        self.options = options
        self.current_mode = None
        self.modes = None

    # -- options (pseudo_inverse.py:42-66) --------------------------------
    @property
    def options(self):
        return self._options

    @options.setter
    def options(self, opt):
        if opt is None:
            opt = {}
        opt.setdefault("feedforward", True)
        opt.setdefault("multidim_sets", False)
        opt.setdefault("converge_final_set_to_max", False)
        opt.setdefault("pinv_method", "damped")
        opt.setdefault("damping_factor", 1e-7)
        fopts = opt.setdefault("function_opts", {})
        fopts.setdefault("jit", True)
        fopts.setdefault("print_time", False)
        fopts.setdefault("jit_options", {"flags": "-O2"})
        self._options = opt

    # -- skill (pseudo_inverse.py:74-90) ----------------------------------
    @property
    def skill_spec(self):
        return self._skill_spec

    @skill_spec.setter
    def skill_spec(self, spec):
        cnt = spec.count_constraints()
        self.n_set_constraints = cnt["set"]
        self.n_modes = 2 ** cnt["set"]
        self.n_state_var = spec.n_robot_var + (spec.n_virtual_var
                                               if spec.virtual_var is not None else 0)
        # (pseudo_inverse.py:79-88: the stacked state and the list of its velocity symbols)
        self.state_var = (cs.vertcat(spec.robot_var, spec.virtual_var) if spec.virtual_var is not None
                          else cs.vertcat(spec.robot_var))
        self.cntrl_var = [spec.robot_vel_var] + ([spec.virtual_vel_var] if spec.virtual_var is not None else [])
        self._skill_spec = spec
        self.create_activation_map()

    def pinv(self, J):
        """The controller's pseudo-inverse of a symbolic (or numeric) matrix (pseudo_inverse.py:92-105): "standard" is
        cs.pinv; "damped" solves with J J' + lam I when J has at least as many columns as rows, else with J'J + lam I.
        The kernels evaluate the same rule (clik_pinv_static.hpp); this method is the reference's public helper."""
        J = J if isinstance(J, cs.MX) else cs.MX(J)
        if self.options["pinv_method"] == "standard":
            return cs.pinv(J)
        lam = self.options["damping_factor"]
        rows, cols = J.size()
        if cols >= rows:
            return cs.solve(cs.mtimes(J, J.T) + lam * cs.DM.eye(rows), J).T
        return cs.solve(cs.mtimes(J.T, J) + lam * cs.DM.eye(cols), J.T)

    def _tangent_cone_signature(self, cnstr):
        from ..constraints import SetConstraint
        if not isinstance(cnstr, SetConstraint):
            raise TypeError("in_tangent_cone is only available for SetConstraint")
        spec = self.skill_spec
        args, names = [spec.time_var, spec.robot_var], ["time_var", "robot_var"]
        rates, rate_names = [spec.robot_vel_var], ["robot_vel_var"]
        # de/dt along the motion: the partial time derivative plus the Jacobians times the velocity symbols
        # (pseudo_inverse.py:155-160)
        rate = cs.jacobian(cnstr.expression, spec.time_var) + cs.jtimes(cnstr.expression, spec.robot_var,
                                                                         spec.robot_vel_var)
        if spec.virtual_var is not None:
            args, names = args + [spec.virtual_var], names + ["virtual_var"]
            rates, rate_names = rates + [spec.virtual_vel_var], rate_names + ["virtual_vel_var"]
            rate = rate + cs.jtimes(cnstr.expression, spec.virtual_var, spec.virtual_vel_var)
        if spec.input_var is not None:
            args, names = args + [spec.input_var], names + ["input_var"]
        return rate, args + rates, names + rate_names

    def get_in_tangent_cone_function(self, cnstr):
        """cs.Function `(time_var, robot_var[, virtual_var][, input_var], robot_vel_var[, virtual_vel_var]) -> 0 / 1`:
        is a velocity inside the tangent cone of a one-dimensional SetConstraint (pseudo_inverse.py:132-190)?  Inside
        the set (with the 1e-12 margins): yes; below it: only when the expression increases; above: only when it
        decreases.  The kernels run this test after every mode (clik_pinv_static.hpp::cone_s); this is the reference's
        public, host-evaluated form of it."""
        rate, args, names = self._tangent_cone_signature(cnstr)
        e, lo, hi = cnstr.expression, cnstr.set_min, cnstr.set_max
        below_ok = cs.if_else(rate > 0.0, 1.0, 0.0)
        above_ok = cs.if_else(rate < 0.0, 1.0, 0.0)
        in_tc = cs.if_else(lo - e < 1e-12, cs.if_else(e - hi < 1e-12, 1.0, above_ok), below_ok)
        label = "in_tc_" + cnstr.label.replace(" ", "_")
        return cs.Function(label, args, [in_tc], names, ["in_tc_" + cnstr.label])

    def get_in_tangent_cone_function_multidim(self, cnstr):
        """The same for a multidimensional SetConstraint (pseudo_inverse.py:192-257): inside the box (margins 1e-12
        per row): yes; outside, the outward direction is the mean of the signs of the distances to both bounds; when
        every row has left its interval ("corner") the velocity must also make less than 45 degrees with the inward
        direction, otherwise a negative outward component is enough (clik_pinv_static.hpp::cone_s)."""
        rate, args, names = self._tangent_cone_signature(cnstr)
        le, ue = cnstr.expression - cnstr.set_min, cnstr.expression - cnstr.set_max
        row_above, row_below = le >= 1e-12, ue <= 1e-12
        inside = cs.logic_and(cs.dot(row_above - 1, row_above - 1) == 0, cs.dot(row_below - 1, row_below - 1) == 0)
        outward = (cs.sign(le) + cs.sign(ue)) / 2.0
        same = cs.sign(le) == cs.sign(ue)
        corner = cs.dot(same - 1, same - 1) == 0
        along = cs.dot(outward, rate)
        spread = (cs.norm_2(rate) + 1e-10) * cs.norm_2(outward)
        corner_ok = cs.if_else(along < 0.0, cs.fabs(cs.dot(-outward, rate)) / spread < np.cos(np.pi / 4), 0.0)
        going_in = cs.if_else(corner, corner_ok, along < 0.0)
        in_tc = cs.if_else(inside, 1.0, going_in)
        label = "in_tc_" + cnstr.label.replace(" ", "_")
        return cs.Function(label, args, [in_tc], names, ["in_tc_" + cnstr.label])

    def create_activation_map(self):
        """Mode order (pseudo_inverse.py:107-130): bit patterns with set 0 as
        least significant bit, stably sorted by the number of active sets."""
        n_sets = self.n_set_constraints
        if n_sets == 0:
            self.activation_map = []
            return
        patterns = [[(idx >> k) & 1 for k in range(n_sets)]
                    for idx in range(2 ** n_sets)]
        self.activation_map = sorted(patterns, key=sum)

    # -- setup --------------------------------------------------------------
    def get_problem_expressions(self):
        """Per-mode bookkeeping (which sets are active / tested); the
        arithmetic itself lives in the device kernel."""
        set_labels = [c.label for c in self.skill_spec.constraints
                      if c.constraint_class == "SetConstraint"]
        modes = []
        for mode_idx in range(self.n_modes):
            bits = self.activation_map[mode_idx] if self.activation_map else []
            modes.append({
                "active_set_names": [l for l, b in zip(set_labels, bits) if b],
                "in_tangent_cone_set_names": [l for l, b in zip(set_labels, bits) if not b],
            })
        self.modes = modes
        return modes

    def setup_problem_functions(self):
        """Lower the skill and create the device handle (replaces the
        per-mode ``cs.Function`` JIT of pseudo_inverse.py:453-483)."""
        from .. import jit
        self.get_problem_expressions()
        cdesc, copts = self._create_handle()
        handle, d = self._handle, self.descriptor
        # no AOT shape for this skill: instantiate the static templates for it
        self._setup_shape_kernel(lambda: jit.attach(self._lib, handle, cdesc, copts, extern=d.extern_source()))
        # The skill's kernels with its own numbers compiled in (the reference's JIT compiles its functions with the
        # constants of the skill too): for the config-3 family (four lanes per instance at small batches, one lane per
        # instance above) and for single-mode skills without virtual variables (BASELINE configs 1 and 2: one lane
        # per instance, no LDS) - one more hipcc run at set-up.  function_opts["jit_values"] = False or
        # CLIK_JIT_VALUES=0 keeps the kernels that read the skill image from memory.
        jv = self.options["function_opts"].get("jit_values", None)
        env_jv = os.environ.get("CLIK_JIT_VALUES", "1")
        variant1 = self._lib.clik_pinv_kernel_variant(handle, 1).decode()
        single_mode = (d.n_x == 0 and d.n_sets == 0 and variant1 == "lane")
        wanted = (variant1 == "team4" or single_mode) and jv is not False and env_jv != "0"
        self._setup_value_kernel(
            wanted, lambda: jit.attach_values(self._lib, handle, cdesc, copts, extern=d.extern_source()),
            "value-specialised kernel could not be built, using the image-reading one")
        if self.kernel_name == "none":
            raise NotImplementedError(
                "a constraint of this skill has more rows than the built-in kernels are wide (%d) and no "
                "shape-specialised kernel could be instantiated for it (jit disabled, hipcc missing, or the "
                "skill is outside the shape-specialised family)" % DYN_MAX_M)
        self._require_generated_code_kernel()
        self._setup_time_kernel()

    def _c_options(self, d):
        return _capi.pinv_opts_to_c(self.options)

    def kernel_variant(self, batch):
        """``<kernel>/<variant>`` serving a batch of that many instances: ``team4`` (four lanes per
        instance), ``mp2`` / ``mp4`` (one wave per mode), ``lane`` (one instance per lane), ``lane/occ2`` (its
        two-waves-per-SIMD build); ``team4v`` / ``quadv`` / ``lanev`` with the skill's numbers compiled in."""
        return "%s/%s" % (self.kernel_name, self._lib.clik_pinv_kernel_variant(self._handle, int(batch)).decode())

    def setup_solver(self):
        """Reference parity: re-runs the problem setup (pseudo_inverse.py:506-510)."""
        self.setup_problem_functions()

    def setup_initial_problem_solver(self):
        """Does nothing, as in the reference (pseudo_inverse.py:485-488)."""
        pass

    def solve_initial_problem(self, time_var0, robot_var0, virtual_var0=None,
                              robot_vel_var0=None, input_var0=None):
        """Zeros, as in the reference (pseudo_inverse.py:490-504)."""
        spec = self.skill_spec
        res_virt = cs.DM.zeros(spec.n_virtual_var, 1) if virtual_var0 is not None else None
        res_slack = cs.DM.zeros(spec.n_slack_var, 1) if spec.slack_var is not None else None
        return res_virt, res_slack

    # -- per-tick -------------------------------------------------------------
    def solve_batch(self, time_var, robot_var, virtual_var=None, input_var=None,
                    out=None, return_mode=True):
        """One controller tick for a batch.

        robot_var [B, n_q], virtual_var [B, n_x], input_var [B, n_y] as numpy
        arrays or torch tensors (tensors on the controller's device are used
        in place).  ``time_var``: one time stamp for the batch, or an array with one per
        instance (robots at different phases of a trajectory): ONE launch of the per-instance-time kernel
        (clik_pinv_solve_batch_t); a skill served by the dynamic fallback kernel has no such variant, its batch is
        grouped by distinct time stamps, one launch per group.  With ``options["time_on_device"]`` the per-instance
        time terms come from the time kernel (``time_terms_batch``) and ``time_var`` may be a device tensor, read in
        place; a skill on the dynamic fallback kernel keeps the host evaluation, and so does one stamp for the whole
        batch (its time terms travel by value with the launch).  Returns (robot_vel [B,n_q], virtual_vel | None,
        mode [B]) in the container type of ``robot_var``.  The launch is asynchronous on
        torch's current stream when tensors are passed."""
        def one_stamp(tv, Qk, Xk, Yk):
            return self.solve_batch(tv, Qk, virtual_var=Xk, input_var=Yk, return_mode=return_mode)
        return self._tick_batch(time_var, robot_var, virtual_var, input_var, one_stamp, given={"out": out},
                                skip=() if return_mode else ("mode",))

    def bind_batch(self, robot_var, input_var=None, virtual_var=None, out=None,
                   mode_out=None, stream=None):
        """Pre-bind device tensors and return ``tick(time_var=0.0)``: one
        kernel launch per call with no per-call tensor handling (the lean path
        for control loops, CUDA-graph capture and benchmarks).  All tensors
        must already live on the controller's device."""
        return self._bind_tick(robot_var, input_var, virtual_var, given={"out": out, "mode": mode_out})

    # -- resident ticks ----------------------------------------------------------------------------------------
    def resident_start(self, robot_var, input_var, n_ticks, time_var=0.0, out=None, mode_out=None, timeout_s=2.0,
                       stream=None, ring_depth=1, integrate_dt=0.0, max_speed=0.0, publish_ahead=0):
        """Launch ONE kernel that stays on the device and runs up to ``n_ticks`` ticks, each as soon as its ticket
        is published (include/clik.h, clik_pinv_resident_run): for closed loops whose inputs are produced on the
        device (or copied in behind a stream) every tick, at the price of a device-side hand-off instead of a launch.
        ``robot_var`` / ``input_var`` must be device tensors (the producer overwrites them in place); with
        ``ring_depth`` D > 1 they are rings ``[D, B, n]`` and tick k uses slot ``(k - 1) % D`` (outputs likewise), so
        that a producer can write the next tick's rows while this one runs.  ``integrate_dt`` > 0 keeps the state in
        the kernel: ``robot_var`` is read at tick 1 only and then stepped with ``q += clamp(dq, +-max_speed) * dt``
        after every tick (the notebooks' loop), so that only the targets ``input_var`` come from outside.  Returns a dict
        with the ``ticket`` (int32 device tensor of 64 words: [0] in_seq, [32] stop, [48] waves, [49] ticks_done),
        ``done`` (int32 device tensor, one slot per wave: the last tick that wave finished), ``waves`` per tick,
        ``out`` and ``mode`` tensors and the launch ``stream``.  The kernel
        leaves after ``n_ticks``, on ``ticket[32] != 0`` or when its poll budget (``timeout_s`` at a nominal 0.2 us per
        poll) is used up, whatever happens.  Whoever feeds it (copies, producer kernels) must use a stream that does not
        share a hardware queue with ``stream``: ``resident_feed_stream()`` hands one out (asking for another priority is
        not enough: which queue a new stream lands on depends on how many the process has made)."""
        self._require_handle()
        D = ring_depth_request(ring_depth)
        if self._feedback is not None and integrate_dt > 0.0:
            raise NotImplementedError(
                "options['velocity_feedback'] has no resident form: resident_start(integrate_dt > 0) keeps the state in "
                "the kernel and would feed nothing back (resident ticks fed by a producer are unchanged: the caller "
                "owns input_var there)")
        # (one instance may come as a 1-D device tensor: what to_device_matrix made of it here, kept)
        robot_var, input_var = (v.reshape(1, -1) if D == 1 and isinstance(v, _torch().Tensor) and v.dim() == 1 else v
                                for v in (robot_var, input_var))
        if integrate_dt > 0.0:
            # the state stays in the kernel (include/clik.h): q is read at tick 1 and stepped with
            # q += clamp(dq, +-max_speed) * integrate_dt after every tick; only input_var comes from outside
            entry, extra = "clik_pinv_resident_run_state", (float(integrate_dt), float(max_speed))
        else:
            entry, extra = "clik_pinv_resident_run", ()
        return self._resident_run(entry, robot_var, input_var, D, n_ticks, time_var, timeout_s, stream, publish_ahead,
                                  given={"out": out, "mode": mode_out}, extra=extra)

    def solve(self, time_var, robot_var, virtual_var=None, input_var=None,
              warmstart_robot_vel_var=None, warmstart_virtual_vel_var=None,
              warmstart_slack_var=None):
        """Single-instance tick with the reference's signature and return
        convention (pseudo_inverse.py:512-556): ``(robot_vel DM n x 1,
        virtual_vel DM | None, None)`` and ``self.current_mode``."""
        slot = self._solve_slot(time_var, robot_var, virtual_var, input_var)
        d = self.descriptor
        nq, nx = d.n_q, d.n_x
        self.current_mode = int(slot.out_i[0])
        cntrl_rob = cs.DM(slot.out_f[:nq].copy())
        cntrl_virt = None
        if nx and virtual_var is not None and self.skill_spec._has_virtual:
            cntrl_virt = cs.DM(slot.out_f[nq:nq + nx].copy())
        return cntrl_rob, cntrl_virt, None


    def _slot_results(self):
        d = self.descriptor
        return d.n_q + d.n_x, 1
