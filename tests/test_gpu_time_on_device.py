"""GPU: ``options["time_on_device"]`` - the time-term tables of rollouts and per-instance-time ticks filled on the device
by the skill's time kernel (clik_time.hpp, codegen.emit_time_slots) - against the host evaluator, the oracle and the same
controllers without the option."""
import ctypes as C

import numpy as np
import pytest

import casclik_amd as cc
from casclik_amd import _capi, skills
from casclik_amd.controllers.base_controller import rollout_stage_times

import time_skills
from host_loops import oracle_tick, rollout_loop
from tolerances import PINV_RTOL, QP_RTOL

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# |dev - host| <= C_ULP u (1 + |host|).  The worst ratio measured over the three skills, all times and both methods on one
# MI355X is 2.18 (profiles/time_on_device.md: the device contracts a * b + c into one rounding and evaluates sin / cos /
# exp with its own routines, the host evaluator rounds every node with libm); four times that, rounded up to a power of
# two, for other boxes and compiler releases.
C_ULP = 16.0
DT = 0.05


def _pinv(spec, on, **opts):
    ctrl = cc.PseudoInverseController(skill_spec=spec, options=dict(opts, time_on_device=on))
    ctrl.setup_problem_functions()
    return ctrl


@pytest.fixture(scope="module")
def track(ur5_fk):
    spec = time_skills.tracking_spec(ur5_fk)
    return spec, _pinv(spec, True), _pinv(spec, False)


@pytest.fixture(scope="module")
def track_qp(ur5_fk):
    spec = time_skills.track_qp_spec(ur5_fk)
    out = [spec]
    for on in (True, False):
        ctrl = cc.ReactiveQPController(skill_spec=spec, options={"time_on_device": on})
        ctrl.setup_problem_functions()
        ctrl.setup_solver()
        out.append(ctrl)
    return tuple(out)


@pytest.fixture(scope="module")
def table_ctrls(track):
    import notebook_figures
    return {"tracking": track[1], "moe": _pinv(time_skills.moe_spec(notebook_figures.moe_fk()), True),
            "mixed": _pinv(time_skills.mixed_spec(), True), "ops": _pinv(time_skills.ops_time_spec(), True)}


def _start(B, seed):
    return time_skills.UR5_HOME + np.random.default_rng(seed).normal(scale=0.1, size=(B, 6))


# ---- B1 ---------------------------------------------------------------------------------------------------------------
def _host_table(d, times, dt, method):
    return np.stack([d.time_terms(float(t)) for t in rollout_stage_times(times, dt, method)])


@pytest.mark.parametrize("name", ["tracking", "moe", "mixed", "ops"])
def test_table_equals_the_host_evaluator(table_ctrls, name):
    ctrl = table_ctrls[name]
    d = ctrl.descriptor
    rng = np.random.default_rng(7)
    worst = 0.0
    for method, stages in (("euler", 1), ("rk4", 4)):
        for n in (1, 63, 64, 65, 257):
            times = np.concatenate([rng.uniform(0.0, 30.0, size=n), time_skills.TIMES])
            dev = ctrl.time_terms_batch(times, dt=DT, method=method)
            assert isinstance(dev, np.ndarray) and dev.shape == (times.size * stages, 2 * d.n_tslots)
            host = _host_table(d, times, DT, method)         # (tick-major, stage-minor)
            assert np.isfinite(host).all()
            ratio = np.abs(dev - host) / (U * (1.0 + np.abs(host)))
            worst = max(worst, float(ratio.max()))
            print("%s %s n=%d: worst |dev - host| / (u (1 + |host|)) = %.3f" % (name, method, n, ratio.max()))
            assert (ratio <= C_ULP).all()                    # (every entry of every row)
            if stages == 4:
                rows = dev.reshape(times.size, 4, -1)
                assert np.array_equal(rows[:, 1], rows[:, 2])
                assert np.array_equal(rows[:, 0], ctrl.time_terms_batch(times)), "stage 0 is the tick's own time"
    print("%s: worst ratio %.3f" % (name, worst))


@pytest.mark.parametrize("t", time_skills.TIMES_BEYOND_THE_FAST_RANGE)
def test_table_beyond_the_straight_line_range_of_sincos_joint(table_ctrls, t):
    """0.1 t = +-2e5 rad: `TimeSlots` takes the library path of sincos_joint (|x| > 1e5), under the same bound; alone,
    among ordinary times (the branch is per lane) and at the four stages of an rk4 tick"""
    ctrl = table_ctrls["tracking"]
    d = ctrl.descriptor
    assert abs(0.1 * t) > 1e5
    for times in (np.array([t]), np.concatenate([time_skills.TIMES[:31], [t], time_skills.TIMES[31:], [t + 0.25]])):
        for method, stages in (("euler", 1), ("rk4", 4)):
            dev = ctrl.time_terms_batch(times, dt=DT, method=method)
            host = _host_table(d, times, DT, method)
            assert dev.shape == host.shape == (times.size * stages, 2 * d.n_tslots) and np.isfinite(host).all()
            ratio = np.abs(dev - host) / (U * (1.0 + np.abs(host)))
            print("tracking t=%g %s n=%d: worst |dev - host| / (u (1 + |host|)) = %.3f" % (t, method, times.size, ratio.max()))
            assert (ratio <= C_ULP).all()
    assert np.abs(_host_table(d, np.array([t]), DT, "euler")).max() > 0.1       # (the slots are not all zero there)


# ---- B2 ---------------------------------------------------------------------------------------------------------------
def test_table_is_deterministic_and_keeps_the_container(table_ctrls):
    import torch
    ctrl = table_ctrls["mixed"]
    times = np.concatenate([np.random.default_rng(9).uniform(0.0, 30.0, size=301), time_skills.TIMES])
    for method in ("euler", "rk4"):
        a = ctrl.time_terms_batch(times, dt=DT, method=method)
        b = ctrl.time_terms_batch(times, dt=DT, method=method)
        h = times.size // 2
        halves = np.concatenate([ctrl.time_terms_batch(times[:h], dt=DT, method=method),
                                 ctrl.time_terms_batch(times[h:], dt=DT, method=method)])
        assert isinstance(a, np.ndarray) and np.array_equal(a, b) and np.array_equal(a, halves)
        t_dev = torch.from_numpy(times).to(ctrl._device)
        c = ctrl.time_terms_batch(t_dev, dt=DT, method=method)
        assert isinstance(c, torch.Tensor) and c.device == ctrl._device and c.dtype == torch.float64
        assert np.array_equal(c.cpu().numpy(), a)
    assert ctrl.time_terms_batch(np.zeros(0)).shape == (0, 2 * ctrl.descriptor.n_tslots)


# ---- B3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_rollout_with_device_time(track, method):
    import torch
    spec, on, off = track
    assert on._time_kernel and off._time_kernel is None and on.kernel_name == off.kernel_name
    Q = _start(70, 8)
    n_ticks, vmax = 6, 0.4
    times = 3.0 + DT * np.arange(n_ticks)
    q_on, dq_on, mode_on = on.rollout_batch(times, Q, dt=DT, max_speed=vmax, method=method)
    orc = rollout_loop(oracle_tick(spec, False), False, times, Q, None, lambda i: None, DT, vmax, rk4=method == "rk4")[-1]
    qo, vo = orc["q"], orc["dq"]
    print("%s: against the oracle loop |q| %.3g |dq| %.3g" % (method, np.abs(q_on - qo).max(), np.abs(dq_on - vo).max()))
    assert np.abs(q_on - qo).max() < 1e-9 and np.abs(dq_on - vo).max() < 1e-8
    q_off, dq_off, mode_off = off.rollout_batch(times, Q, dt=DT, max_speed=vmax, method=method)
    print("%s: against the option off |q| %.3g |dq| %.3g" % (method, np.abs(q_on - q_off).max(), np.abs(dq_on - dq_off).max()))
    assert np.abs(q_on - q_off).max() < 1e-10 and np.abs(dq_on - dq_off).max() < 1e-9
    assert np.array_equal(mode_on, mode_off)
    # the times as a device tensor: used in place, same bits
    q_t, dq_t, mode_t = on.rollout_batch(torch.from_numpy(times).to(on._device), Q, dt=DT, max_speed=vmax, method=method)
    assert np.array_equal(q_t, q_on) and np.array_equal(dq_t, dq_on) and np.array_equal(mode_t, mode_on)
    with pytest.raises(ValueError):
        on.rollout_batch(times, Q, dt=DT, method="heun")


# ---- B4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_qp_rollout_with_device_time(track_qp, method):
    spec, on, off = track_qp
    assert on._time_kernel and off._time_kernel is None
    Q = _start(70, 21)
    times = 1.0 + DT * np.arange(6)
    a = on.rollout_batch(times, Q, dt=DT, max_speed=0.5, method=method)
    b = off.rollout_batch(times, Q, dt=DT, max_speed=0.5, method=method)
    assert (a[3] == 0).all() and np.array_equal(a[3], b[3])
    for got, ref in ((a[0], b[0]), (a[1], b[1])):
        assert np.allclose(got, ref, rtol=QP_RTOL, atol=QP_RTOL * max(1.0, np.abs(ref).max()))


# ---- B5 ---------------------------------------------------------------------------------------------------------------
def test_recording_rollout_with_device_time(track):
    spec, on, off = track
    Q = _start(70, 8)
    n_ticks, k, vmax = 8, 2, 0.4
    times = 3.0 + DT * np.arange(n_ticks)
    q, dq, mode, rec = on.rollout_batch(times, Q, dt=DT, max_speed=vmax, record_every=k)
    assert set(rec) == {"q", "dq", "mode"}
    assert rec["q"].shape == (n_ticks // k, 70, 6) and rec["dq"].shape == (n_ticks // k, 70, 6)
    assert rec["mode"].shape == (n_ticks // k, 70)
    assert np.array_equal(rec["q"][-1], q) and np.array_equal(rec["dq"][-1], dq) and np.array_equal(rec["mode"][-1], mode)
    q0, dq0, mode0, rec0 = off.rollout_batch(times, Q, dt=DT, max_speed=vmax, record_every=k)
    assert np.abs(rec["q"] - rec0["q"]).max() < 1e-10 and np.abs(rec["dq"] - rec0["dq"]).max() < 1e-9
    assert np.array_equal(rec["mode"], rec0["mode"])
    assert np.abs(q - q0).max() < 1e-10 and np.abs(dq - dq0).max() < 1e-9


# ---- B6 ---------------------------------------------------------------------------------------------------------------
def test_per_instance_times_from_the_device(track):
    import torch
    from oracle import clik_oracle as orc
    spec, on, off = track
    rng = np.random.default_rng(12)
    Q = time_skills.UR5_HOME + rng.normal(scale=0.1, size=(97, 6))
    times = rng.uniform(0.0, 30.0, size=97)
    dq, _, mode = on.solve_batch(times, Q)
    for b in range(97):
        rdq, rmode = orc.pinv_solve_batch(spec, None, float(times[b]), Q[b:b + 1])
        assert mode[b] == rmode[0]
        assert np.allclose(dq[b], rdq[0], rtol=PINV_RTOL, atol=PINV_RTOL * max(1.0, np.abs(rdq).max()))
    dq_t, _, mode_t = on.solve_batch(torch.from_numpy(times).to(on._device), Q)
    assert np.array_equal(dq_t, dq) and np.array_equal(mode_t, mode)
    with pytest.raises(ValueError):
        on.solve_batch(times[:5], Q)
    with pytest.raises(ValueError):
        on.solve_batch(torch.from_numpy(times[:5]).to(on._device), Q)
    # one stamp for the batch keeps the host evaluator: the same bits as without the option
    assert np.array_equal(on.solve_batch(4.0, Q)[0], off.solve_batch(4.0, Q)[0])


def test_per_instance_times_from_the_device_qp(track_qp):
    import torch
    from oracle import clik_oracle as orc
    spec, on, off = track_qp
    rng = np.random.default_rng(13)
    Q = time_skills.UR5_HOME + rng.normal(scale=0.1, size=(70, 6))
    times = rng.uniform(0.0, 30.0, size=70)
    dq, _, sl, status = on.solve_batch(times, Q)
    assert (status == 0).all()
    for b in range(0, 70, 3):
        rdq = orc.qp_solve_batch(spec, float(times[b]), Q[b:b + 1])[0]
        assert np.allclose(dq[b], rdq[0], rtol=QP_RTOL, atol=QP_RTOL * max(1.0, np.abs(rdq).max()))
    dq_t, _, _, status_t = on.solve_batch(torch.from_numpy(times).to(on._device), Q)
    assert np.array_equal(dq_t, dq) and np.array_equal(status_t, status)
    with pytest.raises(ValueError):
        on.solve_batch(times[:5], Q)


# ---- B7 ---------------------------------------------------------------------------------------------------------------
def test_c_abi_edges(track, iiwa_fk):
    import torch
    spec, on, off = track
    lib = on._lib
    dev = on._device
    n_ts = on.descriptor.n_tslots
    t = torch.zeros(8, dtype=torch.float64, device=dev)
    out = torch.full((8 * 4, 2 * n_ts), -7.0, dtype=torch.float64, device=dev)
    tp, op = C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())
    with torch.cuda.device(dev):
        # no time kernel attached (the controller without the option)
        assert lib.clik_pinv_time_terms(off._handle, 8, tp, 1, 0.0, op, None) == _capi.CLIK_EUNSUPPORTED
        assert b"time kernel" in lib.clik_last_error()
        assert lib.clik_pinv_time_terms(on._handle, 8, tp, 3, 0.0, op, None) == _capi.CLIK_EINVAL
        assert b"stages" in lib.clik_last_error()
        assert lib.clik_pinv_time_terms(on._handle, -1, tp, 1, 0.0, op, None) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_time_terms(on._handle, 8, None, 1, 0.0, op, None) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_time_terms(on._handle, 8, tp, 1, 0.0, None, None) == _capi.CLIK_EINVAL
        assert lib.clik_pinv_time_terms(on._handle, 0, tp, 1, 0.0, op, None) == _capi.CLIK_OK
        torch.cuda.synchronize()
        assert (out == -7.0).all()              # (none of the calls above wrote anything)
        Q = torch.from_numpy(_start(16, 2)).to(dev)
        dq = torch.empty_like(Q)
        mode = torch.empty(16, dtype=torch.int32, device=dev)
        args = lambda q: (16, 2, 0, DT, 0.4, None, C.c_void_p(q.data_ptr()), None, None,      # noqa: E731
                          C.c_void_p(dq.data_ptr()), None, C.c_void_p(mode.data_ptr()), None)
        none5 = (0, 0, None, None, None, None, None)
        q1 = Q.clone()
        assert lib.clik_pinv_rollout_batch_dev(on._handle, *args(q1), *none5) == _capi.CLIK_EINVAL
        assert b"times" in lib.clik_last_error()
        assert lib.clik_pinv_rollout_batch_dev(off._handle, *args(q1)[:5], tp, *args(q1)[6:], *none5) == \
            _capi.CLIK_EUNSUPPORTED
        torch.cuda.synchronize()
        assert torch.equal(q1, Q)
    # a skill without time slots: times = NULL is accepted, the result is clik_pinv_rollout_batch_m's
    sctrl = _pinv(skills.stack_skill(iiwa_fk), False, **skills.STACK_OPTIONS)
    assert sctrl.descriptor.n_tslots == 0
    Qn, Yn = skills.synthetic_inputs(iiwa_fk, 64, seed=5, distribution="mixed")
    sdev = sctrl._device
    Y = torch.from_numpy(Yn).to(sdev)
    res = []
    with torch.cuda.device(sdev):
        for fn, tail in ((lib.clik_pinv_rollout_batch_m, ()), (lib.clik_pinv_rollout_batch_dev, none5)):
            q = torch.from_numpy(Qn).to(sdev)
            dq = torch.empty_like(q)
            mode = torch.empty(64, dtype=torch.int32, device=sdev)
            rc = fn(sctrl._handle, 64, 4, 0, 0.008, 0.6, None, C.c_void_p(q.data_ptr()), None, C.c_void_p(Y.data_ptr()),
                    C.c_void_p(dq.data_ptr()), None, C.c_void_p(mode.data_ptr()), None, *tail)
            assert rc == 0, lib.clik_last_error()
            torch.cuda.synchronize()
            res.append((q.cpu().numpy(), dq.cpu().numpy(), mode.cpu().numpy()))
        assert lib.clik_pinv_time_terms(sctrl._handle, 8, None, 1, 0.0, None, None) == _capi.CLIK_OK
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- B8 ---------------------------------------------------------------------------------------------------------------
def test_a_skill_without_time_slots_is_untouched(iiwa_fk):
    spec = skills.stack_skill(iiwa_fk)
    plain = _pinv(spec, False, **skills.STACK_OPTIONS)
    with_opt = _pinv(spec, True, **skills.STACK_OPTIONS)
    after = _pinv(spec, False, **skills.STACK_OPTIONS)
    assert with_opt._time_kernel is None and with_opt.descriptor.n_tslots == 0
    assert plain.kernel_name == with_opt.kernel_name == after.kernel_name
    assert plain.kernel_variant(64) == with_opt.kernel_variant(64) == after.kernel_variant(64)
    Q, Y = skills.synthetic_inputs(iiwa_fk, 64, seed=5, distribution="mixed")
    ref = plain.rollout_batch(np.zeros(4), Q, input_var=Y, dt=0.008, max_speed=0.6)
    for ctrl in (with_opt, after):
        got = ctrl.rollout_batch(np.zeros(4), Q, input_var=Y, dt=0.008, max_speed=0.6)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
    assert with_opt.time_terms_batch(np.zeros(5)).shape == (5, 0)
    with pytest.raises(NotImplementedError, match="time_on_device"):
        after.time_terms_batch(np.zeros(5))


def test_the_option_without_a_kernel_is_refused(ur5_fk):
    """function_opts["jit"] false: no kernel may be instantiated, and there is no silent return to the host path"""
    spec = time_skills.tracking_spec(ur5_fk)
    ctrl = cc.PseudoInverseController(skill_spec=spec, options={"time_on_device": True, "function_opts": {"jit": False}})
    with pytest.raises(NotImplementedError, match="instantiated"):
        ctrl.setup_problem_functions()
