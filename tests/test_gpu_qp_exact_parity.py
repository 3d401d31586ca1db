"""Every tick kernel of the ReactiveQPController family against the 50-digit minimiser (tests/qp_exact.py::qp_exact, held
to an independent route and to its own certificate by tests/test_qp_exact_yardstick.py), each instance held to
max(FLOOR, FACTOR u kappa_S), kappa_S = cond+(Aa H^-1 Aa') of the exact working set - tests/tolerances.py::
qp_close_exact.  On config 4 that bound has a median of 5e-12 where the old rule (kappa with the cond(H) = 1001 factor)
allows 5e-9.  Random batches, and batches of WEAKLY ACTIVE bounds (a state within 1e-11 ... 1e-5 of its bound on either
side, `qp_exact.weak_bound_cases`), cold and hot-started with a hint that holds the state in question: where a solver
that stops on a threshold shows what the threshold costs (profiles/qp_exact_parity.md, with every kernel's figures).

Each case names the kernel it means to test, asserts that this kernel serves the batch, and prints its worst figures
(`pytest -s`).  Statuses must equal the oracle's; rows the oracle reports infeasible are not compared."""
import functools

import numpy as np
import pytest

import casclik_amd as cc
import qp_exact as qe
from tolerances import LAST, U, qp_close_exact, rel_err, rtol_from_cond

pytestmark = pytest.mark.gpu

_SWITCHES = ("CLIK_NO_AOT", "CLIK_FORCE_DYNAMIC", "CLIK_JIT_DEFINES", "CLIK_JIT_VALUES")
_IMAGE = {"function_opts": {"jit_values": False}}
# variant -> (environment, controller options, what `kernel_name` must start with, what `kernel_variant` must end with
# for a cold tick of the case's batch)
_CONFIG4 = {
    "folio4": ({}, None, "qp_static_", "/v/folio4"),
    "image-aot": ({}, _IMAGE, "qp_static_", ""),
    "image-jit": ({"CLIK_NO_AOT": "1"}, _IMAGE, "jit_", ""),
    "dynamic": ({"CLIK_FORCE_DYNAMIC": "1"}, None, "dynamic", ""),
}


def _controller(case, monkeypatch, env=None, options=None):
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    ctrl = cc.ReactiveQPController(skill_spec=case.build()[0], options=None if options is None else dict(options))
    ctrl.setup_problem_functions()
    ctrl.setup_solver()
    return ctrl


def _config4_controller(case, variant, monkeypatch):
    env, options, name, label = _CONFIG4[variant]
    ctrl = _controller(case, monkeypatch, env, options)
    served = ctrl.kernel_variant(qe.B_TICK)
    assert ctrl.kernel_name.startswith(name) and served == ctrl.kernel_name + label, (variant, served)
    assert (variant == "dynamic") == (ctrl.kernel_name == "dynamic")
    return ctrl


def _tick(ctrl, case, hot_set=None, use_hot=False, pad=None):
    """one tick of the case's batch (`pad`: (Q, Y) rows launched in front of it) -> (dq, slack, status) of its rows"""
    _, t, Q, Y = case.build()
    if pad is not None:
        Q, Y = np.vstack([pad[0], Q]), np.vstack([pad[1], Y])
    dq, _, slack, status = ctrl.solve_batch(t, Q, input_var=Y, hot_set=hot_set, use_hot=use_hot)
    n = len(case.build()[2])
    return dq[-n:], slack[-n:], status[-n:]


def _figures(case, served, what, a, sol):
    tol = rtol_from_cond(sol.kappa_s)
    err = np.zeros(len(tol))
    err[sol.ok] = rel_err(a[sol.ok], (sol.dq if what == "dq" else sol.slack)[sol.ok])
    k = int(np.argmax(err / tol))
    text = ("%s through %s, %s: worst err %.2e, err / (u kappa_S) %.2f, err / bound %.3f (instance %d: err %.2e, kappa_S "
            "%.1e); %d instances, %d at the floor" % (
                case, served, what, err.max(), (err / (U * sol.kappa_s)).max(), (err / tol).max(), k, err[k],
                sol.kappa_s[k], int(sol.ok.sum()), int((sol.ok & (tol <= 1e-12)).sum())))
    if case.info is not None:
        # a weakly-active batch: the worst figure per offset
        ds = np.array([np.nan if r is None else r[4] for r in case.info])
        text += "\n     err / bound by ds: " + ", ".join(
            "%+.0e: %.3g" % (d, (err / tol)[ds == d].max()) for d in sorted(set(ds[~np.isnan(ds)])))
    print(text)
    return text


def _hold(case, served, result):
    dq, slack, status = result
    sol = case.solved()
    assert np.array_equal(status, sol.status), (case, served, np.nonzero(status != sol.status)[0][:8])
    # (enough is compared: most of a batch - or, where a case compares chosen rows only, the row it is about)
    assert sol.ok.sum() >= 0.75 * len(sol.ok) if case.only is None else sol.ok[-1]
    texts = [_figures(case, served, what, a, sol) for what, a in (("dq", dq), ("slack", slack))]
    for a, ref, text in zip((dq, slack), (sol.dq, sol.slack), texts):
        assert qp_close_exact(a, ref, sol.kappa_s, rows=sol.ok), text
        assert LAST["rule"] == "kappa_s" and LAST["left_out"] == 0 and LAST["checked"] == sol.ok.sum(), (text, dict(LAST))
    assert np.isnan(dq[sol.status != 0]).all()


def _hot_words(n):
    import torch
    return torch.zeros(n, dtype=torch.int32, device="cuda")


def _holding_hint(case, words):
    """the cold run's words with the state in question HELD at the bound it is about to meet (clik_qp_static.hpp: lower
    bounds in bits 0..15, upper bounds in bits 16..31); filler rows keep their own word"""
    import torch
    out = words.cpu().numpy().copy()
    for k, row in enumerate(case.info):
        if row is not None:
            out[k] = qe.hold_hint(out[k], row[1], row[2])
    return torch.from_numpy(out.astype(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _padding(dist):
    """rows to launch in front of a case so that the batch exceeds one block per compute unit: 64 CUs + 64 instances in
    all, beyond which a cold tick keeps the lone-wave kernel"""
    import torch
    from casclik_amd import skills
    total = 64 * torch.cuda.get_device_properties(0).multi_processor_count + 64
    return skills.synthetic_inputs(skills.iiwa(), total - qe.B_TICK, seed=4, distribution=dist)


# ---- random batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["interior", "mixed"])
@pytest.mark.parametrize("variant", ["folio4", "image-aot", "image-jit", "dynamic"])
def test_config4_cold(variant, dist, monkeypatch):
    """BASELINE config 4 through the four-strategy cold tick, the image-reading kernel from the ahead-of-time table and
    instantiated at run time, and the built-in dynamic-shape kernel (dual iteration over 13 rows)"""
    case = qe.CONFIG4[dist]
    ctrl = _config4_controller(case, variant, monkeypatch)
    _hold(case, ctrl.kernel_variant(qe.B_TICK), _tick(ctrl, case))


@pytest.mark.parametrize("dist", ["interior", "mixed"])
def test_config4_lone_wave_kernel_hot_and_cold(dist, monkeypatch):
    """the value-specialised lone-wave kernel: hot-started from the cold tick's own working sets, and cold behind padding
    (the case's rows are the last two waves and the ragged tail of a batch too large for the four-strategy kernel)"""
    case = qe.CONFIG4[dist]
    ctrl = _config4_controller(case, "folio4", monkeypatch)
    served = ctrl.kernel_variant(qe.B_TICK, hot=True)
    assert served.endswith("/v")
    hot = _hot_words(qe.B_TICK)
    _tick(ctrl, case, hot_set=hot, use_hot=False)
    _hold(case, served + " hot", _tick(ctrl, case, hot_set=hot, use_hot=True))
    pad = _padding(dist)
    served = ctrl.kernel_variant(len(pad[0]) + qe.B_TICK)
    assert served.endswith("/v")
    _hold(case, served + " cold", _tick(ctrl, case, pad=pad))


@pytest.mark.parametrize("soft_walls", [False, True])
@pytest.mark.parametrize("solver", ["mixed", "dual"])
def test_wall_skill(solver, soft_walls, monkeypatch):
    """the Moe-2016 wall skill near its walls at t = 3: the primal active set over states and general rows
    (`qp_mixed_pas`), and the dual iteration over all rows the family ran before (-DCLIK_QP_MIXED_OFF)"""
    case = qe.MOE[soft_walls]
    ctrl = _controller(case, monkeypatch, {"CLIK_JIT_DEFINES": "-DCLIK_QP_MIXED_OFF"} if solver == "dual" else None)
    assert ctrl.kernel_name.startswith("jit_") and not ctrl.value_kernel
    _hold(case, "%s (%s)" % (ctrl.kernel_variant(qe.B_TICK), solver), _tick(ctrl, case))
    if not soft_walls:
        assert (case.solved().status == 2).any()


@pytest.mark.parametrize("jit_values", [False, True])
def test_general_rows_with_and_without_the_numbers_compiled_in(jit_values, monkeypatch):
    """a hard tool-position box, a soft move and speed limits on the UR5: general rows, image-reading and
    value-specialised"""
    case = qe.BOX_MOVE
    ctrl = _controller(case, monkeypatch, options={"function_opts": {"jit_values": jit_values}})
    served = ctrl.kernel_variant(qe.B_TICK)
    assert ctrl.kernel_name.startswith("jit_") and bool(ctrl.value_kernel) == jit_values
    assert served.endswith("/v") == jit_values, served
    _hold(case, served, _tick(ctrl, case))


def test_thirty_rows_through_the_global_workspace_kernel(monkeypatch):
    """30 rows, 20 variables: the built-in kernel with its work area in global memory"""
    case = qe.MANY_ROWS
    ctrl = _controller(case, monkeypatch, {"CLIK_FORCE_DYNAMIC": "1"})
    assert ctrl.n_qp_rows == 30 and ctrl.n_qp_vars == 20 and ctrl.kernel_name == "dynamic"
    _hold(case, ctrl.kernel_variant(qe.B_TICK), _tick(ctrl, case))


# ---- weakly active bounds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["folio4", "image-aot", "dynamic"])
def test_config4_weakly_active_bounds_cold(variant, monkeypatch):
    case = qe.WEAK_CONFIG4
    ctrl = _config4_controller(case, variant, monkeypatch)
    _hold(case, ctrl.kernel_variant(qe.B_TICK), _tick(ctrl, case))


@pytest.mark.parametrize("variant", ["folio4", "image-aot"])
def test_config4_weakly_active_bounds_hot_with_the_state_held(variant, monkeypatch):
    """the normal life of a hot-started controller whose target moves away from a speed limit: the previous tick had the
    bound active, this one has the minimiser inside it by |ds| (or still on it, with a multiplier of that order)"""
    case = qe.WEAK_CONFIG4
    ctrl = _config4_controller(case, variant, monkeypatch)
    served = ctrl.kernel_variant(qe.B_TICK, hot=True)
    assert served == ctrl.kernel_name + ("/v" if variant == "folio4" else "")
    hot = _hot_words(qe.B_TICK)
    _tick(ctrl, case, hot_set=hot, use_hot=False)
    _hold(case, served + " hot, state held", _tick(ctrl, case, hot_set=_holding_hint(case, hot), use_hot=True))


@pytest.mark.parametrize("skill", ["pinned_state", "one_sided"])
def test_edge_skills_weakly_active_bounds_hot_with_the_state_held(skill, monkeypatch):
    """a state whose bounds coincide (the weak state is another one), and states with one bound only"""
    case = qe.WEAK_EDGE[skill]
    ctrl = _controller(case, monkeypatch)
    served = ctrl.kernel_variant(qe.B_TICK, hot=True)
    assert ctrl.kernel_name != "dynamic" and ctrl.value_kernel and served.endswith("/v"), served
    hot = _hot_words(qe.B_TICK)
    _tick(ctrl, case, hot_set=hot, use_hot=False)
    _hold(case, served + " hot, state held", _tick(ctrl, case, hot_set=_holding_hint(case, hot), use_hot=True))


@pytest.mark.parametrize("soft_walls", [False, True])
def test_wall_skill_weakly_active_wall(soft_walls, monkeypatch):
    """a wall moved to where the last instance of the batch is about to meet it: inactive by 1e-6 and 1e-9 of the row's
    bound, at the meeting point, active by as much.  The wall's position is a number of the skill: one controller per
    offset; cold, and hot-started from the cold tick's own working sets.  Compared: the last ten rows."""
    for ds in qe.WALL_OFFSETS:
        case = qe.WALL_WEAK[soft_walls, ds]
        ctrl = _controller(case, monkeypatch)
        assert ctrl.kernel_name.startswith("jit_") and not ctrl.value_kernel
        hot = _hot_words(qe.B_TICK)
        _hold(case, ctrl.kernel_variant(qe.B_TICK) + " cold", _tick(ctrl, case, hot_set=hot, use_hot=False))
        _hold(case, ctrl.kernel_variant(qe.B_TICK, hot=True) + " hot", _tick(ctrl, case, hot_set=hot, use_hot=True))
