"""CPU: what the corner-and-bound pins of tests/golden/ref_pins.npz can tell apart.

The pins are the REFERENCE's run (tests/golden/make_ref_golden.py) on states that reach the branches of its tangent-cone
tests no other fixture reaches: every corner of the joint-limit box (`*_stack_corner` part A), rows on and next to a
bound (parts B, C; `iiwa_sets1d_boundary` for the 1-D test), a task-space box left through its corners
(`iiwa_taskbox_corner`).  tests/test_refpins.py holds the oracle to them; here the oracle is given deliberately wrong
rules (`_wrong=`), and each has to lose a stated number of modes against the pinned ones - conditions on the fixture, so
that a kernel with that rule cannot pass tests/test_gpu_cone_parity.py.  The counts obtained: profiles/cone_parity.md.
`pytest -s` prints them."""
import numpy as np
import pytest

import cone_pins
from tolerances import MAX_LEFT_OUT, MODE_MARGIN


def _report(name, **counts):
    print("%s: %s" % (name, ", ".join("%s %d" % kv for kv in counts.items())))


def test_taskbox_pin_resolves_the_corner_rule():
    name = cone_pins.TASKBOX
    run, (_, mode) = cone_pins.oracle_run(name), cone_pins.pinned(name)
    got = {w: cone_pins.flips(name, "corner_" + w) for w in ("rowwise", "never", "gt", "cos40", "cos50")}
    _report(name, states=len(mode), corner=int(run["corner"].sum()), mode0=int((mode == 0).sum()),
            mode1=int((mode == 1).sum()), **got)
    assert run["corner"].sum() >= 128
    assert (mode == 0).sum() >= 64 and (mode == 1).sum() >= 64
    assert got["rowwise"] >= 64 and got["never"] >= 12 and got["cos40"] >= 8 and got["cos50"] >= 4
    assert got["gt"] >= 64
    # e is a rounded forward-kinematics value here: modes are compared where no decision is within MODE_MARGIN of
    # flipping, and that has to be (nearly) everywhere
    decided = run["margin"] > MODE_MARGIN
    assert decided.mean() >= 1.0 - MAX_LEFT_OUT
    assert np.array_equal(run["mode"][decided], mode[decided])
    print("   decided %d of %d, smallest margin %.2e" % (decided.sum(), len(mode), run["margin"].min()))


@pytest.mark.parametrize("name", cone_pins.STACK_CORNER)
def test_stack_corner_pin_resolves_the_corner_rule_and_the_rows_on_a_bound(name):
    run, (_, mode) = cone_pins.oracle_run(name), cone_pins.pinned(name)
    part = cone_pins.parts(name)
    nA = part["A"].stop
    assert run["corner"][part["A"]].all()
    got = {w: cone_pins.flips(name, "corner_" + w, part["A"]) for w in ("never", "gt", "rowwise", "cos40", "cos50")}
    _report(name + " part A", states=nA, mode0=int((mode[part["A"]] == 0).sum()), mode1=int((mode[part["A"]] == 1).sum()),
            **got)
    assert min((mode[part["A"]] == 0).sum(), (mode[part["A"]] == 1).sum()) >= nA // 4
    assert got["never"] >= nA // 4 and got["gt"] >= nA // 4
    for p in ("B", "C"):
        rows = part[p]
        got = {w: cone_pins.flips(name, w, rows) for w in ("corner_sign0_plus", "corner_sign0_minus", "multidim_loose")}
        _report(name + " part " + p, states=rows.stop - rows.start, corner=int(run["corner"][rows].sum()),
                mode0=int((mode[rows] == 0).sum()), mode1=int((mode[rows] == 1).sum()), **got)
        assert got["corner_sign0_plus"] >= 1 and got["corner_sign0_minus"] >= 1 and got["multidim_loose"] >= 1
        # (a planted row decides whether the state is a corner: both kinds are there)
        assert 0 < run["corner"][rows].sum() < rows.stop - rows.start


def test_sets1d_boundary_pin_resolves_the_1d_thresholds():
    name = "iiwa_sets1d_boundary"
    _, mode = cone_pins.pinned(name)
    got = {w: cone_pins.flips(name, w) for w in ("cone_1d_strict", "cone_eps_zero", "boundary_flipped")}
    _report(name, states=len(mode), **{"mode%d" % m: int((mode == m).sum()) for m in np.unique(mode)}, **got)
    assert got["cone_1d_strict"] >= 1 and got["cone_eps_zero"] >= 1
    assert len(np.unique(mode)) >= 2


@pytest.mark.parametrize("name", cone_pins.STACK_CORNER + (cone_pins.TASKBOX,))
def test_c_oracle_takes_the_corner_branch_as_the_reference_does(name):
    """oracle/clik_oracle_c.c has a corner rule of its own (the numpy oracle is held by tests/test_refpins.py)"""
    from oracle.c_oracle import CPinvOracle
    from tolerances import rtol_from_cond
    import refpins
    built = refpins.product_skill(name)
    Q, _, _, times = refpins.arrays(name)
    dq, _, mode = CPinvOracle(built["spec"], built["options"]).solve_batch(float(times[0]), Q)
    ref, ref_mode = cone_pins.pinned(name)
    assert np.array_equal(mode, ref_mode), np.nonzero(mode != ref_mode)[0]
    assert (refpins.rel_err(dq, ref) < rtol_from_cond(cone_pins.oracle_run(name)["kappa"])).all()


@pytest.mark.parametrize("name", cone_pins.EXACT_MODE_PINS)
def test_the_derivative_side_decides_with_room(name):
    """What makes exact mode equality a fair demand on these pins: their set expressions are the joints themselves, so
    e - bound is one exact fp64 subtraction in any correct evaluation and the comparisons with 0 and 1e-12 cannot depend
    on who made them.  Only out_dir . de, the corner ratio and de of a 1-D set are rounded - and on every state those
    stay further than MODE_MARGIN from their thresholds.  (The position side does sit ON its thresholds: that is what
    the pins are for.)"""
    run, (_, mode) = cone_pins.oracle_run(name), cone_pins.pinned(name)
    assert np.array_equal(run["mode"], mode)
    print("%s: smallest derivative-side margin %.2e, smallest margin %.2e" % (name, run["dmargin"].min(), run["margin"].min()))
    assert (run["dmargin"] > MODE_MARGIN).all(), (np.nonzero(run["dmargin"] <= MODE_MARGIN)[0], run["dmargin"].min())
    assert run["margin"].min() < 1e-11
