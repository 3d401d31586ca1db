"""Shared by tests/test_cone_pins.py (CPU) and tests/test_gpu_cone_parity.py: the fixtures of tests/golden/ref_pins.npz
that hold the tangent-cone tests (pseudo_inverse.py:162-185, :222-252) to the reference's own run at corners and bounds,
and what the oracle says about each of their states.  One oracle solve per pin, shared and never written to."""
import functools

import numpy as np

import refpins
from oracle import clik_oracle

STACK_CORNER = ("iiwa_stack_corner", "ur5_stack_corner")
# the pins whose set expressions are the joints themselves: e - bound is one exact fp64 subtraction, so modes are
# compared on EVERY state (test_the_derivative_side_decides_with_room states what makes that fair)
EXACT_MODE_PINS = ("iiwa_stack_boundary",) + STACK_CORNER + ("iiwa_sets1d_boundary",)
TASKBOX = "iiwa_taskbox_corner"


def parts(name):
    """rows of parts A, B, C of a "corner" pin (tests/golden/make_ref_golden.py::corner_states)"""
    n = refpins.PINS[name + "_Q"].shape[1]
    a = 2 ** n
    total = len(refpins.PINS[name + "_Q"])
    assert total > 2 * a
    return {"A": slice(0, a), "B": slice(a, 2 * a), "C": slice(2 * a, total)}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """-> dict of the oracle's tick on the pin's inputs: dq, mode, kappa (sum of condition numbers, the yardstick of
    tolerances.rtol_from_cond), margin (tangent_cone_margin), dmargin (its derivative side alone), corner (a decision
    of the scan met a multidimensional set with every row outside)"""
    built = refpins.product_skill(name)
    Q, Y, X, times = refpins.arrays(name)
    assert len(times) == 1 and Y is None and X is None
    B = len(Q)
    out = {"kappa": np.zeros(B), "margin": np.full(B, np.inf), "dmargin": np.full(B, np.inf),
           "corner": np.zeros(B, dtype=bool)}
    out["dq"], out["mode"] = clik_oracle.pinv_solve_batch(
        built["spec"], built["options"] or None, float(times[0]), Q, cond_out=out["kappa"], margins_out=out["margin"],
        deriv_margins_out=out["dmargin"], corner_out=out["corner"])
    for a in out.values():
        a.setflags(write=False)
    return out


def pinned(name):
    """the reference's run: (dq, mode) of the pin's single time stamp"""
    return refpins.PINS[name + "_dq"][0], refpins.PINS[name + "_mode"][0]


def flips(name, wrong, rows=slice(None)):
    """modes the oracle with the deliberate deviation `wrong` gets differently from the reference's run, on `rows`"""
    built = refpins.product_skill(name)
    Q, _, _, times = refpins.arrays(name)
    _, mode = clik_oracle.pinv_solve_batch(built["spec"], built["options"] or None, float(times[0]), Q[rows], _wrong=wrong)
    return int((mode != pinned(name)[1][rows]).sum())
