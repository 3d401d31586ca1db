"""GPU: the per-tick surface of both controllers - solve_batch, bind_batch, resident_start, solve - answers the calls of
controller_call_cases.py as the commit before the tick paths moved into BaseController did
(tests/golden/controller_calls.json, written there by tools/record_controller_calls.py): the same structure for every
accepted call, the same exception for every refused one."""
import json
import os

import pytest

import controller_call_cases as ccc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "controller_calls.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env():
    return ccc.Env()


def _same(got, ref, path):
    """equal structures; the sums of float results to rounding (they are the same kernels on the same inputs)"""
    if isinstance(ref, dict):
        assert isinstance(got, dict) and set(got) == set(ref), (path, got, ref)
        for k in ref:
            if k == "abs_sum":
                assert abs(got[k] - ref[k]) <= 1e-9 * (1.0 + abs(ref[k])), (path, got[k], ref[k])
            else:
                _same(got[k], ref[k], path + "/" + k)
    elif isinstance(ref, list):
        assert isinstance(got, list) and len(got) == len(ref), (path, got, ref)
        for i, (g, r) in enumerate(zip(got, ref)):
            _same(g, r, "%s[%d]" % (path, i))
    else:
        assert got == ref and type(got) is type(ref), (path, got, ref)


def test_the_recording_holds_exactly_the_cases():
    with open(os.path.join(HERE, "golden", "controller_calls.json")) as f:
        assert sorted(json.load(f)) == sorted(cid for cid, _, _ in ccc.cases())


@pytest.mark.parametrize("group", ccc.GROUPS)
def test_calls_answer_as_recorded(env, recorded, group):
    got = json.loads(json.dumps(ccc.run_group(env, group)))      # (tuples become lists, as in the file)
    assert got
    for cid, answer in sorted(got.items()):
        ref = recorded[cid]
        if "raises" in ref:
            assert "raises" in answer, (cid, "was refused, is accepted", ref)
            assert answer["raises"][0] == ref["raises"][0], (cid, answer, ref)
            if ccc.shared_wording(cid):
                # (the pseudo-inverse controller's resident refusals adopted the wording both controllers share)
                assert answer["raises"][0] == "ValueError" and cid.split(".")[5] in answer["raises"][1], (cid, answer)
            else:
                assert answer["raises"][1] == ref["raises"][1], (cid, answer, ref)
        else:
            assert "returns" in answer, (cid, "was accepted, is refused", answer)
            _same(answer["returns"], ref["returns"], cid)


def test_one_dimensional_resident_inputs(recorded):
    """one instance as a 1-D device tensor: the pseudo-inverse controller takes it, the QP controller refuses it"""
    assert "returns" in recorded["pinv.resident.one_dimensional"]
    assert recorded["qp.resident.one_dimensional"]["raises"][0] == "ValueError"
    assert "dimensions" in recorded["qp.resident.one_dimensional"]["raises"][1]
