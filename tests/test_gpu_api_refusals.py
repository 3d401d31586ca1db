"""What the entry points of include/clik.h answer to a call they refuse, on device handles: return code and
clik_last_error text exactly as recorded in tests/golden/api_refusals.json (tools/record_api_refusals.py --device) before
the host API was rewritten over a common handle base.  No case launches anything: the kernels attached are stand-ins, and
every pointer of a call is device memory all the same."""
import json
import os

import pytest

import api_refusal_cases as arc
from casclik_amd import _capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_refusals.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runner(iiwa_fk, ur5_fk):
    import torch
    scratch = torch.zeros(1 << 17, dtype=torch.float64, device="cuda")
    r = arc.Runner(_capi.load_library(), iiwa_fk, ur5_fk, True, scratch.data_ptr())
    yield r
    r.close()


def test_device_side_refusals_are_the_recorded_ones(runner, recorded):
    got = runner.run_all(("dev", "full"))
    got.update(runner.setup_results())
    assert sorted(got) == sorted(k for k in recorded if k.startswith(("dev/", "full/")))        # (665 of them)
    wrong = {k: (v, recorded.get(k)) for k, v in got.items() if recorded.get(k) != v}
    assert not wrong, wrong


def test_device_handles_describe_their_skills_as_recorded(runner, recorded):
    """The DevSkill record a handle uploads has no accessor in the ABI (no pointer, no size), so its bytes cannot be read
    back here.  What the library does tell about the skill a device handle holds is compared instead: the words of the
    skill image, the kernel chosen for it at four batch sizes, its sizes and the ShapeDesc text - for the plain handles and
    for the ones with an attached kernel (whose image is on the device).  None of this reads DevSkill::lds_slots or
    DevSkill::zero_token: the first sizes the LDS of every launch of the built-in pinv kernels (the suite's ticks and
    rollouts on them run with it), the second is zero because the record is cleared before it is filled."""
    got = runner.describe_handles(("dev", "full"))
    assert len(got) == 2 * len(arc.SKILLS)
    for k, v in got.items():
        assert recorded[k] == v, k
