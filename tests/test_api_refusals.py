"""What the entry points of include/clik.h answer to a call they refuse, on host-only handles and without a handle (CPU
only): return code and clik_last_error text exactly as recorded in tests/golden/api_refusals.json by
tools/record_api_refusals.py before the host API was rewritten over a common handle base."""
import json
import os

import numpy as np
import pytest

import api_refusal_cases as arc
from casclik_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_refusals.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runner(iiwa_fk, ur5_fk):
    scratch = np.zeros(1 << 17)
    r = arc.Runner(_capi.load_library(), iiwa_fk, ur5_fk, False, scratch.ctypes.data)
    yield r
    r.close()


def test_the_table_covers_every_entry_point_with_a_handle_or_buffers():
    """every symbol of the ABI is in the table, but the queries that cannot fail (they answer 0 / "none" for a null
    handle) and clik_*_destroy"""
    infos = {s: (None, None, 0, 1, 1) for s in arc.SKILLS}
    seen = {c[3] for c in arc.cases(infos)} | {c[2] for c in arc.free_cases()}
    never_fail = {"clik_last_error", "clik_abi_version", "clik_pinv_destroy", "clik_qp_destroy", "clik_pinv_n_modes",
                  "clik_pinv_kernel_name", "clik_pinv_kernel_variant", "clik_qp_kernel_name", "clik_qp_kernel_variant",
                  "clik_qp_n_vars", "clik_qp_n_rows", "clik_qp_workspace_bytes", "clik_qp_is_box_family",
                  "clik_pinv_n_constraint_rows", "clik_qp_n_constraint_rows", "clik_summary_chunk_length",
                  "clik_pinv_summary_work_bytes", "clik_qp_summary_work_bytes"}
    assert set(_capi.exported_symbols()) - seen == never_fail


def test_host_side_refusals_are_the_recorded_ones(runner, recorded):
    got = runner.run_all(("host", "free"))
    assert sorted(got) == sorted(k for k in recorded if k.startswith(("host/", "free/")))       # (246 of them)
    wrong = {k: (v, recorded.get(k)) for k, v in got.items() if recorded.get(k) != v}
    assert not wrong, wrong


def test_host_only_handles_describe_their_skills_as_recorded(runner, recorded):
    got = runner.describe_handles(("host",))
    assert sorted(got) == ["describe/host/" + s for s in sorted(arc.SKILLS)]
    for k, v in got.items():
        assert recorded[k] == v, k
