"""CPU: the marshalling of recording / per-tick-target rollouts that lives in BaseController's module (shapes, the
number of records, errors) and the C ABI's side of it (symbols declared and exported)."""
import os
import re

import numpy as np
import pytest

from casclik_amd import _capi
from casclik_amd.controllers.base_controller import per_tick_input, record_layout, rollout_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clik_pinv_rollout_batch_rec", "clik_qp_rollout_batch_rec", "clik_pinv_attach_rec_kernel",
       "clik_qp_attach_rec_kernel"]


def test_number_of_records():
    assert rollout_records(11, None) is None
    assert rollout_records(11, 1) == 11
    assert rollout_records(11, 4) == 2          # (ticks 4 and 8; 9, 10, 11 are not recorded)
    assert rollout_records(12, 4) == 3
    assert rollout_records(11, 12) == 0         # (k > n_ticks: arrays with zero records)
    assert rollout_records(0, 3) == 0
    assert rollout_records(8, np.int64(2)) == 4


@pytest.mark.parametrize("bad", [0, -1, 2.0, "2", True])
def test_record_every_must_be_a_positive_int(bad):
    with pytest.raises(ValueError, match="record_every"):
        rollout_records(10, bad)


def test_per_tick_input_is_told_by_its_shape():
    assert per_tick_input(None, 5, 7) is False
    assert per_tick_input(np.zeros((3, 7)), 5, 7) is False        # ([B, n_y]: what it meant before)
    assert per_tick_input(np.zeros(7), 5, 7) is False
    assert per_tick_input(np.zeros((5, 7)), 5, 7) is False        # (B == n_ticks is still a 2-D input)
    assert per_tick_input(np.zeros((5, 3, 7)), 5, 7) is True
    assert per_tick_input([[[0.0] * 7] * 3] * 5, 5, 7) is True    # (nested lists count by their shape too)
    with pytest.raises(ValueError, match="4 records, the rollout 5 ticks"):
        per_tick_input(np.zeros((4, 3, 7)), 5, 7)
    with pytest.raises(ValueError, match="7 columns"):
        per_tick_input(np.zeros((5, 3, 6)), 5, 7)


def test_record_layout():
    fields = [("q", 7, "float64"), ("dq", 7, "float64"), ("x", 0, "float64"), ("dx", 0, "float64"),
              ("slack", 3, "float64"), ("status", None, "int32")]
    lay = record_layout(fields, 2, 100)
    assert lay == {"q": ((2, 100, 7), "float64"), "dq": ((2, 100, 7), "float64"), "slack": ((2, 100, 3), "float64"),
                   "status": ((2, 100), "int32")}
    assert list(lay) == ["q", "dq", "slack", "status"]
    assert record_layout(fields, 0, 5)["q"][0] == (0, 5, 7)


def test_new_entry_points_are_declared_and_listed():
    with open(os.path.join(ROOT, "include", "clik.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _capi.exported_symbols()
    # each _rec takes the arguments of _m and then y_per_tick, record_every and the record pointers
    for ctrl in ("pinv", "qp"):
        m = re.search(r"^int clik_%s_rollout_batch_m\((.*?)\);" % ctrl, header, re.M | re.S).group(1)
        rec = re.search(r"^int clik_%s_rollout_batch_rec\((.*?)\);" % ctrl, header, re.M | re.S).group(1)
        norm = lambda s: re.sub(r"\s+", " ", s).strip()     # noqa: E731
        assert norm(rec).startswith(norm(m) + ", int32_t y_per_tick, int32_t record_every, double* rec_q")


def test_new_entry_points_are_exported():
    lib = _capi.load_library()
    for name in NEW:
        assert getattr(lib, name) is not None
    # a null handle is refused, not dereferenced
    assert lib.clik_pinv_rollout_batch_rec(None, 1, 1, 0, 0.1, 0.0, None, None, None, None, None, None, None, None,
                                           0, 1, None, None, None, None, None) == _capi.CLIK_EINVAL
    assert lib.clik_qp_rollout_batch_rec(None, 1, 1, 0, 0.1, 0.0, None, None, None, None, None, None, None, None, None,
                                         0, 1, None, None, None, None, None, None) == _capi.CLIK_EINVAL
