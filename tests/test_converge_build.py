"""CPU: the converging rollouts (clik_converge.hpp, jit._CONVERGE_TEMPLATE / _QP_CONVERGE_TEMPLATE) - their translation
units cross-compiled for gfx950 without scratch, one kernel each; the LDS figure and the waves per block the loaded unit
reports against the layout worked out here; the committed records; the tags of every other template untouched by the new
header; what ``converge_batch`` refuses on the host; and ``select_seeds`` against a plain loop."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from casclik_amd import _capi, jit, skills
from casclik_amd.controllers.base_controller import converge_request, converge_tolerances, select_seeds

import converge_cases as K

_OLD_TEMPLATES = ("_TEMPLATE", "_VALUE_TEMPLATE", "_QP_TEMPLATE", "_QP_VALUE_TEMPLATE", "_REC_TEMPLATE", "_VALUE_REC_TEMPLATE",
                  "_QP_REC_TEMPLATE", "_QP_VALUE_REC_TEMPLATE", "_TIME_TEMPLATE", "_MONITOR_TEMPLATE", "_SUMMARY_TEMPLATE",
                  "_ROLLSUM_TEMPLATE", "_QP_ROLLSUM_TEMPLATE", "_FUNCTION_TEMPLATE")
LDS_CAP = jit.SUMMARY_LDS_BYTES


def _unit(name):
    """(kind, descriptor, C descriptor, C options, shape initialiser, generated code, template) of a fixture's unit"""
    req = jit.unit_request(K.make(name, skills.iiwa(), skills.ur5())[1])
    assert req.eligible
    return (req.kind, req.descriptor, req.cdesc, req.copts, req.init, req.extern,
            jit.CONVERGE_UNITS["converge", req.kind]["template"])


@pytest.mark.parametrize("name", ["pose", "stack", "qp"])
def test_converging_rollout_compiles_for_gfx950_without_scratch(name):
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    kind, d, cdesc, copts, init, extern, tmpl = _unit(name)
    res = jit.unit_resources(jit.unit_text(tmpl, init, extern), init)         # (compiled as shipped)
    kernel = "qp_converge_static_kernel" if kind == "qp" else "pinv_converge_static_kernel"
    assert len(res) == 1 and all(kernel in k for k in res), sorted(res)        # (Euler only, nothing else)
    for k, r in res.items():
        assert r["ScratchSize"] == 0, (k, r)
        print(name, k[-50:], r)


def _info(so, symbol):
    fn = getattr(jit._load(so), symbol)
    fn.restype, fn.argtypes = C.c_longlong, [C.c_int]
    return fn


@pytest.mark.parametrize("name", ["pose", "stack", "qp"])
def test_lds_and_waves_are_what_the_layout_gives(name):
    """the figures of the header's constexpr functions, as the built unit reports them, against the layout of
    clik_converge.hpp worked out here: [image | tol | per wave: state and target rows] for the PseudoInverseController,
    [the QP tick's block | tol] for the ReactiveQPController (the tick's block: what the summarising rollout reports, less
    its running values)"""
    if jit._hipcc() is None:
        pytest.skip("hipcc not available")
    kind, d, cdesc, copts, init, extern, tmpl = _unit(name)
    so, _ = jit.build_shape_library(init, template=tmpl, extern=extern)
    info = _info(so, "clik_jit_converge_info")
    m_tot = sum(int(t["m"]) for t in d.tasks)
    m_set = sum(int(t["m"]) for t in d.tasks if t["cls"] == 1)
    assert info(0) == m_tot and info(1) == m_set and info(3) == 1
    tol_doubles = (m_tot + 1) & ~1
    if kind == "pinv":
        words = jit.host_image_words(_capi.load_library(), kind, cdesc, copts)
        img_doubles = ((len(words) * 8 + 1023) // 1024) * 128
        wave_doubles = (d.n_q + d.n_x + d.n_y) * 64
        lds = lambda wv: (img_doubles + tol_doubles + wv * wave_doubles) * 8       # noqa: E731
        best, best_cu = 0, 0
        for wv in range(1, 5):
            if lds(wv) <= LDS_CAP and min(LDS_CAP // lds(wv) * wv, 4) > best_cu:
                best, best_cu = wv, min(LDS_CAP // lds(wv) * wv, 4)
        assert best > 0 and info(4) == best and info(2) == lds(best), (info(4), info(2), best, lds(best))
    else:
        rs_so, _ = jit.build_shape_library(init, template=jit._QP_ROLLSUM_TEMPLATE, extern=extern)
        rs = _info(rs_so, "clik_jit_rollsum_info")
        nd = ni = 2 * m_tot + m_set
        tick_block = rs(4) - (tol_doubles + nd * 64 + ni * 32) * 8
        assert info(4) == 1 and info(2) == tick_block + tol_doubles * 8, (info(2), tick_block)
    assert info(2) <= LDS_CAP
    print(name, "LDS bytes", info(2), "waves per block", info(4))


def test_the_new_kernels_stay_in_their_own_units():
    from casclik_amd.build import CSRC
    for fn in os.listdir(CSRC):
        if fn.endswith((".hpp", ".hip")) and fn not in ("clik_converge.hpp", "clik_api.hip"):
            text = jit._code_only(open(os.path.join(CSRC, fn)).read())
            assert not any(w in text for w in ("clik_converge", "converge_t", "converge_s", "converge_i", "converge_k",
                                                "launch_converge", "launch_qp_converge", "ConvergeArgs")), fn
    api = jit._code_only(open(os.path.join(CSRC, "clik_api.hip")).read())
    assert "converge_static_kernel" not in api and "clik_converge.hpp" not in api        # entry points, no kernel
    for tmpl in _OLD_TEMPLATES:
        assert "converge" not in getattr(jit, tmpl), tmpl
    text = open(os.path.join(CSRC, "clik_converge.hpp")).read()
    assert re.findall(r'#include [<"]([^>"]+)[>"]', jit._code_only(text)) == []
    assert "atomic" not in jit._code_only(text)
    assert re.findall(r'#include "([^"]+)"', jit._CONVERGE_TEMPLATE) == ["clik_pinv_rec.hpp", "clik_summary.hpp",
                                                                         "clik_converge.hpp"]
    assert re.findall(r'#include "([^"]+)"', jit._QP_CONVERGE_TEMPLATE) == ["clik_qp_rec.hpp", "clik_summary.hpp",
                                                                            "clik_converge.hpp"]
    units = jit.CONVERGE_UNITS
    assert sorted(units) == [("converge", "pinv"), ("converge", "qp")] and not set(units) & set(jit.UNITS)
    assert units["converge", "pinv"]["refuse"] is jit._too_many_sets and units["converge", "qp"]["refuse"] is None
    assert units["converge", "pinv"]["entry"] is jit._converge_entry is units["converge", "qp"]["entry"]
    for (what, kind), unit in units.items():
        assert unit["attach"] == "clik_%s_attach_converge_kernel" % kind and unit["attach"] in _capi.exported_symbols()
        for symbol in unit["symbols"]:
            assert re.search(r'^extern "C" [\w ]+\b%s\(' % re.escape(symbol), unit["template"], re.M), symbol


def test_existing_templates_keep_their_tags(tmp_path, monkeypatch):
    """clik_converge.hpp is hashed into the tags of the two units that include it and into no other"""
    import shutil
    from casclik_amd.build import CSRC
    digest = lambda fn: hashlib.sha256(jit._code_only(open(os.path.join(CSRC, fn)).read()).encode()).hexdigest()[:12]   # noqa: E731
    mine_t = (jit._CONVERGE_TEMPLATE, jit._QP_CONVERGE_TEMPLATE)
    for tmpl in mine_t:
        assert jit._unit_stamp(tmpl) == digest("clik_summary.hpp") + digest("clik_converge.hpp")
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, str(copy), ignore=shutil.ignore_patterns("_obj"))
    stamp = jit._source_stamp()
    old = {t: jit._cache_tag("{1}", "code", False, [], getattr(jit, t)) for t in _OLD_TEMPLATES}
    old[""] = jit._cache_tag("{1}", "code", False, [], "")
    mine = {t: jit._cache_tag("{1}", "code", False, [], t) for t in mine_t}
    monkeypatch.setattr(jit, "CSRC", str(copy))
    text = open(os.path.join(CSRC, "clik_converge.hpp")).read()
    (copy / "clik_converge.hpp").write_text(text + "\nnamespace clik { constexpr int kConvergeEdited = 1; }\n")
    assert jit._source_stamp() == stamp
    for t, tag in mine.items():
        assert jit._cache_tag("{1}", "code", False, [], t) != tag
    for t, tag in old.items():
        assert jit._cache_tag("{1}", "code", False, [], getattr(jit, t) if t else "") == tag, t


def test_the_committed_records_hold_the_units_of_the_gpu_tests():
    """... and ``_records`` gives each the cache name the attach asks for, which ``prebuild_recorded`` builds"""
    tags = set(jit.recorded_tags())
    for name in ("pose", "stack", "qp", "virtual"):
        kind, d, cdesc, copts, init, extern, tmpl = _unit(name)
        assert os.path.exists(os.path.join(jit.CONVERGE_RECORDS, "req_%s.json" % jit._request_id(init, extern, False, [], tmpl))), name
        sched = jit.sched_strategy(tmpl, init)
        assert jit._cache_tag(init, extern, False, jit._sched_key(sched), tmpl) in tags, name


def test_what_the_host_refuses():
    tol, n = converge_request(1e-6, 1000, 0.0, None, 20)
    assert tol.dtype == np.float64 and tol.shape == (20,) and (tol == 1e-6).all() and n == 1000
    tol, n = converge_request(np.where(np.arange(20) < 6, 1e-4, np.inf), 0, 1e-9, np.zeros((5, 7)), 20)
    assert np.isinf(tol[6:]).all() and (tol[:6] == 1e-4).all() and n == 0
    assert (converge_tolerances(0.0, 3) == 0.0).all()
    for bad in (-1e-3, float("nan"), -np.inf, np.full(19, 1e-3), np.where(np.arange(20) == 3, -1.0, 1e-3),
                np.where(np.arange(20) == 7, np.nan, 1e-3)):
        with pytest.raises(ValueError, match="tol"):
            converge_request(bad, 10, 0.0, None, 20)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="max_ticks"):
            converge_request(1e-6, bad, 0.0, None, 20)
    for bad in (-1e-9, float("nan")):
        with pytest.raises(ValueError, match="min_step"):
            converge_request(1e-6, 10, bad, None, 20)
    with pytest.raises(ValueError, match="targets are fixed"):
        converge_request(1e-6, 10, 0.0, np.zeros((10, 5, 7)), 20)


def test_select_seeds_against_a_plain_loop():
    import torch
    S = 4
    tol = np.array([1e-3, np.inf, 0.0, 1e-2])
    #            ticks status  residual (rows: finite tol, inf tol, zero tol, finite tol)
    cases = [
        # target 0: two converged seeds tie on ticks -> the lower index (1); a faster one that failed does not count
        (3, 1, [5.0, 0, 0, 0]), (7, 0, [0, 9, 0, 0]), (7, 0, [0, 0, 0, 0]), (9, 0, [0, 0, 0, 0]),
        # target 1: the fewest ticks wins whatever its index
        (9, 0, [0, 0, 0, 0]), (8, 0, [0, 0, 0, 0]), (2, 0, [0, 0, 0, 0]), (2, 4, [np.nan] * 4),
        # target 2: none converged -> the smallest max residual / tol over rows 0 and 3 (the inf and zero rows do not
        # count): 3.0, 2.5, 2.5, NaN -> seeds 1 and 2 tie, the lower index
        (5, 1, [3e-3, 0, 0, 1e-2]), (5, 2, [1e-3, 1e9, 1e9, 2.5e-2]), (5, 3, [2.5e-3, 0, 7, 0]), (0, 4, [np.nan] * 4),
        # target 3: all non-finite -> the first
        (0, 4, [np.nan] * 4), (0, 4, [np.nan] * 4), (0, 4, [np.nan] * 4), (0, 4, [np.nan] * 4),
        # target 4: a status-4 seed is never chosen while another is left, however bad that one is
        (0, 4, [np.nan] * 4), (0, 4, [np.nan] * 4), (9, 1, [1e6, 0, 0, 1e6]), (0, 4, [np.nan] * 4),
    ]
    ticks = np.array([c[0] for c in cases], dtype=np.int32)
    status = np.array([c[1] for c in cases], dtype=np.int32)
    residual = np.array([c[2] for c in cases], dtype=np.float64)
    want = K.select_seeds_loop(ticks, status, residual, tol, S)
    assert want.tolist() == [1, 2, 1, 0, 2]
    got = select_seeds(torch.from_numpy(ticks), torch.from_numpy(status), torch.from_numpy(residual), torch.from_numpy(tol), S)
    assert got.dtype == torch.int64 and got.tolist() == want.tolist()
    # random data with many ties; no row counts when every tolerance is inf or zero: the lowest index of the best class
    rng = np.random.default_rng(0)
    for trial in range(20):
        T, S = 7, 5
        ticks = rng.integers(0, 4, T * S).astype(np.int32)
        status = rng.choice([0, 1, 1, 2, 3, 4], T * S).astype(np.int32)
        residual = np.round(rng.uniform(0, 3, (T * S, 4)), 0) * 1e-3
        residual[status == 4] = np.nan
        tol_t = tol if trial % 2 == 0 else np.array([np.inf, np.inf, 0.0, 0.0])
        got = select_seeds(torch.from_numpy(ticks), torch.from_numpy(status), torch.from_numpy(residual), tol_t, S)
        assert got.tolist() == K.select_seeds_loop(ticks, status, residual, tol_t, S).tolist(), trial
