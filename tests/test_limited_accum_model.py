"""Pins tests/limited_accum_model.py (the contract of the limited D8 accumulation in Python, exact rationals) on rasters
worked by hand, against tests/weighted_accum_model.py where there is no limit, and against the reference's
MoveWaterIntoPits through tests/golden/ref_limited.npz; and checks the exported names and the C-ABI's argument errors,
which need no GPU."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limited_accum_model as lm  # noqa: E402
import weighted_accum_model as wm  # noqa: E402

NAN, INF = float("nan"), float("inf")


def _run(dirs, supply, capacity=None, factor=None, supply_nodata=-9.0, **kw):
    f = lambda a: None if a is None else np.array(a, np.float64)  # noqa: E731
    r = lm.limited(np.array(dirs, np.uint8), f(supply), supply_nodata, f(capacity), f(factor), **kw)
    return r["out"].tolist(), r["kept"].tolist(), {k: float(v) for k, v in r["result"].items()}


def test_a_chain_with_a_deficit():
    dirs = [[5, 5, 5, 0]]
    out, kept, res = _run(dirs, [[2, -2, 1, 0]])                          # filled exactly
    assert out == [[2, 0, 1, 1]] and kept == [[0, 0, 0, 0]]
    assert res == {"supplied": 1, "left": 1, "kept_pos": 0, "kept_neg": 0}
    out, kept, res = _run(dirs, [[3, -2, 1, 0]])                          # overfilled: the rest moves on
    assert out == [[3, 1, 2, 2]] and kept == [[0, 0, 0, 0]]
    assert res == {"supplied": 2, "left": 2, "kept_pos": 0, "kept_neg": 0}
    out, kept, res = _run(dirs, [[1, -2, 1, 0]])                          # underfilled: the deficit that is left
    assert out == [[1, 0, 1, 1]] and kept == [[0, -1, 0, 0]]
    assert res == {"supplied": 0, "left": 1, "kept_pos": 0, "kept_neg": -1}


def test_a_confluence_below_two_clamps():
    out, kept, res = _run([[5, 0, 1]], [[3, 0.5, 5]], capacity=[[1, INF, 2]])
    assert out == [[1, 3.5, 2]] and kept == [[2, 0, 3]]
    assert res == {"supplied": 8.5, "left": 3.5, "kept_pos": 5, "kept_neg": 0}


def test_a_capacity_of_zero_and_a_negative_one():
    for cap in (0.0, -3.0):
        out, kept, _ = _run([[5, 5, 0]], [[1, 1, 1]], capacity=[[NAN, cap, NAN]])
        assert out == [[1, 0, 1]] and kept == [[0, 2, 0]]


def test_a_factor_of_one_half():
    out, kept, res = _run([[5, 5, 0]], [[4, 0, 0]], factor=[[0.5, 0.5, 0.5]])
    assert out == [[2, 1, 0.5]] and kept == [[2, 1, 0.5]]
    assert res == {"supplied": 4, "left": 0.5, "kept_pos": 3.5, "kept_neg": 0}
    out, kept, _ = _run([[5, 5, 0]], [[4, 0, 0]], factor=[[NAN, 0.0, 2.0]])   # NaN is 1; 0 stops everything; 2 is used as given
    assert out == [[4, 0, 0]] and kept == [[0, 4, 0]]
    out, kept, _ = _run([[5, 0]], [[4, 3]], factor=[[1, 2.0]])
    assert out == [[4, 14]] and kept == [[0, -7]]
    out, kept, _ = _run([[5, 0]], [[4, 3]], factor=[[1, 2.0]], capacity=[[3, 5]])   # the factor first, then the capacity
    assert out == [[3, 5]] and kept == [[1, 1]]


def test_a_loop_of_three_cells_with_a_tributary():
    # cells 0 -> 1 -> 3 -> 0 form the loop; 5 -> 2 -> 1 is the tributary; cell 4 stands alone
    dirs = [[5, 8, 1], [3, 0, 3]]
    out, kept, res = _run(dirs, [[1, 2, 4], [8, 16, 32]])
    assert out == [[0, 0, 36], [0, 16, 32]] and kept == [[1, 38, 0], [8, 0, 0]]
    assert res == {"supplied": 63, "left": 16, "kept_pos": 47, "kept_neg": 0}
    out, kept, _ = _run(dirs, [[1, 2, 4], [8, 16, 32]], capacity=[[NAN, 0, 10], [NAN, NAN, NAN]])
    assert out == [[0, 0, 10], [0, 16, 32]] and kept == [[1, 12, 26], [8, 0, 0]]    # a loop cell's own limits play no part


def test_nodata_of_both_kinds():
    out, kept, _ = _run([[5, 5, 255, 1, 1]], [[1, 2, 3, 4, 5]], nodata_out=-7.0)
    assert out == [[1, 3, -7, 9, 5]] and kept == [[0, 0, -7, 0, 0]]
    out, kept, res = _run([[5, 5, 5, 0]], [[1.5, NAN, -0.0, 0.25]], supply_nodata=0.0)  # a NaN and -0.0 == NoData add nothing
    assert out == [[1.5, 1.5, 1.5, 1.75]] and res["supplied"] == 1.75
    out, _, _ = _run([[5, 5, 0]], [[1, 2, 3]], dir_nodata=0)
    assert out == [[1, 3, -1]]


def test_without_limits_it_is_the_weighted_sum():
    rng = np.random.default_rng(5)
    for h, w in ((23, 31), (5, 64), (40, 7)):
        d = rng.integers(0, 9, (h, w)).astype(np.uint8)
        d[rng.random((h, w)) < 0.05] = 255
        s = rng.integers(0, 50, (h, w)).astype(np.float64) / 8
        s[rng.random((h, w)) < 0.1] = -9.0
        r = lm.limited(d, s, -9.0)
        exp = wm.weighted_sum(d, s, -9.0, sum_nodata=-1.0)
        # a loop cell's out is 0 and what the sum holds there is its kept
        assert np.array_equal(np.where(r["loop"], r["kept"], r["out"]), exp)
        assert (r["kept"][~r["loop"] & (d != 255)] == 0).all() and r["loop"].any()


def test_the_model_equals_the_references_move_water_into_pits():
    seen = 0
    for name, dirs, label, tables in lm.reference_cases():
        for k, (supply, after, vol) in enumerate(tables):
            assert (supply.reshape(-1)[0] <= 0), (name, k)
            r = lm.limited(dirs, supply, np.nan)
            assert not r["loop"].any()
            assert np.array_equal(np.minimum(r["kept"], 0.0), after), (name, k)
            assert (r["kept"] <= 0).all()                                  # no capacity, no factor: nothing else is kept
            got = lm.per_label_left(r["out"], r["link"], label, vol.size)
            assert np.array_equal(got, vol), (name, k)
            seen += int((after < 0).any()) + int((vol > 0).any())
    assert seen >= 30                                                      # deficits left and water in the pits, both


def test_the_names_are_exported(rd):
    for name in ("d8_flow_accum_limited", "d8_flow_accum_limited_dev"):
        assert name in rd.__all__ and callable(getattr(rd, name))


class Result(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("supplied", "left", "kept_pos", "kept_neg")]


def test_argument_errors_need_no_gpu(rd):
    L = rd.lib()
    assert ctypes.sizeof(Result) == 32 and ctypes.sizeof(rd.api.rdgpu_limited_result) == 32
    for suf in ("i32", "u8", "i64"):
        assert not hasattr(L, f"rdgpu_d8_flow_accum_limited_{suf}")
    dirs = np.zeros((4, 5), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd, ond = ctypes.c_uint8(255), ctypes.c_double(-1.0)
    ARG = 2
    for suf, ct, dt in (("f32", ctypes.c_float, np.float32), ("f64", ctypes.c_double, np.float64)):
        host, dev = getattr(L, f"rdgpu_d8_flow_accum_limited_{suf}"), getattr(L, f"rdgpu_d8_flow_accum_limited_dev_{suf}")
        sup, cap, fac = np.ones((4, 5), dt), np.ones((4, 5), dt), np.ones((4, 5), dt)
        out, kept, res = np.full((4, 5), 77.0), np.full((4, 5), 77.0), Result(77.0, 77.0, 77.0, 77.0)
        r, snd = ctypes.byref(res), ct(0)
        calls = [
            host(None, nd, p(sup), snd, p(cap), p(fac), 5, 4, p(out), p(kept), ond, r),            # null pointers
            host(p(dirs), nd, None, snd, p(cap), p(fac), 5, 4, p(out), p(kept), ond, r),
            host(p(dirs), nd, p(sup), snd, None, None, 5, 4, None, None, ond, None),                # no output requested
            host(p(dirs), nd, p(sup), snd, None, None, 0, 4, p(out), p(kept), ond, r),              # sizes
            host(p(dirs), nd, p(sup), snd, None, None, 5, -4, p(out), p(kept), ond, r),
            host(p(dirs), nd, p(sup), snd, None, None, 70000, 70000, p(out), p(kept), ond, r),      # more than 0xFFFF0000 cells
            host(p(dirs), nd, p(sup), snd, None, None, 65536, 65536, p(out), None, ond, None),
            dev(None, nd, p(sup), snd, p(cap), p(fac), 5, 4, p(out), p(kept), ond, r, None),
            dev(p(dirs), nd, None, snd, None, None, 5, 4, p(out), p(kept), ond, r, None),
            dev(p(dirs), nd, p(sup), snd, None, None, 5, 4, None, None, ond, None, None),
            dev(p(dirs), nd, p(sup), snd, None, None, 5, 0, p(out), p(kept), ond, r, None),
            dev(p(dirs), nd, p(sup), snd, None, None, -5, 4, None, p(kept), ond, None, None),
            dev(p(dirs), nd, p(sup), snd, None, None, 70000, 70000, p(out), None, ond, r, None),
        ]
        assert calls == [ARG] * len(calls), (suf, calls)
        assert (out == 77).all() and (kept == 77).all() and [getattr(res, k) for k, _ in Result._fields_] == [77.0] * 4
        # the texts of the weighted entries where the cause is the same
        L.rdgpu_last_error.restype = ctypes.c_char_p
        for call, text in ((lambda: host(None, nd, p(sup), snd, None, None, 5, 4, p(out), None, ond, None), "null pointer"),
                           (lambda: host(p(dirs), nd, p(sup), snd, None, None, 5, 4, None, None, ond, None), "no output requested"),
                           (lambda: host(p(dirs), nd, p(sup), snd, None, None, 0, 4, p(out), None, ond, None),
                            "width and height must be positive"),
                           (lambda: dev(p(dirs), nd, p(sup), snd, None, None, 70000, 70000, p(out), None, ond, None, None),
                            "raster too large")):
            assert call() == ARG
            msg = L.rdgpu_last_error().decode()
            assert msg.endswith(": " + text) and msg.startswith("rdgpu_d8_flow_accum_limited_"), msg
    sup = np.ones((4, 5), np.float32)
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_limited(dirs.astype(np.int32), sup, -1.0)                    # wrong dtypes
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_limited(dirs, sup.astype(np.int32), -1)
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_limited(dirs, sup, -1.0, capacity=sup.astype(np.float64))    # the limits have the supply's type
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_limited(dirs, sup, -1.0, factor=sup[:3])                     # wrong shapes
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_limited(dirs, sup[:3], -1.0)
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_limited(dirs, sup, -1.0, want=("total",))
