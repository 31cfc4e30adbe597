"""Pins tests/weighted_accum_model.py (the stand-in reference of the weighted D8 accumulation and of the total upstream
length) on rasters worked by hand and against the reference's FlowAccumulation code path, and checks the exported names
and the C-ABI's argument errors, which need no GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weighted_accum_model as wm  # noqa: E402

NONE = wm.NONE
# the reference's dx / dy tables (common/constants.hpp:44-45), index = code
DX = [0, -1, -1, 0, 1, 1, 1, 0, -1]
DY = [0, 0, -1, -1, -1, 0, 1, 1, 1]


def _sum(dirs, weights, nodata, dtype=np.int32, dir_nodata=255, sum_nodata=-1):
    r = wm.weighted_sum(np.array(dirs, np.uint8), np.array(weights, dtype), nodata, dir_nodata, sum_nodata)
    assert r.dtype == (np.float64 if np.dtype(dtype).kind == "f" else np.int64)
    return r.tolist()


def _steps(dirs, dir_nodata=255):
    return wm.upstream_steps(np.array(dirs, np.uint8), dir_nodata).tolist()


def test_the_models_offsets_are_the_reference_tables():
    for code in range(1, 9):
        assert wm.OFFS[code] == (DX[code], DY[code])


def test_a_confluence_of_eight_donors():
    dirs = [[6, 7, 8], [5, 0, 1], [4, 3, 2]]                 # every neighbour points at the centre
    assert _sum(dirs, [[1, 2, 3], [4, 5, 6], [7, 8, 9]], -1) == [[1, 2, 3], [4, 45, 6], [7, 8, 9]]
    assert _steps(dirs) == [[[0, 0, 0], [0, 2, 0], [0, 0, 0]], [[0, 0, 0], [0, 2, 0], [0, 0, 0]], [[0, 0, 0], [0, 4, 0], [0, 0, 0]]]


def test_a_chain():
    dirs = [[5, 5, 5, 5, 0]]
    assert _sum(dirs, [[3, 1, 4, 1, 5]], -1, np.int16) == [[3, 4, 8, 9, 14]]
    assert _sum(dirs, [[-3, 1, -4, 1, 5]], 99, np.int8) == [[-3, -2, -6, -5, 0]]
    assert _steps(dirs) == [[[0, 1, 2, 3, 4]], [[0] * 5], [[0] * 5]]
    # 2^31 - 1 five times: past 2^32
    big = 2**31 - 1
    assert _sum(dirs, [[big] * 5], -1, np.int32) == [[big, 2 * big, 3 * big, 4 * big, 5 * big]]


def test_a_loop_of_three_cells_with_a_tributary():
    # cells 0 -> 1 -> 3 -> 0 form the loop; 5 -> 2 -> 1 is the tributary; cell 4 stands alone
    dirs = [[5, 8, 1], [3, 0, 3]]
    assert _sum(dirs, [[1, 2, 4], [8, 16, 32]], -1) == [[1, 38, 36], [8, 16, 32]]   # the loop's links carry nothing
    assert _steps(dirs) == [[[0, 1, 0], [0, 0, 0]], [[0, 1, 1], [0, 0, 0]], [[0, 0, 0], [0, 0, 0]]]


def test_a_nodata_hole():
    dirs = [[5, 5, 255, 1, 1]]                               # cells 1 and 3 point at the hole: their trees end there
    assert _sum(dirs, [[1, 2, 3, 4, 5]], -1) == [[1, 3, -1, 9, 5]]
    assert _sum(dirs, [[1, 2, 3, 4, 5]], -1, sum_nodata=-7) == [[1, 3, -7, 9, 5]]
    assert _steps(dirs) == [[[0, 1, NONE, 1, 0]], [[0, 0, NONE, 0, 0]], [[0, 0, NONE, 0, 0]]]
    # another NoData code, one that is also a direction code; codes that are no direction
    assert _sum([[5, 3, 1]], [[1, 2, 3]], 0, np.uint16, dir_nodata=3) == [[1, -1, 3]]
    assert _sum([[9, 1, 200]], [[1, 2, 3]], 0, np.uint16) == [[3, 2, 3]]
    assert _sum([[5, 5, 0]], [[1, 2, 3]], 77, np.uint8, dir_nodata=0) == [[1, 3, -1]]


def test_a_weight_nodata_cell_in_mid_chain():
    dirs = [[5, 5, 5, 0]]
    assert _sum(dirs, [[1, -9, 4, 2]], -9) == [[1, 1, 5, 7]]                         # adds nothing, passes on
    nan = float("nan")
    assert _sum(dirs, [[1.5, nan, 4.0, 2.0]], -9.0, np.float32) == [[1.5, 1.5, 5.5, 7.5]]
    assert _sum(dirs, [[1.5, -0.0, 4.0, 0.0]], 0.0, np.float64) == [[1.5, 1.5, 5.5, 5.5]]   # -0.0 == a NoData of 0.0
    assert _sum(dirs, [[1.5, nan, 4.0, 2.0]], nan, np.float64) == [[1.5, 1.5, 5.5, 7.5]]    # a NaN NoData matches nothing
    inf = float("inf")
    assert _sum(dirs, [[1.0, inf, 4.0, 2.0]], -9.0, np.float64) == [[1.0, inf, inf, inf]]


def test_an_edge_cell_that_points_inward():
    dirs = [[0, 0, 0], [5, 5, 5], [0, 0, 0]]                 # (0, 1) on the edge flows in; (2, 1) would flow off the raster
    assert _sum(dirs, [[1, 1, 1], [1, 1, 1], [1, 1, 1]], -1) == [[1, 1, 1], [1, 2, 3], [1, 1, 1]]
    assert _steps(dirs)[0] == [[0, 0, 0], [0, 1, 2], [0, 0, 0]]


def test_float_sums_are_the_correctly_rounded_true_sums():
    dirs = np.array([[5, 5, 5, 0]], np.uint8)
    w = np.array([[1e100, 1.0, -1e100, 1.0]], np.float64)
    s, k, mag = wm.weighted_sum(dirs, w, -9.0, detail=True)
    assert s.tolist() == [[1e100, 1e100, 1.0, 2.0]] and k.tolist() == [[1, 2, 3, 4]] and mag[0, 3] == 2e100


def test_the_length_is_the_flow_path_formula():
    steps = np.array([[[3, NONE]], [[2, NONE]], [[5, NONE]]], np.uint32)
    got = wm.path_length(steps, 2.0, -3.0, -1.0)
    assert got.tolist() == [[3 * 2.0 + 2 * 3.0 + 5 * math.sqrt(13.0), -1.0]]


def _random_dirs(seed, h, w):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 9, (h, w)).astype(np.uint8)
    d[rng.random((h, w)) < 0.05] = 255
    return d, rng


def test_the_model_equals_the_references_flow_accumulation(orc):
    # random codes: confluences, direction loops, NoData holes; integer-valued weights make both sides exact
    for seed, (h, w) in enumerate(((23, 31), (5, 64), (40, 7))):
        d, rng = _random_dirs(seed, h, w)
        d = wm.zero_border(d)
        wts = rng.integers(-50, 50, (h, w)).astype(np.int32)
        exp = orc.port.flow_accumulation(wm.props9(d), wts.astype(np.float64))
        got = wm.weighted_sum(d, wts, np.int32(-2**31))
        assert np.array_equal(got.astype(np.float64), exp)
        assert (got != wts)[d != 255].any()


def test_the_names_are_exported(rd):
    for name in ("d8_flow_accum_weighted", "d8_flow_accum_weighted_dev", "d8_total_upstream_length", "d8_total_upstream_length_dev"):
        assert name in rd.__all__ and callable(getattr(rd, name))


TYPES = (("i8", ctypes.c_int8, np.int8), ("u8", ctypes.c_uint8, np.uint8), ("i16", ctypes.c_int16, np.int16),
         ("u16", ctypes.c_uint16, np.uint16), ("i32", ctypes.c_int32, np.int32), ("u32", ctypes.c_uint32, np.uint32),
         ("f32", ctypes.c_float, np.float32), ("f64", ctypes.c_double, np.float64))


def test_argument_errors_need_no_gpu(rd):
    L = rd.lib()
    for suf, _, _ in TYPES:                                              # all 16 symbols
        assert hasattr(L, f"rdgpu_d8_flow_accum_weighted_{suf}") and hasattr(L, f"rdgpu_d8_flow_accum_weighted_dev_{suf}")
    for suf in ("i64", "u64"):
        assert not hasattr(L, f"rdgpu_d8_flow_accum_weighted_{suf}")
    dirs = np.zeros((4, 5), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd = ctypes.c_uint8(255)
    ARG = 2
    for suf, ct, dt in TYPES:
        flt = suf in ("f32", "f64")
        wts = np.ones((4, 5), dt)
        out = np.full((4, 5), 77, np.float64 if flt else np.int64)
        snd = ctypes.c_double(-1.0) if flt else ctypes.c_int64(-1)
        host, dev = getattr(L, f"rdgpu_d8_flow_accum_weighted_{suf}"), getattr(L, f"rdgpu_d8_flow_accum_weighted_dev_{suf}")
        wnd = ct(0)
        calls = [
            host(None, nd, p(wts), wnd, 5, 4, p(out), snd),                       # null pointers
            host(p(dirs), nd, None, wnd, 5, 4, p(out), snd),
            host(p(dirs), nd, p(wts), wnd, 5, 4, None, snd),
            host(p(dirs), nd, p(wts), wnd, 0, 4, p(out), snd),                    # sizes
            host(p(dirs), nd, p(wts), wnd, 5, -4, p(out), snd),
            host(p(dirs), nd, p(wts), wnd, 70000, 70000, p(out), snd),            # more than 0xFFFF0000 cells
            host(p(dirs), nd, p(wts), wnd, 65536, 65536, p(out), snd),
            dev(None, nd, p(wts), wnd, 5, 4, p(out), snd, None),
            dev(p(dirs), nd, None, wnd, 5, 4, p(out), snd, None),
            dev(p(dirs), nd, p(wts), wnd, 5, 4, None, snd, None),
            dev(p(dirs), nd, p(wts), wnd, 5, 0, p(out), snd, None),
            dev(p(dirs), nd, p(wts), wnd, -5, 4, p(out), snd, None),
            dev(p(dirs), nd, p(wts), wnd, 70000, 70000, p(out), snd, None),
        ]
        assert calls == [ARG] * len(calls), (suf, calls)
        assert (out == 77).all()
    steps = np.full((3, 4, 5), 77, np.uint32)
    length = np.full((4, 5), 77.0)
    host, dev = L.rdgpu_d8_total_upstream_length, L.rdgpu_d8_total_upstream_length_dev
    one, lnd = ctypes.c_double(1.0), ctypes.c_double(-1.0)
    calls = [
        host(None, nd, 5, 4, one, one, p(steps), p(length), lnd),                 # null dirs
        host(p(dirs), nd, 5, 4, one, one, None, None, lnd),                       # no output requested
        host(p(dirs), nd, 0, 4, one, one, p(steps), p(length), lnd),              # sizes
        host(p(dirs), nd, 5, -4, one, one, p(steps), p(length), lnd),
        host(p(dirs), nd, 70000, 70000, one, one, p(steps), p(length), lnd),
        host(p(dirs), nd, 5, 4, ctypes.c_double(0.0), one, p(steps), p(length), lnd),              # the cell lengths
        host(p(dirs), nd, 5, 4, one, ctypes.c_double(float("nan")), p(steps), p(length), lnd),
        host(p(dirs), nd, 5, 4, ctypes.c_double(float("inf")), one, p(steps), p(length), lnd),
        dev(None, nd, 5, 4, one, one, p(steps), p(length), lnd, None),
        dev(p(dirs), nd, 5, 4, one, one, None, None, lnd, None),
        dev(p(dirs), nd, 5, 0, one, one, p(steps), p(length), lnd, None),
        dev(p(dirs), nd, 70000, 70000, one, one, p(steps), p(length), lnd, None),
        dev(p(dirs), nd, 5, 4, one, ctypes.c_double(0.0), p(steps), p(length), lnd, None),
    ]
    assert calls == [ARG] * len(calls), calls
    assert (steps == 77).all() and (length == 77).all()
    wts = np.ones((4, 5), np.float32)
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_weighted(dirs.astype(np.int32), wts, -1.0)                   # wrong dtypes
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_weighted(dirs, wts.astype(np.int64), -1)
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_weighted(dirs, wts[:3], -1.0)                                # wrong shapes
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_accum_weighted(dirs[0], wts[0], -1.0)
    with pytest.raises(rd.RdgpuError):
        rd.d8_total_upstream_length(dirs, want=())                                    # an empty want
    with pytest.raises(rd.RdgpuError):
        rd.d8_total_upstream_length(dirs, want=("dist",))
    with pytest.raises(rd.RdgpuError):
        rd.d8_total_upstream_length(dirs, cell_x=0.0)
    with pytest.raises(rd.RdgpuError):
        rd.d8_total_upstream_length(dirs.astype(np.int16))
