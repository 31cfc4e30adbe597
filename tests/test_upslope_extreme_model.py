"""Pins tests/upslope_extreme_model.py (the stand-in reference of the upslope extremes) on rasters worked by hand and
against a brute-force walk of every cell's path, and checks the C-ABI's argument errors, which need no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upslope_extreme_model as xm  # noqa: E402

NONE, MAX, MIN = xm.NONE, xm.MAX, xm.MIN
# the reference's dx / dy tables (common/constants.hpp:44-45), index = code
DX = [0, -1, -1, 0, 1, 1, 1, 0, -1]
DY = [0, 0, -1, -1, -1, 0, 1, 1, 1]


def _run(dirs, values, nodata, which, dtype=None, dir_nodata=255):
    d = np.array(dirs, np.uint8)
    v = np.array(values, dtype) if dtype is not None else np.asarray(values)
    r = xm.upslope_extreme(d, v, nodata, which, dir_nodata)
    assert r["extreme"].dtype == v.dtype and r["at_cell"].dtype == np.uint32
    return r["extreme"].tolist(), r["at_cell"].tolist()


def test_the_models_offsets_are_the_reference_tables():
    for code in range(1, 9):
        assert xm.OFFS[code] == (DX[code], DY[code])


def test_a_chain_of_five():
    dirs, vals = [[5, 5, 5, 5, 0]], [[3, 1, 4, 1, 5]]
    assert _run(dirs, vals, -1, MAX, np.int16) == ([[3, 3, 4, 4, 5]], [[0, 0, 2, 2, 4]])
    assert _run(dirs, vals, -1, MIN, np.int16) == ([[3, 1, 1, 1, 1]], [[0, 1, 1, 1, 1]])   # 1 at cells 1 and 3: the lower index


def test_a_fork_with_equal_values_the_lowest_index_wins():
    # (0,0) and (2,0) flow into (1,0), which flows south into (1,1): the lowest index lies UPSTREAM of (1,1)
    dirs = [[5, 7, 1], [0, 0, 0]]
    vals = [[7, 2, 7], [1, 7, 1]]
    assert _run(dirs, vals, 255, MAX, np.uint8) == ([[7, 7, 7], [1, 7, 1]], [[0, 0, 2], [3, 0, 5]])
    # the same fork upside down: (0,1) and (2,1) flow into (1,1), which flows north into (1,0): cell 1 is DOWNSTREAM of the others
    dirs = [[0, 0, 0], [5, 3, 1]]
    vals = [[1, 7, 1], [7, 2, 7]]
    assert _run(dirs, vals, 255, MAX, np.uint8) == ([[1, 7, 1], [7, 7, 7]], [[0, 1, 2], [3, 3, 5]])
    vals = [[9, 2, 9], [2, 7, 2]]
    assert _run(dirs, vals, 255, MIN, np.uint8) == ([[9, 2, 9], [2, 2, 2]], [[0, 1, 2], [3, 3, 5]])


def test_a_two_cell_loop_with_feeders():
    dirs = [[5, 5, 1, 1]]                                    # 0 -> 1 <-> 2 <- 3
    vals = [[9, 2, 5, 1]]
    assert _run(dirs, vals, -1, MAX, np.int32) == ([[9, 9, 9, 1]], [[0, 0, 0, 3]])    # on a feeder: every loop cell gets it
    assert _run(dirs, vals, -1, MIN, np.int32) == ([[9, 1, 1, 1]], [[0, 3, 3, 3]])
    vals = [[0, 2, 5, 1]]
    assert _run(dirs, vals, -1, MAX, np.int32) == ([[0, 5, 5, 1]], [[0, 2, 2, 3]])    # on the loop: every loop cell, no feeder
    vals = [[0, 5, 5, 1]]
    assert _run(dirs, vals, -1, MAX, np.int32) == ([[0, 5, 5, 1]], [[0, 1, 1, 3]])    # a tie on the loop


def test_a_path_that_ends_at_a_nodata_direction():
    dirs = [[5, 5, 255, 1]]                                  # cells 1 and 3 point at a NoData cell: their trees end there
    vals = [[4, 6, 100, 8]]
    assert _run(dirs, vals, -1, MAX, np.int16) == ([[4, 6, -1, 8]], [[0, 1, NONE, 3]])
    assert _run(dirs, vals, -1, MIN, np.int16) == ([[4, 4, -1, 8]], [[0, 0, NONE, 3]])
    # another NoData code, one that is also a direction code; and a path off the raster
    assert _run([[5, 3, 1]], [[1, 2, 3]], 0, MAX, np.uint16, dir_nodata=3) == ([[1, 0, 3]], [[0, NONE, 2]])
    assert _run([[1, 1, 1]], [[1, 2, 3]], 0, MAX, np.uint16) == ([[3, 3, 3]], [[2, 2, 2]])
    assert _run([[9, 1, 200]], [[1, 2, 3]], 0, MAX, np.uint16) == ([[2, 2, 3]], [[1, 1, 2]])   # codes that are no direction


def test_a_nodata_value_and_a_nan_on_the_path():
    dirs = [[5, 5, 5, 5, 0]]
    nan = float("nan")
    vals = np.array([[-9999.0, nan, 2.0, -9999.0, 1.0]], np.float32)
    e, a = _run(dirs, vals, -9999.0, MAX)
    assert e == [[-9999.0, -9999.0, 2.0, 2.0, 2.0]] and a == [[NONE, NONE, 2, 2, 2]]
    e, a = _run(dirs, vals, -9999.0, MIN)
    assert e == [[-9999.0, -9999.0, 2.0, 2.0, 1.0]] and a == [[NONE, NONE, 2, 2, 4]]
    # a NaN NoData: nothing equals it, a NaN value still does not contribute, and it comes back with its bits
    nd = np.array([0x7FC01234], np.uint32).view(np.float32)[0]
    r = xm.upslope_extreme(np.array(dirs, np.uint8), vals, nd, MAX)
    assert r["at_cell"].tolist() == [[0, 0, 2, 2, 2]]
    assert r["extreme"].view(np.uint32).tolist() == [np.float32([-9999.0, -9999.0, 2.0, 2.0, 2.0]).view(np.uint32).tolist()]
    r = xm.upslope_extreme(np.array([[5, 0]], np.uint8), np.array([[nan, nan]], np.float32), nd, MIN)
    assert r["at_cell"].tolist() == [[NONE, NONE]] and r["extreme"].view(np.uint32).tolist() == [[0x7FC01234] * 2]
    # infinities are values like any other
    vals = np.array([[np.inf, -np.inf, 0.0, 3.0, 1.0]], np.float32)
    assert _run(dirs, vals, 3.0, MAX)[1] == [[0, 0, 0, 0, 0]] and _run(dirs, vals, 3.0, MIN)[1] == [[0, 1, 1, 1, 1]]


def test_minus_zero_against_plus_zero():
    dirs = [[5, 5, 0]]
    vals = np.array([[0.0, -0.0, -0.0]], np.float32)
    r = xm.upslope_extreme(np.array(dirs, np.uint8), vals, 5.0, MAX)
    assert r["at_cell"].tolist() == [[0, 0, 0]] and not np.signbit(r["extreme"]).any()          # +0 is the larger
    r = xm.upslope_extreme(np.array(dirs, np.uint8), vals, 5.0, MIN)
    assert r["at_cell"].tolist() == [[0, 1, 1]] and np.signbit(r["extreme"]).tolist() == [[False, True, True]]
    vals = np.array([[-0.0, 0.0, -0.0]], np.float32)
    r = xm.upslope_extreme(np.array(dirs, np.uint8), vals, 5.0, MAX)
    assert r["at_cell"].tolist() == [[0, 1, 1]] and np.signbit(r["extreme"]).tolist() == [[True, False, False]]
    r = xm.upslope_extreme(np.array(dirs, np.uint8), vals, 5.0, MIN)
    assert r["at_cell"].tolist() == [[0, 0, 0]] and np.signbit(r["extreme"]).all()
    # -0.0 equals a NoData of 0.0: nothing contributes, and the NoData comes back as +0
    for which in (MAX, MIN):
        r = xm.upslope_extreme(np.array(dirs, np.uint8), vals, 0.0, which)
        assert r["at_cell"].tolist() == [[NONE] * 3] and r["extreme"].view(np.uint32).tolist() == [[0, 0, 0]]


def _brute(dirs, values, nodata, which, dir_nodata=255):
    """walk every contributing cell's path and update every cell on it"""
    h, w = dirs.shape
    best = {}
    vals = values.ravel().tolist()
    for c in range(h * w):
        y, x = divmod(c, w)
        if dirs[y, x] == dir_nodata or vals[c] == nodata:
            continue
        seen = set()
        px, py = x, y
        while True:
            p = py * w + px
            if p in seen:
                break
            seen.add(p)
            b = best.get(p)
            if b is None or (vals[c] > b[0] if which == MAX else vals[c] < b[0]) or (vals[c] == b[0] and c < b[1]):
                best[p] = (vals[c], c)
            d = int(dirs[py, px])
            if not 1 <= d <= 8:
                break
            nx, ny = px + DX[d], py + DY[d]
            if not (0 <= nx < w and 0 <= ny < h) or dirs[ny, nx] == dir_nodata:
                break
            px, py = nx, ny
    ext = np.full(h * w, nodata, values.dtype)
    at = np.full(h * w, NONE, np.uint32)
    for p, (v, c) in best.items():
        ext[p], at[p] = v, c
    return ext.reshape(h, w), at.reshape(h, w)


@pytest.mark.parametrize("which", [MAX, MIN], ids=["max", "min"])
@pytest.mark.parametrize("seed", range(4))
def test_against_a_walk_of_every_path(seed, which):
    rng = np.random.default_rng(seed)
    dirs = rng.integers(0, 10, (37, 41)).astype(np.uint8)               # codes 0..9: 9 is no direction; loops are common
    dirs[rng.random(dirs.shape) < 0.05] = 255
    vals = rng.integers(0, 8, dirs.shape).astype(np.int16)              # ties everywhere; 3 is NoData
    r = xm.upslope_extreme(dirs, vals, 3, which)
    e, a = _brute(dirs, vals, 3, which)
    assert np.array_equal(r["at_cell"], a) and np.array_equal(r["extreme"], e)
    part, link = xm.links(dirs)
    loops = 0                                                            # there are loops in it
    for c in range(dirs.size):
        seen, x = set(), c
        while x >= 0 and x not in seen:
            seen.add(x)
            x = int(link[x])
        loops += x >= 0
    assert loops > 0
    nd = int(rng.integers(1, 9))
    r = xm.upslope_extreme(dirs, vals, 3, which, nd)
    e, a = _brute(dirs, vals, 3, which, nd)
    assert np.array_equal(r["at_cell"], a) and np.array_equal(r["extreme"], e)


TYPES = (("i8", ctypes.c_int8), ("u8", ctypes.c_uint8), ("i16", ctypes.c_int16), ("u16", ctypes.c_uint16), ("i32", ctypes.c_int32),
         ("u32", ctypes.c_uint32), ("f32", ctypes.c_float))


def test_argument_errors_need_no_gpu(rd):
    L = rd.lib()
    for suf, _ in TYPES:                                                 # all 14 symbols
        assert hasattr(L, f"rdgpu_d8_upslope_extreme_{suf}") and hasattr(L, f"rdgpu_d8_upslope_extreme_dev_{suf}")
    for suf in ("f64", "i64", "u64"):
        assert not hasattr(L, f"rdgpu_d8_upslope_extreme_{suf}")
    dirs = np.zeros((4, 5), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd = ctypes.c_uint8(255)
    ARG = 2
    for suf, ct in TYPES:
        dt = np.float32 if suf == "f32" else np.dtype(suf[0] + str(int(suf[1:]) // 8))
        vals = np.ones((4, 5), dt)
        ext = np.full((4, 5), 77, dt)
        at = np.full((4, 5), 77, np.uint32)
        host, dev = getattr(L, f"rdgpu_d8_upslope_extreme_{suf}"), getattr(L, f"rdgpu_d8_upslope_extreme_dev_{suf}")
        vnd = ct(0)
        calls = [
            host(None, nd, p(vals), vnd, 5, 4, 0, p(ext), p(at)),                  # null dirs
            host(p(dirs), nd, None, vnd, 5, 4, 0, p(ext), p(at)),                  # null values
            host(p(dirs), nd, p(vals), vnd, 5, 4, 1, None, None),                  # both outputs null
            host(p(dirs), nd, p(vals), vnd, 5, 4, 2, p(ext), p(at)),               # which
            host(p(dirs), nd, p(vals), vnd, 5, 4, -1, p(ext), p(at)),
            host(p(dirs), nd, p(vals), vnd, 0, 4, 0, p(ext), p(at)),               # sizes
            host(p(dirs), nd, p(vals), vnd, 5, -4, 0, p(ext), p(at)),
            host(p(dirs), nd, p(vals), vnd, 70000, 70000, 0, p(ext), p(at)),       # more than 0xFFFF0000 cells
            host(p(dirs), nd, p(vals), vnd, 65536, 65536, 0, p(ext), p(at)),
            dev(None, nd, p(vals), vnd, 5, 4, 0, p(ext), p(at), None),
            dev(p(dirs), nd, None, vnd, 5, 4, 0, p(ext), p(at), None),
            dev(p(dirs), nd, p(vals), vnd, 5, 4, 0, None, None, None),
            dev(p(dirs), nd, p(vals), vnd, 5, 4, 7, p(ext), p(at), None),
            dev(p(dirs), nd, p(vals), vnd, 5, 0, 1, p(ext), p(at), None),
            dev(p(dirs), nd, p(vals), vnd, -5, 4, 1, p(ext), p(at), None),
            dev(p(dirs), nd, p(vals), vnd, 70000, 70000, 1, p(ext), p(at), None),
        ]
        assert calls == [ARG] * len(calls), (suf, calls)
        assert (ext == 77).all() and (at == 77).all()
    vals = np.ones((4, 5), np.float32)
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs.astype(np.int32), vals, value_nodata=-1.0)          # wrong dtypes
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs, vals.astype(np.float64), value_nodata=-1.0)
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs, vals.astype(np.int64), value_nodata=-1)
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs, vals[:3], value_nodata=-1.0)                       # wrong shapes
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs[0], vals[0], value_nodata=-1.0)
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs, vals, value_nodata=-1.0, want=())                  # an empty want
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs, vals, value_nodata=-1.0, want=("where",))
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs, vals, which="largest", value_nodata=-1.0)
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_extreme(dirs, vals)                                              # no NoData given, none of its own
