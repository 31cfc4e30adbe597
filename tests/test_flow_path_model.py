"""Pins tests/flow_path_model.py (the stand-in reference of the flow-path products) on rasters worked by hand, against
tests/upslope_model.py where the two definitions meet, and checks the C-ABI's argument errors, which need no GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_path_model as fm  # noqa: E402
import stream_cases as sc  # noqa: E402
import upslope_model as um  # noqa: E402

NONE = fm.NONE
# the reference's dx / dy tables (common/constants.hpp:44-45), index = code
DX = [0, -1, -1, 0, 1, 1, 1, 0, -1]
DY = [0, 0, -1, -1, -1, 0, 1, 1, 1]


def test_the_models_offsets_are_the_reference_tables():
    for code in range(1, 9):
        assert fm.OFFS[code] == (DX[code], DY[code])
        assert fm.plane_of(code) == (0 if DY[code] == 0 else 1 if DX[code] == 0 else 2)
    assert [fm.plane_of(c) for c in range(1, 9)] == [0, 2, 1, 2, 0, 2, 1, 2]


@pytest.mark.parametrize("code", range(1, 9))
def test_one_code_on_a_5x5_raster(code):
    """every cell points the same way: the path leaves the raster after k steps, all in the plane of the code; the last
    cell inside is the drainage cell"""
    dirs = np.full((5, 5), code, np.uint8)
    r = fm.flow_path(dirs)
    dx, dy = DX[code], DY[code]
    plane = 0 if dy == 0 else 1 if dx == 0 else 2
    for y in range(5):
        for x in range(5):
            k, ex, ey = 0, x, y
            while 0 <= ex + dx < 5 and 0 <= ey + dy < 5:
                ex, ey, k = ex + dx, ey + dy, k + 1
            assert r["to_cell"][y, x] == ey * 5 + ex
            exp = [0, 0, 0]
            exp[plane] = k
            assert r["steps"][:, y, x].tolist() == exp, (code, x, y)
            assert r["dist"][y, x] == k * (math.sqrt(2.0) if plane == 2 else 1.0)


def test_a_bent_path_counts_each_plane():
    # (0,0) -> east -> (1,0) -> south-east -> (2,1) -> south -> (2,2) -> south -> (2,3): NO_FLOW
    dirs = sc.paint(sc.blank(4, 4), [(0, 0), (1, 0), (2, 1), (2, 2), (2, 3)])
    r = fm.flow_path(dirs)
    assert r["to_cell"][0, 0] == 3 * 4 + 2 and r["steps"][:, 0, 0].tolist() == [1, 2, 1]
    assert r["steps"][:, 1, 2].tolist() == [0, 2, 0] and r["steps"][:, 3, 2].tolist() == [0, 0, 0]
    assert r["to_cell"][3, 3] == 15 and r["dist"][3, 3] == 0.0          # a NO_FLOW cell drains to itself
    assert r["dist"][0, 0] == 1.0 + 2.0 + math.sqrt(2.0)
    chan = sc.mask_of((4, 4), [(2, 1)])
    r = fm.flow_path(dirs, 255, chan)
    assert r["to_cell"][0, 0] == 6 and r["steps"][:, 0, 0].tolist() == [1, 0, 1]
    assert r["to_cell"][1, 2] == 6 and r["steps"][:, 1, 2].tolist() == [0, 0, 0]
    assert r["to_cell"][2, 2] == NONE and r["steps"][:, 2, 2].tolist() == [NONE] * 3 and r["dist"][2, 2] == -1.0
    assert r["to_cell"][3, 3] == NONE                                    # NO_FLOW off the channels: no stop cell met


def test_two_cell_loop_and_a_stop_cell_on_a_loop():
    dirs = sc.blank(3, 5)
    dirs[1, 1], dirs[1, 2] = 5, 1                                        # (1,1) <-> (2,1)
    dirs[1, 0] = 5                                                       # a feeder
    dirs[1, 3] = 1                                                       # and one from the other side
    for chan in (None, np.zeros((3, 5), np.uint8)):
        r = fm.flow_path(dirs, 255, chan)
        for x in range(4):
            assert r["to_cell"][1, x] == NONE and r["dist"][1, x] == -1.0
    chan = sc.mask_of((3, 5), [(2, 1)])
    r = fm.flow_path(dirs, 255, chan)
    assert r["to_cell"][1].tolist()[:4] == [7, 7, 7, 7]                  # the stop cell breaks the loop
    assert r["steps"][0, 1].tolist()[:4] == [2, 1, 0, 1]
    assert r["to_cell"][0, 0] == NONE


def test_path_off_the_raster_and_a_nodata_target():
    dirs = np.array([[5, 5, 5], [5, 5, 255], [7, 0, 3]], np.uint8)
    r = fm.flow_path(dirs)
    assert r["to_cell"].tolist() == [[2, 2, 2], [4, 4, NONE], [6, 7, 8]]  # (2,2) points at NoData: it is the last cell
    assert r["steps"][0].tolist() == [[2, 1, 0], [1, 0, NONE], [0, 0, 0]]
    chan = np.array([[0, 1, 0], [0, 0, 1], [0, 0, 0]], np.uint8)          # (2,1) is NoData: marked, but no stop cell
    r = fm.flow_path(dirs, 255, chan)
    assert r["to_cell"].tolist() == [[1, 1, NONE], [NONE, NONE, NONE], [NONE, NONE, NONE]]
    assert r["steps"][0, 0].tolist() == [1, 0, NONE]
    # another NoData code, one that is also a direction code
    d3 = np.array([[5, 3, 1]], np.uint8)
    r = fm.flow_path(d3, 3)
    assert r["to_cell"].tolist() == [[0, NONE, 2]]


def test_dist_on_anisotropic_cells_and_signs():
    dirs = sc.paint(sc.blank(4, 4), [(0, 0), (1, 0), (2, 1), (2, 2), (2, 3)])
    diag = math.sqrt(30.0 * 30.0 + 10.5 * 10.5)
    for cell in ((30.0, 10.5), (-30.0, -10.5), (30.0, -10.5)):
        r = fm.flow_path(dirs, cell=cell, dist_nodata=-7.0)
        assert r["dist"][0, 0] == 1 * 30.0 + 2 * 10.5 + 1 * diag
        assert r["dist"][1, 2] == 2 * 10.5
    assert fm.flow_path(np.full((1, 2), 255, np.uint8), dist_nodata=-7.0)["dist"].tolist() == [[-7.0, -7.0]]


def test_hand_of_the_model():
    dirs = np.array([[5, 5, 0]], np.uint8)
    dem = np.array([[9, 4, 6]], np.int16)
    t = fm.flow_path(dirs)["to_cell"]
    assert fm.hand(dem, t, -1).tolist() == [[3.0, -2.0, 0.0]]             # not clamped
    assert fm.hand(np.array([[9, -1, 6]], np.int16), t, -1).tolist() == [[3.0, -9999.0, 0.0]]
    assert fm.hand(np.array([[9, 4, -1]], np.int16), t, -1, -5.0).tolist() == [[-5.0, -5.0, -5.0]]


@pytest.mark.parametrize("seed", range(4))
def test_without_channels_the_drainage_cell_is_the_upslope_models_outlet(seed):
    rng = np.random.default_rng(seed)
    dirs = rng.integers(0, 10, (37, 41)).astype(np.uint8)               # codes 0..9: 9 is no direction; loops are common
    dirs[rng.random(dirs.shape) < 0.05] = 255
    r = fm.flow_path(dirs)
    assert np.array_equal(r["to_cell"], um.outlets(dirs))
    assert ((r["to_cell"] == NONE) == (r["steps"][0] == NONE)).all()
    nd = int(rng.integers(1, 9))
    assert np.array_equal(fm.flow_path(dirs, nd)["to_cell"], um.outlets(dirs, nd))


def test_argument_errors_need_no_gpu(rd):
    L = rd.lib()
    dirs = np.zeros((4, 5), np.uint8)
    dem = np.zeros((4, 5), np.float32)
    out = np.full((4, 5), 77.0, np.float64)
    tc = np.full((4, 5), 77, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd, one, nodist = ctypes.c_uint8(255), ctypes.c_double(1.0), ctypes.c_double(-1.0)
    ARG = 2
    calls = [
        L.rdgpu_d8_flow_path(None, nd, 5, 4, None, one, one, p(tc), None, p(out), nodist),                       # null dirs
        L.rdgpu_d8_flow_path(p(dirs), nd, 5, 4, None, one, one, None, None, None, nodist),                       # no output
        L.rdgpu_d8_flow_path(p(dirs), nd, 0, 4, None, one, one, p(tc), None, p(out), nodist),                    # zero size
        L.rdgpu_d8_flow_path(p(dirs), nd, 5, -4, None, one, one, p(tc), None, p(out), nodist),
        L.rdgpu_d8_flow_path(p(dirs), nd, 70000, 70000, None, one, one, p(tc), None, p(out), nodist),            # too many cells
        L.rdgpu_d8_flow_path(p(dirs), nd, 5, 4, None, ctypes.c_double(0.0), one, p(tc), None, p(out), nodist),   # cell_x = 0
        L.rdgpu_d8_flow_path(p(dirs), nd, 5, 4, None, one, ctypes.c_double(float("nan")), p(tc), None, p(out), nodist),
        L.rdgpu_d8_flow_path(p(dirs), nd, 5, 4, None, ctypes.c_double(float("inf")), one, p(tc), None, p(out), nodist),
        L.rdgpu_d8_flow_path_dev(None, nd, 5, 4, None, one, one, p(tc), None, None, nodist, None),
        L.rdgpu_d8_flow_path_dev(p(dirs), nd, 5, 4, None, one, one, None, None, None, nodist, None),
        L.rdgpu_d8_flow_path_dev(p(dirs), nd, 5, 0, None, one, one, p(tc), None, None, nodist, None),
        L.rdgpu_d8_flow_path_dev(p(dirs), nd, 5, 4, None, one, ctypes.c_double(0.0), p(tc), None, None, nodist, None),
        L.rdgpu_d8_hand_f32(None, nd, p(dem), ctypes.c_float(-1), 5, 4, None, p(out), nodist),
        L.rdgpu_d8_hand_f32(p(dirs), nd, None, ctypes.c_float(-1), 5, 4, None, p(out), nodist),
        L.rdgpu_d8_hand_f32(p(dirs), nd, p(dem), ctypes.c_float(-1), 5, 4, None, None, nodist),                  # no output
        L.rdgpu_d8_hand_f32(p(dirs), nd, p(dem), ctypes.c_float(-1), 0, 4, None, p(out), nodist),
        L.rdgpu_d8_hand_dev_i16(p(dirs), nd, p(dem), ctypes.c_int16(-1), 5, 0, None, p(out), nodist, None),
        L.rdgpu_d8_hand_dev_u32(None, nd, p(dem), ctypes.c_uint32(1), 5, 4, None, p(out), nodist, None),
    ]
    assert calls == [ARG] * len(calls), calls
    assert (out == 77.0).all() and (tc == 77).all()
    for suf in ("i8", "u8", "i16", "u16", "i32", "u32", "f32", "f64"):
        assert hasattr(L, f"rdgpu_d8_hand_{suf}") and hasattr(L, f"rdgpu_d8_hand_dev_{suf}")
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_path(dirs.astype(np.int32))
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_path(dirs, want=())
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_path(dirs, want=("length",))
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_distance(dirs, channels=np.zeros((3, 3), np.uint8))
    with pytest.raises(rd.RdgpuError):
        rd.d8_flow_distance(dirs, cell=(0.0, 1.0))
    with pytest.raises(rd.RdgpuError):
        rd.d8_hand(dem.astype(np.int64), dirs, -1)
    with pytest.raises(rd.RdgpuError):
        rd.d8_hand(dem[:2], dirs, -1)
