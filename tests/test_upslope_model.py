"""The numpy model of the upslope products (tests/upslope_model.py) against the COMPILED REFERENCE's d8_upslope_cells
(tests/golden/ref_upslope.npz, tests/golden/make_golden_upslope.py): every raster bit for bit, no cell left out.  The host
function rdgpu_d8_upslope_line (no GPU call) is checked here too: it equals the model's line and the set of 2-cells of
every golden, and returns the argument error for lines that leave the raster."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from digest import load_golden  # noqa: E402
import upslope_model as um  # noqa: E402

G = load_golden(os.path.join(GOLDEN, "ref_upslope.npz"))
CASES = sorted({k.split("/")[0] for k in G})
RDGPU_ERR_ARG = 2


def _lib():
    import richdem_amd as rd

    return rd.lib()


def _c_line(w, h, x0, y0, x1, y1):
    """(return code, cells) of rdgpu_d8_upslope_line"""
    L = _lib()
    n = ctypes.c_uint32(0xDEAD)
    rc = L.rdgpu_d8_upslope_line(w, h, x0, y0, x1, y1, None, ctypes.c_uint32(0), ctypes.byref(n))
    if rc != 0:
        return rc, None
    cells = np.full(n.value + 1, 0xABCDEF, np.uint32)
    rc = L.rdgpu_d8_upslope_line(w, h, x0, y0, x1, y1, cells.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(n.value),
                                 ctypes.byref(n))
    assert cells[-1] == 0xABCDEF
    return rc, cells[:-1]


def test_the_golden_file_has_the_cases_the_engine_must_survive():
    assert len([c for c in CASES if c.startswith("fa_")]) == 24
    shapes = {G[c + "/dirs"].shape for c in CASES}
    assert {(64, 64), (129, 65), (130, 200), (37, 1), (1, 37), (257, 300)} <= shapes
    assert {"loop_in_tile", "loop_across_tiles", "noflow_nodata"} <= set(CASES)
    kinds = set()
    for c in CASES:
        for x0, y0, x1, y1 in G[c + "/lines"]:
            dx, dy = int(x1) - int(x0), int(y1) - int(y0)
            kinds.add("point" if dx == 0 and dy == 0 else "vertical" if dx == 0 else "horizontal" if dy == 0 else
                      ("swapped_" if dx < 0 else "") + ("steep" if abs(dy) > abs(dx) else "shallow") + ("_up" if dy * dx < 0 else "_down"))
    assert {"point", "vertical", "horizontal", "steep_up", "steep_down", "shallow_up", "shallow_down", "swapped_shallow_up",
            "swapped_shallow_down"} <= kinds, kinds
    assert any((G[c + "/dirs"] == 255).any() for c in CASES if c.startswith("holes_"))


@pytest.mark.parametrize("case", CASES)
def test_model_equals_the_reference(case):
    dirs, nodata = G[case + "/dirs"], int(G[case + "/nodata"])
    for i, ln in enumerate(G[case + "/lines"]):
        exp = G[f"{case}/up{i}"]
        got = um.upslope_cells(dirs, *(int(v) for v in ln), nodata=nodata)
        assert got.dtype == np.uint8 and np.array_equal(got, exp), (case, i, tuple(ln), int((got != exp).sum()))


@pytest.mark.parametrize("case", CASES)
def test_c_line_equals_the_model_and_the_references_two_cells(case):
    dirs = G[case + "/dirs"]
    h, w = dirs.shape
    for i, ln in enumerate(G[case + "/lines"]):
        ln = tuple(int(v) for v in ln)
        rc, cells = _c_line(w, h, *ln)
        assert rc == 0, (case, ln)
        assert np.array_equal(cells, um.line((h, w), *ln)), (case, ln)
        two = np.flatnonzero(G[f"{case}/up{i}"].ravel() == 2)
        assert np.array_equal(np.unique(cells), two), (case, ln)


def test_model_outlets_and_catchments_agree_with_the_reference_pour_points():
    """the basin of an outlet is what drains through it: the outlet model against the reference's pour-point rasters"""
    for case in ("frac_200x130", "holes_300x257", "noflow_nodata"):
        dirs, nodata = G[case + "/dirs"], int(G[case + "/nodata"])
        h, w = dirs.shape
        out = um.outlets(dirs, nodata)
        for i, ln in enumerate(G[case + "/lines"]):
            x0, y0, x1, y1 = (int(v) for v in ln)
            if (x0, y0) != (x1, y1) or dirs[y0, x0] == nodata or out[y0, x0] != y0 * w + x0:
                continue                                   # pour points that are outlets themselves
            assert np.array_equal(out == y0 * w + x0, G[f"{case}/up{i}"] != 255), (case, ln)


def test_line_oddities():
    assert list(um.line((10, 10), 3, 4, 3, 4)) == [43]                         # the pour point: slope NaN
    assert list(um.line((10, 10), 3, 4, 3, 8)) == [43, 44]                     # x0 == x1, y0 != y1
    assert list(um.line((10, 10), 6, 2, 2, 2)) == [22, 23, 24, 25, 26]         # swapped end points
    steep = um.line((20, 20), 2, 2, 4, 12)                                     # y moves one row per column: stops short
    assert list(steep) == [2 * 20 + 2, 2 * 20 + 3, 3 * 20 + 3, 3 * 20 + 4, 4 * 20 + 4, 4 * 20 + 5]
    for args in ((10, 10, 3, 4, 3, 4), (10, 10, 3, 4, 3, 8), (10, 10, 6, 2, 2, 2), (20, 20, 2, 2, 4, 12)):
        rc, cells = _c_line(*args)
        assert rc == 0 and np.array_equal(cells, um.line((args[1], args[0]), *args[2:]))


@pytest.mark.parametrize("args", [
    (10, 10, 0, 0, 9, 9),        # x1 = width - 1 with a final half step: (x1 + 1, y) would be marked
    (10, 10, 9, 3, 9, 7),        # x0 == x1 at the right edge: (x0 + 1, y0)
    (10, 10, -1, 3, 5, 3), (10, 10, 2, 3, 10, 3), (10, 10, 2, -1, 5, 3), (10, 10, 2, 10, 5, 3),   # an end point outside
    (10, 10, 5, 3, 2, 10),       # ... after the swap
    (10, 4, 0, 0, 8, 30),        # a steep line that walks off the bottom
    (0, 10, 0, 0, 0, 0), (10, -3, 0, 0, 0, 0),
])
def test_c_line_refuses_lines_that_leave_the_raster(args):
    w, h = args[0], args[1]
    if w > 0 and h > 0:
        assert um.line((h, w), *args[2:]) is None
    L = _lib()
    n = ctypes.c_uint32(0)
    cells = np.full(64, 0xABCDEF, np.uint32)
    rc = L.rdgpu_d8_upslope_line(*args, cells.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(64), ctypes.byref(n))
    assert rc == RDGPU_ERR_ARG
    assert (cells == 0xABCDEF).all()                                            # nothing is written


def test_c_line_capacity():
    L = _lib()
    n = ctypes.c_uint32(0)
    cells = np.full(8, 0xABCDEF, np.uint32)
    rc = L.rdgpu_d8_upslope_line(10, 10, 0, 2, 8, 2, cells.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(8), ctypes.byref(n))
    assert rc == RDGPU_ERR_ARG and n.value == 9 and (cells == 0xABCDEF).all()
    assert L.rdgpu_d8_upslope_line(10, 10, 0, 2, 8, 2, None, ctypes.c_uint32(0), None) == RDGPU_ERR_ARG


def test_python_names_are_exported():
    import richdem_amd as rd

    for name in ("d8_upslope_line", "d8_upslope_cells", "d8_catchments", "d8_outlets", "d8_upslope_cells_dev",
                 "d8_catchments_dev", "d8_outlets_dev"):
        assert callable(getattr(rd, name)) and name in rd.__all__
    assert list(rd.d8_upslope_line((10, 10), 3, 4, 3, 8)) == [43, 44]
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_line((10, 10), 0, 0, 9, 9)
