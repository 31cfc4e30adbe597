"""Pins tests/longest_path_model.py (the stand-in reference of the longest upstream flow path) on rasters worked by hand
and against a brute-force walk of every path that compares the TRUE lengths of the step triples (exact arithmetic, no
rounding), checks that on_basin_path marks exactly the walk from the outlet's head down to the outlet, and checks the
C-ABI's argument errors and the exported names, which need no GPU."""
import ctypes
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longest_path_model as lm  # noqa: E402
from flow_path_model import NONE, OFFS, plane_of  # noqa: E402

S2 = math.sqrt(2.0)


def _run(dirs, cell=(1.0, 1.0), nodata=255, length_nodata=-1.0):
    r = lm.longest_flow_path(np.array(dirs, np.uint8), nodata, cell, length_nodata)
    assert r["from_cell"].dtype == np.uint32 and r["steps"].dtype == np.uint32 and r["length"].dtype == np.float64
    assert r["on_basin_path"].dtype == np.uint8
    return r


def test_a_y_of_two_unequal_tributaries():
    # 0 -> 1 -> 2 -> south to 7 <- north from 12; 7 -> 8 -> 9; everything else is a lone outlet
    dirs = [[5, 5, 7, 0, 0],
            [0, 0, 5, 5, 0],
            [0, 0, 3, 0, 0]]
    r = _run(dirs)
    assert r["from_cell"].tolist() == [[0, 0, 0, 3, 4], [5, 6, 0, 0, 0], [10, 11, 12, 13, 14]]
    assert r["length"].tolist() == [[0, 1, 2, 0, 0], [0, 0, 3, 4, 5], [0, 0, 0, 0, 0]]
    assert r["steps"][0].tolist() == [[0, 1, 2, 0, 0], [0, 0, 2, 3, 4], [0, 0, 0, 0, 0]]
    assert r["steps"][1].tolist() == [[0, 0, 0, 0, 0], [0, 0, 1, 1, 1], [0, 0, 0, 0, 0]]
    assert not r["steps"][2].any()
    assert r["on_basin_path"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 0, 1, 1]]   # the short tributary is off it
    r = _run(dirs, cell=(-2.0, 0.5))                      # the sign of a cell length is ignored
    assert r["length"].tolist() == [[0, 2, 4, 0, 0], [0, 0, 4.5, 6.5, 8.5], [0, 0, 0, 0, 0]]


def test_equal_tributaries_the_lowest_index_wins():
    # 5 -> 6 -> 7 <- 8 <- 9, 2 south to 7, 7 south to 12: cells 5 and 9 are both 3 away from the outlet
    dirs = [[0, 0, 7, 0, 0],
            [5, 5, 7, 1, 1],
            [0, 0, 0, 0, 0]]
    r = _run(dirs)
    assert r["from_cell"].tolist() == [[0, 1, 2, 3, 4], [5, 5, 5, 9, 9], [10, 11, 5, 13, 14]]
    assert r["length"].tolist() == [[0, 0, 0, 0, 0], [0, 1, 2, 1, 0], [0, 0, 3, 0, 0]]
    assert r["on_basin_path"].tolist() == [[1, 1, 0, 1, 1], [1, 1, 1, 0, 0], [1, 1, 1, 1, 1]]
    # upside down: the outlet is cell 2, the tie is between 5 and 9 again, and cell 12 is a head of its own
    r = _run([[0, 0, 0, 0, 0], [5, 5, 3, 1, 1], [0, 0, 3, 0, 0]])
    assert r["from_cell"].tolist() == [[0, 1, 5, 3, 4], [5, 5, 5, 9, 9], [10, 11, 12, 13, 14]]
    assert r["on_basin_path"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 0, 0], [1, 1, 0, 1, 1]]


def test_a_diagonal_against_an_orthogonal_detour():
    # into the outlet 8: 0 -> 4 -> 8 along the diagonal (2 sqrt 2), 1 -> 2 -> 5 -> 8 round the corner (3), 6 -> 7 -> 8 (2)
    dirs = [[6, 5, 7],
            [0, 6, 7],
            [5, 5, 0]]
    r = _run(dirs)
    assert r["from_cell"].tolist() == [[0, 1, 1], [3, 0, 1], [6, 6, 1]]
    assert r["length"].tolist() == [[0, 0, 1], [0, S2, 2], [0, 1, 3]]
    assert r["steps"][:, 2, 2].tolist() == [1, 2, 0] and r["steps"][:, 1, 1].tolist() == [0, 0, 1]
    assert r["on_basin_path"].tolist() == [[0, 1, 1], [1, 0, 1], [0, 0, 1]]
    # without the detour's first cell the two diagonal steps win against two orthogonal ones, though the counts are equal
    dirs[0][1] = 0
    r = _run(dirs)
    assert r["from_cell"][2, 2] == 0 and r["length"][2, 2] == 2 * S2 and r["steps"][:, 2, 2].tolist() == [0, 0, 2]
    assert r["on_basin_path"].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]]


def test_cell_3_by_4_where_3_plus_4_ties_with_the_diagonal():
    # diag = 5 exactly: two diagonal steps (0 -> 6 -> 12) and 2 x + 1 y (9 -> 14 -> 13 -> 12) are both 10 long
    dirs = [[6, 0, 0, 0, 0],
            [0, 6, 0, 0, 7],
            [0, 0, 0, 1, 1]]
    for cell in ((3.0, 4.0), (-3.0, 4.0), (3.0, -4.0)):
        r = _run(dirs, cell)
        assert r["from_cell"][2, 2] == 0 and r["length"][2, 2] == 10.0 and r["steps"][:, 2, 2].tolist() == [0, 0, 2]
        assert r["from_cell"][2, 3] == 9 and r["length"][2, 3] == 7.0
        assert r["on_basin_path"][1, 1] == 1 and r["on_basin_path"][2, 3] == 0
    # upside down the orthogonal branch has the lower index
    dirs = [[0, 0, 0, 1, 1],
            [0, 4, 0, 0, 3],
            [4, 0, 0, 0, 0]]
    r = _run(dirs, (3.0, 4.0))
    assert r["from_cell"][0, 2] == 9 and r["length"][0, 2] == 10.0 and r["steps"][:, 0, 2].tolist() == [2, 1, 0]
    assert r["on_basin_path"][1, 1] == 0 and r["on_basin_path"][0, 3] == 1
    r = _run(dirs, (4.0, 3.0))                            # no tie any more: 2 x + 1 y is 11
    assert r["from_cell"][0, 2] == 9 and r["length"][0, 2] == 11.0


def test_nodata_loops_and_a_lone_outlet():
    dirs = [[5, 5, 1, 1, 255, 0, 1]]                      # 0 -> 1 <-> 2 <- 3 | NoData | a lone outlet <- 6
    r = _run(dirs, length_nodata=-7.5)
    assert r["from_cell"].tolist() == [[NONE, NONE, NONE, NONE, NONE, 6, 6]]
    assert r["length"].tolist() == [[-7.5, -7.5, -7.5, -7.5, -7.5, 1.0, 0.0]]
    assert r["steps"][:, 0, :5].tolist() == [[NONE] * 5] * 3 and r["steps"][:, 0, 5:].tolist() == [[1, 0], [0, 0], [0, 0]]
    assert r["on_basin_path"].tolist() == [[0, 0, 0, 0, 0, 1, 1]]
    r = _run([[0]])                                       # D == 0.0: the outlet is its own head
    assert r["from_cell"].tolist() == [[0]] and r["length"].tolist() == [[0.0]] and r["on_basin_path"].tolist() == [[1]]
    r = _run([[5, 3, 1]], nodata=3)                       # a NoData code that is also a direction: both neighbours end at themselves
    assert r["from_cell"].tolist() == [[0, NONE, 2]]


def _longer(a, b, cx, cy, s):
    """the sign of len(a) - len(b) for step triples, len = nx cx + ny cy + nd sqrt(s), in exact arithmetic"""
    da = (a[0] - b[0]) * cx + (a[1] - b[1]) * cy
    db = a[2] - b[2]
    if da >= 0 and db >= 0:
        return 1 if (da > 0 or db > 0) else 0
    if da <= 0 and db <= 0:
        return -1
    lhs, rhs = da * da, db * db * s                       # opposite signs: compare |da| with |db| sqrt(s)
    if lhs == rhs:
        return 0
    return (1 if lhs > rhs else -1) * (1 if da > 0 else -1)


def _brute(dirs, cell, nodata=255):
    """every cell's path walked to its end; every cell on it learns how far away the walk's first cell is.  Returns
    per cell the head and the triple from it (None without a path), and every cell's walk."""
    h, w = dirs.shape
    cx, cy = Fraction(abs(cell[0])), Fraction(abs(cell[1]))
    s = cx * cx + cy * cy
    best = {}
    walks = {}
    for c in range(h * w):
        if dirs.flat[c] == nodata:
            continue
        walk, seen, p, ok = [], set(), c, True
        while True:
            if p in seen:
                ok = False                                # a direction loop: no path
                break
            seen.add(p)
            d = int(dirs.flat[p])
            if d not in OFFS:
                walk.append((p, None))
                break
            x, y = p % w, p // w
            tx, ty = x + OFFS[d][0], y + OFFS[d][1]
            if not (0 <= tx < w and 0 <= ty < h) or dirs[ty, tx] == nodata:
                walk.append((p, None))
                break
            walk.append((p, plane_of(d)))
            p = ty * w + tx
        if not ok:
            continue
        walks[c] = [p for p, _ in walk]
        t = [0, 0, 0]
        for p, pl in walk:
            b = best.get(p)
            cmp = 1 if b is None else _longer(t, b[1], cx, cy, s)
            if cmp > 0 or (cmp == 0 and c < b[0]):
                best[p] = (c, tuple(t))
            if pl is not None:
                t[pl] += 1
    return best, walks


@pytest.mark.parametrize("cell", [(1.0, 1.0), (30.0, 10.5), (3.0, 4.0)], ids=str)
@pytest.mark.parametrize("seed", range(4))
def test_against_a_walk_of_every_path(seed, cell):
    rng = np.random.default_rng(seed)
    dirs = rng.integers(0, 10, (37, 41)).astype(np.uint8)               # codes 0..9: 9 is no direction; loops are common
    dirs[rng.random(dirs.shape) < 0.05] = 255
    r = lm.longest_flow_path(dirs, 255, cell, -1.0)
    best, walks = _brute(dirs, cell)
    h, w = dirs.shape
    cxy = (abs(cell[0]), abs(cell[1]), math.sqrt(cell[0] * cell[0] + cell[1] * cell[1]))
    with_path = 0
    for c in range(h * w):
        y, x = divmod(c, w)
        if c not in best:
            assert c not in walks
            assert r["from_cell"][y, x] == NONE and r["length"][y, x] == -1.0 and r["on_basin_path"][y, x] == 0
            assert (r["steps"][:, y, x] == NONE).all()
            continue
        with_path += 1
        head, t = best[c]
        assert r["from_cell"][y, x] == head, (c, head, t)
        assert r["steps"][:, y, x].tolist() == list(t)
        assert r["length"][y, x] == t[0] * cxy[0] + t[1] * cxy[1] + t[2] * cxy[2]
    assert 0 < with_path < dirs.size - int((dirs == 255).sum())         # some cells drain into loops
    # on_basin_path marks exactly the walk from the outlet's head down to the outlet
    marked = set(np.flatnonzero(r["on_basin_path"].ravel()).tolist())
    expect = set()
    for c, walk in walks.items():
        if walk[-1] == c:                                                # an outlet
            expect.update(walks[best[c][0]])
            assert walks[best[c][0]][-1] == c
    assert marked == expect


def test_argument_errors_need_no_gpu(rd):
    L = rd.lib()
    host, dev = L.rdgpu_d8_longest_flow_path, L.rdgpu_d8_longest_flow_path_dev
    dirs = np.zeros((4, 5), np.uint8)
    fc = np.full((4, 5), 77, np.uint32)
    st = np.full((3, 4, 5), 77, np.uint32)
    ln = np.full((4, 5), 77.0, np.float64)
    ob = np.full((4, 5), 77, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd, one, lnd = ctypes.c_uint8(255), ctypes.c_double(1.0), ctypes.c_double(-1.0)
    dbl = ctypes.c_double
    outs = (p(fc), p(st), p(ln), lnd, p(ob))
    ARG = 2
    calls = [
        host(None, nd, 5, 4, one, one, *outs),                                          # null dirs
        host(p(dirs), nd, 5, 4, one, one, None, None, None, lnd, None),                 # no output requested
        host(p(dirs), nd, 0, 4, one, one, *outs),                                       # sizes
        host(p(dirs), nd, 5, -4, one, one, *outs),
        host(p(dirs), nd, 70000, 70000, one, one, *outs),                               # more than 0xFFFF0000 cells
        host(p(dirs), nd, 65536, 65536, one, one, *outs),
        host(p(dirs), nd, 5, 4, dbl(0.0), one, *outs),                                  # cell lengths
        host(p(dirs), nd, 5, 4, one, dbl(-0.0), *outs),
        host(p(dirs), nd, 5, 4, dbl(float("nan")), one, *outs),
        host(p(dirs), nd, 5, 4, one, dbl(float("inf")), *outs),
        host(p(dirs), nd, 5, 4, one, dbl(float("-inf")), *outs),
        dev(None, nd, 5, 4, one, one, *outs, None),
        dev(p(dirs), nd, 5, 4, one, one, None, None, None, lnd, None, None),
        dev(p(dirs), nd, 5, 0, one, one, *outs, None),
        dev(p(dirs), nd, -5, 4, one, one, *outs, None),
        dev(p(dirs), nd, 70000, 70000, one, one, *outs, None),
        dev(p(dirs), nd, 5, 4, dbl(0.0), one, *outs, None),
        dev(p(dirs), nd, 5, 4, one, dbl(float("nan")), *outs, None),
    ]
    assert calls == [ARG] * len(calls), calls
    assert (fc == 77).all() and (st == 77).all() and (ln == 77.0).all() and (ob == 77).all()
    with pytest.raises(rd.RdgpuError):
        rd.d8_longest_flow_path(dirs.astype(np.int32))                                  # a wrong dtype
    with pytest.raises(rd.RdgpuError):
        rd.d8_longest_flow_path(dirs[0])                                                # a wrong shape
    with pytest.raises(rd.RdgpuError):
        rd.d8_longest_flow_path(dirs, want=())                                          # an empty want
    with pytest.raises(rd.RdgpuError):
        rd.d8_longest_flow_path(dirs, want=("to_cell",))
    with pytest.raises(rd.RdgpuError):
        rd.d8_longest_flow_path(dirs, cell=1.0)                                         # no pair
    with pytest.raises(rd.RdgpuError):
        rd.d8_longest_flow_path(dirs, cell=(0.0, 1.0))                                  # the C-ABI's own check


def test_the_names_are_exported(rd):
    for name in ("d8_longest_flow_path", "d8_longest_flow_path_dev"):
        assert name in rd.__all__ and callable(getattr(rd, name))
    # the pybind module and the reference-style wrapper keep the reference's surface
    from richdem_amd import pyrichdem

    assert not hasattr(pyrichdem, "d8_longest_flow_path")
