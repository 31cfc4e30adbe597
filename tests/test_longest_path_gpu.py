"""The longest upstream flow path on the engine (csrc/longest.hip) against the Python model (tests/longest_path_model.py,
pinned by tests/test_longest_path_model.py): host C-ABI and `_dev` entries, all four planes on every cell, bit for bit,
inputs unchanged.  Shapes are the smallest that reach every path of the kernels: one cell, one row, one column, a tile, one
more or less than a tile, several tiles; paths longer than a tile's 4095 links and than 65 535; paths through tile corners;
loops inside a tile, across an edge, across a corner and through twelve tiles.  Everything is equality."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longest_path_model as lm  # noqa: E402
import stream_cases as sc  # noqa: E402
from flow_path_model import NONE, OFFS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (193, 70), (257, 259)]   # (height, width)
PLANES = ("from_cell", "steps", "length", "on_basin_path")
CELLS = [(1.0, 1.0), (30.0, 10.5), (3.0, 4.0)]
_MODEL = {}
_FRACTAL = {}


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((_bits(got) != _bits(exp)).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(_bits(got) != _bits(exp))[:5].tolist())


def _model(key, dirs, cell, dir_nodata=255, length_nodata=-1.0):
    """the model's planes, computed once per case"""
    if key not in _MODEL:
        _MODEL[key] = lm.longest_flow_path(dirs, dir_nodata, cell, length_nodata)
    return _MODEL[key]


def _dev(rd, dirs, cell, want=PLANES, dir_nodata=255, length_nodata=-1.0):
    """the `_dev` entry on sentinel-filled tensors: the planes asked for, and the proof that the others were left alone"""
    import torch

    h, w = dirs.shape
    buf = {"from_cell": torch.full((h, w), 77, dtype=torch.int32, device="cuda"),
           "steps": torch.full((3, h, w), 77, dtype=torch.int32, device="cuda"),
           "length": torch.full((h, w), 77.0, dtype=torch.float64, device="cuda"),
           "on_basin_path": torch.full((h, w), 77, dtype=torch.uint8, device="cuda")}
    t = torch.from_numpy(dirs.copy()).cuda()
    rd.d8_longest_flow_path_dev(t, dir_nodata, cell, length_nodata, **{k: buf[k] for k in want})
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dirs)
    out = {k: buf[k].cpu().numpy() for k in PLANES}
    for k in PLANES:
        if k not in want:
            assert (out[k] == 77).all(), k + " was not requested but written"
    return {k: (out[k].view(np.uint32) if k in ("from_cell", "steps") else out[k]) for k in want}


def _check(rd, key, dirs, cell=(1.0, 1.0), dir_nodata=255, length_nodata=-1.0):
    exp = _model(f"{key}/{cell}/{dir_nodata}/{length_nodata}", dirs, cell, dir_nodata, length_nodata)
    keep = dirs.copy()
    got = rd.d8_longest_flow_path(dirs, dir_nodata, cell, length_nodata, want=PLANES)
    dev = _dev(rd, dirs, cell, PLANES, dir_nodata, length_nodata)
    for k in PLANES:
        _same(got[k], exp[k], f"{key} {cell} {k} host")
        _same(dev[k], exp[k], f"{key} {cell} {k} dev")
    assert np.array_equal(dirs, keep)
    return exp


def _fractal(rd, h, w, holes=False):
    """directions as the stream-order tests take them: the engine's fill and flat resolution of a fractal DEM"""
    from richdem_amd.synth import fractal_dem

    if (h, w, holes) not in _FRACTAL:
        dem = fractal_dem(w, h, seed=7 + h + w)
        filled = rd.FillDepressions(dem)
        if holes:                                            # NoData islands
            filled[h // 3:h // 3 + 3, w // 4:w // 4 + 5] = -9999
            filled[h // 2, w // 2] = -9999
            filled[0, 0] = -9999
        _FRACTAL[(h, w, holes)] = rd.barnes_flat_resolution_d8(filled, -9999)
    return _FRACTAL[(h, w, holes)].copy()


@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests(rd, shape, holes):
    dirs = _fractal(rd, *shape, holes=holes)
    cell = CELLS[(shape[0] + holes) % 3]
    e = _check(rd, f"fractal{shape}{holes}", dirs, cell)
    part = dirs != 255
    assert ((e["from_cell"] != NONE) == part).all()          # a filled and flat-resolved DEM has no loops
    assert e["on_basin_path"][part].any() == part.any() and not e["on_basin_path"][~part].any()


def _boustrophedon(h, w):
    """ONE path through every cell: along the rows, alternately east and west, one step south at the end of each"""
    dirs = np.zeros((h, w), np.uint8)
    order = []
    for y in range(h):
        east = y % 2 == 0
        dirs[y, :] = 5 if east else 1
        dirs[y, w - 1 if east else 0] = 7
        order += [(x, y) for x in (range(w) if east else range(w - 1, -1, -1))]
    dirs[order[-1][1], order[-1][0]] = 0
    return dirs, order


def test_one_path_through_every_cell(rd):
    """257 x 259: 66 562 links, more than a tile's 4095 and than 65 535, across tile edges in every row"""
    h, w = 257, 259
    dirs, order = _boustrophedon(h, w)
    e = _check(rd, "snake", dirs, (30.0, 10.5))
    assert (e["from_cell"] == 0).all() and e["on_basin_path"].all()
    x, y = order[-1]
    assert e["steps"][:, y, x].tolist() == [(w - 1) * h, h - 1, 0]
    assert e["length"][y, x] == float((w - 1) * h) * 30.0 + float(h - 1) * 10.5
    # the same path the other way round: the head is the last cell, the highest index of all
    back = np.zeros((h, w), np.uint8)
    sc.paint(back, order[::-1])
    e = _check(rd, "snake back", back)
    assert (e["from_cell"] == y * w + x).all() and e["length"][0, 0] == float(h * w - 1)


def test_the_longer_tributary_behind_a_tile_crossing(rd):
    dirs, chan = sc.serpentine(200, tributaries=True)
    assert dirs[1, 64] == 3 and dirs[3, 127] == 3                           # one-cell tributaries into the channel
    dirs[0, :64] = 0                                                        # the channel now starts at (64, 0): its tributary is longer
    e = _check(rd, "serpentine", dirs)
    on = (chan != 0) & (dirs != 3)
    on[0, :64] = False
    assert (e["from_cell"][on] == 1 * 200 + 64).all() and e["from_cell"][1, 64] == 264 and e["from_cell"][3, 127] == 3 * 200 + 127
    assert e["on_basin_path"][on].all() and e["on_basin_path"][1, 64] == 1 and e["on_basin_path"][3, 127] == 0
    _check(rd, "serpentine", dirs, (3.0, 4.0))


@pytest.mark.parametrize("code", range(1, 9))
def test_one_direction_through_tile_edges_and_corners(rd, code):
    """a straight run (odd codes) or a diagonal staircase (even codes) to the raster's border: the diagonals of the tiles
    pass through the tile corners"""
    dirs = np.full((130, 130), code, np.uint8)
    e = _check(rd, f"uniform{code}", dirs, CELLS[code % 3])
    dx, dy = OFFS[code]
    x, y = (129 if dx > 0 else 0 if dx < 0 else 40), (129 if dy > 0 else 0 if dy < 0 else 40)   # an outlet
    hx, hy = x - 129 * dx, y - 129 * dy                                   # the other end of its row, column or diagonal
    assert e["from_cell"][y, x] == hy * 130 + hx and int(e["steps"][:, y, x].sum()) == 129


@pytest.mark.parametrize("lower", ["left", "right"])
def test_equal_tributaries_that_join_in_another_tile(rd, lower):
    """two tributaries of 90 steps, heads in the tiles left and right of the one they join in; with cells of 1 x 1 a step
    along y is as long as one along x, so the right tributary may start one row higher and have the lower index"""
    h = w = 200
    dirs = sc.blank(h, w)
    left = [(x, 100) for x in range(10, 101)]
    right = [(x, 100) for x in range(190, 99, -1)] if lower == "left" else [(189, 99)] + [(x, 100) for x in range(189, 99, -1)]
    assert len(left) == len(right) == 91
    sc.paint(dirs, left, last=None)
    sc.paint(dirs, right, last=None)
    sc.paint(dirs, [(100, y) for y in range(100, 151)])
    e = _check(rd, f"join{lower}", dirs)
    hl, hr = left[0][1] * w + left[0][0], right[0][1] * w + right[0][0]
    win = min(hl, hr)
    assert win == (hl if lower == "left" else hr)
    assert e["from_cell"][100, 100] == win and e["from_cell"][150, 100] == win and e["length"][150, 100] == 140.0
    assert e["from_cell"][100, 99] == hl and e["from_cell"][100, 101] == hr
    lose = right if lower == "left" else left
    assert all(e["on_basin_path"][y, x] == 0 for x, y in lose[:-1]) and e["on_basin_path"][100, 100] == 1


@pytest.mark.parametrize("at", [(8, 5), (63, 20), (62, 20), (20, 63), (63, 63), (100, 127)], ids=str)
def test_loops_with_feeders(rd, at):
    """a 4-cell loop inside a tile, across a tile edge (x = 62 .. 65), across a tile corner; trees draining into it have no
    path either; a tree next to them keeps its answers"""
    dirs, loop, feeders = sc.loop_with_tributary(at[0], at[1], (150, 135))
    tree = [(at[0] - 4 + i, at[1] + 5) for i in range(8)]
    sc.paint(dirs, tree)
    e = _check(rd, f"loop{at}", dirs, (30.0, 10.5), length_nodata=-5.0)
    for x, y in loop + feeders:
        assert e["from_cell"][y, x] == NONE and e["length"][y, x] == -5.0 and e["on_basin_path"][y, x] == 0
    (hx, hy), (ox, oy) = tree[0], tree[-1]
    assert e["from_cell"][oy, ox] == hy * 135 + hx and e["length"][oy, ox] == 7 * 30.0
    assert int((e["from_cell"] == NONE).sum()) == len(loop) + len(feeders)


def test_ring_through_twelve_tiles(rd):
    h = w = 250
    ring = [(x, 10) for x in range(10, 240)] + [(240, y) for y in range(10, 240)] + [(x, 240) for x in range(240, 10, -1)] + \
           [(10, y) for y in range(240, 10, -1)]
    assert len({(x // 64, y // 64) for x, y in ring}) == 12
    dirs = sc.paint(sc.blank(h, w), ring + [ring[0]], last=None)
    feeder = [(x, 100) for x in range(30, 10, -1)]
    sc.paint(dirs, feeder + [(10, 100)], last=None)                         # a tributary from inside
    tree = [(x, 120) for x in range(30, 100)]
    sc.paint(dirs, tree)
    e = _check(rd, "ring", dirs)
    assert all(e["from_cell"][y, x] == NONE for x, y in ring + feeder)
    assert int((e["from_cell"] == NONE).sum()) == len(ring) + len(feeder)
    assert e["from_cell"][120, 99] == 120 * w + 30 and e["length"][120, 99] == 69.0


def test_a_raster_of_lone_outlets(rd):
    """D == 0.0 everywhere: an all-zero bit pattern must still be a contribution"""
    dirs = np.zeros((130, 70), np.uint8)
    e = _check(rd, "lone", dirs, (30.0, 10.5))
    assert np.array_equal(e["from_cell"], np.arange(dirs.size, dtype=np.uint32).reshape(dirs.shape))
    assert (e["length"] == 0.0).all() and not e["steps"].any() and e["on_basin_path"].all()
    e = _check(rd, "codes that are no direction", np.full((5, 70), 9, np.uint8))
    assert (e["length"] == 0.0).all()
    e = _check(rd, "all nodata", np.full((70, 5), 255, np.uint8), length_nodata=-3.0)
    assert (e["from_cell"] == NONE).all() and (e["length"] == -3.0).all() and not e["on_basin_path"].any()
    e = _check(rd, "nodata code 5", np.full((66, 66), 5, np.uint8), dir_nodata=5)
    assert (e["from_cell"] == NONE).all()


@pytest.mark.parametrize("cell", [(30.0, 10.5), (-30.0, 10.5), (3.0, 4.0)], ids=str)
def test_cell_sizes_and_the_length_formula(rd, cell):
    dirs = _fractal(rd, 65, 130, holes=True)
    e = _check(rd, "cells", dirs, cell)
    got = rd.d8_longest_flow_path(dirs, cell=cell, want=("steps", "length"))
    cx, cy = abs(cell[0]), abs(cell[1])
    diag = math.sqrt(cx * cx + cy * cy)
    nx, ny, nd = (got["steps"][i].astype(np.float64) for i in range(3))
    formula = nx * cx + ny * cy + nd * diag                               # numpy rounds every product and every sum
    has = got["steps"][0] != NONE
    assert has.any() and (~has).any()
    _same(got["length"][has], formula[has], f"the formula {cell}")
    assert (got["length"][~has] == -1.0).all() and (e["length"] >= 0)[has].all()


@pytest.mark.parametrize("want", [c for r in range(1, 5) for c in itertools.combinations(PLANES, r)], ids="+".join)
def test_output_subsets(rd, want):
    dirs = _fractal(rd, 65, 130, holes=True)
    exp = _model("subsets", dirs, (30.0, 10.5))
    got = rd.d8_longest_flow_path(dirs, cell=(30.0, 10.5), want=want)
    dev = _dev(rd, dirs, (30.0, 10.5), want)
    assert sorted(got) == sorted(want) and sorted(dev) == sorted(want)
    for k in want:
        _same(got[k], exp[k], f"{want} {k} host")
        _same(dev[k], exp[k], f"{want} {k} dev")


def test_recurrence_at_4000_on_the_device(rd):
    """no model: on a loop-free forest the recurrence "my (D(head), -head) is the lexicographic maximum of my own (D, -index)
    and of the pairs of the neighbours that point at me" has one solution.  G(seed=3), filled, flat-resolved."""
    import torch

    n = 4000
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    del Z
    cell = (30.0, 10.5)
    i32 = dict(dtype=torch.int32, device="cuda")
    to_cell, steps_fp = torch.full((n, n), 77, **i32), torch.full((3, n, n), 77, **i32)
    D = torch.full((n, n), 77.0, dtype=torch.float64, device="cuda")
    rd.d8_flow_path_dev(dirs, cell=cell, to_cell=to_cell, steps=steps_fp, dist=D)
    fc, steps = torch.full((n, n), 77, **i32), torch.full((3, n, n), 77, **i32)
    length = torch.full((n, n), 77.0, dtype=torch.float64, device="cuda")
    onp = torch.full((n, n), 77, dtype=torch.uint8, device="cuda")
    keep = dirs.clone()
    rd.d8_longest_flow_path_dev(dirs, cell=cell, from_cell=fc, steps=steps, length=length, on_basin_path=onp)
    torch.cuda.synchronize()
    assert torch.equal(keep, dirs)
    del keep
    part = dirs != 255
    has = to_cell != -1
    assert int(part.sum()) > n * n // 2 and torch.equal(has, part) and torch.equal(fc != -1, has)
    idx = torch.arange(n * n, **i32).view(n, n)
    src = torch.where(has, fc, torch.zeros_like(fc)).to(torch.int64)
    Dh = torch.where(has, D.view(-1)[src], torch.full_like(D, -1.0))      # D of the head the engine names
    best_v, best_i = torch.where(has, D, torch.full_like(D, -1.0)), torch.where(has, idx, torch.full_like(idx, -1))
    pad = torch.nn.functional.pad
    dP, vP, iP = pad(dirs, (1, 1, 1, 1), value=255), pad(Dh, (1, 1, 1, 1), value=-1.0), pad(fc, (1, 1, 1, 1), value=-1)
    for code, (dx, dy) in OFFS.items():                                   # the neighbour at (x - dx, y - dy) with this code points at (x, y)
        sl = (slice(1 - dy, 1 - dy + n), slice(1 - dx, 1 - dx + n))
        cand = part & (dP[sl] == code) & (iP[sl] != -1)
        cv, ci = vP[sl], iP[sl]
        take = cand & ((cv > best_v) | ((cv == best_v) & (ci < best_i)))
        best_v, best_i = torch.where(take, cv, best_v), torch.where(take, ci, best_i)
    assert bool((fc == best_i).all()) and bool((Dh == best_v).all())
    assert int((fc[has] != idx[has]).sum()) > n * n // 4
    del dP, vP, iP, best_v, best_i, Dh
    assert bool((steps[:, ~has] == -1).all()) and bool((length[~has] == -1.0).all()) and bool((onp[~has] == 0).all())
    for p in range(3):
        assert bool((steps[p][has] == steps_fp[p].view(-1)[src][has] - steps_fp[p][has]).all())
    cx, cy, diag = 30.0, 10.5, math.sqrt(30.0 * 30.0 + 10.5 * 10.5)
    formula = steps[0].double() * cx + steps[1].double() * cy + steps[2].double() * diag
    assert bool((length[has] == formula[has]).all())
    outlet = torch.where(has, to_cell, torch.zeros_like(to_cell)).to(torch.int64)
    assert torch.equal(onp, (has & (fc == fc.view(-1)[outlet])).to(torch.uint8))
    assert 0 < int(onp.sum()) < int(has.sum())


def test_same_result_after_the_workspace_is_released(rd):
    dirs = _fractal(rd, 193, 70)
    first = rd.d8_longest_flow_path(dirs, want=PLANES)
    rd.release_workspace()
    again = rd.d8_longest_flow_path(dirs, want=PLANES)
    small = rd.d8_longest_flow_path(dirs[:5, :7].copy(), want=PLANES)     # stale scratch must not matter
    exp = lm.longest_flow_path(dirs[:5, :7].copy())
    for k in PLANES:
        _same(again[k], first[k], "after release_workspace " + k)
        _same(small[k], exp[k], "small after large " + k)
