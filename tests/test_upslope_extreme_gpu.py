"""Upslope extremes on the engine (csrc/extreme.hip) against the Python model (tests/upslope_extreme_model.py, pinned by
tests/test_upslope_extreme_model.py): host C-ABI and `_dev` entries, both planes on every cell, bit for bit, inputs
unchanged.  Shapes are the smallest that reach every path of the kernels: one cell, one row, one column, a tile, one more or
less than a tile, several tiles; paths longer than a tile's 4095 links and than 65 535; paths through tile corners; loops
inside a tile, across an edge, across a corner and through twelve tiles.  Everything is equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc  # noqa: E402
import upslope_extreme_model as xm  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (193, 70), (257, 259)]   # (height, width)
PLANES = ("extreme", "at_cell")
MODES = ("max", "min")
NONE = xm.NONE
_MODEL = {}
_FRACTAL = {}


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((_bits(got) != _bits(exp)).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(_bits(got) != _bits(exp))[:5].tolist())


def _model(key, dirs, vals, nodata, which, dir_nodata=255):
    """the model's planes, computed once per case"""
    if key not in _MODEL:
        _MODEL[key] = xm.upslope_extreme(dirs, vals, nodata, MODES.index(which), dir_nodata)
    return _MODEL[key]


def _dev(rd, dirs, vals, nodata, which, want=PLANES, dir_nodata=255):
    """the `_dev` entry on sentinel-filled tensors: the planes asked for, and the proof that the others were left alone;
    None where this torch cannot hold the element type"""
    import torch

    try:
        v = torch.from_numpy(vals.copy()).cuda()
        buf = {"extreme": torch.from_numpy(np.full(dirs.shape, 77, vals.dtype)).cuda(),
               "at_cell": torch.from_numpy(np.full(dirs.shape, 77, np.int32)).cuda()}
    except (TypeError, RuntimeError):
        return None
    t = torch.from_numpy(dirs.copy()).cuda()
    rd.d8_upslope_extreme_dev(t, v, which, nodata, dir_nodata=dir_nodata, **{k: buf[k] for k in want})
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dirs) and np.array_equal(_bits(v.cpu().numpy()), _bits(vals))
    out = {k: buf[k].cpu().numpy() for k in PLANES}
    for k in PLANES:
        if k not in want:
            assert (out[k] == 77).all(), k + " was not requested but written"
    return {k: (out[k].view(np.uint32) if k == "at_cell" else out[k]) for k in want}


def _check(rd, key, dirs, vals, nodata, which, dir_nodata=255):
    exp = _model(f"{key}/{which}", dirs, vals, nodata, which, dir_nodata)
    keep, keepv = dirs.copy(), vals.copy()
    got = rd.d8_upslope_extreme(dirs, vals, which, nodata, dir_nodata, want=PLANES)
    dev = _dev(rd, dirs, vals, nodata, which, PLANES, dir_nodata)
    for k in PLANES:
        _same(got[k], exp[k], f"{key} {which} {k} host")
        if dev is not None:
            _same(dev[k], exp[k], f"{key} {which} {k} dev")
    assert np.array_equal(dirs, keep) and np.array_equal(_bits(vals), _bits(keepv))
    has = exp["at_cell"] != NONE                                        # extreme == values[at_cell], bit for bit
    assert np.array_equal(_bits(exp["extreme"])[has], _bits(vals).ravel()[exp["at_cell"][has]])
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
        _FRACTAL[(h, w, holes)] = (filled, rd.barnes_flat_resolution_d8(filled, -9999))
    filled, dirs = _FRACTAL[(h, w, holes)]
    return filled.copy(), dirs.copy()


@pytest.mark.parametrize("which", MODES)
@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests(rd, shape, holes, which):
    """the values are the DEM itself (the maximum of a filled DEM sits at the heads, the minimum at the cell itself or in
    a flat), and small integers 0..7, NoData 3, so that every tile is full of ties"""
    filled, dirs = _fractal(rd, *shape, holes=holes)
    key = f"fractal{shape}{holes}"
    e = _check(rd, key + "dem", dirs, filled, -9999.0, which)
    part = dirs != 255
    assert ((e["at_cell"] != NONE) == part).all() or holes
    small = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 8, shape).astype(np.uint8)
    e = _check(rd, key + "small", dirs, small, 3, which)
    assert (e["at_cell"][~part] == NONE).all() and (e["extreme"][~part] == 3).all()


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


@pytest.mark.parametrize("which", MODES)
@pytest.mark.parametrize("where", ["head", "middle", "mouth"])
def test_one_path_through_every_cell(rd, where, which):
    """257 x 259: 66 562 links, more than a tile's 4095 and than 65 535, across tile edges in every row"""
    h, w = 257, 259
    dirs, order = _boustrophedon(h, w)
    pos = {"head": 0, "middle": len(order) // 2, "mouth": len(order) - 1}[where]
    sx, sy = order[pos]
    vals = np.full((h, w), 5, np.int32)
    vals[sy, sx] = 9 if which == "max" else 1
    e = _check(rd, f"snake{where}", dirs, vals, -1, which)
    for i, (x, y) in enumerate(order[::997] + [order[-1]]):
        i = min(i * 997, len(order) - 1)
        # upstream of the special cell: a tie of fives, the lowest index on the path so far, which lies in row 0
        assert e["at_cell"][y, x] == (sy * w + sx if i >= pos else 0), (i, x, y)


@pytest.mark.parametrize("which", MODES)
def test_extreme_on_a_tributary_behind_a_tile_crossing(rd, which):
    dirs, chan = sc.serpentine(200, tributaries=True)
    rng = np.random.default_rng(5)
    vals = rng.integers(-50, 50, dirs.shape).astype(np.int16)
    assert dirs[1, 64] == 3 and dirs[3, 127] == 3                           # one-cell tributaries into the channel
    vals[1, 64] = 1000 if which == "max" else -1000
    e = _check(rd, "serpentine", dirs, vals, -32768, which)
    on = (chan != 0) & (dirs != 3)
    a = e["at_cell"][on]
    assert (a == 1 * 200 + 64).sum() == on.sum() - 64 and e["at_cell"][0, 63] != 264 and e["at_cell"][0, 64] == 264


@pytest.mark.parametrize("code", range(1, 9))
def test_one_direction_through_tile_edges_and_corners(rd, code):
    """a straight run (odd codes) or a diagonal staircase (even codes) to the raster's border: the diagonals of the tiles
    pass through the tile corners"""
    dirs = np.full((130, 130), code, np.uint8)
    rng = np.random.default_rng(code)
    vals = rng.integers(0, 8, dirs.shape).astype(np.int8)
    fl = rng.standard_normal(dirs.shape).astype(np.float32)
    for which in MODES:
        _check(rd, f"uniform{code}", dirs, vals, 3, which)
        _check(rd, f"uniform{code}f", dirs, fl, -9999.0, which)


@pytest.mark.parametrize("which", MODES)
@pytest.mark.parametrize("at", [(8, 5), (63, 20), (62, 20), (20, 63), (63, 63), (100, 127)], ids=str)
def test_loops_with_feeders(rd, at, which):
    """a 4-cell loop inside a tile, across a tile edge (x = 62 .. 65), across a tile corner; trees draining into it"""
    dirs, loop, feeders = sc.loop_with_tributary(at[0], at[1], (150, 135))
    w = 135
    base, best = (5, 9) if which == "max" else (5, 1)
    vals = np.full(dirs.shape, base, np.uint16)
    fx, fy = feeders[0]
    vals[fy, fx] = best                                                     # on a feeder: every loop cell gets it
    e = _check(rd, f"loop{at}feeder", dirs, vals, 0, which)
    for x, y in loop:
        assert e["at_cell"][y, x] == fy * w + fx and e["extreme"][y, x] == best
    tx, ty = feeders[-1]                                                    # the other feeder lies upstream of the loop only
    assert e["extreme"][ty, tx] == base
    vals = np.full(dirs.shape, base, np.uint16)
    lx, ly = loop[2]
    vals[ly, lx] = best                                                     # on a loop cell: every loop cell, but no feeder
    e = _check(rd, f"loop{at}on", dirs, vals, 0, which)
    for x, y in loop:
        assert e["at_cell"][y, x] == ly * w + lx
    for x, y in feeders:
        assert e["extreme"][y, x] == base and e["at_cell"][y, x] != ly * w + lx
    vals = np.random.default_rng(at[0]).integers(0, 4, dirs.shape).astype(np.uint16)   # and ties all over
    _check(rd, f"loop{at}ties", dirs, vals, 0, which)


@pytest.mark.parametrize("which", MODES)
def test_ring_through_twelve_tiles(rd, which):
    h = w = 250
    ring = [(x, 10) for x in range(10, 240)] + [(240, y) for y in range(10, 240)] + [(x, 240) for x in range(240, 10, -1)] + \
           [(10, y) for y in range(240, 10, -1)]
    tiles = {(x // 64, y // 64) for x, y in ring}
    assert len(tiles) == 12
    dirs = sc.paint(sc.blank(h, w), ring + [ring[0]], last=None)
    feeder = [(x, 100) for x in range(30, 10, -1)]
    sc.paint(dirs, feeder + [(10, 100)], last=None)                         # a tributary from inside
    base, best = (5.5, 9.25) if which == "max" else (5.5, -1.5)
    vals = np.full((h, w), base, np.float32)
    vals[100, 30] = best                                                    # on the feeder's head
    e = _check(rd, "ring feeder", dirs, vals, -9999.0, which)
    assert all(e["at_cell"][y, x] == 100 * w + 30 for x, y in ring + feeder)
    vals = np.full((h, w), base, np.float32)
    vals[240, 200] = best                                                   # on the ring
    e = _check(rd, "ring on", dirs, vals, -9999.0, which)
    assert all(e["at_cell"][y, x] == 240 * w + 200 for x, y in ring)
    assert all(e["extreme"][y, x] == np.float32(base) for x, y in feeder)
    vals = np.random.default_rng(1).integers(0, 3, (h, w)).astype(np.float32)
    _check(rd, "ring ties", dirs, vals, -9999.0, which)


@pytest.mark.parametrize("which", MODES)
@pytest.mark.parametrize("code", [5, 1, 7, 3, 6, 2])
def test_ties_across_tiles(rd, code, which):
    """equal extremes in different tiles: with codes 5, 7 and 6 the lower index lies upstream of the higher one, with 1, 3
    and 2 downstream of it; downstream of both the lower index wins either way"""
    h = w = 200
    dirs = np.full((h, w), code, np.uint8)
    vals = np.full((h, w), 4, np.int16)
    a, b = (10, 10), (150, 150) if code in (6, 2) else (150, 10) if code in (5, 1) else (10, 150)
    for x, y in (a, b):
        vals[y, x] = 7 if which == "max" else 1
    e = _check(rd, f"ties{code}", dirs, vals, -1, which)
    dx, dy = xm.OFFS[code]
    lo, hi = a[1] * w + a[0], b[1] * w + b[0]
    beyond = (b[0] + 20 * dx, b[1] + 20 * dy) if code in (5, 7, 6) else (a[0] + 5 * dx, a[1] + 5 * dy)
    between = (a[0] + 70 * abs(dx), a[1] + 70 * abs(dy))
    assert e["at_cell"][beyond[1], beyond[0]] == lo
    assert e["at_cell"][between[1], between[0]] == (lo if code in (5, 7, 6) else hi)


INT_TYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32]


@pytest.mark.parametrize("which", MODES)
@pytest.mark.parametrize("dtype", INT_TYPES, ids=lambda t: np.dtype(t).name)
def test_integer_types_at_their_limits(rd, dtype, which):
    """the type's minimum and maximum at cell 0 and at the last cell: a real key must never decode as "no contribution" """
    _, dirs = _fractal(rd, 65, 130)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(3)
    mid = rng.integers(int(info.min) // 2, int(info.max) // 2, dirs.shape).astype(dtype)
    nodata = int(mid[5, 5])
    for first, last in ((info.min, info.max), (info.max, info.min), (info.min, info.min), (info.max, info.max)):
        vals = mid.copy()
        vals[0, 0], vals[-1, -1] = first, last
        e = _check(rd, f"limits{np.dtype(dtype).name}{first}{last}", dirs, vals, nodata, which)
        assert e["at_cell"][0, 0] != NONE and e["at_cell"][-1, -1] != NONE
        best = info.max if which == "max" else info.min
        if first == best:
            assert e["at_cell"][0, 0] == 0 and e["extreme"][0, 0] == best
        if last == best:
            assert e["at_cell"][-1, -1] == dirs.size - 1 and e["extreme"][-1, -1] == best
    # every cell at the limit the mode does NOT look for, NoData the other one: keys with an all-zero high word
    vals = np.full(dirs.shape, info.min if which == "max" else info.max, dtype)
    e = _check(rd, f"limits{np.dtype(dtype).name}flat", dirs, vals, int(info.max if which == "max" else info.min), which)
    assert (e["at_cell"] != NONE).all()


@pytest.mark.parametrize("which", MODES)
def test_float32_infinities_zeros_and_nans(rd, which):
    _, dirs = _fractal(rd, 65, 130)
    rng = np.random.default_rng(11)
    base = rng.standard_normal(dirs.shape).astype(np.float32)
    inf = np.float32(np.inf)
    for first, last in ((-inf, inf), (inf, -inf)):
        vals = base.copy()
        vals[0, 0], vals[-1, -1] = first, last
        e = _check(rd, f"f32inf{first}", dirs, vals, -9999.0, which)
        assert e["at_cell"][0, 0] != NONE and e["at_cell"][-1, -1] != NONE
    # zeros of both signs everywhere, a few other values: the order tells -0 from +0
    vals = np.where(rng.random(dirs.shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    vals[rng.random(dirs.shape) < 0.02] = 1.0 if which == "min" else -1.0
    e = _check(rd, "f32zeros", dirs, vals, -9999.0, which)
    assert np.signbit(e["extreme"]).any() and (~np.signbit(e["extreme"])).any()
    e = _check(rd, "f32zeros nodata 0", dirs, vals, 0.0, which)           # -0 == +0 == NoData: only the few others contribute
    assert (e["extreme"][e["at_cell"] != NONE] != 0).all() and (_bits(e["extreme"])[e["at_cell"] == NONE] == 0).all()
    # NaN values never contribute; a NaN NoData equals nothing and comes back with its bits
    vals = base.copy()
    vals[rng.random(dirs.shape) < 0.3] = np.nan
    vals[0, :] = np.nan
    vals.view(np.uint32)[1, :] = 0xFFC00001                               # NaNs of another sign and payload
    e = _check(rd, "f32nan", dirs, vals, -9999.0, which)
    assert not np.isnan(e["extreme"]).any() and (e["at_cell"] == NONE).any()
    nd = np.array([0x7FC01234], np.uint32).view(np.float32)[0]
    e = _check(rd, "f32nan nodata", dirs, vals, nd, which)
    none = e["at_cell"] == NONE
    assert none.any() and (_bits(e["extreme"])[none] == 0x7FC01234).all() and not np.isnan(e["extreme"][~none]).any()


@pytest.mark.parametrize("want", [("extreme",), ("at_cell",), PLANES], ids="+".join)
def test_output_subsets(rd, want):
    filled, dirs = _fractal(rd, 65, 130, holes=True)
    for which in MODES:
        exp = _model(f"subsets/{which}", dirs, filled, -9999.0, which)
        got = rd.d8_upslope_extreme(dirs, filled, which, -9999.0, want=want)
        dev = _dev(rd, dirs, filled, -9999.0, which, want)
        assert sorted(got) == sorted(want) and sorted(dev) == sorted(want)
        for k in want:
            _same(got[k], exp[k], f"{want} {k} host")
            _same(dev[k], exp[k], f"{want} {k} dev")
    as_rdarray = rd.rdarray(filled, no_data=-9999.0)                       # value_nodata=None: the array's own
    _same(np.asarray(rd.d8_upslope_extreme(dirs, as_rdarray, want=want)[want[0]]), _model("subsets/max", dirs, filled, -9999.0, "max")[want[0]],
          "the array's own no_data")


@pytest.mark.parametrize("which", MODES)
def test_a_raster_without_a_contributing_cell(rd, which):
    _, dirs = _fractal(rd, 65, 130)
    vals = np.full(dirs.shape, 6, np.int16)
    e = _check(rd, "all nodata values", dirs, vals, 6, which)
    assert (e["at_cell"] == NONE).all() and (e["extreme"] == 6).all()
    vals = np.arange(dirs.size, dtype=np.int32).reshape(dirs.shape)
    e = _check(rd, "all nodata directions", np.full(dirs.shape, 255, np.uint8), vals, -1, which)
    assert (e["at_cell"] == NONE).all() and (e["extreme"] == -1).all()
    e = _check(rd, "nodata code 5", np.full(dirs.shape, 5, np.uint8), vals, -1, which, dir_nodata=5)
    assert (e["at_cell"] == NONE).all()


@pytest.mark.parametrize("which", MODES)
def test_recurrence_at_4000_on_the_device(rd, which):
    """no model: on a loop-free forest the recurrence "my pair is the better of my own and of the pairs of the neighbours
    whose link points at me" has one solution.  G(seed=3), filled, flat-resolved; the values are the filled DEM.  The
    lexicographic compare runs on two tensors, value and index, not on a packed word."""
    import torch

    n = 4000
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    ext = torch.full((n, n), 77.0, dtype=torch.float32, device="cuda")
    at = torch.full((n, n), 77, dtype=torch.int32, device="cuda")
    keep = Z.clone()
    rd.d8_upslope_extreme_dev(dirs, Z, which, -9999.0, extreme=ext, at_cell=at)
    torch.cuda.synchronize()
    assert torch.equal(keep, Z)
    del keep
    part = dirs != 255
    idx = torch.arange(n * n, dtype=torch.int32, device="cuda").view(n, n)
    own_has = part & (Z != -9999.0) & ~torch.isnan(Z)
    best_v = torch.where(own_has, Z, torch.zeros_like(Z))
    best_i = torch.where(own_has, idx, torch.full_like(idx, -1))
    best_has = own_has.clone()
    pad = torch.nn.functional.pad
    dP, eP, aP = pad(dirs, (1, 1, 1, 1), value=255), pad(ext, (1, 1, 1, 1), value=0.0), pad(at, (1, 1, 1, 1), value=-1)
    for code, (dx, dy) in xm.OFFS.items():                                # the neighbour at (x - dx, y - dy) with this code points at (x, y)
        sl = (slice(1 - dy, 1 - dy + n), slice(1 - dx, 1 - dx + n))
        cand = part & (dP[sl] == code) & (aP[sl] != -1) & (code != 255)
        cv, ci = eP[sl], aP[sl]
        better = (cv > best_v) if which == "max" else (cv < best_v)
        take = cand & (~best_has | better | ((cv == best_v) & (ci < best_i)))
        best_v, best_i, best_has = torch.where(take, cv, best_v), torch.where(take, ci, best_i), best_has | take
    assert int(part.sum()) > n * n // 2 and int(best_has.sum()) == int(part.sum())
    assert bool((at[best_has] == best_i[best_has]).all())
    assert bool((ext.view(torch.int32)[best_has] == best_v.view(torch.int32)[best_has]).all())
    assert bool((at[~best_has] == -1).all()) and bool((ext[~best_has] == -9999.0).all())
    got = at[best_has].to(torch.int64)
    assert bool((Z.view(-1).view(torch.int32)[got] == ext.view(torch.int32)[best_has]).all())   # extreme == values[at_cell]
    # the extreme is no worse than the cell's own value, and on a filled DEM the minimum upstream is the cell itself or a flat's
    assert bool((ext[own_has] >= Z[own_has]).all()) if which == "max" else bool((ext[own_has] <= Z[own_has]).all())
    assert int((at[part] != idx[part]).sum()) > n * n // 4 if which == "max" else True


def test_same_result_after_the_workspace_is_released(rd):
    filled, dirs = _fractal(rd, 193, 70)
    first = rd.d8_upslope_extreme(dirs, filled, "max", -9999.0)
    rd.release_workspace()
    again = rd.d8_upslope_extreme(dirs, filled, "max", -9999.0)
    small = rd.d8_upslope_extreme(dirs[:5, :7].copy(), filled[:5, :7].copy(), "min", -9999.0)   # stale scratch must not matter
    exp = xm.upslope_extreme(dirs[:5, :7], filled[:5, :7], -9999.0, xm.MIN)
    for k in PLANES:
        _same(again[k], first[k], "after release_workspace " + k)
        _same(small[k], exp[k], "small after large " + k)
