"""Drainage cell, step counts, flow distance and HAND on the engine (csrc/flowpath.hip) against the Python model
(tests/flow_path_model.py, pinned by tests/test_flow_path_model.py): host C-ABI and `_dev` entries, every requested plane
on every cell, bit for bit, inputs unchanged.  Shapes are the smallest that reach every path of the kernels: one cell,
one row, one column, a tile, one more or less than a tile, several tiles; paths longer than a tile's 4095 steps and than
65 535; paths through tile corners; loops inside a tile, across an edge and across a corner."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_path_model as fm  # noqa: E402
import stream_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (193, 70), (257, 259)]   # (height, width)
PLANES = ("to_cell", "steps", "dist")
_MODEL = {}


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((_bits(got) != _bits(exp)).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(_bits(got) != _bits(exp))[:5].tolist())


def _model(key, dirs, nodata, chan, cell, dist_nodata):
    """the model's planes, computed once per case"""
    if key not in _MODEL:
        _MODEL[key] = fm.flow_path(dirs, nodata, chan, cell, dist_nodata)
    return _MODEL[key]


def _dev(rd, dirs, nodata, chan, cell, dist_nodata, want=PLANES):
    """the `_dev` entry on sentinel-filled tensors: the planes asked for, and the proof that the others were left alone"""
    import torch

    h, w = dirs.shape
    t = torch.from_numpy(dirs.copy()).cuda()
    c = None if chan is None else torch.from_numpy(chan.copy()).cuda()
    buf = {"to_cell": torch.full((h, w), 77, dtype=torch.int32, device="cuda"),
           "steps": torch.full((3, h, w), 77, dtype=torch.int32, device="cuda"),
           "dist": torch.full((h, w), 77.0, dtype=torch.float64, device="cuda")}
    rd.d8_flow_path_dev(t, nodata, c, cell, dist_nodata, **{k: buf[k] for k in want})
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dirs) and (c is None or np.array_equal(c.cpu().numpy(), chan))
    for k in PLANES:
        if k not in want:
            assert bool((buf[k] == 77).all()), k + " was not requested but written"
    return {k: (buf[k].cpu().numpy() if k == "dist" else buf[k].cpu().numpy().view(np.uint32)) for k in want}


def _check(rd, key, dirs, nodata=255, chan=None, cell=(1.0, 1.0), dist_nodata=-1.0):
    exp = _model(key, dirs, nodata, chan, cell, dist_nodata)
    keep, keepc = dirs.copy(), None if chan is None else chan.copy()
    got = rd.d8_flow_path(dirs, nodata, chan, cell, dist_nodata, want=PLANES)
    dev = _dev(rd, dirs, nodata, chan, cell, dist_nodata)
    for k in PLANES:
        _same(got[k], exp[k], f"{key} {k} host")
        _same(dev[k], exp[k], f"{key} {k} dev")
    assert np.array_equal(dirs, keep) and (chan is None or np.array_equal(chan, keepc))
    return exp


def _fractal(rd, h, w, holes=False):
    """directions as the stream-order tests take them: the engine's fill and flat resolution of a fractal DEM"""
    from richdem_amd.synth import fractal_dem

    dem = fractal_dem(w, h, seed=7 + h + w)
    filled = rd.FillDepressions(dem)
    if holes:                                            # NoData islands
        filled[h // 3:h // 3 + 3, w // 4:w // 4 + 5] = -9999
        filled[h // 2, w // 2] = -9999
        filled[0, 0] = -9999
    return filled, rd.barnes_flat_resolution_d8(filled, -9999)


@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests(rd, shape, holes):
    _, dirs = _fractal(rd, *shape, holes=holes)
    key = f"fractal{shape}{holes}"
    exp = _check(rd, key, dirs)
    assert np.array_equal(rd.d8_outlets(dirs), exp["to_cell"])          # without a mask: d8_outlets' answer, bit for bit
    acc = rd.d8_flow_accum(dirs)
    for thr in (1.0, 20.0, float(acc.max()) + 1.0):
        chan = rd.d8_channels(acc, thr)
        e = _check(rd, f"{key}thr{thr}", dirs, 255, chan)
        stop = (chan != 0) & (dirs != 255)
        assert (e["to_cell"][stop] == np.flatnonzero(stop)).all()
        if thr > acc.max():                                              # an empty mask: nothing has a drainage cell
            assert not chan.any() and (e["to_cell"] == fm.NONE).all() and (e["dist"] == -1.0).all()


def _boustrophedon(h, w):
    """ONE path through every cell: along the rows, alternately east and west, one step south at the end of each"""
    dirs = np.zeros((h, w), np.uint8)
    for y in range(h):
        east = y % 2 == 0
        dirs[y, :] = 5 if east else 1
        dirs[y, w - 1 if east else 0] = 7
    last = (w - 1 if (h - 1) % 2 == 0 else 0, h - 1)
    dirs[last[1], last[0]] = 0
    return dirs, last


@pytest.mark.parametrize("shape", [(65, 130), (257, 259)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_path_through_every_cell(rd, shape):
    """(257, 259): 66 562 steps, more than a tile's 4095 and than 65 535, across tile edges in every row"""
    h, w = shape
    dirs, last = _boustrophedon(h, w)
    e = _check(rd, f"snake{shape}", dirs)
    assert (e["to_cell"] == last[1] * w + last[0]).all()
    assert int(e["steps"][0, 0, 0]) + int(e["steps"][1, 0, 0]) == h * w - 1 and e["steps"][2].max() == 0
    e = _check(rd, f"snake{shape}end", dirs, 255, sc.mask_of(shape, [last]))
    assert int(e["steps"][0, 0, 0]) == h * (w - 1) and int(e["steps"][1, 0, 0]) == h - 1
    mid = (w // 2, h // 2)
    e = _check(rd, f"snake{shape}mid", dirs, 255, sc.mask_of(shape, [mid]))
    assert e["to_cell"][0, 0] == mid[1] * w + mid[0] and e["to_cell"][h - 1, w // 2] == fm.NONE
    e = _check(rd, f"snake{shape}none", dirs, 255, np.zeros(shape, np.uint8))
    assert (e["to_cell"] == fm.NONE).all()


@pytest.mark.parametrize("code", range(1, 9))
def test_one_direction_through_tile_edges_and_corners(rd, code):
    """a straight run (odd codes) or a diagonal staircase (even codes) to the raster's border: the diagonals of the tiles
    pass through the tile corners"""
    dirs = np.full((130, 130), code, np.uint8)
    e = _check(rd, f"uniform{code}", dirs)
    p = fm.plane_of(code)
    assert e["steps"][p].max() == 129 and all(e["steps"][q].max() == 0 for q in range(3) if q != p)
    chan = np.zeros((130, 130), np.uint8)
    chan[::37, ::29] = 1
    chan[64, 64] = chan[63, 63] = chan[127, 128] = 1
    _check(rd, f"uniform{code}masked", dirs, 255, chan)


@pytest.mark.parametrize("at", [(8, 5), (63, 20), (20, 63), (63, 63), (100, 127)], ids=str)
def test_loops_with_feeders(rd, at):
    """a 4-cell loop inside a tile, across a tile edge, across a tile corner; trees draining into it"""
    dirs, loop, feeders = sc.loop_with_tributary(at[0], at[1], (150, 135))
    e = _check(rd, f"loop{at}", dirs)
    for x, y in loop + feeders:
        assert e["to_cell"][y, x] == fm.NONE and e["dist"][y, x] == -1.0
    on_loop = sc.mask_of(dirs.shape, [loop[2]])                            # a stop cell ON the loop breaks it
    e = _check(rd, f"loop{at}stop", dirs, 255, on_loop)
    for x, y in loop + feeders:
        assert e["to_cell"][y, x] == loop[2][1] * 135 + loop[2][0]
    on_the_way = sc.mask_of(dirs.shape, [feeders[2]])                      # a stop cell on a feeder: what lies below it still loops
    e = _check(rd, f"loop{at}feeder", dirs, 255, on_the_way)
    assert e["to_cell"][feeders[0][1], feeders[0][0]] == feeders[2][1] * 135 + feeders[2][0]
    assert e["to_cell"][loop[0][1], loop[0][0]] == fm.NONE


def test_long_loop_through_many_tiles(rd):
    h = w = 200
    ring = [(x, 10) for x in range(10, 190)] + [(190, y) for y in range(10, 190)] + [(x, 190) for x in range(190, 10, -1)] + \
           [(10, y) for y in range(190, 10, -1)]
    dirs = sc.paint(sc.blank(h, w), ring + [ring[0]], last=None)
    sc.paint(dirs, [(x, 100) for x in range(20, 11, -1)] + [(11, 100), (10, 100)], last=None)   # a tributary from inside
    e = _check(rd, "ring", dirs)
    assert e["to_cell"][100, 15] == fm.NONE and e["to_cell"][10, 10] == fm.NONE and e["to_cell"][0, 0] == 0
    e = _check(rd, "ring stop", dirs, 255, sc.mask_of((h, w), [(190, 100)]))
    assert e["to_cell"][100, 15] == 100 * w + 190 and e["steps"][:, 190, 100].max() > 0


def test_anisotropic_cells_and_their_signs(rd):
    """30.0^2 and 10.5^2 are exact, so diag is the same double in C and in the model; a swapped plane or a contracted
    multiply-add shows in the bits"""
    _, dirs = _fractal(rd, 193, 70, holes=True)
    diag = math.sqrt(30.0 * 30.0 + 10.5 * 10.5)
    for cell in ((30.0, 10.5), (-30.0, -10.5)):
        e = _check(rd, f"aniso{cell}", dirs, 255, None, cell, -3.0)
        s = e["steps"].astype(np.float64)
        exp = s[0] * 30.0 + s[1] * 10.5 + s[2] * diag
        exp[e["to_cell"] == fm.NONE] = -3.0
        _same(e["dist"], exp, f"aniso{cell} formula")
        assert (s[0] != s[1]).any() and (s[2] > 0).any()
    snake, _ = _boustrophedon(257, 259)
    _check(rd, "aniso snake", snake, 255, None, (30.0, 10.5), -3.0)


@pytest.mark.parametrize("want", [("to_cell",), ("steps",), ("dist",), PLANES], ids="+".join)
def test_output_subsets(rd, want):
    _, dirs = _fractal(rd, 65, 130)
    chan = rd.d8_channels(rd.d8_flow_accum(dirs), 20.0)
    exp = _model("subsets", dirs, 255, chan, (2.0, 3.0), -1.0)
    got = rd.d8_flow_path(dirs, 255, chan, (2.0, 3.0), -1.0, want=want)
    dev = _dev(rd, dirs, 255, chan, (2.0, 3.0), -1.0, want)
    assert sorted(got) == sorted(want) and sorted(dev) == sorted(want)
    for k in want:
        _same(got[k], exp[k], f"{want} {k} host")
        _same(dev[k], exp[k], f"{want} {k} dev")
    if want == ("dist",):
        _same(rd.d8_flow_distance(dirs, 255, chan, (2.0, 3.0)), exp["dist"], "d8_flow_distance")


HAND_TYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64]


@pytest.mark.parametrize("dtype", HAND_TYPES, ids=lambda t: np.dtype(t).name)
def test_hand_of_every_element_type(rd, dtype):
    import torch

    filled, dirs = _fractal(rd, 193, 70)
    dt = np.dtype(dtype)
    unit = (filled.astype(np.float64) - filled.min()) / float(filled.max() - filled.min())
    if dt.kind == "f":
        dem = (filled.astype(np.float64) * (1.0 + 2.0 ** -40) + 1e-7).astype(dt)   # float64: elevations that do not fit float32
        nodata = -9999.0
    else:
        info = np.iinfo(dt)
        dem = (info.min + 1 + unit * (float(info.max) - float(info.min) - 2)).astype(dt)   # the type's whole range
        nodata = int(info.max)
    if dt == np.float64:
        assert (dem.astype(np.float32).astype(np.float64) != dem).any()
    acc = rd.d8_flow_accum(dirs)
    chan = rd.d8_channels(acc, 20.0)
    for mask in (None, chan):
        t = _model(f"hand{mask is None}", dirs, 255, mask, (1.0, 1.0), -1.0)["to_cell"]
        z = dem.copy()
        ends = np.unique(t[t != fm.NONE])
        z.ravel()[ends[len(ends) // 2]] = nodata                               # NoData AT a drainage cell
        up = np.flatnonzero((t.ravel() != fm.NONE) & (t.ravel() != np.arange(t.size)))
        z.ravel()[up[len(up) // 3]] = nodata                                   # and at a cell upstream of one
        exp = fm.hand(z, t, nodata, -9999.0)
        assert (exp == -9999.0).sum() > (t == fm.NONE).sum() + 1 and (exp != -9999.0).any()
        keep = z.copy()
        _same(rd.d8_hand(z, dirs, nodata, 255, mask), exp, f"hand {dt.name} host")
        assert np.array_equal(z, keep)
        name = {"uint16": "uint16", "uint32": "uint32"}.get(dt.name)
        if name is None or hasattr(torch, name):
            try:
                zt = torch.from_numpy(z.copy()).cuda()
            except (TypeError, RuntimeError):
                zt = None                                                      # an element type this torch cannot hold
            if zt is not None:
                out = torch.full(dirs.shape, 77.0, dtype=torch.float64, device="cuda")
                rd.d8_hand_dev(zt, torch.from_numpy(dirs).cuda(), nodata, out, 255, None if mask is None else torch.from_numpy(mask).cuda())
                torch.cuda.synchronize()
                _same(out.cpu().numpy(), exp, f"hand {dt.name} dev")
                assert np.array_equal(zt.cpu().numpy(), keep)


def test_structure_at_4000_on_the_device(rd):
    """no model: the recurrence the definition implies, checked in torch on G(seed=3), filled, flat-resolved, channels at
    >= 50 cells of accumulation"""
    import torch

    n = 4000
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, area)
    chan = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_channels_dev(area, 50.0, chan)
    del Z, area
    to = torch.empty((n, n), dtype=torch.int32, device="cuda")
    outlets = torch.empty((n, n), dtype=torch.int32, device="cuda")
    rd.d8_flow_path_dev(dirs, to_cell=to)
    rd.d8_outlets_dev(dirs, outlets)
    assert torch.equal(to, outlets)
    steps = torch.empty((3, n, n), dtype=torch.int32, device="cuda")
    rd.d8_flow_path_dev(dirs, 255, chan, to_cell=to, steps=steps)
    torch.cuda.synchronize()
    idx = torch.arange(n * n, dtype=torch.int64, device="cuda")
    d = dirs.view(-1).to(torch.int64)
    to, steps = to.view(-1).to(torch.int64), steps.view(3, -1).to(torch.int64)
    stop = (chan.view(-1) != 0) & (d != 255)
    assert int(stop.sum()) > 1000
    assert bool((to[stop] == idx[stop]).all()) and bool((steps[:, stop] == 0).all())
    dx = torch.tensor([0, -1, -1, 0, 1, 1, 1, 0, -1], device="cuda")
    dy = torch.tensor([0, 0, -1, -1, -1, 0, 1, 1, 1], device="cuda")
    plane = torch.tensor([-1, 0, 2, 1, 2, 0, 2, 1, 2], device="cuda")
    code = torch.where((d >= 1) & (d <= 8), d, torch.zeros_like(d))
    tx, ty = idx % n + dx[code], idx // n + dy[code]
    linked = ~stop & (code != 0) & (tx >= 0) & (tx < n) & (ty >= 0) & (ty < n)
    tgt = torch.where(linked, ty * n + tx, idx)
    defined = to != -1
    assert int(defined.sum()) > n * n // 2
    assert bool((~defined | stop | linked).all())                        # a defined cell that is no stop cell has a target
    assert bool((to[linked] == to[tgt][linked]).all())                   # ... and the target's drainage cell, defined or not
    for p in range(3):
        own = (plane[code] == p).to(torch.int64)
        ok = steps[p] == steps[p][tgt] + own
        assert bool(ok[linked & defined].all()), p
    assert bool((steps[:, ~defined] == -1).all())
    assert bool((~defined[~stop & ~linked]).all())                       # no target and no stop cell: no drainage cell


def test_same_result_after_the_workspace_is_released(rd):
    _, dirs = _fractal(rd, 193, 70)
    first = rd.d8_flow_path(dirs, want=PLANES)
    rd.release_workspace()
    again = rd.d8_flow_path(dirs, want=PLANES)
    small = rd.d8_flow_path(dirs[:5, :7].copy(), want=PLANES)             # a small raster after a larger one: stale scratch must not matter
    exp = fm.flow_path(dirs[:5, :7])
    for k in PLANES:
        _same(again[k], first[k], "after release_workspace " + k)
        _same(small[k], exp[k], "small after large " + k)
