"""Weighted D8 accumulation and total upstream length on the engine (csrc/accum_weighted.hip) against the Python model
(tests/weighted_accum_model.py, pinned by tests/test_weighted_accum_model.py): host C-ABI and `_dev` entries, every cell,
inputs unchanged.  Shapes are the smallest that reach every path of the kernels: one cell, one row, one column, a tile, one
more or less than a tile, several tiles; a path longer than a tile's 4095 links and than 65 535; loops inside a tile, across
an edge, across a corner and through twelve tiles.  Integer sums, step counts and lengths are equalities; so are float sums
whose partial sums are all representable; general float sums are held to the recursive-summation bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc  # noqa: E402
import weighted_accum_model as wm  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (193, 70), (257, 259)]   # (height, width)
INT_TYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32]
FLOAT_TYPES = [np.float32, np.float64]
NONE = wm.NONE
_FRACTAL = {}
_STEPS = {}


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((_bits(got) != _bits(exp)).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(_bits(got) != _bits(exp))[:5].tolist())


def _sum_dev(rd, dirs, wts, nodata, dir_nodata=255, sum_nodata=-1):
    """the `_dev` entry on a sentinel-filled tensor; None where this torch cannot hold the element type"""
    import torch

    if not hasattr(torch, wts.dtype.name):                  # (uint16 / uint32 in an older torch: decided before the device is touched)
        return None
    v = torch.from_numpy(wts.copy()).cuda()
    out = torch.full(dirs.shape, 77, dtype=torch.float64 if wts.dtype.kind == "f" else torch.int64, device="cuda")
    t = torch.from_numpy(dirs.copy()).cuda()
    rd.d8_flow_accum_weighted_dev(t, v, nodata, out, dir_nodata=dir_nodata, sum_nodata=sum_nodata)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dirs) and np.array_equal(_bits(v.cpu().numpy()), _bits(wts))
    return out.cpu().numpy()


def _sums(rd, dirs, wts, nodata, dir_nodata=255, sum_nodata=-1):
    """host and `_dev` results (the second None where torch lacks the type); the inputs are unchanged"""
    keep, keepw = dirs.copy(), wts.copy()
    got = rd.d8_flow_accum_weighted(dirs, wts, nodata, dir_nodata, sum_nodata)
    dev = _sum_dev(rd, dirs, wts, nodata, dir_nodata, sum_nodata)
    assert np.array_equal(dirs, keep) and np.array_equal(_bits(wts), _bits(keepw))
    return got, dev


def _check_sum(rd, what, dirs, wts, nodata, dir_nodata=255, sum_nodata=-1):
    exp = wm.weighted_sum(dirs, wts, nodata, dir_nodata, sum_nodata)
    got, dev = _sums(rd, dirs, wts, nodata, dir_nodata, sum_nodata)
    _same(got, exp, what + " host")
    if dev is not None:
        _same(dev, exp, what + " dev")
    return exp


def _length_dev(rd, dirs, cell, want, dir_nodata=255):
    import torch

    buf = {"steps": torch.full((3,) + dirs.shape, 77, dtype=torch.int32, device="cuda"),
           "length": torch.full(dirs.shape, 77.0, dtype=torch.float64, device="cuda")}
    t = torch.from_numpy(dirs.copy()).cuda()
    rd.d8_total_upstream_length_dev(t, cell[0], cell[1], dir_nodata, length_nodata=-1.0, **{k: buf[k] for k in want})
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dirs)
    out = {k: buf[k].cpu().numpy() for k in buf}
    for k in buf:
        if k not in want:
            assert (out[k] == 77).all(), k + " was not requested but written"
    return {k: (out[k].view(np.uint32) if k == "steps" else out[k]) for k in want}


def _check_length(rd, key, dirs, cell=(1.0, 1.0), dir_nodata=255, want=("steps", "length")):
    if (key, dir_nodata) not in _STEPS:
        _STEPS[(key, dir_nodata)] = wm.upstream_steps(dirs, dir_nodata)
    steps = _STEPS[(key, dir_nodata)]
    exp = {"steps": steps, "length": wm.path_length(steps, cell[0], cell[1], -1.0)}
    keep = dirs.copy()
    got = rd.d8_total_upstream_length(dirs, cell[0], cell[1], dir_nodata, want=want, length_nodata=-1.0)
    dev = _length_dev(rd, dirs, cell, want, dir_nodata)
    assert np.array_equal(dirs, keep) and sorted(got) == sorted(want) and sorted(dev) == sorted(want)
    for k in want:
        _same(got[k], exp[k], f"{key} {k} host")
        _same(dev[k], exp[k], f"{key} {k} dev")
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


def _int_weights(rng, shape, dtype):
    info = np.iinfo(dtype)
    return rng.integers(int(info.min), int(info.max) + 1, shape).astype(dtype)


def _exact_float_weights(rng, shape, dtype):
    """k / 1024 with |k| < 2^20: every one is an f32, and every partial sum over fewer than 2^23 cells is a double"""
    return (rng.integers(-(2**20) + 1, 2**20, shape).astype(np.float64) / 1024.0).astype(dtype)


@pytest.mark.parametrize("dtype", INT_TYPES + FLOAT_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests(rd, shape, holes, dtype):
    dirs = _fractal(rd, *shape, holes=holes)
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    if np.dtype(dtype).kind == "f":
        wts = _exact_float_weights(rng, shape, dtype)
        nodata = float(wts[0, -1])
    else:
        wts = _int_weights(rng, shape, dtype)
        nodata = int(wts[0, -1])
    e = _check_sum(rd, f"fractal{shape}{holes}{np.dtype(dtype).name}", dirs, wts, nodata)
    assert (e[dirs == 255] == -1).all() and ((dirs == 255).any() or not holes)


@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upstream_length_and_unit_weights_on_fractal_forests(rd, shape, holes):
    dirs = _fractal(rd, *shape, holes=holes)
    e = _check_length(rd, f"fractal{shape}{holes}", dirs, cell=(0.3, -0.7))
    part = dirs != 255
    assert (e["steps"][:, ~part] == NONE).all() and (e["length"][~part] == -1.0).all()
    # unit weights on loop-free directions: the cell count of d8_flow_accum, and one link per cell of the tree above
    ones = np.ones(shape, np.uint8)
    got, dev = _sums(rd, dirs, ones, 0)
    area = rd.d8_flow_accum(dirs, 255, np.float64)
    assert np.array_equal(got[part].astype(np.float64), area[part]) and np.array_equal(got, dev)
    assert np.array_equal(e["steps"].astype(np.int64).sum(axis=0)[part], got[part] - 1)


@pytest.mark.parametrize("want", [("steps",), ("length",)], ids="+".join)
def test_output_subsets(rd, want):
    _check_length(rd, "fractal(65, 130)True", _fractal(rd, 65, 130, holes=True), cell=(2.0, 5.0), want=want)


def _boustrophedon(h, w):
    """ONE path through every cell: along the rows, alternately east and west, one step south at the end of each"""
    order = []
    for y in range(h):
        order += [(x, y) for x in (range(w) if y % 2 == 0 else range(w - 1, -1, -1))]
    return sc.paint(sc.blank(h, w), order), order


def test_one_path_through_every_cell(rd):
    """257 x 259: 66 562 links, more than a tile's 4095 and than 65 535, across tile edges in every row; i32 weights near
    2^31, so that the sums pass 2^32 and 2^47"""
    h, w = 257, 259
    dirs, order = _boustrophedon(h, w)
    rng = np.random.default_rng(1)
    wts = (2**31 - 1 - rng.integers(0, 1000, (h, w))).astype(np.int32)
    ox, oy = np.array([p[0] for p in order]), np.array([p[1] for p in order])
    exp = np.empty((h, w), np.int64)
    exp[oy, ox] = np.cumsum(wts[oy, ox].astype(np.int64))
    assert exp[oy[-1], ox[-1]] > 2**47 and exp[oy[2], ox[2]] > 2**32
    got, dev = _sums(rd, dirs, wts, -1)
    _same(got, exp, "snake host")
    _same(dev, exp, "snake dev")
    got, dev = _sums(rd, dirs, -wts, 1)                     # and below -2^47
    _same(got, -exp, "snake negative host")
    _same(dev, -exp, "snake negative dev")
    # the upstream length: the three planes at the i-th cell of the path sum to i, and the length is the flow-path distance
    # of the REVERSED path, whose outlet is this path's head
    cell = (0.3, 0.7)
    r = rd.d8_total_upstream_length(dirs, cell[0], cell[1])
    d = _length_dev(rd, dirs, cell, ("steps", "length"))
    back = rd.d8_flow_path(sc.paint(sc.blank(h, w), order[::-1]), 255, None, cell, -1.0, want=("steps", "dist"))
    i = np.empty((h, w), np.int64)
    i[oy, ox] = np.arange(len(order))
    assert np.array_equal(r["steps"].astype(np.int64).sum(axis=0), i)
    _same(r["steps"], back["steps"], "snake steps")
    _same(r["length"], back["dist"], "snake length")
    _same(d["steps"], back["steps"], "snake steps dev")
    _same(d["length"], back["dist"], "snake length dev")


@pytest.mark.parametrize("code", range(1, 9))
def test_one_direction_through_tile_edges_and_corners(rd, code):
    """a straight run (odd codes) or a diagonal staircase (even codes) to the raster's border: the diagonals of the tiles
    pass through the tile corners"""
    dirs = np.full((130, 130), code, np.uint8)
    rng = np.random.default_rng(code)
    _check_sum(rd, f"uniform{code}", dirs, _int_weights(rng, dirs.shape, np.int16), 3)
    _check_sum(rd, f"uniform{code}f", dirs, _exact_float_weights(rng, dirs.shape, np.float32), -9999.0)
    _check_length(rd, f"uniform{code}", dirs, cell=(1.5, 2.5))


@pytest.mark.parametrize("at", [(8, 5), (63, 20), (62, 20), (20, 63), (63, 63), (100, 127)], ids=str)
def test_loops_with_feeders(rd, at):
    """a 4-cell loop inside a tile, across a tile edge (x = 62 .. 65), across a tile corner; trees draining into it: a loop
    cell gets its own weight and the trees that enter the loop there, and the loop's links carry nothing"""
    dirs, loop, feeders = sc.loop_with_tributary(at[0], at[1], (150, 135))
    rng = np.random.default_rng(at[0])
    wts = rng.integers(1, 1000, dirs.shape).astype(np.uint16)
    e = _check_sum(rd, f"loop{at}", dirs, wts, 0)
    w_ = lambda c: int(wts[c[1], c[0]])  # noqa: E731
    trib, side, tail = feeders[:5], feeders[5:7], feeders[7:]
    assert e[loop[0][1], loop[0][0]] == w_(loop[0]) + sum(map(w_, trib + side))
    assert e[loop[2][1], loop[2][0]] == w_(loop[2]) + sum(map(w_, tail))
    assert e[loop[1][1], loop[1][0]] == w_(loop[1]) and e[loop[3][1], loop[3][0]] == w_(loop[3])
    assert e[trib[2][1], trib[2][0]] == sum(map(w_, trib[:3] + side))          # the tributaries stay ordinary
    s = _check_length(rd, f"loop{at}", dirs, cell=(1.0, 2.0))
    assert s["steps"][:, loop[0][1], loop[0][0]].tolist() == [5, 2, 0] and s["steps"][:, loop[2][1], loop[2][0]].tolist() == [0, 0, 5]
    assert s["steps"][:, loop[1][1], loop[1][0]].tolist() == [0, 0, 0]
    _check_sum(rd, f"loop{at}f", dirs, _exact_float_weights(rng, dirs.shape, np.float64), -9999.0)


def test_ring_through_twelve_tiles(rd):
    h = w = 250
    ring = [(x, 10) for x in range(10, 240)] + [(240, y) for y in range(10, 240)] + [(x, 240) for x in range(240, 10, -1)] + \
           [(10, y) for y in range(240, 10, -1)]
    assert len({(x // 64, y // 64) for x, y in ring}) == 12
    dirs = sc.paint(sc.blank(h, w), ring + [ring[0]], last=None)
    feeder = [(x, 100) for x in range(30, 10, -1)]
    sc.paint(dirs, feeder + [(10, 100)], last=None)                         # a tributary from inside
    wts = np.random.default_rng(1).integers(-1000, 1000, (h, w)).astype(np.int32)
    e = _check_sum(rd, "ring", dirs, wts, -2**31)
    assert e[100, 10] == int(wts[100, 10]) + int(wts[100, 11:31].sum()) and e[10, 100] == wts[10, 100]
    s = _check_length(rd, "ring", dirs)
    assert s["steps"][:, 100, 10].tolist() == [20, 0, 0] and not s["steps"][:, 240, 100].any()


@pytest.mark.parametrize("dir_nodata", [0, 9, 255])
def test_direction_nodata_codes(rd, dir_nodata):
    dirs = _fractal(rd, 65, 130, holes=True)
    dirs[dirs == 255] = dir_nodata                                          # (with 0: the outlets do not participate either)
    rng = np.random.default_rng(dir_nodata)
    e = _check_sum(rd, f"nodata{dir_nodata}", dirs, _int_weights(rng, dirs.shape, np.int8), -128, dir_nodata, sum_nodata=-7)
    assert (dirs == dir_nodata).any() and (e[dirs == dir_nodata] == -7).all()
    _check_sum(rd, f"nodata{dir_nodata}f", dirs, _exact_float_weights(rng, dirs.shape, np.float32), 0.0, dir_nodata, sum_nodata=-2.5)
    _check_length(rd, f"nodata{dir_nodata}", dirs, dir_nodata=dir_nodata)
    e = _check_sum(rd, "all nodata directions", np.full((65, 130), dir_nodata, np.uint8), np.ones((65, 130), np.int32), -1, dir_nodata)
    assert (e == -1).all()


@pytest.mark.parametrize("dtype", FLOAT_TYPES, ids=lambda t: np.dtype(t).name)
def test_weight_nodata_nans_and_signed_zeros_in_mid_path(rd, dtype):
    dirs = _fractal(rd, 65, 130)
    rng = np.random.default_rng(11)
    wts = _exact_float_weights(rng, dirs.shape, dtype)
    wts[rng.random(dirs.shape) < 0.2] = -9999.0
    wts[rng.random(dirs.shape) < 0.2] = np.nan
    wts[3, :] = np.nan
    _bits(wts)[4, :] = _bits(np.array([-np.nan], dtype))[0] | 1             # NaNs of another sign and payload
    e = _check_sum(rd, "nan", dirs, wts, -9999.0)
    assert not np.isnan(e).any()
    _check_sum(rd, "nan nodata", dirs, wts, np.nan)                         # a NaN NoData equals nothing: -9999 is a weight now
    z = np.where(rng.random(dirs.shape) < 0.5, 0.0, -0.0).astype(dtype)     # -0.0 against a NoData of 0.0: nothing contributes
    z[rng.random(dirs.shape) < 0.05] = 1.0
    e = _check_sum(rd, "zeros", dirs, z, 0.0)
    assert not np.signbit(e).any()
    e = _check_sum(rd, "zeros nodata -0.0", dirs, z, -0.0)
    wts = _exact_float_weights(rng, dirs.shape, dtype)
    wts[10, 10], wts[50, 100] = np.inf, -np.inf                             # infinities are added as they are
    got, dev = _sums(rd, dirs, wts, -9999.0)
    assert np.isposinf(got).any() and np.isneginf(got).any() and np.array_equal(got, dev, equal_nan=True)
    fin = wts.copy()
    fin[~np.isfinite(wts)] = 0
    exp = wm.weighted_sum(dirs, fin, -9999.0)
    ok = np.isfinite(got)
    assert ok.sum() > dirs.size // 2 and np.array_equal(got[ok], exp[ok])


@pytest.mark.parametrize("dtype", INT_TYPES, ids=lambda t: np.dtype(t).name)
def test_weight_nodata_in_mid_path_and_integer_limits(rd, dtype):
    dirs = _fractal(rd, 65, 130)
    info = np.iinfo(dtype)
    for nodata, fill in ((int(info.min), int(info.max)), (int(info.max), int(info.min)), (0, int(info.max))):
        wts = np.full(dirs.shape, fill, dtype)
        wts[np.random.default_rng(5).random(dirs.shape) < 0.3] = nodata
        _check_sum(rd, f"limits{np.dtype(dtype).name}{nodata}", dirs, wts, nodata)


@pytest.mark.parametrize("dtype", FLOAT_TYPES, ids=lambda t: np.dtype(t).name)
def test_float_weights_within_the_summation_bound(rd, dtype):
    """seeded random weights of mixed sign, twenty binades apart: |got - sum| <= g * (sum of |w| over T(v)),
    g = (k - 1) u / (1 - (k - 1) u), u = 2^-53, k the contributing cells of T(v): the bound of recursive summation in any
    order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4)).  That theorem bounds the distance to the
    TRUE sum; math.fsum is the true sum rounded once more, by up to u |sum|, and a result that is right by the theorem may
    miss the same bound taken against fsum by that much.  So a cell that equals fsum passes (fsum is within u |sum| of
    the true sum, which is inside the bound for every k >= 2, and for k <= 1 nothing is rounded), and every other cell is
    held to the bound against the true sum in exact integer arithmetic (wm.exact_sums).  Nothing here is tuned."""
    from fractions import Fraction

    dirs = _fractal(rd, 257, 259, holes=True)
    rng = np.random.default_rng(2)
    wts = (rng.standard_normal(dirs.shape) * np.exp(rng.uniform(-10, 10, dirs.shape))).astype(dtype)
    wts[rng.random(dirs.shape) < 0.05] = -9999.0
    exp = wm.weighted_sum(dirs, wts, -9999.0)
    true, mag, k, shift = wm.exact_sums(dirs, wts, -9999.0)
    got, dev = _sums(rd, dirs, wts, -9999.0)
    part = dirs != 255
    u = Fraction(1, 2**53)
    for name, r in (("host", got), ("dev", dev)):
        assert np.array_equal(r[~part], exp[~part])
        worst, checked = Fraction(0), 0
        for c in np.flatnonzero((_bits(r) != _bits(exp)).ravel() & part.ravel()).tolist():
            err = abs(Fraction(float(r.ravel()[c])) * 2**shift - true[c])
            bound = (k[c] - 1) * u / (1 - (k[c] - 1) * u) * mag[c]
            assert k[c] >= 3 and err <= bound, (name, c, k[c], float(err / bound))
            worst, checked = max(worst, err / bound), checked + 1
        print(name, np.dtype(dtype).name, "cells:", int(part.sum()), "differing from fsum:", checked, "largest k:", max(k),
              "largest error / bound among those:", float(worst))
        assert checked > 0                                                    # the weights did exercise the rounding


def test_same_result_after_the_workspace_is_released(rd):
    dirs = _fractal(rd, 193, 70)
    wts = _int_weights(np.random.default_rng(0), dirs.shape, np.int16)
    first = rd.d8_flow_accum_weighted(dirs, wts, 5)
    rd.release_workspace()
    _same(rd.d8_flow_accum_weighted(dirs, wts, 5), first, "after release_workspace")
    small = rd.d8_total_upstream_length(dirs[:5, :7].copy())                # stale scratch must not matter
    _same(small["steps"], wm.upstream_steps(dirs[:5, :7]), "small after large")
    _same(rd.d8_flow_accum_weighted(dirs[:5, :7].copy(), wts[:5, :7].copy(), 5), wm.weighted_sum(dirs[:5, :7], wts[:5, :7], 5), "small sum")


def test_the_references_flow_accumulation_on_the_same_directions(rd, orc):
    """the reference's code path on the proportions of these directions; it counts the dependencies of interior cells only, so
    the code of every border cell is zeroed before both sides run.  Integer-valued weights: equality."""
    for h, w in ((65, 130), (63, 65)):
        dirs = wm.zero_border(_fractal(rd, h, w, holes=True))
        dirs[20:24, 20:24] = [[5, 5, 5, 7], [3, 0, 0, 7], [3, 0, 0, 7], [3, 1, 1, 1]]   # and a direction loop
        wts = np.random.default_rng(h).integers(-50, 50, (h, w)).astype(np.float64)
        exp = orc.port.flow_accumulation(wm.props9(dirs), wts)
        got, dev = _sums(rd, dirs, wts, -9999.0)
        _same(got, exp, "reference host")
        _same(dev, exp, "reference dev")
        _same(rd.d8_flow_accum_weighted(dirs, wts.astype(np.int32), -9999).astype(np.float64), exp, "reference i32")
