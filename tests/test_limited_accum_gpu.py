"""Limited D8 accumulation on the engine (csrc/accum_limited.hip) against the Python model (tests/limited_accum_model.py,
pinned by tests/test_limited_accum_model.py): host C-ABI and `_dev` entries, every cell, inputs unchanged.  The shapes are
those of tests/test_weighted_accum_gpu.py.  Wherever the inputs are dyadic the comparison is an equality, and that the
inputs ARE dyadic enough is asserted on the model's exact values (_exact): with q the smallest power of two that divides
every exact total, product, out and kept, and M the sum of |supply| over the raster, M / q < 2^53 makes every partial sum
in any order a double.  General float supplies are held to the contract's bound against the exact rational values."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limited_accum_model as lm  # noqa: E402
import stream_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (193, 70), (257, 259)]   # (height, width)
FLOAT_TYPES = [np.float32, np.float64]
LIMITS = ["none", "capacity", "factor", "both"]
KEYS = ("supplied", "left", "kept_pos", "kept_neg")
_FRACTAL = {}


def _same(got, exp, what):
    """equal as numbers, every cell (the contract gives a zero no sign), and no NaN"""
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got != exp).sum())
    print(what, "cells differing:", bad)
    assert bad == 0 and not np.isnan(got).any(), (what, bad, np.argwhere(got != exp)[:5].tolist())


def _exact(r, supply, nodata, factor):
    """every partial sum and product of this case is a double, in whatever order (the module's docstring)"""
    den = max((v.denominator for k in ("out_exact", "kept_exact") for v in r[k] if v is not None), default=1)
    assert den & (den - 1) == 0
    den *= 4 if factor is not None else 1                   # factor * total before the clamps: factors are multiples of 1/4
    s = supply.astype(np.float64).ravel()
    mag = sum(abs(Fraction(x)) for x in s[np.array(lm.wm.contributes(supply, nodata))].tolist())
    return mag * den < 2**53


def _dev(rd, dirs, supply, nodata, cap, fac, dir_nodata, nodata_out, want=("out", "kept", "result")):
    """the `_dev` entry on sentinel-filled tensors: the planes in `want`; what was not requested keeps its sentinel"""
    import torch

    up = lambda a: None if a is None else torch.from_numpy(a.copy()).cuda()  # noqa: E731
    t, s, c, f = up(dirs), up(supply), up(cap), up(fac)
    buf = {"out": torch.full(dirs.shape, 77.0, dtype=torch.float64, device="cuda"),
           "kept": torch.full(dirs.shape, 77.0, dtype=torch.float64, device="cuda"),
           "result": torch.full((4,), 77.0, dtype=torch.float64, device="cuda")}
    rd.d8_flow_accum_limited_dev(t, s, nodata, c, f, dir_nodata, nodata_out=nodata_out, **{k: buf[k] for k in want})
    torch.cuda.synchronize()
    for dev, host in ((t, dirs), (s, supply), (c, cap), (f, fac)):
        assert host is None or np.array_equal(dev.cpu().numpy().view(np.uint8), host.view(np.uint8)), "an input was written"
    got = {k: buf[k].cpu().numpy() for k in buf}
    for k in buf:
        if k not in want:
            assert (got[k] == 77.0).all(), k + " was not requested but written"
    return {k: got[k] for k in want}


def _both(rd, dirs, supply, nodata, cap=None, fac=None, dir_nodata=255, nodata_out=-1.0):
    """host and `_dev` results as {"out", "kept", "result": float64[4]}; the inputs are unchanged"""
    keep = [None if a is None else a.copy() for a in (dirs, supply, cap, fac)]
    host = rd.d8_flow_accum_limited(dirs, supply, nodata, cap, fac, dir_nodata, nodata_out)
    for a, k in zip((dirs, supply, cap, fac), keep):
        assert a is None or np.array_equal(a.view(np.uint8), k.view(np.uint8)), "an input was written"
    host["result"] = np.array([host["result"][k] for k in KEYS])
    return host, _dev(rd, dirs, supply, nodata, cap, fac, dir_nodata, nodata_out)


def _check(rd, what, dirs, supply, nodata, cap=None, fac=None, dir_nodata=255, nodata_out=-1.0):
    """host and `_dev` equal the model on every cell, and result equals the sums of the planes, which balance exactly"""
    r = lm.limited(dirs, supply, nodata, cap, fac, dir_nodata, nodata_out)
    assert _exact(r, supply, nodata, fac), what + ": the case is not dyadic enough for an equality"
    exp = np.array([float(r["result"][k]) for k in KEYS])
    assert all(Fraction(e) == r["result"][k] for e, k in zip(exp, KEYS))
    for name, got in zip(("host", "dev"), _both(rd, dirs, supply, nodata, cap, fac, dir_nodata, nodata_out)):
        _same(got["out"], r["out"], f"{what} out {name}")
        _same(got["kept"], r["kept"], f"{what} kept {name}")
        print(what, name, "result", got["result"].tolist())
        assert got["result"].tolist() == exp.tolist(), (what, name)
        assert got["result"][0] == got["result"][1] + got["result"][2] + got["result"][3]
    return r


def _fractal(rd, h, w, holes=False):
    """directions as the weighted tests take them: the engine's fill and flat resolution of a fractal DEM"""
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


def _supply(rng, shape, dtype, lo=-(2**10) + 1, hi=2**10):
    """k / 1024 of mixed sign, |k| < 2^10: every one is an f32"""
    return (rng.integers(lo, hi, shape).astype(np.float64) / 1024.0).astype(dtype)


def _limits(rng, shape, dtype, which):
    """capacity: k / 1024 in [-1, 8) with NaN (no limit) on a third of the cells; factor: 1 on most cells, 0, 0.25 and 0.5 on
    the others, zeros often enough that no path carries more than a few halvings (_exact asserts what that is for)"""
    cap = fac = None
    if which in ("capacity", "both"):
        cap = _supply(rng, shape, dtype, -1024, 8 * 1024)
        cap[rng.random(shape) < 0.33] = np.nan
    if which in ("factor", "both"):
        fac = rng.choice(np.array([1.0, 0.0, 0.5, 0.25], dtype), shape, p=[0.85, 0.09, 0.03, 0.03])
    return cap, fac


@pytest.mark.parametrize("which", LIMITS)
@pytest.mark.parametrize("dtype", FLOAT_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests(rd, shape, holes, dtype, which):
    dirs = _fractal(rd, *shape, holes=holes)
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    supply = _supply(rng, shape, dtype)
    cap, fac = _limits(rng, shape, dtype, which)
    r = _check(rd, f"fractal{shape}{holes}{np.dtype(dtype).name}{which}", dirs, supply, float(supply[0, -1]), cap, fac)
    assert (r["out"][dirs == 255] == -1).all() and ((dirs == 255).any() or not holes)
    if shape[0] * shape[1] > 4000:
        assert (r["kept"][dirs != 255] < 0).any() and (r["kept"] > 0).any() == (which != "none")


def _boustrophedon(h, w):
    """ONE path through every cell: along the rows, alternately east and west, one step south at the end of each"""
    order = []
    for y in range(h):
        order += [(x, y) for x in (range(w) if y % 2 == 0 else range(w - 1, -1, -1))]
    return sc.paint(sc.blank(h, w), order), order


@pytest.mark.parametrize("which", ["none", "capacity"])
def test_one_path_through_every_cell(rd, which):
    """257 x 259: 66 562 links, more than a tile's 4095 and than 65 535, across tile edges in every row.  Deficits alternate
    with supplies: the carried value is a random walk held at 0, which it hits and leaves thousands of times"""
    h, w = 257, 259
    dirs, order = _boustrophedon(h, w)
    rng = np.random.default_rng(3)
    supply = (rng.integers(-10, 9, (h, w)) / 8.0).astype(np.float32)        # a drift of -1/8 per cell: the walk keeps coming back
    cap = np.full((h, w), 2.5, np.float32) if which == "capacity" else None
    r = _check(rd, "snake " + which, dirs, supply, -9999.0, cap)
    carried, zeros, exp = 0.0, 0, np.empty((h, w))
    for x, y in order:                                       # the recurrence itself, beside the model
        carried = min(max(carried + float(supply[y, x]), 0.0), 2.5 if cap is not None else np.inf)
        zeros += carried == 0.0
        exp[y, x] = carried
    assert np.array_equal(r["out"], exp) and zeros > 5000 and (exp > 0).sum() > 5000


@pytest.mark.parametrize("at", [(20, 20), (64, 20), (63, 20), (20, 64), (64, 64), (63, 63)], ids=str)
def test_confluences_of_clamped_tributaries(rd, at):
    """three channels meet inside a tile, across a tile edge and across a tile corner; every tributary is clamped by a
    capacity one cell above the confluence and halved once on its way"""
    dirs = sc.three_way(at[0], at[1], (140, 135))
    rng = np.random.default_rng(at[0] + at[1])
    supply = (rng.integers(8, 64, dirs.shape) / 8.0).astype(np.float64)
    cap = np.full(dirs.shape, np.nan)
    fac = np.ones(dirs.shape)
    for dx, dy in ((-1, 0), (0, -1), (1, 0)):
        cap[at[1] + dy, at[0] + dx] = 1.5 + dx + dy          # 0.5, 0.5 and 2.5: below what arrives
        fac[at[1] + 3 * dy, at[0] + 3 * dx] = 0.5
    r = _check(rd, f"confluence{at}", dirs, supply, -1.0, cap, fac)
    assert r["out"][at[1], at[0]] == supply[at[1], at[0]] + 0.5 + 0.5 + 2.5
    _check(rd, f"confluence{at} f32", dirs, supply.astype(np.float32), -1.0, cap.astype(np.float32), fac.astype(np.float32))


@pytest.mark.parametrize("code", range(1, 9))
def test_one_direction_through_tile_edges_and_corners(rd, code):
    dirs = np.full((130, 130), code, np.uint8)
    rng = np.random.default_rng(code)
    supply = _supply(rng, dirs.shape, np.float32)
    cap, fac = _limits(rng, dirs.shape, np.float32, "both")
    _check(rd, f"uniform{code}", dirs, supply, -9999.0)
    _check(rd, f"uniform{code} both", dirs, supply, -9999.0, cap, fac)


@pytest.mark.parametrize("at", [(8, 5), (63, 20), (62, 20), (20, 63), (63, 63), (100, 127)], ids=str)
def test_loops_with_feeders(rd, at):
    """the weighted tests' 4-cell loops (in a tile, across an edge, across a corner) with their tributaries: a loop cell's out
    is 0 and its kept its own supply plus the out of the trees that enter there; a loop cell's own limits play no part"""
    dirs, loop, feeders = sc.loop_with_tributary(at[0], at[1], (150, 135))
    rng = np.random.default_rng(at[0])
    supply = (rng.integers(8, 64, dirs.shape) / 8.0).astype(np.float64)
    cap = np.full(dirs.shape, np.nan)
    trib = feeders[:5]
    cap[trib[-1][1], trib[-1][0]] = 3.0                       # the last cell before the loop
    for x, y in loop:
        cap[y, x] = 0.0
    s_ = lambda c: float(supply[c[1], c[0]])  # noqa: E731
    r = _check(rd, f"loop{at}", dirs, supply, -1.0)
    for x, y in loop:
        assert r["loop"][y, x] and r["out"][y, x] == 0
    assert r["kept"][loop[0][1], loop[0][0]] == s_(loop[0]) + sum(map(s_, feeders[:7]))
    assert r["kept"][loop[1][1], loop[1][0]] == s_(loop[1])
    r = _check(rd, f"loop{at} capacity", dirs, supply, -1.0, cap)
    assert r["kept"][loop[0][1], loop[0][0]] == s_(loop[0]) + 3.0
    assert r["result"]["left"] == sum(Fraction(s_((x, y))) for y in range(150) for x in range(135) if dirs[y, x] == 0)


def test_ring_through_twelve_tiles(rd):
    h = w = 250
    ring = [(x, 10) for x in range(10, 240)] + [(240, y) for y in range(10, 240)] + [(x, 240) for x in range(240, 10, -1)] + \
           [(10, y) for y in range(240, 10, -1)]
    assert len({(x // 64, y // 64) for x, y in ring}) == 12
    dirs = sc.paint(sc.blank(h, w), ring + [ring[0]], last=None)
    sc.paint(dirs, [(x, 100) for x in range(30, 10, -1)] + [(10, 100)], last=None)      # a tributary from inside
    supply = _supply(np.random.default_rng(1), (h, w), np.float32, 1, 1024)
    fac = np.full((h, w), 0.5, np.float32)
    r = _check(rd, "ring", dirs, supply, -1.0, None, None)
    assert r["kept"][100, 10] == float(supply[100, 10]) + float(supply[100, 11:31].astype(np.float64).sum()) and r["out"][100, 10] == 0
    assert r["kept"][10, 100] == supply[10, 100] and r["loop"].sum() == len(ring)
    r = _check(rd, "ring factor", dirs, supply, -1.0, None, fac)
    assert r["kept"][10, 100] == supply[10, 100] and 0 < r["kept"][100, 10] - float(supply[100, 10]) < 1


@pytest.mark.parametrize("dir_nodata", [0, 9, 255])
def test_direction_nodata_codes(rd, dir_nodata):
    dirs = _fractal(rd, 65, 130, holes=True)
    dirs[dirs == 255] = dir_nodata                                          # (with 0: the outlets do not participate either)
    rng = np.random.default_rng(dir_nodata)
    supply = _supply(rng, dirs.shape, np.float32)
    cap, fac = _limits(rng, dirs.shape, np.float32, "both")
    r = _check(rd, f"nodata{dir_nodata}", dirs, supply, 0.0, cap, fac, dir_nodata, nodata_out=-7.0)
    assert (dirs == dir_nodata).any() and (r["out"][dirs == dir_nodata] == -7).all() and (r["kept"][dirs == dir_nodata] == -7).all()
    r = _check(rd, "all nodata directions", np.full((65, 130), dir_nodata, np.uint8), supply, 0.0, cap, fac, dir_nodata)
    assert (r["out"] == -1).all() and r["result"]["supplied"] == 0


@pytest.mark.parametrize("dtype", FLOAT_TYPES, ids=lambda t: np.dtype(t).name)
def test_supply_nodata_nans_and_signed_zeros(rd, dtype):
    dirs = _fractal(rd, 65, 130)
    rng = np.random.default_rng(11)
    supply = _supply(rng, dirs.shape, dtype)
    supply[rng.random(dirs.shape) < 0.2] = -9999.0
    supply[rng.random(dirs.shape) < 0.2] = np.nan
    supply[3, :] = np.nan
    cap, fac = _limits(rng, dirs.shape, dtype, "both")
    _check(rd, "nan", dirs, supply, -9999.0, cap, fac)
    z = np.where(rng.random(dirs.shape) < 0.5, 0.0, -0.0).astype(dtype)     # -0.0 against a NoData of 0.0: nothing contributes
    z[rng.random(dirs.shape) < 0.05] = 1.0
    z[rng.random(dirs.shape) < 0.05] = -1.0
    _check(rd, "zeros", dirs, z, 0.0, cap, fac)
    _check(rd, "zeros nodata -0.0", dirs, z, -0.0)


@pytest.mark.parametrize("dtype", FLOAT_TYPES, ids=lambda t: np.dtype(t).name)
def test_capacity_values(rd, dtype):
    """NaN and +inf are no limit, a negative capacity is 0, and a NULL raster equals a raster of +inf"""
    dirs = _fractal(rd, 65, 130, holes=True)
    rng = np.random.default_rng(12)
    supply = _supply(rng, dirs.shape, dtype)
    cap = rng.choice(np.array([np.nan, np.inf, -2.0, 0.0, 0.5, 3.0], dtype), dirs.shape)
    r = _check(rd, "capacity values", dirs, supply, -9999.0, cap)
    part = dirs != 255
    assert (r["out"][part & (cap <= 0)] == 0).all() and (r["out"][part & (cap == 0.5)] <= 0.5).all()
    assert (r["out"][part & ~(cap < np.inf)] > 3.0).any()
    none = _both(rd, dirs, supply, -9999.0)
    inf = _both(rd, dirs, supply, -9999.0, np.full(dirs.shape, np.inf, dtype))
    for a, b in zip(none, inf):
        for k in ("out", "kept", "result"):
            assert np.array_equal(a[k], b[k]), k


def test_without_limits_it_is_the_weighted_accumulation(rd):
    dirs = _fractal(rd, 257, 259, holes=True)
    supply = _supply(np.random.default_rng(13), dirs.shape, np.float64, 0, 2**20)
    supply[5, :] = -9999.0
    exp = rd.d8_flow_accum_weighted(dirs, supply, -9999.0, sum_nodata=-1.0)
    for got in _both(rd, dirs, supply, -9999.0):
        assert np.array_equal(got["out"].view(np.uint64), exp.view(np.uint64))
        assert (got["kept"][dirs != 255] == 0).all() and (got["kept"][dirs == 255] == -1).all()
        assert got["result"][0] == got["result"][1] == float(supply[(dirs != 255) & (supply != -9999.0)].sum())


@pytest.mark.parametrize("want", [("out",), ("kept",), ("result",), ("out", "result"), ("kept", "out")], ids="+".join)
def test_output_subsets(rd, want):
    """a plane that is not requested is not written, and what is requested does not depend on the rest"""
    dirs = _fractal(rd, 65, 130, holes=True)
    rng = np.random.default_rng(14)
    supply = _supply(rng, dirs.shape, np.float32)
    cap, fac = _limits(rng, dirs.shape, np.float32, "both")
    full = _dev(rd, dirs, supply, -9999.0, cap, fac, 255, -1.0)
    part = _dev(rd, dirs, supply, -9999.0, cap, fac, 255, -1.0, want=want)
    host = rd.d8_flow_accum_limited(dirs, supply, -9999.0, cap, fac, want=[k for k in want if k != "result"])
    assert sorted(host) == sorted(set(want) | {"result"})
    for k in want:
        assert np.array_equal(part[k], full[k]), k
        assert np.array_equal(host[k] if k != "result" else np.array([host[k][n] for n in KEYS]), full[k]), k


@pytest.mark.parametrize("dtype", FLOAT_TYPES, ids=lambda t: np.dtype(t).name)
def test_float_supplies_within_the_bound(rd, dtype):
    """seeded random supplies of mixed sign, twenty binades apart, factors in [0, 1] and capacities: every out is within
    g * (sum of |s| over T(v)), g = k u / (1 - k u), of the model's EXACT rational value, every kept within that plus one
    rounding of its own, u |kept| -- the contract's bound, taken against exact values and never against a float re-summation"""
    dirs = _fractal(rd, 193, 70, holes=True)
    rng = np.random.default_rng(2)
    supply = (rng.standard_normal(dirs.shape) * np.exp(rng.uniform(-10, 10, dirs.shape))).astype(dtype)
    supply[rng.random(dirs.shape) < 0.05] = -9999.0
    fac = rng.random(dirs.shape).astype(dtype)
    fac[rng.random(dirs.shape) < 0.5] = 1.0
    cap = np.exp(rng.uniform(-5, 12, dirs.shape)).astype(dtype)
    cap[rng.random(dirs.shape) < 0.5] = np.nan
    r = lm.limited(dirs, supply, -9999.0, cap, fac)
    bound = lm.bound(dirs, supply, -9999.0)
    u = Fraction(1, 2**53)
    part = (dirs != 255).ravel()
    for name, got in zip(("host", "dev"), _both(rd, dirs, supply, -9999.0, cap, fac)):
        worst, inexact = Fraction(0), 0
        out, kept = got["out"].ravel().tolist(), got["kept"].ravel().tolist()
        for c in np.flatnonzero(part).tolist():
            eo, ek = abs(Fraction(out[c]) - r["out_exact"][c]), abs(Fraction(kept[c]) - r["kept_exact"][c])
            assert eo <= bound[c] and ek <= bound[c] + u * abs(r["kept_exact"][c]), (name, c, float(eo), float(ek), float(bound[c]))
            if bound[c]:
                worst = max(worst, eo / bound[c])
            inexact += eo != 0
        assert np.array_equal(got["out"].ravel()[~part], r["out"].ravel()[~part])
        print(name, np.dtype(dtype).name, "cells:", int(part.sum()), "inexact out:", inexact, "largest error / bound:", float(worst))
        assert inexact > 1000                                                 # the supplies did exercise the rounding
        res = got["result"]
        assert abs(res[0] - (res[1] + res[2] + res[3])) <= 1e-9 * (abs(res[2]) + abs(res[3]) + abs(res[1]))


def test_same_result_after_the_workspace_is_released(rd):
    dirs = _fractal(rd, 193, 70)
    rng = np.random.default_rng(0)
    supply = _supply(rng, dirs.shape, np.float32)
    first = rd.d8_flow_accum_limited(dirs, supply, 5.0)
    rd.release_workspace()
    again = rd.d8_flow_accum_limited(dirs, supply, 5.0)
    assert all(np.array_equal(first[k], again[k]) for k in ("out", "kept")) and first["result"] == again["result"]
    _check(rd, "small after large", dirs[:5, :7].copy(), supply[:5, :7].copy(), 5.0)   # stale scratch must not matter


def test_the_references_move_water_into_pits(rd):
    """tests/golden/ref_limited.npz: the reference's descent on its own flow directions.  min(kept, 0) is its wtd afterwards
    and the out of the cells without a link, summed per label, its water_vol per depression -- both bit for bit"""
    for name, dirs, label, tables in lm.reference_cases():
        link = lm.wm.links(dirs)[1]
        for k, (supply, after, vol) in enumerate(tables):
            for which, got in zip(("host", "dev"), _both(rd, dirs, supply, np.nan)):
                assert np.array_equal(np.minimum(got["kept"], 0.0), after), (name, k, which)
                assert np.array_equal(lm.per_label_left(got["out"], link, label, vol.size), vol), (name, k, which)
                assert got["result"][1] == vol.sum() and got["result"][2] == 0


def test_feeding_fill_spill_merge(rd):
    """INTEGRATION.md's composition on a 200 x 130 DEM: D8 directions of the unfilled DEM, supply = rain - deficit, the out of
    the cells without a link as Fill-Spill-Merge's water raster: its water_in is result.left"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden_dephier import perm_case

    dem = perm_case(np.int32, 200, 130, 705)
    rng = np.random.default_rng(705)
    rain = np.full(dem.shape, 0.5)
    deficit = rng.integers(0, 2048, dem.shape) / 1024.0
    dirs = rd.d8_flow_directions(dem, -2**31)
    r = rd.d8_flow_accum_limited(dirs, rain - deficit, np.nan)
    link = np.array(lm.wm.links(dirs)[1]).reshape(dem.shape)
    water = np.where(link < 0, r["out"], 0.0)
    labels, table = rd.depression_hierarchy(dem)
    depth, res = rd.fill_spill_merge(dem, labels, table, water)
    assert res["water_in"] == r["result"]["left"] == water.sum() and r["result"]["left"] > 0
    assert r["result"]["kept_neg"] == np.minimum(r["kept"], 0.0).sum() < 0 and r["result"]["kept_pos"] == 0
    assert abs(res["standing"] + res["ocean"] - res["water_in"]) <= dem.size * 2.0**-52 * res["water_in"]
