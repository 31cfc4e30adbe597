"""rdgpu_fill_spill_merge_<T> and its _dev form on the GPU against the model of the contract (tests/fsm_model.py): both
doors on every golden case and water, every element type, the hand-made rasters, the cascade of roots and the rasters
shaped for the kernels' seams (tests/fsm_cases.py); non-dyadic water; the refusals.

Every water value but the non-dyadic test's is a multiple of 2^-10 and the f32 elevations are dyadic, so every gather
sum and every prefix sum is exact in any order: node_water, the lake counts and the lake tops must then equal the
model's exactly, and a depth may differ from the model's by the rounding of one division and one subtraction."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from digest import load_golden  # noqa: E402
import dephier_model as dm  # noqa: E402
import fsm_cases as fc  # noqa: E402
import fsm_model as fm  # noqa: E402
from make_golden_dephier import perm_case  # noqa: E402

pytestmark = pytest.mark.gpu

TYPES = {"u8": np.uint8, "i8": np.int8, "i16": np.int16, "u16": np.uint16, "i32": np.int32, "u32": np.uint32, "f32": np.float32}
SUFFIX = {np.dtype(v): k for k, v in TYPES.items()}
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 2, 3


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_door(rd, dem, labels, table, water, want_nw=True, depth=None):
    """the raw host entry: (rc, depth, node_water, result)"""
    h, w = dem.shape
    depth = np.full((h, w), -7.0) if depth is None else depth
    nw = np.full(len(table), -7.0) if want_nw else None
    res = np.zeros(1, rd.FSM_RESULT_DTYPE)
    rc = getattr(rd.lib(), "rdgpu_fill_spill_merge_" + SUFFIX[dem.dtype])(
        _ptr(dem), w, h, _ptr(labels), _ptr(table) if len(table) else None, ctypes.c_uint32(len(table)), _ptr(water), _ptr(depth),
        _ptr(nw) if want_nw and len(table) else None, _ptr(res))
    return rc, depth, nw, res[0]


def dev_door(rd, dem, labels, table, water, want_nw=True):
    """the raw _dev entry on torch tensors (the elevations go up as bytes: torch has no tensor type for some of them)"""
    import torch

    h, w = dem.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d, lab, wat = up(dem), up(labels), up(water)
    tab = up(table) if len(table) else None
    depth = torch.full((h, w), -7.0, dtype=torch.float64, device="cuda")
    nw = torch.full((max(len(table), 1),), -7.0, dtype=torch.float64, device="cuda")
    res = torch.zeros(rd.FSM_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = getattr(rd.lib(), "rdgpu_fill_spill_merge_dev_" + SUFFIX[dem.dtype])(
        p(d), w, h, p(lab), p(tab), ctypes.c_uint32(len(table)), p(wat), p(depth), p(nw) if want_nw and len(table) else None, p(res),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), dem.view(np.uint8).reshape(-1)) and np.array_equal(wat.cpu().numpy(), water.view(np.uint8).reshape(-1))
    return rc, depth.cpu().numpy(), nw.cpu().numpy()[:len(table)] if want_nw else None, res.cpu().numpy().view(rd.FSM_RESULT_DTYPE)[0]


def check_both_doors(rd, dem, labels, table, water, exact=True, doors=(host_door, dev_door)):
    dem, labels, water = np.ascontiguousarray(dem), np.ascontiguousarray(labels, dtype=np.int32), np.ascontiguousarray(water, dtype=np.float64)
    r = fm.fill_spill_merge(dem, labels, table, water)
    cells, win = dem.size, r["water_in"]
    for door in doors:
        rc, depth, nw, res = door(rd, dem, labels, table, water)
        assert rc == OK, (door.__name__, rd.last_error() if hasattr(rd, "last_error") else rc)
        assert (int(res["lakes"]), int(res["full_lakes"])) == (r["lakes"], r["full_lakes"]), door.__name__
        if exact:
            assert np.array_equal(nw, r["node_water"]), door.__name__
            assert np.array_equal(np.flatnonzero(fm.lake_tops(table, nw) == np.arange(len(table))), r["tops"])
            assert float(res["water_in"]) == win
            # one division and one subtraction: 4 ulp of the lake's level
            lvl = np.where(np.isfinite(r["cell_level"]), np.abs(r["cell_level"]), 0.0)
            tol = 4.0 * np.spacing(lvl) * np.isfinite(r["cell_level"])
        else:
            # a gather error of delta moves a level by at most delta: at least one cell is wet
            tol = np.full(dem.shape, 2.0 ** -40 * max(1.0, win))
            assert np.allclose(nw, r["node_water"], rtol=0, atol=2.0 ** -40 * max(1.0, win))
        err = np.abs(depth - r["depth"])
        print(door.__name__, "largest depth error", float(err.max()), "of", float(tol.max()), "lakes", r["lakes"], "records", r["records"])
        assert (err <= tol).all(), door.__name__
        assert (depth[[0, -1], :] == 0).all() and (depth[:, [0, -1]] == 0).all()
        bound = cells * 2.0 ** -52 * win
        assert abs(float(res["ocean"]) - r["ocean"]) <= bound and abs(float(res["standing"]) - r["standing"]) <= bound
        assert abs(float(res["standing"]) - float(depth.sum())) <= bound
        # the same without node_water
        rc2, depth2, _, res2 = door(rd, dem, labels, table, water, want_nw=False)
        assert rc2 == OK and np.array_equal(depth2, depth) and res2.tobytes()[24:] == res.tobytes()[24:]
        assert abs(float(res2["ocean"]) - float(res["ocean"])) <= bound
    return r


@functools.lru_cache(maxsize=None)
def _golden():
    G = load_golden(os.path.join(GOLDEN, "ref_fsm.npz"))
    out = {}
    for name, k, dem, water, wtd, _ in fc.golden_cases(G):
        out.setdefault(name, (dem, []))[1].append((water, wtd))
    return out


@functools.lru_cache(maxsize=None)
def _hier(name, t):
    return dm.hierarchy(_golden()[name][0], t)


NAMES = ["frac_f32_40x30", "frac_f32_65x129", "frac_f32_300x257", "perm_i32_65x129", "perm_i32_200x130"]


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("name", NAMES)
def test_golden_cases_both_doors(rd, name, k):
    dem, waters = _golden()[name]
    labels, table = _hier(name, 8)
    water, wtd = waters[k]
    assert np.array_equal(water * 1024.0, np.round(water * 1024.0))
    r = check_both_doors(rd, dem, labels, table, water)
    # and the reference itself, every cell: the model's bound plus the depth's own rounding
    _, depth, _, _ = host_door(rd, np.ascontiguousarray(dem), np.ascontiguousarray(labels), table, np.ascontiguousarray(water))
    span = float(dem.max()) - float(dem.min())
    assert float(np.abs(depth - wtd).max()) <= 2.0 ** -44 * max(1.0, span)
    assert r["lakes"] > 0 or k == 3


@pytest.mark.parametrize("name,k", [("frac_f32_65x129", 1), ("perm_i32_200x130", 0)])
def test_topology_4_hierarchies(rd, name, k):
    dem, waters = _golden()[name]
    labels, table = _hier(name, 4)
    check_both_doors(rd, dem, labels, table, waters[k][0])


@pytest.mark.parametrize("suf", list(TYPES))
def test_every_element_type(rd, suf):
    p = perm_case(np.int32, 65, 129, 31).astype(np.int64)          # -4192 .. 4192, locally shuffled
    if suf == "u8":
        dem = (p % 256).astype(np.uint8)
    elif suf == "i8":
        dem = (p % 256 - 128).astype(np.int8)
    elif suf == "u16":
        dem = (p + 5000).astype(np.uint16)
    elif suf == "u32":
        dem = (p + 0x7FFFFFF0).astype(np.uint32)                     # both sides of the sign bit
    elif suf == "f32":
        dem = (p * 0.25).astype(np.float32)
    else:
        dem = p.astype(TYPES[suf])
    labels, table = dm.hierarchy(dem, 8)
    water = np.full(dem.shape, 0.5)
    water[::7, ::5] = 40.0 + 1.0 / 1024.0
    r = check_both_doors(rd, dem, labels, table, water)
    assert r["lakes"] > 5 and r["full_lakes"] < r["lakes"]


@pytest.mark.parametrize("name", list(fc.hand_made()))
def test_hand_made_rasters(rd, name):
    dem, water, exp = fc.hand_made()[name]
    labels, table = dm.hierarchy(dem, 8)
    check_both_doors(rd, dem, labels, table, water)
    for door in (host_door, dev_door):
        rc, depth, nw, res = door(rd, dem, labels, table, water)
        assert rc == OK and nw.tolist() == exp["node_water"] and float(res["ocean"]) == exp["ocean"]
        assert float(np.abs(depth - exp["depth"]).max()) <= 4 * np.spacing(128.0)      # (no level above 230)


def test_cascade_of_roots(rd):
    dem, water = fc.cascade()
    labels, table = dm.hierarchy(dem, 8)
    r = check_both_doors(rd, dem, labels, table, water)
    st = rd.fsm_stats()
    assert st["longest_pour"] == r["longest_pour"] == fc.CASCADE_PITS - 1 and st["pours"] == 1
    assert (st["lakes"], st["partial_lakes"], st["records"]) == (fc.CASCADE_PITS, 0, 0)


def test_one_segment_across_many_scan_blocks(rd):
    dem, water = fc.bowl_130()
    labels, table = dm.hierarchy(dem, 8)
    r = check_both_doors(rd, dem, labels, table, water)
    st = rd.fsm_stats()
    assert st["records"] == r["records"] == 127 * 127 and (st["lakes"], st["partial_lakes"]) == (1, 1)


def test_thousands_of_short_segments(rd):
    dem, water = fc.egg_carton()
    labels, table = dm.hierarchy(dem, 8)
    r = check_both_doors(rd, dem, labels, table, water)
    st = rd.fsm_stats()
    assert st["records"] == r["records"] and st["partial_lakes"] == r["lakes"] - r["full_lakes"] > 1000
    assert (st["shortcut_hits"], st["longest_pour"], st["pours"]) == (r["shortcut_hits"], r["longest_pour"], r["pours"])
    assert st["sort_bits"] == 32 + 11 and st["leaves"] == int(np.count_nonzero(table["lchild"] == dm.NONE))


@pytest.mark.parametrize("shape", [(40, 1), (40, 3), (3, 257), (1, 1)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_thin_rasters(rd, shape):
    from richdem_amd.synth import fractal_dem

    h, w = shape
    dem = np.ascontiguousarray(np.floor(fractal_dem(max(w, 4), max(h, 4), 9)[:h, :w]).astype(np.int32))
    labels, table = dm.hierarchy(dem, 8)
    assert len(table) <= 40
    water = np.full(shape, 3.0 / 1024.0)
    r = check_both_doors(rd, dem, labels, table, water)
    if len(table) == 0:
        assert r["ocean"] == r["water_in"] and r["lakes"] == 0


def test_non_dyadic_water(rd):
    dem, _ = _golden()["perm_i32_65x129"]
    labels, table = _hier("perm_i32_65x129", 8)
    water = np.full(dem.shape, 0.1)
    r = check_both_doors(rd, dem, labels, table, water, exact=False)
    assert r["records"] > 20 and 0 < r["full_lakes"] < r["lakes"]


def test_api_functions(rd):
    import torch

    dem, water, exp = fc.hand_made()["both_full_parent_lake"]
    labels, table = rd.depression_hierarchy(dem)
    depth, res = rd.fill_spill_merge(dem, labels, table, water)
    assert float(np.abs(depth - exp["depth"]).max()) <= 4 * np.spacing(9.0) and res["node_water"].tolist() == exp["node_water"]
    assert (res["lakes"], res["full_lakes"], res["ocean"], res["water_in"]) == (1, 0, 0.0, 20.0)
    assert "node_water" not in rd.fill_spill_merge(dem, labels, table, water, node_water=False)[1]
    st = rd.fsm_stats()
    assert st["nodes"] == 3 and st["leaves"] == 2 and st["records"] == 15 and st["host_ms"] > 0
    d, lab, wat = torch.from_numpy(dem).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(water).cuda()
    tab = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    out, nw = torch.empty_like(wat), torch.zeros(3, dtype=torch.float64, device="cuda")
    got = rd.fill_spill_merge_dev(d, lab, tab, 3, wat, out, nw).cpu().numpy().view(rd.FSM_RESULT_DTYPE)[0]
    assert np.array_equal(out.cpu().numpy(), depth) and nw.cpu().tolist() == exp["node_water"] and int(got["lakes"]) == 1
    # the stages are timed under "fsm."
    rd.lib().rdgpu_profile_enable(1)
    try:
        rd.lib().rdgpu_profile_reset()
        rd.fill_spill_merge(dem, labels, table, water)
        rd.lib().rdgpu_profile_collect()
        names, i = set(), 0
        while True:
            s = rd.lib().rdgpu_profile_name(i)
            if not s:
                break
            names.add(s.decode())
            i += 1
    finally:
        rd.lib().rdgpu_profile_enable(0)
    assert {"fsm.extract", "fsm.gather", "fsm.host_pass", "fsm.sort", "fsm.scan", "fsm.level", "fsm.depth"} <= names


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _small():
    dem, water, _ = fc.hand_made()["both_full_parent_lake"]
    labels, table = dm.hierarchy(dem, 8)
    return np.ascontiguousarray(dem), np.ascontiguousarray(labels), table.copy(), water.copy()


@pytest.mark.parametrize("bad", [-1.0 / 1024.0, np.nan, np.inf, -np.inf])
def test_unsupported_water_leaves_the_depth_alone(rd, bad):
    dem, labels, table, water = _small()
    water[3, 4] = bad
    for door in (host_door, dev_door):
        rc, depth, nw, res = door(rd, dem, labels, table, water)
        assert rc == ERR_UNSUPPORTED and (depth == -7.0).all() and (nw == -7.0).all(), door.__name__


def test_refused_arguments(rd):
    dem, labels, table, water = _small()
    for door in (host_door, dev_door):
        lab = labels.copy()
        lab[2, 2] = 2                                               # == leaves
        rc, depth, nw, _ = door(rd, dem, lab, table, water)
        assert rc == ERR_ARG and (depth == -7.0).all() and (nw == -7.0).all()
        lab[2, 2] = -2
        assert door(rd, dem, lab, table, water)[0] == ERR_ARG
        tab = table.copy()
        tab["lchild"][2] = 2                                        # a child id not below its parent's
        rc, depth, nw, _ = door(rd, dem, labels, tab, water)
        assert rc == ERR_ARG and (depth == -7.0).all() and (nw == -7.0).all()
        tab = table.copy()
        tab["geolink"][0] = 2                                       # not a leaf
        assert door(rd, dem, labels, tab, water)[0] == ERR_ARG
        tab = table.copy()
        tab["parent"][0] = 7                                        # out of range
        assert door(rd, dem, labels, tab, water)[0] == ERR_ARG
    L = rd.lib()
    depth = np.full(dem.shape, -7.0)
    res = np.zeros(1, rd.FSM_RESULT_DTYPE)
    f = L.rdgpu_fill_spill_merge_i32
    args = [_ptr(dem), 7, 5, _ptr(labels), _ptr(table), ctypes.c_uint32(3), _ptr(water), _ptr(depth), None, _ptr(res)]
    assert f(*args) == OK and (depth != -7.0).all()
    depth[:] = -7.0
    for i, v in ((0, None), (3, None), (4, None), (6, None), (7, None), (1, 0), (2, -5), (7, _ptr(water))):
        a = list(args)
        a[i] = v
        assert f(*a) == ERR_ARG, i
        assert (depth == -7.0).all()
    # a table that belongs to another DEM: unspecified values, an ordinary return
    other = dm.hierarchy(fc.hand_made()["first_spills_into_second"][0], 8)[1].copy()
    other["volume"] = [1e300, 0.0, 5.0]
    other["geolink"] = [0, 1, 1]
    water[2, 3] = 1.0                                               # leaf 1: full from the start, and its geolink is itself
    assert host_door(rd, dem, labels, other, water)[0] == OK
    for suf, dt in (("f64", np.float64), ("i64", np.int64), ("u64", np.uint64)):
        z = np.zeros((5, 7), dt)
        assert getattr(L, "rdgpu_fill_spill_merge_" + suf)(_ptr(z), 7, 5, _ptr(labels), _ptr(table), ctypes.c_uint32(3), _ptr(water),
                                                             _ptr(depth), None, None) == ERR_UNSUPPORTED
        assert getattr(L, "rdgpu_fill_spill_merge_dev_" + suf)(None, 7, 5, None, None, ctypes.c_uint32(0), None, None, None, None,
                                                                 None) == ERR_UNSUPPORTED
    assert (depth == -7.0).all()


def test_every_new_symbol_is_exported(rd):
    L = rd.lib()
    for suf in list(TYPES) + ["f64", "i64", "u64"]:
        assert hasattr(L, f"rdgpu_fill_spill_merge_{suf}") and hasattr(L, f"rdgpu_fill_spill_merge_dev_{suf}")
    assert hasattr(L, "rdgpu_fsm_get_stats") and callable(rd.fill_spill_merge) and callable(rd.fsm_stats)
