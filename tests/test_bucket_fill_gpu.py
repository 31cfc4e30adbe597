"""rdgpu_bucket_fill_from_edges_<T> and its _dev form on the GPU against the model (tests/dephier_ocean_model.py:
connected components of the eligible cells) and the COMPILED REFERENCE's BucketFillFromEdges
(tests/golden/ref_dephier_ocean.npz), exactly: every byte of the mask and the count, both doors, both topologies."""
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
import dephier_ocean_model as om  # noqa: E402

pytestmark = pytest.mark.gpu

TYPES = {"u8": np.uint8, "i8": np.int8, "i16": np.int16, "u16": np.uint16, "i32": np.int32, "u32": np.uint32, "f32": np.float32,
         "f64": np.float64, "i64": np.int64, "u64": np.uint64}
SHAPES = [(1, 1), (1, 9), (9, 1), (64, 64), (129, 65), (300, 257)]     # (height, width)


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden(os.path.join(GOLDEN, "ref_dephier_ocean.npz"))


def dev_door(rd, check, value, mask, t):
    """bucket_fill_from_edges_dev on torch tensors; dtypes torch has no tensor type for go through the raw entry"""
    import torch

    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8).copy()).cuda()
    h, w = check.shape
    try:
        c = torch.from_numpy(check.copy()).cuda()
        filled = rd.bucket_fill_from_edges_dev(c, value, m, t)
    except (TypeError, rd.RdgpuError):
        suf = {np.dtype(v): k for k, v in TYPES.items()}[check.dtype]
        c = torch.from_numpy(check.view(np.uint8).reshape(-1).copy()).cuda()
        filled = torch.zeros(1, dtype=torch.int64, device="cuda")
        ct = {"u16": ctypes.c_uint16, "u32": ctypes.c_uint32, "u64": ctypes.c_uint64}[suf]
        rc = getattr(rd.lib(), "rdgpu_bucket_fill_from_edges_dev_" + suf)(
            ctypes.c_void_p(c.data_ptr()), w, h, t, ct(int(value)), ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(filled.data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy().view(np.uint8).reshape(-1), check.view(np.uint8).reshape(-1))   # check is not written
    return m.cpu().numpy(), int(filled.cpu()[0])


def both_doors(rd, check, value, mask, t, expect=None):
    check = np.ascontiguousarray(check)
    exp, n = om.bucket_fill(check, value, mask, t) if expect is None else expect
    before = check.copy()
    mask_in = None if mask is None else mask.copy()
    got, filled = rd.bucket_fill_from_edges(check, value, mask, t)
    assert check.tobytes() == before.tobytes() and (mask is None or np.array_equal(mask, mask_in))
    assert got.dtype == np.uint8 and np.array_equal(got, exp) and filled == n
    got, filled = dev_door(rd, check, value, np.zeros(check.shape, np.uint8) if mask is None else mask, t)
    assert np.array_equal(got, exp) and filled == n
    return exp, n


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_random_regions_at_every_shape(rd, shape, t):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for p in (0.45, 0.62, 0.9):            # around the percolation thresholds of D8 and D4, and nearly full
        check = (rng.random(shape) < p).astype(np.int16) * 7
        _, n = both_doors(rd, check, 7, None, t)
        pre = (rng.random(shape) < 0.1).astype(np.uint8) * 200          # any non-zero byte is "set", and stays as it is
        exp, _ = both_doors(rd, check, 7, pre, t)
        assert np.array_equal(exp[pre != 0], pre[pre != 0])
    if shape == (1, 1):
        assert n == 1                      # the only cell is a border cell


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("name", ["perm_u16_40x30", "perm_i32_65x129", "frac_f32_65x129", "frac_f32_200x130"])
def test_the_reference_on_the_golden_seas(rd, name, t):
    G = _golden()
    check = G[name + "/bucket/check"]
    ref = G[f"{name}/bucket/t{t}/mask"]
    both_doors(rd, check, 1, None, t, expect=(ref, int(ref.sum())))
    wall, ref = G[f"{name}/bucket_wall/t{t}/mask_in"], G[f"{name}/bucket_wall/t{t}/mask"]
    both_doors(rd, check, 1, wall, t, expect=(ref, int(ref.sum()) - int(wall.sum())))


def serpentine(n=130):
    """a one-cell-wide channel that runs the width to and fro on the odd rows, joined at alternate ends on the even rows:
    it crosses every 64-cell seam in every odd row and touches the border at its mouth (0, 1) alone"""
    c = np.zeros((n, n), np.uint8)
    c[1:n - 1:2, 1:n - 1] = 1
    c[2:n - 2:4, n - 2] = 1
    c[4:n - 2:4, 1] = 1
    c[0, 1] = 1
    return c


def spiral(n=97):
    c = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    c[0, 0] = 1
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        ahead2 = (ny + dy, nx + dx)
        if not (0 <= ny < n and 0 <= nx < n) or c[ny, nx] or (0 <= ahead2[0] < n and 0 <= ahead2[1] < n and c[ahead2]):
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            a2 = (ny + dy, nx + dx)
            if not (0 <= ny < n and 0 <= nx < n) or c[ny, nx] or (0 <= a2[0] < n and 0 <= a2[1] < n and c[a2]):
                break
        y, x = ny, nx
        c[y, x] = 1
    return c


@pytest.mark.parametrize("t", [8, 4])
def test_serpentine_and_spiral(rd, t):
    s = serpentine()
    exp, n = both_doors(rd, s, 1, None, t)
    assert n == int(s.sum()) > 130 * 40 and np.array_equal(exp, s)              # one channel, reached from its mouth alone
    cut = np.zeros_like(s)
    cut[64, :] = 1                                                              # a wall of pre-set bytes cuts the channel
    exp, n = both_doors(rd, s, 1, cut, t)
    assert (exp[65:] == 0).all() and (exp[64] == 1).all() and n == int(s[:64].sum())
    sp = spiral()
    # the outer turn of the spiral runs along the border ring; under D4 and D8 alike the whole arm is one component
    exp, n = both_doors(rd, sp, 1, None, t)
    assert n == int(sp.sum()) > 97 * 40


def test_lake_diagonal_nan_and_negative_zero(rd):
    c = np.zeros((9, 70), np.float32)
    c[3:6, 30:40] = 5.0                                                         # an enclosed lake: touches no edge
    for t in (8, 4):
        exp, n = both_doors(rd, c, 5.0, None, t)
        assert n == 0 and not exp.any()
    d = np.zeros((6, 66), np.int32)
    d[0, 63] = d[1, 64] = d[2, 65] = 1                                          # a diagonal across the 64-cell seam
    d[4, 1] = d[3, 0] = 1
    exp, n = both_doors(rd, d, 1, None, 8)
    assert n == 5
    exp, n = both_doors(rd, d, 1, None, 4)
    assert n == 3 and exp[1, 64] == 0 and exp[4, 1] == 0
    f = np.full((5, 5), np.nan, np.float32)
    assert both_doors(rd, f, np.nan, None, 8)[1] == 0                           # NaN equals nothing
    z = np.ones((4, 6), np.float64)
    z[0, 0], z[1, 1], z[2, 2] = 0.0, -0.0, 0.0
    exp, n = both_doors(rd, z, -0.0, None, 8)
    assert n == 3
    ring_free = np.zeros((8, 8), np.uint8)
    ring_free[1:-1, 1:-1] = 1                                                   # no eligible ring cell
    assert both_doors(rd, ring_free, 1, None, 8)[1] == 0


@pytest.mark.parametrize("shape", [(300, 257), (1024, 1024)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_every_cell_eligible(rd, shape):
    c = np.full(shape, -3, np.int8)
    for t in (8, 4):
        exp, n = both_doors(rd, c, -3, None, t, expect=(np.ones(shape, np.uint8), shape[0] * shape[1]))


@pytest.mark.parametrize("suf", list(TYPES))
def test_every_element_type(rd, suf):
    rng = np.random.default_rng(5)
    dt = TYPES[suf]
    hi = {"u8": 255, "i8": -128, "i16": -32768, "u16": 65535, "i32": -2 ** 31, "u32": 2 ** 32 - 1, "f32": -9999.0, "f64": 1e300,
          "i64": -2 ** 63, "u64": 2 ** 64 - 1}[suf]
    check = np.where(rng.random((70, 131)) < 0.6, dt(hi), dt(3)).astype(dt)
    both_doors(rd, check, hi, None, 8)
    both_doors(rd, check, hi, (rng.random((70, 131)) < 0.05).astype(np.uint8), 4)


def test_refused_arguments_and_exports(rd):
    L = rd.lib()
    c = np.zeros((8, 8), np.float32)
    m = np.full((8, 8), 9, np.uint8)
    p, mp = c.ctypes.data_as(ctypes.c_void_p), m.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 8, 8, 8, mp), (p, 8, 8, 8, None), (p, 0, 8, 8, mp), (p, 8, -1, 8, mp), (p, 8, 8, 6, mp), (p, 65536, 32768, 8, mp)):
        filled = ctypes.c_uint64(0xDEAD)
        assert L.rdgpu_bucket_fill_from_edges_f32(args[0], args[1], args[2], args[3], ctypes.c_float(0.0), args[4], ctypes.byref(filled)) == 2, args
        assert filled.value == 0xDEAD and (m == 9).all()
    assert L.rdgpu_bucket_fill_from_edges_f32(p, 8, 8, 8, ctypes.c_float(0.0), mp, None) == 0                # filled is nullable
    for suf in TYPES:
        assert hasattr(L, "rdgpu_bucket_fill_from_edges_" + suf) and hasattr(L, "rdgpu_bucket_fill_from_edges_dev_" + suf)
    assert rd.bucket_fill_from_edges(np.zeros((4, 4), np.uint8), 0.5)[1] == 0                               # no u8 equals 0.5
    with pytest.raises(rd.RdgpuError):
        rd.bucket_fill_from_edges(np.zeros((4, 4), np.uint8), 0, topology=5)


def test_ocean_mask_is_the_apps_rule(rd):
    G = _golden()
    dem = G["frac_f32_65x129/dem"].copy()
    q = np.sort(dem.ravel())[dem.size // 4]
    dem[dem < q] = -5.0                                                        # the sea, quantised to one level
    dem[40:55, 20:40] = -9999.0                                                # a NoData hole inside
    sea, _ = om.bucket_fill(dem, -5.0, None, 8)
    m = rd.ocean_mask(dem, ocean_level=-5.0, nodata=-9999.0)
    assert m.dtype == np.uint8 and np.array_equal(m != 0, (sea != 0) | (dem == -9999.0))
    mb = rd.ocean_mask(dem, ocean_level=-5.0, nodata=-9999.0, border=True)
    assert np.array_equal(mb != 0, (m != 0) | (om.ring_mask(dem.shape) != 0))
    assert np.array_equal(rd.ocean_mask(dem, border=True), om.ring_mask(dem.shape))
    assert np.array_equal(rd.ocean_mask(dem, nodata=-9999.0) != 0, dem == -9999.0)
