"""rdgpu_depression_hierarchy_ocean_<T> and its _dev form on the GPU against the model of the contract
(tests/dephier_ocean_model.py): every golden case of tests/golden/ref_dephier_ocean.npz and every element type, labels
and table field for field, the f32 volume within the header's bound; ocean == NULL and the ring mask against the entry
without a mask, byte for byte; the error and empty cases; small shapes with land on the border; the hand-made rasters."""
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
import dephier_ocean_model as om  # noqa: E402
from richdem_amd.synth import fractal_dem  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = dm.NONE
EXACT = ("parent", "lchild", "rchild", "pit_cell", "inside_cell", "outside_cell", "geolink", "cells", "level", "pit_elevation")
TYPES = {"u8": np.uint8, "i8": np.int8, "i16": np.int16, "u16": np.uint16, "i32": np.int32, "u32": np.uint32, "f32": np.float32}
SUFFIX = {np.dtype(v): k for k, v in TYPES.items()}
ERR_ARG, ERR_UNSUPPORTED = 2, 3


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden(os.path.join(GOLDEN, "ref_dephier_ocean.npz"))


CASES = [str(c) for c in _golden()["cases"]]


def case_dem(case):
    return om.golden_case_dem(_golden(), case)


def assert_same(got_labels, got, labels, tab, is_float):
    assert len(got) == len(tab)
    assert np.array_equal(got_labels, labels)
    for k in EXACT:
        assert np.array_equal(got[k], tab[k]), k
    if not is_float:
        assert np.array_equal(got["volume"], tab["volume"])
    else:
        # |v - exact| <= cells * 2^-52 * exact; the model's value is the exact one rounded once (2^-53)
        m = tab["volume"]
        tol = tab["cells"].astype(np.float64) * 2.0 ** -52 * m + 2.0 ** -53 * m
        assert (np.abs(got["volume"] - m) <= tol).all()


def dev_door(rd, dem, t, ocean):
    """(labels, table) through rdgpu_depression_hierarchy_ocean_dev_<T> (the elevations go up as bytes: torch has no tensor
    type for some of them); the sizing call first"""
    import torch

    h, w = dem.shape
    d = torch.from_numpy(np.ascontiguousarray(dem).view(np.uint8).reshape(-1).copy()).cuda()
    o = None if ocean is None else torch.from_numpy(np.ascontiguousarray(ocean).view(np.uint8).copy()).cuda()
    fn = getattr(rd.lib(), "rdgpu_depression_hierarchy_ocean_dev_" + SUFFIX[dem.dtype])
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    op = None if o is None else ctypes.c_void_p(o.data_ptr())
    cp, lp = ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(counts.data_ptr() + 4)
    assert fn(ctypes.c_void_p(d.data_ptr()), w, h, t, op, None, None, ctypes.c_uint32(0), cp, lp, stream) == 0
    torch.cuda.synchronize()
    n, leaves = (int(v) for v in counts.cpu())
    lab = torch.full((h, w), 77, dtype=torch.int32, device="cuda")
    table = torch.zeros(max(n, 1) * rd.DEPHIER_NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    assert fn(ctypes.c_void_p(d.data_ptr()), w, h, t, op, ctypes.c_void_p(lab.data_ptr()), ctypes.c_void_p(table.data_ptr()) if n else None,
              ctypes.c_uint32(n), cp, lp, stream) == 0
    torch.cuda.synchronize()
    assert [int(v) for v in counts.cpu()] == [n, leaves]
    assert np.array_equal(d.cpu().numpy(), np.ascontiguousarray(dem).view(np.uint8).reshape(-1))
    if o is not None:
        assert np.array_equal(o.cpu().numpy(), np.ascontiguousarray(ocean).view(np.uint8))      # the mask is never written
    got = table.cpu().numpy().view(rd.DEPHIER_NODE_DTYPE)[:n]
    assert leaves == int(np.count_nonzero(got["lchild"] == NONE))
    return lab.cpu().numpy(), got


def both_doors(rd, dem, t, ocean, expect=None):
    dem = np.ascontiguousarray(dem)
    labels, tab = om.hierarchy(dem, t, ocean) if expect is None else expect
    before, mask_before = dem.copy(), None if ocean is None else ocean.copy()
    got_labels, got = rd.depression_hierarchy(dem, t, ocean=ocean)
    assert dem.tobytes() == before.tobytes() and (ocean is None or np.array_equal(ocean, mask_before))
    assert_same(got_labels, got, labels, tab, dem.dtype.kind == "f")
    got_labels, got = dev_door(rd, dem, t, ocean)
    assert_same(got_labels, got, labels, tab, dem.dtype.kind == "f")
    return labels, tab


@functools.lru_cache(maxsize=None)
def _model(case, t):
    return om.hierarchy(case_dem(case), t, _golden()[case + "/mask"])


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("case", CASES)
def test_golden_cases_equal_the_model_through_both_doors(rd, case, t):
    both_doors(rd, case_dem(case), t, _golden()[case + "/mask"], expect=_model(case, t))


def typed_dem(suf, shape, seed=11):
    """a fractal in the element type's range: many equal elevations in the narrow types"""
    h, w = shape
    z = fractal_dem(w, h, seed).astype(np.float64)            # 0 .. 2000
    if suf == "f32":
        return z.astype(np.float32)
    scale, off = {"i32": (1000.0, -1_000_000), "u32": (1000.0, 0x7FFF0000), "i16": (30.0, -30000), "u16": (30.0, 0),
                  "i8": (1 / 8.0, -128), "u8": (1 / 8.0, 0)}[suf]
    return (np.floor(z * scale).astype(np.int64) + off).astype(TYPES[suf])


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("suf", list(TYPES))
def test_every_element_type(rd, suf, t):
    dem = typed_dem(suf, (129, 65))
    rng = np.random.default_rng(3)
    ocean = (rng.random(dem.shape) < 0.01).astype(np.uint8)
    ocean[0, :20] = 1                                         # a stretch of coast; the rest of the ring is land
    ocean[60:70, 30:40] = 1                                   # an inland sea
    both_doors(rd, dem, t, ocean)
    both_doors(rd, dem, t, ocean.astype(bool))                # (bool masks are taken as they are)


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("name", ["perm_u16_40x30", "perm_i32_65x129", "perm_f32_65x129", "frac_f32_200x130"])
def test_null_and_the_ring_mask_are_the_entry_without_a_mask(rd, name, t):
    """byte for byte: labels, counts and the whole table.  The f32 inputs are multiples of one power of two below 2^24 of
    it (make_golden_dephier.py), so their volume sums are exact in double in any order and reproducible."""
    dem = np.ascontiguousarray(load_golden(os.path.join(GOLDEN, "ref_dephier.npz"))[name + "/dem"])
    labels, tab = rd.depression_hierarchy(dem, t)
    suf = SUFFIX[dem.dtype]
    h, w = dem.shape
    for ocean in (None, om.ring_mask(dem.shape)):
        lab = np.full(dem.shape, 77, np.int32)
        table = np.zeros(len(tab), rd.DEPHIER_NODE_DTYPE)
        count, leaves = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = getattr(rd.lib(), "rdgpu_depression_hierarchy_ocean_" + suf)(
            dem.ctypes.data_as(ctypes.c_void_p), w, h, t, None if ocean is None else ocean.ctypes.data_as(ctypes.c_void_p),
            lab.ctypes.data_as(ctypes.c_void_p), table.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(table)),
            ctypes.byref(count), ctypes.byref(leaves))
        assert rc == 0 and count.value == len(tab) and leaves.value == int(np.count_nonzero(tab["lchild"] == NONE))
        assert lab.tobytes() == labels.tobytes() and table.tobytes() == tab.tobytes()
        lab_d, tab_d = dev_door(rd, dem, t, ocean)
        assert lab_d.tobytes() == labels.tobytes() and tab_d.tobytes() == tab.tobytes()


def test_no_ocean_is_refused_and_all_ocean_is_empty(rd):
    import torch

    dem = typed_dem("f32", (64, 64))
    h, w = dem.shape
    none = np.zeros(dem.shape, np.uint8)
    labels = np.full(dem.shape, 77, np.int32)
    table = np.zeros(8, rd.DEPHIER_NODE_DTYPE)
    table["cells"] = 0xABCD
    for t in (8, 4):
        count, leaves = ctypes.c_uint32(0xDEAD), ctypes.c_uint32(0xBEEF)
        rc = rd.lib().rdgpu_depression_hierarchy_ocean_f32(
            dem.ctypes.data_as(ctypes.c_void_p), w, h, t, none.ctypes.data_as(ctypes.c_void_p), labels.ctypes.data_as(ctypes.c_void_p),
            table.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(8), ctypes.byref(count), ctypes.byref(leaves))
        assert rc == ERR_ARG and b"no ocean cells" in rd.lib().rdgpu_last_error()
        assert (count.value, leaves.value) == (0xDEAD, 0xBEEF) and (labels == 77).all() and (table["cells"] == 0xABCD).all()
        # the device door: nothing is written either
        d, o = torch.from_numpy(dem.copy()).cuda(), torch.from_numpy(none).cuda()
        lab = torch.full(dem.shape, 77, dtype=torch.int32, device="cuda")
        tb = torch.full((8 * 56,), 0x5A, dtype=torch.uint8, device="cuda")
        with pytest.raises(rd.RdgpuError) as e:
            rd.depression_hierarchy_dev(d, lab, tb, t, ocean=o)
        torch.cuda.synchronize()
        assert e.value.code == ERR_ARG and bool((lab == 77).all()) and bool((tb == 0x5A).all())
        with pytest.raises(rd.RdgpuError):
            rd.depression_hierarchy(dem, t, ocean=none)
        # every cell ocean
        labs, tab = both_doors(rd, dem, t, np.ones(dem.shape, np.uint8))
        assert len(tab) == 0 and (labs == -1).all()
        assert rd.depression_hierarchy_into(dem, None, None, t, ocean=np.ones(dem.shape, np.uint8)) == (0, 0)
    with pytest.raises(rd.RdgpuError):
        rd.depression_hierarchy(dem, 8, ocean=np.zeros((3, 3), np.uint8))      # a mask of another shape
    # the other refusals are those of the entry without a mask
    p, op = dem.ctypes.data_as(ctypes.c_void_p), np.ones(dem.shape, np.uint8).ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 64, 64, 8), (p, 0, 64, 8), (p, 64, 64, 5), (p, 65536, 32768, 8)):
        count = ctypes.c_uint32(0xDEAD)
        assert rd.lib().rdgpu_depression_hierarchy_ocean_f32(*args, op, None, None, ctypes.c_uint32(0), ctypes.byref(count), None) == ERR_ARG
        assert count.value == 0xDEAD
    for suf, dt in (("f64", np.float64), ("i64", np.int64), ("u64", np.uint64)):
        z = np.zeros((8, 8), dt)
        count = ctypes.c_uint32(0xDEAD)
        assert getattr(rd.lib(), "rdgpu_depression_hierarchy_ocean_" + suf)(
            z.ctypes.data_as(ctypes.c_void_p), 8, 8, 8, op, None, None, ctypes.c_uint32(0), ctypes.byref(count), None) == ERR_UNSUPPORTED
        assert count.value == 0xDEAD
        assert getattr(rd.lib(), "rdgpu_depression_hierarchy_ocean_dev_" + suf)(None, 8, 8, 8, None, None, None, ctypes.c_uint32(0),
                                                                             None, None, None) == ERR_UNSUPPORTED
    for suf in TYPES:
        assert hasattr(rd.lib(), "rdgpu_depression_hierarchy_ocean_" + suf) and hasattr(rd.lib(), "rdgpu_depression_hierarchy_ocean_dev_" + suf)


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (129, 65), (130, 200)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_small_shapes_with_land_on_the_border(rd, shape, t):
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    for suf in ("i32", "u8", "f32"):
        dem = typed_dem(suf, shape, seed=7) if min(shape) > 3 else rng.permutation(h * w).reshape(shape).astype(TYPES[suf])
        ocean = np.zeros(shape, np.uint8)
        ocean.ravel()[int(rng.integers(h * w))] = 1           # ONE ocean cell, anywhere: the ring is land
        labels, tab = both_doors(rd, dem, t, ocean)
        if min(shape) > 3:
            ring = om.ring_mask(shape).astype(bool) & (ocean == 0)
            assert (labels[ring] >= 0).any()                  # land on the border belongs to depressions


def test_the_hand_made_rasters(rd):
    z = np.array([[1, 4, 6], [3, 5, 7], [8, 2, 9]], np.int32)
    ocean = np.zeros((3, 3), np.uint8)
    ocean[2, 2] = 1
    labels, tab = both_doors(rd, z, 8, ocean)                 # a land pit in the corner, the ocean cell the highest
    assert labels.tolist() == [[0, 0, 0], [0, 0, 1], [1, 1, -1]] and tab["outside_cell"][2] == 8 and tab["geolink"][2] == NONE
    both_doors(rd, z, 4, ocean)
    z = np.array([[7, 1, 5, 2, 8]], np.int16)
    ocean = np.array([[0, 0, 1, 0, 0]], np.uint8)
    for t in (8, 4):
        labels, tab = both_doors(rd, z, t, ocean)             # both pits spill over the ocean cell between them
        assert tab["outside_cell"].tolist() == [2, 2] and tab["level"].tolist() == [5, 5]
    z = np.array([[5, 3, 4, 1, 6, 2, 9, 0, 7]], np.uint8)
    ocean = np.zeros_like(z)
    ocean[0, 4] = 1
    for t in (8, 4):
        both_doors(rd, z, t, ocean)
        both_doors(rd, np.ascontiguousarray(z.T), t, np.ascontiguousarray(ocean.T))
        both_doors(rd, np.array([[4, 1], [3, 2]], np.float32), t, np.array([[1, 0], [0, 0]], np.uint8))
    # equal-valued ocean cells and an equal-valued plateau of land beside them
    z = np.full((6, 7), 4, np.int8)
    ocean = np.zeros_like(z, dtype=np.uint8)
    ocean[:, 0] = 1
    z[2:4, 3:6] = 1
    for t in (8, 4):
        both_doors(rd, z, t, ocean)
