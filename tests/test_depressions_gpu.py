"""The depression inventory on the GPU, through the C-ABI (richdem_amd/api.py), against tests/depression_model.py: integer
element types equal in every field, floating point equal in everything but the volume, which is held to
|v - fsum| <= cells * 2^-52 * fsum (depression_model.compare)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depression_model as dm  # noqa: E402

pytestmark = pytest.mark.gpu
TOPOS = ((8, "D8"), (4, "D4"))
SENTINEL = (0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF, -1.5, -2.5, -3.5)


def _check(rd, orc, dem, topo, nm):
    exp_labels, exp_table = dm.depressions_model(orc, dem, topo)
    labels, table = rd.depressions(dem, nm)
    assert table.dtype == rd.DEPRESSION_DTYPE
    dm.compare(labels, table, exp_labels, exp_table, dem.dtype)
    return labels, table


@pytest.mark.parametrize("dtype", dm.DTYPES, ids=lambda d: np.dtype(d).name)
def test_hand_written_rasters_every_dtype(rd, orc, dtype):
    for name, rows in dm.HAND.items():
        for topo, nm in TOPOS:
            dem = np.array(rows, dtype)
            _, table = _check(rd, orc, dem, topo, nm)
            if name == "diagonal_pits":
                assert len(table) == (1 if topo == 8 else 2)
            if np.issubdtype(np.dtype(dtype), np.signedinteger) or np.issubdtype(np.dtype(dtype), np.floating):
                _check(rd, orc, (dem - 50).astype(dtype), topo, nm)   # elevations below zero


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)])
def test_rasters_without_interior(rd, orc, shape):
    dem = np.arange(shape[0] * shape[1], dtype=np.float32).reshape(shape)[::-1].copy()
    for topo, nm in TOPOS:
        labels, table = _check(rd, orc, dem, topo, nm)
        assert len(table) == 0 and not labels.any()


@pytest.mark.parametrize("dtype", [np.int32, np.uint8, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_lake_across_the_row_segment_boundary(rd, orc, dtype):
    dem = dm.lake_row(dtype)
    assert dem.shape == (5, 67)
    for topo, nm in TOPOS:
        _, table = _check(rd, orc, dem, topo, nm)
        assert len(table) == 1 and table["cells"][0] == 65 and table["outlet_cell"][0] == 2 * 67 + 66


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_rough_bowl_one_lake_many_basins(rd, orc, dtype):
    dem = dm.rough_bowl(dtype)
    if np.issubdtype(np.dtype(dtype), np.floating):   # values that differ in their last bits: the sums round
        dem[1:-1, 1:-1] += (np.random.default_rng(2).random((68, 128)) / 3).astype(dtype)
    assert dem.shape == (70, 130)
    for topo, nm in TOPOS:
        _, table = _check(rd, orc, dem, topo, nm)
        assert len(table) == 1 and table["cells"][0] == 68 * 128 and table["outlet_cell"][0] == 33 * 130
    assert rd.fill_stats()["basins"] > 100   # (of the last call: the lake is a union of many basins)


@pytest.mark.parametrize("topo,nm", TOPOS)
def test_random_u8_ties_everywhere(rd, orc, topo, nm):
    dem = np.random.default_rng(41).integers(0, 8, (150, 200)).astype(np.uint8)
    _, table = _check(rd, orc, dem, topo, nm)
    assert len(table) > 200


@pytest.fixture(scope="module")
def synth(rd):
    import torch

    t = torch.empty((260, 300), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(t, 7)
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_synthetic_dem(rd, orc, synth, dtype):
    dem = synth.astype(dtype)
    if dtype is np.float64:   # values no float32 holds: the dense-rank path has to carry them
        dem = dem + np.random.default_rng(3).random(dem.shape) * 1e-7
        assert not np.array_equal(dem.astype(np.float32).astype(np.float64), dem)
    _, table = _check(rd, orc, dem, 8, "D8")
    assert len(table) > 20
    _check(rd, orc, dem, 4, "D4")


def test_capacity(rd, orc):
    dem = np.random.default_rng(43).integers(0, 8, (60, 70)).astype(np.uint8)
    exp_labels, exp_table = dm.depressions_model(orc, dem, 8)
    n = len(exp_table)
    assert n > 10
    assert rd.depressions_into(dem, None, None) == n                      # the sizing call
    for cap in (0, n - 1, n + 5):
        labels = np.full(dem.shape, -7, np.int32)
        table = np.array([SENTINEL] * (cap + 3), rd.DEPRESSION_DTYPE)
        assert rd.depressions_into(dem, labels, table[:cap]) == n
        assert np.array_equal(labels, exp_labels)
        k = min(n, cap)
        dm.compare(None, table[:k], None, exp_table[:k], dem.dtype)
        assert (table[k:] == np.array([SENTINEL], rd.DEPRESSION_DTYPE)).all()   # nothing past the first min(N, capacity)


def test_without_labels(rd, orc):
    dem = np.random.default_rng(44).integers(0, 8, (40, 90)).astype(np.int16)
    exp_labels, exp_table = dm.depressions_model(orc, dem, 8)
    labels, table = rd.depressions(dem, "D8", labels=False)
    assert labels is None
    dm.compare(None, table, None, exp_table, dem.dtype)


def test_int64_is_unsupported(rd):
    for dtype in (np.int64, np.uint64):
        with pytest.raises(rd.RdgpuError) as e:
            rd.depressions(np.zeros((5, 5), dtype))
        assert e.value.code == 3   # RDGPU_ERR_UNSUPPORTED


def test_argument_errors(rd):
    L = rd.lib()
    import ctypes

    dem = np.zeros((4, 4), np.float32)
    n = ctypes.c_uint32()
    p = dem.ctypes.data_as(ctypes.c_void_p)
    assert L.rdgpu_depressions_f32(p, 4, 4, 8, None, None, 0, None) == 2          # null count
    assert L.rdgpu_depressions_f32(p, 4, 4, 8, None, None, 3, ctypes.byref(n)) == 2   # null table, capacity 3
    assert L.rdgpu_depressions_f32(p, 4, 4, 6, None, None, 0, ctypes.byref(n)) == 2   # topology
    assert L.rdgpu_depressions_f32(None, 4, 4, 8, None, None, 0, ctypes.byref(n)) == 2


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32], ids=lambda d: np.dtype(d).name)
def test_dev_entry_on_another_stream(rd, orc, synth, dtype):
    import torch

    dem = synth.astype(dtype) if dtype is not np.int32 else (synth * 4).astype(np.int32)
    exp_labels, exp_table = dm.depressions_model(orc, dem, 8)
    h_labels, h_table = rd.depressions(dem, "D8")
    n = len(h_table)
    t = torch.from_numpy(dem).cuda()
    labels = torch.full(dem.shape, -1, dtype=torch.int32, device="cuda")
    table = torch.zeros((n + 2, 5), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        count = rd.depressions_dev(t, labels, table, "D8")
        only_count = rd.depressions_dev(t, None, None, "D8")
    s.synchronize()
    assert int(count.item()) == n and int(only_count.item()) == n
    d_labels = labels.cpu().numpy()
    d_table = table.cpu().numpy().view(rd.DEPRESSION_DTYPE).ravel()
    assert np.array_equal(d_labels, h_labels)
    for f in ("first_cell", "pit_cell", "outlet_cell", "cells", "level", "pit_elevation"):
        assert np.array_equal(d_table[f][:n], h_table[f]), f
    dm.compare(h_labels, h_table, exp_labels, exp_table, dem.dtype)
    dm.compare(d_labels, d_table[:n], exp_labels, exp_table, dem.dtype)
    assert not d_table[n:].view(np.uint8).any()
    assert torch.equal(t.cpu(), torch.from_numpy(dem))   # the DEM is an input


@pytest.mark.parametrize("topo,nm", TOPOS)
def test_cross_checks_against_the_fill(rd, synth, topo, nm):
    """No model: the inventory against the engine's own fill."""
    for dem in (synth, np.random.default_rng(45).integers(0, 8, (90, 110)).astype(np.uint8)):
        filled = rd.FillDepressions(dem, topology=nm)
        labels, table = rd.depressions(dem, nm)
        mask = filled > dem
        assert np.array_equal(labels > 0, mask)
        assert int(table["cells"].sum()) == int(mask.sum())
        assert np.array_equal(np.bincount(labels.ravel(), minlength=len(table) + 1)[1:], table["cells"])
        z, f = dem.ravel(), filled.ravel()
        assert np.array_equal(z[table["outlet_cell"]].astype(np.float64), table["level"])
        assert np.array_equal(f[table["first_cell"]].astype(np.float64), table["level"])
        assert np.array_equal(z[table["pit_cell"]].astype(np.float64), table["pit_elevation"])
        assert (np.diff(table["first_cell"].astype(np.int64)) > 0).all()
