"""Upslope cells, catchments and outlets on the engine (csrc/upslope.hip).  d8_upslope_cells against the COMPILED
REFERENCE's rasters (tests/golden/ref_upslope.npz) through the host C-ABI (richdem_amd.api over ctypes) and the `_dev`
entries (torch tensors); catchments and outlets against the numpy model (tests/upslope_model.py, itself pinned to the
reference by tests/test_upslope_model.py) on the same rasters and on fresh seeded shapes.  Every comparison is exact and
over every cell; inputs must be unchanged afterwards."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from digest import load_golden  # noqa: E402
import upslope_model as um  # noqa: E402

pytestmark = pytest.mark.gpu

G = load_golden(os.path.join(GOLDEN, "ref_upslope.npz"))
CASES = sorted({k.split("/")[0] for k in G})


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got != exp).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad)


def _dev_catchments(rd, dirs, cells, labels, unreached, nodata):
    import torch

    t = torch.from_numpy(dirs.copy()).cuda()
    keep = t.clone()
    c = torch.from_numpy(np.asarray(cells, np.uint32).view(np.int32).copy()).cuda()
    lab = torch.from_numpy(np.asarray(labels, np.int32).copy()).cuda()
    out = torch.full(dirs.shape, 123456, dtype=torch.int32, device="cuda")
    rd.d8_catchments_dev(t, c, lab, out, unreached, nodata)
    torch.cuda.synchronize()
    assert torch.equal(t, keep)
    return out.cpu().numpy()


def _dev_outlets(rd, dirs, nodata):
    import torch

    t = torch.from_numpy(dirs.copy()).cuda()
    keep = t.clone()
    out = torch.full(dirs.shape, 123456, dtype=torch.int32, device="cuda")
    rd.d8_outlets_dev(t, out, nodata)
    torch.cuda.synchronize()
    assert torch.equal(t, keep)
    return out.cpu().numpy().view(np.uint32)


def _dev_upslope(rd, t, ln, nodata):
    import torch

    out = torch.full(tuple(t.shape), 77, dtype=torch.uint8, device="cuda")
    rd.d8_upslope_cells_dev(t, *ln, out, nodata)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_upslope_cells_every_entry_equals_the_reference(rd, case):
    import torch

    dirs, nodata = G[case + "/dirs"], int(G[case + "/nodata"])
    keep = dirs.copy()
    t = torch.from_numpy(dirs.copy()).cuda()
    t_keep = t.clone()
    for i, ln in enumerate(G[case + "/lines"]):
        ln = tuple(int(v) for v in ln)
        exp = G[f"{case}/up{i}"]
        _same(rd.d8_upslope_cells(dirs, *ln, nodata=nodata), exp, f"{case} line {ln} host")
        _same(_dev_upslope(rd, t, ln, nodata), exp, f"{case} line {ln} dev")
    assert np.array_equal(dirs, keep) and torch.equal(t, t_keep)


def _seeds_for(dirs, nodata, rng, n):
    """many seeds: random cells, two on one path, duplicate cells with different labels, NoData / NO_FLOW cells, corners"""
    h, w = dirs.shape
    if n == 1:
        return rng.integers(0, h * w, 1).astype(np.uint32), np.array([41], np.int32)
    cells = list(rng.integers(0, h * w, max(n, 3)))
    c0 = int(cells[0])
    d = int(dirs.ravel()[c0])
    if 1 <= d <= 8 and d != nodata:                                        # the cell downstream of the first seed
        x, y = c0 % w + int(um.D8X[d]), c0 // w + int(um.D8Y[d])
        if 0 <= x < w and 0 <= y < h:
            cells.append(y * w + x)
    cells += [cells[1], cells[2], cells[1]]                                # duplicates, other labels
    cells += list(np.flatnonzero(dirs.ravel() == nodata)[:3]) + list(np.flatnonzero(dirs.ravel() == 0)[:3])
    cells += [0, w - 1, (h - 1) * w, h * w - 1]
    cells = np.array(cells, np.uint32)
    labels = (rng.integers(-2**31, 2**31, cells.size)).astype(np.int32)
    return cells, labels


@pytest.mark.parametrize("case", CASES)
def test_catchments_and_outlets_equal_the_model(rd, case):
    dirs, nodata = G[case + "/dirs"], int(G[case + "/nodata"])
    keep = dirs.copy()
    h, w = dirs.shape
    rng = np.random.default_rng(len(case) * 7919 + h * 31 + w)
    exp_o = um.outlets(dirs, nodata)
    _same(rd.d8_outlets(dirs, nodata), exp_o, case + " outlets host")
    _same(_dev_outlets(rd, dirs, nodata), exp_o, case + " outlets dev")
    for n, unreached in ((1, 0), (max(2, h * w // 50), -7), (0, 5)):
        cells, labels = _seeds_for(dirs, nodata, rng, n) if n else (np.zeros(0, np.uint32), np.zeros(0, np.int32))
        exp = um.catchments(dirs, cells, labels, unreached, nodata)
        _same(rd.d8_catchments(dirs, cells, labels, unreached, nodata), exp, f"{case} catchments host {cells.size} seeds")
        _same(_dev_catchments(rd, dirs, cells, labels, unreached, nodata), exp, f"{case} catchments dev {cells.size} seeds")
    # consistency of the three products
    for ln in G[case + "/lines"][:4]:
        ln = tuple(int(v) for v in ln)
        lc = rd.d8_upslope_line(dirs.shape, *ln)
        c = rd.d8_catchments(dirs, lc, np.ones(lc.size, np.int32), 255, nodata).astype(np.uint8)
        c.ravel()[lc] = 2
        _same(rd.d8_upslope_cells(dirs, *ln, nodata=nodata), c, f"{case} upslope == catchments of the line {ln}")
    ids = np.unique(exp_o[exp_o != um.NONE])
    basins = rd.d8_catchments(dirs, ids, ids.view(np.int32), -1, nodata).view(np.uint32)
    # (NoData cells and cells that drain into a direction loop reach no seed: unreached -1 is the outlets' 0xFFFFFFFF)
    _same(basins, rd.d8_outlets(dirs, nodata), case + " catchments seeded with every outlet == outlets")
    assert np.array_equal(dirs, keep)


SHAPES = [(1, 1), (1, 64), (64, 1), (63, 65), (127, 129), (66, 191), (257, 131)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["random", "nodata", "loops"])
def test_fresh_shapes_equal_the_model(rd, shape, kind):
    """random direction codes (loops, NO_FLOW, codes above 8 and NoData included) on shapes that are not multiples of 4 or
    64; an all-NoData raster; a raster that is one big loop"""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w + len(kind))
    nodata = 255
    if kind == "random":
        dirs = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 200, 255], np.uint8), (h, w),
                          p=[.03, .1, .1, .1, .1, .15, .15, .1, .1, .02, .02, .03])
    elif kind == "nodata":
        dirs = np.full((h, w), 9, np.uint8)
        nodata = 9
    else:
        dirs = np.full((h, w), 5, np.uint8)                                 # east along the top, back west below: loops
        dirs[:, -1] = 7
        dirs[1::2, :] = 1
        dirs[1::2, 0] = 3
    keep = dirs.copy()
    exp_o = um.outlets(dirs, nodata)
    _same(rd.d8_outlets(dirs, nodata), exp_o, f"{shape} {kind} outlets host")
    _same(_dev_outlets(rd, dirs, nodata), exp_o, f"{shape} {kind} outlets dev")
    for n in (0, 1, 3 + h * w // 20):
        cells, labels = _seeds_for(dirs, nodata, rng, n) if n else (np.zeros(0, np.uint32), np.zeros(0, np.int32))
        exp = um.catchments(dirs, cells, labels, -5, nodata)
        _same(rd.d8_catchments(dirs, cells, labels, -5, nodata), exp, f"{shape} {kind} catchments host {cells.size} seeds")
        _same(_dev_catchments(rd, dirs, cells, labels, -5, nodata), exp, f"{shape} {kind} catchments dev {cells.size} seeds")
    for ln in ((0, 0, 0, 0), (w - 1, h - 1, w - 1, h - 1), (0, h // 2, w - 1, h // 2), (0, 0, w - 2, h - 1)):
        if um.line(shape, *ln) is None:
            continue
        exp = um.upslope_cells(dirs, *ln, nodata=nodata)
        _same(rd.d8_upslope_cells(dirs, *ln, nodata=nodata), exp, f"{shape} {kind} upslope host {ln}")
    assert np.array_equal(dirs, keep)


def test_argument_errors_write_nothing(rd):
    import torch

    L = rd.lib()
    dirs = np.full((10, 12), 5, np.uint8)
    out = np.full((10, 12), 1234, np.int32)
    cells = np.array([3, 120, 5], np.uint32)                                 # 120 == width * height: outside
    labels = np.array([1, 2, 3], np.int32)
    rc = L.rdgpu_d8_catchments(dirs.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint8(255), 12, 10,
                               cells.ctypes.data_as(ctypes.c_void_p), labels.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(3),
                               ctypes.c_int32(0), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 2 and (out == 1234).all()
    t = torch.from_numpy(dirs).cuda()
    o = torch.full((10, 12), 1234, dtype=torch.int32, device="cuda")
    with pytest.raises(rd.RdgpuError):
        rd.d8_catchments_dev(t, torch.from_numpy(cells.view(np.int32)).cuda(), torch.from_numpy(labels).cuda(), o)
    torch.cuda.synchronize()
    assert bool((o == 1234).all())
    u = torch.full((10, 12), 77, dtype=torch.uint8, device="cuda")
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_cells_dev(t, 0, 0, 11, 9, u)                           # a half step past the right edge
    with pytest.raises(rd.RdgpuError):
        rd.d8_upslope_cells(dirs, 0, 0, 12, 3)
    torch.cuda.synchronize()
    assert bool((u == 77).all())
    with pytest.raises(rd.RdgpuError):
        rd.d8_catchments(dirs, [[12, 0]], [1])
    with pytest.raises(rd.RdgpuError):
        rd.d8_outlets(dirs.astype(np.int32))
    xy = rd.d8_catchments(dirs, [[3, 2], [0, 0]], [8, 9], -1)                # (x, y) pairs
    assert np.array_equal(xy, um.catchments(dirs, [2 * 12 + 3, 0], [8, 9], -1))
