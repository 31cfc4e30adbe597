"""D-infinity across flats on the engine (csrc/mfd.hip: k_tarboton_flats) against the model composed from the CPU oracle
(tests/dinf_flats_model.py, pinned by tests/test_dinf_flats_model.py): proportions, statistics, accumulation, distance,
host and `_dev` entries, every element type, refused calls.

The kernel's tile is 64 x 32, so the rasters are 130 wide and 67 high: flats straddle a tile's column border and its row
border, and the last tiles are partial."""
import ctypes
import os
import sys

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinf_flats_model as model  # noqa: E402
import mfd_distance_model as dist_model  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 130, 67
NDV = np.float32(-9999)
ENV = "RDGPU_MFD_STACK_BELOW"
_CACHE = {}


def ulp_diff_f32(a, b):
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the cases ---------------------------------------------------------------------------------------------------
def rim(flat_or_lower):
    """10 + the Chebyshev distance to the cells given: rises away from them, no two equal neighbours without a lower one"""
    ys, xs = np.nonzero(flat_or_lower)
    yy, xx = np.mgrid[0:H, 0:W]
    return (10 + np.min(np.maximum(abs(yy[..., None] - ys), abs(xx[..., None] - xs)), axis=-1)).astype(np.float32)


def case_plateau():                                    # (a)
    flat = np.zeros((H, W), bool)
    flat[10:56, 20:111] = True
    low = flat.copy()
    low[30, 111:] = True
    z = rim(low)
    z[flat] = 5
    z[30, 111:] = 4 - 0.01 * np.arange(W - 111, dtype=np.float32)
    return z, NDV


def case_random(orc):                                  # (b)
    z = model.random_integer_dem(orc, 0, W, H)
    z[20:27, 60:70] = NDV
    z[40, 0] = NDV
    return z, NDV


def case_no_flats():                                   # (d)
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx + 0.37 * yy + 0.2 * np.random.default_rng(4).random((H, W))).astype(np.float32), NDV


def case_pit():                                        # (e): a level pit floor, no outlet; the DEM is not filled
    flat = np.zeros((H, W), bool)
    flat[28:36, 60:70] = True
    z = rim(flat)
    z[flat] = 5
    return z, NDV


def case_edge_flat():                                  # (f): a level area that includes cells of the raster's edge
    flat = np.zeros((H, W), bool)
    flat[25:45, 0:70] = True
    flat[0:12, 100:W] = True
    z = rim(flat)
    z[flat] = 5
    return z, NDV


CASES = {
    "a_plateau": lambda orc: case_plateau(),
    "b_random": case_random,
    "c_lakes": lambda orc: (orc.port.fill(fractal_dem(260, 200, 305)), NDV),
    "d_no_flats": lambda orc: case_no_flats(),
    "e_pit": lambda orc: case_pit(),
    "f_edge_flat": lambda orc: case_edge_flat(),
}
DRAINING = ("a_plateau", "b_random", "c_lakes")


def _case(orc, name):
    """(dem, nodata, the model's proportions, its info), computed once and left unchanged"""
    if name not in _CACHE:
        dem, nd = CASES[name](orc)
        dem = np.ascontiguousarray(dem)
        props, info = model.compose(orc, dem, nd)
        for a in (dem, props, info["patched"]):
            a.setflags(write=False)
        _CACHE[name] = (dem, nd, props, info)
    return _CACHE[name]


def _engine(rd, orc, name):
    """the engine's proportions and statistics of a case, once"""
    key = ("engine", name)
    if key not in _CACHE:
        dem, nd, _, _ = _case(orc, name)
        got = rd.fm_tarboton_flats(dem, nd)
        st = rd.dinf_flats_stats()
        got.setflags(write=False)
        _CACHE[key] = (got, st)
    return _CACHE[key]


def _check_props(rd, name, dem, nd, got, st, exp, info):
    print(name, "stats", st, "model", model.stats_of(info), "two receivers", info["two_receivers"], "one receiver", info["one_receiver"])
    assert got.shape == exp.shape and got.dtype == np.float32
    assert np.array_equal(np.sign(got), np.sign(exp)), name                     # the same receivers and markers everywhere
    u = ulp_diff_f32(got, exp)
    print(name, "max ulp", int(u.max()))
    assert (u <= 1).all(), (name, int(u.max()))
    plain = rd.FlowProportions(dem, "Dinf", nodata=nd)
    keep = ~info["patched"]
    assert np.array_equal(_bits(got[keep]), _bits(plain[keep])), name           # unpatched cells: FM_Tarboton's bits
    assert st == model.stats_of(info), name


# ---- proportions and statistics ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_proportions_and_stats(rd, orc, name):
    dem, nd, exp, info = _case(orc, name)
    keep = dem.copy()
    got, st = _engine(rd, orc, name)
    _check_props(rd, name, dem, nd, got, st, exp, info)
    assert np.array_equal(dem, keep)                                             # the DEM is not altered
    patched = info["patched"]
    if name in DRAINING:
        assert st["patched_cells"] > 0 and st["unresolved_cells"] == 0
        assert (got[..., 0][patched] == 0.0).all()                               # every patched cell passes flow on
    if name == "a_plateau":
        assert patched[10:56, 20:111].sum() == 46 * 91 - 3 == st["patched_cells"]   # three cells touch the outlet: low edges
        assert patched[20:40, 63:65].all() and patched[31:33, 30:100].all()      # across the tiles' borders
    if name == "d_no_flats":
        assert st == {"noflow_cells": 0, "patched_cells": 0, "fallback_cells": 0, "unresolved_cells": 0}
        assert np.array_equal(_bits(got), _bits(rd.FlowProportions(dem, "Dinf", nodata=nd)))
    if name == "e_pit":                                                          # no outlet: nothing is patched
        assert st["patched_cells"] == 0 and st["noflow_cells"] == 80
        assert np.array_equal(_bits(got), _bits(rd.FlowProportions(dem, "Dinf", nodata=nd)))
    if name == "f_edge_flat":                                                    # the edge cells are the low edges
        assert st["patched_cells"] == 20 * 69 + 11 * 29 and st["unresolved_cells"] == 0
        assert (got[25:45, 0, 0] == -1.0).all() and (got[35, 1:70, 0] == 0.0).all()   # edge cells never pass flow on


def test_every_path_is_entered(orc):
    """over (a)-(c) together: the fallback, patched cells with two receivers and patched cells with one receiver all occur
    (the wide plateau has no fallback cell, the random integers hardly a two-receiver one: the set covers the three)"""
    tot = {"fallback_cells": 0, "two_receivers": 0, "one_receiver": 0}
    for name in DRAINING:
        info = _case(orc, name)[3]
        for k in tot:
            tot[k] += info[k]
    print(tot)
    assert all(v >= 300 for v in tot.values()), tot


# ---- accumulation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack_below", [None, "0", "4000000000"])
def test_accumulation(rd, orc, monkeypatch, stack_below):
    """fa_tarboton_flats against the oracle's accumulation run on the engine's own proportions: only the summation order
    differs (rtol 1e-12, the existing bound); in every mode of the work list"""
    if stack_below is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, stack_below)
    for name in CASES:
        dem, nd, _, info = _case(orc, name)
        got9, _ = _engine(rd, orc, name)
        exp = orc.port.flow_accumulation(got9)
        got = rd.fa_tarboton_flats(dem, nd)
        assert np.allclose(got, exp, rtol=1e-12, atol=0), (name, float(np.abs(got / exp - 1).max()))
        assert np.array_equal(got == -1, exp == -1) and np.array_equal(got == -1, dem == nd), name
        assert rd.dinf_flats_stats() == model.stats_of(info), name
        if name in DRAINING:
            assert got.max() > 3 * rd.FlowAccumulation(dem, "Dinf", nodata=nd).max(), name
        # the reference-style front door: the same entry (two runs add a cell's donors in the order they arrive)
        assert np.allclose(rd.FlowAccumulation(dem, "Tarboton", nodata=nd, resolve_flats=True), got, rtol=1e-12, atol=0), name


def test_accumulation_with_weights(rd, orc):
    dem, nd, _, _ = _case(orc, "b_random")
    got9, _ = _engine(rd, orc, "b_random")
    w = np.random.default_rng(7).integers(0, 4, dem.shape).astype(np.float64)
    keep = w.copy()
    exp = orc.port.flow_accumulation(got9, w)
    got = rd.fa_tarboton_flats(dem, nd, weights=w)
    assert np.allclose(got, exp, rtol=1e-12, atol=0) and np.array_equal(got == -1, exp == -1)
    assert np.array_equal(w, keep)
    acc = w.copy()
    rd.FlowAccumulation(rd.rdarray(dem, no_data=float(nd)), "Dinf", weights=rd.rdarray(acc, no_data=-1), in_place=True, resolve_flats=True)
    assert np.allclose(acc, got, rtol=1e-12, atol=0)


# ---- `_dev` forms ------------------------------------------------------------------------------------------------
def _torch_dem(dem):
    import torch

    try:
        return torch.from_numpy(np.array(dem, order="C")).cuda()
    except TypeError:                                   # a torch without this unsigned type: the host entry stands alone
        return None


def _dev_equals_host(rd, dem, nd, chan):
    """proportions, statistics, distance, drop and HAND of the `_dev` entries: the host entries' bits"""
    import torch

    t = _torch_dem(dem)
    if t is None:
        return False
    h, w = dem.shape
    p9 = torch.full((h, w, 9), 77.0, dtype=torch.float32, device="cuda")
    rd.fm_tarboton_flats_dev(t, nd, p9)
    st = rd.dinf_flats_stats()
    host9 = rd.fm_tarboton_flats(dem, nd)
    assert st == rd.dinf_flats_stats()
    assert np.array_equal(_bits(p9.cpu().numpy()), _bits(host9))
    wts = np.random.default_rng(11).integers(1, 5, (h, w)).astype(np.float64)
    acc = torch.from_numpy(wts.copy()).cuda()
    rd.fa_tarboton_flats_dev(t, nd, acc)
    torch.cuda.synchronize()
    # the accumulation adds a cell's donors with atomics in the order they arrive, so two runs of the SAME entry may differ
    # in the last bits where a cell has three or more donors with fractional shares: held to the summation-order bound
    dacc, hacc = acc.cpu().numpy(), rd.fa_tarboton_flats(dem, nd, weights=wts)
    assert np.allclose(dacc, hacc, rtol=1e-12, atol=0) and np.array_equal(dacc == -1, hacc == -1)
    tc = torch.from_numpy(chan).cuda()
    dist = torch.full((h, w), 77.0, dtype=torch.float64, device="cuda")
    drop = torch.full((h, w), 77.0, dtype=torch.float64, device="cuda")
    rd.dinf_distance_down_flats_dev(t, nd, tc, "ave", False, (2.0, 3.0), -7.0, dist=dist, drop=drop)
    host = rd.dinf_distance_down_flats(dem, nd, chan, "ave", False, (2.0, 3.0), -7.0, want=("dist", "drop"))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(host["dist"])) and np.array_equal(_bits(drop.cpu().numpy()), _bits(host["drop"]))
    out = torch.full((h, w), 77.0, dtype=torch.float64, device="cuda")
    rd.dinf_hand_flats_dev(t, nd, tc, out, "min", True, -7.0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(rd.dinf_hand_flats(dem, nd, chan, "min", True, -7.0)))
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(dem))                    # inputs are never written
    return True


@pytest.mark.parametrize("name", ["a_plateau", "b_random", "e_pit"])
def test_dev_forms_equal_host_forms(rd, orc, name):
    dem, nd, _, _ = _case(orc, name)
    chan = (rd.fa_tarboton_flats(dem, nd) >= 40).astype(np.uint8)
    assert _dev_equals_host(rd, dem, nd, chan)


def test_dev_form_on_a_side_stream(rd, orc):
    import torch

    dem, nd, _, info = _case(orc, "b_random")
    host9, _ = _engine(rd, orc, "b_random")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(dem.copy()).cuda()
        p9 = torch.empty(dem.shape + (9,), dtype=torch.float32, device="cuda")
        rd.fm_tarboton_flats_dev(t, nd, p9)
        after = p9 + 0.0
    assert rd.dinf_flats_stats() == model.stats_of(info)                         # waits for the call's stream
    torch.cuda.synchronize()
    assert np.array_equal(_bits(after.cpu().numpy()), _bits(host9))


# ---- distance and HAND -------------------------------------------------------------------------------------------
def _reaches(props, chan):
    """cells from which some path of positive shares leads to a cell of chan (interior donors only, as the engine's graph)"""
    reach = chan.astype(bool).copy()
    give = props[..., 1:] > 0
    give[0, :] = give[-1, :] = give[:, 0] = give[:, -1] = False
    while True:
        new = reach.copy()
        for n in range(1, 9):
            nb = np.zeros_like(reach)
            ys = slice(max(0, -model.DY[n]), reach.shape[0] - max(0, model.DY[n]))
            xs = slice(max(0, -model.DX[n]), reach.shape[1] - max(0, model.DX[n]))
            yd = slice(max(0, model.DY[n]), reach.shape[0] - max(0, -model.DY[n]))
            xd = slice(max(0, model.DX[n]), reach.shape[1] - max(0, -model.DX[n]))
            nb[ys, xs] = reach[yd, xd]                                           # nb[c] = reach[neighbour n of c]
            new |= give[..., n - 1] & nb
        if np.array_equal(new, reach):
            return reach
        reach = new


@pytest.mark.parametrize("name", DRAINING)
def test_distance_and_hand(rd, orc, monkeypatch, name):
    """dinf_distance_down_flats against the distance model run on the engine's own proportions: bit for bit, as the plain
    D-infinity route; every cell of a drainable flat with a channel downstream gets a distance"""
    monkeypatch.delenv("RDGPU_MFD_DISTANCE_STACK_BELOW", raising=False)
    dem, nd, _, info = _case(orc, name)
    got9, _ = _engine(rd, orc, name)
    acc = orc.port.flow_accumulation(got9)
    chan = (acc >= 40).astype(np.uint8)
    assert chan.sum() > 0
    elev = dem.astype(np.float64)
    for ch, stat, strict in ((None, "ave", True), (chan, "ave", True), (chan, "min", False), (chan, "max", True)):
        exp = dist_model.distance_down(got9, ch, elev, stat, strict, cell=(2.0, 3.0), out_nodata=-7.0)
        got = rd.dinf_distance_down_flats(dem, nd, ch, stat, strict, (2.0, 3.0), -7.0, want=("dist", "drop"))
        for k in ("dist", "drop"):
            bad = got[k].view(np.uint64) != exp[k].view(np.uint64)
            print(name, stat, strict, k, "cells differing:", int(bad.sum()))
            assert not bad.any(), (name, stat, strict, k, np.argwhere(bad)[:5].tolist())
    assert rd.dinf_flats_stats() == model.stats_of(info)
    patched = info["patched"]
    lenient = rd.dinf_distance_down_flats(dem, nd, chan, "ave", False, (1.0, 1.0), -1.0)["dist"]
    down = _reaches(got9, chan) & patched & (chan == 0)
    print(name, "patched cells off the channels with a channel downstream:", int(down.sum()), "of", int(patched.sum()))
    assert down.sum() >= 500, name
    assert (lenient[down] > 0).all() and np.isfinite(lenient[down]).all(), name
    plain = rd.dinf_distance_down(dem, nd, chan, "ave", False, (1.0, 1.0), -1.0)["dist"]
    assert (plain[down] == -1.0).all(), name                       # the plain route dams every one of them
    hand = rd.dinf_hand_flats(dem, nd, chan, "ave", False, -7.0)
    assert np.array_equal(_bits(hand), _bits(rd.dinf_distance_down_flats(dem, nd, chan, "ave", False, (1.0, 1.0), -7.0, want=("drop",))["drop"]))
    assert (hand[down] >= 0).all(), name                                         # a filled surface never rises downstream


# ---- element types, shapes, size ---------------------------------------------------------------------------------
TYPES = [("u8", np.uint8, 255), ("i8", np.int8, -128), ("u16", np.uint16, 65535), ("i16", np.int16, -32768),
         ("u32", np.uint32, 4000000000), ("i32", np.int32, -9999), ("f32", np.float32, -9999.0), ("f64", np.float64, -9999.0)]


@pytest.mark.parametrize("suffix,dtype,nodata", TYPES, ids=[t[0] for t in TYPES])
def test_element_types(rd, orc, suffix, dtype, nodata):
    z = model.random_integer_dem(orc, 20 + len(suffix), 70, 40).astype(dtype)    # levels 0..11 fit every type
    z[10:13, 30:36] = nodata
    nd = z.dtype.type(nodata)
    exp, info = model.compose(orc, z, nd)
    assert info["patched_cells"] > 100 and info["fallback_cells"] > 0
    got = rd.fm_tarboton_flats(z, nd)
    _check_props(rd, suffix, z, nd, got, rd.dinf_flats_stats(), exp, info)
    acc = rd.fa_tarboton_flats(z, nd)
    ref = orc.port.flow_accumulation(got)
    assert np.allclose(acc, ref, rtol=1e-12, atol=0) and np.array_equal(acc == -1, z == nd)
    chan = (acc >= 25).astype(np.uint8)
    assert _dev_equals_host(rd, z, nd, chan) or suffix in ("u16", "u32")


SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3)]     # (height, width)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_small_shapes(rd, orc, shape):
    for z in (np.full(shape, 5, np.float32), np.random.default_rng(3).integers(0, 3, shape).astype(np.float32)):
        exp, info = model.compose(orc, z, NDV)
        got = rd.fm_tarboton_flats(z, NDV)
        _check_props(rd, str(shape), z, NDV, got, rd.dinf_flats_stats(), exp, info)
        assert np.array_equal(rd.fa_tarboton_flats(z, NDV), orc.port.flow_accumulation(got))
        assert (rd.dinf_distance_down_flats(z, NDV)["dist"] == 0.0).all() or shape == (3, 3)


def test_large_filled_fractal(rd, orc):
    """(i) 1000 x 800: 16 x 25 tiles, lakes of every size, tiles without a flat cell beside tiles full of them"""
    dem = orc.port.fill(fractal_dem(1000, 800, 7))
    exp, info = model.compose(orc, dem, NDV)
    got = rd.fm_tarboton_flats(dem, NDV)
    st = rd.dinf_flats_stats()
    _check_props(rd, "1000x800", dem, NDV, got, st, exp, info)
    assert st["patched_cells"] > 50000 and st["fallback_cells"] > 0 and st["unresolved_cells"] == 0
    acc = rd.fa_tarboton_flats(dem, NDV)
    ref = orc.port.flow_accumulation(got)
    assert np.allclose(acc, ref, rtol=1e-12, atol=0)
    edge = np.ones(dem.shape, bool)
    edge[1:-1, 1:-1] = False
    # every cell drains to the raster's edge: a cell's two float32 shares sum to 1 within 2^-24, a path is shorter than
    # 1800 cells, so what arrives is the cell count within 1800 * 2^-24 = 1.1e-4
    assert acc[edge].sum() == pytest.approx(dem.size, rel=1.1e-4)


# ---- the plain entries share the workspace -----------------------------------------------------------------------
def test_plain_entries_are_unchanged_by_a_flats_call(rd, orc):
    dem, nd, _, _ = _case(orc, "b_random")
    chan = (rd.FlowAccumulation(dem, "Dinf", nodata=nd) >= 5).astype(np.uint8)

    def plain():
        return (rd.FlowAccumulation(dem, "Dinf", nodata=nd), rd.FlowProportions(dem, "Dinf", nodata=nd),
                rd.dinf_distance_down(dem, nd, chan, "ave", False, want=("dist", "drop")))

    a0, p0, d0 = plain()
    rd.fa_tarboton_flats(dem, nd)
    rd.dinf_distance_down_flats(dem, nd, chan, want=("dist", "drop"))
    rd.fm_tarboton_flats(dem, nd)
    a1, p1, d1 = plain()
    assert np.array_equal(_bits(a0), _bits(a1)) and np.array_equal(_bits(p0), _bits(p1))
    assert all(np.array_equal(_bits(d0[k]), _bits(d1[k])) for k in ("dist", "drop"))
    assert not np.array_equal(p0, rd.fm_tarboton_flats(dem, nd))


# ---- refused calls -----------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(rd):
    L = rd.lib()
    h, w = 6, 7
    dem = np.ones((h, w), np.float32)
    p9 = np.full((h, w, 9), 77.0, np.float32)
    acc = np.full((h, w), 77.0)
    dist = np.full((h, w), 77.0)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    F, D = ctypes.c_float, ctypes.c_double

    def fm(z=dem, ww=w, hh=h, out=p9):
        return L.rdgpu_fm_tarboton_flats_f32(P(z), F(-9999), ww, hh, P(out))

    def fa(z=dem, ww=w, hh=h, out=acc):
        return L.rdgpu_fa_tarboton_flats_f32(P(z), F(-9999), ww, hh, P(out))

    def dd(z=dem, ww=w, hh=h, out=dist, stat=0):
        return L.rdgpu_dinf_distance_down_flats_f32(P(z), F(-9999), ww, hh, None, stat, 1, D(1.0), D(1.0), P(out), None, D(-1.0))

    def fm_dev(z=dem, ww=w, hh=h, out=p9):
        return L.rdgpu_fm_tarboton_flats_dev_f32(P(z), F(-9999), ww, hh, P(out), None)

    def fa_dev(z=dem, ww=w, hh=h, out=acc):
        return L.rdgpu_fa_tarboton_flats_dev_f32(P(z), F(-9999), ww, hh, P(out), None)

    # refused before any device work: the host arrays handed to the _dev forms are never touched
    bad = [dict(z=None), dict(out=None), dict(ww=0), dict(hh=0), dict(ww=-3), dict(hh=-1), dict(ww=65536, hh=32768),
           dict(ww=46341, hh=46341)]                    # 2^31 and 2 147 488 281 cells: above 0x7FFF0000, below the plain limit
    for kw in bad:
        for fn in (fm, fa, dd, fm_dev, fa_dev):
            rc = fn(**kw)
            assert rc == 2, (fn.__name__, kw, rc)                                # RDGPU_ERR_ARG
            assert b"rdgpu_" in L.rdgpu_last_error()
    assert dd(stat=3) == 2
    assert (p9 == 77.0).all() and (acc == 77.0).all() and (dist == 77.0).all()
    assert L.rdgpu_dinf_flats_get_stats(None) == 2
    assert fm() == 0 and (p9[1:-1, 1:-1, 0] == 0.0).all() and (p9[0, :, 0] == -1.0).all()   # (the same call, valid: a level
    # raster is one flat whose low edges are the raster's edge cells)
    for method in ("D8", "D4", "Quinn", "Holmgren", "Freeman", "OCallaghanD8"):
        for call in (lambda: rd.FlowAccumulation(dem, method, exponent=2.0, resolve_flats=True),
                     lambda: rd.FlowProportions(dem, method, exponent=2.0, resolve_flats=True),
                     lambda: rd.FlowAccumulation(rd.rdarray(dem, no_data=-9999), method, exponent=2.0, resolve_flats=True),
                     lambda: rd.FlowProportions(rd.rdarray(dem, no_data=-9999), method, exponent=2.0, resolve_flats=True)):
            with pytest.raises(rd.RdgpuError, match=method):
                call()
    for call in (lambda: rd.fm_tarboton_flats(dem.astype(np.int64), -9999),
                 lambda: rd.fa_tarboton_flats(dem, -9999, weights=np.ones((3, 3))),
                 lambda: rd.dinf_distance_down_flats(dem, -9999, stat="median"),
                 lambda: rd.dinf_distance_down_flats(dem, -9999, want=())):
        with pytest.raises(rd.RdgpuError):
            call()
    assert np.array_equal(rd.FlowProportions(dem, "Dinf", resolve_flats=False), rd.FlowProportions(dem, "Dinf"))


def test_every_new_symbol_is_exported(rd):
    for s in ("u8", "i8", "u16", "i16", "u32", "i32", "f32", "f64"):
        for stem in ("rdgpu_fm_tarboton_flats_", "rdgpu_fm_tarboton_flats_dev_", "rdgpu_fa_tarboton_flats_",
                     "rdgpu_fa_tarboton_flats_dev_", "rdgpu_dinf_distance_down_flats_", "rdgpu_dinf_distance_down_flats_dev_"):
            assert hasattr(rd.lib(), stem + s), stem + s
    assert hasattr(rd.lib(), "rdgpu_dinf_flats_get_stats")
    for n in ("fm_tarboton_flats", "fa_tarboton_flats", "dinf_distance_down_flats", "dinf_hand_flats", "fm_tarboton_flats_dev",
              "fa_tarboton_flats_dev", "dinf_distance_down_flats_dev", "dinf_hand_flats_dev", "dinf_flats_stats"):
        assert callable(getattr(rd, n)) and n in rd.__all__, n
