"""Terrain attributes on the engine (csrc/terrain.hip) against the COMPILED REFERENCE's outputs (tests/golden/ref_terrain.npz)
through every entry point -- the host C-ABI via api, `_dev` with torch tensors, the fused multi-output launch -- and against
the numpy model (tests/terrain_model.py, itself pinned to the reference) on fresh seeded shapes that straddle tile edges.
rise/run, percentage and the three curvatures: bit equality.  atan / atan2 / log attributes: at most 1 float32 ULP.
No cell is left out; a NaN (the NaN-NoData case) must be a NaN on both sides."""
import json
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from digest import load_golden  # noqa: E402
import terrain_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu

G = load_golden(os.path.join(GOLDEN, "ref_terrain.npz"))
CASES = sorted({k.split("/")[0] for k in G})
HIST = {}


def _check(name, attrib, got, exp):
    assert got.dtype == np.float32 and got.shape == exp.shape
    if attrib in tm.ALGEBRAIC:
        assert tm.same_bits(got, exp), (name, attrib, int((got.view(np.int32) != exp.view(np.int32)).sum()))
    else:
        u = tm.ulps32(got, exp)
        h = HIST.setdefault(attrib, [0, 0, 0])
        for i in range(3):
            h[i] += int((u == i).sum()) if i < 2 else int((u >= 2).sum())
        assert u.max() <= 1, (name, attrib, int(u.max()), int((u > 1).sum()))


def _torch_dem(dem):
    import torch

    if dem.dtype in (np.uint16, np.uint32, np.uint64):
        signed = torch.from_numpy(dem.view({2: np.int16, 4: np.int32, 8: np.int64}[dem.dtype.itemsize]).copy()).cuda()
        return signed.view(getattr(torch, dem.dtype.name))
    return torch.from_numpy(dem.copy()).cuda()


@pytest.mark.parametrize("case", CASES)
def test_every_entry_point_equals_the_reference(rd, case):
    import torch

    dem, nodata = G[case + "/dem"], G[case + "/nodata"][0]
    nodata = float(nodata) if dem.dtype.kind == "f" else int(nodata)
    zscale, cx, cy, out_nd = (float(v) for v in G[case + "/params"])
    keep = dem.copy()
    fused = rd.terrain_attributes(dem, tm.ATTRIBS, nodata, zscale, (cx, cy), out_nd)          # host, ONE launch
    t = _torch_dem(dem)
    t_keep = t.clone()
    outs = {a: torch.empty(dem.shape, dtype=torch.float32, device="cuda") for a in tm.ATTRIBS}
    rd.terrain_attributes_dev(t, tm.ATTRIBS, nodata, outs, zscale, (cx, cy), out_nd)          # device, ONE launch
    some = ("slope_riserun", "aspect", "curvature")
    outs3 = {a: torch.empty(dem.shape, dtype=torch.float32, device="cuda") for a in some}
    rd.terrain_attributes_dev(t, some, nodata, outs3, zscale, (cx, cy), out_nd)
    for a in tm.ATTRIBS:
        exp = G[case + "/" + a]
        one = rd.terrain_attribute(dem, a, nodata, zscale, (cx, cy), out_nd)                 # host, single
        _check(case, a, one, exp)
        o = torch.empty(dem.shape, dtype=torch.float32, device="cuda")
        rd.terrain_attribute_dev(t, a, nodata, o, zscale, (cx, cy), out_nd)                   # device, single
        torch.cuda.synchronize()
        # the fused outputs equal the single-attribute outputs bit for bit, on every path
        for name, other in (("dev", o.cpu().numpy()), ("fused host", fused[a]), ("fused dev", outs[a].cpu().numpy())):
            assert tm.same_bits(other, one), (case, a, name)
        if a in some:
            assert tm.same_bits(outs3[a].cpu().numpy(), one), (case, a, "fused subset")
    assert np.array_equal(dem.view(np.uint8), keep.view(np.uint8)) and torch.equal(t.view(torch.uint8), t_keep.view(torch.uint8))
    # SPI / CTI of the stored accumulation (with NoData cells) and the reference's rise/run slope
    acc, slope = G[case + "/acc"], G[case + "/slope_riserun"]
    for which, host, dev in (("spi", rd.terrain_spi, rd.terrain_spi_dev), ("cti", rd.terrain_cti, rd.terrain_cti_dev)):
        got = host(acc, slope, float(G[case + "/acc_nodata"]), out_nd, (cx, cy))
        _check(case, which, got, G[case + "/" + which])
        o = torch.empty(dem.shape, dtype=torch.float32, device="cuda")
        dev(torch.from_numpy(acc).cuda(), torch.from_numpy(slope).cuda(), o, float(G[case + "/acc_nodata"]), out_nd, (cx, cy))
        torch.cuda.synchronize()
        assert tm.same_bits(o.cpu().numpy(), got), (case, which)
        assert (got[acc == -1.0] == -1.0).all() and (got[slope == np.float32(out_nd)] == -1.0).all()


def test_shapes_that_straddle_tile_edges_equal_the_model(rd):
    """tiles are 64 x 32: widths and heights of 1..3 tiles +- 1, fresh random float32 / int16 / float64 DEMs with holes"""
    rng = np.random.default_rng(2024)
    widths = sorted({t * 64 + d for t in (1, 2, 3) for d in (-1, 0, 1)} | {1, 2, 3})
    heights = sorted({t * 32 + d for t in (1, 2, 3) for d in (-1, 0, 1)} | {1, 2})
    n = 0
    for w in widths:
        for h in (heights if w in (1, 63, 64, 65, 193) else (31, 33, 65)):
            dt = (np.float32, np.int16, np.float64)[n % 3]
            dem = (rng.normal(0, 300, (h, w))).astype(dt)
            dem[rng.random((h, w)) < 0.03] = dt(-9999)
            zs, cell = ((1.0, (1.0, 1.0)), (2.5, (3.0, 7.0)))[n % 2]
            got = rd.terrain_attributes(dem, tm.ATTRIBS, -9999, zs, cell, -1234.5)
            for a in tm.ATTRIBS:
                _check(f"{w}x{h}", a, got[a], tm.terrain_attribute(dem, a, -9999, zs, cell, -1234.5))
            n += 1
    assert n >= 40


def test_dev_on_a_non_default_stream(rd):
    import torch

    from richdem_amd.synth import fractal_dem

    dem = fractal_dem(700, 300, 5)
    exp = {a: tm.terrain_attribute(dem, a, -9999.0) for a in tm.ATTRIBS}
    t = torch.from_numpy(dem).cuda()
    outs = {a: torch.empty((300, 700), dtype=torch.float32, device="cuda") for a in tm.ATTRIBS}
    single = torch.empty((300, 700), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rd.terrain_attributes_dev(t, tm.ATTRIBS, -9999.0, outs)
        rd.terrain_attribute_dev(t, "profile_curvature", -9999.0, single)
    s.synchronize()
    for a in tm.ATTRIBS:
        _check("stream", a, outs[a].cpu().numpy(), exp[a])
    assert tm.same_bits(single.cpu().numpy(), outs["profile_curvature"].cpu().numpy())
    assert torch.equal(t.cpu(), torch.from_numpy(dem))


def test_rdarray_supplies_nodata_and_cell_lengths(rd):
    from richdem_amd.synth import fractal_dem

    dem = fractal_dem(90, 70, 6).copy()
    dem[3, 4] = -5.0
    r = rd.rdarray(dem, no_data=-5.0, geotransform=(0.0, 30.0, 0.0, 0.0, 0.0, -10.0))
    got = rd.terrain_attribute(r, "slope_degrees")
    _check("rdarray", "slope_degrees", got, tm.terrain_attribute(dem, "slope_degrees", -5.0, 1.0, (30.0, 10.0)))
    assert got[3, 4] == -9999.0


def test_zz_record_the_ulp_histograms():
    """(runs last in this file) the measured float32-ULP histograms of the transcendental attributes over every cell compared
    above: [0 ULP, 1 ULP, more]"""
    assert HIST and all(h[2] == 0 for h in HIST.values()), HIST
    records = os.environ.get("RDGPU_TEST_RECORDS") or os.path.join(ROOT, "build", "test_records")   # (build/ is not tracked)
    os.makedirs(records, exist_ok=True)
    with open(os.path.join(records, "terrain_ulps.json"), "w") as f:
        json.dump(HIST, f, indent=1)
    warnings.warn("terrain attributes, float32 ULPs [0, 1, >1] per attribute: " + json.dumps(HIST), UserWarning)
