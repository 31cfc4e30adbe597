"""Terrain attributes at FULL size inside the suite: the 40000 x 40000 bench DEM G(seed=3) is generated on the device (its band
digests prove it is the raster the reference saw), ONE fused launch computes rise/run, percentage and the three curvatures,
and every one of the 1.6e9 cells of each plane enters a band digest (tests/golden/digest.py) that must equal the compiled
reference's (tests/golden/ref_s3_terrain_digests.npz, make_golden_terrain.py --s3): bit equality, no tolerance.
HBM: 6.4 GB in + 6.4 GB per output."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from digest import band_digests_torch, load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
FIVE = ("slope_riserun", "slope_percentage", "curvature", "planform_curvature", "profile_curvature")


def test_s3_five_algebraic_attributes_equal_the_reference_bit_for_bit(rd):
    import torch

    path = os.path.join(GOLDEN, "ref_s3_terrain_digests.npz")
    assert os.path.exists(path), "tests/golden/ref_s3_terrain_digests.npz missing (make_golden_terrain.py --s3)"
    g = load_golden(path)
    n, rows = int(g["size"]), int(g["band_rows"])
    assert n == 40000 and g["slope_riserun"].size == 40
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=int(g["seed"]))
    assert np.array_equal(band_digests_torch(Z, rows), g["dem"]), "the device-generated DEM is not the reference's input"
    outs = {a: torch.empty((n, n), dtype=torch.float32, device="cuda") for a in FIVE}
    try:
        rd.terrain_attributes_dev(Z, FIVE, -9999.0, outs)                 # ONE launch, one read of the DEM
        torch.cuda.synchronize()
        assert np.array_equal(band_digests_torch(Z, rows), g["dem"])      # input unmodified
        for a in FIVE:
            bad = np.flatnonzero(band_digests_torch(outs[a], rows) != g[a])
            assert bad.size == 0, f"{a}: {bad.size} of {g[a].size} bands differ from the reference, first {bad[:8].tolist()}"
    finally:
        del outs, Z
        rd.release_workspace()
        torch.cuda.empty_cache()


def _ulps32(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2**31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2**31) - ib, ib)
    return np.abs(ia - ib)


def test_s2_transcendental_attributes_within_one_ulp_of_the_reference(rd):
    """10000 x 10000 G(seed=3): slope_degrees, slope_radians, aspect and SPI (of the engine's own fill -> flat-resolved
    directions -> d8_flow_accum, whose band digests must equal the reference's accumulation) at a fixed sample of 262 144
    cells against the compiled reference (tests/golden/ref_s2_terrain.npz): at most 1 float32 ULP; the histogram and the
    number of bit-equal bands go to s2_terrain.json in $RDGPU_TEST_RECORDS (default build/test_records)."""
    import json
    import warnings

    import torch

    from conftest import ROOT

    path = os.path.join(GOLDEN, "ref_s2_terrain.npz")
    assert os.path.exists(path), "tests/golden/ref_s2_terrain.npz missing (make_golden_terrain.py --s2)"
    g = load_golden(path)
    n, rows = int(g["size"]), int(g["band_rows"])
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=int(g["seed"]))
    assert np.array_equal(band_digests_torch(Z, rows), g["dem"])
    k, stride = int(g["sample_k"]), int(g["sample_stride"])
    pos = (torch.arange(k, dtype=torch.int64, device="cuda") * stride) % (n * n)
    report = {}
    out = torch.empty((n, n), dtype=torch.float32, device="cuda")

    def compare(name):
        u = _ulps32(out.reshape(-1)[pos].cpu().numpy(), g[name + "_sample"])
        bands = band_digests_torch(out, rows)
        report[name] = {"sample_cells": k, "ulp_histogram": {str(i): int((u == i).sum()) for i in range(3)},
                        "max_ulp": int(u.max()), "bands_bitwise_equal": int((bands == g[name + "_bands"]).sum()),
                        "bands": int(bands.size)}
        return int(u.max())

    worst = 0
    for a in ("slope_degrees", "slope_radians", "aspect"):
        rd.terrain_attribute_dev(Z, a, -9999.0, out)
        torch.cuda.synchronize()
        worst = max(worst, compare(a))
    slope = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.terrain_attribute_dev(Z, "slope_riserun", -9999.0, slope)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    acc = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, acc)
    torch.cuda.synchronize()
    assert np.array_equal(band_digests_torch(acc, rows), g["acc_bands"]), "the accumulation is not the reference's"
    rd.terrain_spi_dev(acc, slope, out, -1.0, -9999.0)
    torch.cuda.synchronize()
    worst = max(worst, compare("spi"))
    records = os.environ.get("RDGPU_TEST_RECORDS") or os.path.join(ROOT, "build", "test_records")
    os.makedirs(records, exist_ok=True)
    with open(os.path.join(records, "s2_terrain.json"), "w") as f:
        json.dump(report, f, indent=1)
    warnings.warn("terrain attributes at 10000^2 vs the compiled reference: " + json.dumps(report), UserWarning)
    del Z, out, slope, dirs, acc
    rd.release_workspace()
    torch.cuda.empty_cache()
    assert worst <= 1, report
