"""d8_upslope_cells at 10000 x 10000 G(seed=3) against the COMPILED REFERENCE (tests/golden/ref_s2_upslope.npz,
make_golden_upslope.py --s2): the engine's own fill -> flat resolution produces the directions (their band digests must equal
the reference's), then the upslope rasters of the cell with the largest accumulation and of one long shallow line must
equal the reference's in every band digest -- every one of the 1e8 cells enters a digest -- and in the count of 1-cells."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from digest import band_digests_torch, load_golden  # noqa: E402

pytestmark = pytest.mark.gpu


def _bands(name, got, exp):
    bad = np.flatnonzero(got != exp)
    print(name, "bands differing:", bad.size, "of", exp.size)
    assert bad.size == 0, f"{name}: {bad.size} of {exp.size} bands differ from the reference, first bands {bad[:8].tolist()}"


def test_s2_upslope_cells_equal_the_reference(rd):
    import torch

    g = load_golden(os.path.join(GOLDEN, "ref_s2_upslope.npz"))
    n, seed, rows = int(g["size"]), int(g["seed"]), int(g["band_rows"])
    assert n == 10000
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=seed)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    torch.cuda.synchronize()
    del Z
    _bands("directions", band_digests_torch(dirs, rows), g["dirs"])
    keep = dirs.clone()
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, area)
    torch.cuda.synchronize()
    mx, my = (int(v) for v in g["mouth"])
    assert float(area[my, mx].item()) == float(g["mouth_accum"]) == float(area.max().item())
    del area
    up = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    for tag, ln in (("mouth", (mx, my, mx, my)), ("line", tuple(int(v) for v in g["line"]))):
        up.fill_(77)
        rd.d8_upslope_cells_dev(dirs, *ln, up)
        torch.cuda.synchronize()
        _bands("upslope cells, " + tag, band_digests_torch(up, rows), g["up_" + tag])
        ones, twos = int((up == 1).sum().item()), int((up == 2).sum().item())
        print(tag, "ones", ones, "twos", twos, "reference seconds", float(g["ref_seconds/" + tag]))
        assert ones == int(g["ones_" + tag]) and twos == int(g["twos_" + tag])
        assert ones + twos + int((up == 255).sum().item()) == n * n
    assert int(g["ones_mouth"]) + 1 == int(g["mouth_accum"])               # what drains through the mouth IS its accumulation
    assert torch.equal(dirs, keep)
    del up, dirs, keep
    rd.release_workspace()
    torch.cuda.empty_cache()
