"""rdgpu_fill_spill_merge_<T> on hierarchies with a caller-given ocean, on the GPU: the golden cases of
tests/golden/ref_dephier_ocean.npz (quantile sea, one ocean cell, ring and hole; four waters each) through both doors of
both entries -- the hierarchy from rdgpu_depression_hierarchy_ocean_<T>, then Fill-Spill-Merge -- against the model
(tests/fsm_model.py on tests/dephier_ocean_model.py) and the COMPILED REFERENCE's wtd.

The waters are multiples of 2^-10 and the f32 elevations dyadic, so every gather and prefix sum is exact in any order:
node_water and the lake counts equal the model's exactly, and a depth may differ from the model's -- which equals the
reference's wtd bit for bit -- by the rounding of one division and one subtraction."""
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
import fsm_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden(os.path.join(GOLDEN, "ref_dephier_ocean.npz"))


FSM_CASES = [str(c) for c in _golden()["fsm_cases"]]


@functools.lru_cache(maxsize=None)
def _hier(case):
    G = _golden()
    return om.hierarchy(om.golden_case_dem(G, case), 8, G[case + "/mask"])


def check(dem, mask, water, wtd, r, depth, nw, res):
    cells, win = dem.size, r["water_in"]
    assert (int(res["lakes"]), int(res["full_lakes"])) == (r["lakes"], r["full_lakes"])
    assert np.array_equal(nw, r["node_water"]) and float(res["water_in"]) == win
    lvl = np.where(np.isfinite(r["cell_level"]), np.abs(r["cell_level"]), 0.0)
    tol = 4.0 * np.spacing(lvl) * np.isfinite(r["cell_level"])            # one division and one subtraction: 4 ulp of the level
    for ref in (r["depth"], wtd):
        assert (np.abs(depth - ref) <= tol).all()
    assert (depth[mask != 0] == 0).all()                                   # depth is 0 on the ocean cells
    bound = cells * 2.0 ** -52 * win                                       # the header's bound
    assert abs(float(res["ocean"]) - r["ocean"]) <= bound and abs(float(res["standing"]) - r["standing"]) <= bound
    assert abs(win - (float(res["standing"]) + float(res["ocean"]))) <= bound
    assert abs(float(res["standing"]) - float(depth.sum())) <= bound


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("case", FSM_CASES)
def test_golden_cases_through_both_doors(rd, case, k):
    import torch

    G = _golden()
    dem, mask = np.ascontiguousarray(om.golden_case_dem(G, case)), G[case + "/mask"]
    water, wtd = G[f"{case}/w{k}/water"], G[f"{case}/w{k}/wtd"]
    labels, tab = _hier(case)
    r = fm.fill_spill_merge(dem, labels, tab, water)
    assert np.array_equal(r["depth"], wtd)                                 # (what the recipe asserted)
    # the host door, on the engine's own masked hierarchy
    glab, gtab = rd.depression_hierarchy(dem, 8, ocean=mask)
    assert np.array_equal(glab, labels) and len(gtab) == len(tab)
    depth, res = rd.fill_spill_merge(dem, glab, gtab, water)
    check(dem, mask, water, wtd, r, depth, res["node_water"], res)
    # the device door: the hierarchy and the water stay in HBM
    d, o = torch.from_numpy(dem.copy()).cuda(), torch.from_numpy(mask.copy()).cuda()
    dlab = torch.empty(dem.shape, dtype=torch.int32, device="cuda")
    dtab = torch.zeros(len(tab) * rd.DEPHIER_NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    counts = rd.depression_hierarchy_dev(d, dlab, dtab, 8, ocean=o)
    n = int(counts.cpu()[0])
    assert n == len(tab)
    wat = torch.from_numpy(water.copy()).cuda()
    dep = torch.full(dem.shape, -7.0, dtype=torch.float64, device="cuda")
    nw = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    out = rd.fill_spill_merge_dev(d, dlab, dtab, n, wat, dep, nw)
    torch.cuda.synchronize()
    res = out.cpu().numpy().view(rd.FSM_RESULT_DTYPE)[0]
    check(dem, mask, water, wtd, r, dep.cpu().numpy(), nw.cpu().numpy(), {k2: res[k2] for k2 in res.dtype.names})


def test_water_on_ocean_cells_goes_to_the_ocean(rd):
    G = _golden()
    case = "perm_i32_65x129/ringhole"
    dem, mask = np.ascontiguousarray(om.golden_case_dem(G, case)), G[case + "/mask"]
    labels, tab = rd.depression_hierarchy(dem, 8, ocean=mask)
    water = np.where(mask != 0, 0.25, 0.0)                                  # water on the ocean cells alone
    depth, res = rd.fill_spill_merge(dem, labels, tab, water)
    assert not depth.any() and res["ocean"] == res["water_in"] == 0.25 * int(np.count_nonzero(mask)) and res["standing"] == 0
    both = np.full(dem.shape, 0.5)                                          # and on every cell
    depth, res = rd.fill_spill_merge(dem, labels, tab, both)
    r = fm.fill_spill_merge(dem, *_hier(case), both)
    assert (depth[mask != 0] == 0).all() and (depth[mask == 0] > 0).any()
    bound = dem.size * 2.0 ** -52 * res["water_in"]
    assert res["ocean"] >= 0.5 * int(np.count_nonzero(mask)) - bound
    assert abs(res["water_in"] - (res["standing"] + res["ocean"])) <= bound and abs(res["ocean"] - r["ocean"]) <= bound
