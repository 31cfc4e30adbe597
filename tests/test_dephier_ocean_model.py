"""The model of the depression hierarchy with a caller-given ocean and of BucketFillFromEdges
(tests/dephier_ocean_model.py) against the COMPILED REFERENCE (tests/golden/ref_dephier_ocean.npz,
make_golden_dephier_ocean.py): GetDepressionHierarchy on a label raster with the mask's cells OCEAN, in the canonical form
of test_dephier_model.py; FillSpillMerge on those hierarchies, bit for bit; BucketFillFromEdges, exactly.  And on rasters
worked by hand.  No GPU."""
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
import fsm_model as fm  # noqa: E402

G = load_golden(os.path.join(GOLDEN, "ref_dephier_ocean.npz"))
CASES = [str(c) for c in G["cases"]]
FSM_CASES = [str(c) for c in G["fsm_cases"]]
RASTERS = sorted({c.split("/")[0] for c in CASES})
NONE = dm.NONE
NO_DEP = 0xFFFFFFFF
KINDS = ("ring", "quantile", "bucket", "onecell", "ringhole", "scatter", "nodata")


def case_dem(case):
    return om.golden_case_dem(G, case)


def _ref(case, t):
    label, u, f = G[f"{case}/t{t}/labels"], G[f"{case}/t{t}/u32"], G[f"{case}/t{t}/f64"]

    def shift(a):
        a = a.astype(np.int64)
        return np.where(a == NO_DEP, NONE, a - 1)

    ocean_parent = (u[1:, 6] & 1).astype(bool)
    return {"labels": label.astype(np.int64) - 1, "parent": np.where(ocean_parent, NONE, shift(u[1:, 0])),
            "lchild": shift(u[1:, 1]), "rchild": shift(u[1:, 2]), "pit_cell": u[1:, 3].astype(np.int64), "level": f[1:, 0],
            "cells": (u[1:, 6] >> 1).astype(np.int64), "volume": f[1:, 2]}


def test_the_cases_are_the_ones_asked_for():
    assert {c.split("/")[1] for c in CASES} == set(KINDS) and len(CASES) == len(KINDS) * len(RASTERS)
    assert {G[r + "/dem"].dtype for r in RASTERS} == {np.dtype(np.uint16), np.dtype(np.int32), np.dtype(np.float32)}
    assert set(FSM_CASES) == {f"{r}/{k}" for r in ("perm_i32_65x129", "frac_f32_200x130") for k in ("quantile", "onecell", "ringhole")}
    for c in CASES:
        mask, dem = G[c + "/mask"], case_dem(c)
        assert mask.shape == dem.shape and mask.any() and not mask.all()
        land = dem[mask == 0]
        assert np.unique(land).size == land.size, c           # tie-free land
    ring = om.ring_mask(G["frac_f32_65x129/dem"].shape).astype(bool)
    assert not G["frac_f32_65x129/onecell/mask"][ring].any() and G["frac_f32_65x129/onecell/mask"].sum() == 1
    assert not G["frac_f32_65x129/scatter/mask"][ring].all()
    assert np.array_equal(G["frac_f32_65x129/ring/mask"] != 0, ring)


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("case", CASES)
def test_model_equals_the_reference_in_canonical_form(case, t):
    dem, mask = case_dem(case), G[case + "/mask"]
    r = _ref(case, t)
    labels, tab = om.hierarchy(dem, t, mask)
    assert (labels[mask != 0] == -1).all()
    P = int(np.count_nonzero(tab["lchild"] == NONE)) if len(tab) else 0
    leaf_of_pit = {int(tab["pit_cell"][i]): i for i in range(P)}
    rl = r["labels"].ravel()
    trans = np.array([-1 if v < 0 else leaf_of_pit[int(r["pit_cell"][v])] for v in rl], np.int64)
    assert np.array_equal(trans, labels.ravel().astype(np.int64))
    assert P == int(np.count_nonzero(r["lchild"] == NONE))
    mine, d_mine = dm.canonical(tab["parent"], tab["lchild"], tab["rchild"], tab["pit_cell"], tab["level"], tab["cells"],
                                tab["volume"])
    ref, d_ref = dm.canonical(r["parent"], r["lchild"], r["rchild"], r["pit_cell"], r["level"], r["cells"], r["volume"])
    for d, internal in ((d_mine, len(tab) - P), (d_ref, len(r["parent"]) - P)):
        assert d < 0.05 * max(internal, 1), (d_mine, d_ref, internal)
    assert mine == ref
    # an ocean cell is charged to no node; geolink is NONE exactly where the outside cell drains outside
    out = tab["outside_cell"].astype(np.int64)
    assert np.array_equal(tab["geolink"] == NONE, labels.ravel()[out] == -1)


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("name", RASTERS)
def test_the_ring_mask_and_no_mask_are_the_border_ring_model(name, t):
    dem = G[name + "/dem"]
    labels, tab = dm.hierarchy(dem, t)
    for ocean in (None, om.ring_mask(dem.shape), om.ring_mask(dem.shape).astype(bool)):
        l2, t2 = om.hierarchy(dem, t, ocean)
        assert np.array_equal(l2, labels) and t2.tobytes() == tab.tobytes()
    assert dm.leaves_of.__module__ == "dephier_model"          # the model's own descent is back in place


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("case", FSM_CASES)
def test_fsm_model_on_masked_hierarchies_equals_the_reference_bit_for_bit(case, k):
    dem, mask = case_dem(case), G[case + "/mask"]
    water, wtd = G[f"{case}/w{k}/water"], G[f"{case}/w{k}/wtd"]
    assert (water[mask != 0] == 0).all()
    labels, tab = om.hierarchy(dem, 8, mask)
    r = fm.fill_spill_merge(dem, labels, tab, water)
    assert np.array_equal(r["depth"], wtd)
    assert (r["depth"][mask != 0] == 0).all()
    assert abs(r["water_in"] - (r["standing"] + r["ocean"])) <= dem.size * 2.0 ** -52 * r["water_in"]


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("name", RASTERS)
def test_bucket_model_equals_the_reference(name, t):
    check = G[name + "/bucket/check"]
    got, filled = om.bucket_fill(check, 1, None, t)
    assert np.array_equal(got, G[f"{name}/bucket/t{t}/mask"]) and filled == int(got.sum())
    wall = G[f"{name}/bucket_wall/t{t}/mask_in"]
    got, filled = om.bucket_fill(check, 1, wall, t)
    assert np.array_equal(got, G[f"{name}/bucket_wall/t{t}/mask"]) and filled == int(got.sum()) - int(wall.sum())
    assert (got[wall != 0] == 1).all()
    if t == 8:
        assert np.array_equal(G[name + "/bucket/mask"], G[f"{name}/bucket/t8/mask"])   # the `bucket` mask kind


# ---- rasters worked by hand --------------------------------------------------------------------------------------------
def test_a_land_pit_in_a_raster_corner():
    # cell 0 (value 1) is a pit ON the border; the one ocean cell is 8 (value 9), higher than all the land
    z = np.array([[1, 4, 6],
                  [3, 5, 7],
                  [8, 2, 9]], np.int32)
    ocean = np.zeros((3, 3), np.uint8)
    ocean[2, 2] = 1
    lab, tab = om.hierarchy(z, 8, ocean)
    # D8: 1 -> 0, 3 -> 0, 4 -> 0 (lowest neighbour 1); 2 (6) -> 1 (4) -> 0; 5 (7) -> 7 (2); 6 (8) -> 7; 7 is a pit
    assert lab.tolist() == [[0, 0, 0], [0, 0, 1], [1, 1, -1]]
    assert len(tab) == 3 and tab["pit_cell"].tolist() == [0, 7, 0]
    # edges by key: (3; 3, 7) joins the two leaves at level 3; (9; 8, 4) -- the ocean cell is the HIGHER cell -- makes the
    # merged node a root: its outside cell is the ocean cell, geolink NONE
    assert tab["parent"].tolist() == [2, 2, NONE] and tab["level"].tolist() == [3, 3, 9]
    assert (tab["inside_cell"][0], tab["outside_cell"][0]) == (3, 7) and (tab["inside_cell"][1], tab["outside_cell"][1]) == (7, 3)
    assert (tab["inside_cell"][2], tab["outside_cell"][2], tab["geolink"][2]) == (4, 8, NONE)
    assert tab["cells"].tolist() == [2, 1, 8] and tab["volume"].tolist() == [2, 1, sum(9 - v for v in (1, 4, 6, 3, 5, 7, 8, 2))]
    for m, (cells, vol) in enumerate(dm.brute_cells_volume(z, lab, tab)):
        assert tab["cells"][m] == cells and tab["volume"][m] == float(vol)


def test_a_pit_whose_spill_pairs_higher_cell_is_an_ocean_cell():
    # 1 x 5, D4: the ocean cell 2 (value 5) is a wall between the pits 1 and 3; both spill over it
    z = np.array([[7, 1, 5, 2, 8]], np.int16)
    ocean = np.array([[0, 0, 1, 0, 0]], np.uint8)
    lab, tab = om.hierarchy(z, 4, ocean)
    assert lab.tolist() == [[0, 0, -1, 1, 1]]
    assert len(tab) == 2 and tab["parent"].tolist() == [NONE, NONE]
    assert tab["inside_cell"].tolist() == [1, 3] and tab["outside_cell"].tolist() == [2, 2] and tab["geolink"].tolist() == [NONE, NONE]
    assert tab["level"].tolist() == [5, 5] and tab["cells"].tolist() == [1, 1] and tab["volume"].tolist() == [4, 3]


@pytest.mark.parametrize("t", [8, 4])
def test_one_row_and_two_by_two(t):
    z = np.array([[5, 3, 4, 1, 6, 2, 9, 0, 7]], np.uint8)
    ocean = np.zeros_like(z)
    ocean[0, 4] = 1                                            # the cell of value 6
    lab, tab = om.hierarchy(z, t, ocean)
    # pits: 1 (3), 3 (1), 5 (2), 7 (0); 0 -> 1; 2 -> 3; 6 (9) -> 7; 8 (7) -> 7
    assert lab.tolist() == [[0, 0, 1, 1, -1, 2, 3, 3, 3]]
    # (4; 2, 1) joins leaves 0, 1 -> node 4; (6; 4, 3) roots node 4; (6; 4, 5) roots leaf 2; (9; 6, 5): leaf 3 joins the outside
    assert tab["parent"].tolist() == [4, 4, NONE, NONE, NONE] and tab["level"].tolist() == [4, 4, 6, 9, 6]
    assert tab["geolink"].tolist() == [1, 0, NONE, 2, NONE]
    assert tab["cells"].tolist() == [1, 2, 1, 3, 4]
    z2 = np.array([[4, 1], [3, 2]], np.float32)
    o2 = np.array([[1, 0], [0, 0]], bool)
    lab, tab = om.hierarchy(z2, t, o2)
    assert lab.tolist() == [[-1, 0], [0, 0]] and len(tab) == 1
    assert (tab["inside_cell"][0], tab["outside_cell"][0], tab["level"][0], tab["cells"][0], tab["volume"][0]) == (1, 0, 4, 3, 6)
    lab, tab = om.hierarchy(z2, t, np.ones((2, 2), np.uint8))
    assert (lab == -1).all() and len(tab) == 0
    with pytest.raises(ValueError):
        om.hierarchy(z2, t, np.zeros((2, 2), np.uint8))


def test_bucket_fill_by_hand():
    c = np.array([[1, 0, 0, 0, 0],
                  [0, 1, 0, 1, 0],
                  [0, 0, 0, 1, 0],
                  [0, 0, 0, 0, 0]], np.int8)
    m8, n8 = om.bucket_fill(c, 1, None, 8)
    m4, n4 = om.bucket_fill(c, 1, None, 4)
    assert n8 == 2 and m8[0, 0] == 1 and m8[1, 1] == 1 and m8[1, 3] == 0        # the diagonal link; the lake stays 0
    assert n4 == 1 and m4[1, 1] == 0
    f = np.array([[np.nan, 0.0, -0.0]], np.float32)
    assert om.bucket_fill(f, np.nan, None, 8)[1] == 0 and om.bucket_fill(f, 0.0, None, 8)[0].tolist() == [[0, 1, 1]]
