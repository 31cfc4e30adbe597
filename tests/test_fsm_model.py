"""The Fill-Spill-Merge contract in numpy (tests/fsm_model.py) against the reference's recorded results
(tests/golden/ref_fsm.npz, every cell), its conservation of water, its independence of the pour order, the hand-made
rasters with their expected arrays written out (tests/fsm_cases.py) and the cascade of 2000 roots.  No GPU."""
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
import fsm_cases as fc  # noqa: E402
import fsm_model as fm  # noqa: E402


@functools.lru_cache(maxsize=None)
def _golden():
    G = load_golden(os.path.join(GOLDEN, "ref_fsm.npz"))
    out = {}
    for name, k, dem, water, wtd, diff in fc.golden_cases(G):
        if name not in out:
            out[name] = (dem, *dm.hierarchy(dem, 8), [])
        out[name][3].append((water, wtd, diff))
    return out


NAMES = ["frac_f32_40x30", "frac_f32_65x129", "frac_f32_300x257", "perm_i32_65x129", "perm_i32_200x130"]


def test_the_golden_file_has_the_five_cases():
    assert sorted(_golden()) == sorted(NAMES) and all(len(v[3]) == 4 for v in _golden().values())


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_reference_on_every_cell(name):
    dem, labels, table, waters = _golden()[name]
    span = float(dem.max()) - float(dem.min())
    bound = 2.0 ** -44 * max(1.0, span)
    for k, (water, wtd, recorded) in enumerate(waters):
        assert (water[0, :] == 0).all() and (water[-1, :] == 0).all() and (water[:, 0] == 0).all() and (water[:, -1] == 0).all()
        r = fm.fill_spill_merge(dem, labels, table, water)
        diff = float(np.abs(r["depth"] - wtd).max())
        print(name, "water", k, "largest |model - reference|", diff, "recorded", recorded, "bound", bound)
        assert recorded <= bound
        assert diff <= bound
        # conservation: what stands and what left is what came in
        tol = dem.size * 2.0 ** -52 * r["water_in"]
        assert abs(r["standing"] + r["ocean"] - r["water_in"]) <= tol
        assert abs(float(wtd.sum()) + r["ocean"] - r["water_in"]) <= tol


@pytest.mark.parametrize("name", NAMES)
def test_the_pour_order_does_not_matter(name):
    dem, labels, table, waters = _golden()[name]
    bound = 2.0 ** -44 * max(1.0, float(dem.max()) - float(dem.min()))
    for water, _, _ in waters:
        a = fm.fill_spill_merge(dem, labels, table, water)
        b = fm.fill_spill_merge(dem, labels, table, water, reverse=True)
        diff = float(np.abs(a["depth"] - b["depth"]).max())
        print(name, "largest change of a depth under the reversed pour order", diff)
        assert diff <= min(bound, dem.size * 2.0 ** -52 * a["water_in"])
        assert a["lakes"] == b["lakes"]


@pytest.mark.parametrize("name", NAMES)
def test_the_shortcut_leaves_the_values_of_the_plain_loop(name):
    dem, labels, table, waters = _golden()[name]
    for water, _, _ in waters:
        a = fm.fill_spill_merge(dem, labels, table, water)
        b = fm.fill_spill_merge(dem, labels, table, water, shortcut=False)
        assert np.array_equal(a["node_water"], b["node_water"]) and a["ocean"] == b["ocean"]
        assert np.array_equal(a["depth"], b["depth"]) and b["shortcut_hits"] == 0


@pytest.mark.parametrize("name", list(fc.hand_made()))
def test_hand_made_rasters(name):
    dem, water, exp = fc.hand_made()[name]
    assert 5 <= min(dem.shape) and max(dem.shape) <= 9
    labels, table = dm.hierarchy(dem, 8)
    r = fm.fill_spill_merge(dem, labels, table, water)
    assert np.array_equal(r["depth"], exp["depth"])
    assert r["node_water"].tolist() == exp["node_water"] and r["ocean"] == exp["ocean"]
    assert (r["lakes"], r["full_lakes"], r["tops"].tolist()) == (exp["lakes"], exp["full_lakes"], exp["tops"])
    assert r["water_in"] == float(water.sum())
    assert abs(r["standing"] + r["ocean"] - r["water_in"]) <= dem.size * 2.0 ** -52 * r["water_in"]


def test_cascade_of_roots_without_recursion():
    dem, water = fc.cascade()
    assert dem.shape == (5, 8003)
    labels, table = dm.hierarchy(dem, 8)
    k = fc.CASCADE_PITS
    assert len(table) == k and (table["parent"] == dm.NONE).all()                 # every pit is a root of its own
    assert np.array_equal(table["geolink"][:-1], np.arange(1, k)) and table["geolink"][-1] == dm.NONE
    assert k > sys.getrecursionlimit()                                             # a recursive pour would not get there
    r = fm.fill_spill_merge(dem, labels, table, water)
    assert r["pours"] == 1 and r["longest_pour"] == k - 1                          # one hop per root below the first
    assert r["lakes"] == r["full_lakes"] == k and r["ocean"] == 7.0
    assert np.array_equal(r["node_water"], table["volume"])
    assert r["standing"] == 60.0 * (k - 1) + 100.0
    # a second pour from the top now takes the shortcut to the ocean in one step
    w, ocean, st = fm.pour(table, np.r_[water[2, 3], np.zeros(k - 2), 5.0])
    assert ocean == 12.0 and st["longest_pour"] == k - 1


def test_seam_rasters_are_what_their_names_say():
    dem, water = fc.bowl_130()
    labels, table = dm.hierarchy(dem, 8)
    r = fm.fill_spill_merge(dem, labels, table, water)
    assert len(table) == 1 and (r["lakes"], r["full_lakes"], r["records"]) == (1, 0, 127 * 127)
    assert np.count_nonzero(r["depth"]) > 8000 and r["water_in"] == 64.0 * 128 * 128
    assert abs(r["standing"] - r["water_in"]) <= dem.size * 2.0 ** -52 * r["water_in"]
    dem, water = fc.egg_carton()
    labels, table = dm.hierarchy(dem, 8)
    r = fm.fill_spill_merge(dem, labels, table, water)
    leaves = int(np.count_nonzero(table["lchild"] == dm.NONE))
    assert leaves >= 42 * 42 and r["lakes"] > 1000 and 100 < r["full_lakes"] < r["lakes"] - 1000
    assert np.count_nonzero(r["tops"] >= leaves) > 100 and r["records"] >= r["lakes"] - r["full_lakes"]
    assert abs(r["standing"] + r["ocean"] - r["water_in"]) <= dem.size * 2.0 ** -52 * r["water_in"]
