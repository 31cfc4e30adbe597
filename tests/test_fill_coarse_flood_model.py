"""The two facts a coarse flood ahead of the fill's pair pass would rest on (coarse_flood_model.py),
against the CPU oracle's fill under D8 and D4, for both block sizes measured at full size:

  A.  LB, the fill of the raster of block minima, lies at or below the filled surface on every cell, and a tile it flags
      is one of the finalize's flooded tiles (flooded_tiles_model);
  B.  the basin graph in which every flagged tile's own pairs are replaced by a star and a ring has the plain fill's
      levels: its surface equals the oracle's cell for cell.

Also pins what each raster is built to show."""
import numpy as np
import pytest

import coarse_flood_model as cm
import flooded_tiles_model as fm
from richdem_amd.synth import fractal_dem

RASTERS = {CB: cm.rasters(CB) for CB in cm.BLOCKS}
CASES = [(CB, name) for CB in cm.BLOCKS for name in RASTERS[CB]]


def _check(orc, z, CB, topo, what, pick=0):
    """the three checks; returns (flags, census, the model's info)"""
    fill = orc.port.fill
    W = fill(z, topo)
    h, w = z.shape
    LB = cm.lower_bound(z, CB, topo, fill)
    up = np.repeat(np.repeat(LB, CB, axis=0), CB, axis=1)[:h, :w]
    assert (up <= W).all(), (what, "LB above the filled surface")
    fl, cs = cm.flags(z, CB, topo, fill), cm.census(z, W)
    assert not (fl & ~cs).any(), (what, "a flagged tile that is not flooded")
    M, info = cm.levels_with_flags(z, topo, fl, pick)
    assert M.dtype == W.dtype and np.array_equal(M, W), (what, "the model's surface", int((M != W).sum()))
    return fl, cs, info


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"cb{c[0]}-{c[1]}")
def test_flags_are_flooded_and_the_model_fills(orc, case, topo):
    CB, name = case
    z, expected = RASTERS[CB][name]
    fl, cs, info = _check(orc, z, CB, topo, f"{name} CB {CB} D{topo}", pick=1)
    print(name, f"CB {CB} D{topo}", "flagged:", int(fl.sum()), "census:", int(cs.sum()), info)
    assert int(fl.sum()) == expected, (name, CB, topo, int(fl.sum()))


@pytest.mark.parametrize("CB", cm.BLOCKS)
@pytest.mark.parametrize("whs", list(cm.FRACTALS), ids=lambda c: f"{c[0]}x{c[1]}s{c[2]}")
def test_fractals(orc, whs, CB):
    w, h, seed = whs
    z = fractal_dem(w, h, seed)
    flagged, n_census = cm.FRACTALS[whs]
    for topo in (8, 4):
        fl, cs, info = _check(orc, z, CB, topo, f"fractal {whs} CB {CB} D{topo}")
        print("fractal", whs, f"CB {CB} D{topo}", "flagged:", int(fl.sum()), "census:", int(cs.sum()), info)
        if topo == 8:
            assert int(fl.sum()) == flagged[CB], (whs, CB, int(fl.sum()))
            if n_census is not None:
                assert int(cs.sum()) == n_census


def test_the_model_without_flags_is_the_plain_fill(orc):
    for z in (fm.many_nodes(), fm.two_lakes(), fm.dissolved_under_wall(), fractal_dem(520, 390, 11)):
        for topo in (8, 4):
            M, info = cm.levels_with_flags(z, topo, np.zeros(cm.interior_tiles(z.shape).shape, bool))
            assert info["dropped"] == 0 and info["added"] == 0 and np.array_equal(M, orc.port.fill(z, topo))


@pytest.mark.parametrize("CB", cm.BLOCKS)
def test_the_rasters_show_what_they_are_for(orc, CB):
    fill = orc.port.fill
    r = RASTERS[CB]
    # the thin wall floods its centre tile and no block sees the lake
    z = r["thin wall"][0]
    assert cm.census(z, fill(z, 8)).sum() == 1 and (cm.lower_bound(z, CB, 8, fill) < 10).all()
    # the spill: the lake stands at 9, the channel's first cell lies on the last inner tile's ring and is not raised
    n = r["spill east"][0].shape[0]
    y0 = x0 = n - 2 * CB - cm.T
    for where, (y, x) in (("east", (y0 + 20, x0 + cm.T)), ("south", (y0 + cm.T, x0 + 20)), ("southwest", (y0 + cm.T, x0 - 1))):
        z = r["spill " + where][0]
        W = fill(z, 8)
        assert (y, x) in cm.ring_cells(y0, x0, 8) and z[y, x] == 9 and W[y, x] == 9 and W[y0 + 5, x0 + 5] == 9
        assert cm.flags(z, CB, 8, fill)[y0 // cm.T, x0 // cm.T]
    assert (y0 + cm.T, x0 - 1) not in cm.ring_cells(y0, x0, 4)               # (D4 does not look SW: another tile's record)
    # two lakes: 10 and 20 on either side of a wall of 30 that no block sees; flagged tiles on both sides
    z, xw = cm.two_thick_lakes(CB)
    W = fill(z, 8)
    ym = z.shape[0] // 2
    assert W[ym, xw - 5] == 10 and W[ym, xw + 5] == 20 and W[ym, xw] == 30
    assert (cm.lower_bound(z, CB, 8, fill)[2:-2, 2:-2] == 10).all()
    fl = cm.flags(z, CB, 8, fill)
    assert fl[ym // cm.T, xw // cm.T - 1] and fl[ym // cm.T, xw // cm.T + 1] and not fl[:, xw // cm.T].any()
    # a ring cell at the level keeps its bits and keeps its tile out
    t0 = (2 * CB + cm.T - 1) // cm.T * cm.T
    for kind, level in (("at", 10.0), ("island", 10.0), ("minus zero", 0.0)):
        z = r["ring " + {"at": "at level"}.get(kind, kind)][0]
        W = fill(z, 8)
        y, x = t0 + 20, t0 + cm.T
        assert (y, x) in cm.ring_cells(t0, t0, 8) and W[y, x] == z[y, x] == level and W[y, x - 1] == level > z[y, x - 1]
        assert np.signbit(W[y, x]) == (kind == "minus zero")
        fl = cm.flags(z, CB, 8, fill)
        assert fl[t0 // cm.T, t0 // cm.T] and not fl[t0 // cm.T, t0 // cm.T + 1]
    # many nodes: more basins in a flagged tile than a wavefront has lanes, by far
    for topo in (8, 4):
        z = r["many nodes"][0]
        _, info = cm.levels_with_flags(z, topo, cm.flags(z, CB, topo, fill))
        assert info["most_basins_in_a_flagged_tile"] > 4 * 64
    # the rasters have teeth: a ring record that weighs K alone joins the two lakes below their wall
    z, xw = cm.two_thick_lakes(CB)
    M, _ = cm.levels_with_flags(z, 8, cm.flags(z, CB, 8, fill), ring_key=False)
    assert not np.array_equal(M, fill(z, 8)) and M[ym, xw + 5] < 20


def test_the_librarys_block_size_is_modelled(rd):
    assert rd.fill_coarse_block() in cm.BLOCKS
