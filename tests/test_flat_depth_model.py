"""CPU-side checks of the rasters of flat_depth_cases.py: every case that test_flats_depth_gpu.py runs really is a flat
whose towards-lower levels end at exactly D, drains completely in the oracle, and stays small.

OVERSIZE: two of the 292 cases cannot meet the 200 000-cell limit.  A channel row of the 64-wide block adds at most
61 levels (62 channel cells, the two diagonal steps at a turn give two of them the same level), the raster with 24 wall
columns beside it is 88 wide, so D = 0x10000 + 5000 = 70 536 needs 2 * ceil(70 536 / 61) + 1 = 2315 rows = 203 720 cells; even
with the block's own margin column given up to the padding (63 channel cells, 62 levels a row) it would be
2277 * 88 = 200 376.  Those two are held to exactly that size instead; every other case to the limit."""
import numpy as np
import pytest

import flat_depth_cases as fc

OVERSIZE = {(64, False, 24, fc.FAR[1]): 2315 * 88, (64, True, 24, fc.FAR[1]): 2315 * 88}


def test_the_case_lists_are_what_the_depth_tests_promise():
    assert set(range(0xFEF0, 0x10111, 32)) <= set(fc.BAND) and min(fc.BAND) == 0xFEF0 and max(fc.BAND) == 0x10110
    for lo, hi in ((0xFEFE, 0xFF01), (0xFFEE, 0xFFF1), (0xFFFD, 0x10002)):
        assert set(range(lo, hi + 1)) <= set(fc.BAND)
    assert fc.FAR == (0x10000 + 600, 0x10000 + 5000) and all(d <= 0xFE00 for d in fc.SHALLOW) and len(fc.SHALLOW) == 2
    assert len(fc.SWEEP) == 8 * len(fc.DEPTHS) == len(set(fc.SWEEP))
    assert sorted({s for (_, _, s, _) in fc.SEAMS}) == list(range(0, 64, 8)) and len(fc.SEAMS) == 16
    assert all(w == 200 and d == 0x10000 + 600 for (w, _, _, d) in fc.SEAMS)
    assert len(fc.SCHEDULE_CASES) == 14 and len(fc.ROUTE_CASES) == 5
    assert set(OVERSIZE) <= set(fc.ALL_CASES)


@pytest.mark.parametrize("geometry", fc.GEOMETRIES + [(200, t, s) for t in (False, True) for s in fc.SEAM_SHIFTS if s not in (0, 24)],
                         ids=lambda g: f"w{g[0]}{'T' if g[1] else ''}-s{g[2]}")
def test_cases_are_exactly_that_deep_and_drain(orc, geometry):
    cases = [c for c in fc.ALL_CASES if c[:3] == geometry]
    assert cases
    for case in cases:
        width, transpose, shift, depth = case
        dem = fc.build(case)
        assert dem.dtype == np.int32 and dem.shape[0 if transpose else 1] == width + shift, fc.case_id(case)
        if case in OVERSIZE:
            assert dem.size == OVERSIZE[case], (fc.case_id(case), dem.shape)
        else:
            assert dem.size < fc.MAX_CELLS, (fc.case_id(case), dem.shape)
        _, mask, _ = orc.port.resolve_flats(dem, fc.NODATA)
        assert int(mask.max()) == 2 * depth, (fc.case_id(case), int(mask.max()))
        chan = dem == fc.CHANNEL
        assert int(mask[chan].max()) == 2 * depth and int((dem == fc.LOW).sum()) == 1
        dirs = orc.port.flat_resolution(dem, fc.NODATA)
        assert (dirs[chan] != 0).all(), fc.case_id(case)


def test_every_case_belongs_to_a_checked_geometry():
    geoms = set(fc.GEOMETRIES) | {(200, t, s) for t in (False, True) for s in fc.SEAM_SHIFTS}
    assert {c[:3] for c in fc.ALL_CASES} == geoms


def test_the_channel_is_one_cell_wide_beside_walls():
    """Every channel cell touches a wall (away level 1 everywhere), channel rows lie on every second raster row."""
    dem = fc.build((200, False, 8, 0xFFF0))
    chan = dem == fc.CHANNEL
    pad = np.pad(dem, 1, constant_values=fc.WALL)
    wall_near = np.zeros_like(chan)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            wall_near |= pad[dy:dy + dem.shape[0], dx:dx + dem.shape[1]] == fc.WALL
    assert wall_near[chan].all()
    assert (chan[1::2].sum(axis=1) >= 1).all() and (chan[2::2].sum(axis=1) <= 1).all() and not chan[0].any()
    assert (dem[:, :8] != fc.CHANNEL).all() and dem[1, 8] == fc.LOW
    t = fc.build((200, True, 8, 0xFFF0))
    assert np.array_equal(t.T, dem)
