"""The model of D-infinity across flats (tests/dinf_flats_model.py) on the CPU: a plateau whose flat mask is written down
here by hand, and six random-integer DEMs after the fill, where every cell of a drainable flat must get flow and the
accumulation over the composed proportions must carry every cell's unit to the raster's edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinf_flats_model as model  # noqa: E402

NDV = np.float32(-9999)
LEFT, UPLEFT, UP, UPRIGHT, RIGHT, DOWNRIGHT, DOWN, DOWNLEFT = range(1, 9)

# A 7 x 7 level block (rows 3..9, columns 2..8) drains through a one-cell-wide corridor (row 6, columns 9..15) into the
# outlet (6, 16) and on to the raster's edge; the rim rises with the distance from them.  flat_mask of the flat's rows
# 3..9, columns 2..15 (Barnes: twice the distance towards the low edge (6, 15), plus the distance away from higher ground
# counted back from the flat's largest; 0 outside the flat):
PLATEAU_MASK = np.array([
    [31, 29, 27, 25, 23, 23, 23, 0, 0, 0, 0, 0, 0, 0],
    [31, 28, 26, 24, 22, 20, 21, 0, 0, 0, 0, 0, 0, 0],
    [31, 28, 25, 23, 21, 20, 19, 0, 0, 0, 0, 0, 0, 0],
    [31, 28, 25, 22, 21, 20, 19, 17, 15, 13, 11, 9, 7, 2],
    [31, 28, 25, 23, 21, 20, 19, 0, 0, 0, 0, 0, 0, 0],
    [31, 28, 26, 24, 22, 20, 21, 0, 0, 0, 0, 0, 0, 0],
    [31, 29, 27, 25, 23, 23, 23, 0, 0, 0, 0, 0, 0, 0]], np.int32)


def plateau():
    h, w = 13, 20
    flat = np.zeros((h, w), bool)
    flat[3:10, 2:9] = True
    flat[6, 9:16] = True
    low = flat.copy()
    low[6, 16:] = True
    ys, xs = np.nonzero(low)
    yy, xx = np.mgrid[0:h, 0:w]
    z = (10 + np.min(np.maximum(abs(yy[..., None] - ys), abs(xx[..., None] - xs)), axis=-1)).astype(np.float32)
    z[flat] = 5
    z[6, 16:] = (4, 3, 2, 1)
    mask = np.zeros((h, w), np.int32)
    mask[3:10, 2:16] = PLATEAU_MASK
    return z, flat, mask


def shares(props, y, x):
    return {n: float(props[y, x, n]) for n in range(1, 9) if props[y, x, n] > 0}


def test_plateau_with_a_hand_written_mask(orc):
    z, flat, mask = plateau()
    d8, omask, labels = orc.port.resolve_flats(z, NDV)
    assert np.array_equal(omask, mask)                                 # the oracle agrees with the mask written above
    assert np.array_equal(labels != 0, flat) and len(np.unique(labels[flat])) == 1
    assert np.array_equal(d8 == 0, flat & ~((np.arange(20) == 15) & (np.arange(13) == 6)[:, None]))
    base = orc.port.fm_tarboton(z, NDV)
    props, info = model.compose_from(orc, base, d8, mask, labels)
    assert model.stats_of(info) == {"noflow_cells": 55, "patched_cells": 55, "fallback_cells": 7, "unresolved_cells": 0}
    assert info["two_receivers"] == 18 and info["one_receiver"] == 30
    assert np.array_equal(props[~info["patched"]], base[~info["patched"]])
    # the corridor, and the block cell in front of it: no facet lies inside the flat (or none descends) -- everything to the
    # first neighbour with a smaller mask value, which is the one to the right
    for x in range(8, 15):
        assert shares(props, 6, x) == {RIGHT: 1.0}, x
    # the block's axis flows right; its corners turn towards the axis with both receivers of one facet
    for x in range(2, 8):
        assert shares(props, 6, x) == {RIGHT: 1.0}, x
    # masks 31 -> 29 (s1 = 2) -> 28 (s2 = 1): the angle r = atan2(1, 2) in the facet; FM_Tarboton (Tarboton1997.hpp:99-112)
    # stores r / (pi / 4) for the facet's first neighbour where the facet's sign is -1, and for its second where it is +1
    a = float(np.float32(np.arctan2(1.0, 2.0) / (np.pi / 4)))
    assert shares(props, 3, 2) == pytest.approx({RIGHT: a, DOWNRIGHT: 1 - a}, rel=1e-6)
    assert shares(props, 9, 2) == pytest.approx({RIGHT: a, UPRIGHT: 1 - a}, rel=1e-6)
    assert shares(props, 3, 8) == pytest.approx({DOWN: a, DOWNLEFT: 1 - a}, rel=1e-6)
    # every share of a patched cell points at a strictly smaller mask value of the same flat
    for y, x in np.argwhere(info["patched"]):
        s = shares(props, y, x)
        assert s and sum(s.values()) == pytest.approx(1.0, rel=1e-6)
        for n in s:
            assert flat[y + model.DY[n], x + model.DX[n]] and mask[y + model.DY[n], x + model.DX[n]] < mask[y, x], (y, x, n)
    # one unit per flat cell: all 56 pass the low edge and reach the raster's edge; without the patch none moves
    acc = orc.port.flow_accumulation(props, flat.astype(np.float64))
    assert acc[6, 15] == pytest.approx(56.0, rel=1e-12) and acc[6, 19] == pytest.approx(56.0, rel=1e-12)
    assert orc.port.flow_accumulation(base, flat.astype(np.float64)).max() == 1.0


@pytest.mark.parametrize("seed", range(6))
def test_random_integer_dems_drain(orc, seed):
    dem = model.random_integer_dem(orc, seed)
    assert dem.shape == (71, 97)
    props, info = model.compose(orc, dem, NDV)
    st = model.stats_of(info)
    print(seed, st, "two receivers", info["two_receivers"], "one receiver", info["one_receiver"])
    assert 2000 <= st["patched_cells"] == st["noflow_cells"] and st["fallback_cells"] >= 500 and st["unresolved_cells"] == 0
    assert info["one_receiver"] >= 500
    flows = props[..., 0] == 0.0
    assert flows[1:-1, 1:-1].all()                                       # every interior cell, the patched ones among them
    acc = orc.port.flow_accumulation(props)
    edge = np.ones(dem.shape, bool)
    edge[1:-1, 1:-1] = False
    assert (acc >= 1.0).all()
    # nothing is held back in a cycle or a dam: a cell's two float32 shares sum to 1 within 2^-24 and a path is shorter than
    # 1000 cells, so the edge receives the cell count within 1000 * 2^-24 = 6e-5 -- less than one cell of 6887
    assert acc[edge].sum() == pytest.approx(dem.size, rel=6e-5)
    before = orc.port.flow_accumulation(orc.port.fm_tarboton(dem, NDV))
    assert before[edge].sum() < 0.7 * dem.size and acc.max() > 20 * before.max()
