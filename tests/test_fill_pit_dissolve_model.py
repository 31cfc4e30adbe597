"""Dissolved pits, as a numpy model against the oracle's fill -- on the CPU, independent of any kernel.

A pit whose lowest neighbour q does not drain into it is no depression of its own: it points at q, its catchment joins
q's tree, and it alone keeps the floor key(q) (pit_dissolve_model.py).  The claim pinned here: the fill of the coarser
forest with that floor is the oracle's surface, cell for cell, under D8 and D4 -- with every such pit dissolved, with only
those whose q lies in their 64 x 64 tile (what k_descent16 does, and the count the GPU test compares), and with none."""
import numpy as np
import pytest

import pit_dissolve_model as pm
from richdem_amd.synth import fractal_dem, fractal_dem_int


def _dems():
    rng = np.random.default_rng(5)
    return {
        "fractal 190x130": fractal_dem(190, 130, 11),
        "fractal 300x257": fractal_dem(300, 257, 3),
        "fractal 64x64": fractal_dem(64, 64, 3),
        "plateaus x0.05": fractal_dem_int(160, 120, 12, 0.05),
        "plateaus x1.0": fractal_dem_int(160, 120, 12, 1.0),
        "white noise 70x60": rng.random((60, 70)).astype(np.float32),
        "integers 0..2": rng.integers(0, 3, (50, 40)).astype(np.int32),
        "integers 0..5": rng.integers(0, 6, (50, 40)).astype(np.int32),
        "3x3": rng.random((3, 3)).astype(np.float32),
        "5x7": rng.random((7, 5)).astype(np.float32),
        "9x4": rng.random((4, 9)).astype(np.float32),
        "diagonal pits 130x130": pm.diagonal_pits(130, 130),
        "border pit": pm.border_pit(),
    }


DEMS = _dems()


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", sorted(DEMS))
def test_model_with_dissolved_pits_equals_the_oracle(orc, name, topo):
    z = DEMS[name]
    exp = orc.port.fill(z, topo)
    infos = {}
    for what, kw in (("all", dict(tile=None)), ("in tile", dict(tile=64)), ("none", dict(dissolve=False))):
        got, info = pm.fill_dissolve(z, topo, **kw)
        infos[what] = info
        print(name, f"D{topo}", what, info)
        assert got.dtype == exp.dtype and np.array_equal(got, exp), (name, topo, what, int((got != exp).sum()))
        assert info["basins"] + info["dissolved"] == info["pits"]
    assert infos["none"]["dissolved"] == 0
    assert infos["all"]["dissolved"] == infos["all"]["candidates"] >= infos["in tile"]["dissolved"]
    assert infos["in tile"]["dissolved"] == infos["in tile"]["candidates"] - infos["in tile"]["ring_out"]


@pytest.mark.parametrize("topo", [8, 4])
def test_the_diagonal_plane_dissolves_chains_and_every_pit(orc, topo):
    """every pit of the plane is dissolvable (its q runs on down the slope), so no basin is left; the pits on a tile's first
    row or column have their q in the next tile and stay, under the tile restriction"""
    z = pm.diagonal_pits(130, 130)
    _, info = pm.fill_dissolve(z, topo, tile=None)
    assert info["pits"] > 300 and info["dissolved"] == info["pits"] and info["basins"] == 0, info
    _, tiled = pm.fill_dissolve(z, topo, tile=64)
    assert tiled["ring_in"] > 0 and tiled["ring_out"] > 0 and tiled["basins"] == tiled["ring_out"], tiled
    exp = orc.port.fill(z, topo)
    y, x = np.mgrid[0:130, 0:130]
    raised = exp != z
    assert raised.sum() == info["pits"]                              # single cells: nothing but the pits is raised
    assert (exp[raised] == (2 * y + 3 * x)[raised] - (5 if topo == 8 else 3)).all()   # ... to the key of q


def test_a_pit_beside_the_border_dissolves_into_the_outside(orc):
    z = pm.border_pit()
    for topo in (8, 4):
        got, info = pm.fill_dissolve(z, topo, tile=64)
        assert info == dict(pits=1, dissolved=1, basins=0, candidates=1, ring_in=0, ring_out=0, rounds=0), info
        assert np.array_equal(got, orc.port.fill(z, topo))
        assert got[1, 3] == (z[0, 2] if topo == 8 else z[0, 3])
