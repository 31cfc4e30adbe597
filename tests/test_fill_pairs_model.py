"""tests/pairs_model.py on the CPU: the rasters of test_fill_pairs_residency_gpu.py are what their names say (boundary cells
per pair tile, nodes per descent tile, the crossings' low passes), and the committed list-cap rasters are what
tests/tools/make_pairs_list_cap.py makes."""
import numpy as np
import pytest

import flooded_tiles_model as fm
import pairs_model as pmod
import pit_dissolve_model as pm


@pytest.mark.parametrize("topo", [8, 4])
def test_forest_is_the_dissolve_models(topo):
    """the basins of pairs_model.forest are those fill_dissolve contracts: same count, and the fill it gives is the oracle's
    (test_fill_pit_dissolve_model.py) -- here only the count, on the raster with the most basins"""
    z = pmod.small_basins()
    _, lab = pmod.forest(z, topo)
    _, info = pm.fill_dissolve(z, topo, tile=64)
    assert int(lab.max()) == info["basins"]


@pytest.mark.parametrize("topo", [8, 4])
def test_small_basins_overflow_the_list_and_not_the_node_table(topo):
    z = pmod.small_basins()
    ptr, lab = pmod.forest(z, topo)
    bc, nd = pmod.boundary_cells(lab, topo), pmod.nodes(ptr, z.shape)
    assert bc.shape == (3, 3) and nd.shape == (2, 3)
    assert bc.max() > 1024 and bc.min() <= pmod.LIST_CAP and nd.max() <= pmod.NT_CAP


@pytest.mark.parametrize("topo", [8, 4])
def test_list_cap_rasters(topo):
    g = pmod.golden()
    for n in (pmod.LIST_CAP, pmod.LIST_CAP + 1, 1024, 1025):
        z = g[f"d{topo}_{n}"]
        assert z.dtype == np.float32 and z.shape == (50, 100)
        ptr, lab = pmod.forest(z, topo)
        bc = pmod.boundary_cells(lab, topo)
        assert bc[0, 0] == n == bc.max() and pmod.nodes(ptr, z.shape).max() <= pmod.NT_CAP


def test_many_nodes_lie_between_the_caps():
    z = fm.many_nodes()
    ptr, _ = pmod.forest(z, 4, dissolve=False)
    nd = pmod.nodes(ptr, z.shape)
    assert pmod.NT_CAP < nd[1, 1] <= 1024 and nd[1, 1] >= fm.pits_in_centre_d4(z)


def test_crossings_have_their_low_pass_across_a_tile_edge():
    z = pmod.ring_crossings()
    _, lab = pmod.forest(z, 8)
    for name, cells in pmod.CROSSINGS.items():
        a, b = cells[1], cells[2]
        assert (a[0] // 32, a[1] // 64) != (b[0] // 32, b[1] // 64), name
        assert pmod.low_pass_only_at(z, lab, a, b), name
