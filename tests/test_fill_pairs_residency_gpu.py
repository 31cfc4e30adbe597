"""The pair pass of the compact fill (k_pairs16, csrc/fill.hip) on the paths that seven
resident blocks per CU brought: a ring without the row above the tile, a boundary list of LIST_CAP = 1 008 cells with one
pass per band of eight rows when a tile has more, and a node table of NT_CAP = 512 entries in LDS.

Every case is compared with the CPU oracle's fill cell for cell, bits included, under D8 and D4; the debug line must show
that the compact path ran to its end (none of FALLBACKS, two stream synchronisations); the input must be unchanged.  What
makes a case a case is asserted on the CPU first, with tests/pairs_model.py (the descent forest of pit_dissolve_model.py,
the boundary cells per 64 x 32 pair tile, the nodes per 64 x 64 descent tile):

  band passes       130 x 70 (2 x 3 pair tiles, ragged both ways), smoothed white noise: a pair tile with more than 1 024
                    boundary cells, no descent tile above 512 nodes
  the cap exactly   a tile with exactly LIST_CAP boundary cells (one pass) and the same raster with ONE cell changed and
                    LIST_CAP + 1 (the band passes); the same at 1 024 and 1 025, half a tile's cells -- both in band
                    passes
  many nodes        the flooded-tiles tests' white-noise tile, D4 without dissolving: 513 ... 1 024 nodes, gathered from
                    the node table in HBM since NT_CAP is 512 (it was staged in LDS before)
  ring crossings    214 x 141 (not multiples of 64 / 32): pairs of depressions whose only low pass is one step across the
                    top edge of a pair tile (S, SW, SE), across each of its four corners, across its left edge from the
                    second row down and in its first row -- found through the ring cells of the tile above / to the left
  fractal           520 x 390, seeds 3 and 11: the host entry, the device entry, and a stream of its own"""
import numpy as np
import pytest

import flooded_tiles_model as fm
import pairs_model as pmod
from richdem_amd.synth import fractal_dem

pytestmark = pytest.mark.gpu

FALLBACKS = ("node table overflow", "hook chain unfinished", "pair list overflow")
SWITCHES = ("RDGPU_DEVICES", "RDGPU_FILL_EDGES", "RDGPU_FILL_EDGE_CAP", "RDGPU_FILL_ROUND_BATCH", "RDGPU_FILL_TAIL_ROOTS",
            "RDGPU_FILL_DISSOLVE", "RDGPU_FILL_FLOODED", "RDGPU_FILL_COUNT_FLOODED")
_ORACLE = {}
_MODEL = {}


def _oracle(orc, key, z, topo):
    if (key, topo) not in _ORACLE:
        exp = orc.port.fill(z, topo)
        exp.setflags(write=False)
        _ORACLE[(key, topo)] = exp
    return _ORACLE[(key, topo)]


def _model(key, z, topo, dissolve=True):
    """(boundary cells per pair tile, nodes per descent tile, basin of every cell), once per raster and topology"""
    if (key, topo, dissolve) not in _MODEL:
        ptr, lab = pmod.forest(z, topo, dissolve)
        _MODEL[(key, topo, dissolve)] = (pmod.boundary_cells(lab, topo), pmod.nodes(ptr, z.shape), lab)
    return _MODEL[(key, topo, dissolve)]


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got.view(np.uint8) != exp.view(np.uint8)).reshape(got.shape + (-1,)).any(axis=-1).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:8].tolist())


def _dev(rd, z, topo, own_stream=False):
    import torch

    t = torch.from_numpy(z).cuda()
    if own_stream:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            rd.fill_depressions_dev(t, topology=topo)
        st.synchronize()
    else:
        rd.fill_depressions_dev(t, topology=topo)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _check(rd, orc, monkeypatch, capfd, key, z, topo, entry="host", dissolve=True):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RDGPU_FILL_DEBUG", "1")
    if not dissolve:
        monkeypatch.setenv("RDGPU_FILL_DISSOLVE", "0")
    keep = z.copy()
    exp = _oracle(orc, key, z, topo)
    what = f"{key} D{topo} {entry}"
    capfd.readouterr()
    if entry == "host":
        got = rd.FillDepressions(z, topology=topo)
    else:
        got = _dev(rd, z, topo, own_stream=entry == "stream")
    st = rd.fill_stats()
    err = capfd.readouterr().err
    assert not any(m in err for m in FALLBACKS), (what, err)          # the compact path ran to its end
    assert st["host_syncs"] == 2 and st["basins"] > 0, (what, st)
    _same(got, exp, what)
    assert np.array_equal(z.view(np.uint8), keep.view(np.uint8))


@pytest.mark.parametrize("topo", [8, 4])
def test_band_passes_on_small_basins(rd, orc, monkeypatch, capfd, topo):
    z = pmod.small_basins()
    assert z.shape == (70, 130)
    bc, nd, _ = _model("small basins", z, topo)
    print("boundary cells per pair tile:", bc.tolist(), "nodes per descent tile:", nd.tolist())
    assert bc.max() > 1024 and bc.max() > pmod.LIST_CAP              # more than the list holds: one pass per band
    assert bc.min() <= pmod.LIST_CAP                                 # and tiles listed at once beside it
    assert nd.max() <= pmod.NT_CAP                                   # every node table staged in LDS
    _check(rd, orc, monkeypatch, capfd, "small basins", z, topo)


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("cells", [pmod.LIST_CAP, 1024])
def test_the_list_cap_exactly_and_one_more(rd, orc, monkeypatch, capfd, cells, topo):
    g = pmod.golden()
    a, b = g[f"d{topo}_{cells}"], g[f"d{topo}_{cells + 1}"]
    assert int((a.view(np.uint32) != b.view(np.uint32)).sum()) == 1   # the same raster with one cell changed
    for z, n in ((a, cells), (b, cells + 1)):
        bc, nd, _ = _model(f"cap {n}", z, topo)
        assert bc[0, 0] == n == bc.max(), (n, bc.tolist())
        assert nd.max() <= pmod.NT_CAP, nd.tolist()
        for other in (8, 4):                                          # (the other topology: checked against the oracle as well)
            _check(rd, orc, monkeypatch, capfd, f"cap {n} for D{topo}", z, other)


def test_node_table_past_nt_cap_is_gathered(rd, orc, monkeypatch, capfd):
    z = fm.many_nodes()
    _, nd, _ = _model("many nodes", z, 4, dissolve=False)
    print("nodes per descent tile:", nd.tolist())
    assert pmod.NT_CAP < nd[1, 1] <= 1024, nd.tolist()               # staged in LDS before, gathered now
    assert fm.pits_in_centre_d4(z) > pmod.NT_CAP
    assert np.delete(nd.ravel(), 4).max() <= pmod.NT_CAP             # the tiles around it: staged
    _check(rd, orc, monkeypatch, capfd, "many nodes", z, 4, dissolve=False)


@pytest.mark.parametrize("topo", [8, 4])
def test_ring_crossings(rd, orc, monkeypatch, capfd, topo):
    z = pmod.ring_crossings()
    h, w = z.shape
    assert w % 64 and h % 32
    if topo == 8:                                                     # (the chains are 8-connected: under D4 their cells are
        _, _, lab = _model("ring crossings", z, 8)                    # pits of their own, and the case is the oracle's alone)
        for name, cells in pmod.CROSSINGS.items():
            a, b = cells[1], cells[2]
            assert (a[0] // 32, a[1] // 64) != (b[0] // 32, b[1] // 64), name          # a | b lies across a tile edge
            assert pmod.low_pass_only_at(z, lab, a, b), name
    _check(rd, orc, monkeypatch, capfd, "ring crossings", z, topo)


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("entry", ["host", "dev", "stream"])
@pytest.mark.parametrize("seed", [3, 11])
def test_fractal(rd, orc, monkeypatch, capfd, seed, entry, topo):
    _check(rd, orc, monkeypatch, capfd, f"fractal 520x390 s{seed}", fractal_dem(520, 390, seed), topo, entry=entry)
