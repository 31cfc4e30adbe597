"""Flooded tiles in the compact fill's finalize (k_descent16 / k_finalize16, csrc/fill.hip).

The descent leaves every tile's largest key; the finalize stages a tile's node levels first and, when they are one level
strictly above that key, writes the level to the whole tile without loading its elevations or labels.  Every case below
is checked for three things:

* the output equals the CPU oracle's fill cell for cell, bits included;
* it equals, bit for bit, the same call under RDGPU_FILL_FLOODED=0 (every tile read, as before);
* under RDGPU_FILL_COUNT_FLOODED=1 `fill_flooded_tiles()` equals the census of the oracle's output
  (flooded_tiles_model.flooded_tiles): the path is taken, and only where it may be.  Switched off, the count is 0.

`host_syncs` stays 2 throughout.  The rasters (flooded_tiles_model.py) and what each is for:

  bowl              192 x 192, low relief inside a wall of 10 two cells in from the border: the centre tile is flooded
  island above      one cell of the centre tile at 11: the tile takes the general path, the count drops to 0
  island at level   that cell at exactly 10.0: strictly above fails, the tile is read, the cell keeps its bits
  minus zero        a lake at +0.0 over cells at -0.0 in the centre tile: their sign bits stay
  many nodes        white noise under the wall, D4 and no dissolving: more than 256 nodes in the centre tile -- the strided
                    level loop and the reduction across the block
  dissolved pits    the diagonal-pit plane under a wall: dissolved pits inside a flooded tile
  width 198         two interior flooded tiles on the scalar store path; and a 192-wide raster whose base is off by one element
  ragged            150 x 133 under one lake, a cell above the level in the only tile inside the raster's border ring: no tile
                    is flooded, the partial tiles keep their values
  ragged flooded    the same without that cell: one flooded tile beside partial ones, odd width
  two lakes         lakes at 10 and 20 whose shared wall runs down the centre tile: mixed beside tiles flooded at different levels
  bowl <type>       every element type the plain fill is instantiated for: Key32<T>::from of the level
  fractal           520 x 390 and 1030 x 770, seeds 3 and 11: the count equals the census (which may be 0)
  stream            the device entry on a stream of its own"""
import numpy as np
import pytest

import flooded_tiles_model as fm
from richdem_amd.synth import fractal_dem

pytestmark = pytest.mark.gpu

FALLBACKS = ("node table overflow", "hook chain unfinished", "pair list overflow")
SWITCHES = ("RDGPU_DEVICES", "RDGPU_FILL_EDGES", "RDGPU_FILL_EDGE_CAP", "RDGPU_FILL_ROUND_BATCH", "RDGPU_FILL_TAIL_ROOTS",
            "RDGPU_FILL_DISSOLVE", "RDGPU_FILL_FLOODED", "RDGPU_FILL_COUNT_FLOODED")
RASTERS = fm.rasters()
_ORACLE = {}


def _oracle(orc, key, z, topo):
    """(oracle's fill, census of flooded tiles), once per raster and topology, never written to"""
    if (key, topo) not in _ORACLE:
        exp = orc.port.fill(z, topo)
        exp.setflags(write=False)
        _ORACLE[(key, topo)] = (exp, fm.flooded_tiles(z, exp))
    return _ORACLE[(key, topo)]


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got.view(np.uint8) != exp.view(np.uint8)).reshape(got.shape + (-1,)).any(axis=-1).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:8].tolist())


def _host(rd, z, topo):
    return rd.FillDepressions(z, topology=topo)


def _dev(rd, z, topo, offset=0, own_stream=False):
    """the device entry; offset: the raster's first element lies `offset` elements into an aligned allocation"""
    import torch

    flat = torch.zeros(z.size + offset, dtype=torch.from_numpy(z[:1, :1]).dtype, device="cuda")
    t = flat[offset:].view(z.shape)
    t.copy_(torch.from_numpy(z))
    assert t.is_contiguous() and (t.data_ptr() - flat.data_ptr()) == offset * z.itemsize
    if own_stream:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            rd.fill_depressions_dev(t, topology=topo)
            n = rd.fill_flooded_tiles()
        st.synchronize()
    else:
        rd.fill_depressions_dev(t, topology=topo)
        n = rd.fill_flooded_tiles()
    torch.cuda.synchronize()
    return t.cpu().numpy(), n


def _check(rd, orc, monkeypatch, capfd, key, z, topo, entry="host", dissolve=True, **kw):
    """the three checks of one raster through one entry; returns the census"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RDGPU_FILL_DEBUG", "1")
    if not dissolve:
        monkeypatch.setenv("RDGPU_FILL_DISSOLVE", "0")
    keep = z.copy()
    exp, census = _oracle(orc, key, z, topo)
    what = f"{key} D{topo} {entry}"

    def run():
        capfd.readouterr()
        if entry == "host":
            got = _host(rd, z, topo)
            n = rd.fill_flooded_tiles()
        else:
            got, n = _dev(rd, z, topo, **kw)
        st = rd.fill_stats()
        err = capfd.readouterr().err
        assert not any(m in err for m in FALLBACKS), (what, err)
        assert st["host_syncs"] == 2, (what, st)
        return got, n

    got, n_uncounted = run()                                   # as shipped: no counter
    _same(got, exp, what)
    assert n_uncounted == 0, (what, n_uncounted)
    monkeypatch.setenv("RDGPU_FILL_COUNT_FLOODED", "1")
    got1, n = run()
    print(what, "flooded tiles:", n, "census:", census)
    _same(got1, exp, what + ", counted")
    assert n == census, (what, n, census)
    monkeypatch.setenv("RDGPU_FILL_FLOODED", "0")
    got0, n0 = run()
    _same(got0, got, what + ", switched off")                  # bit for bit what the fast path wrote
    _same(got0, exp, what + ", switched off, oracle")
    assert n0 == 0, (what, n0)
    assert np.array_equal(z.view(np.uint8), keep.view(np.uint8))
    return census


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", list(RASTERS))
def test_flooded_tiles_equal_the_oracle_and_the_census(rd, orc, monkeypatch, capfd, name, topo):
    census = _check(rd, orc, monkeypatch, capfd, name, RASTERS[name], topo)
    assert census == fm.EXPECTED[name], (name, topo, census)


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", ["bowl", "island at level", "minus zero", "width 198"])
def test_flooded_tiles_device_entry(rd, orc, monkeypatch, capfd, name, topo):
    census = _check(rd, orc, monkeypatch, capfd, name, RASTERS[name], topo, entry="dev")
    assert census == fm.EXPECTED[name]


def test_flooded_tiles_many_nodes_without_dissolving(rd, orc, monkeypatch, capfd):
    z = RASTERS["many nodes"]
    assert fm.pits_in_centre_d4(z) > 256                       # every one a node of the centre tile: the loop strides
    assert _check(rd, orc, monkeypatch, capfd, "many nodes", z, 4, dissolve=False) == 1


@pytest.mark.parametrize("name", ["bowl", "dissolved pits"])
def test_flooded_tiles_unaligned_base(rd, orc, monkeypatch, capfd, name):
    """192 wide, but the first element one past an aligned address: the scalar loads and stores"""
    assert _check(rd, orc, monkeypatch, capfd, name, RASTERS[name], 8, entry="dev", offset=1) == 1


def test_flooded_tiles_on_a_stream_of_its_own(rd, orc, monkeypatch, capfd):
    assert _check(rd, orc, monkeypatch, capfd, "two lakes", RASTERS["two lakes"], 8, entry="dev", own_stream=True) == 2


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("whs", fm.FRACTALS, ids=lambda c: f"{c[0]}x{c[1]}s{c[2]}")
def test_flooded_tiles_fractal(rd, orc, monkeypatch, capfd, whs, topo):
    w, h, seed = whs
    _check(rd, orc, monkeypatch, capfd, f"fractal {whs}", fractal_dem(w, h, seed), topo)
