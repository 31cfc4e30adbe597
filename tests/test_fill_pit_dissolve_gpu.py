"""Dissolved pits in the compact fill (k_descent16 / k_pairs16 / k_resolve_nodes / k_finalize16, csrc/fill.hip; DESIGN.md
section 3a) against the CPU oracle's fill, exact and over every cell, under D8 and D4.

A pit whose lowest neighbour q lies in its 64 x 64 descent tile and does not drain into it gets no basin: it points at q,
its label carries a flag and q's direction, and the finalize raises it alone to max(key(q), level).  For every raster:

* both entries (host pointer, HBM-resident tensor) equal the oracle bytewise;
* the engine's `dissolved_pits` is the count of the numpy model (pit_dissolve_model.py, itself checked against the oracle in
  test_fill_pit_dissolve_model.py) under the same tile restriction, and `basins` stays the pits of the descent forest;
* with RDGPU_FILL_DISSOLVE=0 nothing dissolves and the surface is the same.

The rasters, and what each is for:

  fractal 257 wide x 300 (seed 3), f32   width no multiple of 4: the kernels' unaligned instantiations, edge tiles
  fractal 256 wide x 192                 interior tiles, the vector path
  the diagonal-pit plane, 130 x 130      chains p -> q -> r -> p2 across rows, quads and wavefronts' row blocks; pits on a
                                         tile's last row / column (q inside) and first row / column (q outside: they stay);
                                         pits beside the raster's border; under D8 no basin at all is left in tile (0, 0)
  floor(fractal * 0.05), i32 and i16     ties: plateaus, pits level with their q
  random {0..2}, i32, 50 x 40            dense ties
  fractal + an irrational offset, f64    not representable in f32: the 64-bit route over dense ranks (u32 engine)
  one pit beside the border, 9 x 7       nothing but a dissolved pit: no basin, no table, no round -- the finalize alone

Candidates on a tile's ring (first or last row or column of a 64 x 64 tile), counted by the model and asserted below: the
fractals (f32 and f64), the plane and the plateau rasters hold some whose q lies inside the tile; the fractals and the
plane also some whose q lies outside it (the plane: 42 under D8, 22 under D4), which stay pits."""
import numpy as np
import pytest

import pit_dissolve_model as pm
from richdem_amd.synth import fractal_dem, fractal_dem_int

pytestmark = pytest.mark.gpu

FALLBACKS = ("node table overflow", "hook chain unfinished", "pair list overflow")


def _f64():
    z = fractal_dem(150, 100, 4).astype(np.float64) + np.pi * 1e-7
    assert (z.astype(np.float32).astype(np.float64) != z).any()            # the rank route, not the f32 engine
    return z


def _dems():
    rng = np.random.default_rng(5)
    return {
        "fractal 257w": fractal_dem(257, 300, 3),
        "fractal 256w": fractal_dem(256, 192, 3),
        "diagonal pits": pm.diagonal_pits(130, 130),
        "plateaus i32": fractal_dem_int(200, 150, 3, 0.05),
        "plateaus i16": fractal_dem_int(200, 150, 3, 0.05, dtype=np.int16),
        "integers 0..2": rng.integers(0, 3, (40, 50)).astype(np.int32),
        "f64 ranks": _f64(),
        "border pit": pm.border_pit(),
    }


DEMS = _dems()
RING = ("fractal 257w", "fractal 256w", "diagonal pits", "plateaus i32", "plateaus i16", "f64 ranks")   # candidates on a tile ring, q inside
RING_OUT = ("fractal 257w", "fractal 256w", "diagonal pits", "f64 ranks")                              # ... and q outside the tile
_MODEL = {}


def _model(orc, name, topo):
    """(oracle's fill, model's info under the tile restriction), once per raster and topology, never written to"""
    if (name, topo) not in _MODEL:
        z = DEMS[name]
        exp = orc.port.fill(z, topo)
        got, info = pm.fill_dissolve(z, topo, tile=64)
        assert np.array_equal(got, exp)
        exp.setflags(write=False)
        _MODEL[(name, topo)] = (exp, info)
    return _MODEL[(name, topo)]


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got.view(np.uint8) != exp.view(np.uint8)).reshape(got.shape + (-1,)).any(axis=-1).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:8].tolist())


def _fills(rd, capfd, z, topo, what):
    """both entries' fills of z with the compact path seen to its end; (host result, device result, stats of the host's, of the device's)"""
    import torch

    capfd.readouterr()
    host = rd.FillDepressions(z, topology=topo)
    sh = rd.fill_stats()
    t = torch.from_numpy(z.copy()).cuda()
    rd.fill_depressions_dev(t, topology=topo)
    torch.cuda.synchronize()
    sd = rd.fill_stats()
    err = capfd.readouterr().err
    print(what, sh, sd)
    assert not any(m in err for m in FALLBACKS), (what, err)
    return host, t.cpu().numpy(), sh, sd


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", list(DEMS))
def test_dissolved_pits_equal_the_oracle_and_the_model(rd, orc, monkeypatch, capfd, name, topo):
    for k in ("RDGPU_DEVICES", "RDGPU_FILL_EDGES", "RDGPU_FILL_EDGE_CAP", "RDGPU_FILL_ROUND_BATCH", "RDGPU_FILL_TAIL_ROOTS",
              "RDGPU_FILL_DISSOLVE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RDGPU_FILL_DEBUG", "1")
    z = DEMS[name]
    keep = z.copy()
    exp, info = _model(orc, name, topo)
    print(name, f"D{topo}", "model:", info)
    if name in RING:
        assert info["ring_in"] > 0, info
    if name in RING_OUT:
        assert info["ring_out"] > 0, info
    if name != "integers 0..2":
        assert info["dissolved"] > 0, info
    host, dev, sh, sd = _fills(rd, capfd, z, topo, f"{name} D{topo}")
    _same(host, exp, f"{name} D{topo} host")
    _same(dev, exp, f"{name} D{topo} dev")
    for st in (sh, sd):
        assert st["dissolved_pits"] == info["dissolved"], (st, info)
        assert st["basins"] == info["pits"], (st, info)                    # the pits of the descent forest, as ever
    monkeypatch.setenv("RDGPU_FILL_DISSOLVE", "0")
    host0, dev0, sh0, sd0 = _fills(rd, capfd, z, topo, f"{name} D{topo}, switched off")
    _same(host0, exp, f"{name} D{topo} host, switched off")
    _same(dev0, exp, f"{name} D{topo} dev, switched off")
    for st in (sh0, sd0):
        assert st["dissolved_pits"] == 0 and st["basins"] == info["pits"], (st, info)
    assert np.array_equal(z, keep)


def test_fewer_pair_records_with_dissolved_pits(rd, orc, monkeypatch, capfd):
    """what the rule is for: on fractal terrain about a third of the pits dissolve, and the pair pass hands fewer records
    to the rounds"""
    for k in ("RDGPU_DEVICES", "RDGPU_FILL_EDGES", "RDGPU_FILL_EDGE_CAP", "RDGPU_FILL_DISSOLVE"):
        monkeypatch.delenv(k, raising=False)
    z = DEMS["fractal 256w"]
    rd.FillDepressions(z, topology=8)
    on = rd.fill_stats()
    monkeypatch.setenv("RDGPU_FILL_DISSOLVE", "0")
    rd.FillDepressions(z, topology=8)
    off = rd.fill_stats()
    print(on, off)
    assert on["basins"] == off["basins"] and 0 < on["dissolved_pits"] < on["basins"]
    assert 0 < on["edge_records"] < off["edge_records"]
