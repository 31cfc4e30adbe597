"""The fact the finalize's flooded-tile path rests on (k_finalize16, csrc/fill.hip), against the CPU
oracle's fill under D8 and D4: in a 64 x 64 tile that lies wholly in the raster and in which every cell is strictly
raised, the filled surface is constant.  Also pins what each raster of test_fill_flooded_tiles_gpu.py is built to show:
how many such tiles it holds (flooded_tiles_model.EXPECTED)."""
import numpy as np
import pytest

import flooded_tiles_model as fm
from richdem_amd.synth import fractal_dem

RASTERS = fm.rasters()


def flooded_tiles(z, W, T=64):
    """the number of T x T tiles lying wholly in the raster in which W > z everywhere"""
    return fm.flooded_tiles(z, W, T)


def _constant_in_flooded_tiles(z, W, what):
    lv = fm.flooded_levels(z, W)
    assert len(lv) == flooded_tiles(z, W)
    for y0, x0, lo, hi in lv:
        assert lo == hi, (what, y0, x0, lo, hi)
    return len(lv)


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", list(RASTERS))
def test_flooded_tiles_are_level(orc, name, topo):
    z = RASTERS[name]
    W = orc.port.fill(z, topo)
    n = _constant_in_flooded_tiles(z, W, f"{name} D{topo}")
    print(name, f"D{topo}", "flooded tiles:", n, "cells raised:", float((W > z).mean()))
    assert n == fm.EXPECTED[name], (name, topo, n)


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("whs", fm.FRACTALS, ids=lambda c: f"{c[0]}x{c[1]}s{c[2]}")
def test_flooded_tiles_are_level_fractal(orc, whs, topo):
    w, h, seed = whs
    z = fractal_dem(w, h, seed)
    W = orc.port.fill(z, topo)
    n = _constant_in_flooded_tiles(z, W, f"fractal {whs} D{topo}")
    print("fractal", whs, f"D{topo}", "flooded tiles:", n, "of", len(fm.tiles_inside(z.shape)))


def test_the_rasters_show_what_they_are_for(orc):
    z = RASTERS["island at level"]
    assert z[96, 96] == np.float32(10.0) and orc.port.fill(z, 8)[96, 96] == z[96, 96]       # level with the lake: not raised
    z = RASTERS["minus zero"]
    W = orc.port.fill(z, 8)
    assert np.signbit(W[96, 97]) and W[96, 96] == 0.0 and not np.signbit(W[96, 96])          # -0.0 kept beside +0.0
    z = RASTERS["many nodes"]
    assert fm.pits_in_centre_d4(z) > 256                                                     # the strided level loop
    z = RASTERS["two lakes"]
    W = orc.port.fill(z, 8)
    assert W[96, 96] == 10.0 and W[96, 224] == 20.0 and W[96, 160] == 30.0
    assert flooded_tiles(fm.bowl(), orc.port.fill(fm.bowl(), 8), T=32) > flooded_tiles(fm.bowl(), orc.port.fill(fm.bowl(), 8))
