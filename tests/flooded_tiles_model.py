"""Flooded tiles of the fill's finalize (k_finalize16, csrc/fill.hip): the census the engine's
counter is checked against, and the rasters of test_fill_flooded_tiles_model.py / test_fill_flooded_tiles_gpu.py.

A 64 x 64 descent tile that lies wholly in the raster and in which every cell is strictly raised comes out at one level:
two adjacent strictly raised cells have the same filled value (were W(a) < W(b), the path b -> a -> a's way out would have
maximum W(a) < W(b), against W(b) being b's minimax), and a tile's cells are connected.  The finalize writes such a tile
without reading it."""
import numpy as np

import pit_dissolve_model as pm
from richdem_amd.synth import fractal_dem

T = 64


def tiles_inside(shape, T=T):
    """(y0, x0) of the T x T tiles of the grid anchored at (0, 0) that lie wholly in the raster"""
    h, w = shape
    return [(y0, x0) for y0 in range(0, h - T + 1, T) for x0 in range(0, w - T + 1, T)]


def flooded_tiles(z, W, T=T):
    """the number of T x T tiles lying wholly in the raster in which W > z everywhere"""
    return sum(1 for y0, x0 in tiles_inside(z.shape, T) if (W[y0:y0 + T, x0:x0 + T] > z[y0:y0 + T, x0:x0 + T]).all())


def flooded_levels(z, W, T=T):
    """[(y0, x0, min W, max W)] of those tiles: min == max is the fact the engine's fast path rests on"""
    out = []
    for y0, x0 in tiles_inside(z.shape, T):
        a, b = z[y0:y0 + T, x0:x0 + T], W[y0:y0 + T, x0:x0 + T]
        if (b > a).all():
            out.append((y0, x0, b.min(), b.max()))
    return out


# ---- the rasters ------------------------------------------------------------------------------------------------------

def _smooth(h, w, seed):
    """low relief in [0, 1): a fractal surface squeezed under any wall"""
    f = fractal_dem(w, h, seed).astype(np.float64)
    f = (f - f.min()) / max(float(f.max() - f.min()), 1e-30)
    return (f * 0.875).astype(np.float32)


def wall(z, level, inset=2):
    """a closed wall of height `level`, `inset` cells in from the raster's border, laid over z (in place)"""
    h, w = z.shape
    a, b, c, d = inset, h - 1 - inset, inset, w - 1 - inset
    z[a, c:d + 1] = level
    z[b, c:d + 1] = level
    z[a:b + 1, c] = level
    z[a:b + 1, d] = level
    return z


def bowl(h=192, w=192, level=10.0, seed=2):
    """low relief inside a wall two cells in from the border: everything inside the wall floods to `level`"""
    return wall(_smooth(h, w, seed), np.float32(level))


def island(value, h=192, w=192):
    """the bowl with one cell of the centre tile at `value`"""
    z = bowl(h, w)
    z[h // 2, w // 2] = value
    return z


def ragged():
    """150 rows of 133 under one lake: the only tile inside the raster's border ring, (64, 64), holds a cell above the
    level; every other tile, flooded as it is, holds border cells or hangs over the raster's end"""
    z = bowl(150, 133)
    z[96, 96] = 11
    return z


def minus_zero():
    """a bowl whose level is +0.0 (the wall), relief below it, and cells of the centre tile at -0.0: level with the lake,
    not raised, and their sign bit stays"""
    z = _smooth(192, 192, 2) - np.float32(2.0)
    z[:2, :] -= 4
    z[-2:, :] -= 4
    z[:, :2] -= 4
    z[:, -2:] -= 4
    wall(z, np.float32(0.0))
    for y, x in ((70, 70), (96, 97), (127, 64), (100, 100), (100, 101)):
        z[y, x] = np.float32(-0.0)
    assert np.signbit(z[96, 97]) and not np.signbit(z[2, 2])
    return z


def many_nodes(seed=9):
    """white noise in and around the centre tile under the wall: every few cells a pit of its own"""
    z = bowl()
    rng = np.random.default_rng(seed)
    z[58:134, 58:134] = rng.random((76, 76), dtype=np.float32)
    return z


def pits_in_centre_d4(z):
    """strict D4 minima in the centre tile of a 192 x 192 raster: nodes of that tile when no pit dissolves"""
    c = z[64:128, 64:128]
    return int(((c < z[63:127, 64:128]) & (c < z[65:129, 64:128]) & (c < z[64:128, 63:127]) & (c < z[64:128, 65:129])).sum())


def dissolved_under_wall():
    """the diagonal-pit plane (pit_dissolve_model) under a wall above its highest cell: dissolved pits in a flooded tile"""
    z = pm.diagonal_pits(192, 192)
    return wall(z, np.float32(2000.0))


def two_lakes():
    """192 x 320, five tiles across: a lake at 10 on the left and one at 20 on the right; their shared wall (30) runs down
    the centre tile, which is mixed; the interior tiles on either side flood at different levels"""
    h, w = 192, 320
    z = _smooth(h, w, 5)
    wall(z, np.float32(10.0))
    z[2, 160:w - 2] = 20
    z[h - 3, 160:w - 2] = 20
    z[2:h - 2, w - 3] = 20
    z[2:h - 2, 160] = 30
    return z


INT_TYPES = (np.uint8, np.int8, np.int16, np.uint16, np.int32, np.uint32)


def typed_bowl(dtype):
    """the bowl in an integer type: relief 0..39 (plateaus) under a wall of 60; signed types 90 lower, below zero throughout"""
    z = np.floor(_smooth(192, 192, 4).astype(np.float64) * 45.0).astype(np.int64)
    wall(z, 60)
    if np.issubdtype(dtype, np.signedinteger):
        z -= 90
    return z.astype(dtype)


def rasters():
    """name -> raster, every case of the two test files (the fractals apart)"""
    d = {
        "bowl": bowl(),
        "island above": island(np.float32(11.0)),
        "island at level": island(np.float32(10.0)),
        "minus zero": minus_zero(),
        "many nodes": many_nodes(),
        "dissolved pits": dissolved_under_wall(),
        "width 198": bowl(192, 198),
        "ragged": ragged(),
        "ragged flooded": bowl(150, 133),
        "two lakes": two_lakes(),
    }
    for t in INT_TYPES:
        d["bowl " + np.dtype(t).name] = typed_bowl(t)
    return d


# flooded tiles each raster must show (D8 and D4 alike); the fractals' counts are whatever the census says
EXPECTED = {"bowl": 1, "island above": 0, "island at level": 0, "minus zero": 0, "many nodes": 1, "dissolved pits": 1,
            "width 198": 2, "ragged": 0, "ragged flooded": 1, "two lakes": 2, **{"bowl " + np.dtype(t).name: 1 for t in INT_TYPES}}

FRACTALS = [(520, 390, 3), (520, 390, 11), (1030, 770, 3), (1030, 770, 11)]   # (width, height, seed)
