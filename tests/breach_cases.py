"""The input rasters of the breaching tests, by name: make_golden_breach.py runs the compiled reference on them and stores its
outputs in tests/golden/ref_breach.npz; the tests rebuild the inputs here.  Every case is small and aims at one way the
kernels can go wrong; the tiles of the engine are 64 x 64."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from richdem_amd.synth import fractal_dem  # noqa: E402

SIZES = ((97, 70), (130, 129), (257, 259))          # (width, height): breach paths cross tile edges and corners at 64, 128
SUFFIX = {"uint8": "u8", "int8": "i8", "uint16": "u16", "int16": "i16", "uint32": "u32", "int32": "i32", "float32": "f32"}
TYPES = tuple(np.dtype(k) for k in SUFFIX)
WALL = 1.0e6


def _lake(q, lo, hi):
    """a flat-bottomed lake behind a closed rim across the tile corner at (64, 64)"""
    if q.shape[0] > 75 and q.shape[1] > 75:
        q[56:73, 56:73] = hi
        q[58:71, 58:71] = lo
    return q


def quantised(w, h, dtype, levels, offset=0):
    """the fractal DEM of that size in `levels` steps from `offset`: ties in every tile, flat-bottomed lakes"""
    z = fractal_dem(w, h, 4100 + w).astype(np.float64)
    q = np.minimum(levels - 1, np.floor((z - z.min()) / (z.max() - z.min()) * levels)).astype(np.int64) + offset
    return _lake(q, offset, offset + levels - 1).astype(dtype)


def corridor(w=257, h=259, low=None):
    """A walled serpentine corridor, one cell wide, along the odd rows: it RISES from the raster's edge at (0, 1) to a flat
    two-cell pit at its inner end that is lower than all of it, so one walk carves the whole corridor: more links than a tile
    holds cells.  Walls are pairwise distinct and above everything.  low: a fraction of the way from the pit back to the
    edge where two cells are lower than the pit, so that the pit's walk stops there."""
    dem = (WALL + np.arange(w * h, dtype=np.float64).reshape(h, w)).astype(np.float32)
    cells = []
    rows = list(range(1, h - 1, 2))
    for k, y in enumerate(rows):
        xs = range(0 if k == 0 else 1, w - 1) if k % 2 == 0 else range(w - 2, 0, -1)
        cells += [(y, x) for x in xs]
        if k + 1 < len(rows):
            cells.append((y + 1, w - 2 if k % 2 == 0 else 1))
    for i, (y, x) in enumerate(cells):
        dem[y, x] = 100.0 + i
    for y, x in cells[-2:]:
        dem[y, x] = 50.0
    if low is not None:
        i = int(len(cells) * (1.0 - low))
        for y, x in cells[i:i + 2]:
            dem[y, x] = 7.0
    return dem, len(cells)


def nested():
    """a bowl with a second, deeper bowl inside it: the inner pit's walk is absorbed by the outer one's path"""
    y, x = np.mgrid[0:40, 0:48]
    dem = (np.hypot(x - 30, y - 20) * 4).astype(np.int32) + 100          # a cone towards (30, 20) ...
    dem[:, :3] += 300                                                      # ... behind a high west side
    dem = np.minimum(dem, 100 + 4 * 14)                                    # a plateau round it
    dem[:, 47] = 90                                                        # the way out: east
    dem[18:23, 28:33] = np.array([[60, 60, 60, 60, 60], [60, 40, 40, 40, 60], [60, 40, 10, 40, 60], [60, 40, 40, 40, 60],
                                  [60, 60, 60, 60, 60]])
    dem[20, 30:32] = 10
    return dem.astype(np.int32)


def equal_pits():
    """two flat pits of one level in different tiles on one walled channel that leaves the raster at (0, 10)"""
    dem = np.full((21, 140), 500, np.int16)
    dem[10, :139] = 50
    dem[10, 20:22] = 20
    dem[10, 130:132] = 20
    return dem


def extremes(dtype):
    """the type's minimum and maximum at a pit and on a path: a channel through a plateau of the type's maximum (whose interior
    cells are pits at that level); f32: -inf and +inf, and zeros of both signs along the channel"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        lo, hi, mid = -np.inf, np.inf, 1.5
    else:
        lo, hi = np.iinfo(dtype).min, np.iinfo(dtype).max
        mid = lo // 2 + hi // 2
    dem = np.full((12, 70), hi, dtype)
    dem[5, :66] = mid
    dem[5, 3:5] = lo
    dem[5, 30:32] = lo
    dem[5, 64:66] = lo
    dem[8, 0:40] = mid           # a second channel whose pit holds the plateau's level: the maximum on a path
    dem[8, 38:40] = hi
    if dtype.kind == "f":
        dem[5, 10:14] = [0.0, -0.0, 0.0, -0.0]
        dem[5, 40:42] = -0.0
        dem[2, 5:9] = np.finfo(np.float32).max
    return dem


def tilted(w=40, h=30):
    y, x = np.mgrid[0:h, 0:w]
    return (3 * x + 5 * y).astype(np.float32)


def _build():
    c = {}
    for w, h in SIZES:
        c[f"frac_f32_{w}x{h}"] = lambda w=w, h=h: fractal_dem(w, h, 4100 + w)
        c[f"q_u8_{w}x{h}"] = lambda w=w, h=h: quantised(w, h, np.uint8, 8)
        c[f"q_i16_{w}x{h}"] = lambda w=w, h=h: quantised(w, h, np.int16, 60, -30)
        c[f"q_u16_{w}x{h}"] = lambda w=w, h=h: quantised(w, h, np.uint16, 40, 65000)
    c["q_i8_97x70"] = lambda: quantised(97, 70, np.int8, 12, -6)
    c["q_i32_97x70"] = lambda: quantised(97, 70, np.int32, 25, -2000000000)
    c["q_u32_97x70"] = lambda: quantised(97, 70, np.uint32, 25, 4000000000)
    c["corridor_f32"] = lambda: corridor()[0]
    c["corridor_low_f32"] = lambda: corridor(low=2.0 / 3.0)[0]
    c["nested_i32"] = nested
    c["equal_pits_i16"] = equal_pits
    for t in TYPES:
        c[f"extremes_{SUFFIX[t.name]}"] = lambda t=t: extremes(t)
    c["one_f32_1x1"] = lambda: np.array([[3.0]], np.float32)
    c["thin_i16_2x5"] = lambda: np.array([[5, 1, 5, 1, 5], [5, 5, 5, 5, 5]], np.int16).T.copy()
    c["pit_u8_3x3"] = lambda: np.array([[9, 9, 9], [9, 1, 9], [9, 8, 9]], np.uint8)
    c["tilted_f32_40x30"] = tilted
    return c


CASES = _build()


def plateau_depth(dem):
    """the largest number of breadth-first rings (8-connected) from a cell to the nearest cell of another value or to the
    raster's edge: what bounds the passes of the tie order"""
    h, w = dem.shape
    inside = np.ones((h, w), bool)
    depth = 0
    while True:
        p = np.pad(dem, 1, mode="edge")
        m = np.pad(inside, 1, mode="constant", constant_values=False)
        keep = inside.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    keep &= (p[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] == dem) & m[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
        if not keep.any():
            return depth
        inside = keep
        depth += 1
