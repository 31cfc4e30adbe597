"""A plain numpy / Python model of the depression inventory (include/rdgpu.h, "depression inventory"), and the small
rasters the CPU and GPU tests share.

Given the DEM and its filled surface W (``orc.port.fill``), a cell is raised iff W > dem; a depression is a connected
component of the raised cells under the topology.  Labels are numbered by ascending lowest raster index; the table
follows the contract field by field, with ``math.fsum`` for the volume.
"""
import math

import numpy as np

DEPRESSION_DTYPE = np.dtype([("first_cell", np.uint32), ("pit_cell", np.uint32), ("outlet_cell", np.uint32), ("cells", np.uint32),
                             ("level", np.float64), ("pit_elevation", np.float64), ("volume", np.float64)])

_N8 = ((-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1))   # (dx, dy)
_N4 = ((-1, 0), (0, -1), (1, 0), (0, 1))


def _find(par, x):
    while par[x] != x:
        par[x] = par[par[x]]
        x = par[x]
    return x


def depressions_from_fill(dem: np.ndarray, filled: np.ndarray, topo: int = 8):
    """(labels int32 [h, w], table DEPRESSION_DTYPE [N]) of ``dem`` whose filled surface is ``filled``."""
    assert dem.shape == filled.shape and dem.ndim == 2 and topo in (8, 4)
    h, w = dem.shape
    nbrs = _N8 if topo == 8 else _N4
    raised = (filled > dem).ravel()
    z = dem.ravel()
    wf = filled.ravel()
    n = h * w
    par = list(range(n))
    cells = np.flatnonzero(raised)
    for c in cells:
        c = int(c)
        x, y = c % w, c // w
        for dx, dy in nbrs:
            xx, yy = x + dx, y + dy
            if 0 <= xx < w and 0 <= yy < h:
                q = yy * w + xx
                if raised[q]:
                    a, b = _find(par, c), _find(par, q)
                    if a != b:
                        par[max(a, b)] = min(a, b)
    labels = np.zeros(n, np.int32)
    ids = {}
    members = []
    for c in cells:   # ascending raster order: a new root met here is the depression with the next lowest first cell
        c = int(c)
        r = _find(par, c)
        if r not in ids:
            ids[r] = len(members)
            members.append([])
        members[ids[r]].append(c)
        labels[c] = ids[r] + 1
    table = np.zeros(len(members), DEPRESSION_DTYPE)
    outlet = [None] * len(members)
    for c in np.flatnonzero(~raised):
        c = int(c)
        x, y = c % w, c // w
        for dx, dy in nbrs:
            xx, yy = x + dx, y + dy
            if 0 <= xx < w and 0 <= yy < h:
                q = yy * w + xx
                if raised[q] and wf[q] == z[c]:
                    i = labels[q] - 1
                    if outlet[i] is None or c < outlet[i]:
                        outlet[i] = c
    integer = np.issubdtype(dem.dtype, np.integer)
    for i, m in enumerate(members):
        assert outlet[i] is not None, "the flood enters every depression from a cell at its level"
        pit = min(m, key=lambda c: (z[c], c))
        lvl = z[outlet[i]]
        assert all(wf[c] == lvl for c in m)
        if integer:
            vol = float(sum(int(lvl) - int(z[c]) for c in m))
        else:
            vol = math.fsum(float(lvl) - float(z[c]) for c in m)
        table[i] = (m[0], pit, outlet[i], len(m), float(lvl), float(z[pit]), vol)
    return labels.reshape(h, w), table


def depressions_model(orc, dem: np.ndarray, topo: int = 8):
    dem = np.ascontiguousarray(dem)
    return depressions_from_fill(dem, orc.port.fill(dem, topo), topo)


def compare(got_labels, got_table, exp_labels, exp_table, dtype):
    """Integer element types: everything equal.  Floating point: everything equal but the volume, for which
    |v - fsum| <= cells * 2^-52 * fsum (every term is non-negative and costs one rounding of at most 2^-53 relative; a
    sum of `cells` non-negative terms in any order adds at most (cells - 1) * 2^-53)."""
    assert len(got_table) == len(exp_table), (len(got_table), len(exp_table))
    if got_labels is not None:
        assert got_labels.dtype == np.int32 and np.array_equal(got_labels, exp_labels)
    for f in ("first_cell", "pit_cell", "outlet_cell", "cells", "level", "pit_elevation"):
        assert np.array_equal(got_table[f], exp_table[f]), f
    if np.issubdtype(np.dtype(dtype), np.integer):
        assert np.array_equal(got_table["volume"], exp_table["volume"])
    else:
        err = np.abs(got_table["volume"] - exp_table["volume"])
        bound = exp_table["cells"].astype(np.float64) * 2.0 ** -52 * exp_table["volume"]
        print("volume: largest error / bound =", float((err / np.maximum(bound, 1e-300)).max()) if len(err) else 0.0)
        assert (err <= bound).all()


# ---- the hand-written rasters (values 0..9: every element type holds them) ------------------------------------------
HAND = {
    "single_pit": [[5, 5, 5],
                   [5, 1, 5],
                   [5, 5, 5]],
    "diagonal_pits": [[9, 9, 9, 9],
                      [9, 1, 9, 9],
                      [9, 9, 2, 9],
                      [9, 9, 9, 9]],
    "nested_pit": [[9, 9, 9, 9, 9, 9, 9],
                   [9, 4, 4, 4, 4, 4, 9],
                   [9, 4, 2, 4, 1, 4, 9],
                   [9, 4, 4, 4, 4, 4, 9],
                   [9, 9, 9, 9, 9, 9, 9]],
    "equal_lowest": [[7, 7, 7, 7],
                     [7, 2, 2, 7],
                     [7, 7, 7, 7]],
    "two_rim_cells": [[9, 9, 9, 9, 9],
                      [5, 3, 3, 3, 5],
                      [9, 9, 9, 9, 9]],
    "flat": [[3, 3, 3, 3]] * 4,
    "cascade": [[9, 9, 9, 9, 9, 9, 9],
                [9, 2, 6, 1, 9, 9, 9],
                [9, 9, 9, 4, 9, 9, 9]],
}
DTYPES = (np.uint8, np.int8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64)


def lake_row(dtype=np.int32):
    """67 x 5 (w x h): one lake along the middle row that crosses the 64-lane boundary of a row segment."""
    z = np.full((5, 67), 50, dtype)
    z[2, 1:66] = 10 + (np.arange(65) % 7)
    z[2, 66] = 30   # the rim's lowest cell: the lake stands at 30
    return z


def rough_bowl(dtype=np.int32, seed=5):
    """130 x 70 (w x h): a wide shallow bowl with a rough bottom -- one lake over several row segments and fill tiles,
    made of many basins of the descent forest."""
    rng = np.random.default_rng(seed)
    z = np.full((70, 130), 100, dtype)
    z[1:-1, 1:-1] = (40 + rng.integers(0, 8, (68, 128))).astype(dtype)
    z[33, 0] = 60   # the spill
    return z
