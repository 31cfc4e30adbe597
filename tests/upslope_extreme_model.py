"""A plain Python model of the upslope extremes (include/rdgpu.h, "upslope extremes"): the keys of the contributing cells
pushed downstream in topological order (in-degrees over the links, a Kahn queue); what the queue leaves lies on direction
loops, and every cell of a loop then gets the best key among that loop's cells.  Serial, O(cells).  Keys are compared as
Python tuples (rank of the value, -cell), never as a packed word, and the rank of a float is (its value, its sign bit), not
a transformation of its bits: the model shares neither code nor tiling nor encoding with the engine.  The hand-written
rasters in tests/test_upslope_extreme_model.py pin it, and it then stands in for a reference that does not exist."""
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
MAX, MIN = 0, 1
# the reference's dx / dy tables (common/constants.hpp:44-45), index = code
OFFS = {1: (-1, 0), 2: (-1, -1), 3: (0, -1), 4: (1, -1), 5: (1, 0), 6: (1, 1), 7: (0, 1), 8: (-1, 1)}


def links(dirs, dir_nodata=255):
    """per cell (flat): participates, and the flat index of the cell its link points to (-1: its tree ends here)"""
    h, w = dirs.shape
    d = dirs.astype(np.int64)
    part = d != dir_nodata
    ys, xs = np.mgrid[0:h, 0:w]
    dx = np.zeros(9, np.int64)
    dy = np.zeros(9, np.int64)
    for c, (ox, oy) in OFFS.items():
        dx[c], dy[c] = ox, oy
    code = np.where((d >= 1) & (d <= 8), d, 0)
    tx, ty = xs + dx[code], ys + dy[code]
    ok = part & (code != 0) & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    t = np.where(ok, ty * w + tx, 0)
    ok &= part.ravel()[t]
    return part.ravel(), np.where(ok, t, -1).ravel()


def ranks(values, value_nodata, which):
    """per cell (flat): None where the cell's value does not contribute, else a tuple that is LARGER for a better value"""
    v = np.ascontiguousarray(values).ravel()
    nd = np.asarray(value_nodata, dtype=v.dtype)
    contributes = v != nd                                   # == in T: -0.0 equals a NoData of 0.0
    if v.dtype.kind == "f":
        contributes &= ~np.isnan(v)                         # a NaN never contributes
        neg = np.signbit(v).tolist()
        val = v.astype(np.float64).tolist()
        if which == MAX:                                    # -0 below +0
            r = [(x, 0 if s else 1) for x, s in zip(val, neg)]
        else:
            r = [(-x, 1 if s else 0) for x, s in zip(val, neg)]
    else:
        val = v.astype(object).tolist() if v.dtype.itemsize == 8 else v.tolist()
        r = [(x, 0) for x in val] if which == MAX else [(-x, 0) for x in val]
    return [k if c else None for k, c in zip(r, contributes.tolist())]


def upslope_extreme(dirs, values, value_nodata, which=MAX, dir_nodata=255):
    """{"extreme": values' dtype, "at_cell": uint32}, both [h, w]"""
    assert which in (MAX, MIN) and values.shape == dirs.shape
    h, w = dirs.shape
    n = h * w
    part, link = links(dirs, dir_nodata)
    part, link = part.tolist(), link.tolist()
    rk = ranks(values, value_nodata, which)
    key = [(rk[c] + (-c,)) if part[c] and rk[c] is not None else None for c in range(n)]
    indeg = [0] * n
    for c in range(n):
        if link[c] >= 0:
            indeg[link[c]] += 1
    queue = deque(c for c in range(n) if part[c] and indeg[c] == 0)
    done = [not p for p in part]
    while queue:
        c = queue.popleft()
        done[c] = True
        t = link[c]
        if t < 0:
            continue
        if key[c] is not None and (key[t] is None or key[c] > key[t]):
            key[t] = key[c]
        indeg[t] -= 1
        if indeg[t] == 0:
            queue.append(t)
    for c in range(n):                                       # what the queue has left lies on loops
        if done[c]:
            continue
        loop, x = [], c
        while not done[x]:
            done[x] = True
            loop.append(x)
            x = link[x]
        assert x == c
        best = None
        for x in loop:
            if key[x] is not None and (best is None or key[x] > best):
                best = key[x]
        for x in loop:
            key[x] = best
    at = np.array([NONE if k is None else -k[-1] for k in key], np.uint32)
    v = np.ascontiguousarray(values).ravel()
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize]
    ext = np.empty(n, v.dtype)
    ext.view(bits)[:] = np.asarray(value_nodata, dtype=v.dtype).reshape(1).view(bits)[0]   # NoData with its bits unchanged
    has = at != NONE
    ext.view(bits)[has] = v.view(bits)[at[has]]
    return {"extreme": ext.reshape(h, w), "at_cell": at.reshape(h, w)}
