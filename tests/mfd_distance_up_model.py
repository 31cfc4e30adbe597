"""A plain Python model of the distance and rise up to the sources over D-infinity / MFD proportions (include/rdgpu.h,
"flow distance and rise UP to the sources"): the definition written out as a Kahn order -- a cell is computed when the
last of its donors has been decided -- with every value a Python float, which is an IEEE double whose every product, sum
and quotient is rounded on its own.  It shares no code with the engine and none with mfd_distance_model.py; the
hand-computed rasters, the duality with the down model and the memoised recursion in tests/test_mfd_distance_up_model.py
pin it, and it then stands in for a reference that does not exist.

One traversal gives all three statistics (the order in which cells are decided does not depend on stat), so a test module
computes a case once and shares it."""
import math

import numpy as np

# position m around a cell -> (dx, dy): 1 left, 2 up-left, 3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left
AROUND = ((1, -1, 0), (2, -1, -1), (3, 0, -1), (4, 1, -1), (5, 1, 0), (6, 1, 1), (7, 0, 1), (8, -1, 1))
STAT_NAMES = ("ave", "min", "max")


def step_lengths(cell):
    cx, cy = abs(float(cell[0])), abs(float(cell[1]))
    diag = math.sqrt(cx * cx + cy * cy)
    return [None, cx, diag, cy, diag, cx, diag, cy, diag]


def links_into(props, min_share=0.0):
    """(data, into): data bool [h, w]; into[c] = [(m, d, share)] in the order m = 1..8 -- the neighbour m of c is the cell d,
    a data cell off the raster's edge whose share towards c (its neighbour m + 4 or m - 4) is above min_share in float32"""
    props = np.asarray(props, np.float32)
    h, w, _ = props.shape
    ms = np.float32(min_share)
    data = props[..., 0] != np.float32(-2.0)
    gives = data.copy()                                   # the cells that can be donors: data cells off the raster's edge
    gives[0, :] = gives[-1, :] = gives[:, 0] = gives[:, -1] = False
    into = [[] for _ in range(h * w)]
    for m, dx, dy in AROUND:                              # (m ascending: every cell's list comes out in the order m = 1..8)
        ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))      # the cells c ...
        yd, xd = slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx))      # ... and their neighbour m
        p = np.zeros((h, w), np.float32)
        p[ys, xs] = props[yd, xd, m + 4 if m <= 4 else m - 4]
        ok = np.zeros((h, w), bool)
        ok[ys, xs] = data[ys, xs] & gives[yd, xd]
        ok &= p > ms
        cells = np.flatnonzero(ok).tolist()
        shares = p.ravel()[ok.ravel()].tolist()           # float32 -> double: exact
        for c, s in zip(cells, shares):
            into[c].append((m, c + dy * w + dx, s))
    return data, into


def distance_up_all(props, elev=None, min_share=0.0, cell=(1.0, 1.0), out_nodata=-1.0):
    """{"ave" | "min" | "max": {"dist": float64 [h, w], "rise": float64 [h, w] (with elev)}, "ndonors": int [h, w],
    "decided": bool [h, w] (False on NoData and on what a cycle of links holds up)}"""
    props = np.asarray(props, np.float32)
    h, w, _ = props.shape
    n = h * w
    data, into = links_into(props, min_share)
    length = step_lengths(cell)
    z = None if elev is None else [float(v) for v in np.asarray(elev, np.float64).ravel()]
    planes = ("dist",) if z is None else ("dist", "rise")
    left = [len(lk) for lk in into]
    out_of = [[] for _ in range(n)]
    for c in range(n):
        for _, d, _ in into[c]:
            out_of[d].append(c)
    q = {(s, k): [0.0] * n for s in STAT_NAMES for k in planes}
    decided = [False] * n
    todo = [c for c in range(n) if data.flat[c] and left[c] == 0]                   # the sources: their values are 0
    for c in todo:
        decided[c] = True

    def combine(c):
        lk = into[c]
        for k in planes:
            for s in STAT_NAMES:
                vals = q[(s, k)]
                v = [vals[d] + (length[m] if k == "dist" else z[d] - z[c]) for m, d, _ in lk]
                if s == "ave":
                    if len(v) == 1:
                        res = v[0]
                    else:
                        num = den = 0.0
                        for (_, _, p), vd in zip(lk, v):
                            num = num + p * vd
                            den = den + p
                        res = num / den
                else:
                    res = v[0]
                    for vd in v[1:]:
                        if (vd < res) if s == "min" else (vd > res):
                            res = vd
                vals[c] = res

    while todo:
        d = todo.pop()
        for c in out_of[d]:
            left[c] -= 1
            if left[c] == 0:
                combine(c)
                decided[c] = True
                todo.append(c)

    dec = np.array(decided, bool).reshape(h, w)
    out = {"ndonors": np.array([len(lk) for lk in into]).reshape(h, w), "decided": dec}
    for s in STAT_NAMES:
        out[s] = {}
        for k in planes:
            a = np.array(q[(s, k)], np.float64).reshape(h, w)
            a[~dec] = out_nodata
            out[s][k] = a
    return out


def distance_up(props, elev=None, stat="ave", min_share=0.0, cell=(1.0, 1.0), out_nodata=-1.0):
    return distance_up_all(props, elev, min_share, cell, out_nodata)[stat]
