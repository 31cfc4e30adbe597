"""A plain Python model of the weighted D8 accumulation and of the total upstream length (include/rdgpu.h, "weighted
accumulation on the D8 direction forest"): in-degrees over the links and a Kahn queue, serial, O(cells).  A cell the queue
never releases lies on a direction loop; it keeps what reached it, so the links of a loop carry nothing.
Integer sums are Python integers.  For float weights every cell carries the LIST of the contributing weights of T(v) and
the sum is math.fsum of it: the correctly rounded true sum, whatever order the engine adds in.  The model shares neither
code nor tiling nor encoding with the engine; the hand-written rasters in tests/test_weighted_accum_model.py pin it."""
import math
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
# the reference's dx / dy tables (common/constants.hpp:44-45), index = code
OFFS = {1: (-1, 0), 2: (-1, -1), 3: (0, -1), 4: (1, -1), 5: (1, 0), 6: (1, 1), 7: (0, 1), 8: (-1, 1)}


def links(dirs, dir_nodata=255):
    """per cell (flat lists): participates, the flat index its link points to (-1: its tree ends here), the link's kind
    (0 along x, 1 along y, 2 diagonal; -1 without a link)"""
    h, w = dirs.shape
    part, link, kind = [], [], []
    for y in range(h):
        for x in range(w):
            d = int(dirs[y, x])
            part.append(d != dir_nodata)
            t, k = -1, -1
            if d != dir_nodata and d in OFFS:
                tx, ty = x + OFFS[d][0], y + OFFS[d][1]
                if 0 <= tx < w and 0 <= ty < h and int(dirs[ty, tx]) != dir_nodata:
                    t = ty * w + tx
                    k = 0 if OFFS[d][1] == 0 else 1 if OFFS[d][0] == 0 else 2
            link.append(t)
            kind.append(k)
    return part, link, kind


def _kahn(part, link, start, merge):
    """acc[v] = merge over T(v) of start[u]; merge(a, b) returns the combination (a may be changed in place)"""
    n = len(part)
    indeg = [0] * n
    for c in range(n):
        if link[c] >= 0:
            indeg[link[c]] += 1
    acc = list(start)
    queue = deque(c for c in range(n) if part[c] and indeg[c] == 0)
    while queue:
        c = queue.popleft()
        t = link[c]
        if t < 0:
            continue
        acc[t] = merge(acc[t], acc[c])
        indeg[t] -= 1
        if indeg[t] == 0:
            queue.append(t)
    return acc


def contributes(weights, weight_nodata):
    v = np.ascontiguousarray(weights).ravel()
    c = v != np.asarray(weight_nodata, dtype=v.dtype)        # == in W: -0.0 equals a NoData of 0.0
    if v.dtype.kind == "f":
        c &= ~np.isnan(v)                                    # a NaN never contributes
    return c.tolist()


def weighted_sum(dirs, weights, weight_nodata, dir_nodata=255, sum_nodata=-1, detail=False):
    """int64 [h, w] for integer weights, float64 for float weights; detail=True (float weights): also, per cell, the number
    of contributing cells of T(v) and the sum of their |w| (math.fsum), for the error bound"""
    assert weights.shape == dirs.shape
    h, w = dirs.shape
    part, link, _ = links(dirs, dir_nodata)
    con = contributes(weights, weight_nodata)
    flat = np.ascontiguousarray(weights).ravel()
    if flat.dtype.kind != "f":
        vals = [int(x) for x in flat.tolist()]
        acc = _kahn(part, link, [vals[c] if part[c] and con[c] else 0 for c in range(h * w)], lambda a, b: a + b)
        out = np.array([acc[c] if part[c] else int(sum_nodata) for c in range(h * w)], np.int64).reshape(h, w)
        return out
    vals = flat.astype(np.float64).tolist()                  # exact
    # every cell keeps the list of its own T(v): the copies cost the sum of the cells' depths, fine on a forest
    def merge(a, b):
        a.extend(b)
        return a
    acc = _kahn(part, link, [[vals[c]] if part[c] and con[c] else [] for c in range(h * w)], merge)
    out = np.array([math.fsum(acc[c]) if part[c] else float(sum_nodata) for c in range(h * w)], np.float64).reshape(h, w)
    if not detail:
        return out
    k = np.array([len(acc[c]) if part[c] else 0 for c in range(h * w)], np.int64).reshape(h, w)
    mag = np.array([math.fsum(abs(x) for x in acc[c]) if part[c] else 0.0 for c in range(h * w)], np.float64).reshape(h, w)
    return out, k, mag


def upstream_steps(dirs, dir_nodata=255):
    """uint32 [3, h, w]: per kind, the links of the cells of T(v), v excluded; 0xFFFFFFFF where v does not participate"""
    h, w = dirs.shape
    part, link, kind = links(dirs, dir_nodata)
    out = np.empty((3, h * w), np.uint32)
    for k in range(3):
        own = [1 if kind[c] == k else 0 for c in range(h * w)]
        acc = _kahn(part, link, own, lambda a, b: a + b)
        out[k] = [acc[c] - own[c] if part[c] else NONE for c in range(h * w)]
    return out.reshape(3, h, w)


def path_length(steps, cell_x=1.0, cell_y=1.0, length_nodata=-1.0):
    """rdgpu_d8_flow_path's dist on the three counts: a rounding after every product and every sum"""
    cx, cy = abs(float(cell_x)), abs(float(cell_y))
    diag = math.sqrt(cx * cx + cy * cy)
    nx, ny, nd = (steps[k].astype(np.float64) for k in range(3))
    length = (nx * cx + ny * cy) + nd * diag
    return np.where(steps[0] == NONE, length_nodata, length)


# ---- for the cross-check against the reference's FlowAccumulation ------------------------------------------------------
def zero_border(dirs, dir_nodata=255):
    """the reference counts the dependencies of interior cells only (flow_accumulation_generic.hpp:48-49): the code of every
    border cell that participates is set to 0 before both sides run"""
    d = dirs.copy()
    edge = np.ones(d.shape, bool)
    edge[1:-1, 1:-1] = False
    d[edge & (d != dir_nodata)] = 0
    return d


def props9(dirs, dir_nodata=255):
    """the proportions array of these directions as the reference's FM_D8 lays it out: slot 0 is -2 for NoData, -1 for no
    flow, 0 where the cell has a receiver, whose slot is 1"""
    h, w = dirs.shape
    p = np.zeros((h, w, 9), np.float32)
    code = np.where((dirs >= 1) & (dirs <= 8) & (dirs != dir_nodata), dirs, 0)
    p[..., 0] = np.where(dirs == dir_nodata, -2.0, np.where(code == 0, -1.0, 0.0))
    ys, xs = np.nonzero(code)
    p[ys, xs, code[ys, xs]] = 1.0
    return p


# ---- exact sums of float weights, for the error bound ------------------------------------------------------------------
def exact_sums(dirs, weights, weight_nodata, dir_nodata=255):
    """per cell (flat lists, integers in units of 2^-shift): the TRUE sum of the contributing weights of T(v), the sum of
    their magnitudes, and their number k; and shift.  Every finite double is an integer multiple of 2^-1074, so the sums
    are taken in Python integers and nothing is rounded."""
    part, link, _ = links(dirs, dir_nodata)
    con = contributes(weights, weight_nodata)
    vals = np.ascontiguousarray(weights).ravel().astype(np.float64).tolist()
    ratios = [v.as_integer_ratio() if part[c] and con[c] else (0, 1) for c, v in enumerate(vals)]
    shift = max(q.bit_length() - 1 for _, q in ratios)       # (every denominator is a power of two)
    ints = [p << (shift - (q.bit_length() - 1)) for p, q in ratios]
    start = [(n, abs(n), 1 if part[c] and con[c] else 0) for c, n in enumerate(ints)]
    acc = _kahn(part, link, start, lambda a, b: (a[0] + b[0], a[1] + b[1], a[2] + b[2]))
    return [a[0] for a in acc], [a[1] for a in acc], [a[2] for a in acc], shift
