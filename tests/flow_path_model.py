"""A plain Python model of the flow-path products (include/rdgpu.h, "flow distance, drainage cell and HAND"): every path
walked cell by cell with a visited set, straight from the definition; what a walk has settled is kept, so a cell is
walked once.  It shares no code and no tiling with the engine; the hand-written rasters in
tests/test_flow_path_model.py pin it, and it then stands in for a reference that does not exist."""
import math

import numpy as np

# D8 numbering 234/105/876: code -> (dx, dy)
OFFS = {1: (-1, 0), 2: (-1, -1), 3: (0, -1), 4: (1, -1), 5: (1, 0), 6: (1, 1), 7: (0, 1), 8: (-1, 1)}
NONE = 0xFFFFFFFF


def plane_of(code):
    """0: a step along x (dy == 0), 1: along y (dx == 0), 2: diagonal"""
    dx, dy = OFFS[code]
    return 0 if dy == 0 else 1 if dx == 0 else 2


def stop_cells(dirs, nodata=255, chan=None):
    return None if chan is None else ((chan != 0) & (dirs != nodata))


def diag_of(cell):
    cx, cy = abs(float(cell[0])), abs(float(cell[1]))
    return cx, cy, math.sqrt(cx * cx + cy * cy)


def flow_path(dirs, nodata=255, chan=None, cell=(1.0, 1.0), dist_nodata=-1.0):
    """dict: to_cell uint32 [h, w], steps uint32 [3, h, w], dist float64 [h, w]"""
    h, w = dirs.shape
    n = h * w
    d = dirs.ravel().tolist()
    stop = stop_cells(dirs, nodata, chan)
    stop = None if stop is None else stop.ravel().tolist()
    settled = [False] * n
    to = [NONE] * n
    cnt = [(0, 0, 0)] * n

    def step(c):
        """("end", the drainage cell or None) where the walk stops at c, else ("next", the target, the step's plane)"""
        dc = d[c]
        if dc == nodata:
            return "end", None, None
        if stop is not None and stop[c]:
            return "end", c, None
        here = c if stop is None else None           # the path ends here: the last cell that is not NoData | no stop cell met
        if dc not in OFFS:
            return "end", here, None
        x, y = c % w, c // w
        tx, ty = x + OFFS[dc][0], y + OFFS[dc][1]
        if not (0 <= tx < w and 0 <= ty < h):
            return "end", here, None
        t = ty * w + tx
        if stop is None and d[t] == nodata:
            return "end", here, None
        return "next", t, plane_of(dc)

    for c0 in range(n):
        if settled[c0]:
            continue
        walk, seen, c = [], set(), c0
        while True:
            if settled[c]:
                base = (to[c], cnt[c])
                break
            if c in seen:                             # a direction loop: nothing on this walk has a drainage cell
                base = (NONE, (0, 0, 0))
                break
            kind, a, p = step(c)
            if kind == "end":
                settled[c], to[c], cnt[c] = True, (NONE if a is None else a), (0, 0, 0)
                base = (to[c], cnt[c])
                break
            seen.add(c)
            walk.append((c, p))
            c = a
        t, k = base
        for c, p in reversed(walk):
            if t != NONE:
                k = tuple(v + (1 if i == p else 0) for i, v in enumerate(k))
            settled[c], to[c], cnt[c] = True, t, k
    to_cell = np.array(to, np.uint32).reshape(h, w)
    steps = np.array(cnt, np.uint32).T.reshape(3, h, w).copy()
    none = to_cell == NONE
    steps[:, none] = NONE
    cx, cy, diag = diag_of(cell)
    nx, ny, nd = (steps[i].astype(np.float64) for i in range(3))
    dist = nx * cx + ny * cy + nd * diag              # numpy rounds every product and every sum: no fused multiply-add
    dist[none] = dist_nodata
    return {"to_cell": to_cell, "steps": steps, "dist": dist}


def hand(dem, to_cell, dem_nodata, out_nodata=-9999.0):
    """float64: dem[c] - dem[to_cell[c]]; out_nodata without a drainage cell or where either elevation is dem_nodata"""
    flat = dem.ravel()
    none = to_cell.ravel() == NONE
    t = np.where(none, 0, to_cell.ravel()).astype(np.int64)
    nd = np.array(dem_nodata).astype(dem.dtype)
    bad = none | (flat == nd) | (flat[t] == nd)
    out = flat.astype(np.float64) - flat[t].astype(np.float64)
    out[bad] = out_nodata
    return out.reshape(dem.shape)
