"""A plain Python model of the stream reaches (include/rdgpu.h, "stream reaches on the D8 direction forest"): tops found
from the channel children, every reach walked down from its top through only-children, catchments by a memoised walk to
the first channel cell -- straight from the definition, linear in the cells.  It shares no code with the engine (no
bottoms mask, no flow-path pass); the hand-built forests in tests/test_stream_reach_model.py pin it, and it then stands in
for a reference that does not exist."""
import math

import numpy as np

# D8 numbering 234/105/876: code -> (dx, dy)
OFFS = {1: (-1, 0), 2: (-1, -1), 3: (0, -1), 4: (1, -1), 5: (1, 0), 6: (1, 1), 7: (0, 1), 8: (-1, 1)}
# rdgpu_reach: 48 bytes, no padding
REACH_DTYPE = np.dtype([("top_cell", np.uint32), ("bottom_cell", np.uint32), ("down", np.uint32), ("up", np.uint32),
                        ("cells", np.uint32), ("catchment_cells", np.uint32), ("steps", np.uint32, (3,)), ("order", np.uint32),
                        ("length", np.float64)])


def _plane(code):
    dx, dy = OFFS[code]
    return 0 if dy == 0 else 1 if dx == 0 else 2


def _targets(dirs, nodata):
    """flat index of the cell every cell's code 1..8 points at, -1 without a code or off the raster"""
    h, w = dirs.shape
    ys, xs = np.mgrid[0:h, 0:w]
    tgt = np.full((h, w), -1, np.int64)
    for code, (dx, dy) in OFFS.items():
        tx, ty = xs + dx, ys + dy
        ok = (dirs == code) & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
        tgt[ok] = (ty * w + tx)[ok]
    if nodata in OFFS:
        tgt[dirs == nodata] = -1
    return tgt.ravel()


def stream_reaches(dirs, nodata=255, chan=None, order=None, cell=(1.0, 1.0)):
    """dict: reach, catchment (uint32 [h, w]), table (REACH_DTYPE [N]), bottoms (uint8 [h, w])"""
    h, w = dirs.shape
    n = h * w
    d = dirs.ravel()
    valid = d != nodata
    m = valid.copy() if chan is None else (valid & (chan.ravel() != 0))
    raw = _targets(dirs, nodata)
    ctgt = np.where(m & (raw >= 0) & m[np.maximum(raw, 0)], raw, -1)       # the channel target of a channel cell
    nchild = np.bincount(ctgt[ctgt >= 0], minlength=n)
    tops = np.flatnonzero(m & (nchild != 1))
    ct, nc, codes = ctgt.tolist(), nchild.tolist(), d.tolist()
    reaches = []                                                            # (bottom, top, cells, steps)
    for t in tops.tolist():
        c, cells, steps = t, 1, [0, 0, 0]
        while True:
            nxt = ct[c]
            if nxt >= 0:
                steps[_plane(codes[c])] += 1
            if nxt < 0 or nc[nxt] >= 2:                                     # a mouth | the cell before a junction: the bottom
                break
            c, cells = nxt, cells + 1                                       # c is nxt's only child
            assert cells <= n
        reaches.append((c, t, cells, steps))
    reaches.sort()                                                          # by the bottom's raster index
    assert len({r[0] for r in reaches}) == len(reaches)                     # every bottom has exactly one top
    table = np.zeros(len(reaches), REACH_DTYPE)
    reach = np.zeros(n, np.uint32)
    for i, (b, t, cells, steps) in enumerate(reaches):
        c = t
        while True:
            assert reach[c] == 0
            reach[c] = i + 1
            if c == b:
                break
            c = ct[c]
    o = None if order is None else order.ravel()
    cx, cy = abs(float(cell[0])), abs(float(cell[1]))
    diag = math.sqrt(cx * cx + cy * cy)
    for i, (b, t, cells, steps) in enumerate(reaches):
        table[i] = (t, b, 0 if ct[b] < 0 else reach[ct[b]], nc[t], cells, 0, tuple(steps), 0 if o is None else o[t], 0.0)
    s = table["steps"].astype(np.float64).reshape(-1, 3)
    table["length"] = s[:, 0] * cx + s[:, 1] * cy + s[:, 2] * diag          # numpy rounds every product and every sum
    # catchments: the first channel cell on every cell's path, walks memoised
    full = np.where(valid & (raw >= 0) & valid[np.maximum(raw, 0)], raw, -1).tolist()
    first = [-2] * n                                                        # -2 unknown, -3 on the walk, -1 none, else the cell
    mm, vv = m.tolist(), valid.tolist()
    for c0 in range(n):
        if first[c0] != -2:
            continue
        walk, c = [], c0
        while True:
            if not vv[c]:
                ans = -1
                break
            if first[c] == -3:                                              # a loop met before any channel cell
                ans = -1
                break
            if first[c] != -2:
                ans = first[c]
                break
            if mm[c]:
                ans = first[c] = c
                break
            first[c] = -3
            walk.append(c)
            if full[c] < 0:
                ans = -1
                break
            c = full[c]
        for c in walk:
            first[c] = ans
        if first[c0] == -2:
            first[c0] = ans
    first = np.array(first, np.int64)
    catchment = np.where(first >= 0, reach[np.maximum(first, 0)], 0).astype(np.uint32)
    catchment[~valid] = 0
    table["catchment_cells"] = np.bincount(catchment, minlength=len(reaches) + 1)[1:]
    bottoms = np.zeros(n, np.uint8)
    bottoms[table["bottom_cell"]] = 1
    return {"reach": reach.reshape(h, w), "catchment": catchment.reshape(h, w), "table": table, "bottoms": bottoms.reshape(h, w)}
