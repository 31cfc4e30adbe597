"""A plain Python model of the channel network products (include/rdgpu.h, "channel network and Strahler stream order"):
a Kahn queue over the channel cells, straight from the definition.  It shares no code with the engine; the hand-written
forests in tests/test_stream_model.py pin it, and it then stands in for a reference that does not exist."""
from collections import deque

import numpy as np

# D8 numbering 234/105/876: code -> (dx, dy)
OFFS = {1: (-1, 0), 2: (-1, -1), 3: (0, -1), 4: (1, -1), 5: (1, 0), 6: (1, 1), 7: (0, 1), 8: (-1, 1)}
HEAD, JUNCTION, ORDER_STEP, MOUTH, PLAIN = 1, 2, 3, 4, 5


def channel_mask(dirs, nodata=255, chan=None):
    m = dirs != nodata
    if chan is not None:
        m &= chan != 0
    return m


def _targets(dirs, nodata, chan):
    """flat index of every channel cell's channel target, -1 where its tree ends; and the channel mask"""
    h, w = dirs.shape
    m = channel_mask(dirs, nodata, chan)
    tgt = np.full(h * w, -1, np.int64)
    ys, xs = np.nonzero(m)
    for y, x in zip(ys.tolist(), xs.tolist()):
        d = int(dirs[y, x])
        if d not in OFFS:
            continue
        tx, ty = x + OFFS[d][0], y + OFFS[d][1]
        if 0 <= tx < w and 0 <= ty < h and m[ty, tx]:
            tgt[y * w + x] = ty * w + tx
    return tgt, m


def stream_order(dirs, nodata=255, chan=None):
    """uint8 raster: the Strahler order of every channel cell, 0 off the channels, 255 on what the queue never releases"""
    h, w = dirs.shape
    tgt, m = _targets(dirs, nodata, chan)
    pending = np.zeros(h * w, np.int64)           # channel children not yet released
    for c in np.nonzero(tgt >= 0)[0].tolist():
        pending[tgt[c]] += 1
    best = np.zeros(h * w, np.int64)              # largest order among the released children
    count = np.zeros(h * w, np.int64)             # how many of them have it
    order = np.where(m.reshape(-1), 255, 0).astype(np.int64)
    queue = deque(c for c in np.nonzero(m.reshape(-1))[0].tolist() if pending[c] == 0)
    while queue:
        c = queue.popleft()
        o = 1 if best[c] == 0 else (best[c] + 1 if count[c] >= 2 else best[c])
        order[c] = o
        t = tgt[c]
        if t < 0:
            continue
        if o > best[t]:
            best[t], count[t] = o, 1
        elif o == best[t]:
            count[t] += 1
        pending[t] -= 1
        if pending[t] == 0:
            queue.append(t)
    assert order[m.reshape(-1) & (order != 255)].max(initial=0) < 255
    return order.astype(np.uint8).reshape(h, w)


def stream_links(dirs, order, nodata=255, chan=None):
    """uint8 raster of kinds: first match of head, junction, order step, mouth, plain; 0 off the channels"""
    h, w = dirs.shape
    tgt, m = _targets(dirs, nodata, chan)
    nchild = np.zeros(h * w, np.int64)
    child = np.full(h * w, -1, np.int64)
    for c in np.nonzero(tgt >= 0)[0].tolist():
        nchild[tgt[c]] += 1
        child[tgt[c]] = c
    o = order.reshape(-1)
    kind = np.zeros(h * w, np.uint8)
    for c in np.nonzero(m.reshape(-1))[0].tolist():
        if nchild[c] == 0:
            kind[c] = HEAD
        elif nchild[c] >= 2:
            kind[c] = JUNCTION
        elif o[child[c]] != o[c]:
            kind[c] = ORDER_STEP
        elif tgt[c] < 0:
            kind[c] = MOUTH
        else:
            kind[c] = PLAIN
    return kind.reshape(h, w)


def channels(accum, threshold, accum_nodata=-1.0):
    return ((accum != accum_nodata) & (accum >= threshold)).astype(np.uint8)
