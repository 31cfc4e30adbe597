"""A plain Python model of the distance and drop down to the stop cells over D-infinity / MFD proportions (include/rdgpu.h,
"flow distance and drop (HAND) DOWN to the stop cells"): the definition written out as a reverse Kahn order -- a cell is
computed when the last of its receivers has been decided -- with every value a Python float, which is an IEEE double
whose every product, sum and quotient is rounded on its own, exactly what an np.float64 scalar does.  It shares no code
with the engine; the hand-computed rasters in tests/test_mfd_distance_model.py pin it, and it then stands in for a
reference that does not exist.

One traversal gives every combination the engine offers (the order in which cells are decided does not depend on stat or
strict), so a test module computes a case once and shares it."""
import math
from collections import deque

import numpy as np

# neighbour n -> (dx, dy): 1 left, 2 up-left, 3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left
OFFS = {1: (-1, 0), 2: (-1, -1), 3: (0, -1), 4: (1, -1), 5: (1, 0), 6: (1, 1), 7: (0, 1), 8: (-1, 1)}
STATS = {"ave": 0, "min": 1, "max": 2}
NODATA, RESOLVED, DEAD, UNDECIDED = 0, 1, 2, 3


def receivers(props):
    """bool [9, h, w]: plane n is "neighbour n is a receiver" -- a positive share to a data cell inside the raster, from
    a cell that is not on the raster's edge"""
    h, w, _ = props.shape
    data = props[..., 0] != np.float32(-2.0)
    rec = np.zeros((9, h, w), bool)
    if h >= 3 and w >= 3:
        for n, (dx, dy) in OFFS.items():
            rec[n, 1:-1, 1:-1] = (data[1:-1, 1:-1] & (props[1:-1, 1:-1, n] > 0)
                                  & data[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx])
    return data, rec


def lengths(cell):
    cx, cy = abs(float(cell[0])), abs(float(cell[1]))
    diag = math.sqrt(cx * cx + cy * cy)
    return {n: (cx if n in (1, 5) else cy if n in (3, 7) else diag) for n in OFFS}


def distance_down_all(props, chan=None, elev=None, cell=(1.0, 1.0), out_nodata=-1.0):
    """{(stat, strict): {"dist": float64 [h, w], "drop": float64 [h, w] (with elev), "state": uint8 [h, w]}} for stat in
    "ave", "min", "max" and strict in True, False; plus the key "nrecv": int [h, w], the receivers per cell."""
    props = np.asarray(props, np.float32)
    h, w, _ = props.shape
    n_cells = h * w
    data, rec = receivers(props)
    nrecv = rec.sum(axis=0)
    stop = data & ((np.asarray(chan) != 0) if chan is not None else (nrecv == 0))
    ln = lengths(cell)
    share = [None] + [[float(v) for v in props[..., n].ravel()] for n in range(1, 9)]      # float32 -> double: exact
    recl = [None] + [rec[n].ravel().tolist() for n in range(1, 9)]
    z = None if elev is None else [float(v) for v in np.asarray(elev, np.float64).ravel()]
    datal, stopl = data.ravel().tolist(), stop.ravel().tolist()
    pending = nrecv.ravel().tolist()
    step = {n: dy * w + dx for n, (dx, dy) in OFFS.items()}
    opp = {n: n + 4 if n <= 4 else n - 4 for n in OFFS}
    combos = [(st, strict) for strict in (True, False) for st in (0, 1, 2)]
    state = {True: [NODATA] * n_cells, False: [NODATA] * n_cells}
    qd = {k: [0.0] * n_cells for k in combos}
    qh = {k: [0.0] * n_cells for k in combos}

    queue = deque()
    for c in range(n_cells):
        if not datal[c]:
            continue
        if stopl[c]:
            s = RESOLVED
        elif pending[c] == 0:
            s = DEAD
        else:
            s = UNDECIDED
        state[True][c] = state[False][c] = s
        if s != UNDECIDED:
            queue.append(c)

    def decide(d):
        rs = [n for n in range(1, 9) if recl[n][d]]
        for strict in (True, False):
            stt = state[strict]
            con = [n for n in rs if stt[d + step[n]] == RESOLVED]
            ok = (len(con) == len(rs)) if strict else (len(con) >= 1)
            stt[d] = RESOLVED if ok else DEAD
            if not ok:
                continue
            for st in (0, 1, 2):
                for q, plane in ((qd[(st, strict)], 0), (qh[(st, strict)], 1)):
                    if plane == 1 and z is None:
                        continue
                    v = {}
                    for n in con:
                        r = d + step[n]
                        inc = ln[n] if plane == 0 else z[d] - z[r]
                        v[n] = q[r] + inc
                    if st == 0:
                        if len(con) == 1:
                            res = v[con[0]]
                        else:
                            num, den = 0.0, 0.0
                            for n in con:
                                num = num + share[n][d] * v[n]
                                den = den + share[n][d]
                            res = num / den
                    else:
                        res = v[con[0]]
                        for n in con[1:]:
                            if (v[n] < res) if st == 1 else (v[n] > res):
                                res = v[n]
                    q[d] = res

    while queue:
        c = queue.popleft()
        x, y = c % w, c // w
        for m, (dx, dy) in OFFS.items():                 # the donors of c: the neighbour m of c that has c as a receiver
            tx, ty = x + dx, y + dy
            if not (0 <= tx < w and 0 <= ty < h):
                continue
            d = ty * w + tx
            if not datal[d] or stopl[d] or not recl[opp[m]][d]:
                continue
            pending[d] -= 1
            if pending[d] == 0:
                decide(d)
                queue.append(d)

    out = {"nrecv": nrecv}
    names = {v: k for k, v in STATS.items()}
    for st, strict in combos:
        s = np.array(state[strict], np.uint8).reshape(h, w)
        res = {"state": s}
        for name, q in (("dist", qd), ("drop", qh)):
            if name == "drop" and z is None:
                continue
            a = np.array(q[(st, strict)], np.float64).reshape(h, w)
            a[s != RESOLVED] = out_nodata
            res[name] = a
        out[(names[st], strict)] = res
    return out


def distance_down(props, chan=None, elev=None, stat="ave", strict=True, cell=(1.0, 1.0), out_nodata=-1.0):
    return distance_down_all(props, chan, elev, cell, out_nodata)[(stat, bool(strict))]
