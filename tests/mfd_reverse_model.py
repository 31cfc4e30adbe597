"""A plain Python model of the reverse accumulation, the largest weight downslope and the upslope dependence over
D-infinity / MFD proportions (include/rdgpu.h, "reverse accumulation ..."): the definition written out as a reverse Kahn
order -- a cell is computed when the last of its receivers has been decided -- with every value a Python float, which is
an IEEE double whose every product and sum is rounded on its own.  It shares no code with the engine; the hand-computed
rasters in tests/test_mfd_reverse_model.py pin it, and it then stands in for a reference that does not exist.  The
receivers are those of tests/mfd_distance_model.py (the same graph)."""
import math
import os
import sys
from collections import deque

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mfd_distance_model import OFFS, receivers  # noqa: E402

NODATA, RESOLVED, EMPTY, UNDECIDED = 0, 1, 2, 3


def cell_weights(data, weights, weight_nodata, dest):
    """(weight per cell as a list of floats, "contributes" per cell as a list of bools) for the data mask given"""
    n = data.size
    if weights is None:
        if dest is None:
            raise ValueError("neither weights nor dest")
        a = (np.asarray(dest).ravel() != 0)
        return [1.0 if v else 0.0 for v in a.tolist()], [True] * n
    wl = [float(v) for v in np.asarray(weights, np.float64).ravel()]
    wnd = float("nan") if weight_nodata is None else float(weight_nodata)
    return wl, [not (v == wnd) and not math.isnan(v) for v in wl]


def reverse_accum(props, weights=None, dest=None, weight_nodata=None, out_nodata=-1.0):
    """{"racc": float64 [h, w], "wmax": float64 [h, w] (with weights), "state": uint8 [h, w], "nrecv": int [h, w]}; nrecv
    counts the receivers of the graph itself (an absorbing cell keeps its count there, though its R(c) is taken as empty)"""
    props = np.asarray(props, np.float32)
    h, w, _ = props.shape
    n_cells = h * w
    data, rec = receivers(props)
    nrecv = rec.sum(axis=0)
    absorb = data & (np.asarray(dest) != 0) if dest is not None else np.zeros((h, w), bool)
    wl, conl = cell_weights(data, weights, weight_nodata, dest)
    share = [None] + [[float(v) for v in props[..., n].ravel()] for n in range(1, 9)]      # float32 -> double: exact
    recl = [None] + [rec[n].ravel().tolist() for n in range(1, 9)]
    datal, absl = data.ravel().tolist(), absorb.ravel().tolist()
    pending = np.where(absorb, 0, nrecv).ravel().tolist()
    step = {n: dy * w + dx for n, (dx, dy) in OFFS.items()}
    opp = {n: n + 4 if n <= 4 else n - 4 for n in OFFS}
    state = [NODATA] * n_cells
    racc = [0.0] * n_cells
    wmax = [0.0] * n_cells

    def decide(c):
        s = wl[c] if conl[c] else 0.0
        has, m = conl[c], wl[c]
        if not absl[c]:
            for n in range(1, 9):
                if not recl[n][c]:
                    continue
                r = c + step[n]
                s = s + share[n][c] * racc[r]
                if state[r] == RESOLVED and (not has or wmax[r] > m):
                    has, m = True, wmax[r]
        racc[c] = s
        wmax[c] = m
        state[c] = RESOLVED if has else EMPTY

    queue = deque()
    for c in range(n_cells):
        if not datal[c]:
            continue
        if pending[c] == 0:
            decide(c)
            queue.append(c)
        else:
            state[c] = UNDECIDED
    while queue:
        c = queue.popleft()
        x, y = c % w, c // w
        for m, (dx, dy) in OFFS.items():                 # the donors of c: the neighbour m of c that has c as a receiver
            tx, ty = x + dx, y + dy
            if not (0 <= tx < w and 0 <= ty < h):
                continue
            d = ty * w + tx
            if not datal[d] or absl[d] or not recl[opp[m]][d]:
                continue
            pending[d] -= 1
            if pending[d] == 0:
                decide(d)
                queue.append(d)

    st = np.array(state, np.uint8).reshape(h, w)
    out = {"state": st, "nrecv": nrecv}
    a = np.array(racc, np.float64).reshape(h, w)
    a[(st == NODATA) | (st == UNDECIDED)] = out_nodata
    out["racc"] = a
    if weights is not None:
        m = np.array(wmax, np.float64).reshape(h, w)
        m[st != RESOLVED] = out_nodata
        out["wmax"] = m
    return out
