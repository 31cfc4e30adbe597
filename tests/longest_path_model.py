"""A plain Python model of the longest upstream flow path (include/rdgpu.h, "longest upstream flow path"), serial and
built on flow_path_model.flow_path: D, steps and the outlet of every cell come from that model; the cells are then visited
from the farthest one to the nearest, each handing its best (D, lowest index) to the cell it flows to.  A cell's D is
strictly greater than its target's only in real numbers -- after rounding it may be equal -- so the order of the visits is
by the number of steps to the outlet, which is exact.  It shares no code and no tiling with the engine;
tests/test_longest_path_model.py pins it on hand-worked rasters and against a brute-force walk of every path."""
import numpy as np

from flow_path_model import NONE, OFFS, diag_of, flow_path


def longest_flow_path(dirs, nodata=255, cell=(1.0, 1.0), length_nodata=-1.0):
    """dict: from_cell uint32 [h, w], steps uint32 [3, h, w], length float64 [h, w], on_basin_path uint8 [h, w]"""
    h, w = dirs.shape
    n = h * w
    fp = flow_path(dirs, nodata, None, cell, -1.0)
    to = fp["to_cell"].ravel()
    st = fp["steps"].reshape(3, n)
    dist = fp["dist"].ravel()
    has = to != NONE
    d = dirs.ravel()
    best_d = np.where(has, dist, -1.0).tolist()       # D of the head found so far
    best_c = np.where(has, np.arange(n), NONE).tolist()
    total = np.where(has, st.astype(np.int64).sum(axis=0), -1)
    for c in np.argsort(-total, kind="stable").tolist():   # the farthest cells first: all of U(c) has reported before c does
        if not has[c] or to[c] == c:
            continue
        dx, dy = OFFS[int(d[c])]
        t = c + dy * w + dx
        if best_d[c] > best_d[t] or (best_d[c] == best_d[t] and best_c[c] < best_c[t]):
            best_d[t], best_c[t] = best_d[c], best_c[c]
    from_cell = np.array(best_c, np.uint32)
    src = np.where(has, from_cell, 0).astype(np.int64)
    steps = (st[:, src] - st).astype(np.uint32)
    steps[:, ~has] = NONE
    cx, cy, diag = diag_of(cell)
    nx, ny, nd = (steps[i].astype(np.float64) for i in range(3))
    length = nx * cx + ny * cy + nd * diag             # numpy rounds every product and every sum: no fused multiply-add
    length[~has] = length_nodata
    out_head = from_cell[np.where(has, to, 0).astype(np.int64)]
    on_path = (has & (from_cell == out_head)).astype(np.uint8)
    return {"from_cell": from_cell.reshape(h, w), "steps": steps.reshape(3, h, w), "length": length.reshape(h, w),
            "on_basin_path": on_path.reshape(h, w)}
