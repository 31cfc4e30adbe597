"""A plain numpy model of the three upslope products (catchments, outlets, upslope cells) and of the reference's line:
pointer doubling on flat indices with a bounded number of rounds.  tests/test_upslope_model.py pins it to the compiled
reference's outputs (tests/golden/ref_upslope.npz) bit for bit, so it may stand in for the reference where the reference
has no function (many seeds, outlets).

"The path of cell c" is c, the cell c's direction points to, and so on; it ends at a cell without a direction 1..8 or
whose target is off the raster.  A path that runs into a direction loop never ends."""
import numpy as np

D8X = np.array([0, -1, -1, 0, 1, 1, 1, 0, -1], np.int64)      # reference common/constants.hpp:44-45
D8Y = np.array([0, 0, -1, -1, -1, 0, 1, 1, 1], np.int64)
NONE = np.uint32(0xFFFFFFFF)


def _links(dirs, nodata, stop_before_nodata):
    """per cell the flat index of the next cell of its path, itself where the path ends"""
    h, w = dirs.shape
    d = dirs.astype(np.int64)
    flows = (dirs != nodata) & (d >= 1) & (d <= 8)
    k = np.where(flows, d, 0)
    yy, xx = np.mgrid[0:h, 0:w]
    tx, ty = xx + D8X[k], yy + D8Y[k]
    ok = flows & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    txc, tyc = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
    if stop_before_nodata:
        ok &= dirs[tyc, txc] != nodata
    self_ = yy * w + xx
    return np.where(ok, tyc * w + txc, self_).ravel()


def _ends(nxt):
    """(end, settled): the cell every path ends at; settled is False where the path never ends"""
    n = nxt.size
    p = nxt.copy()
    for _ in range(int(np.ceil(np.log2(max(n, 2)))) + 1):
        p = p[p]
    return p, nxt[p] == p     # (not p[p] == p: 2^k steps round a loop of 2^j cells come back to the start)


def catchments(dirs, seed_cells, seed_labels, unreached=0, nodata=255):
    h, w = dirs.shape
    n = h * w
    cells = np.asarray(seed_cells, np.int64).reshape(-1)
    labels = np.asarray(seed_labels, np.int32).reshape(-1)
    assert cells.size == labels.size and ((cells >= 0) & (cells < n)).all()
    pos = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(pos, cells, np.arange(cells.size, dtype=np.int64))      # the first entry of the list wins
    seeded = pos < cells.size
    nxt = _links(dirs, nodata, False)
    idx = np.arange(n, dtype=np.int64)
    nxt = np.where(seeded, idx, nxt)                                       # a seed absorbs
    end, settled = _ends(nxt)
    hit = settled & seeded[end]
    out = np.full(n, unreached, np.int32)
    out[hit] = labels[pos[end[hit]]]
    return out.reshape(h, w)


def outlets(dirs, nodata=255):
    h, w = dirs.shape
    end, settled = _ends(_links(dirs, nodata, True))
    out = np.where(settled & (dirs.ravel() != nodata), end, np.int64(NONE)).astype(np.uint32)
    return out.reshape(h, w)


def line(shape, x0, y0, x1, y1):
    """flat indices of the cells the reference's modified Bresenham marks (d8_methods.hpp:186-212), in its order; None
    where it would mark a cell outside the raster"""
    h, w = shape
    if x0 > x1:
        x0, x1, y0, y1 = x1, x0, y1, y0
    deltax, deltay = x1 - x0, y1 - y0
    with np.errstate(all="ignore"):
        deltaerr = np.float32(deltay) / np.float32(deltax)
    if deltaerr < 0:
        deltaerr = -deltaerr
    error = np.float32(0)
    step = (deltay > 0) - (deltay < 0)
    cells = []

    def mark(x, y):
        if not (0 <= x < w and 0 <= y < h):
            return False
        cells.append(y * w + x)
        return True

    y = y0
    for x in range(x0, x1 + 1):
        if not mark(x, y):
            return None
        with np.errstate(all="ignore"):
            error = np.float32(error + deltaerr)
        if error >= np.float32(0.5):
            if not mark(x + 1, y):
                return None
            y += step
            with np.errstate(all="ignore"):
                error = np.float32(error - np.float32(1))
    return np.array(cells, np.uint32)


def upslope_cells(dirs, x0, y0, x1, y1, nodata=255):
    cells = line(dirs.shape, x0, y0, x1, y1)
    assert cells is not None, "the line leaves the raster"
    c = catchments(dirs, cells, np.ones(cells.size, np.int32), 255, nodata).astype(np.uint8)
    c.ravel()[cells] = 2
    return c
