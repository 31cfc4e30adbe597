"""Hand-built D8 forests for the stream-order tests: directions painted cell by cell, background code 0 (NO_FLOW)."""
import numpy as np

from stream_model import OFFS

CODE = {v: k for k, v in OFFS.items()}


def blank(h, w):
    return np.zeros((h, w), np.uint8)


def paint(dirs, path, last=0):
    """path: cells (x, y), each a D8 neighbour of the next; every cell points at its successor, the last gets `last`"""
    for (x, y), (nx, ny) in zip(path[:-1], path[1:]):
        dirs[y, x] = CODE[(nx - x, ny - y)]
    if last is not None:
        x, y = path[-1]
        dirs[y, x] = last
    return dirs


def mask_of(shape, cells):
    m = np.zeros(shape, np.uint8)
    for x, y in cells:
        m[y, x] = 1
    return m


def binary_tree(k, ox=0, oy=0, shape=None):
    """A perfect binary tree of order k: 2^(k-1) leaves two columns apart on the bottom row, siblings running diagonally up to
    their parent.  Root at (ox + 2^(k-1) - 1, oy); width 2^k - 1, height 2^(k-1).  Returns dirs, root, the cells of the tree."""
    wid, hgt = 2 ** k - 1, 2 ** (k - 1)
    shape = shape or (oy + hgt, ox + wid)
    dirs = blank(*shape)
    cells = []

    def build(level, cx, cy):          # the subtree of order `level` whose root is (cx, cy)
        cells.append((cx, cy))
        if level == 1:
            return
        dx = 2 ** (level - 2)
        for sgn in (-1, 1):
            path = [(cx + sgn * i, cy + i) for i in range(dx, 0, -1)] + [(cx, cy)]
            paint(dirs, path, last=None)
            cells.extend(path[1:-1])
            build(level - 1, cx + sgn * dx, cy + dx)

    root = (ox + 2 ** (k - 1) - 1, oy)
    build(k, *root)
    return dirs, root, cells


def serpentine(n=200, tributaries=False):
    """One channel through an n x n raster: along the even rows, alternately right and left, one turn cell in the odd row
    between.  With tributaries: a one-cell tributary (in the odd row below) into the first cell behind every crossing of a
    multiple of 64 along a row.  Returns dirs and the channel mask."""
    path = []
    for i, y in enumerate(range(0, n - 1, 2)):
        xs = range(n) if i % 2 == 0 else range(n - 1, -1, -1)
        path += [(x, y) for x in xs]
        if y + 2 < n - 1:
            path.append((path[-1][0], y + 1))
    dirs = paint(blank(n, n), path)
    cells = list(path)
    if tributaries:
        for i, y in enumerate(range(0, n - 1, 2)):
            for b in range(64, n, 64):
                x = b if i % 2 == 0 else b - 1
                if x in (0, n - 1):
                    continue
                dirs[y + 1, x] = 3                         # (0, -1): up into the channel
                cells.append((x, y + 1))
    return dirs, mask_of((n, n), cells)


def loop_with_tributary(x, y, shape):
    """A 4-cell loop whose top-left cell is (x, y); a tributary with a junction of its own flows into (x, y) from the left,
    and a second feeder (the "tail") into (x + 1, y + 1) from below right.  Returns dirs, loop cells, feeder cells."""
    dirs = blank(*shape)
    loop = [(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)]
    paint(dirs, loop + [loop[0]], last=None)
    trib = [(x - 5 + i, y) for i in range(5)]
    paint(dirs, trib + [loop[0]], last=None)
    side = [(x - 3, y - 2), (x - 3, y - 1), (x - 3, y)]
    paint(dirs, side, last=None)
    tail = [(x + 2 + i, y + 2 + i) for i in range(4, -1, -1)]
    paint(dirs, tail + [loop[2]], last=None)
    return dirs, loop, trib + side[:-1] + tail


def three_way(cx, cy, shape):
    """Three channels of order 2 (each a two-head fork) meet at (cx, cy): from the left, from above and from the right."""
    dirs = blank(*shape)
    for (dx, dy) in ((-1, 0), (0, -1), (1, 0)):
        px, py = -dy, dx                                   # across the arm
        arm = [(cx + dx * i, cy + dy * i) for i in range(4, 0, -1)]
        paint(dirs, arm + [(cx, cy)], last=None)
        for s in (-1, 1):
            paint(dirs, [(arm[0][0] + dx + s * px, arm[0][1] + dy + s * py), arm[0]], last=None)
    return dirs
