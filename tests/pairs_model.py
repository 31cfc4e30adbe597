"""numpy model of what the compact fill's pair pass (k_pairs16, csrc/fill.hip) sees of a raster, and
the rasters of test_fill_pairs_residency_gpu.py.  Not a test module.

The descent forest is pit_dissolve_model's (pits dissolved inside their 64 x 64 tile, as the engine does).  From it:

  nodes(...)           per 64 x 64 descent tile, the roots of the tile: pits, cells draining off the raster, cells whose
                       descent neighbour lies outside the tile -- the entries of the tile's node table
  boundary_cells(...)  per 64 x 32 pair tile, the cells with an E / SE / S / SW (D4: E / S) neighbour of another basin --
                       the entries of the tile's boundary list (a neighbour outside the raster counts as "outside", the
                       basin of every cell that drains off the raster)"""
import os

import numpy as np

import pit_dissolve_model as pm

DT, TW, TH = 64, 64, 32
LIST_CAP = 1008          # boundary cells the pair pass lists at once (csrc/fill.hip)
NT_CAP = 512             # node-table entries it stages in LDS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs_list_cap.npz")


def forest(z, topo=8, dissolve=True):
    """(ptr, lab): the descent pointer of every cell (flat index; N = off the raster; a pit points at itself) after the
    in-tile dissolving, and the basin of every cell (0 .. B - 1; B = outside).  The pointers are fill_dissolve's."""
    SH = pm.SH8 if topo == 8 else pm.SH4
    h, w = z.shape
    N = h * w
    _, inv = np.unique(z, return_inverse=True)
    k = inv.reshape(h, w).astype(np.int64) + 1
    idx = np.arange(N, dtype=np.int64).reshape(h, w)
    OUT = np.int64(N)
    border = np.zeros((h, w), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    qk, qi = np.full((h, w), pm.BIG), np.full((h, w), pm.BIG)
    for dy, dx in SH:
        kn, inn = pm.shifted(k, dy, dx, pm.BIG), pm.shifted(idx, dy, dx, pm.BIG)
        better = (kn < qk) | ((kn == qk) & (inn < qi))
        qk, qi = np.where(better, kn, qk), np.where(better, inn, qi)
    drains = (qk < k) | ((qk == k) & (qi < idx))
    ptr = np.where(drains, qi, idx)
    ptr[border] = OUT
    ptr = ptr.ravel().copy()
    pits = np.flatnonzero(ptr == np.arange(N))
    if dissolve and len(pits):
        q = qi.ravel()[pits]
        cand = ptr[q] != pits
        intile = ((pits // w) // DT == (q // w) // DT) & ((pits % w) // DT == (q % w) // DT)
        take = cand & intile
        ptr[pits[take]] = q[take]
    ext = np.append(ptr, OUT)
    while True:
        nxt = ext[ext]
        if (nxt == ext).all():
            break
        ext = nxt
    root = ext[:N]
    roots = np.flatnonzero(root == np.arange(N))
    rid = np.full(N + 1, -1, np.int64)
    rid[roots] = np.arange(len(roots))
    rid[N] = len(roots)
    return ptr, rid[root].reshape(h, w)


def nodes(ptr, shape):
    """roots per 64 x 64 descent tile"""
    h, w = shape
    N = h * w
    i = np.arange(N)
    y, x = i // w, i % w
    t = np.where(ptr == N, i, ptr)                       # (a cell draining off the raster is a root like a pit)
    root = (t == i) | ((t // w) // DT != y // DT) | ((t % w) // DT != x // DT)
    out = np.zeros((-(-h // DT), -(-w // DT)), np.int64)
    np.add.at(out, (y[root] // DT, x[root] // DT), 1)
    return out


def boundary(lab, topo=8):
    """bool per cell: a neighbour to the E, SE, S or SW (D4: E, S) belongs to another basin"""
    outside = lab[0, 0]                                   # (a corner cell drains off the raster)
    sh = [(0, 1), (1, 1), (1, 0), (1, -1)] if topo == 8 else [(0, 1), (1, 0)]
    b = np.zeros(lab.shape, bool)
    for dy, dx in sh:
        b |= pm.shifted(lab, dy, dx, outside) != lab
    return b


def boundary_cells(lab, topo=8):
    """boundary cells per 64 x 32 pair tile"""
    b = boundary(lab, topo)
    h, w = lab.shape
    y, x = np.nonzero(b)
    out = np.zeros((-(-h // TH), -(-w // TW)), np.int64)
    np.add.at(out, (y // TH, x // TW), 1)
    return out


# ---- the rasters ------------------------------------------------------------------------------------------------------

def small_basins(h=70, w=130, seed=5):
    """white noise smoothed once (3 x 3 box) with 35 % of the noise itself laid back over it: basins a few cells wide --
    more than 1 024 boundary cells in a pair tile under D8 and under D4, at most NT_CAP nodes in every descent tile"""
    rng = np.random.default_rng(seed)
    a = rng.random((h + 2, w + 2))
    s = sum(a[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    return (0.65 * s + 0.35 * a[1:-1, 1:-1]).astype(np.float32)


#: ring_crossings: per crossing the chain of cells a', a | b, b', tail ... -- a (basin 1) and b (basin 2) are neighbours across
#: an edge of a pair tile; which tile's ring cell the pair is found through is noted beside each
CROSSINGS = {
    "top edge, S": [(30, 90), (31, 90), (32, 90), (33, 89), (34, 88), (35, 87), (36, 86)],          # bottom ring row of (64, 0)
    "top edge, SW": [(30, 102), (31, 101), (32, 100), (33, 99), (34, 98), (35, 97)],                # bottom ring row of (64, 0)
    "top edge, SE": [(30, 108), (31, 109), (32, 110), (33, 110), (34, 109), (35, 108), (36, 107)],  # bottom ring row of (64, 0)
    "top-left corner": [(30, 62), (31, 63), (32, 64), (33, 65), (34, 64), (35, 63), (36, 62)],      # SE corner of (0, 0)'s ring
    "top-right corner": [(30, 129), (31, 128), (32, 127), (33, 126), (34, 125), (35, 124)],         # SW corner of (128, 0)'s ring
    "bottom-left corner": [(62, 65), (63, 64), (64, 63), (65, 62), (66, 61), (67, 60)],             # SW corner of (64, 32)'s ring
    "bottom-right corner": [(62, 126), (63, 127), (64, 128), (65, 129), (66, 128), (67, 127)],      # SE corner of (64, 32)'s ring
    "left column, SW": [(39, 65), (40, 64), (41, 63), (42, 62), (43, 61)],                          # left ring column of (64, 32)
    "left edge, first row": [(96, 129), (96, 128), (96, 127), (96, 126), (96, 125), (96, 124)],     # right ring column of (64, 96)
}


def ring_crossings(h=141, w=214):
    """A plane falling towards the raster's west edge (one basin: outside) with chains of low cells dug across the edges
    of the pair tile at (64, 32) (and one across the left edge of the tile at (128, 96), in its first row).  A chain is
    a' (10, a pit), a (20) | b (21), b' (11, a pit), then a tail rising by one per cell: two depressions whose only LOW
    pass (21) is the step a | b across the tile edge -- everywhere else they meet over plane cells hundreds higher.  The
    pair with that key is found through a ring cell of the tile that holds the upper / left one of a and b: its row below,
    its right column, its left column from the second row down, never through the row above a tile or the cell left of
    its first row, which the pair pass does not stage."""
    y, x = np.mgrid[0:h, 0:w]
    z = (100.0 + 4.0 * x + 0.25 * y).astype(np.float32)
    for cells in CROSSINGS.values():
        vals = [10.0, 20.0, 21.0, 11.0] + [12.0 + j for j in range(len(cells) - 4)]
        for (cy, cx), v in zip(cells, vals):
            z[cy, cx] = np.float32(v)
    return z


def low_pass_only_at(z, lab, a, b, topo=8):
    """the two basins of cells a and b are different depressions, and the lowest pass between them is the step a | b alone"""
    la, lb, outside = lab[a], lab[b], lab[0, 0]
    if la == lb or la == outside or lb == outside:
        return False
    SH = pm.SH8 if topo == 8 else pm.SH4
    best, at = None, []
    for dy, dx in SH:
        ln, zn = pm.shifted(lab, dy, dx, -1), pm.shifted(z, dy, dx, np.float32(np.inf))
        m = (lab == la) & (ln == lb)
        ys, xs = np.nonzero(m)
        for cy, cx in zip(ys, xs):
            k = max(float(z[cy, cx]), float(zn[cy, cx]))
            if best is None or k < best:
                best, at = k, [((cy, cx), (cy + dy, cx + dx))]
            elif k == best:
                at.append(((cy, cx), (cy + dy, cx + dx)))
    return at == [(tuple(a), tuple(b))]                   # (seen from basin 1's side: one step, a -> b)


def golden():
    """the list-cap rasters (made by tests/tools/make_pairs_list_cap.py): name -> float32 raster"""
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}
