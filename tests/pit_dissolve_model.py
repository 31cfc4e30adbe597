"""numpy model of the fill with DISSOLVED PITS (k_descent16 in csrc/fill.hip), and the rasters its
tests share.  Not a test module: test_fill_pit_dissolve_model.py checks it against the oracle on the CPU,
test_fill_pit_dissolve_gpu.py takes the engine's `dissolved_pits` from it.

The rule.  p is a pit of the descent forest (no border cell, no lower neighbour in the (key, index) order), q its lowest
neighbour in that order.  If q does not point at p, then p points at q: p is no root any more, its catchment joins q's
tree, and p alone keeps a floor key(q):  W(p) = max(key(q), level of its basin),  W(c) = max(key(c), level) elsewhere.
Basins, pair weights and the Boruvka contraction are those of tests/tools/proto_fill.py on the coarser forest.

tile: None -- every such pit dissolves; 64 -- only those whose q lies in the pit's own 64 x 64 tile (the engine)."""
import numpy as np

SH8 = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]   # (dy, dx)
SH4 = [(0, -1), (-1, 0), (0, 1), (1, 0)]
BIG = np.int64(1) << 60


def shifted(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` outside the raster"""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    yn, xn = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
    out[ys, xs] = a[yn, xn]
    return out


def contract(k, comp0, B, SH):
    """Boruvka rounds on the basins comp0 (0 .. B - 1; B: the outside) with pass weights max(k, k of the neighbour):
    the level of every basin (0 for the outside).  As tests/tools/proto_fill.py, every round from the raster."""
    OUTC = B
    cur, acc = np.arange(B + 1), np.zeros(B + 1, np.int64)
    ids = np.arange(B + 1)
    rounds = 0
    while not (cur == OUTC).all():
        rounds += 1
        comp = cur[comp0]
        best = np.full(B + 1, np.iinfo(np.int64).max, np.int64)
        for dy, dx in SH:
            kn, cn = shifted(k, dy, dx, -1), shifted(comp, dy, dx, -1)
            m = (cn >= 0) & (cn != comp) & (comp != OUTC)
            np.minimum.at(best, comp[m], np.maximum(k, kn)[m] * (B + 2) + cn[m])
        roots = np.flatnonzero((cur == ids) & (ids != OUTC))
        assert (best[roots] < np.iinfo(np.int64).max).all()
        bw, bt = best[roots] // (B + 2), best[roots] % (B + 2)
        par, pm = ids.copy(), np.zeros(B + 1, np.int64)
        par[roots], pm[roots] = bt, bw
        mutual = (par[par[roots]] == roots) & (bt != OUTC) & (roots < bt)   # a mutual pair: the smaller id stays root
        par[roots[mutual]], pm[roots[mutual]] = roots[mutual], 0
        while True:
            pp, mm = par[par], np.maximum(pm, pm[par])
            if (pp == par).all():
                break
            par, pm = pp, mm
        c = cur.copy()
        cur, acc = par[c], np.maximum(acc, pm[c])
    return acc, rounds


def fill_dissolve(z, topo=8, tile=None, dissolve=True):
    """(filled raster, info).  info: pits (of the descent forest), dissolved, basins (= pits - dissolved), candidates
    (pits whose q does not drain into them, wherever q lies), ring_in / ring_out (candidates on the first or last row or
    column of their 64 x 64 tile whose q lies inside / outside that tile), rounds."""
    SH = SH8 if topo == 8 else SH4
    h, w = z.shape
    N = h * w
    vals, inv = np.unique(z, return_inverse=True)
    k = inv.reshape(h, w).astype(np.int64) + 1                      # order-preserving keys >= 1
    idx = np.arange(N, dtype=np.int64).reshape(h, w)
    OUT = np.int64(N)
    border = np.zeros((h, w), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    qk, qi = np.full((h, w), BIG), np.full((h, w), BIG)               # the lowest NEIGHBOUR in the (key, index) order
    for dy, dx in SH:
        kn, inn = shifted(k, dy, dx, BIG), shifted(idx, dy, dx, BIG)
        better = (kn < qk) | ((kn == qk) & (inn < qi))
        qk, qi = np.where(better, kn, qk), np.where(better, inn, qi)
    drains = (qk < k) | ((qk == k) & (qi < idx))
    ptr = np.where(drains, qi, idx)
    ptr[border] = OUT
    ptr = ptr.ravel()
    pits = np.flatnonzero(ptr == np.arange(N))
    q = qi.ravel()[pits]                                              # (a pit is no border cell: q exists)
    cand = ptr[q] != pits                                             # q does not point at p (a border q points outside)
    py, px, qy, qx = pits // w, pits % w, q // w, q % w
    T = 64
    intile = (py // T == qy // T) & (px // T == qx // T)
    ring = (py % T == 0) | (py % T == T - 1) | (px % T == 0) | (px % T == T - 1)
    take = cand & (intile if tile else True) & bool(dissolve)
    assert tile in (None, T)
    floor = k.ravel().copy()
    ptr = ptr.copy()
    ptr[pits[take]] = q[take]
    floor[pits[take]] = k.ravel()[q[take]]
    ext = np.append(ptr, OUT)
    while True:
        nxt = ext[ext]
        if (nxt == ext).all():
            break
        ext = nxt
    root = ext[:N]
    roots = np.flatnonzero(root == np.arange(N))
    assert np.array_equal(roots, pits[~take])                        # the forest's roots: the pits that stayed
    B = len(roots)
    rid = np.full(N + 1, -1, np.int64)
    rid[roots] = np.arange(B)
    rid[N] = B
    lab = rid[root].reshape(h, w)
    assert (lab >= 0).all()
    acc, rounds = contract(k, lab, B, SH)
    kk = np.maximum(floor.reshape(h, w), acc[lab])
    info = dict(pits=len(pits), dissolved=int(take.sum()), basins=B, candidates=int(cand.sum()),
                ring_in=int((cand & ring & intile).sum()), ring_out=int((cand & ring & ~intile).sum()), rounds=rounds)
    return vals[kk - 1], info


# ---- the rasters ------------------------------------------------------------------------------------------------------

def diagonal_pits(h, w):
    """The plane 2 y + 3 x (f32, exact) with pits dug along its diagonals.  A plane cell's lowest neighbour is NW (D8, 5
    below) or W (D4, 3 below); a pit is dug to 6 below its plane value, one below its NW neighbour, so q = NW (D4: W, level
    with q's own W neighbour, which comes first in the index order) and q never drains into it.  Pits: the cells with
    (x + y) % 3 == 0, every third cell of a diagonal, on the diagonals with (x - y) % 4 == 0 -- on EVERY diagonal two
    pits would touch across an anti-diagonal and the upper one drain into the lower.  Down such a diagonal the pointers run
    p -> q -> r -> p2 -> q2 ...: chains of dissolved pits, across rows, quads, wavefronts' row blocks and tiles.  Row 1 and
    column 1 hold pits beside the raster's border (their q is a border cell)."""
    y, x = np.mgrid[0:h, 0:w]
    z = (2 * y + 3 * x).astype(np.float32)
    pit = ((x + y) % 3 == 0) & ((x - y) % 4 == 0) & (y >= 1) & (y <= h - 2) & (x >= 1) & (x <= w - 2)
    z[pit] -= 6
    return z


def border_pit(h=9, w=7):
    """a plane falling to the west with ONE pit, in the second row: its q is a cell of the raster's first row"""
    y, x = np.mgrid[0:h, 0:w]
    z = (7 * y + 3 * x).astype(np.float32)
    z[1, 3] = z[0, 2] - 1                                             # below all eight neighbours; q = (0, 2) (D4: (0, 3))
    return z
