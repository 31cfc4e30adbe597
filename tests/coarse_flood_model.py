"""numpy model of the COARSE FLOOD ahead of the fill's pair pass (k_flag_tiles and k_pairs_flooded
in csrc/fill.hip), and the rasters of test_fill_coarse_flood_model.py / test_fill_coarse_flood_gpu.py.  Not a test module.

Lemma A.  Cut the raster into CB x CB blocks anchored at (0, 0), m = the blocks' minima over their in-raster cells, LB = the
fill of m under the same topology.  Adjacent cells lie in one block or in adjacent blocks (D4-adjacent for D4) and a border
cell lies in a border block, so a path to the border maps to a path of blocks whose maximum is not larger:
LB(block(c)) <= W(c).  An interior 64 x 64 descent tile whose blocks all have LB above the tile's largest cell is wholly
and strictly raised: FLAGGED.  A flagged tile is one of flooded_tiles_model's; the converse does not hold.

Lemma B.  In the basin graph an edge below L between two basins that both end at level L never decides a level.  So a
flagged tile's pairs (all of them below its lake's level L, between basins that end at L) may be replaced by
  a star:  (R, p, K) for R one basin of the tile, every other basin p of the tile's cells, K = the tile's largest key, and
  a ring:  (R, basin(b), max(K, key(b))) for every cell b outside the tile that the tile's forward scan (E, SE, S, SW;
           D4: E, S) meets -- the true weight where key(b) >= L, and below L on both sides where not.
levels_with_flags() does that on pairs_model's descent forest and solves the minimax levels; with no tile flagged it is
the plain fill."""
import numpy as np

import flooded_tiles_model as fm
import pairs_model as pairs
import pit_dissolve_model as pm

T = 64
BLOCKS = (16, 64)   # the block sizes measured at full size; the engine uses rd.fill_coarse_block()


def keys(z):
    """(vals, k): order-preserving integer keys >= 1 of the raster's cells, vals[k - 1] == z"""
    vals, inv = np.unique(z, return_inverse=True)
    return vals, inv.reshape(z.shape).astype(np.int64) + 1


def block_minima(z, CB):
    """minima of the CB x CB blocks over their in-raster cells (the last blocks may be partial), in z's type"""
    h, w = z.shape
    nby, nbx = -(-h // CB), -(-w // CB)
    top = np.inf if np.issubdtype(z.dtype, np.floating) else np.iinfo(z.dtype).max
    p = np.full((nby * CB, nbx * CB), top, z.dtype)
    p[:h, :w] = z
    return p.reshape(nby, CB, nbx, CB).min(axis=(1, 3))


def interior_tiles(shape):
    """bool per 64 x 64 descent tile: the tile holds no border cell and does not hang over the raster's end"""
    h, w = shape
    ty, tx = np.arange(-(-h // T)) * T, np.arange(-(-w // T)) * T
    return ((ty >= 1) & (ty + T <= h - 1))[:, None] & ((tx >= 1) & (tx + T <= w - 1))[None, :]


def tile_maxima(z):
    """the largest cell of every interior tile (z's type; whatever elsewhere)"""
    h, w = z.shape
    out = np.zeros((-(-h // T), -(-w // T)), z.dtype)
    for ty, tx in zip(*np.nonzero(interior_tiles(z.shape))):
        out[ty, tx] = z[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T].max()
    return out


def lower_bound(z, CB, topo, fill):
    """LB, the fill of the block minima (a coarse raster with a side <= 2 is all border: LB = m)"""
    return fill(np.ascontiguousarray(block_minima(z, CB)), topo)


def flags(z, CB, topo, fill):
    """bool per descent tile: interior, and the minimum of LB over the tile's blocks lies above the tile's largest cell.
    fill(raster, topo): the oracle's.  No tile is flagged where the coarse raster has a side <= 2."""
    assert T % CB == 0
    h, w = z.shape
    inner = interior_tiles(z.shape)
    out = np.zeros(inner.shape, bool)
    if -(-h // CB) <= 2 or -(-w // CB) <= 2:
        return out
    LB = lower_bound(z, CB, topo, fill)
    tmax = tile_maxima(z)
    k = T // CB
    for ty, tx in zip(*np.nonzero(inner)):
        out[ty, tx] = LB[ty * k:(ty + 1) * k, tx * k:(tx + 1) * k].min() > tmax[ty, tx]
    return out


def census(z, W):
    """bool per descent tile: interior and every cell strictly raised (flooded_tiles_model's tiles)"""
    out = np.zeros(interior_tiles(z.shape).shape, bool)
    for y0, x0, lo, hi in fm.flooded_levels(z, W):
        out[y0 // T, x0 // T] = True
    return out & interior_tiles(z.shape)


def ring_cells(y0, x0, topo):
    """(y, x) of the cells outside tile (y0, x0) that its forward scan meets"""
    if topo == 4:
        return [(y, x0 + T) for y in range(y0, y0 + T)] + [(y0 + T, x) for x in range(x0, x0 + T)]
    return ([(y, x0 + T) for y in range(y0, y0 + T + 1)] + [(y0 + T, x) for x in range(x0 - 1, x0 + T)]
            + [(y, x0 - 1) for y in range(y0 + 1, y0 + T)])


def _minimax_levels(B, a, b, wgt):
    """level of every basin 0 .. B - 1 (B: the outside, level 0): the smallest over paths to the outside of the largest
    weight on the path.  Kruskal: a component gets its level when it meets the outside's."""
    order = np.argsort(wgt, kind="stable")
    par = np.arange(B + 1)
    members = [[i] for i in range(B)] + [None]           # (the outside's component keeps no list)
    level = np.zeros(B + 1, np.int64)

    def find(x):
        r = x
        while par[r] != r:
            r = par[r]
        while par[x] != r:
            par[x], x = r, par[x]
        return r

    for i in order:
        ra, rb = find(a[i]), find(b[i])
        if ra == rb:
            continue
        out_r = find(B)
        if rb == out_r:
            ra, rb = rb, ra
        if ra == out_r:                                   # rb's basins drain at this weight
            level[members[rb]] = wgt[i]
            members[rb] = None
            par[rb] = ra
            continue
        if len(members[ra]) < len(members[rb]):
            ra, rb = rb, ra
        members[ra].extend(members[rb])
        members[rb] = None
        par[rb] = ra
    assert all(m is None for m in members), "a basin never met the outside"
    return level


def levels_with_flags(z, topo, flagged, pick=0, ring_key=True):
    """(filled raster, info): the fill by the basin graph of pairs_model's forest in which every flagged tile's own pairs are
    replaced by its star and its ring.  pick: which of the tile's basins is R (an index into their sorted list, modulo).
    ring_key=False weighs a ring record K alone: WRONG where key(b) is above the level (the tests' negative control).
    info: basins, records dropped and added, the largest number of distinct basins in a flagged tile."""
    SH = [(0, 1), (1, 1), (1, 0), (1, -1)] if topo == 8 else [(0, 1), (1, 0)]
    h, w = z.shape
    vals, k = keys(z)
    ptr, lab = pairs.forest(z, topo)
    N = h * w
    B = int(lab.max())                                     # (border cells drain off the raster: the outside's label)
    assert lab[0, 0] == B
    kf = np.append(k.ravel(), 0)
    floor = np.maximum(k.ravel(), kf[np.minimum(ptr, N)]).reshape(h, w)   # a dissolved pit keeps its neighbour's key
    ty, tx = np.mgrid[0:h, 0:w]
    own_flagged = flagged[ty // T, tx // T]
    ea, eb, ew = [], [], []
    dropped = 0
    for dy, dx in SH:
        ln, kn = pm.shifted(lab, dy, dx, -1), pm.shifted(k, dy, dx, 0)
        m = (ln >= 0) & (ln != lab)
        dropped += int((m & own_flagged).sum())
        m &= ~own_flagged
        ea.append(lab[m]); eb.append(ln[m]); ew.append(np.maximum(k, kn)[m])
    added, most = 0, 0
    for t_y, t_x in zip(*np.nonzero(flagged)):
        y0, x0 = t_y * T, t_x * T
        own = np.unique(lab[y0:y0 + T, x0:x0 + T])
        assert B not in own                                # an interior tile holds no border cell
        most = max(most, len(own))
        K = int(k[y0:y0 + T, x0:x0 + T].max())
        R = own[pick % len(own)]
        star = own[own != R]
        ea.append(np.full(len(star), R)); eb.append(star); ew.append(np.full(len(star), K))
        rc = np.array(ring_cells(y0, x0, topo))
        rl, rk = lab[rc[:, 0], rc[:, 1]], k[rc[:, 0], rc[:, 1]]
        keep = rl != R
        ea.append(np.full(int(keep.sum()), R)); eb.append(rl[keep]); ew.append(np.maximum(K, rk[keep]) if ring_key else np.full(int(keep.sum()), K))
        added += len(star) + int(keep.sum())
    a, b, wgt = np.concatenate(ea), np.concatenate(eb), np.concatenate(ew)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    pair = lo * (B + 1) + hi                               # the lowest pass per pair of basins
    o = np.lexsort((wgt, pair))
    first = np.ones(len(o), bool)
    first[1:] = pair[o][1:] != pair[o][:-1]
    sel = o[first]
    level = _minimax_levels(B, lo[sel], hi[sel], wgt[sel])
    kk = np.maximum(floor, level[lab])
    W = np.where(kk > k, vals[kk - 1], z)
    return W, dict(basins=B, dropped=dropped, added=added, most_basins_in_a_flagged_tile=most)


# ---- the rasters ------------------------------------------------------------------------------------------------------
# A lake that the COARSE fill holds needs a wall that fills whole blocks: the thick bowl's wall band is the ring of blocks
# one block in from the raster's border.  Its sizes are such that whole tiles lie inside the band.

def size(CB):
    """edge of the square thick bowl: 256 at CB = 16 (4 inner tiles), 448 at CB = 64 (9)"""
    return 256 if CB == 16 else 64 * 5 + 2 * CB


def band(h, w, CB):
    """bool per cell: the ring of whole blocks one block in from the raster's first row and column and from its last WHOLE
    block row and column (what hangs over lies outside the wall)"""
    hb, wb = h // CB * CB, w // CB * CB
    b = np.zeros((h, w), bool)
    b[CB:hb - CB, CB:wb - CB] = True
    b[2 * CB:hb - 2 * CB, 2 * CB:wb - 2 * CB] = False
    return b


def thick_bowl(CB, h=None, w=None, level=10.0, seed=2):
    """low relief in [0, 0.875) under a wall band at `level`"""
    h, w = h or size(CB), w or size(CB)
    z = fm._smooth(h, w, seed)
    z[band(h, w, CB)] = np.float32(level)
    return z


def inner_tiles(h, w, CB):
    """bool per descent tile: the tile lies wholly inside the band (neither in it nor outside it)"""
    ty, tx = np.arange(-(-h // T)) * T, np.arange(-(-w // T)) * T
    hb, wb = h // CB * CB, w // CB * CB
    return ((ty >= 2 * CB) & (ty + T <= hb - 2 * CB))[:, None] & ((tx >= 2 * CB) & (tx + T <= wb - 2 * CB))[None, :]


def spill_on_ring(CB, where):
    """a thick bowl whose band begins right behind the last inner tile (edge 64 m + 2 CB), with a channel of 9s through
    the band that starts on that tile's ring: beside its right column ("east"), below its last row ("south"), at its SW
    corner ("southwest").  The lake spills there, at 9: the ring record is the spill."""
    n = 64 * 3 + 2 * CB if CB == 16 else size(CB)
    z = thick_bowl(CB, n, n)
    y0 = x0 = n - 2 * CB - T                                  # the last inner tile
    assert inner_tiles(n, n, CB)[y0 // T, x0 // T] and y0 % T == 0
    if where == "east":
        z[y0 + 20, x0 + T:x0 + T + CB] = 9
    elif where == "south":
        z[y0 + T:y0 + T + CB, x0 + 20] = 9
    else:
        z[y0 + T:y0 + T + CB, x0 - 1] = 9
    return z


def two_thick_lakes(CB):
    """two tiles more across: a lake at 10 on the left, one at 20 on the right, and between them a wall of 30 one cell wide
    down the first column of a tile.  The blocks do not see that wall (LB is 10 on both sides), the tiles on either side of
    the wall's tile are flagged, and the ring of the left one is the wall."""
    h, w = size(CB), size(CB) + 2 * T
    z = thick_bowl(CB, h, w, seed=5)
    xw = (2 * CB + T - 1) // T * T + 2 * T                    # first column of the third tile inside the band
    b = band(h, w, CB)
    right = np.zeros((h, w), bool)
    right[:, xw:] = True
    z[b & right] = 20
    z[CB:h - CB, xw] = 30
    return z, xw


def level_ring(CB, kind):
    """the thick bowl with a cell AT the lake's level (not raised) in the first column of the second inner tile, on the ring of
    the first: "at" -- the cell alone; "island" -- cells of 11 beside it; "minus zero" -- the lake at +0.0, the cell -0.0"""
    n = size(CB)
    t0 = (2 * CB + T - 1) // T * T                            # the first inner tile's origin
    y, x = t0 + 20, t0 + T
    if kind == "minus zero":
        z = fm._smooth(n, n, 2) - np.float32(2.0)
        outside = np.ones((n, n), bool)
        outside[CB:n - CB, CB:n - CB] = False
        z[outside] -= 4
        z[band(n, n, CB)] = np.float32(0.0)
        z[y, x] = np.float32(-0.0)
        assert np.signbit(z[y, x]) and not np.signbit(z[CB, CB])
        return z
    z = thick_bowl(CB)
    z[y, x] = 10
    if kind == "island":
        z[y - 1:y + 2, x + 1:x + 3] = 11
    return z


def many_nodes_thick(CB, seed=9):
    """white noise under the level over the first inner tile and twelve cells beyond: every few cells a basin of its own"""
    z = thick_bowl(CB)
    t0 = (2 * CB + T - 1) // T * T
    z[t0:t0 + 76, t0:t0 + 76] = np.random.default_rng(seed).random((76, 76), dtype=np.float32)
    return z


def dissolved_under_thick_wall(CB):
    """the diagonal-pit plane (pit_dissolve_model) under the thick wall above its highest cell"""
    n = size(CB)
    z = pm.diagonal_pits(n, n)
    z[band(n, n, CB)] = np.float32(4000.0)
    return z


def typed_thick_bowl(CB, dtype):
    """the thick bowl in an integer type (relief 0..39 under a wall of 60; signed types 90 lower, below zero throughout)"""
    n = size(CB)
    z = np.floor(fm._smooth(n, n, 4).astype(np.float64) * 45.0).astype(np.int64)
    z[band(n, n, CB)] = 60
    if np.issubdtype(dtype, np.signedinteger):
        z -= 90
    return z.astype(dtype)


def rasters(CB):
    """name -> (raster, flagged tiles it must show under D8 and D4 alike)"""
    n = size(CB)
    n_in = int(inner_tiles(n, n, CB).sum())
    ns = 64 * 3 + 2 * CB if CB == 16 else n                   # (spill_on_ring's edge)
    n_spill = int(inner_tiles(ns, ns, CB).sum())
    lakes, xw = two_thick_lakes(CB)
    in_lakes = inner_tiles(*lakes.shape, CB)
    n_lakes = int(in_lakes.sum() - in_lakes[:, xw // T].sum())   # (the wall's tiles hold cells above their lake)
    d = {
        "thick bowl": (thick_bowl(CB), n_in),
        "thin wall": (fm.bowl(), 0),                           # flooded_tiles_model's: census 1, its rim blocks hold outside cells
        "spill east": (spill_on_ring(CB, "east"), n_spill),
        "spill south": (spill_on_ring(CB, "south"), n_spill),
        "spill southwest": (spill_on_ring(CB, "southwest"), n_spill),
        "two lakes": (lakes, n_lakes),
        "ring at level": (level_ring(CB, "at"), n_in - 1),
        "ring island": (level_ring(CB, "island"), n_in - 1),
        "ring minus zero": (level_ring(CB, "minus zero"), n_in - 1),
        "many nodes": (many_nodes_thick(CB), n_in),
        "dissolved pits": (dissolved_under_thick_wall(CB), n_in),
        "odd 262 x 259": (thick_bowl(CB, size(CB) + 3, size(CB) + 6), n_in),
        "odd width 258": (thick_bowl(CB, size(CB), size(CB) + 2), n_in),
        "border tiles": (thick_bowl(16, 128, 128), 0),         # a lake the blocks hold, and every tile touches the border
    }
    for t in fm.INT_TYPES:
        d["thick bowl " + np.dtype(t).name] = (typed_thick_bowl(CB, t), n_in)
    return d


# the fractals (richdem_amd.synth.fractal_dem): (width, height, seed) -> ({CB: flagged tiles}, census or None), D8
FRACTALS = {
    (2048, 2048, 3): ({16: 110, 64: 80}, 121),
    (2048, 2048, 11): ({16: 44, 64: 31}, 54),
    (1536, 1536, 3): ({16: 3, 64: 2}, None),
    (1030, 770, 3): ({16: 0, 64: 0}, None),
}
