"""The depression hierarchy's contract (include/rdgpu.h, "depression hierarchy") in plain numpy / Python: the descent
by (value, index), the leaf labels, the minimum edge per pair of leaves, a serial Kruskal with the outside as a node, and
the cells and volumes of every node, exact (the volume is the correctly rounded exact sum for every element type).

    labels, table = hierarchy(dem, topology)

`table` is a structured array of NODE_DTYPE, the mirror of rdgpu_dephier_node.  `canonical(...)` is the form in which a
tree is compared with the reference's, whose order among outlets that share a saddle cell is arbitrary."""
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF
NODE_DTYPE = np.dtype([("parent", np.uint32), ("lchild", np.uint32), ("rchild", np.uint32), ("pit_cell", np.uint32),
                       ("inside_cell", np.uint32), ("outside_cell", np.uint32), ("geolink", np.uint32),
                       ("cells", np.uint32), ("level", np.float64), ("pit_elevation", np.float64),
                       ("volume", np.float64)])
assert NODE_DTYPE.itemsize == 56

_N8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]       # (dy, dx)
_N4 = [(-1, 0), (0, -1), (0, 1), (1, 0)]


def cell_ranks(dem):
    """rank[c]: the position of cell c in the strict total order by (value, raster index)."""
    flat = np.ascontiguousarray(dem).ravel()
    if flat.dtype.kind == "f":
        flat = flat + flat.dtype.type(0)          # -0.0 is 0.0
    order = np.argsort(flat, kind="stable")
    rank = np.empty(flat.size, np.int64)
    rank[order] = np.arange(flat.size)
    return rank


def leaves_of(dem, topology):
    """(leaf, pits): leaf[c] = the leaf id of the pit c descends to, -1 for the outside; pits = the pit cells."""
    h, w = dem.shape
    n = h * w
    rank = cell_ranks(dem).reshape(h, w)
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    ptr = np.full(n + 1, n, np.int64)             # cell n: the outside
    if h > 2 and w > 2:
        best_r = rank[1:-1, 1:-1].copy()
        best_i = idx[1:-1, 1:-1].copy()
        for dy, dx in (_N8 if topology == 8 else _N4):
            r = rank[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
            i = idx[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
            m = r < best_r
            best_r = np.where(m, r, best_r)
            best_i = np.where(m, i, best_i)
        ptr[idx[1:-1, 1:-1].ravel()] = best_i.ravel()
    while True:
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            break
        ptr = nxt
    root = ptr[:n]
    pits = np.flatnonzero(root == np.arange(n))
    lid = np.full(n + 1, -1, np.int64)
    lid[pits] = np.arange(pits.size)
    return lid[root], pits


def leaf_edges(dem, topology, leaf, P):
    """The minimum edge of every pair of adjacent leaves, in ascending key: arrays (hi, lo) of cells."""
    h, w = dem.shape
    rank = cell_ranks(dem)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    fwd = [(0, 1), (1, -1), (1, 0), (1, 1)] if topology == 8 else [(0, 1), (1, 0)]
    A, B = [], []
    for dy, dx in fwd:
        ys = slice(0, h - dy)
        xa = slice(max(0, -dx), w - max(0, dx))
        xb = slice(max(0, dx), w - max(0, -dx))
        A.append(idx[ys, xa].ravel())
        B.append(idx[dy:h, xb].ravel())
    a, b = np.concatenate(A), np.concatenate(B)
    la, lb = leaf[a], leaf[b]
    m = la != lb
    a, b, la, lb = a[m], b[m], la[m], lb[m]
    up = rank[a] > rank[b]
    hi, lo = np.where(up, a, b), np.where(up, b, a)
    la, lb = np.where(la < 0, P, la), np.where(lb < 0, P, lb)
    pair = np.minimum(la, lb) * (P + 1) + np.maximum(la, lb)
    o = np.lexsort((lo, rank[hi], pair))
    hi, lo, pair = hi[o], lo[o], pair[o]
    first = np.ones(pair.size, bool)
    first[1:] = pair[1:] != pair[:-1]
    hi, lo = hi[first], lo[first]
    o = np.lexsort((lo, rank[hi]))
    return hi[o], lo[o]


def exact_values(dem):
    """(Z, scale): dem[c] == Z[c] * scale exactly, Z integers (Python ints for floats), scale a Fraction."""
    flat = np.ascontiguousarray(dem).ravel()
    if flat.dtype.kind in "iu":
        return flat.astype(np.int64), Fraction(1)
    assert flat.dtype == np.float32
    bits = flat.view(np.uint32).astype(np.int64)
    e = (bits >> 23) & 0xFF
    man = bits & 0x7FFFFF
    man = np.where(e > 0, man | 0x800000, man)
    e = np.where(e > 0, e, 1)                    # value = man * 2^(e - 150)
    sign = np.where(bits >> 31, -1, 1)
    emin = int(e.min())
    Z = np.array([int(s) * (int(m) << (int(x) - emin)) for s, m, x in zip(sign, man, e)], dtype=object)
    return Z, Fraction(2) ** (emin - 150)


def hierarchy(dem, topology=8):
    dem = np.ascontiguousarray(dem)
    h, w = dem.shape
    n = h * w
    leaf, pits = leaves_of(dem, topology)
    labels = leaf.reshape(h, w).astype(np.int32)
    P = pits.size
    if P == 0:
        return labels, np.zeros(0, NODE_DTYPE)
    rank = cell_ranks(dem)
    hi, lo = leaf_edges(dem, topology, leaf, P)
    # Kruskal, the outside as set P
    uf = list(range(P + 1))
    top = list(range(P + 1))

    def find(x):
        r = x
        while uf[r] != r:
            r = uf[r]
        while uf[x] != r:
            uf[x], x = r, uf[x]
        return r

    parent, lch, rch = [NONE] * P, [NONE] * P, [NONE] * P
    pit = [int(p) for p in pits]
    inside, outside, spill_hi = [NONE] * P, [NONE] * P, [NONE] * P
    for k in range(hi.size):
        ch, cl = int(hi[k]), int(lo[k])
        a, b = int(leaf[ch]), int(leaf[cl])
        ra, rb = find(P if a < 0 else a), find(P if b < 0 else b)
        if ra == rb:
            continue
        out = find(P)
        if ra == out or rb == out:
            r, cin, cout = (rb, cl, ch) if ra == out else (ra, ch, cl)
            A = top[r]
            inside[A], outside[A], spill_hi[A] = cin, cout, ch
            uf[r] = out
            continue
        A, B = top[ra], top[rb]
        N = len(parent)
        inside[A], outside[A], spill_hi[A] = ch, cl, ch
        inside[B], outside[B], spill_hi[B] = cl, ch, ch
        parent[A] = parent[B] = N
        first = A if rank[pit[A]] < rank[pit[B]] else B
        parent.append(NONE)
        lch.append(first)
        rch.append(B if first == A else A)
        pit.append(pit[first])
        inside.append(NONE)
        outside.append(NONE)
        spill_hi.append(NONE)
        uf[rb] = ra
        top[ra] = N
    count = len(parent)
    assert all(s != NONE for s in spill_hi), "a set never reached the outside"
    par = np.array([-1 if p == NONE else p for p in parent], np.int64)
    sh = np.array(spill_hi, np.int64)
    flat = dem.ravel()
    vals = flat.astype(np.float64)               # exact for every supported element type
    lv = vals[sh]
    # charge every cell to its first ancestor-or-self whose level is not below it (levels do not fall towards the root)
    depth = np.zeros(count, np.int64)
    for v in range(count - 1, -1, -1):
        if par[v] >= 0:
            depth[v] = depth[par[v]] + 1
    ups = [par]
    while (1 << len(ups)) < int(depth.max()) + 1:
        p = ups[-1]
        ups.append(np.where(p >= 0, p[np.maximum(p, 0)], -1))
    cells_in = np.flatnonzero(leaf >= 0)
    v = leaf[cells_in].copy()
    zc = vals[cells_in]
    below = lv[v] < zc
    for p in reversed(ups):
        u = p[v]
        ok = below & (u >= 0) & (lv[np.maximum(u, 0)] < zc)
        v = np.where(ok, u, v)
    v = np.where(below, par[v], v)
    ch_cells, ch_node = cells_in[v >= 0], v[v >= 0]
    Z, scale = exact_values(dem)
    mc = np.bincount(ch_node, minlength=count).astype(np.int64)
    if Z.dtype == object:
        sz = [0] * count
        for c, m in zip(ch_cells.tolist(), ch_node.tolist()):
            sz[m] += Z[c]
    else:
        acc = np.zeros(count, np.int64)
        np.add.at(acc, ch_node, Z[ch_cells])
        sz = [int(x) for x in acc]
    tc = [int(x) for x in mc]
    for m in range(P, count):
        tc[m] += tc[lch[m]] + tc[rch[m]]
        sz[m] += sz[lch[m]] + sz[rch[m]]
    table = np.zeros(count, NODE_DTYPE)
    table["parent"], table["lchild"], table["rchild"] = parent, lch, rch
    table["pit_cell"], table["inside_cell"], table["outside_cell"] = pit, inside, outside
    g = leaf[np.array(outside, np.int64)]
    table["geolink"] = np.where(g < 0, NONE, g).astype(np.uint32)
    table["cells"] = tc
    table["level"] = lv
    table["pit_elevation"] = vals[np.array(pit, np.int64)]
    table["volume"] = [float((tc[m] * int(Z[sh[m]]) - sz[m]) * scale) for m in range(count)]
    return labels, table


def brute_cells_volume(dem, labels, table):
    """cells and volume of every node straight from their definition (small rasters only): (cells, volume as Fraction)."""
    flat = np.ascontiguousarray(dem).ravel()
    lab = labels.ravel()
    P = int(np.count_nonzero(table["lchild"] == NONE))
    under = [None] * len(table)
    for m in range(len(table)):
        under[m] = {m} if m < P else under[int(table["lchild"][m])] | under[int(table["rchild"][m])]
    out = []
    for m in range(len(table)):
        L = Fraction(float(table["level"][m]))
        sel = [Fraction(float(flat[c])) for c in range(flat.size) if int(lab[c]) in under[m] and Fraction(float(flat[c])) <= L]
        out.append((len(sel), sum((L - z for z in sel), Fraction(0))))
    return out


def canonical(parent, lchild, rchild, pit_cell, level, cells, volume):
    """The tree with every internal node dissolved whose own level equals the level it was created at (its children's
    level): the set of (frozenset of leaf pit cells, level, cells, volume, is top-level) over the leaves and the
    remaining internal nodes, and the number of internal nodes dissolved.  Ids must have child < parent."""
    count = len(parent)
    none = {NONE, -1}
    pits = [None] * count
    kept = set()
    dissolved = 0
    for m in range(count):
        leafnode = int(lchild[m]) in none
        pits[m] = frozenset([int(pit_cell[m])]) if leafnode else pits[int(lchild[m])] | pits[int(rchild[m])]
        if not leafnode and level[m] == level[int(lchild[m])]:
            dissolved += 1
            continue
        # top-level: nothing kept lies above it
        p, is_top = int(parent[m]), True
        while p not in none:
            if level[p] != level[int(lchild[p])]:
                is_top = False
                break
            p = int(parent[p])
        kept.add((pits[m], float(level[m]), int(cells[m]), float(volume[m]), is_top))
    return kept, dissolved
