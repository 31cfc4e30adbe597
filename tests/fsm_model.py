"""Fill-Spill-Merge's contract (include/rdgpu.h, "fill-spill-merge") in plain numpy / Python, on top of the hierarchy of
tests/dephier_model.py: the gather of the water per leaf, the serial pour over the node table (iterative, with the
shortcut over full nodes), the lake tops, the closed-form level of every lake and the depth raster.

    r = fill_spill_merge(dem, labels, table, water)            # labels, table = dephier_model.hierarchy(dem, topology)
    r["depth"], r["node_water"], r["ocean"], r["standing"], r["water_in"], r["lakes"], r["full_lakes"], r["tops"]

`pour_naive` is the loop of the contract as it is written there, without the shortcut: the two must agree bit for bit."""
import numpy as np

from dephier_model import NONE

OCEAN = -2          # a shortcut's target: the rest of the water is lost


def _columns(table):
    return ([int(v) for v in table["parent"]], [int(v) for v in table["lchild"]], [int(v) for v in table["rchild"]],
            [int(v) for v in table["geolink"]], [float(v) for v in table["volume"]])


def pour(table, leaf_water, reverse=False, shortcut=True):
    """(w, ocean, stats): the state after pouring leaf_water[l] into every leaf l with water, ascending (or descending)."""
    par, lch, rch, geo, vol = _columns(table)
    count = len(par)
    w = [0.0] * count
    jump = [NONE] * count
    ocean = 0.0
    st = {"pours": 0, "longest_pour": 0, "shortcut_hits": 0}
    leaves = range(len(leaf_water))
    for leaf in (reversed(leaves) if reverse else leaves):
        x = float(leaf_water[leaf])
        if not x > 0:
            continue
        st["pours"] += 1
        n, hops, path = leaf, 0, []
        while True:
            if w[n] < vol[n]:
                cap = vol[n] - w[n]
                if x < cap:
                    w[n] += x
                    break
                w[n] = vol[n]
                x -= cap
            if x <= 0:
                break
            if shortcut and jump[n] != NONE:
                nxt = jump[n]
                st["shortcut_hits"] += 1
            else:
                p = par[n]
                if p == NONE:
                    nxt = OCEAN if geo[n] == NONE else geo[n]
                else:
                    s = rch[p] if lch[p] == n else lch[p]
                    if w[s] >= vol[s]:
                        if w[p] == 0:
                            w[p] = min(vol[p], vol[lch[p]] + vol[rch[p]])
                        nxt = p
                    else:
                        nxt = geo[n]
            path.append(n)
            n = nxt
            if n == OCEAN:
                ocean += x
                break
            hops += 1
        if shortcut:
            for m in path:
                jump[m] = n
        st["longest_pour"] = max(st["longest_pour"], hops)
    return np.array(w, np.float64), ocean, st


def pour_naive(table, leaf_water, reverse=False):
    return pour(table, leaf_water, reverse, shortcut=False)


def lake_tops(table, w):
    """top[n]: the highest ancestor-or-self of n that is a lake top, -1 for none (one descending pass)."""
    count = len(table)
    par = table["parent"]
    top = np.full(count, -1, np.int64)
    for n in range(count - 1, -1, -1):
        p = int(par[n])
        if p != NONE and top[p] >= 0:
            top[n] = top[p]
        elif w[n] > 0:
            top[n] = n
    return top


def fill_spill_merge(dem, labels, table, water, reverse=False, shortcut=True):
    dem = np.ascontiguousarray(dem)
    z = dem.astype(np.float64).ravel()
    lab = np.ascontiguousarray(labels).ravel().astype(np.int64)
    wat = np.ascontiguousarray(water, dtype=np.float64).ravel()
    assert np.isfinite(wat).all() and (wat >= 0).all()
    count = len(table)
    P = int(np.count_nonzero(table["lchild"] == NONE)) if count else 0
    inside = lab >= 0
    leaf_water = np.bincount(lab[inside], weights=wat[inside], minlength=P) if P else np.zeros(0)
    ocean0 = float(wat[~inside].sum())
    w, spilled, st = pour(table, leaf_water, reverse, shortcut)
    top = lake_tops(table, w)
    tops = np.flatnonzero(top == np.arange(count))
    full = w[tops] >= table["volume"][tops]
    level = np.where(full, table["level"][tops], -np.inf)
    # the partial lakes: the cells below the lake's spill level, by (dem, index)
    rank_of = np.full(count + 1, -1, np.int64)
    rank_of[tops] = np.arange(tops.size)
    cell_rank = np.where(inside, rank_of[top[np.maximum(lab, 0)]] if count else -1, -1)
    cr = np.maximum(cell_rank, 0)
    rec = (cell_rank >= 0) & ~full[cr] & (z < table["level"][tops][cr]) if tops.size else np.zeros(z.size, bool)
    cells = np.flatnonzero(rec)
    order = np.lexsort((cells, z[cells], cell_rank[cells]))
    cells = cells[order]
    seg = cell_rank[cells]
    starts = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]]) if cells.size else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], cells.size]
    for a, b in zip(starts, ends):
        r = int(seg[a])
        zs = z[cells[a:b]]
        k = np.arange(1, b - a + 1, dtype=np.float64)
        cand = (w[tops[r]] + np.cumsum(zs)) / k
        ok = cand <= np.r_[zs[1:], np.inf]
        level[r] = cand[int(np.argmax(ok))]
    h = np.where(cell_rank >= 0, level[cr] if tops.size else -np.inf, -np.inf)
    depth = np.where(z < h, h - z, 0.0)
    water_in = float(leaf_water.sum()) + ocean0
    return {"depth": depth.reshape(dem.shape), "node_water": w, "ocean": ocean0 + spilled, "water_in": water_in,
            "standing": float(depth.sum()), "lakes": int(tops.size), "full_lakes": int(np.count_nonzero(full)),
            "tops": tops, "level": level, "cell_level": h.reshape(dem.shape), "leaf_water": leaf_water, "records": int(cells.size), **st}
