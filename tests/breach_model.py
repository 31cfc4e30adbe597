"""Depression breaching in numpy / plain Python: the serial algorithm of CompleteBreaching_Lindsay2016<D8>
(depressions/Lindsay2016.hpp:48-178) restated on a stable heap, and the closure form the engine computes
(csrc/breach.hip).  tests/test_breach_model.py pins the two against each other and against the compiled
reference's goldens; tests/test_breach_gpu.py checks the engine against this file.

Directions are the engine's D8 codes: 0 none, 1..8 index DX / DY, dir_nodata = the cell does not participate."""
from __future__ import annotations

import heapq

import numpy as np

DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
INV = (0, 5, 6, 7, 8, 1, 2, 3, 4)


def type_max(dtype):
    """what the reference's minimum over the neighbours starts at"""
    dtype = np.dtype(dtype)
    return np.finfo(dtype).max if dtype.kind == "f" else np.iinfo(dtype).max


# ---- stage 1: the pit pass -------------------------------------------------------------------------------------------
def pit_pass_serial(dem):
    """the reference's loop (:78-123), in raster order and in place: (raised DEM, pit mask)"""
    z = dem.copy()
    h, w = z.shape
    pits = np.zeros((h, w), np.uint8)
    top = type_max(z.dtype)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            lo = top
            for n in range(1, 9):
                v = z[y + DY[n], x + DX[n]]
                if v < lo:
                    lo = v
            if z[y, x] <= lo:
                z[y, x] = lo
                pits[y, x] = 1
    return z, pits


def _neighbour_min(planes, top):
    lo = np.full(planes[0].shape, top, planes[0].dtype)
    for p in planes:
        lo = np.minimum(lo, p)
    return lo


def pit_pass_local(dem):
    """the same as a stencil: d1 from the cell's ring, pit from d1 of the neighbours that precede the cell in raster order
    and z of those that follow"""
    z = dem
    h, w = z.shape
    d1 = z.copy()
    pits = np.zeros((h, w), np.uint8)
    if h < 3 or w < 3:
        return d1, pits
    top = type_max(z.dtype)
    c = z[1:-1, 1:-1]
    sh = lambda a, n: a[1 + DY[n]:h - 1 + DY[n], 1 + DX[n]:w - 1 + DX[n]]  # noqa: E731
    lo = _neighbour_min([sh(z, n) for n in range(1, 9)], top)
    d1[1:-1, 1:-1] = np.where(c < lo, lo, c)
    before = [n for n in range(1, 9) if DY[n] < 0 or (DY[n] == 0 and DX[n] < 0)]
    lo2 = _neighbour_min([sh(d1, n) if n in before else sh(z, n) for n in range(1, 9)], top)
    pits[1:-1, 1:-1] = c <= lo2
    return d1, pits


# ---- stage 2: the flood's tree ---------------------------------------------------------------------------------------
def flood_tree(d1):
    """Priority-Flood of d1 on a stable queue (elevation, then insertion order): edge cells seeded in raster order, a popped
    cell pushes its unvisited neighbours in the order 1..8.  Returns (dirs, pop order): dirs of an interior cell points at
    the cell that pushed it, edge cells hold 0."""
    h, w = d1.shape
    dirs = np.zeros((h, w), np.uint8)
    visited = np.zeros((h, w), bool)
    z = d1.tolist()
    heap, count, order = [], 0, []
    for y in range(h):
        for x in range(w):
            if y == 0 or x == 0 or y == h - 1 or x == w - 1:
                heap.append((z[y][x], count, y, x))
                count += 1
                visited[y, x] = True
    heapq.heapify(heap)
    vis = visited.tolist()
    dl = dirs.tolist()
    while heap:
        _, _, y, x = heapq.heappop(heap)
        order.append(y * w + x)
        for n in range(1, 9):
            ny, nx = y + DY[n], x + DX[n]
            if ny < 0 or nx < 0 or ny >= h or nx >= w or vis[ny][nx]:
                continue
            vis[ny][nx] = True
            dl[ny][nx] = INV[n]
            heapq.heappush(heap, (z[ny][nx], count, ny, nx))
            count += 1
    return np.array(dl, np.uint8).reshape(h, w), np.array(order, np.int64)


# ---- stage 3: the carve ------------------------------------------------------------------------------------------------
def links(dirs, dir_nodata=255):
    """flat index of every cell's link target, -1 where it has none (the engine's links: code 1..8, target inside the raster
    and participating)"""
    h, w = dirs.shape
    d = dirs.astype(np.int64)
    ok = (d >= 1) & (d <= 8) & (dirs != dir_nodata)
    dd = np.where(ok, d, 0)
    ys, xs = np.mgrid[0:h, 0:w]
    ty, tx = ys + np.array(DY)[dd], xs + np.array(DX)[dd]
    ok &= (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
    tyc, txc = np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)
    ok &= dirs[tyc, txc] != dir_nodata
    return np.where(ok, tyc * w + txc, -1).ravel()


def _keys(dem):
    """monotone integer keys of the engine's order (f32: the total order on the bits); NaN cells get None-like -1 mask"""
    if dem.dtype.kind == "f":
        b = dem.view(np.uint32).astype(np.int64)
        k = np.where(b >> 31, 0xFFFFFFFF - b, b + 0x80000000)
        return k.ravel(), np.isnan(dem).ravel()
    return dem.astype(np.int64).ravel(), np.zeros(dem.size, bool)


def carve_serial_walks(dem, dirs, pits, pop_order, dir_nodata=255):
    """the reference's walks (:138-153), one per pit in the order the pits are popped, each reading the DEM as the earlier
    walks left it.  A walk also stops where it meets a cell for the second time (a direction loop; the reference's tree has
    none).  Returns (final, path)."""
    key, nan = _keys(dem)
    key = key.copy()
    nxt = links(dirs, dir_nodata)
    part = (dirs != dir_nodata).ravel()
    out = dem.copy().ravel()
    path = np.zeros(dem.size, np.uint8)
    pm = pits.ravel()
    for c in pop_order:
        if not (pm[c] and part[c] and not nan[c]):
            continue
        level, val = key[c], out[c]
        seen, cc = set(), c
        while cc >= 0 and cc not in seen and not nan[cc] and key[cc] >= level:
            seen.add(cc)
            key[cc], out[cc], path[cc] = level, val, 1
            cc = nxt[cc]
    return out.reshape(dem.shape), path.reshape(dem.shape)


def breach_along(dem, dirs, pits, dir_nodata=255):
    """The contract of rdgpu_d8_breach_along as a closure: final(c) = the least dem(p) over the pits p with a chain of links
    p -> ... -> c on which every cell, c included, has dem >= dem(p); dem(c) without one.  Pits by rising level: a walk may
    stop at a cell an earlier (lower or equal) walk has taken, for that walk went on wherever this one could.
    Returns (final, path)."""
    key, nan = _keys(dem)
    nxt = links(dirs, dir_nodata)
    part = (dirs != dir_nodata).ravel()
    flat = dem.ravel()
    out = flat.copy()
    path = np.zeros(dem.size, np.uint8)
    pm = np.flatnonzero((pits.ravel() != 0) & part & ~nan)
    for c in pm[np.argsort(key[pm], kind="stable")]:
        level, val, cc = key[c], flat[c], c
        while cc >= 0 and not path[cc] and not nan[cc] and key[cc] >= level:
            out[cc], path[cc] = val, 1
            cc = nxt[cc]
    return out.reshape(dem.shape), path.reshape(dem.shape)


def breach_along_recurrence(dem, dirs, pits, dir_nodata=255):
    """The same on a FOREST (no loops) by the issue's recurrence, children before parents:
    M(c) = min(pit(c) ? dem(c) : inf, min over children k of [M(k) <= dem(c) ? M(k) : inf])."""
    key, nan = _keys(dem)
    nxt = links(dirs, dir_nodata)
    n = dem.size
    INF = 1 << 40
    part = (dirs != dir_nodata).ravel()
    M = np.where((pits.ravel() != 0) & part & ~nan, key, INF)
    src = np.arange(n)                                   # the cell whose value M is
    indeg = np.bincount(nxt[nxt >= 0], minlength=n)
    stack = list(np.flatnonzero(indeg == 0))
    while stack:
        c = stack.pop()
        t = nxt[c]
        if t < 0:
            continue
        if not nan[t] and M[c] <= key[t] and M[c] < M[t]:
            M[t], src[t] = M[c], src[c]
        indeg[t] -= 1
        if indeg[t] == 0:
            stack.append(t)
    flat = dem.ravel()
    out = np.where(M < INF, flat[src], flat)
    return out.reshape(dem.shape), (M < INF).astype(np.uint8).reshape(dem.shape)


# the composition law of the carve's steps: a step is g(x) = min(c, x if x <= a else inf) with c <= a
INF = float("inf")


def step(a, c):
    return lambda x: min(c, x if x <= a else INF)


def compose(first, second):
    """(a, c) of `second after first`"""
    (a1, c1), (a2, c2) = first, second
    return min(a1, a2), min(c2, c1 if c1 <= a2 else INF)


# ---- the whole thing ----------------------------------------------------------------------------------------------------
def canonical(dem):
    """the engine writes a zero of either sign as +0 (the reference compares -0 == +0)"""
    if dem.dtype.kind == "f":
        dem = dem.copy()
        dem[dem == 0] = 0
    return dem


def breach(dem):
    """CompleteBreaching_Lindsay2016<D8>: dict with d1, pits, dirs (the flood's tree), out, path"""
    h, w = dem.shape
    if h < 3 or w < 3:
        return {"d1": dem.copy(), "pits": np.zeros((h, w), np.uint8), "dirs": np.zeros((h, w), np.uint8), "out": dem.copy(),
                "path": np.zeros((h, w), np.uint8)}
    d1, pits = pit_pass_local(dem)
    d1 = canonical(d1)
    dirs, order = flood_tree(d1)
    out, path = breach_along(d1, dirs, pits)
    return {"d1": d1, "pits": pits, "dirs": dirs, "out": out, "path": path, "order": order}


def breach_serial(dem):
    """the reference's loops as they stand (:78-174): the pit pass in place, then ONE flood with the walks inside it, every
    key read from the DEM at push time"""
    h, w = dem.shape
    if h < 3 or w < 3:
        return dem.copy()
    zz, pits = pit_pass_serial(dem)
    z = canonical(zz).ravel().tolist()
    pm = pits.ravel().tolist()
    back = [-1] * (h * w)
    vis = [False] * (h * w)
    heap, count = [], 0
    for y in range(h):
        for x in range(w):
            if y == 0 or x == 0 or y == h - 1 or x == w - 1:
                heap.append((z[y * w + x], count, y, x))
                count += 1
                vis[y * w + x] = True
    heapq.heapify(heap)
    while heap:
        _, _, y, x = heapq.heappop(heap)
        c = y * w + x
        if pm[c]:
            cc, target = c, z[c]
            while cc != -1 and z[cc] >= target:
                z[cc] = target
                cc = back[cc]
        for n in range(1, 9):
            ny, nx = y + DY[n], x + DX[n]
            if ny < 0 or nx < 0 or ny >= h or nx >= w or vis[ny * w + nx]:
                continue
            vis[ny * w + nx] = True
            back[ny * w + nx] = c
            heapq.heappush(heap, (z[ny * w + nx], count, ny, nx))
            count += 1
    return np.array(z, dem.dtype).reshape(h, w)
