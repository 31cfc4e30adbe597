"""The depression hierarchy with a caller-given ocean and BucketFillFromEdges, as include/rdgpu.h states them, in plain
numpy ("A CALLER-GIVEN OCEAN" and "bucket fill from the edges").

    labels, table = hierarchy(dem, topology, ocean)         # ocean: a mask of the DEM's shape, None = the border ring
    mask, filled = bucket_fill(check, value, mask, topology)

Only the descent differs from tests/dephier_model.py: a cell of the mask drains outside, every other cell -- the border
ring's included -- looks at the neighbours it has inside the raster.  hierarchy() puts that descent in the place of the
model's for the length of the call and runs the rest of the model unchanged."""
import numpy as np

import dephier_model as dm

NONE = dm.NONE
NODE_DTYPE = dm.NODE_DTYPE
canonical = dm.canonical
brute_cells_volume = dm.brute_cells_volume


def ring_mask(shape):
    m = np.zeros(shape, np.uint8)
    m[0, :] = m[-1, :] = 1
    m[:, 0] = m[:, -1] = 1
    return m


def golden_case_dem(G, case):
    """the DEM of case <raster>/<mask kind> of tests/golden/ref_dephier_ocean.npz: the raster's, with the hole of equal
    values of the nodata kind (restated from the recipe, make_golden_dephier_ocean.masks_of)"""
    name, kind = case.split("/")
    dem = G[name + "/dem"]
    if kind == "nodata":
        h, w = dem.shape
        hw, hh = (20, 15) if w >= 60 else (8, 6)
        dem = dem.copy()
        dem[h // 3:h // 3 + hh, w // 4:w // 4 + hw] = 65535 if dem.dtype == np.uint16 else -9999
    return dem


def leaves_of(dem, topology, ocean):
    """(leaf, pits) as dephier_model.leaves_of, for the ocean mask `ocean`"""
    h, w = dem.shape
    n = h * w
    rank = dm.cell_ranks(dem).reshape(h, w)
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    best_r, best_i = rank.copy(), idx.copy()
    for dy, dx in (dm._N8 if topology == 8 else dm._N4):
        # the cells (y, x) whose neighbour (y + dy, x + dx) lies inside the raster
        ys, yn = slice(max(0, -dy), h - max(0, dy)), slice(max(0, dy), h - max(0, -dy))
        xs, xn = slice(max(0, -dx), w - max(0, dx)), slice(max(0, dx), w - max(0, -dx))
        m = rank[yn, xn] < best_r[ys, xs]
        best_r[ys, xs] = np.where(m, rank[yn, xn], best_r[ys, xs])
        best_i[ys, xs] = np.where(m, idx[yn, xn], best_i[ys, xs])
    ptr = np.full(n + 1, n, np.int64)             # cell n: the outside
    ptr[:n] = np.where(np.asarray(ocean).ravel() != 0, n, best_i.ravel())
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


def hierarchy(dem, topology=8, ocean=None):
    dem = np.ascontiguousarray(dem)
    if ocean is None:
        ocean = ring_mask(dem.shape)
    ocean = np.asarray(ocean)
    assert ocean.shape == dem.shape
    if not ocean.any():
        raise ValueError("no ocean cells")
    saved = dm.leaves_of
    dm.leaves_of = lambda d, t: leaves_of(d, t, ocean)
    try:
        return dm.hierarchy(dem, topology)
    finally:
        dm.leaves_of = saved


def bucket_fill(check, value, mask=None, topology=8):
    """(mask after the fill as uint8, number of bytes set): connected components of the eligible cells (scipy), those
    with a cell on the border ring"""
    from scipy import ndimage

    check = np.asarray(check)
    out = np.zeros(check.shape, np.uint8) if mask is None else np.array(mask, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        elig = (check == check.dtype.type(value)) & (out == 0)
    lab, _ = ndimage.label(elig, structure=np.ones((3, 3), int) if topology == 8 else None)
    ring = ring_mask(check.shape).astype(bool)
    hit = np.unique(lab[ring & elig])
    new = elig & np.isin(lab, hit)
    out[new] = 1
    return out, int(np.count_nonzero(new))
