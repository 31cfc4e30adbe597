"""Expected values for D-infinity across flats (include/rdgpu.h "D-infinity across flats"), composed from what the
CPU oracle offers: FM_Tarboton gives the base and -- run once on a raster of 3 x 3 blocks -- the facet rule on the patched
cells' windows of flat_mask; resolve_flats gives the D8 directions before flats, the mask and the labels.  What this module
adds is the substitution of the neighbours of another flat and the fallback to the first lower neighbour of the same flat.

Proportions layout [h, w, 9]: slot 0 is the marker (-2 NoData, -1 no flow, 0 flow), slots 1..8 the shares to the neighbours
1 left, 2 up-left, 3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left."""
import numpy as np

DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
OTHER = np.int32(np.iinfo(np.int32).min)      # stands for a neighbour of another flat: the NoData value of the windows
STAT_KEYS = ("noflow_cells", "patched_cells", "fallback_cells", "unresolved_cells")


def compose_from(orc, base, d8, mask, labels):
    """(props, info) from FM_Tarboton's proportions `base` and resolve_flats' (d8 before flats, flat_mask, labels).
    info: the four counts of rdgpu_dinf_flats_stats, the boolean raster `patched`, and how many patched cells ended with
    two receivers / one receiver from a facet."""
    h, w = d8.shape
    props = base.copy()
    interior = np.zeros((h, w), bool)
    interior[1:-1, 1:-1] = True
    patched = (d8 == 0) & (labels != 0)
    assert not (patched & ~interior).any(), "an edge cell always has a D8 direction"
    assert (base[..., 0][patched] == -1.0).all(), "a cell without a lower neighbour has no descending facet"
    info = {"noflow_cells": int(((base[..., 0] == -1.0) & interior).sum()), "patched_cells": int(patched.sum()),
            "fallback_cells": 0, "unresolved_cells": 0, "patched": patched, "two_receivers": 0, "one_receiver": 0}
    ys, xs = np.nonzero(patched)
    n = len(ys)
    if n == 0:
        return props, info
    oy, ox = np.mgrid[-1:2, -1:2]
    wy, wx = ys[:, None, None] + oy, xs[:, None, None] + ox                      # [n, 3, 3]
    win = mask[wy, wx].astype(np.int32)
    assert (win >= 0).all()
    win[labels[wy, wx] != labels[ys, xs][:, None, None]] = OTHER
    blocks = np.ascontiguousarray(win.transpose(1, 0, 2).reshape(3, 3 * n))     # block k: columns 3k .. 3k + 2
    facet = orc.port.fm_tarboton(blocks, OTHER)[1, 1::3]                         # the block centres: interior cells
    assert facet.shape == (n, 9) and (facet[:, 0] != -2.0).all()
    center = win[:, 1, 1]
    lower = np.stack([(win[:, 1 + DY[m], 1 + DX[m]] != OTHER) & (win[:, 1 + DY[m], 1 + DX[m]] < center) for m in range(1, 9)], axis=1)
    dry = facet[:, 0] == -1.0                                                    # no facet descends:
    served = dry & lower.any(axis=1)                                             # everything to the first lower neighbour
    rows = facet.copy()
    k = np.nonzero(served)[0]
    rows[k, 0] = 0.0
    rows[k, 1 + np.argmax(lower[k], axis=1)] = 1.0
    info["fallback_cells"] = int(served.sum())
    info["unresolved_cells"] = int((dry & ~served).sum())
    nrecv = (facet[:, 1:] > 0).sum(axis=1)
    info["two_receivers"], info["one_receiver"] = int((nrecv == 2).sum()), int((nrecv == 1).sum())
    props[ys, xs] = rows
    return props, info


def compose(orc, dem, nodata):
    dem = np.ascontiguousarray(dem)
    d8, mask, labels = orc.port.resolve_flats(dem, nodata)
    return compose_from(orc, orc.port.fm_tarboton(dem, nodata), d8, mask, labels)


def stats_of(info):
    return {k: info[k] for k in STAT_KEYS}


def random_integer_dem(orc, seed, width=97, height=71, levels=12):
    """random integer elevations after the oracle's fill: narrow and wide lakes all over the raster"""
    z = np.random.default_rng(seed).integers(0, levels, (height, width)).astype(np.float32)
    return orc.port.fill(z)
