"""Rasters whose towards-lower breadth-first levels end at a chosen depth D around the 16-bit limit of the plane engine
(csrc/flat_planes.inc): the cases of test_flat_depth_model.py (CPU) and test_flats_depth_gpu.py.

The raster: walls (50) with a one-cell-wide serpentine channel of one elevation (10) -- channel rows on every second raster
row, joined by one cell at alternating ends -- and a single lower cell (1) beside the first channel cell.  Every channel
cell touches a wall, so the away-from-higher level is 1 everywhere and flat_mask = 2 x towards level (Barnes's numbering: the
low-edge cell is level 1, one more per step along the channel; the diagonal steps at the turns cut the corners, so the depth
is NOT the number of channel cells).  The depth is therefore taken from the oracle: one long channel per
(width, transpose, shift), its levels read off the oracle's flat_mask once; the case of depth D is that raster with every
channel cell deeper than D turned into wall, and the wall-only rows behind the end cropped.

  width      64: the whole channel in one tile column -- a visit walks ~2000 levels inside one 64 x 64 tile;
             200: the channel crosses a vertical tile seam every 64 levels
  transpose  the same crossings at horizontal seams
  shift      that many wall columns on the left (rows if transposed): moves the seams relative to the levels
  depth      D, the deepest towards level
"""
import functools

import numpy as np

CHANNEL, WALL, LOW = 10, 50, 1
NODATA = np.int32(-9999)
MAX_CELLS = 200_000

# The points of the 16-bit encoding, none of them taken from the engine: 0xFFFF is the planes' "not reached" pattern, 0x10000
# the first level that wraps, one 256-level segment of a visit below either.
FAR = (0x10000 + 600, 0x10000 + 5000)
SHALLOW = (0xFD00, 0xFE00)                     # the plane engine must NOT have stepped aside: plane_repeats == 0
AROUND_FFF0 = tuple(range(0xFFEE, 0xFFF2))
AROUND_10000 = tuple(range(0xFFFD, 0x10003))
BAND = tuple(sorted(set(range(0xFEF0, 0x10110 + 1, 32)) | set(range(0xFEFE, 0xFF02)) | set(AROUND_FFF0) | set(AROUND_10000)))
DEPTHS = SHALLOW + BAND + FAR
DEEPEST = max(DEPTHS)

GEOMETRIES = [(width, transpose, shift) for width in (64, 200) for transpose in (False, True) for shift in (0, 24)]
SWEEP = [(w, t, s, d) for (w, t, s) in GEOMETRIES for d in DEPTHS]
SEAM_SHIFTS = tuple(range(0, 64, 8))
SEAMS = [(200, t, s, FAR[0]) for t in (False, True) for s in SEAM_SHIFTS]
SCHEDULE_CASES = ([(200, False, 0, d) for d in AROUND_FFF0 + AROUND_10000]
                  + [(200, False, s, FAR[0]) for s in (0, 16, 32, 48)])
ROUTE_CASES = [(200, False, 0, d) for d in (0xFEFF, 0xFFEF, 0xFFFF, 0x10000, FAR[0])]
ALL_CASES = sorted(set(SWEEP) | set(SEAMS) | set(SCHEDULE_CASES) | set(ROUTE_CASES))


def case_id(case):
    w, t, s, d = case
    return f"w{w}{'T' if t else ''}-s{s}-D{d:#x}"


def _serpentine(width, nrows, shift):
    """nrows channel rows in a block `width` wide (channel columns 1 .. width - 2), `shift` wall columns to its left."""
    dem = np.full((2 * nrows + 1, shift + width), WALL, np.int32)
    x0, x1 = shift + 1, shift + width - 2
    for k in range(nrows):
        y = 2 * k + 1
        dem[y, x0:x1 + 1] = CHANNEL
        if k + 1 < nrows:
            dem[y + 1, x1 if k % 2 == 0 else x0] = CHANNEL
    dem[1, shift] = LOW
    return dem


def _oracle():
    import oracle

    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def long_channel(width, transpose, shift):
    """(raster, towards level of every channel cell (0 elsewhere)) of a channel deeper than every case needs."""
    nrows = (DEEPEST + 64) // (width - 3) + 2          # a channel row adds width - 3 levels (measured below, not assumed)
    dem = _serpentine(width, nrows, shift)
    if transpose:
        dem = np.ascontiguousarray(dem.T)
    _, mask, _ = _oracle().port.resolve_flats(dem, NODATA)
    chan = dem == CHANNEL
    # (the walls are flats of their own where the padding is wide, a few levels deep: only the channel's mask is a level)
    assert (mask[chan] > 0).all() and (mask[chan] % 2 == 0).all() and mask[~chan].max() < 256
    level = np.where(chan, mask // 2, 0)
    assert level.max() >= DEEPEST, (width, transpose, shift, int(level.max()))
    dem.setflags(write=False)
    level.setflags(write=False)
    return dem, level


def build(case):
    """The raster of one case (int32, its own copy)."""
    width, transpose, shift, depth = case
    base, level = long_channel(width, transpose, shift)
    dem = base.copy()
    dem[level > depth] = WALL
    keep = np.flatnonzero((dem != WALL).any(axis=0 if transpose else 1))[-1] + 2   # one wall line behind the last channel line
    return np.ascontiguousarray(dem[:, :keep] if transpose else dem[:keep])


@functools.lru_cache(maxsize=64)
def expected(case):
    """The oracle's directions for one case, computed once and shared (read-only)."""
    exp = _oracle().port.flat_resolution(build(case), NODATA)
    exp.setflags(write=False)
    return exp
