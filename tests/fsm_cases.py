"""Inputs shared by the Fill-Spill-Merge tests (tests/test_fsm_model.py on the CPU, tests/test_fsm_gpu.py on the GPU): the
hand-made rasters with their expected arrays written out, the cascade of roots, the rasters shaped for the kernels'
seams, and the golden cases of tests/golden/ref_fsm.npz."""
import numpy as np

NONE = 0xFFFFFFFF


def ring(inner, border=9):
    """`inner` with a border ring of `border` around it, int32"""
    inner = np.asarray(inner, np.int32)
    z = np.full((inner.shape[0] + 2, inner.shape[1] + 2), border, np.int32)
    z[1:-1, 1:-1] = inner
    return z


def on(shape, cells):
    """a float64 raster, zero but for {(y, x): value}"""
    w = np.zeros(shape, np.float64)
    for (y, x), v in cells.items():
        w[y, x] = v
    return w


# one pit in a 5 x 5 raster: level 9 (the ring), 9 cells, volume 8 + 4 * 5 + 4 * 4 = 44
BOWL = ring([[5, 4, 5], [4, 1, 4], [5, 4, 5]])
# two pits in a row of a 5 x 7 raster: leaf 0 (the 3; level 6, volume 3), leaf 1 (the 1 and the saddle 6; level 6, volume 5),
# their parent (level 9, all 15 interior cells, volume 6 + 3 + 8 + 12 = 29)
TWO = ring([[8, 8, 8, 8, 8], [3, 6, 1, 8, 8], [8, 8, 8, 8, 8]])


def staircase(k):
    """5 x (4k + 3), int32: k pits in the middle row going down to the right, every one a root of its own that spills into
    the next one's tree (the last one over the ring).  Pit i: elevation b = 100 (k - i), its three cells b + 20, b, b + 10,
    the wall to its left b + 130; level b + 30 (the last: b + 40), volume 10 + 30 + 20 = 60 (the last: 20 + 40 + 30 + 10 = 100)."""
    big = 1_000_000
    z = np.full((5, 4 * k + 3), big, np.int32)
    b = 100 * (k - np.arange(k))
    z[2, 1:4 * k + 1:4] = b + 130
    z[2, 2:4 * k + 2:4] = b + 20
    z[2, 3:4 * k + 3:4] = b
    z[2, 4:4 * k + 4:4] = b + 10
    z[2, 4 * k + 1] = b[-1] + 30
    z[2, 4 * k + 2] = b[-1] + 40
    return z


def hand_made():
    """name -> (dem, water, expected): expected has depth (the full array), node_water, ocean, lakes, full_lakes, tops"""
    c = {}
    zero = np.zeros((5, 5))
    # 4.5 into the bowl: the cells sorted are 1 4 4 4 4 5 5 5 5; (4.5 + 17) / 5 = 4.3 <= 5 is the first that holds
    w = np.zeros((5, 5))
    w[1:4, 1:4] = 0.5
    w[0, 2] = 1.0                                               # a ring cell: to the ocean
    h = 21.5 / 5
    c["one_pit_partly"] = (BOWL, w, dict(depth=on((5, 5), {(2, 2): h - 1, (1, 2): h - 4, (2, 1): h - 4, (2, 3): h - 4, (3, 2): h - 4}),
                                         node_water=[4.5], ocean=1.0, lakes=1, full_lakes=0, tops=[0]))
    w = np.zeros((5, 5))
    w[1:4, 1:4] = 10.0
    c["one_pit_overfilled"] = (BOWL, w, dict(depth=np.where(BOWL < 9, 9.0 - BOWL, 0.0), node_water=[44.0], ocean=46.0, lakes=1,
                                             full_lakes=1, tops=[0]))
    # 5 on the first pit: 3 fill it to its saddle, 2 go over the spill pair into the second one
    c["first_spills_into_second"] = (TWO, on((5, 7), {(2, 1): 5.0}),
                                     dict(depth=on((5, 7), {(2, 1): 3.0, (2, 3): 2.0}), node_water=[3.0, 2.0, 0.0], ocean=0.0,
                                          lakes=2, full_lakes=1, tops=[0, 1]))
    # 20 on the first pit: 3 + 5 fill both, the parent starts at 8 and takes the other 12; the 15 cells sorted are
    # 1 3 6 8 ... 8, and only the last position holds: (20 + 106) / 15 = 8.4, above the saddle at 6
    h = 126.0 / 15
    d = np.zeros((5, 7))
    d[1:4, 1:6] = h - TWO[1:4, 1:6]
    c["both_full_parent_lake"] = (TWO, on((5, 7), {(2, 1): 20.0}),
                                  dict(depth=d, node_water=[3.0, 5.0, 20.0], ocean=0.0, lakes=1, full_lakes=0, tops=[2]))
    # two roots on 5 x 9: the upper pit (220 200 210; level 230, the wall that drains to the lower pit; volume 60) and the
    # lower one (100 110 130; level 140, the ring cell; volume 80).  75 on the upper pit fill it and the other 15 go over
    # its spill into the lower pit's tree: (15 + 100) / 1 = 115 > 110, (15 + 210) / 2 = 112.5 <= 130
    z = np.full((5, 9), 1_000_000, np.int32)
    z[2] = [1_000_000, 220, 200, 210, 230, 100, 110, 130, 140]
    c["root_spills_into_another_tree"] = (z, on(z.shape, {(2, 2): 75.0}),
                                          dict(depth=on(z.shape, {(2, 1): 10.0, (2, 2): 30.0, (2, 3): 20.0, (2, 5): 12.5, (2, 6): 2.5}),
                                               node_water=[60.0, 15.0], ocean=0.0, lakes=2, full_lakes=1, tops=[0, 1]))
    c["zero_water"] = (BOWL, zero, dict(depth=zero, node_water=[0.0], ocean=0.0, lakes=0, full_lakes=0, tops=[]))
    w = np.zeros((5, 5))
    w[0, :] = w[-1, :] = w[:, 0] = w[:, -1] = 0.25
    c["water_on_the_ring_only"] = (BOWL, w, dict(depth=zero, node_water=[0.0], ocean=4.0, lakes=0, full_lakes=0, tops=[]))
    return c


CASCADE_PITS = 2000


def cascade():
    """(dem, water): 2000 roots in a row on 5 x 8003, water on the top pit only, enough to fill them all and 7 to spare"""
    z = staircase(CASCADE_PITS)
    return z, on(z.shape, {(2, 3): 60.0 * (CASCADE_PITS - 1) + 100.0 + 7.0})


def bowl_130():
    """(dem, water): 130 x 130 f32, one pit, distinct dyadic elevations (multiples of 2^-6 rising with the Chebyshev
    distance from the centre, ties broken by the raster index): the 127 x 127 = 16 129 cells nearer than the ring lie below
    the spill level 252.  The water, 64 on every interior cell, fills about half of the volume: one partial lake whose
    16 129 records are one segment of the scan."""
    y, x = np.mgrid[0:130, 0:130]
    r = np.maximum(abs(y - 64), abs(x - 65)).astype(np.int64)
    order = np.lexsort((np.arange(r.size), r.ravel()))
    z = np.empty(r.size, np.float32)
    z[order] = np.arange(r.size, dtype=np.float32) / 64.0       # below 2^24 units: exact
    w = np.zeros((130, 130))
    w[1:-1, 1:-1] = 64.0
    return z.reshape(130, 130), w


def egg_carton():
    """(dem, water): 129 x 129 i32, a pit at every interior (3i + 2, 3j + 2) with walls of distinct, scattered heights between them;
    the water differs from pit to pit (multiples of 2, up to 8 190, against leaf volumes around 5 000): some 1 500 lakes,
    a quarter of them full, some 200 merged ones, and most segments of the scan one or two records long"""
    y, x = np.mgrid[0:129, 0:129]
    pit = (y % 3 == 2) & (x % 3 == 2) & (y < 128) & (x < 128)
    idx = (y * 129 + x).astype(np.int64)
    z = np.where(pit, idx % 1000, 2000 + (idx * 7919) % 16642).astype(np.int32)   # (7919 is prime: the walls are distinct)
    w = np.where(pit, ((idx * 7919) % 4096) * 2.0, 0.0)
    return z, w


def golden_cases(G):
    """(case name, water index, dem, water, the reference's wtd, the recorded largest difference) of ref_fsm.npz"""
    for name in [str(s) for s in G["cases"]]:
        for k in range(4):
            yield name, k, G[name + "/dem"], G[f"{name}/w{k}/water"], G[f"{name}/w{k}/wtd"], float(G[f"{name}/w{k}/max_diff"])
