"""The compact fill's node chase on the tile-edge records, against the CPU oracle's fill, exact and over every cell.

k_resolve_nodes (csrc/fill.hip) follows a pending node from tile to tile; the label of the cell it arrives at comes from
the neighbouring descent tile's edge records -- the outer columns (edgeS) or the outer rows (edgeR) of the 64 x 64 tile --
and k_finalize16 forms the nodes' levels itself.  The DEMs here are the smallest on which that lookup can go wrong:

* planes tilted so that the descent runs along the diagonals (through the tiles' corner cells, which lie in both
  records), along the columns only or along the rows only, on rasters with ragged last tiles and widths that are no
  multiple of 4.  WALLED BOXES with one notch each turn whole regions into basins whose level (the notch) lies above every
  cell of the plane: a node resolved into the wrong basin, or to the outside, raises its cells to the wrong level or not
  at all, so it cannot stay hidden behind max(z, level);
* one channel that winds along the tile seams and crosses them about 130 times, through rows and columns in turn: chains
  of many hops, shortened by the first chaser and followed by the others;
* seeded fractal terrain; the row-block shards (records of a cut raster, node levels from the table pass that path
  keeps); the fill with interior outlets under pf_flowdirs (no records: the labels come from the raster).

Which path ran is asserted from the engine's debug line, as tests/test_fallback_engines_gpu.py does: a fill that fell
back to the classic path would not touch the records at all."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WALL = 10000.0
FALLBACKS = ("node table overflow", "hook chain unfinished", "pair list overflow")


def walled(h, w, sx, sy, boxes, pits=()):
    """z = sx * x + sy * y (shifted to be >= 0), the perimeter of every box (y0, y1, x0, x1) a wall with ONE notch in the
    middle of its top side at 5000 + 100 k, and single cells dug to -5"""
    y, x = np.mgrid[0:h, 0:w]
    z = (sx * x + sy * y).astype(np.float32)
    z -= z.min()
    assert z.max() < 4000
    for k, (y0, y1, x0, x1) in enumerate(boxes):
        assert 1 <= y0 < y1 <= h - 2 and 1 <= x0 < x1 <= w - 2, (h, w, boxes[k])
        z[y0, x0:x1 + 1] = z[y1, x0:x1 + 1] = WALL
        z[y0:y1 + 1, x0] = z[y0:y1 + 1, x1] = WALL
        z[y0, (x0 + x1) // 2] = 5000.0 + 100.0 * k
    for py, px in pits:
        assert 1 <= py <= h - 2 and 1 <= px <= w - 2
        z[py, px] = -5.0
    return z


def diagonal(h, w):
    """every descent path runs towards the top left corner along a diagonal: the paths on a tile's main diagonal leave it
    through its corner cell.  One box round the whole interior, one nested inside it across the seams at 64 and 128 (the
    outer one's corner pit collects chains over every tile), pits on both sides of the tile corner at (64, 64)"""
    return walled(h, w, 1, 1, [(2, h - 3, 2, w - 3), (50, min(h, w) - 8, 40, min(h, w) - 6)],
                  pits=[(63, 63), (64, 64), (20, 30), (100, 70), (h - 5, w - 5)])


def serpentine(to_border):
    """192 x 192: a plateau (5000 + x + y) with a channel one cell wide that descends from 3000 along a path of 4-connected
    steps: it wiggles across the seam y = 63|64 eastwards (top / bottom row records), then across x = 127|128 southwards
    (column records), then across y = 127|128 westwards, then across x = 63|64 southwards, and ends in a pit, or runs on
    to the raster's left border.  Two pits in the plateau: with the channel ending at the border there are basins all the
    same, and their levels lie above the channel."""
    h = w = 192
    path = [(63, 3)]

    def wiggle(n, along, across):
        """n periods of: across, along, along, back across, along, along"""
        s = 1
        for _ in range(n):
            for dy, dx in ((across[0] * s, across[1] * s), along, along):
                path.append((path[-1][0] + dy, path[-1][1] + dx))
            s = -s

    wiggle(61, (0, 1), (1, 0))           # x: 3 -> 125, y flips between 63 and 64
    while path[-1][1] < 127:
        path.append((path[-1][0], path[-1][1] + 1))
    if path[-1][0] != 64:
        path.append((64, path[-1][1]))
    path.append((65, 127))
    wiggle(29, (1, 0), (0, 1))           # y: 65 -> 123, x flips between 127 and 128
    while path[-1][0] < 127:
        path.append((path[-1][0] + 1, path[-1][1]))
    if path[-1][1] != 127:
        path.append((127, 127))
    path.append((127, 126))
    wiggle(29, (0, -1), (1, 0))          # x: 126 -> 68, y flips between 127 and 128
    while path[-1][1] > 64:
        path.append((path[-1][0], path[-1][1] - 1))
    if path[-1][0] != 128:
        path.append((128, 64))
    path.append((129, 64))
    wiggle(28, (1, 0), (0, -1))          # y: 129 -> 185, x flips between 64 and 63
    if to_border:
        while path[-1][1] > 0:
            path.append((path[-1][0], path[-1][1] - 1))
    assert len(set(path)) == len(path) and all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(path, path[1:]))
    assert all(0 <= py < h and 0 <= px < w for py, px in path)
    cross = sum((a[0] // 64, a[1] // 64) != (b[0] // 64, b[1] // 64) for a, b in zip(path, path[1:]))
    assert cross >= 100, cross
    y, x = np.mgrid[0:h, 0:w]
    z = (5000 + x + y).astype(np.float32)
    for s, (py, px) in enumerate(path):
        z[py, px] = 3000.0 - s
    z[30, 150] = z[160, 150] = 4000.0
    return z


def nested_depressions():
    """130 x 130, every elevation distinct: a bowl of radius 50 whose rim drains to the border, inside it a smaller bowl
    behind a rim of its own"""
    h = w = 130
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r1 = np.hypot(x - 65, y - 65)
    r2 = np.hypot(x - 84, y - 70)
    z = np.where(r1 < 50, 20 + 0.5 * r1, 60 - 0.2 * (r1 - 50))
    z = np.where(r2 < 14, 40.0 + 0.1 * r2, z)
    z = np.where(r2 < 12, 5 + 0.5 * r2, z)
    z = (z + np.random.default_rng(5).permutation(h * w).reshape(h, w) * 1e-6).ravel()
    assert np.unique(z).size == z.size
    ranks = np.empty(h * w, np.float32)                                    # the surface's ranks: distinct in float32 too
    ranks[np.argsort(z)] = np.arange(h * w, dtype=np.float32)
    return ranks.reshape(h, w)


BUILT = {
    "diagonal-129x129": lambda: diagonal(129, 129),
    "diagonal-200x131": lambda: diagonal(131, 200),                        # 200 wide, 131 high
    "diagonal-131x200": lambda: diagonal(200, 131),                        # 131 wide (no multiple of 4), 200 high
    "serpentine-pit": lambda: serpentine(False),
    "serpentine-border": lambda: serpentine(True),
    # one column of tiles: every hop goes through a top / bottom row record; one row of tiles: through a column record
    "rows-only-64x300": lambda: walled(300, 64, 1, 3, [(2, 297, 2, 61), (100, 200, 10, 50)], pits=[(64, 30), (63, 31), (250, 5)]),
    "cols-only-300x64": lambda: walled(64, 300, 3, 1, [(2, 61, 2, 297), (10, 50, 100, 200)], pits=[(30, 64), (31, 63), (5, 250)]),
    # 65 x 65: the tiles beside the first hold border cells only; the plane falls towards them
    "corner-65x65": lambda: walled(65, 65, -1, -1, [(10, 40, 10, 40)], pits=[(50, 50), (62, 30)]),
}


@functools.lru_cache(maxsize=None)
def _dem(name):
    z = BUILT[name]()
    z.setflags(write=False)
    return z


_EXPECTED = {}


def _expected(orc, key, dem, topo):
    """the oracle's fill, computed once per DEM and topology and never written to"""
    if (key, topo) not in _EXPECTED:
        exp = orc.port.fill(dem, topo)
        exp.setflags(write=False)
        _EXPECTED[(key, topo)] = exp
    return _EXPECTED[(key, topo)]


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got != exp).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:8].tolist())


def _fill_compact(rd, monkeypatch, capfd, dem, topo, what):
    """the host entry's fill of dem, having checked that the compact path ran to its end; returns (filled, fill_stats)"""
    for k in ("RDGPU_DEVICES", "RDGPU_FILL_EDGES", "RDGPU_FILL_EDGE_CAP", "RDGPU_FILL_ROUND_BATCH", "RDGPU_FILL_TAIL_ROOTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RDGPU_FILL_DEBUG", "1")
    keep = dem.copy()
    capfd.readouterr()
    got = rd.FillDepressions(dem, topology=topo)
    err = capfd.readouterr().err
    stats = rd.fill_stats()
    print(what, stats)
    assert "fill_fused: pair pass" in err and not any(m in err for m in FALLBACKS), (what, err)
    assert stats["basins"] >= 1 and stats["jump_passes"] == 1 and stats["host_syncs"] == 2, (what, stats)
    assert np.array_equal(dem, keep)
    return got, stats


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", list(BUILT))
def test_built_dems_equal_the_oracle(rd, orc, monkeypatch, capfd, name, topo):
    import torch

    dem = _dem(name)
    exp = _expected(orc, name, dem, topo)
    assert (exp != dem).any()                                              # something is raised: the basins matter
    got, _ = _fill_compact(rd, monkeypatch, capfd, dem, topo, f"{name} D{topo}")
    _same(got, exp, f"{name} D{topo} host")
    t = torch.from_numpy(dem.copy()).cuda()                                # the HBM-resident entry
    rd.fill_depressions_dev(t, topology=topo)
    torch.cuda.synchronize()
    _same(t.cpu().numpy(), exp, f"{name} D{topo} dev")


def test_the_built_dems_are_what_they_claim(orc):
    """on the CPU: the boxes are basins filled to their notches, the channel that ends in a pit is raised as a whole and the
    one that reaches the border is not raised at all"""
    z = _dem("diagonal-129x129")
    exp = _expected(orc, "diagonal-129x129", z, 8)
    assert exp[30, 30] == 5000.0 and exp[80, 80] == 5100.0 and exp[1, 1] == z[1, 1]
    for topo in (8, 4):
        zp, zb = _dem("serpentine-pit"), _dem("serpentine-border")
        ep, eb = _expected(orc, "serpentine-pit", zp, topo), _expected(orc, "serpentine-border", zb, topo)
        ch_p, ch_b = zp <= 3000.0, zb <= 3000.0
        assert ch_p.sum() > 400 and (ep[ch_p] > 5000.0).all() and np.unique(ep[ch_p]).size == 1
        assert (eb[ch_b] == zb[ch_b]).all() and eb[30, 150] > 5000.0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", [(190, 257), (257, 190), (512, 512)])
def test_fractal_dems_equal_the_oracle(rd, orc, monkeypatch, capfd, shape, seed):
    import torch

    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(t, seed)
    torch.cuda.synchronize()
    dem = t.cpu().numpy()
    what = f"fractal {shape[0]}x{shape[1]} seed {seed}"
    exp = _expected(orc, what, dem, 8)
    got, stats = _fill_compact(rd, monkeypatch, capfd, dem, 8, what)
    _same(got, exp, what + " host")
    rd.fill_depressions_dev(t)
    torch.cuda.synchronize()
    _same(t.cpu().numpy(), exp, what + " dev")
    assert stats["cells"] == dem.size
    # (the oracle exposes no count of pit basins to set stats["basins"] against)


@pytest.mark.parametrize("shape", [(300, 200), (200, 300)])
def test_three_row_blocks_equal_the_single_device_fill(rd, orc, monkeypatch, capfd, shape):
    """the shard path: records of the cut rasters (k_descent16<CUT>), node levels from k_node_levels for the export"""
    h, w = shape
    dem = walled(h, w, 1, 1, [(2, h - 3, 2, w - 3), (40, h - 30, 30, w - 20)], pits=[(h // 3, 70), (2 * h // 3, 64), (h // 2, 63)])
    single, _ = _fill_compact(rd, monkeypatch, capfd, dem, 8, f"blocks {h}x{w}, single")
    monkeypatch.setenv("RDGPU_DEVICES", "0,0,0")
    capfd.readouterr()
    got = rd.FillDepressions(dem, topology=8)
    err = capfd.readouterr().err
    monkeypatch.delenv("RDGPU_DEVICES")
    assert err.count("fill_fused: pair pass") >= 3 and not any(m in err for m in FALLBACKS), err   # three compact local phases
    _same(got, single, f"blocks {h}x{w}: three row blocks against one")
    _same(single, _expected(orc, f"blocks {h}x{w}", dem, 8), f"blocks {h}x{w}: against the oracle")


def test_outlet_fills_of_pf_flowdirs_equal_the_oracle(rd, orc):
    """the fills with interior outlets skip tiles, so they keep no records: the chase reads the raster's labels"""
    import torch

    dem = nested_depressions()
    nd = np.float32(-9999)
    exp = orc.port.pf_flowdirs(dem, nd)
    t = torch.from_numpy(dem.copy()).cuda()
    dirs = torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda")
    rd.pf_flowdirs_dev(t, nd, dirs)
    torch.cuda.synchronize()
    _same(dirs.cpu().numpy(), exp, "nested depressions, pf_flowdirs_dev")
    st = rd.pf_flowdirs_stats()
    print(st)
    assert st["unresolved"] == 0 and st["levels"] >= 2, st
    assert np.array_equal(t.cpu().numpy(), dem)
