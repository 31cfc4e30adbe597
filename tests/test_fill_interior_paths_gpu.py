"""The interior-tile paths of the compact fill's two raster kernels, against the CPU oracle's fill, exact and over every cell.

k_descent16 (csrc/fill.hip) classifies the cells of a 64 x 64 descent tile and stores their labels without any in-raster,
border or cut-row test when the tile and its halo lie inside the raster and the tile holds no cell of the raster's first
or last row or column; k_pairs16 loads the node table of a descent tile with one load per thread or with four, by the
tile's node count, for the tile it PREFETCHES, which is not the one it works on (the same shapes stand ready for interior
paths in its ring and detection: measured, no gain, not kept).  Both kernels form their float keys without compares.
The rasters here are the smallest on which one of those decisions can go wrong (an edge tile taken for an interior one
reads or writes past a row's end, or misses a border cell; an interior one taken for an edge tile only costs time):

* 128 x 128 has no interior descent tile, 129 x 129 exactly one, whose halo column is the raster's last column;
* 64 and 65 rows, 129 wide: the pair tile at y0 = 32 is just not / just interior;
* 192 x 192, 193 x 191; 131 x 197 (no multiple of 4 wide: the kernels' unaligned instantiations);
* 200 x 63 and 63 x 200: no interior tile in one direction;
* a raster of 3280 pair tiles, more than the persistent pair pass has blocks, so that every block walks tiles of both kinds;
* the row-block shards (the descent's CUT instantiation) and pf_flowdirs (OUTLETS, which keeps the general body).

Content: seeded fractal terrain, and tilted planes with a walled box and one notch (test_fill_node_records_gpu.walled): a
cell labelled into the wrong basin is raised to the wrong level, or not at all.  Pits sit in the corner cells of the
interior tile and in the raster's border tiles.  Which path ran is asserted from the engine's debug line."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WALL = 10000.0
FALLBACKS = ("node table overflow", "hook chain unfinished", "pair list overflow")

# (rows, columns)
SHAPES = [(128, 128), (129, 129), (64, 129), (65, 129), (192, 192), (193, 191), (131, 197), (200, 63), (63, 200)]


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


def boxed(h, w):
    """a plane falling towards the top left corner, one box round the whole interior (its walls run through the border
    tiles), one nested across the seams at 32 and 64 where there is room.  Pits: the four corner cells of the descent tile
    at (64, 64) and the cells diagonally outside them, the corners of the pair tile at (32, 64), and the raster's border
    tiles -- inside the outer box, and between it and the raster's edge."""
    boxes = [(2, h - 3, 2, w - 3)]
    if h >= 60 and w >= 60:
        boxes.append((20, h - 12, 24, w - 10))
    walls = np.zeros((h, w), bool)
    for y0, y1, x0, x1 in boxes:
        walls[y0, x0:x1 + 1] = walls[y1, x0:x1 + 1] = True
        walls[y0:y1 + 1, x0] = walls[y0:y1 + 1, x1] = True
    cand = [(64, 64), (64, 127), (127, 64), (127, 127), (63, 63), (128, 128), (63, 128), (128, 63), (32, 64), (32, 127),
            (63, 64), (31, 70), (4, 4), (h - 5, w - 5), (4, w - 5), (h - 5, 4), (1, w // 2), (h - 2, w // 3), (h // 2, 1),
            (h // 3, w - 2)]
    pits = [(py, px) for py, px in cand if 1 <= py <= h - 2 and 1 <= px <= w - 2 and not walls[py, px]]
    assert len(pits) >= 8
    return walled(h, w, 1, 1, boxes, pits)


@functools.lru_cache(maxsize=None)
def _boxed(h, w):
    z = boxed(h, w)
    z.setflags(write=False)
    return z


_FRACTAL = {}


def _fractal(rd, h, w, seed):
    """seeded fractal terrain from the library's generator, made once per shape"""
    import torch

    if (h, w, seed) not in _FRACTAL:
        t = torch.empty((h, w), dtype=torch.float32, device="cuda")
        rd.synth_dem_dev(t, seed)
        torch.cuda.synchronize()
        z = t.cpu().numpy()
        z.setflags(write=False)
        _FRACTAL[(h, w, seed)] = z
    return _FRACTAL[(h, w, seed)]


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
    assert np.array_equal(dem.view(np.uint32), keep.view(np.uint32))
    return got, stats


def _both_entries(rd, orc, monkeypatch, capfd, dem, topo, what):
    import torch

    exp = _expected(orc, what, dem, topo)
    got, stats = _fill_compact(rd, monkeypatch, capfd, dem, topo, f"{what} D{topo}")
    _same(got, exp, f"{what} D{topo} host")
    t = torch.from_numpy(dem.copy()).cuda()                                # the HBM-resident entry
    rd.fill_depressions_dev(t, topology=topo)
    torch.cuda.synchronize()
    _same(t.cpu().numpy(), exp, f"{what} D{topo} dev")
    return exp, stats


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_boxed_planes_equal_the_oracle(rd, orc, monkeypatch, capfd, shape, topo):
    h, w = shape
    dem = _boxed(h, w)
    exp, _ = _both_entries(rd, orc, monkeypatch, capfd, dem, topo, f"boxed {h}x{w}")
    assert (exp != dem).any()
    assert exp[8, 8] == 5000.0                                             # the outer box stands full to its notch


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_terrain_equals_the_oracle(rd, orc, monkeypatch, capfd, shape, topo):
    h, w = shape
    dem = _fractal(rd, h, w, 7)
    exp, stats = _both_entries(rd, orc, monkeypatch, capfd, dem, topo, f"fractal {h}x{w}")
    assert (exp != dem).any() and stats["cells"] == dem.size


def test_every_pair_block_walks_tiles_of_both_kinds(rd, orc, monkeypatch, capfd):
    """2600 rows of 2500: 40 x 82 = 3280 pair tiles for at most 1536 resident blocks, 240 of the tiles on the raster's
    edge: a block's prefetch runs from interior tiles to edge tiles and back"""
    h, w = 2600, 2500
    assert -(-w // 64) * -(-h // 32) == 3280
    dem = _fractal(rd, h, w, 11)
    _, stats = _both_entries(rd, orc, monkeypatch, capfd, dem, 8, f"fractal {h}x{w}")
    assert stats["cells"] == h * w and stats["scan_tiles"] == 3280, stats


def test_three_row_blocks_equal_the_oracle(rd, orc, monkeypatch, capfd):
    """the shard path: the descent's CUT instantiation, whose cut rows never lie in an interior tile"""
    h, w = 300, 200
    dem = walled(h, w, 1, 1, [(2, h - 3, 2, w - 3), (40, h - 30, 30, w - 20)],
                 pits=[(h // 3, 70), (2 * h // 3, 64), (h // 2, 63), (99, 64), (100, 127), (101, 100), (199, 64), (200, 127)])
    exp = _expected(orc, "blocks", dem, 8)
    single, _ = _fill_compact(rd, monkeypatch, capfd, dem, 8, "blocks, single")
    _same(single, exp, "blocks: one device against the oracle")
    monkeypatch.setenv("RDGPU_DEVICES", "0,0,0")
    capfd.readouterr()
    got = rd.FillDepressions(dem, topology=8)
    err = capfd.readouterr().err
    monkeypatch.delenv("RDGPU_DEVICES")
    assert err.count("fill_fused: pair pass") >= 3 and not any(m in err for m in FALLBACKS), err   # three compact local phases
    _same(got, exp, "blocks: three row blocks against the oracle")


def test_outlet_fills_of_pf_flowdirs_equal_the_oracle(rd, orc):
    """the fills with interior outlets (OUTLETS) keep the general body of the descent; the pair pass is shared"""
    import torch

    dem = _fractal(rd, 192, 192, 5)
    nd = np.float32(-9999)
    exp = orc.port.pf_flowdirs(dem, nd)
    t = torch.from_numpy(dem.copy()).cuda()
    dirs = torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda")
    rd.pf_flowdirs_dev(t, nd, dirs)
    torch.cuda.synchronize()
    _same(dirs.cpu().numpy(), exp, "fractal 192x192, pf_flowdirs_dev")
    st = rd.pf_flowdirs_stats()
    print(st)
    assert st["unresolved"] == 0, st
    assert np.array_equal(t.cpu().numpy(), dem)


# ---- Key32<float>::to without compares ----------------------------------------------------------------------------

F32 = np.float32
SPECIALS = np.array([0x00000000, 0x80000000,               # +0, -0
                     0x00000001, 0x80000001,               # the smallest denormals
                     0x007FFFFF, 0x807FFFFF,               # the largest denormals
                     0x00800000, 0x80800000,               # the smallest normals
                     0x7F7FFFFF, 0xFF7FFFFF,               # the largest normals
                     0x7F800000, 0xFF800000,               # +inf, -inf
                     0x3F800000, 0xBF800000], np.uint32)


def _patterns(n, seed):
    """n random non-NaN bit patterns, the special ones spread among them several times over"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    nan = (b & 0x7F800000) == 0x7F800000
    b[nan] &= np.uint32(0xFF7FFFFF)                                        # NaN and inf patterns become finite ones
    at = rng.permutation(n)[:SPECIALS.size * 8]
    b[at] = np.tile(SPECIALS, 8)
    v = b.view(F32)
    assert not np.isnan(v).any()
    return v


def test_keys_order_every_kind_of_float(rd, orc, monkeypatch, capfd):
    """a raster of three rows: the outer rows hold 10^6 bit patterns -- zeros of both signs, denormals, the extremes,
    infinities, random ones -- and stay as they are; the middle row is -inf and +inf in turn, so every second cell is a
    pit between two walls and is raised to the lowest of its six border neighbours.  The outcome depends on the ORDER of
    the patterns' keys alone: +0 = -0 < the smallest denormal, negative denormals below both, and so on.  Compared with the
    oracle's float compares."""
    import torch

    n = 500000
    dem = np.empty((3, n), F32)
    dem[0], dem[2] = _patterns(n, 1), _patterns(n, 2)
    dem[1, 0::2] = np.inf
    dem[1, 1::2] = -np.inf
    dem[1, 1001:1101:2] = _patterns(200, 3)[:50]                               # (and some cells that may not be raised at all)
    exp = orc.port.fill(dem, 8)
    assert (exp[1] != dem[1]).sum() > n // 4 and np.array_equal(exp[0], dem[0]) and np.array_equal(exp[2], dem[2])
    levels = np.unique(exp[1].view(np.uint32)).size
    print("distinct levels in the middle row:", levels)
    assert levels > 1000
    for k in ("RDGPU_DEVICES", "RDGPU_FILL_EDGES", "RDGPU_FILL_EDGE_CAP"):
        monkeypatch.delenv(k, raising=False)
    got = rd.FillDepressions(dem, topology=8)
    _same(got, exp, "patterns 3 x 500000 host")
    t = torch.from_numpy(dem.copy()).cuda()
    rd.fill_depressions_dev(t)
    torch.cuda.synchronize()
    out = t.cpu().numpy()
    _same(out, exp, "patterns 3 x 500000 dev")
    # cells that were not raised keep their bits (a -0.0 stays -0.0), raised ones carry the bits of the cell they rose to
    kept = out[1] == dem[1]
    assert np.array_equal(out[0].view(np.uint32), dem[0].view(np.uint32))
    assert np.array_equal(out[1][kept].view(np.uint32), dem[1][kept].view(np.uint32))


def test_fills_stay_exact_with_signed_zeros_and_denormals(rd, orc, monkeypatch, capfd):
    """fractal terrain scaled into the denormal range and shifted to straddle zero, zeros of both signs sown in: the
    compact path, both entries"""
    z = _fractal(rd, 193, 191, 7).astype(np.float64)
    z = (z - np.median(z)) / np.abs(z - np.median(z)).max()                # -1 .. 1
    dem = (z * 3e-39).astype(F32)                                          # all denormal
    assert (np.abs(dem[dem != 0]) < np.finfo(F32).tiny).all() and (dem < 0).any() and (dem > 0).any()
    rng = np.random.default_rng(9)
    ys, xs = rng.integers(1, 192, 600), rng.integers(1, 190, 600)
    dem[ys[:300], xs[:300]] = F32(-0.0)
    dem[ys[300:], xs[300:]] = F32(0.0)
    exp, _ = _both_entries(rd, orc, monkeypatch, capfd, dem, 8, "denormal fractal 193x191")
    assert (exp != dem).any()
