"""The engines that take over when the fast one cannot run, against the CPU oracle.

d8_flow_accum (csrc/accum.hip) has three engines -- tile links with subtree sums (default), tile links with the
last-arriver walk in every tile (RDGPU_ACCUM_SUMS=0; also what the default hands its slow tiles to), the raster-wide walk
(RDGPU_ACCUM_LINKS=0) -- and the fill (csrc/fill.hip, fill_fused) leaves a DEM to the classic path when its node table
overflows.  Every engine runs here on hand-built rasters that sit on the engines' internal limits: direction loops across
tile seams and round a tile corner, a loop and a loop-free path as long as a tile (4096 cells: the bound the pointer
jumping's twelve trips rest on), a NoData value that is itself a direction code, and DEMs with the highest possible pit
density.  Expected values come from the oracle (orc.port.*, pinned to the compiled reference by test_oracle_pinning.py) and
from tests/upslope_model.py; every comparison is exact and over every cell; inputs must be unchanged afterwards.  The
profiler's launch counts and the fill's debug line prove that a switch or a fallback really ran."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upslope_model as um  # noqa: E402

pytestmark = pytest.mark.gpu

T = 64                                                                     # the tile side of accum.hip and upslope.hip
W_, N_, E_, S_ = 1, 3, 5, 7                                                # upslope_model.D8X / D8Y


# ---- A. direction rasters ---------------------------------------------------------------------------------------------
RING = (113, 143)                                                          # the ring's first and last row / column


def seam_loops():
    """192 x 192, everything flows east and off the right edge, except four loops that the rows feed from one or two tiles
    away: two-cycles across the seams x = 63|64 and y = 63|64, a four-cycle round the tile corner at (64, 64), and a ring
    of 120 cells round the corner at (128, 128) that passes through four tiles"""
    d = np.full((3 * T, 3 * T), E_, np.uint8)
    d[20, T] = W_                                                          # (63,20) -> (64,20) -> back
    d[T - 1, 20], d[T, 20] = S_, N_                                        # (20,63) -> (20,64) -> back
    d[T - 1, T - 1], d[T - 1, T], d[T, T], d[T, T - 1] = E_, S_, W_, N_    # (63,63) -> (64,63) -> (64,64) -> (63,64) ->
    a, b = RING
    d[a, a:b] = E_                                                         # clockwise: top, right, bottom, left
    d[a:b, b] = S_
    d[b, a + 1:b + 1] = W_
    d[a + 1:b + 1, a] = N_
    return d


def tile_cycle():
    """192 x 192, the centre tile is ONE cycle over all of its 4096 cells (east and west along the rows over columns 1..63,
    back up column 0); the eight tiles around it flow into it"""
    d = np.zeros((3 * T, 3 * T), np.uint8)
    d[:T, :T], d[:T, T:2 * T], d[:T, 2 * T:] = 6, S_, 8
    d[T:2 * T, :T], d[T:2 * T, 2 * T:] = E_, W_
    d[2 * T:, :T], d[2 * T:, T:2 * T], d[2 * T:, 2 * T:] = 4, N_, 2
    c = d[T:2 * T, T:2 * T]
    c[0::2, 1:T - 1], c[0::2, T - 1] = E_, S_
    c[1::2, 2:], c[1::2, 1] = W_, S_
    c[T - 1, 1] = W_
    c[:, 0] = N_
    c[0, 0] = E_
    return d


SNAKE_END = (3 * T - 1, 2 * T)                                              # (x, y) of the last cell of tile_snakes' path


def _boustrophedon(hh, ww, by_cols, flip):
    """the cells (y, x) of an hh x ww tile in boustrophedon order, from the top left corner (flip: from the bottom right)"""
    out = []
    for i in range(ww if by_cols else hh):
        run = range(hh if by_cols else ww)
        for j in (run if i % 2 == 0 else reversed(run)):
            y, x = (j, i) if by_cols else (i, j)
            out.append((hh - 1 - y, ww - 1 - x) if flip else (y, x))
    return out


def tile_snakes():
    """130 rows x 192 columns without a loop: every tile is a boustrophedon over all of its cells that leaves into the next
    tile, the tiles chained in a boustrophedon too -- ONE path over every cell of the raster, 4096 cells of it in each full
    tile and 128 in each 2-row bottom tile; it leaves the raster eastwards from (191, 128)"""
    h, w = 2 * T + 2, 3 * T
    #        tile row, tile column, columns first?, from the bottom right?
    order = [(0, 0, True, False), (0, 1, True, False), (0, 2, False, False),      # eastwards; the last one ends bottom left
             (1, 2, False, False), (1, 1, True, True), (1, 0, True, True),        # westwards along the tiles' bottom rows
             (2, 0, True, False), (2, 1, True, False), (2, 2, True, False)]       # eastwards through the 2-row tiles
    path = []
    for ty, tx, by_cols, flip in order:
        hh = min(T, h - ty * T)
        path += [(ty * T + y, tx * T + x) for y, x in _boustrophedon(hh, T, by_cols, flip)]
    assert len(path) == h * w and len(set(path)) == h * w
    code = {(0, -1): W_, (-1, 0): N_, (0, 1): E_, (1, 0): S_}
    d = np.zeros((h, w), np.uint8)
    for (y, x), (y2, x2) in zip(path, path[1:]):
        d[y, x] = code[(y2 - y, x2 - x)]
    assert path[-1] == (SNAKE_END[1], SNAKE_END[0])
    d[path[-1]] = E_
    return d


CODE_SHAPES = [(1, 1), (1, 200), (200, 1), (65, 129), (130, 191)]
CODE_NODATA = [255, 3, 0]                                                  # 3: a NoData value that is a direction code


def codes(shape, nd):
    """random codes 0..9, 200 and nd, weighted like test_upslope_gpu.test_fresh_shapes_equal_the_model"""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w + 7 * nd)
    return rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 200, nd], np.uint8), (h, w),
                      p=[.03, .1, .1, .1, .1, .15, .15, .1, .1, .02, .02, .03])


BUILT = {"seam_loops": (seam_loops, 255), "tile_cycle": (tile_cycle, 255), "tile_snakes": (tile_snakes, 255)}
for _s in CODE_SHAPES:
    for _nd in CODE_NODATA:
        BUILT[f"codes-{_s[0]}x{_s[1]}-nd{_nd}"] = (functools.partial(codes, _s, _nd), _nd)
RASTERS = list(BUILT)
ENGINES = {"default": {}, "sums0": {"RDGPU_ACCUM_SUMS": "0"}, "links0": {"RDGPU_ACCUM_LINKS": "0"}}
DTYPES = (np.int32, np.float64, np.float32)                                # every total is below 2^24: float32 is exact


@functools.lru_cache(maxsize=None)
def _raster(name):
    make, nd = BUILT[name]
    d = make()
    d.setflags(write=False)
    return d, nd


_EXPECTED = {}


def _expected(orc, name, dt):
    """the oracle's accumulation, computed once per raster and type and never written to"""
    key = (name, np.dtype(dt).name)
    if key not in _EXPECTED:
        dirs, nd = _raster(name)
        exp = orc.port.d8_flow_accum(dirs, nd, dt)
        exp.setflags(write=False)
        _EXPECTED[key] = exp
    return _EXPECTED[key]


def _loop_free(name):
    dirs, nd = _raster(name)
    return bool(um._ends(um._links(dirs, nd, False))[1].all())


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got != exp).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:8].tolist())


def _set_engine(monkeypatch, engine):
    for k in ("RDGPU_ACCUM_SUMS", "RDGPU_ACCUM_LINKS", "RDGPU_DEVICES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENGINES[engine].items():
        monkeypatch.setenv(k, v)


def test_the_rasters_are_what_they_claim(orc):
    """the helpers above, on the CPU: the loops are loops of the stated length, the snake is one path over every cell"""
    d, nd = _raster("tile_snakes")
    h, w = d.shape
    exp = _expected(orc, "tile_snakes", np.int32)
    assert _loop_free("tile_snakes") and exp.max() == h * w and exp[SNAKE_END[1], SNAKE_END[0]] == h * w
    assert sorted(exp.ravel().tolist()) == list(range(1, h * w + 1))       # every cell lies on the one path
    for name, start, length in (("tile_cycle", (T, T), T * T), ("seam_loops", (RING[0], RING[0]), 120),
                                ("seam_loops", (T - 1, T - 1), 4), ("seam_loops", (20, T - 1), 2), ("seam_loops", (T - 1, 20), 2)):
        d, nd = _raster(name)
        nxt = um._links(d, nd, False)
        c0 = start[1] * d.shape[1] + start[0]
        c, seen = int(nxt[c0]), 1
        while c != c0 and seen <= d.size:
            c, seen = int(nxt[c]), seen + 1
        assert c == c0 and seen == length, (name, start, seen)
        assert not _loop_free(name)
    d, nd = _raster("tile_cycle")
    assert not um._ends(um._links(d, nd, False))[1].any()                  # every cell is on the cycle or drains into it


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", RASTERS)
def test_accum_engines_equal_the_oracle(rd, orc, monkeypatch, name, engine):
    import torch

    dirs, nd = _raster(name)
    keep = dirs.copy()
    _set_engine(monkeypatch, engine)
    for dt in DTYPES:
        _same(rd.d8_flow_accum(dirs, nd, dt), _expected(orc, name, dt), f"{name} {engine} {np.dtype(dt).name} host")
    if name == "tile_snakes":
        assert _expected(orc, name, np.int32).max() == dirs.size
    # the HBM-resident entry on a stream of its own
    t = torch.from_numpy(dirs.copy()).cuda()
    t_keep = t.clone()
    area = torch.full(dirs.shape, -77, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rd.d8_flow_accum_dev(t, area, nd)
    side.synchronize()
    _same(area.cpu().numpy(), _expected(orc, name, np.float64), f"{name} {engine} float64 dev, side stream")
    assert np.array_equal(dirs, keep) and torch.equal(t, t_keep)


@pytest.mark.parametrize("engine", list(ENGINES))
def test_the_switches_change_the_launched_kernels(rd, orc, monkeypatch, engine):
    """a switch that silently does nothing fails here: the profiler's launch counts of one call per setting (names that
    were not launched are absent from profile_totals)"""
    dirs, nd = _raster("tile_cycle")
    _set_engine(monkeypatch, engine)
    rd.profile_enable(True)
    try:
        rd.profile_reset()
        got = rd.d8_flow_accum(dirs, nd, np.int32)
        tot = rd.profile_totals()
    finally:
        rd.profile_enable(False)
        rd.profile_reset()
    n = {k: v[1] for k, v in tot.items() if k.startswith("accum.")}
    print(engine, n)
    _same(got, _expected(orc, "tile_cycle", np.int32), f"tile_cycle {engine} profiled")
    if engine == "links0":
        assert n.get("accum.walk_unit", 0) >= 1 and n.get("accum.link_tile", 0) == 0 and n.get("accum.link_final", 0) == 0, n
    elif engine == "sums0":
        assert n.get("accum.link_tile", 0) >= 1 and n.get("accum.link_final", 0) >= 1, n
        assert n.get("accum.link_final_loops", 0) == 0 and n.get("accum.walk_unit", 0) == 0, n
    else:
        assert n.get("accum.link_tile", 0) >= 1 and n.get("accum.link_final_loops", 0) >= 1 and n.get("accum.walk_unit", 0) == 0, n


# the loop-free rasters (tile_snakes and whichever random ones happen to have no loop), with as many rows as blocks
BLOCK_CASES = [(n, wd) for n in RASTERS for wd in (2, 3)
               if (n == "seam_loops" or _loop_free(n)) and _raster(n)[0].shape[0] >= wd]


@pytest.mark.parametrize("name,world", BLOCK_CASES)
def test_accum_row_blocks_equal_the_oracle(rd, orc, monkeypatch, name, world):
    """the row-block shards (the raster-wide walk per block): one exchange and the oracle's array on the loop-free rasters,
    the oracle's array after any number of exchanges on seam_loops"""
    import torch

    from richdem_amd.sharded import d8_flow_accum_blocks

    dirs, nd = _raster(name)
    loop_free = _loop_free(name)
    _set_engine(monkeypatch, "default")
    t = torch.from_numpy(dirs.copy()).cuda()
    t_keep = t.clone()
    for dt, tdt in ((np.float64, torch.float64), (np.int32, torch.int32)):
        area = torch.full(dirs.shape, -77, dtype=tdt, device="cuda")
        ex = d8_flow_accum_blocks(t, area, world, nd)
        torch.cuda.synchronize()
        print(name, world, "exchanges:", ex)
        _same(area.cpu().numpy(), _expected(orc, name, dt), f"{name} in {world} row blocks {np.dtype(dt).name}")
        if loop_free:
            assert ex == 1, (name, world, ex)
    assert torch.equal(t, t_keep)


# ---- B. upslope on the same rasters -----------------------------------------------------------------------------------
def _dev(rd, fn, dirs, out_dtype, fill, *args):
    import torch

    t = torch.from_numpy(dirs.copy()).cuda()
    keep = t.clone()
    out = torch.full(dirs.shape, fill, dtype=out_dtype, device="cuda")
    fn(t, out, *args)
    torch.cuda.synchronize()
    assert torch.equal(t, keep)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["seam_loops", "tile_cycle", "tile_snakes"])
def test_upslope_on_the_built_rasters_equals_the_model(rd, name):
    import torch

    dirs, nd = _raster(name)
    keep = dirs.copy()
    h, w = dirs.shape
    last = SNAKE_END[1] * w + SNAKE_END[0]
    exp_o = um.outlets(dirs, nd)
    if name == "tile_snakes":
        assert (exp_o == last).all()                                       # one path: one outlet
    elif name == "tile_cycle":
        assert (exp_o == um.NONE).all()                                    # everything drains into the cycle
    else:
        assert (exp_o[RING[0], RING[0]:RING[1]] == um.NONE).all() and (exp_o[0] == w - 1).all()
    _same(rd.d8_outlets(dirs, nd), exp_o, name + " outlets host")
    _same(_dev(rd, lambda t, o: rd.d8_outlets_dev(t, o, nd), dirs, torch.int32, 123456).view(np.uint32), exp_o, name + " outlets dev")
    # seeds: the snake's last cell, a ring cell, a cell of the tile cycle; one at a time and together
    seeds = np.array([last, RING[0] * w + RING[0] + 5, 100 * w + 100], np.uint32)
    labels = np.array([11, -22, 33], np.int32)
    for pick in ([0], [1], [2], [0, 1, 2]):
        c, lab = seeds[pick], labels[pick]
        exp = um.catchments(dirs, c, lab, -5, nd)
        if name == "tile_snakes" and 0 in pick:
            assert (exp != -5).all()                                       # the last cell's catchment is the raster
        _same(rd.d8_catchments(dirs, c, lab, -5, nd), exp, f"{name} catchments host, seeds {pick}")
        cd = torch.from_numpy(c.view(np.int32).copy()).cuda()
        ld = torch.from_numpy(lab.copy()).cuda()
        _same(_dev(rd, lambda t, o: rd.d8_catchments_dev(t, cd, ld, o, -5, nd), dirs, torch.int32, 123456), exp,
              f"{name} catchments dev, seeds {pick}")
    ln = (SNAKE_END[0], SNAKE_END[1], SNAKE_END[0], SNAKE_END[1])          # a line of one cell
    exp = um.upslope_cells(dirs, *ln, nodata=nd)
    _same(rd.d8_upslope_cells(dirs, *ln, nodata=nd), exp, name + " upslope cells host")
    _same(_dev(rd, lambda t, o: rd.d8_upslope_cells_dev(t, *ln, o, nd), dirs, torch.uint8, 77), exp, name + " upslope cells dev")
    assert np.array_equal(dirs, keep)


# ---- C. the fill at the node table's limit ------------------------------------------------------------------------------
def d4_checker():
    """192 x 192: under D4 every interior cell of value 0 is a pit -- about n/2 = 18 000 of them against a node table of
    n/4 + 4096 = 13 312 entries"""
    y, x = np.mgrid[0:192, 0:192]
    z = (x + y) % 2
    z[0, :] += 2
    z[-1, :] += 2
    z[1:-1, 0] += 2
    z[1:-1, -1] += 2
    return z


def d8_lattice(h, w):
    """0 where x and y are both even, 1 elsewhere: about n/4 pits under D8"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x % 2 == 0) & (y % 2 == 0), 0, 1)


def staircase():
    """400 x 400, a chain of almost 20 000 basins each of which spills into the next: one corridor winds through the raster
    between walls, along it a pit every fourth cell and between two pits a barrier, each barrier lower than the one
    before.  In round 1 every basin's lowest pass leads to the next basin: one chain of hooks longer than the 16384 hops a
    thread of fill.hip's k_chase_links takes by itself."""
    h = w = 400
    path = []
    rows = list(range(1, h - 1, 2))
    for i, y in enumerate(rows):
        xs = list(range(1, w - 1))
        path += [(y, x) for x in (xs if i % 2 == 0 else reversed(xs))]
        if i + 1 < len(rows):
            path.append((y + 1, path[-1][1]))                              # the connector through the wall row
    path.append((path[-1][0], 0 if path[-1][1] == 1 else w - 1))           # out through the border
    L = len(path)
    z = np.full((h, w), float(L + 100), np.float32)                        # walls: above every barrier
    for s, (y, x) in enumerate(path):
        z[y, x] = 0.0 if s % 4 == 0 else (10.0 + (L - s)) if s % 4 == 2 else 5.0
    z[path[-1]] = -1.0
    return z


FILL_DEMS = {"d4_checker": d4_checker, "d8_lattice": lambda: d8_lattice(384, 512), "d8_lattice_small": lambda: d8_lattice(70, 66)}


@functools.lru_cache(maxsize=None)
def _dem(name, dt):
    z = (staircase() if name == "staircase" else FILL_DEMS[name]()).astype(dt)
    z.setflags(write=False)
    return z


def _fill_every_entry(rd, orc, monkeypatch, capfd, dem, topo, what):
    """host entry, HBM-resident entry, three row blocks through the multi-device driver: each equals the oracle; returns
    what the engine wrote to stderr during the single-block host call and during the row blocks' call, and the single
    block's fill_stats"""
    import torch

    keep = dem.copy()
    exp = orc.port.fill(dem, topo)
    monkeypatch.delenv("RDGPU_DEVICES", raising=False)
    monkeypatch.delenv("RDGPU_FILL_EDGES", raising=False)
    monkeypatch.delenv("RDGPU_FILL_EDGE_CAP", raising=False)
    monkeypatch.setenv("RDGPU_FILL_DEBUG", "1")
    capfd.readouterr()
    got = rd.FillDepressions(dem, topology=topo)
    err = capfd.readouterr().err
    stats = rd.fill_stats()
    assert got.tobytes() == exp.tobytes(), (what, "host", int((got != exp).sum()))
    t = torch.from_numpy(dem.copy()).cuda()
    rd.fill_depressions_dev(t, topology=topo)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert got.tobytes() == exp.tobytes(), (what, "dev", int((got != exp).sum()))
    monkeypatch.setenv("RDGPU_DEVICES", "0,0,0")
    got = rd.FillDepressions(dem, topology=topo)
    monkeypatch.delenv("RDGPU_DEVICES")
    err_blocks = capfd.readouterr().err
    assert got.tobytes() == exp.tobytes(), (what, "three row blocks", int((got != exp).sum()))
    assert np.array_equal(dem, keep)
    return err, err_blocks, stats


@pytest.mark.parametrize("dt", [np.float32, np.int16])
@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", list(FILL_DEMS))
def test_fill_at_the_node_table_limit(rd, orc, monkeypatch, capfd, name, topo, dt):
    dem = _dem(name, dt)
    what = f"{name} D{topo} {np.dtype(dt).name}"
    err, err_blocks, _ = _fill_every_entry(rd, orc, monkeypatch, capfd, dem, topo, what)
    overflow = "node table overflow" in err
    print(what, "single block:", "node table overflow -> classic path" if overflow else "fused path",
          "| three row blocks:", "node table overflow in a block" if "node table overflow" in err_blocks else "fused local phases")
    assert "fill_fused:" in err, (what, err)                              # the debug switch spoke: the fused path was entered
    if name == "d4_checker" and topo == 4:
        assert overflow, (what, err)                                       # ~n/2 pits cannot fit n/4 + 4096 nodes
    if name == "d8_lattice_small":
        assert not overflow and "node table overflow" not in err_blocks, (what, err, err_blocks)   # 4096 spare entries
        assert "pair pass" in err, (what, err)                             # ... and the fused path went all the way


def test_fill_a_chain_of_hooks_longer_than_one_chase(rd, orc, monkeypatch, capfd):
    """the longest chain of hooks a raster of this size can hold (see staircase); which path ran is printed, not asserted:
    whether the chase is left unfinished depends on how far the other threads have shortened the chain (fill.hip, at the
    "hook chain unfinished" exit).  On an MI355X: under D4 the fused path resolves the chain of 19 850 basins in one round;
    under D8 the walls' diagonal neighbours overflow the pair list and the classic path takes the raster."""
    dem = _dem("staircase", np.float32)
    seen = []
    for topo in (8, 4):
        err, _, stats = _fill_every_entry(rd, orc, monkeypatch, capfd, dem, topo, f"staircase D{topo}")
        left = [m for m in ("node table overflow", "hook chain unfinished", "pair list overflow") if m in err]
        if not left:
            assert stats["basins"] > 16384 and stats["rounds"] >= 1, stats  # the fused path went through, with the chain in it
        seen.append((f"staircase D{topo}:", f"{left[0]} -> classic path" if left else "fused path", stats))
    for line in seen:                                                      # (after the last capfd.readouterr())
        print(*line)
