"""Stream reaches on the engine (csrc/reaches.hip) against the Python model (tests/stream_reach_model.py, pinned by
tests/test_stream_reach_model.py): the host C-ABI and the `_dev` entry, every requested plane on every cell and every
record bit for bit (`length` through its uint64 view), records past N and planes not requested left alone, inputs
unchanged.  Shapes are the smallest that reach every path of the kernels: one cell, one row, one column, a tile, one more
or less than a tile, several tiles; junctions whose children arrive from other tiles; loops inside a tile, across an edge
and a corner; a reach and a catchment of more than 65 535 cells; more than 4096 reaches in a tile and 65 536 in all."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc  # noqa: E402
import stream_reach_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (193, 70), (257, 259)]   # (height, width)
NONE = 0xFFFFFFFF
FILL = 0x77                                                                                   # the sentinel byte
_MODEL = {}


def _model(key, dirs, nodata, chan, order, cell):
    """the model's answer, computed once per case"""
    if key not in _MODEL:
        _MODEL[key] = rm.stream_reaches(dirs, nodata, chan, order, cell)
    return _MODEL[key]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _host(rd, dirs, nodata=255, chan=None, order=None, cell=(1.0, 1.0), want=("reach", "catchment", "table"), capacity=0):
    """one call of the host C-ABI on sentinel-filled outputs: count, reach, catchment, the table's `capacity` records"""
    h, w = dirs.shape
    reach = np.full((h, w), FILL, np.uint32) if "reach" in want else None
    catch = np.full((h, w), FILL, np.uint32) if "catchment" in want else None
    table = np.frombuffer(bytearray([FILL]) * (48 * capacity), rd.REACH_DTYPE) if "table" in want and capacity else None
    count = ctypes.c_uint32(FILL)
    rc = rd.lib().rdgpu_d8_stream_reaches(_ptr(dirs), ctypes.c_uint8(nodata), w, h, _ptr(chan), _ptr(order), ctypes.c_double(cell[0]),
                                          ctypes.c_double(cell[1]), _ptr(reach), _ptr(catch), _ptr(table),
                                          ctypes.c_uint32(0 if table is None else capacity), ctypes.byref(count))
    assert rc == 0, rc
    return int(count.value), reach, catch, table


def _dev(rd, dirs, nodata=255, chan=None, order=None, cell=(1.0, 1.0), want=("reach", "catchment", "table"), capacity=0):
    """the `_dev` entry on sentinel-filled tensors; the planes not asked for are shown to be left alone"""
    import torch

    h, w = dirs.shape
    t = torch.from_numpy(dirs.copy()).cuda()
    c = None if chan is None else torch.from_numpy(chan.copy()).cuda()
    o = None if order is None else torch.from_numpy(order.copy()).cuda()
    buf = {"reach": torch.full((h, w), FILL, dtype=torch.int32, device="cuda"),
           "catchment": torch.full((h, w), FILL, dtype=torch.int32, device="cuda"),
           "table": torch.full((48 * capacity,), FILL, dtype=torch.uint8, device="cuda")}
    given = {k: buf[k] for k in want if k != "table" or capacity}
    count = rd.d8_stream_reaches_dev(t, nodata, c, o, cell, **given)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dirs) and (c is None or np.array_equal(c.cpu().numpy(), chan))
    assert o is None or np.array_equal(o.cpu().numpy(), order)
    for k in buf:
        if k not in given:
            assert bool((buf[k] == FILL).all()), k + " was not requested but written"
    out = {k: (given[k].cpu().numpy().view(np.uint32) if k in given else None) for k in ("reach", "catchment")}
    table = given["table"].cpu().numpy().view(rd.REACH_DTYPE) if "table" in given else None
    return int(count.cpu().numpy().view(np.uint32)[0]), out["reach"], out["catchment"], table


def _same_records(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.shape, exp.shape)
    a, b = got.view(np.uint8).reshape(-1, 48), exp.view(np.uint8).reshape(-1, 48)   # every field, `length` by its bits
    bad = np.flatnonzero((a != b).any(axis=1))
    print(what, "records differing:", len(bad), "of", len(exp))
    assert len(bad) == 0, (what, bad[:5].tolist(), got[bad[:3]], exp[bad[:3]])


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got != exp).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:5].tolist())


def _check(rd, key, dirs, nodata=255, chan=None, order=None, cell=(1.0, 1.0)):
    exp = _model(key, dirs, nodata, chan, order, cell)
    n = len(exp["table"])
    keep = [None if a is None else a.copy() for a in (dirs, chan, order)]
    for name, entry in (("host", _host), ("dev", _dev)):
        count, reach, catch, table = entry(rd, dirs, nodata, chan, order, cell, capacity=n + 5)
        assert count == n, (key, name, count, n)
        _same(reach, exp["reach"], f"{key} reach {name}")
        _same(catch, exp["catchment"], f"{key} catchment {name}")
        _same_records(table[:n], exp["table"], f"{key} table {name}")
        assert (table[n:].view(np.uint8) == FILL).all(), "records past N were written"
    for a, b in zip((dirs, chan, order), keep):
        assert a is None or np.array_equal(a, b)
    return exp


def _fractal(rd, h, w, holes=False):
    """directions as the flow-path tests take them: the engine's fill and flat resolution of a fractal DEM"""
    from richdem_amd.synth import fractal_dem

    dem = fractal_dem(w, h, seed=7 + h + w)
    filled = rd.FillDepressions(dem)
    if holes:                                            # NoData islands
        filled[h // 3:h // 3 + 3, w // 4:w // 4 + 5] = -9999
        filled[h // 2, w // 2] = -9999
        filled[0, 0] = -9999
    return rd.barnes_flat_resolution_d8(filled, -9999)


@pytest.mark.parametrize("holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests(rd, shape, holes):
    dirs = _fractal(rd, *shape, holes=holes)
    acc = rd.d8_flow_accum(dirs)
    masks = [None] + [rd.d8_channels(acc, thr) for thr in (1.0, 20.0, float(acc.max()) + 1.0)]
    for i, chan in enumerate(masks):
        order = rd.d8_stream_order(dirs, 255, chan)
        cell = (30.0, 10.5) if i == 2 else (1.0, 1.0)       # 30^2 and 10.5^2 are exact: diag is the same double in C and in the model
        e = _check(rd, f"fractal{shape}{holes}{i}", dirs, 255, chan, order, cell)
        t = e["table"]
        assert i != 3 or not chan.any()
        if not ((dirs != 255) & (True if chan is None else chan != 0)).any():   # no channel cell (the smallest shapes, too)
            assert len(t) == 0 and not e["reach"].any() and not e["catchment"].any()
            continue
        assert len(t) > 0 and (t["order"] == order.ravel()[t["top_cell"]]).all()
        # the catchment is the rank of the flow-path engine's drainage cell over the table's bottoms
        bottoms = np.zeros(dirs.shape, np.uint8)
        bottoms.ravel()[t["bottom_cell"]] = 1
        to = rd.d8_flow_path(dirs, 255, bottoms, want=("to_cell",))["to_cell"].ravel()
        label = np.zeros(dirs.size, np.uint32)
        label[t["bottom_cell"]] = np.arange(1, len(t) + 1)
        assert np.array_equal(np.where(to == NONE, 0, label[np.where(to == NONE, 0, to)]), e["catchment"].ravel())


def _junction(jx, jy, shape=(130, 130)):
    """five three-cell tributaries into (jx, jy) from W, N, NW, NE and SW; the junction drains south-east, then east"""
    dirs = sc.blank(*shape)
    cells = []
    for dx, dy in ((-1, 0), (0, -1), (-1, -1), (1, -1), (-1, 1)):
        arm = [(jx + dx * i, jy + dy * i) for i in (3, 2, 1)]
        sc.paint(dirs, arm + [(jx, jy)], last=None)
        cells += arm
    out = [(jx, jy), (jx + 1, jy + 1), (jx + 2, jy + 1), (jx + 3, jy + 1)]
    sc.paint(dirs, out)
    return dirs, sc.mask_of(shape, cells + out)


@pytest.mark.parametrize("at", [(63, 63), (64, 63), (63, 64), (64, 64)], ids=str)
def test_junctions_at_tile_seams(rd, at):
    """the children of the junction, each the bottom of its reach, lie in up to three other tiles than the junction"""
    dirs, mask = _junction(*at)
    e = _check(rd, f"seam{at}", dirs, 255, mask)
    t = e["table"]
    j = at[1] * 130 + at[0]
    assert len(t) == 6 and sorted(t["up"].tolist()) == [0, 0, 0, 0, 0, 5]
    assert t["top_cell"][t["up"] == 5].tolist() == [j] and (t["down"][t["up"] == 0] == e["reach"][at[1], at[0]]).all()
    assert {(b % 130 // 64, b // 130 // 64) for b in t["bottom_cell"].tolist()} >= {(0, 0), ((at[0] + 1) // 64, (at[1] - 1) // 64)}
    _check(rd, f"seam{at}all", dirs)                        # every cell a channel cell


@pytest.mark.parametrize("at", [(8, 5), (62, 62)], ids=str)
def test_loops_with_tributaries(rd, at):
    dirs, loop, feeders = sc.loop_with_tributary(at[0], at[1], (150, 135))
    e = _check(rd, f"looptrib{at}", dirs, 255, sc.mask_of(dirs.shape, loop + feeders))
    t = e["table"]
    assert len(t) == 6 and int((t["up"] == 0).sum()) == 3 and not (t["down"] == 0).any()
    a, b = sorted({int(e["reach"][y, x]) for x, y in loop})
    assert a != 0 and t["down"][a - 1] == b and t["down"][b - 1] == a
    _check(rd, f"looptrib{at}all", dirs)


@pytest.mark.parametrize("at", [(10, 10), (63, 20), (20, 63), (63, 63)], ids=str)
def test_pure_loops(rd, at):
    """a 4-cell loop that nothing joins, inside a tile, across a tile edge, across a tile corner: no reach"""
    x, y = at
    loop = [(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)]
    dirs = sc.paint(sc.blank(130, 135), loop + [loop[0]], last=None)
    e = _check(rd, f"pure{at}", dirs, 255, sc.mask_of(dirs.shape, loop))
    assert len(e["table"]) == 0 and not e["reach"].any() and not e["catchment"].any()
    e = _check(rd, f"pure{at}all", dirs)
    assert len(e["table"]) == dirs.size - 4 and all(e["reach"][cy, cx] == 0 for cx, cy in loop)
    sc.paint(dirs, [(x - 3, y), (x - 2, y), (x - 1, y), (x, y)], last=None)      # a path into the loop draws it into a reach
    e = _check(rd, f"pure{at}fed", dirs, 255, sc.mask_of(dirs.shape, loop))
    assert len(e["table"]) == 0 and not e["catchment"].any()                       # ... but not while the path is off the mask
    e = _check(rd, f"pure{at}fedall", dirs)
    assert all(e["reach"][cy, cx] == e["reach"][y, x] != 0 for cx, cy in loop)
    lab = int(e["reach"][y, x])
    assert e["table"]["down"][lab - 1] == lab and e["table"]["cells"][lab - 1] == 4


def _boustrophedon(h, w):
    """ONE path through every cell: along the rows, alternately east and west, one step south at the end of each"""
    dirs = np.zeros((h, w), np.uint8)
    for y in range(h):
        east = y % 2 == 0
        dirs[y, :] = 5 if east else 1
        dirs[y, w - 1 if east else 0] = 7
    dirs[h - 1, w - 1 if (h - 1) % 2 == 0 else 0] = 0
    return dirs


def test_one_reach_through_every_cell(rd):
    """66 563 cells in one reach: more than a tile's 4095 steps and than 65 535"""
    h, w = 257, 259
    t = _check(rd, "snake", _boustrophedon(h, w), cell=(30.0, 10.5))["table"]
    assert len(t) == 1 and t["cells"][0] == 66563 and int(t["steps"][0, 0]) + int(t["steps"][0, 1]) == 66562
    assert t["catchment_cells"][0] == 66563 and t["length"][0] == (h * (w - 1)) * 30.0 + (h - 1) * 10.5


def test_every_cell_its_own_reach(rd):
    """66 563 reaches, 4096 in a tile: more than the tile's hash table holds and than 65 536 in all"""
    h, w = 257, 259
    e = _check(rd, "lone", np.zeros((h, w), np.uint8))
    t = e["table"]
    assert len(t) == h * w and np.array_equal(e["reach"].ravel(), np.arange(1, h * w + 1, dtype=np.uint32))
    assert (t["cells"] == 1).all() and (t["catchment_cells"] == 1).all() and not t["steps"].any()
    e = _check(rd, "nodata", np.full((h, w), 255, np.uint8))
    assert len(e["table"]) == 0 and not e["catchment"].any()


def test_one_catchment_of_every_cell(rd):
    h, w = 257, 259
    dirs = np.full((h, w), 5, np.uint8)
    dirs[:, w - 1] = 7
    dirs[h - 1, w - 1] = 0
    corner = sc.mask_of((h, w), [(w - 1, h - 1)])
    t = _check(rd, "sink", dirs, 255, corner)["table"]
    assert len(t) == 1 and t["cells"][0] == 1 and t["catchment_cells"][0] == h * w
    column = np.zeros((h, w), np.uint8)
    column[:, w - 1] = 1
    t = _check(rd, "sinkcolumn", dirs, 255, column)["table"]
    assert len(t) == 1 and t["cells"][0] == h and t["catchment_cells"][0] == h * w and t["steps"][0].tolist() == [0, h - 1, 0]


def _fractal_case(rd):
    dirs = _fractal(rd, 65, 130)
    chan = rd.d8_channels(rd.d8_flow_accum(dirs), 20.0)
    order = rd.d8_stream_order(dirs, 255, chan)
    return dirs, chan, order, _model("capacities", dirs, 255, chan, order, (2.0, 3.0))


@pytest.mark.parametrize("entry", [_host, _dev], ids=["host", "dev"])
def test_capacities_and_output_subsets(rd, entry):
    dirs, chan, order, exp = _fractal_case(rd)
    n = len(exp["table"])
    assert n > 8
    for cap in (0, n - 1, n, n + 5):
        count, reach, catch, table = entry(rd, dirs, 255, chan, order, (2.0, 3.0), capacity=cap)
        assert count == n
        _same(reach, exp["reach"], f"capacity {cap} reach")
        _same(catch, exp["catchment"], f"capacity {cap} catchment")
        if cap:
            k = min(n, cap)
            _same_records(table[:k], exp["table"][:k], f"capacity {cap}")
            assert (table[k:].view(np.uint8) == FILL).all()
    for want in (("reach",), ("catchment",), ("table",), ("reach", "table"), ()):
        count, reach, catch, table = entry(rd, dirs, 255, chan, order, (2.0, 3.0), want=want, capacity=n)
        assert count == n                                   # () is the call with only `count`
        assert (reach is None) == ("reach" not in want) and (catch is None) == ("catchment" not in want)
        if reach is not None:
            _same(reach, exp["reach"], f"{want} reach")
        if catch is not None:
            _same(catch, exp["catchment"], f"{want} catchment")
        if "table" in want:
            _same_records(table, exp["table"], f"{want} table")


def test_python_entry_repeatability_and_streams(rd):
    import torch

    dirs, chan, order, exp = _fractal_case(rd)
    n = len(exp["table"])
    got = rd.d8_stream_reaches(dirs, 255, chan, order, (2.0, 3.0))
    assert got["count"] == n and sorted(got) == ["catchment", "count", "reach", "table"]
    _same(got["reach"], exp["reach"], "python reach")
    _same(got["catchment"], exp["catchment"], "python catchment")
    _same_records(got["table"], exp["table"], "python table")
    assert sorted(rd.d8_stream_reaches(dirs, 255, chan, want=())) == ["count"]
    again = _host(rd, dirs, 255, chan, order, (2.0, 3.0), capacity=n)
    rd.release_workspace()
    third = _host(rd, dirs, 255, chan, order, (2.0, 3.0), capacity=n)
    for a, b in zip(again[1:], third[1:]):
        assert a.tobytes() == b.tobytes()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        count, reach, catch, table = _dev(rd, dirs, 255, chan, order, (2.0, 3.0), capacity=n)
    assert count == n
    _same(reach, exp["reach"], "side stream reach")
    _same(catch, exp["catchment"], "side stream catchment")
    _same_records(table, exp["table"], "side stream table")
    small = rd.d8_stream_reaches(dirs[:5, :7].copy())       # a small raster after a larger one: stale scratch must not matter
    e = rm.stream_reaches(dirs[:5, :7].copy())
    _same(small["catchment"], e["catchment"], "small after large")
    _same_records(small["table"], e["table"], "small after large table")
