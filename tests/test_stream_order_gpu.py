"""Channel mask, Strahler stream order and channel-cell kinds on the engine (csrc/streams.hip) against the Python model
(tests/stream_model.py, pinned by tests/test_stream_model.py): host C-ABI and `_dev` entries, bit for bit, every cell.
Shapes are the smallest that reach every path of the kernels: one cell, one row, one column, a tile, one more or less
than a tile, several tiles, channels that cross tile borders many times, junctions on tile corners."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc  # noqa: E402
import stream_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (65, 130), (193, 70), (257, 259)]   # (height, width)
_MODEL = {}


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got != exp).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:5].tolist())


def _model(key, dirs, nodata, chan):
    """the model's order and kinds, computed once per case"""
    if key not in _MODEL:
        order = sm.stream_order(dirs, nodata, chan)
        _MODEL[key] = (order, sm.stream_links(dirs, order, nodata, chan))
    return _MODEL[key]


def _dev(rd, dirs, nodata, chan):
    import torch

    t = torch.from_numpy(dirs.copy()).cuda()
    c = None if chan is None else torch.from_numpy(chan.copy()).cuda()
    order = torch.full(dirs.shape, 77, dtype=torch.uint8, device="cuda")
    kinds = torch.full(dirs.shape, 77, dtype=torch.uint8, device="cuda")
    rd.d8_stream_order_dev(t, order, nodata, c)
    rd.d8_stream_links_dev(t, order, kinds, nodata, c)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dirs) and (c is None or np.array_equal(c.cpu().numpy(), chan))
    return order.cpu().numpy(), kinds.cpu().numpy()


def _check(rd, key, dirs, nodata=255, chan=None):
    exp_o, exp_k = _model(key, dirs, nodata, chan)
    keep = dirs.copy()
    got = rd.d8_stream_order(dirs, nodata, chan)
    _same(got, exp_o, f"{key} order host")
    _same(rd.d8_stream_links(dirs, got, nodata, chan), exp_k, f"{key} kinds host")
    dev_o, dev_k = _dev(rd, dirs, nodata, chan)
    _same(dev_o, exp_o, f"{key} order dev")
    _same(dev_k, exp_k, f"{key} kinds dev")
    assert int((dev_k == sm.ORDER_STEP).sum()) == 0, key + ": an order step"
    assert np.array_equal(dirs, keep)
    return got


def _fractal_dirs(rd, h, w, holes=False):
    from richdem_amd.synth import fractal_dem

    dem = fractal_dem(w, h, seed=7 + h + w)
    filled = rd.FillDepressions(dem)
    if holes:                                            # NoData islands
        filled[h // 3:h // 3 + 3, w // 4:w // 4 + 5] = -9999
        filled[h // 2, w // 2] = -9999
        filled[0, 0] = -9999
    return rd.barnes_flat_resolution_d8(filled, -9999)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests_every_cell_a_channel(rd, shape):
    dirs = _fractal_dirs(rd, *shape)
    order = _check(rd, f"fractal{shape}", dirs)
    print("largest order:", int(order[order != 255].max()), "loop cells:", int((order == 255).sum()), rd.d8_stream_order_stats())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fractal_forests_channels_from_the_engines_accumulation(rd, shape):
    import torch

    dirs = _fractal_dirs(rd, *shape)
    acc = rd.d8_flow_accum(dirs)
    for thr in (4.0, 60.0):
        chan = rd.d8_channels(acc, thr)
        _same(chan, sm.channels(acc, thr), f"{shape} channels host thr {thr}")
        dchan = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
        rd.d8_channels_dev(torch.from_numpy(acc).cuda(), thr, dchan)
        _same(dchan.cpu().numpy(), chan, f"{shape} channels dev thr {thr}")
        _check(rd, f"fractal{shape}thr{thr}", dirs, 255, chan)


def test_serpentine_single_channel_is_all_order_one(rd):
    dirs, chan = sc.serpentine(200)
    order = _check(rd, "serpentine", dirs, 255, chan)
    assert np.array_equal(order, chan)


def test_serpentine_with_a_tributary_at_every_tile_crossing_stays_two(rd):
    dirs, chan = sc.serpentine(200, tributaries=True)
    order = _check(rd, "serpentine+tributaries", dirs, 255, chan)
    assert order.max() == 2 and order[0, 63] == 1 and order[0, 64] == 2 and order[198, 0] == 2


@pytest.mark.parametrize("off", [(0, 0), (1, 1), (37, 5)], ids=str)
def test_perfect_binary_tree_across_twelve_tiles(rd, off):
    """order 8: 255 x 128 cells; with offset (0, 0) the junctions of the upper levels lie on tile corners and edges
    ((63, 64), (191, 64), (127, 0), (31, 96) ...)"""
    dirs, root, cells = sc.binary_tree(8, off[0], off[1], shape=(128 + off[1] + 3, 255 + off[0] + 4))
    order = _check(rd, f"tree8{off}", dirs)
    assert order[root[1], root[0]] == 8
    chan = sc.mask_of(dirs.shape, cells)
    order = _check(rd, f"tree8{off}masked", dirs, 255, chan)
    assert order[root[1], root[0]] == 8 and order.max() == 8


@pytest.mark.parametrize("at", [(64, 64), (63, 64), (64, 63), (128, 64), (70, 70)], ids=str)
def test_three_equal_orders_meeting_from_different_tiles(rd, at):
    dirs = sc.three_way(at[0], at[1], (140, 140))
    order = _check(rd, f"threeway{at}", dirs)
    assert order[at[1], at[0]] == 3


@pytest.mark.parametrize("at", [(63, 63), (8, 5), (63, 20), (100, 127)], ids=str)
def test_direction_loop_with_tributary_and_feeder(rd, at):
    """(63, 63): the loop's four cells lie in four tiles.  The call returns, 255 exactly on the model's cells."""
    dirs, loop, feeders = sc.loop_with_tributary(at[0], at[1], (150, 135))
    order = _check(rd, f"loop{at}", dirs)
    assert sorted(map(tuple, np.argwhere(order == 255)[:, ::-1].tolist())) == sorted(loop)
    chan = sc.mask_of(dirs.shape, loop + feeders)
    _check(rd, f"loop{at}masked", dirs, 255, chan)
    chan[loop[1][1], loop[1][0]] = 0                         # the loop cut by the mask: no loop any more
    order = _check(rd, f"loop{at}cut", dirs, 255, chan)
    assert (order == 255).sum() == 0


def test_long_loop_through_many_tiles(rd):
    h = w = 200
    ring = [(x, 10) for x in range(10, 190)] + [(190, y) for y in range(10, 190)] + [(x, 190) for x in range(190, 10, -1)] + \
           [(10, y) for y in range(190, 10, -1)]
    dirs = sc.paint(sc.blank(h, w), ring + [ring[0]], last=None)
    sc.paint(dirs, [(x, 100) for x in range(20, 11, -1)] + [(11, 100), (10, 100)], last=None)   # a tributary from inside
    order = _check(rd, "ring", dirs)
    assert (order == 255).sum() == len(ring)


@pytest.mark.parametrize("nodata", [255, 9, 3, 0])
def test_nodata_islands_and_other_nodata_codes(rd, nodata):
    dirs = _fractal_dirs(rd, 130, 150, holes=True)
    assert (dirs == 255).sum() >= 17
    dirs = np.where(dirs == 255, np.uint8(nodata), dirs).astype(np.uint8)
    order = _check(rd, f"holes nodata {nodata}", dirs, nodata)
    assert (order[dirs == nodata] == 0).all() and (order[dirs != nodata] != 0).all()


def test_mask_that_is_not_closed_downstream(rd):
    dirs = _fractal_dirs(rd, 130, 150)
    rng = np.random.default_rng(5)
    chan = (rng.random(dirs.shape) < 0.8).astype(np.uint8) * 3           # any non-zero value is a channel
    _check(rd, "open mask", dirs, 255, chan)


def test_argument_errors_leave_the_output_untouched(rd):
    L = rd.lib()
    dirs = np.zeros((4, 5), np.uint8)
    acc = np.ones((4, 5), np.float64)
    out = np.full((4, 5), 77, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd = ctypes.c_uint8(255)
    ARG = 2
    calls = [
        L.rdgpu_d8_stream_order(None, nd, 5, 4, None, p(out)),
        L.rdgpu_d8_stream_order(p(dirs), nd, 5, 4, None, None),
        L.rdgpu_d8_stream_order(p(dirs), nd, 0, 4, None, p(out)),
        L.rdgpu_d8_stream_order(p(dirs), nd, 5, -1, None, p(out)),
        L.rdgpu_d8_stream_order(p(dirs), nd, 70000, 70000, None, p(out)),
        L.rdgpu_d8_stream_order_dev(None, nd, 5, 4, None, p(out), None),
        L.rdgpu_d8_stream_order_dev(p(dirs), nd, 5, 0, None, p(out), None),
        L.rdgpu_d8_channels_f64(None, ctypes.c_double(-1), ctypes.c_double(1), 5, 4, p(out)),
        L.rdgpu_d8_channels_f64(p(acc), ctypes.c_double(-1), ctypes.c_double(float("nan")), 5, 4, p(out)),
        L.rdgpu_d8_channels_f64(p(acc), ctypes.c_double(-1), ctypes.c_double(float("inf")), 5, 4, p(out)),
        L.rdgpu_d8_channels_f64(p(acc), ctypes.c_double(-1), ctypes.c_double(1), 5, 0, p(out)),
        L.rdgpu_d8_channels_dev_f64(p(acc), ctypes.c_double(-1), ctypes.c_double(float("-inf")), 5, 4, p(out), None),
        L.rdgpu_d8_stream_links(p(dirs), nd, 5, 4, None, None, p(out)),
        L.rdgpu_d8_stream_links(p(dirs), nd, 5, 4, None, p(dirs), None),
        L.rdgpu_d8_stream_links(p(dirs), nd, -5, 4, None, p(dirs), p(out)),
        L.rdgpu_d8_stream_links_dev(None, nd, 5, 4, None, p(dirs), p(out), None),
    ]
    assert calls == [ARG] * len(calls), calls
    assert (out == 77).all()
    with pytest.raises(rd.RdgpuError):
        rd.d8_stream_order(dirs.astype(np.int32))
    with pytest.raises(rd.RdgpuError):
        rd.d8_stream_order(dirs, 255, np.zeros((3, 3), np.uint8))
    with pytest.raises(rd.RdgpuError):
        rd.d8_channels(acc, float("nan"))


def test_same_result_after_the_workspace_is_released(rd):
    dirs = _fractal_dirs(rd, 193, 70)
    first = rd.d8_stream_order(dirs)
    rd.release_workspace()
    _same(rd.d8_stream_order(dirs), first, "after release_workspace")
    small = rd.d8_stream_order(dirs[:5, :7].copy())          # a small raster after a larger one: stale scratch must not matter
    _same(small, sm.stream_order(dirs[:5, :7]), "small after large")
    _same(rd.d8_stream_order(dirs), first, "large after small")
