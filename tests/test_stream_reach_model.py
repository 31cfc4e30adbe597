"""Pins tests/stream_reach_model.py (the stand-in reference of the stream reaches) on the hand-built forests of
tests/stream_cases.py, checks the invariants the definitions imply on those and on random rasters, the engine's
formulation ("the first reach-bottom on the path") against the flow-path model, the C-ABI's argument errors and the
record layout, none of which needs a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_path_model as fm  # noqa: E402
import stream_cases as sc  # noqa: E402
import stream_model as sm  # noqa: E402
import stream_reach_model as rm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _invariants(dirs, nodata=255, chan=None):
    """what the definitions imply, whatever the raster; returns the model's result"""
    r = rm.stream_reaches(dirs, nodata, chan)
    t, reach, catch = r["table"], r["reach"].ravel(), r["catchment"].ravel()
    n = len(t)
    m = sm.channel_mask(dirs, nodata, chan).ravel()
    ctgt, _ = sm._targets(dirs, nodata, chan)
    assert (reach[~m] == 0).all() and reach.max(initial=0) == n
    assert int(t["cells"].sum()) == int((reach != 0).sum())
    assert int(t["steps"].sum()) == int(((reach != 0) & (ctgt >= 0)).sum())
    assert int(t["catchment_cells"].sum()) == int((catch != 0).sum())
    assert (catch[m] == reach[m]).all()
    assert (catch[dirs.ravel() == nodata] == 0).all()
    assert (np.diff(t["bottom_cell"].astype(np.int64)) > 0).all()
    assert np.array_equal(t["up"], np.bincount(t["down"], minlength=n + 1)[1:]) and not (t["up"] == 1).any()
    assert (reach[t["top_cell"]] == np.arange(1, n + 1)).all() and (reach[t["bottom_cell"]] == np.arange(1, n + 1)).all()
    assert np.array_equal(np.bincount(reach, minlength=n + 1)[1:], t["cells"])
    order = sm.stream_order(dirs, nodata, chan).ravel()
    for lab in range(1, n + 1):                                             # the order is constant along a reach
        assert len(set(order[reach == lab].tolist())) == 1
    # the engine's route: 1 + rank of the first reach-bottom on the path
    to = fm.flow_path(dirs, nodata, r["bottoms"])["to_cell"].ravel()
    rank = np.cumsum(r["bottoms"].ravel(), dtype=np.int64)                  # inclusive: 1 + the exclusive rank at a bottom
    exp = np.where(to == fm.NONE, 0, rank[np.where(to == fm.NONE, 0, to)])
    assert np.array_equal(catch, exp.astype(np.uint32))
    return r


def _kinds(t):
    return {"n": len(t), "heads": int((t["up"] == 0).sum()), "mouths": int((t["down"] == 0).sum())}


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_binary_tree(k):
    dirs, root, cells = sc.binary_tree(k)
    r = _invariants(dirs, 255, sc.mask_of(dirs.shape, cells))
    t = r["table"]
    assert _kinds(t) == {"n": 2 ** k - 1, "heads": 2 ** (k - 1), "mouths": 1}
    assert (t["up"][t["up"] != 0] == 2).all()
    assert t["bottom_cell"][t["down"] == 0].tolist() == [root[1] * dirs.shape[1] + root[0]]
    if k == 5:
        assert int(t["cells"].max()) == 8
    assert (t["steps"][:, :2] == 0).all() and (t["length"] == t["steps"][:, 2] * np.sqrt(2.0)).all()   # every step is diagonal


def test_three_way_junction():
    dirs = sc.three_way(8, 8, (18, 18))
    mask = (dirs != 0).astype(np.uint8)
    mask[8, 8] = 1
    r = _invariants(dirs, 255, mask)
    t = r["table"]
    assert _kinds(t) == {"n": 10, "heads": 6, "mouths": 1}
    mouth = t[t["down"] == 0][0]
    assert mouth["up"] == 3 and mouth["top_cell"] == mouth["bottom_cell"] == 8 * 18 + 8 and mouth["cells"] == 1
    assert mouth["steps"].tolist() == [0, 0, 0] and mouth["length"] == 0.0


def test_serpentine():
    dirs, mask = sc.serpentine(200)
    t = _invariants(dirs, 255, mask)["table"]
    assert len(t) == 1 and t["cells"][0] == 20099 and t["up"][0] == 0 and t["down"][0] == 0
    assert int(t["steps"][0].sum()) == 20098 and t["steps"][0, 2] == 0
    dirs, mask = sc.serpentine(200, tributaries=True)
    t = _invariants(dirs, 255, mask)["table"]
    assert _kinds(t) == {"n": 601, "heads": 301, "mouths": 1} and int(t["cells"].max()) == 129


def test_loop_with_tributary():
    dirs, loop, feeders = sc.loop_with_tributary(8, 5, (16, 20))
    r = _invariants(dirs, 255, sc.mask_of(dirs.shape, loop + feeders))
    t = r["table"]
    assert _kinds(t) == {"n": 6, "heads": 3, "mouths": 0}
    on_loop = sorted({int(r["reach"][y, x]) for x, y in loop})
    assert len(on_loop) == 2 and 0 not in on_loop
    a, b = on_loop
    assert t["down"][a - 1] == b and t["down"][b - 1] == a                  # the loop: two reaches, each the other's `down`
    assert int(t["cells"][a - 1] + t["cells"][b - 1]) == 4
    assert (r["catchment"][r["reach"] == 0] == 0).all()                      # off the mask nothing flows (background code 0)


def test_pure_loop():
    dirs = sc.blank(6, 6)
    loop = [(2, 2), (3, 2), (3, 3), (2, 3)]
    sc.paint(dirs, loop + [loop[0]], last=None)
    r = _invariants(dirs, 255, sc.mask_of(dirs.shape, loop))
    assert len(r["table"]) == 0 and not r["reach"].any() and not r["catchment"].any()
    r = _invariants(dirs)
    t = r["table"]
    assert len(t) == 32 and (t["cells"] == 1).all() and (t["top_cell"] == t["bottom_cell"]).all()
    assert all(r["reach"][y, x] == 0 for x, y in loop) and int((r["reach"] == 0).sum()) == 4
    feeder = sc.paint(dirs.copy(), [(0, 2), (1, 2), (2, 2)], last=None)       # a path INTO the loop: its cells have reaches,
    r = _invariants(feeder)                                                  # the loop is now reaches too
    assert all(r["reach"][y, x] != 0 for x, y in loop)


@pytest.mark.parametrize("seed", range(40))
def test_invariants_on_random_rasters(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
    dirs = rng.integers(0, 9, (h, w)).astype(np.uint8)
    dirs[rng.random((h, w)) < 0.1] = 255
    _invariants(dirs)
    _invariants(dirs, 255, (rng.random((h, w)) < 0.6).astype(np.uint8))
    _invariants(dirs, int(rng.integers(1, 9)))                                # a NoData code that is also a direction


def test_the_model_is_linear_in_the_cells():
    """one path through every cell of 257 x 259: seconds, not hours"""
    h, w = 257, 259
    dirs = np.zeros((h, w), np.uint8)
    for y in range(h):
        dirs[y, :] = 5 if y % 2 == 0 else 1
        dirs[y, w - 1 if y % 2 == 0 else 0] = 7
    dirs[h - 1, w - 1] = 0
    r = rm.stream_reaches(dirs)
    t = r["table"]
    assert len(t) == 1 and t["cells"][0] == h * w and int(t["steps"][0, 0] + t["steps"][0, 1]) == h * w - 1
    assert t["catchment_cells"][0] == h * w and (r["reach"] == 1).all()


def test_record_layout_is_the_headers(rd, tmp_path):
    assert rd.REACH_DTYPE == rm.REACH_DTYPE and rd.REACH_DTYPE.itemsize == 48
    fields = ["top_cell", "bottom_cell", "down", "up", "cells", "catchment_cells", "steps", "order", "length"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rdgpu.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(rdgpu_reach)'
                   + "".join(f", offsetof(rdgpu_reach, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == rd.REACH_DTYPE.itemsize
    assert out[1:] == [rd.REACH_DTYPE.fields[f][1] for f in fields]
    assert rd.REACH_DTYPE.fields["steps"][0].shape == (3,)


def test_argument_errors_need_no_gpu(rd):
    L = rd.lib()
    dirs = np.zeros((4, 5), np.uint8)
    plane = np.full((4, 5), 77, np.uint32)
    table = np.zeros(3, rd.REACH_DTYPE)
    table["cells"] = 77
    count = ctypes.c_uint32(77)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd, one, cnt = ctypes.c_uint8(255), ctypes.c_double(1.0), ctypes.byref(count)
    u = ctypes.c_uint32
    f = L.rdgpu_d8_stream_reaches
    g = L.rdgpu_d8_stream_reaches_dev
    ARG = 2
    calls = [
        f(None, nd, 5, 4, None, None, one, one, p(plane), p(plane), p(table), u(3), cnt),                       # null dirs
        f(p(dirs), nd, 5, 4, None, None, one, one, p(plane), p(plane), p(table), u(3), None),                   # null count
        f(p(dirs), nd, 5, 4, None, None, one, one, p(plane), p(plane), None, u(3), cnt),                        # null table, capacity 3
        f(p(dirs), nd, 0, 4, None, None, one, one, p(plane), None, p(table), u(3), cnt),
        f(p(dirs), nd, 5, -4, None, None, one, one, p(plane), None, p(table), u(3), cnt),
        f(p(dirs), nd, 70000, 70000, None, None, one, one, p(plane), None, p(table), u(3), cnt),                # too many cells
        f(p(dirs), nd, 5, 4, None, None, ctypes.c_double(0.0), one, p(plane), None, p(table), u(3), cnt),
        f(p(dirs), nd, 5, 4, None, None, one, ctypes.c_double(float("nan")), p(plane), None, p(table), u(3), cnt),
        f(p(dirs), nd, 5, 4, None, None, ctypes.c_double(float("inf")), one, p(plane), None, p(table), u(3), cnt),
        g(None, nd, 5, 4, None, None, one, one, p(plane), None, p(table), u(3), cnt, None),
        g(p(dirs), nd, 5, 4, None, None, one, one, p(plane), None, p(table), u(3), None, None),
        g(p(dirs), nd, 5, 4, None, None, one, one, p(plane), None, None, u(3), cnt, None),
        g(p(dirs), nd, 5, 0, None, None, one, one, p(plane), None, p(table), u(3), cnt, None),
        g(p(dirs), nd, 5, 4, None, None, one, ctypes.c_double(0.0), p(plane), None, p(table), u(3), cnt, None),
    ]
    assert calls == [ARG] * len(calls), calls
    assert (plane == 77).all() and (table["cells"] == 77).all() and count.value == 77
    with pytest.raises(rd.RdgpuError):
        rd.d8_stream_reaches(dirs.astype(np.int32))
    with pytest.raises(rd.RdgpuError):
        rd.d8_stream_reaches(dirs, want=("links",))
    with pytest.raises(rd.RdgpuError):
        rd.d8_stream_reaches(dirs, channels=np.zeros((3, 3), np.uint8))
    with pytest.raises(rd.RdgpuError):
        rd.d8_stream_reaches(dirs, order=np.zeros((4, 5), np.int32))
    with pytest.raises(rd.RdgpuError):
        rd.d8_stream_reaches(dirs, cell=(0.0, 1.0))
