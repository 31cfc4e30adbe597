"""Reverse accumulation, largest weight downslope and upslope dependence over D-infinity / MFD proportions on the engine
(csrc/mfd_reverse.hip) against the Python model (tests/mfd_reverse_model.py, pinned by tests/test_mfd_reverse_model.py):
host C-ABI and `_dev` entries, every requested plane on every cell, bit for bit, inputs unchanged, unrequested planes left
alone.

The proportions of the DEM cases come from the CPU oracle, so the model and the engine see identical floats.  The DEMs
are UNFILLED fractals.  Hand-made proportion rasters (the generators of tests/test_mfd_distance_gpu.py, restated) reach
what a DEM does not: a chain longer than 65 535 cells, eight receivers, eight donors completed by one thread, the spill of
a wavefront's stack and the hand-over of a thread's buffer (proven from the launch count), cycles, shares into NoData,
shares that do not sum to 1.

Proportions layout [h, w, 9]: slot 0 is the marker (-2 NoData), slots 1..8 the shares to the neighbours 1 left, 2 up-left,
3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left."""
import ctypes
import os
import sys

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfd_reverse_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
LEFT, UPLEFT, UP, UPRIGHT, RIGHT, DOWNRIGHT, DOWN, DOWNLEFT = range(1, 9)
NDV = np.float32(-9999)
SENT = 77.0
PLANES = ("racc", "wmax")
ENV = "RDGPU_MFD_DISTANCE_STACK_BELOW"
STACK_BELOW = [None, "0", "4294967295"]      # the default; always k_wl_buffer; always k_wl_stack
MODE = {None: "default", "0": "round", "4294967295": "stack"}
_CACHE = {}


def _same(got, exp, what):
    assert got.dtype == np.float64 and got.shape == exp.shape, (what, got.dtype, got.shape)
    diff = got.view(np.uint64) != exp.view(np.uint64)
    bad = int(diff.sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(diff)[:5].tolist(), got[diff][:5].tolist(), exp[diff][:5].tolist())


def _setenv(monkeypatch, stack_below):
    if stack_below is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, stack_below)


def _dev(rd, props, wts, dest, wnd, nd, want, stream=None):
    """the `_dev` entry on sentinel-filled tensors: the planes asked for, and the proof that the others were left alone"""
    import torch

    h, w = props.shape[:2]
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        tp = torch.from_numpy(props.copy()).cuda()
        tw = None if wts is None else torch.from_numpy(wts.copy()).cuda()
        td = None if dest is None else torch.from_numpy(dest.copy()).cuda()
        buf = {k: torch.full((h, w), SENT, dtype=torch.float64, device="cuda") for k in PLANES}
        rd.mfd_reverse_accum_dev(tp, tw, td, wnd, nd, **{k: buf[k] for k in want})
        after = {k: v + 0.0 for k, v in buf.items()}             # (work that must come after the call)
    torch.cuda.synchronize()
    assert np.array_equal(tp.cpu().numpy(), props) and (td is None or np.array_equal(td.cpu().numpy(), dest))
    assert tw is None or np.array_equal(tw.cpu().numpy().view(np.uint64), wts.view(np.uint64))
    for k in PLANES:
        if k not in want:
            assert bool((after[k] == SENT).all()), k + " was not requested but written"
    return {k: after[k].cpu().numpy() for k in want}


def _check(rd, name, props, wts, dest, wnd, exp, wants=None, nd=-1.0, dev=True):
    """host and `_dev` against the model for each set of planes in `wants`"""
    if wants is None:
        wants = [("racc",)] if wts is None else [("racc", "wmax"), ("wmax",), ("racc",)]
    keep = props.copy(), None if wts is None else wts.copy(), None if dest is None else dest.copy()
    for want in wants:
        got = rd.mfd_reverse_accum(props, wts, dest, wnd, nd, want=want)
        assert tuple(got) == tuple(want)
        for k in want:
            _same(got[k], exp[k], f"{name} want={want} {k} host")
        if dev:
            d = _dev(rd, props, wts, dest, wnd, nd, want)
            for k in want:
                _same(d[k], exp[k], f"{name} want={want} {k} dev")
    assert np.array_equal(props, keep[0]) and (dest is None or np.array_equal(dest, keep[2]))
    assert wts is None or np.array_equal(wts.view(np.uint64), keep[1].view(np.uint64))


# ---- 1: proportions of the CPU oracle on unfilled fractal DEMs ---------------------------------------------------
def _dem(which):
    if which == "small":
        return fractal_dem(130, 70, 11)
    dem = fractal_dem(260, 200, 305)
    if which == "big_nodata":
        dem[90:100, 120:150] = NDV
        dem[0:7, 200:215] = NDV
        dem[150:170, 0:3] = NDV
        dem[60, 61] = NDV
    return dem


def _props(orc, dem, kind):
    if kind == "dinf":
        return orc.port.fm_tarboton(dem, NDV)
    if kind == "quinn":
        return orc.port.fm_mfd(dem, NDV, "Quinn")
    if kind == "holmgren2":
        return orc.port.fm_mfd(dem, NDV, "Holmgren", 2.0)
    return orc.port.fm_d8(dem, NDV)


WND = -3.0


def _case(orc, which, kind):
    """the three runs of a DEM case: (a) the dependence on the channels, (b) integer-valued weights without dest, (c)
    non-dyadic weights with 5 % NaN or weight_nodata and dest"""
    key = (which, kind)
    if key not in _CACHE:
        dem = _dem(which)
        props = _props(orc, dem, kind)
        h, w = dem.shape
        dest = (orc.port.flow_accumulation(props) >= 30).astype(np.uint8)
        rng = np.random.default_rng(len(which) * 100 + len(kind))
        wb = rng.integers(0, 100, (h, w)).astype(np.float64)
        wc = rng.random((h, w))
        holes = rng.random((h, w))
        wc[holes < 0.025] = float("nan")
        wc[(holes >= 0.025) & (holes < 0.05)] = WND
        runs = {"a": (None, dest, None, model.reverse_accum(props, None, dest)),
                "b": (wb, None, None, model.reverse_accum(props, wb, None)),
                "c": (wc, dest, WND, model.reverse_accum(props, wc, dest, WND))}
        for a in (props, dest, wb, wc):
            a.setflags(write=False)
        _CACHE[key] = (props, runs)
    return _CACHE[key]


DEM_CASES = [(which, kind) for which in ("small", "big", "big_nodata") for kind in ("dinf", "quinn", "holmgren2", "d8")]


@pytest.mark.parametrize("which,kind", DEM_CASES, ids=[f"{a}-{b}" for a, b in DEM_CASES])
def test_oracle_proportions_vs_model(rd, orc, monkeypatch, which, kind):
    monkeypatch.delenv(ENV, raising=False)
    props, runs = _case(orc, which, kind)
    data = props[..., 0] != -2.0
    dep = runs["a"][3]
    several = float((dep["nrecv"][data] >= 2).mean())
    between = float(((dep["racc"][data] > 0.0) & (dep["racc"][data] < 1.0)).mean())
    print(f"{which} {kind}: several receivers {several:.3f}, dependence strictly between 0 and 1 {between:.3f}")
    for r in runs.values():
        assert (r[3]["state"][data] != model.UNDECIDED).all()            # every data cell is decided
    if kind == "d8":
        assert between == 0.0
    else:
        assert several >= 0.60
        assert between >= (0.30 if kind == "dinf" else 0.50)
    assert (runs["c"][3]["state"] == model.EMPTY).sum() >= 1
    for tag, (wts, dest, wnd, exp) in runs.items():
        _check(rd, f"{which}-{kind}-{tag}", props, wts, dest, wnd, exp)
        assert rd.mfd_distance_rounds() >= 1
    _same(rd.mfd_upslope_dependence(props, runs["a"][1]), dep["racc"], f"{which}-{kind} mfd_upslope_dependence")


# ---- 2: shapes ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (64, 65), (257, 259)]   # (height, width)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_shapes(rd, orc, monkeypatch, shape):
    """the raster-edge rules, the block edges of the list compaction (4096 cells) and the grid-stride loops"""
    monkeypatch.delenv(ENV, raising=False)
    h, w = shape
    rng = np.random.default_rng(1000 + h * 1000 + w)
    y, x = np.mgrid[0:h, 0:w]
    dem = (rng.random((h, w)) * 6.0 + 0.05 * x + 0.03 * y).astype(np.float32)
    if h * w > 100:
        dem[rng.random((h, w)) < 0.02] = NDV
    dest = (rng.random((h, w)) < 0.05).astype(np.uint8)
    wts = rng.random((h, w)) * 10.0 - 5.0
    wts[rng.random((h, w)) < 0.1] = 2.0
    for kind in ("dinf", "quinn"):
        props = _props(orc, dem, kind)
        _check(rd, f"{h}x{w}-{kind}-w", props, wts, dest, 2.0, model.reverse_accum(props, wts, dest, 2.0, out_nodata=-5.0), nd=-5.0)
        _check(rd, f"{h}x{w}-{kind}-dep", props, None, dest, None, model.reverse_accum(props, None, dest, out_nodata=-5.0), nd=-5.0)
        _check(rd, f"{h}x{w}-{kind}-nodest", props, wts, None, None, model.reverse_accum(props, wts, None, out_nodata=-5.0), nd=-5.0,
               wants=[("racc", "wmax")])


# ---- 3: hand-made proportion rasters (tests/test_mfd_distance_gpu.py's, restated) --------------------------------
def blank(h, w):
    p = np.full((h, w, 9), -1.0, np.float32)
    p[..., 0] = -2.0
    return p


def put(p, y, x, shares=None):
    """name cell (y, x): a data cell with the shares {n: share}"""
    p[y, x, 0] = 0.0 if shares else -1.0
    for n, s in (shares or {}).items():
        p[y, x, n] = s


def chain_into(p, y, x, n, length):
    """`length` cells that each give share 1 to the next in direction n and end by flowing INTO (y, x), which is not touched"""
    for k in range(1, length + 1):
        put(p, y - k * DY[n], x - k * DX[n], {n: 1.0})


def serpentine(size=260):
    """every interior cell of a size x size raster on one chain: 66 564 cells for 260, more than 65 535; the chain ends in
    (1, 1) and its far end is 66 563 steps away"""
    p = blank(size, size)
    for y in range(1, size - 1):
        east = (y % 2) == 1                     # odd rows were laid left to right, so their cells flow back LEFT
        for x in range(1, size - 1):
            first = x == (1 if east else size - 2)
            put(p, y, x, ({UP: 1.0} if y > 1 else None) if first else {LEFT if east else RIGHT: 1.0})
    return p


def eight_receivers():
    """(10, 10) shares to all eight neighbours (fractions that do not sum to 1); neighbour n leads a chain of n more cells"""
    p = blank(21, 21)
    put(p, 10, 10, {n: np.float32(0.03 * n + 0.01) for n in range(1, 9)})
    for n in range(1, 9):
        for k in range(1, n + 1):
            put(p, 10 + k * DY[n], 10 + k * DX[n], {n: 1.0})
        put(p, 10 + (n + 1) * DY[n], 10 + (n + 1) * DX[n])
    return p


def hubs(size=60, pitch=7):
    """a lattice of cells without receivers; each of the eight neighbours of one flows into it and is the end of a ray of 2
    more cells: the hub's thread completes eight donors in one step, continues with one and hands seven on"""
    p = blank(size, size)
    for cy in range(4, size - 4, pitch):
        for cx in range(4, size - 4, pitch):
            put(p, cy, cx)
            for n in range(1, 9):
                chain_into(p, cy, cx, n, 3)
    return p


def comb(lengths, side=3, pitch=4):
    """Horizontal trunks, `pitch` rows apart, that flow LEFT into their head in column 1 (the only cells of the raster
    without a receiver); below every trunk cell hangs a chain of `side` cells that flows UP into it.  The thread of a head
    walks its trunk to the right (the lowest neighbour number it completed) and hands on one side chain per step."""
    nt, width = len(lengths), max(lengths) + 2
    p = blank(nt * pitch + 2, width)
    for i, ln in enumerate(lengths):
        y = 1 + i * pitch
        for x in range(1, ln + 1):
            put(p, y, x, {LEFT: 1.0} if x > 1 else None)
            if x > 1:
                chain_into(p, y, x, UP, side)
    return p


def ring(absorb):
    """(1, 1) -> (1, 2) -> (2, 2) -> (2, 1) -> (1, 1); a chain of 10 cells feeds (1, 2) from the right.  (1, 1) also gives to
    the edge cell (2, 0): the one cell of the first work list when the ring has no absorbing cell -- it takes (1, 1)'s counter
    from 2 to 1, where it stays."""
    p = blank(4, 15)
    put(p, 1, 1, {RIGHT: 0.5, DOWNLEFT: 0.5})
    put(p, 2, 0)
    put(p, 1, 2, {DOWN: 1.0})
    put(p, 2, 2, {LEFT: 1.0})
    put(p, 2, 1, {UP: 1.0})
    chain_into(p, 1, 2, LEFT, 10)
    dest = np.zeros((4, 15), np.uint8)
    if absorb:
        dest[2, 2] = 1
    else:
        dest[0, 0] = 1                      # (a mask without an absorbing cell on the data)
    return p, dest


def into_nodata():
    p = blank(6, 8)
    put(p, 1, 1, {RIGHT: 0.5, UP: 0.5, DOWN: 0.25})     # up and down are NoData: dropped, one receiver is left
    put(p, 1, 2, {RIGHT: 0.7, DOWNRIGHT: 0.2, UP: 0.4})
    put(p, 1, 3, {RIGHT: 1.0})
    put(p, 1, 4, {UP: 1.0})                             # its only share goes into NoData
    put(p, 2, 3, {RIGHT: 0.125, DOWN: 0.5})
    put(p, 2, 4, {RIGHT: 1.0})
    put(p, 2, 5, {RIGHT: 1.0})
    put(p, 2, 6, {RIGHT: 1.0})
    put(p, 2, 7, {LEFT: 1.0})                           # an edge cell with a positive share: no receivers
    put(p, 3, 3)
    return p


def fractions():
    """shares that do not sum to 1 on a 3-wide braid: every cell gives 0.5, 0.25 and 0.125 to the three cells below it"""
    p = blank(40, 9)
    for y in range(1, 38):
        for x in range(2, 7):
            put(p, y, x, {DOWNLEFT: 0.5, DOWN: 0.25, DOWNRIGHT: 0.125})
    for x in range(1, 8):
        put(p, 38, x)
        if x in (1, 7):
            for y in range(2, 38):
                put(p, y, x, {DOWN: 1.0})
    return p


HAND = {
    "comb_spill": lambda: (comb([40] * 64), None),                      # 258 x 42: the later steps of the wavefront spill
    "comb_control": lambda: (comb([40] * 8), None),                     # 56 idle lanes pop what 8 push
    "comb_two_waves": lambda: (comb([40] * 128), None),
    "comb_ragged": lambda: (comb([20 + (7 * i) % 61 for i in range(64)]), None),
    "comb_short": lambda: (comb([12] * 64), None),                      # 11 hand-ons per thread fit in the buffer
    "eight_receivers": lambda: (eight_receivers(), None),
    "hubs": lambda: (hubs(), None),
    "cycle": lambda: ring(False),
    "cycle_with_absorbing": lambda: ring(True),
    "into_nodata": lambda: (into_nodata(), None),
    "fractions": lambda: (fractions(), None),
}

# Launch counts that follow from WL_CAP = 1536 (entries of a wavefront's stack) and WL_BUF = 20 (entries of a thread's buffer),
# by (raster, forced kernel).  The first list is the 64 (8, 128) trunk heads in row-major order: one lane each.
#  stack, 64 trunks of 40: every step of the wavefront pushes 64 side chains and no lane is idle before the trunks end, so
#    the stack (1536) is full after 24 of the 39 steps and the later steps spill: a second launch.  8 trunks: 56 idle lanes
#    pop what 8 push; 64 trunks of 12: 64 x 11 = 704 entries: one launch.
#  round, trunks of 12: a thread buffers 11 side chains (nb + 8 <= 20 throughout), they are launch two and each is walked
#    inline.  Trunks of 40: after 13 buffered chains (nb + 8 > 20) the thread hands its trunk cell over: the trunk alone
#    takes three launches.
#  the cycles: the chain is one thread's inline walk and the ring never completes (or is walked inline from its absorbing cell).
EXPECT_ROUNDS = {
    ("comb_control", "stack"): ("==", 1), ("comb_short", "stack"): ("==", 1),
    ("comb_spill", "stack"): (">=", 2), ("comb_two_waves", "stack"): (">=", 2),
    ("comb_short", "round"): ("==", 2), ("comb_spill", "round"): (">=", 3),
    ("cycle", "stack"): ("<=", 2), ("cycle", "round"): ("<=", 2), ("cycle", "default"): ("<=", 2),
    ("cycle_with_absorbing", "stack"): ("<=", 2), ("cycle_with_absorbing", "round"): ("<=", 2),
}


def _hand(name):
    if name not in _CACHE:
        p, dest = HAND[name]()
        h, w = p.shape[:2]
        rng = np.random.default_rng(len(name))
        wts = rng.random((h, w)) * 100.0 - 30.0
        wts[rng.random((h, w)) < 0.05] = float("nan")
        exp = model.reverse_accum(p, wts, dest, None)
        dep = None
        if dest is not None:
            dep = model.reverse_accum(p, None, dest)
        _CACHE[name] = (p, dest, wts, exp, dep)
    return _CACHE[name]


@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_graphs(rd, monkeypatch, name, stack_below):
    """every kernel of the work list, selected by the engine's switch, gives the model's bits"""
    _setenv(monkeypatch, stack_below)
    p, dest, wts, exp, dep = _hand(name)
    _check(rd, f"{name} {MODE[stack_below]}", p, wts, dest, None, exp, dev=stack_below is None)
    if dep is not None:
        _check(rd, f"{name} {MODE[stack_below]} dependence", p, None, dest, None, dep, dev=stack_below is None)
    rd.mfd_reverse_accum(p, wts, dest)
    rounds = rd.mfd_distance_rounds()
    print(f"rounds {name} {MODE[stack_below]}: {rounds}")
    op, bound = EXPECT_ROUNDS.get((name, MODE[stack_below]), (">=", 1))
    assert {"==": rounds == bound, ">=": rounds >= bound, "<=": rounds <= bound}[op], (name, MODE[stack_below], rounds, op, bound)


def test_hand_made_graphs_are_what_the_cases_need():
    """the rasters themselves (no engine): first lists, sizes and the values that the descriptions above promise"""
    for name, ntr in (("comb_spill", 64), ("comb_control", 8), ("comb_two_waves", 128), ("comb_ragged", 64), ("comb_short", 64)):
        p, _, _, exp, _ = _hand(name)
        data = p[..., 0] != -2.0
        first = data & (exp["nrecv"] == 0)
        assert first.sum() == ntr and first[:, 1].sum() == ntr, name          # the trunk heads and nothing else
        assert (exp["state"][data] != model.UNDECIDED).all()
    assert _hand("comb_spill")[0].shape == (258, 42, 9)
    p, _, _, exp, _ = _hand("eight_receivers")
    assert exp["nrecv"][10, 10] == 8 and not np.isclose(float(p[10, 10, 1:].sum()), 1.0)
    ones = model.reverse_accum(p, np.ones(p.shape[:2]))["racc"]
    s = 1.0
    for n in range(1, 9):
        s = s + float(p[10, 10, n]) * float(n + 1)                            # neighbour n heads a chain of n + 1 cells
    assert ones[10, 10] == s
    p, _, _, exp, _ = _hand("hubs")
    assert exp["nrecv"].max() == 1 and all((p[3:6, 3:6, n] > 0).sum() >= 1 for n in range(1, 9))
    assert model.reverse_accum(p, np.ones(p.shape[:2]))["racc"][4, 1] == 4.0
    s = _hand("cycle")[3]["state"]
    assert (s[1:3, 1:3] == model.UNDECIDED).all() and (s[1, 3:13] == model.UNDECIDED).all() and s[2, 0] != model.UNDECIDED
    assert (_hand("cycle")[3]["racc"][1, 3:13] == -1.0).all()
    e = _hand("cycle_with_absorbing")
    assert (e[3]["state"][1:3, 1:3] != model.UNDECIDED).all()
    assert e[4]["racc"][2, 2] == 1.0 and e[4]["racc"][1, 2] == 1.0 and e[4]["racc"][1, 1] == 0.5 and e[4]["racc"][1, 12] == 1.0
    e = _hand("into_nodata")[3]
    assert e["nrecv"][1, 1] == 1 and e["nrecv"][1, 4] == 0 and e["nrecv"][2, 7] == 0 and e["nrecv"][1, 2] == 2
    e = _hand("fractions")[3]
    assert e["nrecv"][5, 4] == 3 and (e["state"][1:38, 2:7] != model.UNDECIDED).all()


@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
def test_serpentine_longer_than_65535(rd, monkeypatch, stack_below):
    """one chain through 66 564 cells with unit weights: one thread's inline walk; racc counts the cells down to the end exactly"""
    _setenv(monkeypatch, stack_below)
    if "serpentine" not in _CACHE:
        p = serpentine()
        ones = np.ones(p.shape[:2])
        _CACHE["serpentine"] = (p, ones, model.reverse_accum(p, ones))
    p, ones, exp = _CACHE["serpentine"]
    a = exp["racc"]
    assert a.max() == 258.0 * 258.0 > 65535 and a[1, 1] == 1.0 and (a[1:-1, 1:-1] >= 1).all()
    assert sorted(a[1:-1, 1:-1].ravel().tolist()) == [float(k) for k in range(1, 258 * 258 + 1)]
    _check(rd, "serpentine " + MODE[stack_below], p, ones, None, None, exp, wants=[("racc", "wmax")], dev=stack_below is None)
    assert rd.mfd_distance_rounds() == 1


def test_dev_entry_on_a_side_stream(rd, orc, monkeypatch):
    import torch

    monkeypatch.delenv(ENV, raising=False)
    props, runs = _case(orc, "small", "quinn")
    wts, dest, wnd, exp = runs["c"]
    got = _dev(rd, props, wts, dest, wnd, -1.0, PLANES, stream=torch.cuda.Stream())
    for k in PLANES:
        _same(got[k], exp[k], "side stream " + k)


# ---- 4: the compact D-infinity routes against the generic one ----------------------------------------------------
def _typed_dems(width=120, height=90):
    """(suffix, an unfilled fractal DEM of that element type, its NoData value)"""
    base = fractal_dem(width, height, 303)
    lo = float(base.min())
    yield "f32", base, NDV
    yield "f64", base.astype(np.float64) * 1.000001, -9999.0
    yield "i32", np.floor(base * 50.0).astype(np.int32), -9999
    yield "u32", np.floor((base - lo) * 50.0).astype(np.uint32), 4000000000
    yield "i16", np.floor((base - lo) * 20.0 - 3000.0).clip(-32000, 32000).astype(np.int16), -32768
    yield "u16", np.floor((base - lo) * 20.0).clip(0, 65000).astype(np.uint16), 65535
    yield "i8", np.floor((base - lo) * 0.5 - 100.0).clip(-127, 127).astype(np.int8), -128
    yield "u8", np.floor((base - lo) * 0.5).clip(0, 254).astype(np.uint8), 255


@pytest.mark.parametrize("suffix", ["f32", "f64", "i32", "u32", "i16", "u16", "i8", "u8"])
def test_dinf_from_dem_equals_generic(rd, monkeypatch, suffix):
    """dinf_reverse_accum(dem) == mfd_reverse_accum(FlowProportions(dem, "Dinf")): the same shares and the same graph, only
    the accessor differs (DinfAcc, 5 bytes per cell, against PropsAcc)"""
    import torch

    monkeypatch.delenv(ENV, raising=False)
    dem, nodata = next((d, nd) for s, d, nd in _typed_dems() if s == suffix)
    dem = dem.copy()
    dem[20:26, 30:44] = nodata
    keep = dem.copy()
    props = rd.FlowProportions(dem, "Dinf", nodata=nodata)
    dest = (rd.FlowAccumFromProps(props) >= 30).astype(np.uint8)
    rng = np.random.default_rng(17)
    wts = rng.random(dem.shape)
    wts[rng.random(dem.shape) < 0.05] = -1.0
    decided = 0
    for de in (None, dest):
        a = rd.dinf_reverse_accum(dem, nodata, wts, de, -1.0, -7.0, want=("racc", "wmax"))
        b = rd.mfd_reverse_accum(props, wts, de, -1.0, -7.0, want=("racc", "wmax"))
        for k in PLANES:
            _same(a[k], b[k], f"{suffix} {k} compact vs generic")
        decided += int((b["racc"] != -7.0).sum())
    assert decided > 0 and np.array_equal(dem, keep)
    dep = rd.dinf_upslope_dependence(dem, nodata, dest, -7.0)
    _same(dep, rd.mfd_reverse_accum(props, None, dest, None, -7.0)["racc"], f"{suffix} dinf_upslope_dependence")
    _same(dep, rd.mfd_upslope_dependence(props, dest, -7.0), f"{suffix} mfd_upslope_dependence")
    assert ((dep > 0) & (dep < 1)).sum() > 0
    try:
        t = torch.from_numpy(dem).cuda()
    except TypeError:                                   # a torch without this unsigned type: the host entry stands alone
        t = None
    if t is not None:
        td, tw = torch.from_numpy(dest).cuda(), torch.from_numpy(wts).cuda()
        racc = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
        wmax = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
        rd.dinf_reverse_accum_dev(t, nodata, None, td, None, -7.0, racc=racc)
        torch.cuda.synchronize()
        assert bool((wmax == SENT).all())
        _same(racc.cpu().numpy(), dep, f"{suffix} dinf_reverse_accum_dev dependence")
        rd.dinf_reverse_accum_dev(t, nodata, tw, td, -1.0, -7.0, wmax=wmax)
        torch.cuda.synchronize()
        _same(wmax.cpu().numpy(), b["wmax"], f"{suffix} dinf_reverse_accum_dev wmax")
        assert np.array_equal(t.cpu().view(torch.uint8).numpy().ravel(), dem.view(np.uint8).ravel())
        assert np.array_equal(tw.cpu().numpy(), wts) and np.array_equal(td.cpu().numpy(), dest)


def test_dinf_flats_from_dem_equals_generic(rd, orc, monkeypatch):
    """dinf_reverse_accum_flats(dem) == mfd_reverse_accum(fm_tarboton_flats(dem)) on a filled DEM, whose flats pass flow on"""
    import torch

    monkeypatch.delenv(ENV, raising=False)
    dem = orc.port.fill(fractal_dem(130, 70, 11))
    keep = dem.copy()
    props = rd.fm_tarboton_flats(dem, NDV)
    plain = rd.FlowProportions(dem, "Dinf", nodata=NDV)
    assert not np.array_equal(props, plain)                                  # the flats were patched
    dest = (rd.FlowAccumFromProps(props) >= 30).astype(np.uint8)
    wts = np.random.default_rng(18).random(dem.shape)
    a = rd.dinf_reverse_accum_flats(dem, NDV, wts, dest, None, -7.0, want=("racc", "wmax"))
    b = rd.mfd_reverse_accum(props, wts, dest, None, -7.0, want=("racc", "wmax"))
    for k in PLANES:
        _same(a[k], b[k], f"flats {k} compact vs generic")
    dep = rd.dinf_upslope_dependence_flats(dem, NDV, dest, -7.0)
    _same(dep, rd.mfd_upslope_dependence(props, dest, -7.0), "dinf_upslope_dependence_flats")
    assert not np.array_equal(dep, rd.dinf_upslope_dependence(dem, NDV, dest, -7.0))
    t, td = torch.from_numpy(dem).cuda(), torch.from_numpy(dest).cuda()
    racc = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
    rd.dinf_reverse_accum_flats_dev(t, float(NDV), None, td, None, -7.0, racc=racc)
    torch.cuda.synchronize()
    _same(racc.cpu().numpy(), dep, "dinf_reverse_accum_flats_dev dependence")
    assert np.array_equal(dem, keep)


# ---- 5: refused calls ------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(rd):
    from richdem_amd._lib import check

    L = rd.lib()
    h, w = 6, 7
    props = blank(h, w)
    put(props, 2, 2, {RIGHT: 1.0})
    put(props, 2, 3)
    wts = np.ones((h, w))
    dest = np.zeros((h, w), np.uint8)
    dem = np.ones((h, w), np.float32)
    racc, wmax = np.full((h, w), SENT), np.full((h, w), SENT)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    D = ctypes.c_double

    def generic(p=props, ww=w, hh=h, wt=wts, de=dest, ra=racc, wm=wmax):
        return L.rdgpu_mfd_reverse_accum(P(p), ww, hh, P(wt), D(float("nan")), P(de), P(ra), P(wm), D(-1.0))

    def compact(p=dem, ww=w, hh=h, wt=wts, de=dest, ra=racc, wm=wmax):
        return L.rdgpu_dinf_reverse_accum_f32(P(p), ctypes.c_float(-9999), ww, hh, P(wt), D(float("nan")), P(de), P(ra), P(wm), D(-1.0))

    def flats(p=dem, ww=w, hh=h, wt=wts, de=dest, ra=racc, wm=wmax):
        return L.rdgpu_dinf_reverse_accum_flats_f32(P(p), ctypes.c_float(-9999), ww, hh, P(wt), D(float("nan")), P(de), P(ra), P(wm),
                                                    D(-1.0))

    bad = [dict(p=None), dict(ra=None, wm=None), dict(wt=None), dict(wt=None, wm=None, de=None), dict(ww=0), dict(hh=-1),
           dict(ww=65536, hh=65536)]
    for kw in bad:
        for fn in (generic, compact, flats):
            rc = fn(**kw)
            assert rc == 2, (fn.__name__, kw, rc)                             # RDGPU_ERR_ARG
            with pytest.raises(rd.RdgpuError):
                check(rc, "x")
            assert (racc == SENT).all() and (wmax == SENT).all(), kw
    assert flats(ww=46341, hh=46341) == 2 and (racc == SENT).all()            # 0x7FFF0000 < 46341^2 < 0xFFFF0000
    assert generic() == 0 and racc[2, 2] == 2.0 and racc[0, 0] == -1.0 and wmax[2, 3] == 1.0   # (the same call, valid)
    racc[:], wmax[:] = SENT, SENT
    assert generic(wm=None) == 0 and racc[2, 2] == 2.0 and (wmax == SENT).all()                # racc alone
    racc[:] = SENT
    assert generic(ra=None) == 0 and wmax[2, 2] == 1.0 and wmax[0, 0] == -1.0 and (racc == SENT).all()   # wmax alone
    assert generic(wt=None, wm=None) == 0                                     # the dependence: dest alone

    import torch

    tp = torch.from_numpy(props).cuda()
    ta = torch.full((h, w), SENT, dtype=torch.float64, device="cuda")
    tm = torch.full((h, w), SENT, dtype=torch.float64, device="cuda")
    tw = torch.from_numpy(wts).cuda()
    td = torch.from_numpy(dest).cuda()
    tz = torch.from_numpy(dem).cuda()
    for call in (lambda: rd.mfd_reverse_accum_dev(tp, tw),                                    # no output
                 lambda: rd.mfd_reverse_accum_dev(tp, None, td, racc=ta, wmax=tm),            # wmax without weights
                 lambda: rd.mfd_reverse_accum_dev(tp, racc=ta),                               # neither weights nor dest
                 lambda: rd.mfd_reverse_accum_dev(tp, tw, racc=ta[:, :-1]),
                 lambda: rd.mfd_reverse_accum_dev(tp, tw.float(), racc=ta),
                 lambda: rd.dinf_reverse_accum_dev(tz, -9999, tw),
                 lambda: rd.dinf_reverse_accum_dev(tz, -9999, None, td, wmax=tm),
                 lambda: rd.dinf_reverse_accum_flats_dev(tz, -9999, racc=ta),
                 lambda: rd.mfd_reverse_accum(props),
                 lambda: rd.mfd_reverse_accum(props, wts, want=()),
                 lambda: rd.mfd_reverse_accum(props, None, dest, want=("wmax",)),
                 lambda: rd.mfd_reverse_accum(props[..., :8], wts),
                 lambda: rd.dinf_reverse_accum(dem, -9999),
                 lambda: rd.dinf_reverse_accum(dem.astype(np.int64), -9999, wts)):
        with pytest.raises(rd.RdgpuError):
            call()
    torch.cuda.synchronize()
    assert bool((ta == SENT).all()) and bool((tm == SENT).all())


def test_every_new_symbol_is_exported(rd):
    names = ["rdgpu_mfd_reverse_accum", "rdgpu_mfd_reverse_accum_dev"]
    for s in ("u8", "i8", "i16", "u16", "i32", "u32", "f32", "f64"):
        names += [f"rdgpu_dinf_reverse_accum_{s}", f"rdgpu_dinf_reverse_accum_dev_{s}", f"rdgpu_dinf_reverse_accum_flats_{s}",
                  f"rdgpu_dinf_reverse_accum_flats_dev_{s}"]
    for n in names:
        assert hasattr(rd.lib(), n), n
    for n in ("mfd_reverse_accum", "mfd_upslope_dependence", "dinf_reverse_accum", "dinf_reverse_accum_flats",
              "dinf_upslope_dependence", "dinf_upslope_dependence_flats", "mfd_reverse_accum_dev", "dinf_reverse_accum_dev",
              "dinf_reverse_accum_flats_dev"):
        assert callable(getattr(rd, n)) and n in rd.__all__, n
