"""Distance and drop down to the stop cells over D-infinity / MFD proportions on the engine (csrc/mfd_distance.hip) against
the Python model (tests/mfd_distance_model.py, pinned by tests/test_mfd_distance_model.py): host C-ABI and `_dev` entries,
every requested plane on every cell, bit for bit, inputs unchanged, unrequested planes left alone.

The proportions of the DEM cases come from the CPU oracle, so the model and the engine see identical floats.  The DEMs
are UNFILLED fractals: on a filled DEM the flats have no receivers and are DEAD under a channel mask, and little is left
to compare (one lenient-versus-strict case uses one).  Hand-made proportion rasters reach what a DEM does not: a chain
longer than 65 535 cells, eight receivers, eight donors completed by one thread, the spill of a wavefront's stack and the
hand-over of a thread's buffer (proven from the launch count), cycles, shares into NoData, shares that do not sum to 1.

Proportions layout [h, w, 9]: slot 0 is the marker (-2 NoData), slots 1..8 the shares to the neighbours 1 left, 2 up-left,
3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left."""
import ctypes
import os
import sys

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfd_distance_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
LEFT, UPLEFT, UP, UPRIGHT, RIGHT, DOWNRIGHT, DOWN, DOWNLEFT = range(1, 9)
NDV = np.float32(-9999)
STATS = ("ave", "min", "max")
COMBOS = [(s, t) for s in STATS for t in (True, False)]
SENT = 77.0
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


def _dev(rd, props, chan, elev, stat, strict, cell, nd, want, stream=None):
    """the `_dev` entry on sentinel-filled tensors: the planes asked for, and the proof that the others were left alone"""
    import torch

    h, w = props.shape[:2]
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        tp = torch.from_numpy(props.copy()).cuda()
        tc = None if chan is None else torch.from_numpy(chan.copy()).cuda()
        te = None if elev is None else torch.from_numpy(np.ascontiguousarray(elev, np.float64)).cuda()
        buf = {k: torch.full((h, w), SENT, dtype=torch.float64, device="cuda") for k in ("dist", "drop")}
        rd.mfd_distance_down_dev(tp, tc, te, stat, strict, cell, nd, **{k: buf[k] for k in want})
        after = {k: v + 0.0 for k, v in buf.items()}             # (work that must come after the call)
    torch.cuda.synchronize()
    assert np.array_equal(tp.cpu().numpy(), props) and (tc is None or np.array_equal(tc.cpu().numpy(), chan))
    assert te is None or np.array_equal(te.cpu().numpy(), np.asarray(elev, np.float64))
    for k in ("dist", "drop"):
        if k not in want:
            assert bool((after[k] == SENT).all()), k + " was not requested but written"
    return {k: after[k].cpu().numpy() for k in want}


def _check(rd, name, props, chan, elev, exp_all, combos=COMBOS, cell=(1.0, 1.0), nd=-1.0, dev=True):
    """host and `_dev` against the model for the combinations given; ave asks for both planes, min for dist, max for drop"""
    keep = props.copy(), None if chan is None else chan.copy(), None if elev is None else elev.copy()
    got_all = {}
    for stat, strict in combos:
        exp = exp_all[(stat, strict)]
        want = ("dist", "drop") if stat == "ave" else ("dist",) if stat == "min" else ("drop",)
        if elev is None:
            want = ("dist",)
        got = rd.mfd_distance_down(props, chan, elev, stat, strict, cell, nd, want=want)
        assert tuple(got) == want
        for k in want:
            _same(got[k], exp[k], f"{name} {stat} strict={strict} {k} host")
        if dev:
            d = _dev(rd, props, chan, elev, stat, strict, cell, nd, want)
            for k in want:
                _same(d[k], exp[k], f"{name} {stat} strict={strict} {k} dev")
        got_all[(stat, strict)] = got
    assert np.array_equal(props, keep[0]) and (chan is None or np.array_equal(chan, keep[1]))
    assert elev is None or np.array_equal(elev, keep[2])
    return got_all


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


def _case(orc, which, kind, with_chan):
    key = (which, kind, with_chan)
    if key not in _CACHE:
        dem = _dem(which)
        props = _props(orc, dem, kind)
        chan = (orc.port.flow_accumulation(props) >= 30).astype(np.uint8) if with_chan else None
        exp = model.distance_down_all(props, chan, dem, cell=(1.0, 1.0), out_nodata=-1.0)
        for a in (dem, props) + (() if chan is None else (chan,)):
            a.setflags(write=False)
        _CACHE[key] = (dem, props, chan, exp)
    return _CACHE[key]


DEM_CASES = [(which, kind, ch) for which in ("small", "big", "big_nodata") for kind in ("dinf", "quinn", "holmgren2", "d8")
             for ch in (False, True)]


@pytest.mark.parametrize("which,kind,with_chan", DEM_CASES, ids=[f"{a}-{b}-{'chan' if c else 'nochan'}" for a, b, c in DEM_CASES])
def test_oracle_proportions_vs_model(rd, orc, monkeypatch, which, kind, with_chan):
    monkeypatch.delenv(ENV, raising=False)
    dem, props, chan, exp = _case(orc, which, kind, with_chan)
    data = props[..., 0] != -2.0
    strict = exp[("ave", True)]["state"]
    resolved = float((strict[data] == model.RESOLVED).mean())
    several = float((exp["nrecv"][data] >= 2).mean())
    dead = int((strict == model.DEAD).sum())
    print(f"{which} {kind} chan={with_chan}: resolved {resolved:.3f}, several receivers {several:.3f}, dead {dead}")
    assert resolved >= 0.40
    if kind != "d8":
        assert several >= 0.25
    if with_chan:
        assert dead >= 1
    got = _check(rd, f"{which}-{kind}", props, chan, dem.astype(np.float64), exp)
    assert rd.mfd_distance_rounds() >= 1
    if not with_chan:                                   # no cell is DEAD: strict makes no difference
        assert dead == 0
        for stat in STATS:
            for k in got[(stat, True)]:
                _same(got[(stat, True)][k], got[(stat, False)][k], f"{which}-{kind} {stat} {k} strict vs lenient")


def test_filled_dem_lenient_versus_strict(rd, orc, monkeypatch):
    """A filled DEM under Quinn: the flats are DEAD, strict resolves little; lenient resolves what has one way down."""
    monkeypatch.delenv(ENV, raising=False)
    dem = orc.port.fill(fractal_dem(130, 70, 11))
    props = orc.port.fm_mfd(dem, NDV, "Quinn")
    chan = (orc.port.flow_accumulation(props) >= 30).astype(np.uint8)
    exp = model.distance_down_all(props, chan, dem)
    ns, nl = ((exp[("ave", s)]["state"] == model.RESOLVED).sum() for s in (True, False))
    print("filled, Quinn: resolved strict", int(ns), "lenient", int(nl))
    assert nl > ns
    _check(rd, "filled-quinn", props, chan, dem.astype(np.float64), exp)


# ---- 2: shapes ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 70), (70, 1), (3, 3), (64, 64), (65, 130), (257, 259)]   # (height, width)


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
    chan = (rng.random((h, w)) < 0.05).astype(np.uint8)
    for kind, ch in (("dinf", None), ("quinn", chan)):
        props = _props(orc, dem, kind)
        exp = model.distance_down_all(props, ch, dem, cell=(2.0, 3.0), out_nodata=-5.0)
        _check(rd, f"{h}x{w}-{kind}", props, ch, dem.astype(np.float64), exp, combos=[("ave", True), ("min", False), ("max", True)],
               cell=(2.0, -3.0), nd=-5.0)


# ---- 3: hand-made proportion rasters -----------------------------------------------------------------------------
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
    """every interior cell of a size x size raster on one chain: 66 564 cells for 260, more than 65 535; the stop cell is
    (1, 1) and the chain's far end is 66 563 steps away"""
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
    """a lattice of stop cells; each of the eight neighbours of one flows into it and is the end of a ray of 2 more cells:
    the stop cell's thread completes eight donors in one step, continues with one and hands seven on"""
    p = blank(size, size)
    for cy in range(4, size - 4, pitch):
        for cx in range(4, size - 4, pitch):
            put(p, cy, cx)
            for n in range(1, 9):
                chain_into(p, cy, cx, n, 3)
    return p


def comb(lengths, side=3, pitch=4):
    """Horizontal trunks, `pitch` rows apart, that flow LEFT into their head in column 1 (the stop cell: the only cells of
    the raster without a receiver); below every trunk cell hangs a chain of `side` cells that flows UP into it.  The thread
    of a head walks its trunk to the right (the lowest neighbour number it completed) and hands on one side chain per step."""
    nt, width = len(lengths), max(lengths) + 2
    p = blank(nt * pitch + 2, width)
    for i, ln in enumerate(lengths):
        y = 1 + i * pitch
        for x in range(1, ln + 1):
            put(p, y, x, {LEFT: 1.0} if x > 1 else None)
            if x > 1:
                chain_into(p, y, x, UP, side)
    return p


def ring(stop):
    """(1, 1) -> (1, 2) -> (2, 2) -> (2, 1) -> (1, 1); a chain of 10 cells feeds (1, 2) from the right.  (1, 1) also gives to
    the edge cell (2, 0), which is no stop cell under either mask: DEAD, and the one cell of the first work list when the
    ring has no stop cell -- it takes (1, 1)'s counter from 2 to 1, where it stays."""
    p = blank(4, 15)
    put(p, 1, 1, {RIGHT: 0.5, DOWNLEFT: 0.5})
    put(p, 2, 0)
    put(p, 1, 2, {DOWN: 1.0})
    put(p, 2, 2, {LEFT: 1.0})
    put(p, 2, 1, {UP: 1.0})
    chain_into(p, 1, 2, LEFT, 10)
    chan = np.zeros((4, 15), np.uint8)
    if stop:
        chan[2, 2] = 1
    else:
        chan[0, 0] = 1                      # (a mask without a stop cell on the data)
    return p, chan


def into_nodata():
    p = blank(6, 8)
    put(p, 1, 1, {RIGHT: 0.5, UP: 0.5, DOWN: 0.25})     # up and down are NoData: dropped, one receiver is left
    put(p, 1, 2, {RIGHT: 0.7, DOWNRIGHT: 0.2, UP: 0.4})
    put(p, 1, 3, {RIGHT: 1.0})
    put(p, 1, 4, {UP: 1.0})                             # its only share goes into NoData: a stop cell without a mask
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
    "cycle_with_stop": lambda: ring(True),
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
#  the cycles: the chain is one thread's inline walk and the ring never completes (or is walked inline from its stop cell).
EXPECT_ROUNDS = {
    ("comb_control", "stack"): ("==", 1), ("comb_short", "stack"): ("==", 1),
    ("comb_spill", "stack"): (">=", 2), ("comb_two_waves", "stack"): (">=", 2),
    ("comb_short", "round"): ("==", 2), ("comb_spill", "round"): (">=", 3),
    ("cycle", "stack"): ("<=", 2), ("cycle", "round"): ("<=", 2), ("cycle", "default"): ("<=", 2),
    ("cycle_with_stop", "stack"): ("<=", 2), ("cycle_with_stop", "round"): ("<=", 2),
}


def _hand(name):
    if name not in _CACHE:
        p, chan = HAND[name]()
        h, w = p.shape[:2]
        z = np.random.default_rng(len(name)).random((h, w)) * 100.0
        exp = model.distance_down_all(p, chan, z, cell=(1.0, 1.0), out_nodata=-1.0)
        _CACHE[name] = (p, chan, z, exp)
    return _CACHE[name]


@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_graphs(rd, monkeypatch, name, stack_below):
    """every kernel of the work list, selected by the engine's switch, gives the model's bits"""
    _setenv(monkeypatch, stack_below)
    p, chan, z, exp = _hand(name)
    _check(rd, f"{name} {MODE[stack_below]}", p, chan, z, exp, dev=stack_below is None)
    rd.mfd_distance_down(p, chan, None, "ave", True)
    rounds = rd.mfd_distance_rounds()
    print(f"rounds {name} {MODE[stack_below]}: {rounds}")
    op, bound = EXPECT_ROUNDS.get((name, MODE[stack_below]), (">=", 1))
    assert {"==": rounds == bound, ">=": rounds >= bound, "<=": rounds <= bound}[op], (name, MODE[stack_below], rounds, op, bound)


def test_hand_made_graphs_are_what_the_cases_need():
    """the rasters themselves (no engine): first lists, sizes and the values that the descriptions above promise"""
    for name, ntr in (("comb_spill", 64), ("comb_control", 8), ("comb_two_waves", 128), ("comb_ragged", 64), ("comb_short", 64)):
        p, _, _, exp = _hand(name)
        data = p[..., 0] != -2.0
        first = data & (exp["nrecv"] == 0)
        assert first.sum() == ntr and first[:, 1].sum() == ntr, name          # the trunk heads and nothing else
        assert (exp[("ave", True)]["state"][data] == model.RESOLVED).all()
    assert _hand("comb_spill")[0].shape == (258, 42, 9)
    d = _hand("comb_spill")[3][("ave", True)]["dist"]
    assert d[1, 40] == 39.0 and d[4, 40] == 42.0 and d[4, 2] == 4.0
    p, _, _, exp = _hand("eight_receivers")
    assert exp["nrecv"][10, 10] == 8 and exp[("min", True)]["dist"][10, 10] == 2.0
    assert 12.7 < exp[("max", True)]["dist"][10, 10] < 12.8                  # nine diagonal steps
    assert not np.isclose(float(p[10, 10, 1:].sum()), 1.0)
    p, _, _, exp = _hand("hubs")
    assert exp["nrecv"].max() == 1 and all((p[3:6, 3:6, n] > 0).sum() >= 1 for n in range(1, 9))
    assert exp[("ave", True)]["dist"][4, 1] == 3.0
    s = _hand("cycle")[3][("ave", True)]["state"]
    assert (s[1:3, 1:3] == model.UNDECIDED).all() and (s[1, 3:13] == model.UNDECIDED).all()
    e = _hand("cycle_with_stop")[3][("ave", False)]
    assert (e["state"][1:3, 1:3] == model.RESOLVED).all() and e["dist"][1, 12] == 11.0 and e["dist"][2, 1] == 3.0
    e = _hand("into_nodata")[3]
    assert e["nrecv"][1, 1] == 1 and e["nrecv"][1, 4] == 0 and e["nrecv"][2, 7] == 0 and e["nrecv"][1, 2] == 2
    e = _hand("fractions")[3]
    assert e["nrecv"][5, 4] == 3 and (e[("ave", True)]["state"][1:38, 2:7] == model.RESOLVED).all()


@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
def test_serpentine_longer_than_65535(rd, monkeypatch, stack_below):
    """one chain through 66 564 cells: one thread's inline walk; distances to 66 563 are exact integers"""
    _setenv(monkeypatch, stack_below)
    if "serpentine" not in _CACHE:
        p = serpentine()
        z = np.random.default_rng(5).random(p.shape[:2]) * 100.0
        _CACHE["serpentine"] = (p, z, model.distance_down_all(p, None, z))
    p, z, exp = _CACHE["serpentine"]
    d = exp[("ave", True)]["dist"]
    assert d.max() == 258.0 * 258.0 - 1.0 > 65535 and d[1, 1] == 0.0 and (d[1:-1, 1:-1] >= 0).all()
    _check(rd, "serpentine " + MODE[stack_below], p, None, z, exp, combos=[("ave", True)], dev=stack_below is None)
    assert rd.mfd_distance_rounds() == 1


def test_dev_entry_on_a_side_stream(rd, orc, monkeypatch):
    import torch

    monkeypatch.delenv(ENV, raising=False)
    dem, props, chan, exp = _case(orc, "small", "quinn", True)
    got = _dev(rd, props, chan, dem.astype(np.float64), "ave", True, (1.0, 1.0), -1.0, ("dist", "drop"), stream=torch.cuda.Stream())
    for k in ("dist", "drop"):
        _same(got[k], exp[("ave", True)][k], "side stream " + k)


# ---- 4: the compact D-infinity route against the generic one -----------------------------------------------------
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
    """dinf_distance_down(dem) == mfd_distance_down(FlowProportions(dem, "Dinf"), elev=dem): the same shares and the same
    graph, only the accessor differs (DinfAcc, 5 bytes per cell, against PropsAcc)"""
    import torch

    monkeypatch.delenv(ENV, raising=False)
    dem, nodata = next((d, nd) for s, d, nd in _typed_dems() if s == suffix)
    dem = dem.copy()
    dem[20:26, 30:44] = nodata
    keep = dem.copy()
    props = rd.FlowProportions(dem, "Dinf", nodata=nodata)
    chan = (rd.FlowAccumFromProps(props) >= 30).astype(np.uint8)
    resolved = 0
    for ch in (None, chan):
        for stat, strict in (("ave", True), ("min", False), ("max", True)):
            a = rd.dinf_distance_down(dem, nodata, ch, stat, strict, (2.0, 3.0), -7.0, want=("dist", "drop"))
            b = rd.mfd_distance_down(props, ch, dem, stat, strict, (2.0, 3.0), -7.0, want=("dist", "drop"))
            for k in ("dist", "drop"):
                _same(a[k], b[k], f"{suffix} {stat} {k} compact vs generic")
            resolved += int((b["dist"] != -7.0).sum())
    assert resolved > 0 and np.array_equal(dem, keep)
    hand = rd.dinf_hand(dem, nodata, chan, "ave", True, -7.0)
    _same(hand, rd.mfd_distance_down(props, chan, dem, "ave", True, (1.0, 1.0), -7.0, want=("drop",))["drop"], f"{suffix} dinf_hand")
    try:
        t = torch.from_numpy(dem).cuda()
    except TypeError:                                   # a torch without this unsigned type: the host entry stands alone
        t = None
    if t is not None:
        tc = torch.from_numpy(chan).cuda()
        dist = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
        drop = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
        rd.dinf_distance_down_dev(t, nodata, tc, "ave", True, (1.0, 1.0), -7.0, drop=drop)
        torch.cuda.synchronize()
        assert bool((dist == SENT).all())
        _same(drop.cpu().numpy(), hand, f"{suffix} dinf_distance_down_dev drop")
        out = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
        rd.dinf_hand_dev(t, nodata, tc, out, "ave", True, -7.0)
        rd.dinf_distance_down_dev(t, nodata, None, "max", False, (2.0, 3.0), -7.0, dist=dist)
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), hand, f"{suffix} dinf_hand_dev")
        _same(dist.cpu().numpy(), rd.mfd_distance_down(props, None, None, "max", False, (2.0, 3.0), -7.0)["dist"], f"{suffix} dev dist")
        assert np.array_equal(t.cpu().view(torch.uint8).numpy().ravel(), dem.view(np.uint8).ravel())


@pytest.mark.parametrize("suffix", ["f32", "f64", "i32", "u32", "i16", "u16", "i8", "u8"])
def test_drop_with_elevations_of_every_type(rd, orc, monkeypatch, suffix):
    """the drop over one set of proportions with the elevations of each element type == the model fed elev.astype(float64)"""
    monkeypatch.delenv(ENV, raising=False)
    _, props, chan, _ = _case(orc, "small", "dinf", True)
    h, w = props.shape[:2]
    elev = next(d for s, d, _ in _typed_dems(w, h) if s == suffix)
    assert elev.shape == (h, w) and elev.dtype.itemsize == {"8": 1, "6": 2, "2": 4, "4": 8}[suffix[-1]]
    exp = model.distance_down(props, chan, elev.astype(np.float64), "ave", False)
    got = rd.mfd_distance_down(props, chan, elev, "ave", False, want=("drop",))
    _same(got["drop"], exp["drop"], f"drop with {suffix} elevations")
    assert (exp["drop"] != -1.0).sum() > 1000


# ---- 5: refused calls ------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing(rd):
    from richdem_amd._lib import check

    L = rd.lib()
    h, w = 6, 7
    props = blank(h, w)
    put(props, 2, 2, {RIGHT: 1.0})
    put(props, 2, 3)
    elev = np.zeros((h, w))
    dem = np.ones((h, w), np.float32)
    dist, drop = np.full((h, w), SENT), np.full((h, w), SENT)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    D = ctypes.c_double

    def generic(p=props, ww=w, hh=h, el=elev, stat=0, cx=1.0, cy=1.0, di=dist, dr=drop):
        return L.rdgpu_mfd_distance_down(P(p), ww, hh, None, P(el), stat, 1, D(cx), D(cy), P(di), P(dr), D(-1.0))

    def compact(z=dem, ww=w, hh=h, stat=0, cx=1.0, cy=1.0, di=dist, dr=drop):
        return L.rdgpu_dinf_distance_down_f32(P(z), ctypes.c_float(-9999), ww, hh, None, stat, 1, D(cx), D(cy), P(di), P(dr), D(-1.0))

    bad = [dict(p=None), dict(di=None, dr=None), dict(el=None), dict(stat=3), dict(stat=-1), dict(cx=0.0), dict(cy=0.0),
           dict(cx=float("nan")), dict(cy=float("inf")), dict(ww=0), dict(hh=-1), dict(ww=65536, hh=65536)]
    for kw in bad:
        for fn in (generic, compact):
            if fn is compact:
                if "el" in kw:
                    continue
                kw = {("z" if k == "p" else k): v for k, v in kw.items()}
            rc = fn(**kw)
            assert rc == 2, (fn.__name__, kw, rc)                             # RDGPU_ERR_ARG
            with pytest.raises(rd.RdgpuError):
                check(rc, "x")
            assert (dist == SENT).all() and (drop == SENT).all(), kw
    assert generic() == 0 and dist[2, 2] == 1.0 and dist[0, 0] == -1.0        # (the same call, valid)
    assert L.rdgpu_mfd_distance_rounds(None) == 2

    import torch

    tp = torch.from_numpy(props).cuda()
    td = torch.full((h, w), SENT, dtype=torch.float64, device="cuda")
    tr = torch.full((h, w), SENT, dtype=torch.float64, device="cuda")
    tz = torch.from_numpy(dem).cuda()
    for call in (lambda: rd.mfd_distance_down_dev(tp),
                 lambda: rd.mfd_distance_down_dev(tp, dist=td, drop=tr),                      # drop without elev
                 lambda: rd.mfd_distance_down_dev(tp, stat=5, dist=td),
                 lambda: rd.mfd_distance_down_dev(tp, stat="median", dist=td),
                 lambda: rd.mfd_distance_down_dev(tp, cell=(0.0, 1.0), dist=td),
                 lambda: rd.mfd_distance_down_dev(tp, cell=(1.0, float("nan")), dist=td),
                 lambda: rd.mfd_distance_down_dev(tp, dist=td[:, :-1]),
                 lambda: rd.dinf_distance_down_dev(tz, -9999),
                 lambda: rd.dinf_distance_down_dev(tz, -9999, stat=3, dist=td, drop=tr),
                 lambda: rd.dinf_distance_down_dev(tz, -9999, cell=(float("inf"), 1.0), drop=tr),
                 lambda: rd.mfd_distance_down(props, want=("drop",)),
                 lambda: rd.mfd_distance_down(props, want=()),
                 lambda: rd.mfd_distance_down(props, stat="mean"),
                 lambda: rd.mfd_distance_down(props, cell=(0, 1)),
                 lambda: rd.mfd_distance_down(props[..., :8]),
                 lambda: rd.dinf_distance_down(dem, -9999, stat=7),
                 lambda: rd.dinf_distance_down(dem.astype(np.int64), -9999)):
        with pytest.raises(rd.RdgpuError):
            call()
    torch.cuda.synchronize()
    assert bool((td == SENT).all()) and bool((tr == SENT).all())


def test_every_new_symbol_is_exported(rd):
    names = ["rdgpu_mfd_distance_down", "rdgpu_mfd_distance_down_dev", "rdgpu_mfd_distance_rounds",
             "rdgpu_dinf_distance_down_u8", "rdgpu_dinf_distance_down_i8", "rdgpu_dinf_distance_down_i16",
             "rdgpu_dinf_distance_down_u16", "rdgpu_dinf_distance_down_i32", "rdgpu_dinf_distance_down_u32",
             "rdgpu_dinf_distance_down_f32", "rdgpu_dinf_distance_down_f64",
             "rdgpu_dinf_distance_down_dev_u8", "rdgpu_dinf_distance_down_dev_i8", "rdgpu_dinf_distance_down_dev_i16",
             "rdgpu_dinf_distance_down_dev_u16", "rdgpu_dinf_distance_down_dev_i32", "rdgpu_dinf_distance_down_dev_u32",
             "rdgpu_dinf_distance_down_dev_f32", "rdgpu_dinf_distance_down_dev_f64"]
    for n in names:
        assert hasattr(rd.lib(), n), n
    for n in ("mfd_distance_down", "dinf_distance_down", "dinf_hand", "mfd_distance_down_dev", "dinf_distance_down_dev",
              "dinf_hand_dev", "mfd_distance_rounds"):
        assert callable(getattr(rd, n)) and n in rd.__all__, n
