"""Distance and rise up to the sources over D-infinity / MFD proportions on the engine (csrc/mfd_distance_up.hip) against
the Python model (tests/mfd_distance_up_model.py, pinned by tests/test_mfd_distance_up_model.py): host C-ABI and `_dev`
entries, every requested plane on every cell, bit for bit, inputs unchanged, unrequested planes left alone.

The proportions of the DEM cases come from the CPU oracle, so the model and the engine see identical floats.  Hand-made
proportion rasters reach what a DEM does not: a chain longer than 65 535 cells, eight donors of one cell, eight receivers
completed by one thread, the spill of a wavefront's stack and the hand-over of a thread's buffer (proven from the launch
count), a cycle and its tail, shares into NoData and out of the raster, shares that do not sum to 1.

Proportions layout [h, w, 9]: slot 0 is the marker (-2 NoData), slots 1..8 the shares to the neighbours 1 left, 2 up-left,
3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left."""
import ctypes
import os
import sys

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfd_distance_up_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
LEFT, UPLEFT, UP, UPRIGHT, RIGHT, DOWNRIGHT, DOWN, DOWNLEFT = range(1, 9)
NDV = np.float32(-9999)
STATS = ("ave", "min", "max")
SENT = 77.0
ENV = "RDGPU_MFD_DISTANCE_STACK_BELOW"
STACK_BELOW = [None, "0", "4294967295"]      # the default; always k_wl_buffer; always k_wl_stack
MODE = {None: "default", "0": "round", "4294967295": "stack"}
_CACHE = {}


def opp(n):
    return n + 4 if n <= 4 else n - 4


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


def _dev(rd, props, elev, stat, min_share, cell, nd, want, stream=None):
    """the `_dev` entry on sentinel-filled tensors: the planes asked for, and the proof that the others were left alone"""
    import torch

    h, w = props.shape[:2]
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        tp = torch.from_numpy(props.copy()).cuda()
        te = None if elev is None else torch.from_numpy(np.ascontiguousarray(elev, np.float64)).cuda()
        buf = {k: torch.full((h, w), SENT, dtype=torch.float64, device="cuda") for k in ("dist", "rise")}
        rd.mfd_distance_up_dev(tp, te, stat, min_share, cell, nd, **{k: buf[k] for k in want})
        after = {k: v + 0.0 for k, v in buf.items()}             # (work that must come after the call)
    torch.cuda.synchronize()
    assert np.array_equal(tp.cpu().numpy(), props)
    assert te is None or np.array_equal(te.cpu().numpy(), np.asarray(elev, np.float64))
    for k in ("dist", "rise"):
        if k not in want:
            assert bool((after[k] == SENT).all()), k + " was not requested but written"
    return {k: after[k].cpu().numpy() for k in want}


def _check(rd, name, props, elev, exp_all, min_share=0.0, stats=STATS, cell=(1.0, 1.0), nd=-1.0, dev=True):
    """host and `_dev` against the model for the statistics given; ave asks for both planes, min for dist, max for rise"""
    keep = props.copy(), None if elev is None else elev.copy()
    for stat in stats:
        exp = exp_all[stat]
        want = ("dist", "rise") if stat == "ave" else ("dist",) if stat == "min" else ("rise",)
        if elev is None:
            want = ("dist",)
        got = rd.mfd_distance_up(props, elev, stat, min_share, cell, nd, want=want)
        assert tuple(got) == want
        for k in want:
            _same(got[k], exp[k], f"{name} {stat} {k} host")
        if dev:
            d = _dev(rd, props, elev, stat, min_share, cell, nd, want)
            for k in want:
                _same(d[k], exp[k], f"{name} {stat} {k} dev")
    assert np.array_equal(props, keep[0]) and (elev is None or np.array_equal(elev, keep[1]))


# ---- 1: proportions of the CPU oracle on fractal DEMs ------------------------------------------------------------
def _dem(which):
    if which.startswith("small"):
        dem = fractal_dem(130, 70, 11)
        if which == "small_nodata":
            dem[30:36, 50:70] = NDV
            dem[0:4, 100:110] = NDV
            dem[20, 21] = NDV
        return dem
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


def _case(orc, which, kind, min_share):
    if (which, kind) not in _CACHE:
        dem = _dem(which)
        props = _props(orc, dem, kind)
        for a in (dem, props):
            a.setflags(write=False)
        _CACHE[(which, kind)] = (dem, props)
    dem, props = _CACHE[(which, kind)]
    key = (which, kind, min_share)
    if key not in _CACHE:
        _CACHE[key] = model.distance_up_all(props, dem, min_share, cell=(1.0, 1.0), out_nodata=-1.0)
    return dem, props, _CACHE[key]


WHICH = ("small", "small_nodata", "big", "big_nodata")
KINDS = ("dinf", "quinn", "holmgren2", "d8")
MIN_SHARES = (0.0, 0.25, 0.5)
DEM_CASES = [(which, kind, ms) for which in WHICH for kind in KINDS for ms in MIN_SHARES]


@pytest.mark.parametrize("which,kind,min_share", DEM_CASES, ids=[f"{a}-{b}-{c}" for a, b, c in DEM_CASES])
def test_oracle_proportions_vs_model(rd, orc, monkeypatch, which, kind, min_share):
    monkeypatch.delenv(ENV, raising=False)
    dem, props, exp = _case(orc, which, kind, min_share)
    data = props[..., 0] != -2.0
    several = float((exp["ndonors"][data] >= 2).mean())
    sources = float((exp["ndonors"][data] == 0).mean())
    undecided = int((data & ~exp["decided"]).sum())
    print(f"{which} {kind} min_share={min_share}: two or more donors {several:.3f}, sources {sources:.3f}, undecided {undecided}")
    assert undecided == 0
    if min_share == 0.0 and kind != "d8":
        assert several >= 0.40
    if min_share == 0.25 and kind != "d8":
        at0 = _case(orc, which, kind, 0.0)[2]
        assert (exp["ndonors"][data] == 0).sum() > (at0["ndonors"][data] == 0).sum()
    _check(rd, f"{which}-{kind}-{min_share}", props, dem.astype(np.float64), exp, min_share)
    assert rd.mfd_distance_rounds() >= 1


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
    for kind, ms in (("dinf", 0.0), ("quinn", 0.25)):
        props = _props(orc, dem, kind)
        exp = model.distance_up_all(props, dem, ms, cell=(2.0, -3.0), out_nodata=-5.0)
        _check(rd, f"{h}x{w}-{kind}", props, dem.astype(np.float64), exp, ms, cell=(2.0, -3.0), nd=-5.0)


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


def chain(p, y, x, n, length):
    """`length` cells from (y, x) on in direction n, each giving share 1 to the next; the last one gives nothing"""
    for k in range(length):
        put(p, y + k * DY[n], x + k * DX[n], {n: 1.0} if k < length - 1 else None)


def chain_into(p, y, x, n, length):
    """`length` cells that each give share 1 to the next in direction n and end by flowing INTO (y, x), which is not touched"""
    for k in range(1, length + 1):
        put(p, y - k * DY[n], x - k * DX[n], {n: 1.0})


def serpentine(size=260):
    """every interior cell of a size x size raster on one chain: 66 564 cells for 260, more than 65 535; the one source is
    the chain's far end and (1, 1) is 66 563 steps below it"""
    p = blank(size, size)
    for y in range(1, size - 1):
        east = (y % 2) == 1                     # odd rows were laid left to right, so their cells flow back LEFT
        for x in range(1, size - 1):
            first = x == (1 if east else size - 2)
            put(p, y, x, ({UP: 1.0} if y > 1 else None) if first else {LEFT if east else RIGHT: 1.0})
    return p


def eight_donors():
    """all eight neighbours of (10, 10) give to it (fractions that do not sum to 1); the neighbour at position m is the end of
    a chain of m more cells that flows towards the centre; the centre gives nothing"""
    p = blank(23, 23)
    put(p, 10, 10)
    for m in range(1, 9):
        put(p, 10 + DY[m], 10 + DX[m], {opp(m): np.float32(0.03 * m + 0.01)})
        chain_into(p, 10 + DY[m], 10 + DX[m], opp(m), m)
    return p


def hubs(size=150):
    """A 3-pitch lattice of hubs; each hub has no shares, its eight neighbours are sources that feed it: eight threads
    decrement one counter at the same moment, exactly one of them sees it reach zero and reads all eight donors."""
    p = blank(size, size)
    for y in range(2, size - 2, 3):
        for x in range(2, size - 2, 3):
            put(p, y, x)
            for n in range(1, 9):
                put(p, y + DY[n], x + DX[n], {opp(n): np.float32(0.1 * n)})
    return p


def stars(k=8, pitch=7):
    """A lattice of sources that feed all eight neighbours, each the head of a straight outward ray of 2 more cells: one
    thread completes eight receivers in one step, continues with one and hands seven on."""
    p = blank(k * pitch + 2, k * pitch + 2)
    for j in range(k):
        for i in range(k):
            y, x = 4 + j * pitch, 4 + i * pitch
            put(p, y, x, {n: np.float32(0.05 * n) for n in range(1, 9)})
            for n in range(1, 9):
                chain(p, y + DY[n], x + DX[n], n, 3)
    return p


def comb(lengths, side=3, pitch=4):
    """Horizontal trunks, `pitch` rows apart; trunk cell (y, x) feeds the next trunk cell (right) and the head of a side
    chain of `side` cells running down.  The engine continues inline with the lowest n: a lane walks its trunk and hands
    on one side head per step (the trunk's last cell has the side chain as its only receiver)."""
    nt, width = len(lengths), max(lengths) + 2
    p = blank(nt * pitch + 2, width)
    for i, ln in enumerate(lengths):
        y = 1 + i * pitch
        for x in range(1, ln + 1):
            put(p, y, x, {RIGHT: 1.0, DOWN: 1.0} if x < ln else {DOWN: 1.0})
            chain(p, y + 1, x, DOWN, side)
    return p


def edges_and_nodata():
    p = blank(6, 8)
    put(p, 1, 1, {LEFT: 0.5, RIGHT: 0.5, UP: 0.25})     # into the edge cell (1, 0), into (1, 2) and into the edge cell (0, 1)
    put(p, 1, 0, {RIGHT: 1.0, LEFT: 1.0})               # an edge cell with donors; its shares (one of them out of the raster)
    put(p, 0, 1, {DOWN: 1.0, UP: 0.5})                  # ... give nobody a donor
    put(p, 1, 2, {RIGHT: 0.7, DOWNRIGHT: 0.2, UP: 0.4})  # up is NoData: dropped
    put(p, 1, 3, {RIGHT: 1.0, DOWN: 0.3})
    put(p, 1, 4, {UP: 1.0})                             # its only share goes into NoData
    put(p, 2, 3, {RIGHT: 0.125, DOWN: 0.5})             # two donors: (1, 2) and (1, 3)
    put(p, 2, 4, {RIGHT: 1.0})
    put(p, 2, 5, {RIGHT: 1.0})
    put(p, 2, 6, {RIGHT: 1.0})
    put(p, 2, 7, {LEFT: 1.0})                           # an edge cell with a donor and a positive share back: no link
    put(p, 3, 3)
    return p


def ring():
    """(1, 1) -> (1, 2) -> (2, 2) -> (2, 1) -> (1, 1), the last link with share 0.1; (2, 2) also feeds a tail of ten cells to
    its right.  Apart from them a chain of four in row 3, which is decided whatever the ring does."""
    p = blank(5, 15)
    put(p, 1, 1, {RIGHT: 1.0})
    put(p, 1, 2, {DOWN: 1.0})
    put(p, 2, 2, {LEFT: 0.5, RIGHT: 0.5})
    put(p, 2, 1, {UP: 0.1})
    for x in range(3, 13):
        put(p, 2, x, {RIGHT: 1.0} if x < 12 else None)
    chain(p, 3, 5, RIGHT, 4)
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


HAND = {                                                                # name -> (raster, min_share)
    "comb_spill": lambda: (comb([40] * 64), 0.0),                       # 258 x 42: the later steps of the wavefront spill
    "comb_control": lambda: (comb([40] * 8), 0.0),                      # 56 idle lanes pop what 8 push
    "comb_two_waves": lambda: (comb([40] * 128), 0.0),
    "comb_ragged": lambda: (comb([20 + (7 * i) % 61 for i in range(64)]), 0.0),
    "comb_short": lambda: (comb([12] * 64), 0.0),                       # 11 hand-ons per thread fit in the buffer
    "eight_donors": lambda: (eight_donors(), 0.0),
    "hubs": lambda: (hubs(), 0.0),
    "stars": lambda: (stars(), 0.0),
    "edges_and_nodata": lambda: (edges_and_nodata(), 0.0),
    "cycle": lambda: (ring(), 0.0),
    "cycle_broken": lambda: (ring(), 0.25),                             # the 0.1 link is no link: (1, 1) is a source
    "fractions": lambda: (fractions(), 0.0),
}

# Launch counts that follow from WL_CAP = 1536 (entries of a wavefront's stack) and WL_BUF = 20 (entries of a thread's buffer),
# by (raster, forced kernel).  The first list is the 64 (8, 128) trunk heads in row-major order: one lane each.
#  stack, 64 trunks of 40: every step of the wavefront pushes 64 side heads and no lane is idle before the trunks end, so
#    the stack (1536) is full after 24 of the 39 steps and the later steps spill: a second launch.  8 trunks: 56 idle lanes
#    pop what 8 push; 64 trunks of 12: 64 x 11 = 704 entries: one launch.
#  round, trunks of 12: a thread buffers 11 side heads (nb + 8 <= 20 throughout), they are launch two and each is walked
#    inline.  Trunks of 40: after 13 buffered heads (nb + 8 > 20) the thread hands its trunk cell over: the trunk alone
#    takes three launches.
#  the cycle: the first list is row 3's source alone (one inline walk); the ring never completes.  Broken: two sources.
EXPECT_ROUNDS = {
    ("comb_control", "stack"): ("==", 1), ("comb_short", "stack"): ("==", 1),
    ("comb_spill", "stack"): (">=", 2), ("comb_two_waves", "stack"): (">=", 2),
    ("comb_short", "round"): ("==", 2), ("comb_spill", "round"): (">=", 3),
    ("cycle", "stack"): ("==", 1), ("cycle", "round"): ("==", 1), ("cycle", "default"): ("==", 1),
    ("cycle_broken", "stack"): ("==", 1),
}


def _hand(name):
    if name not in _CACHE:
        p, ms = HAND[name]()
        h, w = p.shape[:2]
        z = np.random.default_rng(len(name)).random((h, w)) * 100.0
        exp = model.distance_up_all(p, z, ms, cell=(1.0, 1.0), out_nodata=-1.0)
        _CACHE[name] = (p, ms, z, exp)
    return _CACHE[name]


@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_graphs(rd, monkeypatch, name, stack_below):
    """every kernel of the work list, selected by the engine's switch, gives the model's bits"""
    _setenv(monkeypatch, stack_below)
    p, ms, z, exp = _hand(name)
    _check(rd, f"{name} {MODE[stack_below]}", p, z, exp, ms, dev=stack_below is None)
    rd.mfd_distance_up(p, None, "ave", ms)
    rounds = rd.mfd_distance_rounds()
    print(f"rounds {name} {MODE[stack_below]}: {rounds}")
    op, bound = EXPECT_ROUNDS.get((name, MODE[stack_below]), (">=", 1))
    assert {"==": rounds == bound, ">=": rounds >= bound, "<=": rounds <= bound}[op], (name, MODE[stack_below], rounds, op, bound)


def test_hand_made_graphs_are_what_the_cases_need():
    """the rasters themselves (no engine): first lists, sizes and the values that the descriptions above promise"""
    for name, ntr in (("comb_spill", 64), ("comb_control", 8), ("comb_two_waves", 128), ("comb_ragged", 64), ("comb_short", 64)):
        p, _, _, exp = _hand(name)
        data = p[..., 0] != -2.0
        first = data & (exp["ndonors"] == 0)
        assert first.sum() == ntr and first[:, 1].sum() == ntr, name          # the trunk heads and nothing else
        assert exp["decided"][data].all()
    assert _hand("comb_spill")[0].shape == (258, 42, 9)
    d = _hand("comb_spill")[3]["ave"]["dist"]
    assert d[1, 40] == 39.0 and d[4, 40] == 42.0 and d[4, 2] == 4.0
    p, _, _, exp = _hand("eight_donors")
    assert exp["ndonors"][10, 10] == 8 and exp["min"]["dist"][10, 10] == 2.0
    assert 12.7 < exp["max"]["dist"][10, 10] < 12.8                          # nine diagonal steps
    assert exp["min"]["dist"][10, 10] < exp["ave"]["dist"][10, 10] < exp["max"]["dist"][10, 10]
    assert not np.isclose(sum(float(p[10 + DY[m], 10 + DX[m], opp(m)]) for m in range(1, 9)), 1.0)
    p, _, _, exp = _hand("hubs")
    assert exp["ndonors"].max() == 8 and (exp["ndonors"] == 8).sum() == 49 * 49
    assert exp["min"]["dist"][2, 2] == 1.0 and exp["max"]["dist"][2, 2] == np.sqrt(2.0)
    p, _, _, exp = _hand("stars")
    assert (exp["ndonors"][p[..., 0] != -2.0] == 0).sum() == 64 and exp["ave"]["dist"][4, 1] == 3.0
    p, ms, _, exp = _hand("cycle")
    dec = exp["decided"]
    assert not dec[1:3, 1:3].any() and not dec[2, 3:13].any() and dec[3, 5:9].all()
    assert (exp["ave"]["dist"][2, 1:13] == -1.0).all() and exp["ave"]["dist"][3, 8] == 3.0
    p, ms, _, exp = _hand("cycle_broken")
    assert ms == 0.25 and exp["decided"][p[..., 0] != -2.0].all() and exp["max"]["dist"][2, 12] == 12.0 and exp["max"]["dist"][2, 1] == 3.0
    e = _hand("edges_and_nodata")[3]
    n = e["ndonors"]
    assert n[1, 0] == 1 and n[0, 1] == 1 and n[1, 1] == 0 and n[1, 4] == 1 and n[2, 3] == 2 and n[2, 7] == 1 and n[2, 6] == 1
    assert e["decided"].sum() == 12 and e["ave"]["dist"][2, 7] == e["ave"]["dist"][2, 3] + 4.0
    p, _, _, e = _hand("fractions")
    assert e["ndonors"][5, 4] == 3 and np.array_equal(e["decided"], p[..., 0] != -2.0)


@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
def test_serpentine_longer_than_65535(rd, monkeypatch, stack_below):
    """one chain through 66 564 cells: one thread's inline walk from the one source; distances to 66 563 are exact integers"""
    _setenv(monkeypatch, stack_below)
    if "serpentine" not in _CACHE:
        p = serpentine()
        z = np.random.default_rng(5).random(p.shape[:2]) * 100.0
        _CACHE["serpentine"] = (p, z, model.distance_up_all(p, z))
    p, z, exp = _CACHE["serpentine"]
    d = exp["ave"]["dist"]
    assert (p[..., 0] != -2.0).sum() == 66564 and (exp["ndonors"][p[..., 0] != -2.0] == 0).sum() == 1
    assert d.max() == 258.0 * 258.0 - 1.0 > 65535 and d[1, 1] == d.max() and (d[1:-1, 1:-1] >= 0).all()
    _check(rd, "serpentine " + MODE[stack_below], p, z, exp, stats=("ave",), dev=stack_below is None)
    assert rd.mfd_distance_rounds() == 1
    got = rd.mfd_distance_up(p, None, "max")["dist"]
    assert got.max() == 258.0 * 258.0 - 1.0


def test_dev_entry_on_a_side_stream(rd, orc, monkeypatch):
    import torch

    monkeypatch.delenv(ENV, raising=False)
    dem, props, exp = _case(orc, "small", "quinn", 0.25)
    got = _dev(rd, props, dem.astype(np.float64), "ave", 0.25, (1.0, 1.0), -1.0, ("dist", "rise"), stream=torch.cuda.Stream())
    for k in ("dist", "rise"):
        _same(got[k], exp["ave"][k], "side stream " + k)


def test_rounds_report_the_last_call_of_either_direction(rd, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    p = _hand("comb_spill")[0]
    rd.mfd_distance_up(p)
    up = rd.mfd_distance_rounds()
    q = blank(3, 4)
    put(q, 1, 1, {RIGHT: 1.0})
    put(q, 1, 2)
    rd.mfd_distance_down(q)
    assert up >= 2 and rd.mfd_distance_rounds() == 1
    rd.mfd_distance_up(p)
    assert rd.mfd_distance_rounds() == up


# ---- 4: the compact D-infinity route against the generic one -----------------------------------------------------
def _typed_dems(width=120, height=90):
    """(suffix, a fractal DEM of that element type, its NoData value); the integer ones have flats"""
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
    """dinf_distance_up(dem) == mfd_distance_up(FlowProportions(dem, "Dinf"), elev=dem): the same shares and the same graph,
    only the accessor differs (DinfAcc, 5 bytes per cell, against PropsAcc); the `_flats` twin over fm_tarboton_flats"""
    import torch

    monkeypatch.delenv(ENV, raising=False)
    dem, nodata = next((d, nd) for s, d, nd in _typed_dems() if s == suffix)
    dem = dem.copy()
    dem[20:26, 30:44] = nodata
    keep = dem.copy()
    decided = 0
    for flats in (False, True):
        props = rd.fm_tarboton_flats(dem, nodata) if flats else rd.FlowProportions(dem, "Dinf", nodata=nodata)
        entry = rd.dinf_distance_up_flats if flats else rd.dinf_distance_up
        for stat, ms in (("ave", 0.0), ("min", 0.25), ("max", 0.5)):
            a = entry(dem, nodata, stat, ms, (2.0, 3.0), -7.0, want=("dist", "rise"))
            b = rd.mfd_distance_up(props, dem, stat, ms, (2.0, 3.0), -7.0, want=("dist", "rise"))
            for k in ("dist", "rise"):
                _same(a[k], b[k], f"{suffix} flats={flats} {stat} {k} compact vs generic")
            decided += int((b["dist"] > 0.0).sum())
    assert decided > 0 and np.array_equal(dem, keep)
    try:
        t = torch.from_numpy(dem).cuda()
    except TypeError:                                   # a torch without this unsigned type: the host entries stand alone
        return
    for flats in (False, True):
        host = (rd.dinf_distance_up_flats if flats else rd.dinf_distance_up)(dem, nodata, "ave", 0.25, (1.0, 1.0), -7.0,
                                                                             want=("dist", "rise"))
        dist = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
        rise = torch.full(dem.shape, SENT, dtype=torch.float64, device="cuda")
        fn = rd.dinf_distance_up_flats_dev if flats else rd.dinf_distance_up_dev
        fn(t, nodata, "ave", 0.25, (1.0, 1.0), -7.0, rise=rise)
        torch.cuda.synchronize()
        assert bool((dist == SENT).all())
        _same(rise.cpu().numpy(), host["rise"], f"{suffix} flats={flats} dev rise")
        fn(t, nodata, "ave", 0.25, (1.0, 1.0), -7.0, dist=dist)
        torch.cuda.synchronize()
        _same(dist.cpu().numpy(), host["dist"], f"{suffix} flats={flats} dev dist")
    assert np.array_equal(t.cpu().view(torch.uint8).numpy().ravel(), dem.view(np.uint8).ravel())


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
    dist, rise = np.full((h, w), SENT), np.full((h, w), SENT)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    D, F = ctypes.c_double, ctypes.c_float

    def generic(p=props, ww=w, hh=h, el=elev, stat=0, ms=0.0, cx=1.0, cy=1.0, di=dist, ri=rise):
        return L.rdgpu_mfd_distance_up(P(p), ww, hh, P(el), stat, F(ms), D(cx), D(cy), P(di), P(ri), D(-1.0))

    def compact(z=dem, ww=w, hh=h, stat=0, ms=0.0, cx=1.0, cy=1.0, di=dist, ri=rise):
        return L.rdgpu_dinf_distance_up_f32(P(z), F(-9999), ww, hh, stat, F(ms), D(cx), D(cy), P(di), P(ri), D(-1.0))

    def compact_flats(z=dem, ww=w, hh=h, stat=0, ms=0.0, cx=1.0, cy=1.0, di=dist, ri=rise):
        return L.rdgpu_dinf_distance_up_flats_f32(P(z), F(-9999), ww, hh, stat, F(ms), D(cx), D(cy), P(di), P(ri), D(-1.0))

    bad = [dict(p=None), dict(di=None, ri=None), dict(el=None), dict(stat=3), dict(stat=-1), dict(cx=0.0), dict(cy=0.0),
           dict(cx=float("nan")), dict(cy=float("inf")), dict(ww=0), dict(hh=-1), dict(ww=65536, hh=65536),
           dict(ms=-0.25), dict(ms=float("nan")), dict(ms=float("inf"))]
    for kw in bad:
        for fn in (generic, compact, compact_flats):
            k2 = kw
            if fn is not generic:
                if "el" in kw:
                    continue
                k2 = {("z" if k == "p" else k): v for k, v in kw.items()}
            rc = fn(**k2)
            assert rc == 2, (fn.__name__, kw, rc)                             # RDGPU_ERR_ARG
            with pytest.raises(rd.RdgpuError):
                check(rc, "x")
            assert (dist == SENT).all() and (rise == SENT).all(), kw
    assert compact_flats(ww=65536, hh=32768) == 2 and (dist == SENT).all()    # more than 0x7FFF0000 cells
    assert generic() == 0 and dist[2, 2] == 0.0 and dist[2, 3] == 1.0 and dist[0, 0] == -1.0   # (the same call, valid)

    import torch

    tp = torch.from_numpy(props).cuda()
    td = torch.full((h, w), SENT, dtype=torch.float64, device="cuda")
    tr = torch.full((h, w), SENT, dtype=torch.float64, device="cuda")
    tz = torch.from_numpy(dem).cuda()
    for call in (lambda: rd.mfd_distance_up_dev(tp),
                 lambda: rd.mfd_distance_up_dev(tp, dist=td, rise=tr),                        # rise without elev
                 lambda: rd.mfd_distance_up_dev(tp, stat=5, dist=td),
                 lambda: rd.mfd_distance_up_dev(tp, stat="median", dist=td),
                 lambda: rd.mfd_distance_up_dev(tp, min_share=-1.0, dist=td),
                 lambda: rd.mfd_distance_up_dev(tp, cell=(0.0, 1.0), dist=td),
                 lambda: rd.mfd_distance_up_dev(tp, cell=(1.0, float("nan")), dist=td),
                 lambda: rd.mfd_distance_up_dev(tp, dist=td[:, :-1]),
                 lambda: rd.dinf_distance_up_dev(tz, -9999),
                 lambda: rd.dinf_distance_up_dev(tz, -9999, stat=3, dist=td, rise=tr),
                 lambda: rd.dinf_distance_up_dev(tz, -9999, min_share=float("nan"), dist=td),
                 lambda: rd.dinf_distance_up_flats_dev(tz, -9999, cell=(float("inf"), 1.0), rise=tr),
                 lambda: rd.mfd_distance_up(props, want=("rise",)),
                 lambda: rd.mfd_distance_up(props, want=()),
                 lambda: rd.mfd_distance_up(props, stat="mean"),
                 lambda: rd.mfd_distance_up(props, cell=(0, 1)),
                 lambda: rd.mfd_distance_up(props[..., :8]),
                 lambda: rd.dinf_distance_up(dem, -9999, stat=7),
                 lambda: rd.dinf_distance_up(dem.astype(np.int64), -9999)):
        with pytest.raises(rd.RdgpuError):
            call()
    torch.cuda.synchronize()
    assert bool((td == SENT).all()) and bool((tr == SENT).all())


def test_every_new_symbol_is_exported(rd):
    names = ["rdgpu_mfd_distance_up", "rdgpu_mfd_distance_up_dev"]
    for t in ("u8", "i8", "i16", "u16", "i32", "u32", "f32", "f64"):
        names += [f"rdgpu_dinf_distance_up_{t}", f"rdgpu_dinf_distance_up_dev_{t}", f"rdgpu_dinf_distance_up_flats_{t}",
                  f"rdgpu_dinf_distance_up_flats_dev_{t}"]
    for n in names:
        assert hasattr(rd.lib(), n), n
    for n in ("mfd_distance_up", "dinf_distance_up", "dinf_distance_up_flats", "mfd_distance_up_dev", "dinf_distance_up_dev",
              "dinf_distance_up_flats_dev"):
        assert callable(getattr(rd, n)) and n in rd.__all__, n
