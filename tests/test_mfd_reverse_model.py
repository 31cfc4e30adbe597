"""CPU tests that pin tests/mfd_reverse_model.py, which stands in for a reference that does not exist: rasters whose
answers are written out by hand; a memoised top-down evaluation of the same recurrence written here; the adjoint identity
with the accumulation, sum(racc) == sum(weights * accumulation), where both sides are exact; and on D8 proportions the
dependence against a walk of the paths."""
import math
import os
import sys

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfd_reverse_model as model  # noqa: E402
from mfd_distance_model import OFFS, receivers  # noqa: E402

LEFT, UPLEFT, UP, UPRIGHT, RIGHT, DOWNRIGHT, DOWN, DOWNLEFT = range(1, 9)
DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
ND = -1.0
NDV = np.float32(-9999)
INF = float("inf")


def blank(h, w):
    p = np.full((h, w, 9), -1.0, np.float32)
    p[..., 0] = -2.0
    return p


def put(p, y, x, shares=None):
    """name cell (y, x): a data cell with the shares {n: share}"""
    p[y, x, 0] = 0.0 if shares else -1.0
    for n, s in (shares or {}).items():
        p[y, x, n] = s


def chain(length, h=3):
    """cells (1, 1) .. (1, length) of an h x (length + 2) raster, each flowing RIGHT into the next; the last has no receiver"""
    p = blank(h, length + 2)
    for x in range(1, length + 1):
        put(p, 1, x, {RIGHT: 1.0} if x < length else None)
    return p


def row(length, values, fill=0.0):
    a = np.full((3, length + 2), fill)
    a[1, 1:length + 1] = values
    return a


# ---- 1: by hand ---------------------------------------------------------------------------------------------------
def test_chain_3x5():
    p = chain(3)
    assert p.shape == (3, 5, 9)
    r = model.reverse_accum(p, row(3, [1.0, 2.0, 4.0]))
    assert r["racc"][1, 1:4].tolist() == [7.0, 6.0, 4.0]
    assert r["wmax"][1, 1:4].tolist() == [4.0, 4.0, 4.0]
    rest = np.ones((3, 5), bool)
    rest[1, 1:4] = False
    assert (r["racc"][rest] == ND).all() and (r["wmax"][rest] == ND).all() and (r["state"][rest] == model.NODATA).all()
    assert (r["state"][1, 1:4] == model.RESOLVED).all() and r["nrecv"][1, 1:4].tolist() == [1, 1, 0]
    with pytest.raises(ValueError):
        model.reverse_accum(p)


def test_fork_half_half_and_quarter_three_quarters():
    p = blank(5, 5)
    put(p, 1, 2, {DOWNLEFT: 0.5, DOWNRIGHT: 0.5})
    put(p, 2, 1, {DOWN: 0.25, DOWNRIGHT: 0.75})
    put(p, 2, 3)
    put(p, 3, 1)
    put(p, 3, 2)
    wts = np.zeros((5, 5))
    wts[1, 2], wts[2, 1], wts[2, 3], wts[3, 1], wts[3, 2] = 1.0, 2.0, 8.0, 16.0, 32.0
    r = model.reverse_accum(p, wts)
    assert r["racc"][2, 1] == 2.0 + 0.75 * 32.0 + 0.25 * 16.0 == 30.0      # n = 6 (down-right) before n = 7 (down)
    assert r["racc"][1, 2] == 1.0 + 0.5 * 8.0 + 0.5 * 30.0 == 20.0         # n = 6 before n = 8
    assert r["wmax"][1, 2] == 32.0 and r["wmax"][2, 1] == 32.0 and r["wmax"][2, 3] == 8.0
    assert r["nrecv"][1, 2] == 2 and r["nrecv"][2, 1] == 2
    dest = np.zeros((5, 5), np.uint8)
    dest[3, 2] = 1
    d = model.reverse_accum(p, None, dest)
    assert "wmax" not in d
    assert d["racc"][3, 2] == 1.0 and d["racc"][3, 1] == 0.0 and d["racc"][2, 1] == 0.75 and d["racc"][1, 2] == 0.375
    assert d["racc"][2, 3] == 0.0 and d["racc"][0, 0] == ND


def test_absorbing_cell_mid_chain():
    p = chain(5)
    dest = np.zeros((3, 7), np.uint8)
    dest[1, 3] = 1
    r = model.reverse_accum(p, row(5, [1.0, 2.0, 4.0, 8.0, 16.0]), dest)
    assert r["racc"][1, 1:6].tolist() == [7.0, 6.0, 4.0, 24.0, 16.0]       # nothing below (1, 3) counts above it
    assert r["wmax"][1, 1:6].tolist() == [4.0, 4.0, 4.0, 16.0, 16.0]
    assert r["nrecv"][1, 3] == 1                                           # (the graph itself keeps the link)


def test_weight_nodata_cell_passes_on_what_lies_below():
    p = chain(5)
    wts = row(5, [1.0, 2.0, 4.0, 8.0, 16.0])
    r = model.reverse_accum(p, wts, weight_nodata=4.0)
    assert r["racc"][1, 1:6].tolist() == [27.0, 26.0, 24.0, 24.0, 16.0]
    assert r["wmax"][1, 1:6].tolist() == [16.0] * 5
    wts[1, 2] = float("nan")
    r = model.reverse_accum(p, wts, weight_nodata=float("nan"))
    assert r["racc"][1, 1:6].tolist() == [29.0, 28.0, 28.0, 24.0, 16.0]
    wts = row(5, [1.0, -0.0, 4.0, 0.0, 16.0])
    r = model.reverse_accum(p, wts, weight_nodata=0.0)                     # == on doubles: -0.0 is the NoData 0.0
    assert r["wmax"][1, 1:6].tolist() == [16.0] * 5 and r["racc"][1, 1:6].tolist() == [21.0, 20.0, 20.0, 16.0, 16.0]
    r = model.reverse_accum(p, row(5, [-3.0, -0.0, -4.0, 0.0, -16.0]), weight_nodata=0.0)
    assert r["wmax"][1, 1:6].tolist() == [-3.0, -4.0, -4.0, -16.0, -16.0]  # the zeros do not contribute: no maximum of 0


def ring(absorb):
    """(1, 1) -> (1, 2) -> (2, 2) -> (2, 1) -> (1, 1); a chain of 10 cells feeds (1, 2) from the right; (1, 1) also gives
    half to the edge cell (2, 0)"""
    p = blank(4, 15)
    put(p, 1, 1, {RIGHT: 0.5, DOWNLEFT: 0.5})
    put(p, 2, 0)
    put(p, 1, 2, {DOWN: 1.0})
    put(p, 2, 2, {LEFT: 1.0})
    put(p, 2, 1, {UP: 1.0})
    for k in range(1, 11):
        put(p, 1, 2 + k, {LEFT: 1.0})
    dest = np.zeros((4, 15), np.uint8)
    if absorb:
        dest[2, 2] = 1
    return p, dest


def test_ring_and_ring_broken_by_an_absorbing_cell():
    p, dest = ring(False)
    ones = np.ones((4, 15))
    r = model.reverse_accum(p, ones, dest)
    assert (r["state"][1:3, 1:3] == model.UNDECIDED).all() and (r["state"][1, 3:13] == model.UNDECIDED).all()
    assert (r["racc"][1:3, 1:3] == ND).all() and (r["wmax"][1, 3:13] == ND).all()
    assert r["state"][2, 0] == model.RESOLVED and r["racc"][2, 0] == 1.0
    p, dest = ring(True)
    r = model.reverse_accum(p, ones, dest)
    data = p[..., 0] != -2.0
    assert (r["state"][data] == model.RESOLVED).all()
    assert r["racc"][2, 2] == 1.0 and r["racc"][1, 2] == 2.0 and r["racc"][1, 1] == 1.0 + 0.5 * 2.0 + 0.5 * 1.0
    assert r["racc"][2, 1] == 3.5 and r["racc"][1, 12] == 12.0


def test_share_into_nodata_and_onto_an_edge_cell():
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
    r = model.reverse_accum(p, np.ones((6, 8)))
    a = r["racc"]
    assert r["nrecv"][1, 1] == 1 and r["nrecv"][1, 4] == 0 and r["nrecv"][2, 7] == 0 and r["nrecv"][1, 2] == 2
    assert a[1, 4] == 1.0 and a[1, 3] == 2.0 and a[2, 7] == 1.0 and a[2, 4] == 4.0 and a[3, 3] == 1.0
    assert a[2, 3] == 1.0 + 0.125 * 4.0 + 0.5 * 1.0 == 2.0
    e12 = 1.0 + float(np.float32(0.7)) * 2.0
    e12 = e12 + float(np.float32(0.2)) * 2.0
    assert a[1, 2] == e12 and a[1, 1] == 1.0 + 0.5 * e12


def test_wmax_with_negative_weights_and_minus_infinity():
    p = chain(3)
    r = model.reverse_accum(p, row(3, [-5.0, -INF, -7.0]))
    assert r["wmax"][1, 1:4].tolist() == [-5.0, -7.0, -7.0]
    assert r["racc"][1, 1:4].tolist() == [-INF, -INF, -7.0]
    r = model.reverse_accum(p, row(3, [-INF, -INF, -INF]))
    assert r["wmax"][1, 1:4].tolist() == [-INF] * 3 and (r["state"][1, 1:4] == model.RESOLVED).all()
    r = model.reverse_accum(p, row(3, [-INF, 2.0, INF]))
    assert math.isnan(r["racc"][1, 1]) and r["racc"][1, 2] == INF and r["wmax"][1, 1] == INF


def test_decided_cell_without_a_maximum():
    p = chain(4)
    r = model.reverse_accum(p, row(4, [9.0, float("nan"), 9.0, 3.0]), weight_nodata=9.0)
    assert r["state"][1, 1:5].tolist() == [model.RESOLVED] * 4 and r["wmax"][1, 1:5].tolist() == [3.0] * 4
    dest = np.zeros((3, 6), np.uint8)
    dest[1, 3] = 1
    r = model.reverse_accum(p, row(4, [9.0, float("nan"), 9.0, 3.0]), dest, weight_nodata=9.0, out_nodata=-7.0)
    assert r["state"][1, 1:5].tolist() == [model.EMPTY, model.EMPTY, model.EMPTY, model.RESOLVED]
    assert r["wmax"][1, 1:5].tolist() == [-7.0, -7.0, -7.0, 3.0]
    assert r["racc"][1, 1:5].tolist() == [0.0, 0.0, 0.0, 3.0] and r["racc"][0, 0] == -7.0


# ---- 2: a memoised top-down evaluation of the same recurrence ------------------------------------------------------
def top_down(props, weights, dest, weight_nodata):
    """racc and wmax (None: no maximum) per data cell, from the recurrence alone: a cell's value is asked for, which asks for
    its receivers' (an explicit stack instead of recursion: paths are thousands of cells long).  No cycles are expected."""
    h, w, _ = props.shape
    data, rec = receivers(props)
    wl, conl = model.cell_weights(data, weights, weight_nodata, dest)
    absorb = (np.asarray(dest).ravel() != 0).tolist() if dest is not None else [False] * (h * w)
    flat = props.reshape(h * w, 9)
    recs = {}
    memo = {}

    def rcv(c):
        if c not in recs:
            y, x = divmod(c, w)
            recs[c] = [] if absorb[c] else [(n, c + OFFS[n][1] * w + OFFS[n][0]) for n in range(1, 9) if rec[n, y, x]]
        return recs[c]

    for root in np.flatnonzero(data.ravel()).tolist():
        stack = [root]
        while stack:
            c = stack[-1]
            if c in memo:
                stack.pop()
                continue
            missing = [r for _, r in rcv(c) if r not in memo]
            if missing:
                assert len(stack) <= h * w, "a cycle"
                stack.extend(missing)
                continue
            s = wl[c] if conl[c] else 0.0
            m = wl[c] if conl[c] else None
            for n, r in rcv(c):
                s = s + float(flat[c, n]) * memo[r][0]
                mr = memo[r][1]
                if mr is not None and (m is None or mr > m):
                    m = mr
            memo[c] = (s, m)
            stack.pop()
    return memo


@pytest.mark.parametrize("kind", ["dinf", "quinn"])
def test_model_equals_top_down_recursion(orc, kind):
    dem = fractal_dem(130, 70, 11)
    props = orc.port.fm_tarboton(dem, NDV) if kind == "dinf" else orc.port.fm_mfd(dem, NDV, "Quinn")
    h, w = dem.shape
    rng = np.random.default_rng(7)
    wts = rng.random((h, w))
    wts[rng.random((h, w)) < 0.03] = float("nan")
    wts[rng.random((h, w)) < 0.03] = -2.0
    dest = (orc.port.flow_accumulation(props) >= 30).astype(np.uint8)
    for de in (None, dest):
        r = model.reverse_accum(props, wts, de, weight_nodata=-2.0, out_nodata=ND)
        memo = top_down(props, wts, de, -2.0)
        data = props[..., 0] != -2.0
        assert (r["state"][data] != model.UNDECIDED).all() and len(memo) == int(data.sum())
        exp_a = np.full((h, w), ND)
        exp_m = np.full((h, w), ND)
        for c, (s, m) in memo.items():
            exp_a.flat[c] = s
            if m is not None:
                exp_m.flat[c] = m
        assert np.array_equal(r["racc"].view(np.uint64), exp_a.view(np.uint64))
        assert np.array_equal(r["wmax"].view(np.uint64), exp_m.view(np.uint64))
        assert ((r["state"] == model.EMPTY) == (data & (exp_m == ND))).all()
    assert (r["nrecv"][data] >= 2).mean() > 0.5


# ---- 3: the adjoint identity -------------------------------------------------------------------------------------
def _adjoint(orc, props, seed):
    h, w = props.shape[:2]
    data = props[..., 0] != -2.0
    wts = np.random.default_rng(seed).integers(0, 100, (h, w)).astype(np.float64)
    r = model.reverse_accum(props, wts)
    assert (r["state"][data] == model.RESOLVED).all()
    acc = orc.port.flow_accumulation(props)
    lhs = math.fsum(r["racc"][data].tolist())
    rhs = math.fsum((wts[data] * acc[data]).tolist())
    print("adjoint:", lhs, rhs)
    assert lhs == rhs and lhs > 0
    assert float(r["racc"][data].sum()) == float((wts * acc)[data].sum())
    return r


@pytest.mark.parametrize("dem_args", [(130, 70, 11), (260, 200, 305)], ids=["130x70", "260x200"])
def test_adjoint_identity_on_d8(orc, dem_args):
    """sum over cells of racc == sum over cells of weight x accumulation: both count every (cell, downslope cell) pair once.
    On D8 shares are 1 and the weights are integers below 100, so every value is an integer far below 2^53: equality."""
    dem = fractal_dem(*dem_args)
    r = _adjoint(orc, orc.port.fm_d8(dem, NDV), dem_args[2])
    a = r["racc"][r["state"] == model.RESOLVED]
    assert (a == np.floor(a)).all()


def braid(rows=12):
    """shares 0.5, 0.25 and 0.125 to the three cells below: after `rows` rows every value is a multiple of 2^-36 below 2^17"""
    p = blank(rows + 3, 9)
    for y in range(1, rows + 1):
        for x in range(2, 7):
            put(p, y, x, {DOWNLEFT: 0.5, DOWN: 0.25, DOWNRIGHT: 0.125})
    for x in range(1, 8):
        put(p, rows + 1, x)
        if x in (1, 7):
            for y in range(2, rows + 1):
                put(p, y, x, {DOWN: 1.0})
    return p


def test_adjoint_identity_on_a_braid_of_dyadic_shares(orc):
    r = _adjoint(orc, braid(), 3)
    assert r["nrecv"][5, 4] == 3


# ---- 4: the dependence on D8 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dem_args", [(130, 70, 11), (260, 200, 305)], ids=["130x70", "260x200"])
def test_d8_dependence_is_zero_or_one_and_follows_the_path(orc, dem_args):
    dem = fractal_dem(*dem_args)
    props = orc.port.fm_d8(dem, NDV)
    h, w = dem.shape
    dest = (orc.port.flow_accumulation(props) >= 30).astype(np.uint8)
    r = model.reverse_accum(props, None, dest)
    data, rec = receivers(props)
    assert rec.sum(axis=0).max() == 1
    decided = (r["state"] == model.RESOLVED)
    assert (decided == data).all()
    nxt = np.full(h * w, -1, np.int64)                     # the one receiver of every cell, -1 without
    for n, (dx, dy) in OFFS.items():
        ys, xs = np.nonzero(rec[n])
        nxt[ys * w + xs] = (ys + dy) * w + (xs + dx)
    dl = dest.ravel().tolist()
    nl = nxt.tolist()
    meets = np.zeros(h * w, bool)
    for c in np.flatnonzero(data.ravel()).tolist():
        k, steps = c, 0
        while k >= 0 and not dl[k]:
            k = nl[k]
            steps += 1
            assert steps <= h * w
        meets[c] = k >= 0
    dep = r["racc"].ravel()
    assert set(np.unique(dep[data.ravel()]).tolist()) <= {0.0, 1.0}
    assert ((dep == 1.0) == (meets & data.ravel())).all()
    assert 0 < int(meets.sum()) < int(data.sum())


# ---- 5: the public names -----------------------------------------------------------------------------------------
def test_python_names_are_exported_and_refuse_before_the_library():
    import richdem_amd as rd

    for n in ("mfd_reverse_accum", "mfd_upslope_dependence", "dinf_reverse_accum", "dinf_reverse_accum_flats",
              "dinf_upslope_dependence", "dinf_upslope_dependence_flats", "mfd_reverse_accum_dev", "dinf_reverse_accum_dev",
              "dinf_reverse_accum_flats_dev"):
        assert callable(getattr(rd, n)) and n in rd.__all__, n
    p = chain(3)
    ones = np.ones((3, 5))
    for call in (lambda: rd.mfd_reverse_accum(p),                                   # neither weights nor dest
                 lambda: rd.mfd_reverse_accum(p, dest=np.zeros((3, 5), np.uint8), want=("wmax",)),
                 lambda: rd.mfd_reverse_accum(p, ones, want=()),
                 lambda: rd.mfd_reverse_accum(p, ones, want=("dist",)),
                 lambda: rd.mfd_reverse_accum(p, np.ones((3, 4))),
                 lambda: rd.mfd_reverse_accum(p[..., :8], ones),
                 lambda: rd.mfd_upslope_dependence(p, None),
                 lambda: rd.dinf_reverse_accum(np.ones((3, 5), np.float32), -1.0),
                 lambda: rd.dinf_upslope_dependence(np.ones((3, 5), np.float32), -1.0, None),
                 lambda: rd.dinf_reverse_accum(np.ones((3, 5), np.int64), -1, ones)):
        with pytest.raises(rd.RdgpuError):
            call()
