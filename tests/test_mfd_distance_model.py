"""CPU tests that pin tests/mfd_distance_model.py: rasters whose answers are written out by hand, and properties on D8
proportions, where every cell has at most one receiver (so the three statistics coincide bit for bit) and the resolved
cells are the cells that tests/flow_path_model.py gives a drainage cell."""
import math
import os
import sys

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_path_model as fpm  # noqa: E402
import mfd_distance_model as model  # noqa: E402

LEFT, UPLEFT, UP, UPRIGHT, RIGHT, DOWNRIGHT, DOWN, DOWNLEFT = range(1, 9)
ND = -1.0
STATS = ("ave", "min", "max")


def blank(h, w):
    p = np.full((h, w, 9), -1.0, np.float32)
    p[..., 0] = -2.0
    return p


def put(p, y, x, shares=None):
    """name cell (y, x): a data cell with the shares {n: share}"""
    p[y, x, 0] = 0.0 if shares else -1.0
    for n, s in (shares or {}).items():
        p[y, x, n] = s


def test_chain_of_three():
    p = blank(3, 5)
    put(p, 1, 1, {RIGHT: 1.0})
    put(p, 1, 2, {RIGHT: 1.0})
    put(p, 1, 3)
    z = np.zeros((3, 5))
    z[1, 1:4] = (10.0, 7.0, 3.0)
    for stat in STATS:
        for strict in (True, False):
            r = model.distance_down(p, None, z, stat, strict)
            assert r["dist"][1, 1:4].tolist() == [2.0, 1.0, 0.0]
            assert r["drop"][1, 1:4].tolist() == [7.0, 4.0, 0.0]
            assert (r["state"][1, 1:4] == model.RESOLVED).all()
            rest = np.ones((3, 5), bool)
            rest[1, 1:4] = False
            assert (r["dist"][rest] == ND).all() and (r["drop"][rest] == ND).all() and (r["state"][rest] == model.NODATA).all()


def fork():
    """A = (1, 1) gives 0.25 to B = (1, 2) on its right and 0.75 to C = (2, 2) down-right; B -> (1, 3); C -> (2, 3) -> (2, 4)"""
    p = blank(4, 6)
    put(p, 1, 1, {RIGHT: 0.25, DOWNRIGHT: 0.75})
    put(p, 1, 2, {RIGHT: 1.0})
    put(p, 1, 3)
    put(p, 2, 2, {RIGHT: 1.0})
    put(p, 2, 3, {RIGHT: 1.0})
    put(p, 2, 4)
    return p


def test_fork_quarter_three_quarters():
    p = fork()
    # v_5 = Q(B) + 1 = 2; v_6 = Q(C) + sqrt(2) = 2 + 1.4142135623730951 = 3.414213562373095
    # ave: num = 0.25 * 2 + 0.75 * 3.414213562373095 = 0.5 + 2.560660171779821 = 3.060660171779821, den = 0.25 + 0.75 = 1
    v5, v6 = 2.0, 3.414213562373095
    assert v6 == 2.0 + math.sqrt(2.0)
    assert 0.75 * v6 == 2.560660171779821 and 0.5 + 2.560660171779821 == 3.060660171779821
    exp = {"ave": 3.060660171779821, "min": v5, "max": v6}
    for stat in STATS:
        r = model.distance_down(p, None, None, stat, True)
        assert r["dist"][1, 1] == exp[stat], stat
        assert r["dist"][1, 2] == 1.0 and r["dist"][2, 2] == 2.0 and r["dist"][2, 3] == 1.0
        assert "drop" not in r
    # the drop: z(A) = 9, z(B) = 5, z(1, 3) = 4.5, z(C) = 8, z(2, 3) = 2, z(2, 4) = 1.25
    z = np.zeros((4, 6))
    z[1, 1], z[1, 2], z[1, 3], z[2, 2], z[2, 3], z[2, 4] = 9.0, 5.0, 4.5, 8.0, 2.0, 1.25
    # Q(B) = 0.5, Q(2, 3) = 0.75, Q(C) = 6.75; v_5 = 0.5 + 4 = 4.5, v_6 = 6.75 + 1 = 7.75; ave = (1.125 + 5.8125) / 1 = 6.9375
    exp = {"ave": 6.9375, "min": 4.5, "max": 7.75}
    for stat in STATS:
        r = model.distance_down(p, None, z, stat, False)
        assert r["drop"][1, 1] == exp[stat] and r["drop"][1, 2] == 0.5 and r["drop"][2, 2] == 6.75


def test_shares_that_do_not_sum_to_one():
    """den is the sum of the shares, not 1: shares 0.5 and 0.25 on the fork give (0.5 * 2 + 0.25 * v6) / 0.75"""
    p = fork()
    p[1, 1, RIGHT], p[1, 1, DOWNRIGHT] = 0.5, 0.25
    v6 = 3.414213562373095
    assert model.distance_down(p)["dist"][1, 1] == (1.0 + 0.25 * v6) / 0.75 == 2.471404520791032


def test_dead_terminal_strict_and_lenient():
    """only (1, 3) is a channel: (2, 4) has no receiver and is no stop cell -> DEAD, and so are (2, 3) and C"""
    p = fork()
    chan = np.zeros((4, 6), np.uint8)
    chan[1, 3] = 1
    chan[0, 0] = 1                                                  # (a NoData cell: no stop cell)
    for stat in STATS:
        s = model.distance_down(p, chan, None, stat, True)
        assert [s["state"][y, x] for y, x in ((2, 4), (2, 3), (2, 2), (1, 1))] == [model.DEAD] * 4
        assert s["dist"][1, 1] == ND and s["dist"][1, 2] == 1.0 and s["dist"][1, 3] == 0.0 and s["state"][0, 0] == model.NODATA
        le = model.distance_down(p, chan, None, stat, False)
        assert [le["state"][y, x] for y, x in ((2, 4), (2, 3), (2, 2))] == [model.DEAD] * 3
        assert le["state"][1, 1] == model.RESOLVED and le["dist"][1, 1] == 2.0    # one contributing receiver: v_5 itself


def ring():
    """(1, 1) -> (1, 2) -> (2, 2) -> (2, 1) -> (1, 1), and (1, 3) feeds (1, 2)"""
    p = blank(4, 5)
    put(p, 1, 1, {RIGHT: 1.0})
    put(p, 1, 2, {DOWN: 1.0})
    put(p, 2, 2, {LEFT: 1.0})
    put(p, 2, 1, {UP: 1.0})
    put(p, 1, 3, {LEFT: 1.0})
    return p


def test_cycle_with_and_without_a_stop_cell():
    p = ring()
    for strict in (True, False):
        r = model.distance_down(p, None, None, "ave", strict)
        cells = [(1, 1), (1, 2), (2, 2), (2, 1), (1, 3)]
        assert all(r["state"][c] == model.UNDECIDED and r["dist"][c] == ND for c in cells)
        chan = np.zeros((4, 5), np.uint8)
        chan[2, 2] = 1
        r = model.distance_down(p, chan, None, "ave", strict)
        assert [r["dist"][c] for c in cells] == [2.0, 1.0, 0.0, 3.0, 2.0]
        assert all(r["state"][c] == model.RESOLVED for c in cells)


def test_share_into_nodata_and_edge_cell():
    p = blank(4, 5)
    put(p, 1, 1, {RIGHT: 0.5, UP: 0.5, DOWN: 0.25})     # up is the edge cell (0, 1): NoData here; down is (2, 1): NoData
    put(p, 1, 2, {RIGHT: 1.0})
    put(p, 1, 3, {RIGHT: 1.0})
    put(p, 1, 4, {LEFT: 1.0})                           # an edge cell with a positive share: it has no receivers
    put(p, 2, 3, {DOWN: 1.0})                           # its only share goes into NoData: no receivers, a stop cell
    r = model.distance_down_all(p)
    assert r["nrecv"][1].tolist() == [0, 1, 1, 1, 0] and r["nrecv"][2, 3] == 0
    for key in [(s, t) for s in STATS for t in (True, False)]:
        assert r[key]["dist"][1].tolist() == [ND, 3.0, 2.0, 1.0, 0.0] and r[key]["dist"][2, 3] == 0.0
    chan = np.zeros((4, 5), np.uint8)
    chan[2, 3] = 1
    r = model.distance_down(p, chan, None, "max", False)
    assert (r["state"][1, 1:] == model.DEAD).all() and r["state"][2, 3] == model.RESOLVED


def test_cell_sizes():
    p = blank(5, 5)
    put(p, 1, 1, {RIGHT: 1.0})
    put(p, 1, 2, {DOWN: 1.0})
    put(p, 2, 2, {DOWNRIGHT: 1.0})
    put(p, 3, 3)
    for cell in ((2, 3), (-2, 3), (2.0, -3.0)):
        r = model.distance_down(p, cell=cell)
        d = math.sqrt(13.0)
        assert r["dist"][3, 3] == 0.0 and r["dist"][2, 2] == d and r["dist"][1, 2] == d + 3.0 and r["dist"][1, 1] == (d + 3.0) + 2.0


@pytest.fixture(scope="module")
def d8_case(orc):
    dem = fractal_dem(130, 70, 11)
    dem[30:36, 50:70] = np.float32(-9999)
    props = orc.port.fm_d8(dem, np.float32(-9999))
    chan = (orc.port.flow_accumulation(props) >= 30).astype(np.uint8)
    return dem, props, chan


def test_d8_proportions_one_receiver(d8_case):
    dem, props, chan = d8_case
    assert dem.shape == (70, 130)
    for ch in (None, chan):
        r = model.distance_down_all(props, ch, dem, cell=(2.0, 3.0))
        assert r["nrecv"].max() == 1
        for strict in (True, False):
            a = r[("ave", strict)]
            assert (a["state"] == model.RESOLVED).mean() > 0.4
            for stat in ("min", "max"):
                for plane in ("dist", "drop"):
                    assert np.array_equal(a[plane].view(np.uint64), r[(stat, strict)][plane].view(np.uint64))
        for plane in ("dist", "drop", "state"):     # one receiver: all or at least one is the same condition
            assert np.array_equal(r[("ave", True)][plane], r[("ave", False)][plane])


def test_d8_resolved_cells_have_a_drainage_cell(d8_case):
    dem, props, chan = d8_case
    dirs = np.zeros(dem.shape, np.uint8)
    for n in range(1, 9):
        dirs[props[..., n] > 0] = n
    dirs[props[..., 0] == -2.0] = 255
    for ch in (None, chan):
        exp = fpm.flow_path(dirs, 255, ch)["to_cell"] != fpm.NONE
        got = model.distance_down(props, ch)["state"] == model.RESOLVED
        assert np.array_equal(got, exp)
        if ch is not None:
            assert (model.distance_down(props, ch)["state"] == model.DEAD).any()
