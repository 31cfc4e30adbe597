"""CPU tests that pin tests/mfd_distance_up_model.py, which stands in for a reference that does not exist: rasters whose
answers are written out by hand; the duality with the existing model of the way DOWN (mfd_distance_model.py) on the
transposed graph -- the donors of a cell become its receivers, so the distance up to the sources is the distance down to
the cells without receivers, bit for bit under min and max; and the share-weighted average against a memoised recursion
written here.  Then the public names, and that the Python wrappers refuse bad arguments before they call the library."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfd_distance_model as down  # noqa: E402
import mfd_distance_up_model as model  # noqa: E402

LEFT, UPLEFT, UP, UPRIGHT, RIGHT, DOWNRIGHT, DOWN, DOWNLEFT = range(1, 9)
DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
ND = -1.0
STATS = ("ave", "min", "max")
NDV = np.float32(-9999)


def blank(h, w):
    p = np.full((h, w, 9), -1.0, np.float32)
    p[..., 0] = -2.0
    return p


def put(p, y, x, shares=None):
    """name cell (y, x): a data cell with the shares {n: share}"""
    p[y, x, 0] = 0.0 if shares else -1.0
    for n, s in (shares or {}).items():
        p[y, x, n] = s


# ---- 1: by hand ---------------------------------------------------------------------------------------------------
def test_chain_of_three():
    p = blank(3, 5)
    put(p, 1, 1, {RIGHT: 1.0})
    put(p, 1, 2, {RIGHT: 1.0})
    put(p, 1, 3)
    z = np.zeros((3, 5))
    z[1, 1:4] = (10.0, 7.0, 3.0)
    r = model.distance_up_all(p, z)
    rest = np.ones((3, 5), bool)
    rest[1, 1:4] = False
    for stat in STATS:
        assert r[stat]["dist"][1, 1:4].tolist() == [0.0, 1.0, 2.0]
        assert r[stat]["rise"][1, 1:4].tolist() == [0.0, 3.0, 7.0]
        assert (r[stat]["dist"][rest] == ND).all() and (r[stat]["rise"][rest] == ND).all()
    assert r["ndonors"][1, 1:4].tolist() == [0, 1, 1] and r["decided"][1, 1:4].all() and not r["decided"][rest].any()
    assert "rise" not in model.distance_up(p)


def join():
    """A = (1, 1) gives 0.25 to B = (1, 2) on its right and 0.75 to C = (2, 2) down-right; B gives 1 to (1, 3) and 0.5 to C
    below it; C -> (2, 3) -> (2, 4).  The donors of C in the order of their position around it: A (up-left), then B (up)."""
    p = blank(4, 6)
    put(p, 1, 1, {RIGHT: 0.25, DOWNRIGHT: 0.75})
    put(p, 1, 2, {RIGHT: 1.0, DOWN: 0.5})
    put(p, 1, 3)
    put(p, 2, 2, {RIGHT: 1.0})
    put(p, 2, 3, {RIGHT: 1.0})
    put(p, 2, 4)
    return p


def test_join_of_two_donors():
    p = join()
    # C: v_A = 0 + sqrt(2) = 1.4142135623730951 with share 0.75, v_B = 1 + 1 = 2 with share 0.5
    # ave: num = 0.75 * 1.4142135623730951 + 0.5 * 2 = 1.0606601717798214 + 1 = 2.0606601717798214, den = 0.75 + 0.5 = 1.25
    r2 = math.sqrt(2.0)
    assert r2 == 1.4142135623730951 and 0.75 * r2 == 1.0606601717798214 and 2.0606601717798214 / 1.25 == 1.6485281374238572
    exp = {"ave": 1.6485281374238572, "min": r2, "max": 2.0}
    r = model.distance_up_all(p)
    for stat in STATS:
        d = r[stat]["dist"]
        assert d[1, 1] == 0.0 and d[1, 2] == 1.0 and d[1, 3] == 2.0
        assert d[2, 2] == exp[stat] and d[2, 3] == exp[stat] + 1.0 and d[2, 4] == exp[stat] + 1.0 + 1.0, stat
    assert r["ave"]["dist"][2, 4] == 3.648528137423857
    assert r["ndonors"][2, 2] == 2 and r["ndonors"][1, 1] == 0 and r["decided"][p[..., 0] != -2.0].all()
    # cells 3 wide and 4 high: a diagonal step is 5
    r = model.distance_up_all(p, cell=(3.0, -4.0))
    assert r["min"]["dist"][2, 2] == 5.0 and r["max"]["dist"][2, 2] == 7.0 and r["max"]["dist"][2, 4] == 13.0
    assert r["ave"]["dist"][2, 2] == (0.75 * 5.0 + 0.5 * 7.0) / 1.25 == 5.8
    # the rise: z(A) = 9, z(B) = 6, z(1, 3) = 4.5, z(C) = 8, z(2, 3) = 2, z(2, 4) = 1.25
    z = np.zeros((4, 6))
    z[1, 1], z[1, 2], z[1, 3], z[2, 2], z[2, 3], z[2, 4] = 9.0, 6.0, 4.5, 8.0, 2.0, 1.25
    r = model.distance_up_all(p, z)
    for stat in STATS:                       # every way up from C ends at A: v_A = 9 - 8, v_B = 3 + (6 - 8)
        h = r[stat]["rise"]
        assert h[1, 1] == 0.0 and h[1, 2] == 3.0 and h[1, 3] == 4.5 and h[2, 2] == 1.0 and h[2, 3] == 7.0 and h[2, 4] == 7.75
    z[1, 1] = 7.0                            # not clamped: the way A -> C now climbs, 7 - 8
    r = model.distance_up_all(p, z)
    assert r["min"]["rise"][2, 2] == -1.0 and r["max"]["rise"][2, 2] == -1.0 and r["ave"]["rise"][1, 2] == 1.0


def test_min_share_takes_links_away():
    p = join()
    for ms, src_b in ((0.0, False), (0.2499, False), (0.25, True), (0.5, True)):
        r = model.distance_up_all(p, min_share=ms)
        assert (r["ndonors"][1, 2] == 0) == src_b, ms             # A -> B carries 0.25: a link only below that threshold
        assert r["max"]["dist"][1, 2] == (0.0 if src_b else 1.0)
    r = model.distance_up_all(p, min_share=0.5)                   # B -> C (0.5) is not above 0.5 either: C hears from A alone
    assert r["ndonors"][2, 2] == 1
    for stat in STATS:
        assert r[stat]["dist"][2, 2] == math.sqrt(2.0) and r[stat]["dist"][1, 3] == 1.0
    r = model.distance_up_all(p, min_share=0.75)                  # ... and at 0.75 from nobody
    assert r["ndonors"][2, 2] == 0 and r["ave"]["dist"][2, 2] == 0.0 and r["ave"]["dist"][2, 4] == 2.0
    # the comparison is made in float32: 0.1 as a double is below float32(0.1), which is what the share holds
    q = blank(3, 4)
    put(q, 1, 1, {RIGHT: 0.1})
    put(q, 1, 2)
    assert float(np.float32(0.1)) > 0.1
    assert model.distance_up_all(q, min_share=0.1)["ndonors"][1, 2] == 0
    assert model.distance_up_all(q, min_share=0.0999)["ndonors"][1, 2] == 1


def test_edge_cells_have_donors_but_are_none():
    p = blank(4, 5)
    put(p, 1, 1, {LEFT: 0.5, RIGHT: 0.5})     # into the edge cell (1, 0) and into (1, 2)
    put(p, 1, 0, {RIGHT: 1.0})                # an edge cell with a positive share: it gives nobody a donor
    put(p, 1, 2, {UP: 1.0, DOWN: 0.25})       # into the edge cell (0, 2); down is NoData: dropped
    put(p, 0, 2, {DOWN: 1.0})
    put(p, 2, 1, {LEFT: 1.0})                 # its only share goes into NoData
    r = model.distance_up_all(p)
    assert r["ndonors"][1, 1] == 0 and r["ndonors"][1, 0] == 1 and r["ndonors"][1, 2] == 1 and r["ndonors"][0, 2] == 1
    assert r["ndonors"][2, 1] == 0
    d = r["ave"]["dist"]
    assert d[1, 1] == 0.0 and d[1, 0] == 1.0 and d[1, 2] == 1.0 and d[0, 2] == 2.0 and d[2, 1] == 0.0 and d[2, 2] == ND
    assert r["decided"].sum() == 5


def ring():
    """(1, 1) -> (1, 2) -> (2, 2) -> (2, 1) -> (1, 1), the last link with share 0.1; (2, 2) also feeds a tail of ten cells to
    its right.  Nothing on the ring or downstream of it is ever decided."""
    p = blank(5, 15)
    put(p, 1, 1, {RIGHT: 1.0})
    put(p, 1, 2, {DOWN: 1.0})
    put(p, 2, 2, {LEFT: 0.5, RIGHT: 0.5})
    put(p, 2, 1, {UP: 0.1})
    for x in range(3, 13):
        put(p, 2, x, {RIGHT: 1.0} if x < 12 else None)
    put(p, 3, 5, {RIGHT: 1.0})                # apart from the ring: decided
    put(p, 3, 6)
    return p


def test_cycle_and_its_tail_stay_undecided():
    p = ring()
    r = model.distance_up_all(p, out_nodata=-7.0)
    dec = r["decided"]
    assert not dec[1:3, 1:3].any() and not dec[2, 3:13].any() and dec[3, 5] and dec[3, 6]
    assert (r["max"]["dist"][2, 1:13] == -7.0).all() and r["max"]["dist"][3, 6] == 1.0
    r = model.distance_up_all(p, min_share=0.25)                  # the 0.1 link is gone: (1, 1) is a source
    assert r["decided"][p[..., 0] != -2.0].all()
    d = r["ave"]["dist"]
    assert d[1, 1] == 0.0 and d[1, 2] == 1.0 and d[2, 2] == 2.0 and d[2, 1] == 3.0 and d[2, 12] == 12.0


# ---- 2: the way up is the way down on the transposed graph -------------------------------------------------------
def transposed(props, min_share=0.0):
    """PT(c, m) = P(nbr(c, m), opp(m)) where that is a link, otherwise 0; the data cells stay data cells"""
    h, w, _ = props.shape
    t = np.zeros_like(props)
    t[..., 0] = np.where(props[..., 0] == np.float32(-2.0), np.float32(-2.0), np.float32(0.0))
    data = props[..., 0] != np.float32(-2.0)
    for m in range(1, 9):
        opp = m + 4 if m <= 4 else m - 4
        for y in range(1, h - 1):
            for x in range(1, w - 1):
                ty, tx = y + DY[m], x + DX[m]
                if data[y, x] and data[ty, tx] and props[ty, tx, opp] > np.float32(min_share):
                    t[y, x, m] = props[ty, tx, opp]
    return t


def ringed(dem):
    dem = dem.copy()
    dem[0, :] = dem[-1, :] = dem[:, 0] = dem[:, -1] = NDV
    return dem


def _duality(props, z, min_share):
    data = props[..., 0] != np.float32(-2.0)
    assert not data[0].any() and not data[-1].any() and not data[:, 0].any() and not data[:, -1].any()
    up = model.distance_up_all(props, z, min_share)
    dn = down.distance_down_all(transposed(props, min_share), None, z)
    dec = up["decided"]
    assert np.array_equal(dec, dn[("min", True)]["state"] == down.RESOLVED)
    assert np.array_equal(up["ndonors"], dn["nrecv"])
    for stat in ("min", "max"):
        a, b = up[stat]["dist"], dn[(stat, True)]["dist"]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), stat
    # negation and a - b = -(b - a) are exact (0.0 == -0.0: the sources)
    assert np.array_equal(up["max"]["rise"][dec], -dn[("min", True)]["drop"][dec])
    assert np.array_equal(up["min"]["rise"][dec], -dn[("max", True)]["drop"][dec])
    assert (up["max"]["rise"][~dec] == ND).all() and (up["min"]["rise"][~dec] == ND).all()
    return up


@pytest.mark.parametrize("kind", ["dinf", "quinn", "holmgren2", "d8"])
@pytest.mark.parametrize("min_share", [0.0, 0.25])
def test_duality_on_oracle_proportions(orc, kind, min_share):
    dem = ringed(fractal_dem(44, 36, 17))
    dem[10:14, 20:25] = NDV
    props = {"dinf": lambda: orc.port.fm_tarboton(dem, NDV), "quinn": lambda: orc.port.fm_mfd(dem, NDV, "Quinn"),
             "holmgren2": lambda: orc.port.fm_mfd(dem, NDV, "Holmgren", 2.0), "d8": lambda: orc.port.fm_d8(dem, NDV)}[kind]()
    up = _duality(props, dem.astype(np.float64), min_share)
    data = props[..., 0] != np.float32(-2.0)
    assert up["decided"][data].all() and up["max"]["dist"].max() > 5.0
    if kind != "d8" and min_share == 0.0:
        assert (up["ndonors"][data] >= 2).mean() > 0.3
        assert (up["max"]["dist"] != up["min"]["dist"]).any()


def test_duality_on_random_shares_with_cycles():
    rng = np.random.default_rng(7)
    h, w = 30, 34
    p = blank(h, w)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            if rng.random() < 0.1:
                continue
            ns = [n for n in range(1, 9) if rng.random() < 0.22]
            put(p, y, x, {n: np.float32(rng.random()) for n in ns})
    z = rng.random((h, w)) * 50.0
    up = _duality(p, z, 0.0)
    data = p[..., 0] != -2.0
    frac = float(up["decided"][data].mean())
    assert 0.05 < frac < 0.95, frac                # some cells are held up by cycles, some are not
    _duality(p, z, 0.3)


# ---- 3: ave against a memoised recursion -------------------------------------------------------------------------
@pytest.mark.parametrize("kind,min_share", [("quinn", 0.0), ("dinf", 0.0), ("quinn", 0.125)])
def test_ave_against_a_memoised_recursion(orc, kind, min_share):
    dem = fractal_dem(40, 28, 23)
    dem[5:8, 9:12] = NDV
    props = orc.port.fm_tarboton(dem, NDV) if kind == "dinf" else orc.port.fm_mfd(dem, NDV, "Quinn")
    h, w, _ = props.shape
    z = dem.astype(np.float64)
    ms = np.float32(min_share)
    diag = math.sqrt(2.0 * 2.0 + 3.0 * 3.0)

    def donors(y, x):
        out = []
        for m in range(1, 9):
            ty, tx = y + DY[m], x + DX[m]
            if 1 <= ty <= h - 2 and 1 <= tx <= w - 2 and props[ty, tx, 0] != -2.0 and props[ty, tx, m + 4 if m <= 4 else m - 4] > ms:
                out.append((m, ty, tx, float(props[ty, tx, m + 4 if m <= 4 else m - 4])))
        return out

    @functools.lru_cache(maxsize=None)
    def q(y, x, plane):
        ds = donors(y, x)
        if not ds:
            return 0.0
        v = [q(ty, tx, plane) + ((2.0 if m in (1, 5) else 3.0 if m in (3, 7) else diag) if plane == 0 else float(z[ty, tx]) - float(z[y, x]))
             for m, ty, tx, _ in ds]
        if len(v) == 1:
            return v[0]
        num = den = 0.0
        for (_, _, _, p), vd in zip(ds, v):
            num += p * vd
            den += p
        return num / den

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(20000)
    try:
        exp = np.full((2, h, w), -3.0)
        for y in range(h):
            for x in range(w):
                if props[y, x, 0] != -2.0:
                    exp[0, y, x], exp[1, y, x] = q(y, x, 0), q(y, x, 1)
    finally:
        sys.setrecursionlimit(old)
    got = model.distance_up(props, z, "ave", min_share, cell=(2.0, 3.0), out_nodata=-3.0)
    assert np.array_equal(got["dist"].view(np.uint64), exp[0].view(np.uint64))
    assert np.array_equal(got["rise"].view(np.uint64), exp[1].view(np.uint64))
    assert (got["dist"] > 10.0).sum() > 20


# ---- 4: the public surface ---------------------------------------------------------------------------------------
NAMES = ("mfd_distance_up", "dinf_distance_up", "dinf_distance_up_flats", "mfd_distance_up_dev", "dinf_distance_up_dev",
         "dinf_distance_up_flats_dev")


def test_names_are_public(rd):
    for name in NAMES:
        assert name in rd.__all__ and callable(getattr(rd, name))


def test_wrappers_refuse_bad_arguments_before_the_library(rd, monkeypatch):
    import torch

    import richdem_amd.api as api

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(api, "lib", no_library)
    p = join()
    dem = np.ones((4, 6), np.float32)
    z = np.zeros((4, 6))
    calls = [
        lambda: rd.mfd_distance_up(p[..., :8]),
        lambda: rd.mfd_distance_up(p.astype(np.float64)),
        lambda: rd.mfd_distance_up(p, want=()),
        lambda: rd.mfd_distance_up(p, want=("drop",)),
        lambda: rd.mfd_distance_up(p, want=("rise",)),                      # rise without elevations
        lambda: rd.mfd_distance_up(p, z[:, :-1], want=("rise",)),
        lambda: rd.mfd_distance_up(p, stat="median"),
        lambda: rd.mfd_distance_up(p, stat=3),
        lambda: rd.mfd_distance_up(p, min_share=-0.1),
        lambda: rd.mfd_distance_up(p, min_share=float("nan")),
        lambda: rd.mfd_distance_up(p, min_share=float("inf")),
        lambda: rd.mfd_distance_up(p, min_share="much"),
        lambda: rd.mfd_distance_up(p, cell=(0, 1)),
        lambda: rd.mfd_distance_up(p, cell=(1.0, float("nan"))),
        lambda: rd.mfd_distance_up(p, cell=3.0),
        lambda: rd.dinf_distance_up(dem.astype(np.int64), -9999),
        lambda: rd.dinf_distance_up(dem[0], -9999),
        lambda: rd.dinf_distance_up(dem, -9999, stat=7),
        lambda: rd.dinf_distance_up(dem, -9999, min_share=-1.0),
        lambda: rd.dinf_distance_up(dem, -9999, want=("dist", "drop")),
        lambda: rd.dinf_distance_up_flats(dem, -9999, cell=(float("inf"), 1.0)),
        lambda: rd.dinf_distance_up_flats(dem, -9999, stat="mean"),
        lambda: rd.mfd_distance_up_dev(torch.from_numpy(p), dist=torch.zeros(4, 6, dtype=torch.float64)),    # not on the GPU
        lambda: rd.dinf_distance_up_dev(torch.from_numpy(dem), -9999, dist=torch.zeros(4, 6, dtype=torch.float64)),
        lambda: rd.dinf_distance_up_flats_dev(torch.from_numpy(dem), -9999, dist=torch.zeros(4, 6, dtype=torch.float64)),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(rd.RdgpuError):
            call()
        assert k >= 0
    with pytest.raises(AssertionError, match="the library was called"):     # (a good call does get that far)
        rd.mfd_distance_up(p, z, "max", 0.5, (2.0, -3.0), want=("dist", "rise"))
