"""The Python model of depression breaching (tests/breach_model.py) against the compiled reference's goldens
(tests/golden/ref_breach.npz, CompleteBreaching_Lindsay2016<D8>) and against itself: the local pit rule equals the serial
pass, the closure equals the serial walks (on the flood's trees and on random forests, loops included), the composition law
of the carve's steps holds, and a breached DEM has no depressions.  No GPU; the argument errors of the C-ABI return before
any device work and are checked here as well."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import breach_cases as bc  # noqa: E402
import breach_model as bm  # noqa: E402
from digest import load_golden  # noqa: E402

GOLDEN = load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_breach.npz"))
_MODEL = {}


def model(name):
    """the model's planes of a golden case, computed once and left unchanged"""
    if name not in _MODEL:
        dem = bc.CASES[name]()
        _MODEL[name] = (dem, bm.breach(dem))
    return _MODEL[name]


def random_dems(count, seed):
    rng = np.random.default_rng(seed)
    for i in range(count):
        h, w = rng.integers(1, 41, 2)
        if i % 3 == 0:
            yield rng.integers(0, 6, (h, w)).astype(np.int16)
        elif i % 3 == 1:
            yield rng.permutation(h * w).reshape(h, w).astype(np.int32)
        else:
            z = rng.random((h + 2, w + 2))
            yield ((z[:-2, :-2] + z[1:-1, 1:-1] + z[2:, 2:] + z[:-2, 2:] + z[2:, :-2]) / 5).astype(np.float32)


def test_golden_cases_are_the_registry():
    assert list(GOLDEN["cases"]) == list(bc.CASES)
    for name in bc.CASES:
        dem = bc.CASES[name]()
        assert tuple(GOLDEN[name + "/shape"]) == dem.shape
        if name + "/dem" in GOLDEN:
            assert np.array_equal(GOLDEN[name + "/dem"], dem) and GOLDEN[name + "/dem"].dtype == dem.dtype


@pytest.mark.parametrize("name", list(bc.CASES))
def test_model_equals_reference(name):
    dem, m = model(name)
    exp = GOLDEN[name + "/out"]
    assert exp.dtype == dem.dtype
    bad = int((m["out"] != exp).sum())
    print(name, "cells differing from the reference:", bad, "pits", int(m["pits"].sum()), "on a path", int(m["path"].sum()))
    assert bad == 0
    assert ((m["out"] != m["d1"]) <= (m["path"] == 1)).all()        # a changed cell lies on a path
    assert (m["path"] >= m["pits"]).all()                             # a pit is on its own path


def test_cases_hit_what_they_aim_at():
    dem, m = model("corridor_f32")
    assert int((m["out"] == 50.0).sum()) > 4095 * 4 and bc.corridor()[1] > 4095 * 4          # one carve, many tiles' worth
    low = model("corridor_low_f32")[1]["out"]
    assert int((low == 50.0).sum()) > 4095 and int((low == 7.0).sum()) > 4095                # the walk stops at the low cells
    dem, m = model("equal_pits_i16")
    assert (m["out"][10, :132] == 20).all() and m["pits"][10, 20] and m["pits"][10, 131]     # two pits, tiles 0 and 2, one path
    dem, m = model("nested_i32")
    assert m["pits"].sum() >= 2 and (m["out"][m["path"] == 1] == 10).sum() > 5
    for t in bc.TYPES:
        dem, m = model("extremes_" + bc.SUFFIX[t.name])
        lo, hi = (-np.inf, np.inf) if t.kind == "f" else (np.iinfo(t).min, np.iinfo(t).max)
        assert (m["out"][5, :66] == lo).all()                                                 # the minimum carved to the edge
        if t.kind != "f":
            assert m["pits"][8, 39] and m["path"][8, 38] and m["out"][8, 38] == hi           # the maximum at a pit, on a path
    assert not model("tilted_f32_40x30")[1]["pits"].any()


def test_local_pit_rule_equals_serial_pass():
    for dem in itertools.chain(random_dems(150, 11), (bc.CASES[n]() for n in ("q_u8_97x70", "extremes_f32", "extremes_u8", "pit_u8_3x3"))):
        if min(dem.shape) < 3:
            continue
        z, pits = bm.pit_pass_serial(dem)
        d1, pits2 = bm.pit_pass_local(dem)
        assert np.array_equal(z, d1) and np.array_equal(pits, pits2)


def test_closure_equals_serial_algorithm():
    for dem in random_dems(150, 12):
        m = bm.breach(dem)
        assert np.array_equal(bm.breach_serial(dem), m["out"])
        if min(dem.shape) < 3:
            continue
        walks = bm.carve_serial_walks(m["d1"], m["dirs"], m["pits"], m["order"])
        rec = bm.breach_along_recurrence(m["d1"], m["dirs"], m["pits"])
        for got in (walks, rec):
            assert np.array_equal(got[0], m["out"]) and np.array_equal(got[1], m["path"])


def random_forest(rng, h, w, loops):
    """random directions: with loops = False every link points to a cell of lower random priority (a forest)"""
    dirs = rng.integers(0, 9, (h, w)).astype(np.uint8)
    dirs[rng.random((h, w)) < 0.05] = 255
    if not loops:
        prio = rng.permutation(h * w).reshape(h, w)
        nxt = bm.links(dirs).reshape(h, w)
        bad = (nxt >= 0) & (prio.ravel()[np.maximum(nxt, 0)] >= prio)
        dirs[bad] = 0
    return dirs


def test_closure_on_random_forests_and_loops():
    rng = np.random.default_rng(13)
    for i in range(120):
        h, w = rng.integers(1, 25, 2)
        dem = rng.integers(0, 5, (h, w)).astype(np.int8) if i % 2 else rng.random((h, w)).astype(np.float32)
        if dem.dtype.kind == "f" and i % 4 == 0:
            dem[rng.random((h, w)) < 0.05] = np.nan
        pits = (rng.random((h, w)) < 0.2).astype(np.uint8)
        for loops in (False, True):
            dirs = random_forest(rng, h, w, loops)
            out, path = bm.breach_along(dem, dirs, pits)
            order = rng.permutation(h * w)                                    # the walks commute: any order of the pits
            w_out, w_path = bm.carve_serial_walks(dem, dirs, pits, order)
            assert np.array_equal(out, w_out, equal_nan=True) and np.array_equal(path, w_path)
            if not loops:
                r_out, r_path = bm.breach_along_recurrence(dem, dirs, pits)
                assert np.array_equal(out, r_out, equal_nan=True) and np.array_equal(path, r_path)
            # the contract, cell by cell: nothing rises, a cell off every path is unchanged, NoData directions are untouched
            keep = (path == 0) | (dirs == 255)
            assert np.array_equal(out[keep], dem[keep], equal_nan=True)
            assert not path[dirs == 255].any() and not path[np.isnan(dem.astype(np.float64))].any()


def test_composition_law():
    vals = [0, 1, 2, 3, bm.INF]
    steps = [(a, c) for a in vals[:-1] for c in vals if c <= a or c == bm.INF]
    for s1, s2 in itertools.product(steps, steps):
        a, c = bm.compose(s1, s2)          # (a composed step may inject above its threshold: c <= a holds for one cell only)
        for x in vals:
            assert bm.step(*s2)(bm.step(*s1)(x)) == bm.step(a, c)(x), (s1, s2, x)
    for s1, s2, s3 in itertools.product(steps, steps, steps):
        assert bm.compose(bm.compose(s1, s2), s3) == bm.compose(s1, bm.compose(s2, s3))


@pytest.mark.parametrize("name", [n for n in bc.CASES if "extremes" not in n])
def test_no_depressions_afterwards(name, orc):
    dem, m = model(name)
    if min(dem.shape) < 3:
        return
    out = m["out"].astype(np.float64).astype(np.float32) if dem.dtype.itemsize == 4 and dem.dtype.kind != "f" else m["out"]
    assert not orc.port.has_depressions(np.ascontiguousarray(out))
    assert np.array_equal(orc.port.fill(np.ascontiguousarray(out)), out)


def test_argument_errors_without_a_device(rd):
    L = rd.lib()
    a = np.zeros((4, 4), np.float32)
    d = np.zeros((4, 4), np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nd = ctypes.c_uint8(255)
    out = np.full((4, 4), 77, np.float32)
    path = np.full((4, 4), 77, np.uint8)
    for args in ((None, nd, p(a), p(d), 4, 4, p(out), p(path)), (p(d), nd, None, p(d), 4, 4, p(out), p(path)),
                 (p(d), nd, p(a), None, 4, 4, p(out), p(path)), (p(d), nd, p(a), p(d), 4, 4, None, None),
                 (p(d), nd, p(a), p(d), 0, 4, p(out), p(path)), (p(d), nd, p(a), p(d), 4, -1, p(out), p(path)),
                 (p(d), nd, p(a), p(d), 70000, 70000, p(out), p(path))):
        assert L.rdgpu_d8_breach_along_f32(*args) == 2
        assert L.rdgpu_d8_breach_along_dev_f32(*args, None) == 2
    for args in ((None, ctypes.c_float(0), 0, 4, 4, None, None), (p(a), ctypes.c_float(0), 0, 0, 4, None, None),
                 (p(a), ctypes.c_float(0), 0, 50000, 50000, None, None)):
        assert L.rdgpu_breach_d8_f32(*args) == 2
        assert L.rdgpu_breach_d8_dev_f32(*args, None) == 2
    assert L.rdgpu_breach_get_stats(None) == 2
    assert (out == 77).all() and (path == 77).all() and not a.any()
    for bad in (dict(want=()), dict(want=("out", "nope"))):
        with pytest.raises(rd.RdgpuError):
            rd.d8_breach_along(d, a, d, **bad)
    with pytest.raises(rd.RdgpuError):
        rd.d8_breach_along(d, a.astype(np.float64), d)
    with pytest.raises(rd.RdgpuError):
        rd.breach_depressions(a.astype(np.int64))
    with pytest.raises(rd.RdgpuError):
        rd.breach_depressions(a, want=("levels",))
