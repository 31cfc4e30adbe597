"""The contraction rounds of the compact-label fill: cur[] kept for a round's roots only and the basins settled once after
the rounds (fill.settle_basins), the small rounds in one single-workgroup launch (fill.rounds_tail).  Every case runs with
the tail kernel at its default threshold, switched off (RDGPU_FILL_TAIL_ROOTS=0: every round is full-width launches) and
taking every round from the second on (a huge threshold), each with the rounds enqueued all at once and one per
synchronisation (RDGPU_FILL_ROUND_BATCH=1): the surface is the oracle's, cell for cell, and the number of rounds with work
does not depend on who ran them."""
import functools
import os

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

pytestmark = pytest.mark.gpu

HUGE = "4000000000"
SWITCHES = [{**({} if tail is None else {"RDGPU_FILL_TAIL_ROOTS": tail}), **({} if batch is None else {"RDGPU_FILL_ROUND_BATCH": batch})}
            for tail in (None, "0", HUGE) for batch in (None, "1")]
KEYS = ("RDGPU_FILL_TAIL_ROOTS", "RDGPU_FILL_ROUND_BATCH")


def _with_env(rd, env, dem, topo=8, **kw):
    old = {k: os.environ.get(k) for k in KEYS}
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        out = rd.FillDepressions(dem, topology=topo, **kw)
        return out, rd.fill_stats()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def staircase(n):
    """n x n, a chain of basins each of which spills into the next (tests/test_fallback_engines_gpu.py builds one of 20 000):
    one corridor winds through the raster between walls, along it a pit every fourth cell and between two pits a barrier,
    each barrier lower than the one before.  In round 1 every basin's lowest pass leads to the next basin: ONE chain of
    hooks through all of them."""
    h = w = n
    path = []
    rows = list(range(1, h - 1, 2))
    for i, y in enumerate(rows):
        xs = list(range(1, w - 1))
        path += [(y, x) for x in (xs if i % 2 == 0 else reversed(xs))]
        if i + 1 < len(rows):
            path.append((y + 1, path[-1][1]))
    path.append((path[-1][0], 0 if path[-1][1] == 1 else w - 1))
    L = len(path)
    z = np.full((h, w), float(L + 100), np.float32)
    for s, (y, x) in enumerate(path):
        z[y, x] = 0.0 if s % 4 == 0 else (10.0 + (L - s)) if s % 4 == 2 else 5.0
    z[path[-1]] = -1.0
    return z


def _plane():
    y, x = np.mgrid[0:200, 0:300]
    return (2.0 * y + 3.0 * x).astype(np.float32)


def _one_pit():
    z = _plane()
    z[100, 150] = -5.0
    return z


def _lattice():
    y, x = np.mgrid[0:70, 0:66]
    return np.where((x % 2 == 0) & (y % 2 == 0), 0, 1).astype(np.int32)


DEMS = {
    "fractal_1500x1100": lambda: fractal_dem(1500, 1100, seed=41),
    "fractal_700x900": lambda: fractal_dem(700, 900, seed=42),
    "plateaus_1500x1100": lambda: np.floor(fractal_dem(1500, 1100, seed=43) * 0.05).astype(np.int32),
    "plateaus_700x900": lambda: np.floor(fractal_dem(700, 900, seed=44) * 0.05).astype(np.int32),
    "staircase": lambda: staircase(150),          # 2 750 basins in one chain
    "noise_300x500": lambda: np.random.default_rng(7).random((300, 500)).astype(np.float32),
    "plane": _plane,
    "one_pit": _one_pit,
    "lattice_66x70": _lattice,
    "narrow_40x3000": lambda: fractal_dem(40, 3000, seed=45),
    "fractal_1200x900": lambda: fractal_dem(1200, 900, seed=46),
}


@functools.lru_cache(maxsize=None)
def _dem(name):
    z = DEMS[name]()
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _expected(orc, name, topo):
    exp = orc.port.fill(_dem(name), topo)
    exp.setflags(write=False)
    return exp


def _every_switch(rd, orc, name, topo):
    """the fill under every switch setting against the oracle; returns the statistics, in SWITCHES' order"""
    dem, exp = _dem(name), _expected(orc, name, topo)
    stats = []
    for env in SWITCHES:
        got, st = _with_env(rd, env, dem, topo)
        assert np.array_equal(got, exp), (name, topo, env, st)
        stats.append(st)
    return stats


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", ["fractal_1500x1100", "fractal_700x900", "plateaus_1500x1100", "plateaus_700x900"])
def test_fractal_and_plateau_dems(rd, orc, name, topo):
    stats = _every_switch(rd, orc, name, topo)
    for env, st in zip(SWITCHES, stats):
        assert st["rounds"] == stats[0]["rounds"] and st["rounds"] >= 2, (env, st, stats[0])
        assert st["edge_records"] > 0, (env, st)
        if "RDGPU_FILL_ROUND_BATCH" not in env:
            assert st["host_syncs"] == 2, (env, st)


def test_staircase_of_chained_basins(rd, orc):
    """the longest chain of links the settle pass and the tail kernel's chase can meet; D4, so that the walls' diagonal
    neighbours do not overflow the pair list and the compact-label path is the one that runs"""
    stats = _every_switch(rd, orc, "staircase", 4)
    for env, st in zip(SWITCHES, stats):
        assert st["basins"] >= 2700 and st["edge_records"] > 0, (env, st)
        assert st["rounds"] == stats[0]["rounds"], (env, st, stats[0])


@pytest.mark.parametrize("topo", [8, 4])
def test_white_noise(rd, orc, topo):
    """~230 basins per tile: pairs spill and the list may overflow -- whatever path the raster takes, the surface is equal"""
    stats = _every_switch(rd, orc, "noise_300x500", topo)
    if all(st["edge_records"] > 0 for st in stats):
        for env, st in zip(SWITCHES, stats):
            assert st["rounds"] == stats[0]["rounds"], (env, st, stats[0])


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", ["plane", "one_pit", "lattice_66x70", "narrow_40x3000"])
def test_degenerate_table_sizes(rd, orc, name, topo):
    stats = _every_switch(rd, orc, name, topo)
    if name == "plane":
        assert all(st["basins"] == 0 for st in stats), stats
    if name == "one_pit":
        assert all(st["basins"] == 1 for st in stats), stats


@pytest.mark.parametrize("shards", [2, 3])
def test_row_block_shards(rd, orc, shards):
    """the consumers of the settled cur[] / acc[] and of the node levels"""
    dem, exp = _dem("fractal_1200x900"), _expected(orc, "fractal_1200x900", 8)
    single, _ = _with_env(rd, {}, dem, 8)
    assert np.array_equal(single, exp)
    for env in SWITCHES:
        got, _ = _with_env(rd, env, dem, 8, shards=shards)
        assert np.array_equal(got, single), (shards, env)


def _launches(rd, env, dem, topo):
    rd.profile_enable(True)
    try:
        rd.profile_reset()
        got, st = _with_env(rd, env, dem, topo)
        tot = rd.profile_totals()
    finally:
        rd.profile_enable(False)
        rd.profile_reset()
    return got, st, {k: v[1] for k, v in tot.items() if k.startswith("fill.")}


@pytest.mark.parametrize("name", ["fractal_700x900", "plateaus_700x900"])
def test_launch_counts(rd, orc, name):
    """names that were not launched are absent from profile_totals"""
    dem, exp = _dem(name), _expected(orc, name, 8)
    got, st, n = _launches(rd, {}, dem, 8)
    print(name, "defaults", st, n)
    assert np.array_equal(got, exp)
    assert n.get("fill.update_basins", 0) == 0, n
    assert n.get("fill.settle_basins", 0) == 1, n
    assert n.get("fill.rounds_tail", 0) <= 1 and st["host_syncs"] == 2, (n, st)
    got, st, n = _launches(rd, {"RDGPU_FILL_ROUND_BATCH": "1"}, dem, 8)
    print(name, "batch 1", st, n)
    assert np.array_equal(got, exp)
    assert n.get("fill.rounds_tail", 0) <= st["host_syncs"] - 1, (n, st)       # (one synchronisation per batch, after the first)
    assert n.get("fill.update_basins", 0) == 0 and n.get("fill.settle_basins", 0) == 1, n
    got, st, n = _launches(rd, {"RDGPU_FILL_TAIL_ROOTS": "0"}, dem, 8)
    print(name, "no tail", st, n)
    assert np.array_equal(got, exp)
    assert n.get("fill.rounds_tail", 0) == 0, n
    assert n.get("fill.update_basins", 0) == 0 and n.get("fill.settle_basins", 0) == 1, n
