"""The coarse flood on the workspace's side lane, beside k_resolve_nodes and k_init_tables (csrc/fill.hip, DESIGN.md section
3a r14; RDGPU_FILL_COARSE_LANE=0 puts it back on the caller's stream).  What the lane could break is ORDER: flags read
before k_flag_tiles wrote them, lane work that outlives its call and meets the next call's workspace, a caller's stream that
does not wait for the lane.  Every case runs with RDGPU_FILL_COARSE=1 on coarse_flood_model's rasters and
fractal_dem(1030, 770, 3), the smallest shapes that hold a flagged interior tile (the fractal: none, by the model), and every
precondition is asserted on the CPU with the model."""
import math

import numpy as np
import pytest

import coarse_flood_model as cm
import flooded_tiles_model as fm
import richdem_amd
from richdem_amd.synth import fractal_dem

pytestmark = pytest.mark.gpu

CB = richdem_amd.fill_coarse_block()
FALLBACKS = ("node table overflow", "hook chain unfinished", "pair list overflow")
SWITCHES = ("RDGPU_DEVICES", "RDGPU_FILL_EDGES", "RDGPU_FILL_EDGE_CAP", "RDGPU_FILL_ROUND_BATCH", "RDGPU_FILL_TAIL_ROOTS",
            "RDGPU_FILL_DISSOLVE", "RDGPU_FILL_FLOODED", "RDGPU_FILL_COUNT_FLOODED", "RDGPU_FILL_COARSE", "RDGPU_FILL_COUNT_COARSE",
            "RDGPU_FILL_COARSE_LANE", "RDGPU_FILL_DEBUG")
RASTERS = cm.rasters(CB)
_CACHE = {}


def opened_bowl():
    """the thick bowl with its rim opened: a channel one block wide, below every other cell, from the lake through the wall
    band to the raster's left edge.  Same shape and type as the thick bowl; the coarse lake drains and no tile is flagged."""
    z = RASTERS["thick bowl"][0].copy()
    z[100:100 + CB, 0:3 * CB] = np.float32(-1.0)
    return z


def raster(oracle, name):
    """(raster, oracle's D8 fill, flagged tiles by the model, census of flooded tiles), computed once and left unchanged"""
    if name not in _CACHE:
        z = {"opened bowl": opened_bowl, "fractal": lambda: fractal_dem(1030, 770, 3)}.get(name, lambda: RASTERS[name][0])()
        exp = oracle.port.fill(z, 8)
        for a in (z, exp):
            a.setflags(write=False)
        _CACHE[name] = (z, exp, int(cm.flags(z, CB, 8, oracle.port.fill).sum()), fm.flooded_tiles(z, exp))
    return _CACHE[name]


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got.view(np.uint8) != exp.view(np.uint8)).reshape(got.shape + (-1,)).any(axis=-1).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:8].tolist())


@pytest.fixture
def env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RDGPU_FILL_COARSE", "1")
    return monkeypatch


def _fill_dev(rd, z):
    """one fill through the device entry on torch's current stream; (output, statistics)"""
    import torch

    t = torch.tensor(z, device="cuda")   # (a copy: the shared raster is read-only)
    rd.fill_depressions_dev(t)
    st = rd.fill_stats()
    torch.cuda.synchronize()
    return t.cpu().numpy(), st


def test_flags_are_not_stale(rd, orc, env):
    """A (tiles flagged), B (same shape and type, none flagged), A, B on one workspace: a pair pass that ran ahead of
    k_flag_tiles would see the other raster's flags"""
    env.setenv("RDGPU_FILL_COUNT_COARSE", "1")
    a, b = raster(orc, "thick bowl"), raster(orc, "opened bowl")
    assert a[0].shape == b[0].shape and a[0].dtype == b[0].dtype
    assert a[2] >= 1 and a[2] == RASTERS["thick bowl"][1] and b[2] == 0
    for k, (name, (z, exp, flagged, _)) in enumerate((("A", a), ("B", b), ("A", a), ("B", b))):
        got, st = _fill_dev(rd, z)
        n = rd.fill_coarse_tiles()
        print(k, name, "coarse tiles:", n, "model:", flagged, st)
        _same(got, exp, f"fill {k} ({name})")
        assert n == flagged and st["host_syncs"] == 4, (k, name, n, flagged, st)


@pytest.mark.parametrize("name", ["thick bowl", "two lakes", "fractal"])
def test_lane_on_and_off_agree(rd, orc, env, capfd, name):
    z, exp, flagged, census = raster(orc, name)
    env.setenv("RDGPU_FILL_DEBUG", "1")
    env.setenv("RDGPU_FILL_COUNT_COARSE", "1")
    env.setenv("RDGPU_FILL_COUNT_FLOODED", "1")
    seen = {}
    for lane in (None, "0", "1"):
        if lane is None:
            env.delenv("RDGPU_FILL_COARSE_LANE", raising=False)
        else:
            env.setenv("RDGPU_FILL_COARSE_LANE", lane)
        capfd.readouterr()
        got, st = _fill_dev(rd, z)
        err = capfd.readouterr().err
        seen[lane] = (got, rd.fill_coarse_tiles(), rd.fill_flooded_tiles(), st["host_syncs"])
        print(name, "lane", lane, seen[lane][1:], "model:", flagged, "census:", census)
        assert not any(m in err for m in FALLBACKS), err
    for lane, (got, nc, nf, syncs) in seen.items():
        _same(got, exp, f"{name}, RDGPU_FILL_COARSE_LANE={lane}")
        assert syncs == 4 and nc == flagged and nf == census, (lane, syncs, nc, flagged, nf, census)
    assert np.array_equal(seen[None][0].view(np.uint8), seen["0"][0].view(np.uint8))


@pytest.mark.parametrize("stream", ["null", "own"])
@pytest.mark.parametrize("name", ["thick bowl", "fractal"])
def test_callers_stream_is_ordered_behind_the_lane(rd, orc, env, name, stream):
    """a copy enqueued on the caller's stream directly behind the fill, and nothing waited for but that stream"""
    import torch

    z, exp, flagged, _ = raster(orc, name)
    st = torch.cuda.default_stream() if stream == "null" else torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = torch.tensor(z, device="cuda")
        out = torch.empty_like(t)
        host = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        rd.fill_depressions_dev(t)
        out.copy_(t, non_blocking=True)
        host.copy_(out, non_blocking=True)
        st.synchronize()
    assert rd.fill_stats()["host_syncs"] == 4
    _same(host.numpy(), exp, f"{name} on the {stream} stream")


def test_fallback_leaves_the_lane_clean(rd, orc, env, capfd):
    """the pair list overflows with the lane joined: the classic path takes over, and the next fill on the workspace is right"""
    z, exp, flagged, _ = raster(orc, "thick bowl")
    assert flagged >= 1
    env.setenv("RDGPU_FILL_DEBUG", "1")
    env.setenv("RDGPU_FILL_EDGE_CAP", "64")
    capfd.readouterr()
    got, _ = _fill_dev(rd, z)
    assert "pair list overflow" in capfd.readouterr().err
    _same(got, exp, "thick bowl, pair list of 64 records")
    env.delenv("RDGPU_FILL_EDGE_CAP")
    env.setenv("RDGPU_FILL_COUNT_COARSE", "1")
    for name in ("two lakes", "thick bowl"):
        z, exp, flagged, _ = raster(orc, name)
        capfd.readouterr()
        got, st = _fill_dev(rd, z)
        assert not any(m in capfd.readouterr().err for m in FALLBACKS)
        _same(got, exp, name + " after the fallback")
        assert rd.fill_coarse_tiles() == flagged and st["host_syncs"] == 4, (name, st)


def test_growing_workspace(rd, orc, env):
    """rasters of increasing size one after another from an empty workspace: every buffer of the nested fill and of the
    outer one is regrown, none under a running lane"""
    names = ["spill east", "thick bowl", "odd 262 x 259", "two lakes", "fractal"]
    sizes = [raster(orc, n)[0].size for n in names]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
    rd.release_workspace()
    env.setenv("RDGPU_FILL_COUNT_COARSE", "1")
    for name in names:
        z, exp, flagged, _ = raster(orc, name)
        got, st = _fill_dev(rd, z)
        _same(got, exp, name + ", growing")
        assert rd.fill_coarse_tiles() == flagged and st["host_syncs"] == 4, (name, st)


@pytest.mark.parametrize("name", ["thick bowl", "fractal"])
def test_profile_on_two_streams(rd, orc, env, name):
    """the profiler's events are recorded on the stream of the launch: the nested fill's on the lane"""
    import torch

    z, exp, _, _ = raster(orc, name)
    t = torch.tensor(z, device="cuda")
    rd.profile_reset()
    rd.profile_enable(True)
    try:
        rd.fill_depressions_dev(t)
        torch.cuda.synchronize()
    finally:
        rd.profile_enable(False)
    tot = rd.profile_totals()
    rd.profile_reset()
    nested = {k: v for k, v in tot.items() if k.startswith("coarse.")}
    print(nested)
    assert nested and all(k.startswith("coarse.fill.") for k in nested), nested
    assert nested["coarse.fill.descent"][1] == 1 and nested["coarse.fill.finalize"][1] == 1
    for k, (ms, n) in tot.items():
        assert math.isfinite(ms) and ms >= 0 and n >= 1, (k, ms, n)
    assert tot["fill.flag_tiles"][1] == 1 and tot["fill.pairs_flooded"][1] == 1
    _same(t.cpu().numpy(), exp, name + ", profiled")
