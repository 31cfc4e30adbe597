"""The coarse flood ahead of the compact fill's pair pass (k_descent16's block minima, the nested coarse fill, k_flag_tiles,
k_pairs_flooded; csrc/fill.hip), forced on at these small sizes with RDGPU_FILL_COARSE=1.

Every case is checked for

* the output equal, bits included, to the CPU oracle's fill, to the same call under RDGPU_FILL_COARSE=0 and to the same
  call under RDGPU_FILL_FLOODED=0 (which switches the coarse flood off as well: it needs the tiles' largest keys);
* under RDGPU_FILL_COUNT_COARSE=1 `fill_coarse_tiles()` equal to coarse_flood_model.flags()' count -- the tiles are left
  out of the pair pass, and only where they may be -- and `fill_flooded_tiles()` equal to the census as before;
* `host_syncs` 4 where a coarse fill ran, 2 where it is switched off or, with the variable unset, below the threshold.

The rasters are coarse_flood_model's for the library's block size; test_fill_coarse_flood_model.py says what each shows."""
import ctypes

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
            "RDGPU_FILL_DISSOLVE", "RDGPU_FILL_FLOODED", "RDGPU_FILL_COUNT_FLOODED", "RDGPU_FILL_COARSE", "RDGPU_FILL_COUNT_COARSE")
RASTERS = cm.rasters(CB)
_ORACLE = {}


def _oracle(orc, key, z, topo):
    """(oracle's fill, flagged tiles of the model, census of flooded tiles), once per raster and topology"""
    if (key, topo) not in _ORACLE:
        exp = orc.port.fill(z, topo)
        exp.setflags(write=False)
        _ORACLE[(key, topo)] = (exp, int(cm.flags(z, CB, topo, orc.port.fill).sum()), fm.flooded_tiles(z, exp))
    return _ORACLE[(key, topo)]


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    bad = int((got.view(np.uint8) != exp.view(np.uint8)).reshape(got.shape + (-1,)).any(axis=-1).sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != exp)[:8].tolist())


def _run(rd, z, topo, entry):
    """(output, coarse tiles, flooded tiles, stats) of one fill"""
    if entry == "host":
        got = rd.FillDepressions(z, topology=topo)
    else:
        import torch

        t = torch.from_numpy(z).cuda()
        rd.fill_depressions_dev(t, topology=topo)
        torch.cuda.synchronize()
        got = t.cpu().numpy()
    return got, rd.fill_coarse_tiles(), rd.fill_flooded_tiles(), rd.fill_stats()


def _check(rd, orc, monkeypatch, capfd, key, z, topo, entry="host"):
    """the checks of one raster through one entry; returns the number of flagged tiles"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RDGPU_FILL_DEBUG", "1")
    monkeypatch.setenv("RDGPU_FILL_COUNT_FLOODED", "1")
    monkeypatch.setenv("RDGPU_FILL_COUNT_COARSE", "1")
    keep = z.copy()
    exp, flagged, census = _oracle(orc, key, z, topo)
    what = f"{key} D{topo} {entry}"

    def run(syncs, n_coarse, n_flooded):
        capfd.readouterr()
        got, nc, nf, st = _run(rd, z, topo, entry)
        err = capfd.readouterr().err
        print(what, "coarse tiles:", nc, "model:", flagged, "flooded tiles:", nf, "census:", census, st)
        assert not any(m in err for m in FALLBACKS), (what, err)
        assert st["host_syncs"] == syncs, (what, st)
        assert nc == n_coarse and nf == n_flooded, (what, nc, n_coarse, nf, n_flooded)
        return got

    unset = run(2, 0, census)                                   # below the threshold: as ever
    _same(unset, exp, what + ", unset")
    monkeypatch.setenv("RDGPU_FILL_COARSE", "1")
    got = run(4, flagged, census)
    _same(got, exp, what)
    monkeypatch.delenv("RDGPU_FILL_COUNT_COARSE")
    got1 = run(4, 0, census)                                    # as shipped: no counter
    _same(got1, exp, what + ", uncounted")
    monkeypatch.setenv("RDGPU_FILL_COUNT_COARSE", "1")
    monkeypatch.setenv("RDGPU_FILL_COARSE", "0")
    _same(run(2, 0, census), got, what + ", switched off")
    monkeypatch.setenv("RDGPU_FILL_COARSE", "1")
    monkeypatch.setenv("RDGPU_FILL_FLOODED", "0")
    _same(run(2, 0, 0), got, what + ", flooded tiles switched off")
    assert np.array_equal(z.view(np.uint8), keep.view(np.uint8))
    return flagged


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", list(RASTERS))
def test_coarse_flood_equals_the_oracle_and_the_model(rd, orc, monkeypatch, capfd, name, topo):
    z, expected = RASTERS[name]
    flagged = _check(rd, orc, monkeypatch, capfd, name, z, topo)
    assert flagged == expected, (name, topo, flagged)
    if expected:
        assert flagged >= 1


@pytest.mark.parametrize("topo", [8, 4])
@pytest.mark.parametrize("name", ["thick bowl", "spill southwest", "two lakes", "ring minus zero", "many nodes", "odd width 258",
                                  "thick bowl int16"])
def test_coarse_flood_device_entry(rd, orc, monkeypatch, capfd, name, topo):
    z, expected = RASTERS[name]
    assert _check(rd, orc, monkeypatch, capfd, name, z, topo, entry="dev") == expected >= 1


@pytest.mark.parametrize("whs", [(2048, 2048, 3), (2048, 2048, 11), (1536, 1536, 3), (1030, 770, 3)], ids=lambda c: f"{c[0]}x{c[1]}s{c[2]}")
def test_coarse_flood_fractal(rd, orc, monkeypatch, capfd, whs):
    w, h, seed = whs
    flagged = _check(rd, orc, monkeypatch, capfd, f"fractal {whs}", fractal_dem(w, h, seed), 8, entry="dev")
    assert flagged == cm.FRACTALS[whs][0][CB]


def test_coarse_flood_fractal_d4(rd, orc, monkeypatch, capfd):
    assert _check(rd, orc, monkeypatch, capfd, "fractal 2048 s3", fractal_dem(2048, 2048, 3), 4, entry="dev") >= 1


def test_profile_names_and_launch_counts(rd, orc, monkeypatch):
    """the nested fill's launches appear under coarse.* only; the outer fill's are the switched-off fill's plus the two new ones"""
    import torch

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    z = fractal_dem(2048, 2048, 3)

    def profile():
        t = torch.from_numpy(z).cuda()
        rd.profile_reset()
        rd.profile_enable(True)
        try:
            rd.fill_depressions_dev(t)
            torch.cuda.synchronize()
        finally:
            rd.profile_enable(False)
        return {k: v[1] for k, v in rd.profile_totals().items()}, t.cpu().numpy()

    monkeypatch.setenv("RDGPU_FILL_COARSE", "0")
    off, w_off = profile()
    monkeypatch.setenv("RDGPU_FILL_COARSE", "1")
    on, w_on = profile()
    assert np.array_equal(w_on.view(np.uint8), w_off.view(np.uint8))
    assert not any(k.startswith("coarse.") for k in off)
    nested = {k: n for k, n in on.items() if k.startswith("coarse.")}
    assert nested and all(k.startswith("coarse.fill.") for k in nested), nested
    assert nested["coarse.fill.descent"] == 1 and nested["coarse.fill.finalize"] == 1 and "coarse.fill.flag_tiles" not in nested
    outer = {k: n for k, n in on.items() if not k.startswith("coarse.")}
    assert outer.pop("fill.pairs_flooded") == 1 and outer.pop("fill.flag_tiles") == 1
    assert outer == off, (outer, off)


def test_a_small_pair_list_takes_the_fallback(rd, orc, monkeypatch, capfd):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    z, expected = RASTERS["thick bowl"]
    monkeypatch.setenv("RDGPU_FILL_DEBUG", "1")
    monkeypatch.setenv("RDGPU_FILL_COARSE", "1")
    monkeypatch.setenv("RDGPU_FILL_EDGE_CAP", "64")
    capfd.readouterr()
    got = rd.FillDepressions(z)
    assert "pair list overflow" in capfd.readouterr().err
    _same(got, orc.port.fill(z, 8), "thick bowl, pair list of 64 records")


def test_the_other_fills_ignore_the_switch(rd, orc, monkeypatch):
    """the classic path, the shards and the fill with outlets: outputs and statistics as without the switch"""
    import torch

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    z, _ = RASTERS["thick bowl"]

    def classic():
        return rd.FillDepressions(z), rd.fill_stats()

    def shards():
        return rd.FillDepressions(z, shards=2), rd.fill_stats()

    def outlets():
        t = torch.from_numpy(z).cuda()
        o = torch.zeros(z.shape, dtype=torch.uint8, device="cuda")
        o[100, 100] = 1
        rc = rd.lib().rdgpu_fill_outlets_dev_f32(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(o.data_ptr()), z.shape[1], z.shape[0],
                                                 ctypes.c_void_p(0))
        assert rc == 0
        torch.cuda.synchronize()
        return t.cpu().numpy(), rd.fill_stats()

    for name, f, env in (("classic", classic, {"RDGPU_FILL_EDGES": "0"}), ("shards", shards, {}), ("outlets", outlets, {})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("RDGPU_FILL_COARSE", "0")
        w0, s0 = f()
        monkeypatch.setenv("RDGPU_FILL_COARSE", "1")
        monkeypatch.setenv("RDGPU_FILL_COUNT_COARSE", "1")
        w1, s1 = f()
        assert np.array_equal(w0.view(np.uint8), w1.view(np.uint8)) and s0 == s1, (name, s0, s1)
        assert rd.fill_coarse_tiles() == 0, name
        for k in list(env) + ["RDGPU_FILL_COARSE", "RDGPU_FILL_COUNT_COARSE"]:
            monkeypatch.delenv(k, raising=False)
    assert np.array_equal(classic()[0], orc.port.fill(z, 8))
