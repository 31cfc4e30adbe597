"""Depression breaching on the engine (csrc/breach.hip): rdgpu_breach_d8 against the compiled reference's goldens
(tests/golden/ref_breach.npz) and rdgpu_d8_breach_along against the Python model (tests/breach_model.py, pinned by
tests/test_breach_model.py): host C-ABI and `_dev` entries, every plane on every cell, inputs unchanged.  The cases are those
of tests/breach_cases.py; the direction rasters with loops, the single codes and the serpentine of 66 562 links are built
here.  Everything is equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import breach_cases as bc  # noqa: E402
import breach_model as bm  # noqa: E402
from digest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = load_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_breach.npz"))
_MODEL = {}


def model(name):
    """the model's planes of a golden case, computed once and left unchanged"""
    if name not in _MODEL:
        dem = bc.CASES[name]()
        _MODEL[name] = (dem, bm.breach(dem))
    return _MODEL[name]


def _bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, exp, what, bits=True):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape)
    diff = (_bits(got) != _bits(exp)) if bits else (got != exp)
    bad = int(diff.sum())
    print(what, "cells differing:", bad)
    assert bad == 0, (what, bad, np.argwhere(diff)[:5].tolist())


def _cuda(a):
    """the array as a CUDA tensor; None where this torch cannot hold the element type"""
    import torch

    try:
        return torch.from_numpy(a.copy()).cuda()
    except (TypeError, RuntimeError):
        return None


# ---- rdgpu_breach_d8 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bc.CASES))
def test_breach_equals_reference(rd, name):
    import torch

    dem, m = model(name)
    exp = GOLDEN[name + "/out"]
    keep = dem.copy()
    got = rd.breach_depressions(dem, want=("dirs", "path"))
    st = rd.breach_stats()
    print(name, "stats", st)
    assert np.array_equal(_bits(dem), _bits(keep))
    _same(got["out"], exp, name + " out host", bits=False)             # == the reference (a zero of either sign is a zero)
    _same(got["out"], m["out"], name + " out host against the model")  # bit for bit: -0 is written as +0
    _same(got["dirs"], m["dirs"], name + " dirs host")
    _same(got["path"], m["path"], name + " path host")
    assert st["unresolved"] == 0
    assert st["pits"] == int(m["pits"].sum()) and st["raised"] == int((m["d1"] != dem).sum())
    assert st["lowered"] == int((m["out"] < m["d1"]).sum())
    t = _cuda(dem)
    if t is not None:
        d = torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda")
        p = torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda")
        rd.breach_depressions_dev(t, dirs=d, path=p)
        _same(t.cpu().numpy(), m["out"], name + " out dev")
        _same(d.cpu().numpy(), m["dirs"], name + " dirs dev")
        _same(p.cpu().numpy(), m["path"], name + " path dev")
        assert rd.breach_stats() == st


def test_breach_output_subsets(rd):
    import torch

    name = "q_u8_130x129"
    dem, m = model(name)
    _same(rd.breach_depressions(dem), m["out"], "out alone")
    for want in (("dirs",), ("path",)):
        got = rd.breach_depressions(dem, want=want)
        assert set(got) == {"out", *want}
        _same(got["out"], m["out"], f"out with {want}")
        _same(got[want[0]], m[want[0]], want[0] + " alone")
    for want in ((), ("dirs",), ("path",)):
        t = _cuda(dem)
        buf = {k: torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda") for k in ("dirs", "path")}
        rd.breach_depressions_dev(t, **{k: buf[k] for k in want})
        _same(t.cpu().numpy(), m["out"], f"dev out with {want}")
        for k in ("dirs", "path"):
            if k in want:
                _same(buf[k].cpu().numpy(), m[k], "dev " + k)
            else:
                assert bool((buf[k] == 77).all()), k + " was not requested but written"


def test_breach_nodata_is_unsupported(rd):
    import torch

    dem, m = model("q_i16_97x70")
    absent, present = -9999, int(dem[30, 40])
    assert not (dem == absent).any()
    _same(rd.breach_depressions(dem, nodata=absent), m["out"], "a NoData value the raster does not hold")
    with pytest.raises(rd.RdgpuError) as e:
        rd.breach_depressions(dem, nodata=present, want=("dirs", "path"))
    assert e.value.code == 3
    t = _cuda(dem)
    d = torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda")
    p = torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda")
    with pytest.raises(rd.RdgpuError) as e:
        rd.breach_depressions_dev(t, nodata=present, dirs=d, path=p)
    assert e.value.code == 3
    assert np.array_equal(t.cpu().numpy(), dem) and bool((d == 77).all()) and bool((p == 77).all())


# ---- rdgpu_d8_breach_along -----------------------------------------------------------------------------------------------
def _check_along(rd, what, dirs, dem, pits, dir_nodata=255):
    exp_out, exp_path = bm.breach_along(dem, dirs, pits, dir_nodata)
    keep = (dirs.copy(), dem.copy(), pits.copy())
    got = rd.d8_breach_along(dirs, dem, pits, dir_nodata)
    _same(got["out"], exp_out, what + " out host")
    _same(got["path"], exp_path, what + " path host")
    only = rd.d8_breach_along(dirs, dem, pits, dir_nodata, want="path")
    assert set(only) == {"path"}
    _same(only["path"], exp_path, what + " path alone")
    assert np.array_equal(dirs, keep[0]) and np.array_equal(_bits(dem), _bits(keep[1])) and np.array_equal(pits, keep[2])
    t = _cuda(dem)
    if t is not None:
        import torch

        td, tp = _cuda(dirs), _cuda(pits)
        out = torch.from_numpy(np.full(dem.shape, 77, dem.dtype)).cuda()
        path = torch.full(dem.shape, 77, dtype=torch.uint8, device="cuda")
        rd.d8_breach_along_dev(td, t, tp, out=out, dir_nodata=dir_nodata)
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), exp_out, what + " out dev, alone")
        assert bool((path == 77).all())
        rd.d8_breach_along_dev(td, t, tp, out=out, path=path, dir_nodata=dir_nodata)
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), exp_out, what + " out dev")
        _same(path.cpu().numpy(), exp_path, what + " path dev")
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(dem)) and np.array_equal(td.cpu().numpy(), dirs)
    return exp_out, exp_path


@pytest.mark.parametrize("name", [n for n in bc.CASES if min(bc.CASES[n]().shape) >= 3])
def test_along_on_the_goldens_trees(rd, name):
    dem, m = model(name)
    out, path = _check_along(rd, name, m["dirs"], m["d1"], m["pits"])
    _same(out, m["out"], name + ": the model's closure is the breach")


def _ring(dirs, y0, x0, y1, x1):
    """a clockwise direction loop round the rectangle"""
    dirs[y0, x0:x1] = 5
    dirs[y0:y1, x1] = 7
    dirs[y1, x0 + 1:x1 + 1] = 1
    dirs[y0 + 1:y1 + 1, x0] = 3


LOOPS = {"tile": (10, 10, 11, 11), "edge": (20, 62, 21, 65), "corner": (63, 63, 64, 64)}


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.uint32, np.uint8])
@pytest.mark.parametrize("where", list(LOOPS))
def test_along_random_directions_with_loops(rd, where, dtype):
    rng = np.random.default_rng(200 + list(LOOPS).index(where))
    h, w = 130, 131
    dirs = rng.integers(0, 9, (h, w)).astype(np.uint8)
    dirs[rng.random((h, w)) < 0.03] = 255
    dem = rng.integers(0, 6, (h, w)).astype(dtype)
    if dtype == np.uint32:
        dem = dem + np.uint32(0xFFFFFFFA)                       # up to the type's maximum: the 64-bit words
    if dtype == np.float32:
        dem[rng.random((h, w)) < 0.02] = np.nan
        dem[rng.random((h, w)) < 0.02] = -0.0
    pits = (rng.random((h, w)) < 0.1).astype(np.uint8)
    y0, x0, y1, x1 = LOOPS[where]
    for variant in ("pit on the loop", "pit on a feeder"):
        d, z, p = dirs.copy(), dem.copy(), pits.copy()
        _ring(d, y0, x0, y1, x1)
        base = z[0, 0] * 0 + (dem[~np.isnan(dem.astype(np.float64))].min())
        z[y0:y1 + 1, x0:x1 + 1] = base + 3
        p[y0:y1 + 1, x0 - 3:x1 + 1] = 0
        d[y0, x0 - 3:x0] = 5                                     # a feeder into the loop from the west
        z[y0, x0 - 3:x0] = base + 4
        if variant == "pit on the loop":
            p[y1, x1] = 1
        else:
            p[y0, x0 - 3] = 1
            z[y0, x0 - 3] = base + 2
        out, path = _check_along(rd, f"{where} {np.dtype(dtype).name} {variant}", d, z, p)
        assert path[y0:y1 + 1, x0:x1 + 1].all()                  # the level goes all the way round
        if variant == "pit on a feeder":
            assert (out[y0:y1 + 1, x0:x1 + 1] == base + 2).all() and (out[y0, x0 - 3:x0] == base + 2).all()


@pytest.mark.parametrize("code", range(1, 9))
def test_along_single_code(rd, code):
    rng = np.random.default_rng(300 + code)
    dirs = np.full((130, 130), code, np.uint8)
    dem = rng.integers(0, 4, (130, 130)).astype(np.int8)
    pits = (rng.random((130, 130)) < 0.1).astype(np.uint8)
    _check_along(rd, f"code {code}", dirs, dem, pits)


def test_along_serpentine_past_16_bits(rd):
    """one chain through all 66 563 cells of 257 x 259: more links than a tile holds cells and than 16 bits count; a cell
    below the pit two thirds of the way stops the walk, a second pit goes on from there"""
    h, w = 259, 257
    dirs = np.zeros((h, w), np.uint8)
    dirs[0::2, :] = 5
    dirs[1::2, :] = 1
    dirs[0::2, w - 1] = 7
    dirs[1::2, 0] = 7
    dirs[h - 1, w - 1 if (h - 1) % 2 == 0 else 0] = 0
    order = np.arange(h * w).reshape(h, w)
    order[1::2] = order[1::2, ::-1]                              # position along the chain
    dem = (10 + order % 7).astype(np.int32)
    pits = np.zeros((h, w), np.uint8)
    pits.ravel()[np.argmin(order)] = 1
    dem.ravel()[np.argmin(order)] = 5
    stop = np.flatnonzero(order.ravel() == 2 * h * w // 3)[0]
    dem.ravel()[stop] = 1
    out, path = _check_along(rd, "serpentine, one walk", dirs, dem, pits)
    assert int(path.sum()) == 2 * h * w // 3 > 4095 * 10 and (out[path == 1] == 5).all()
    dem.ravel()[stop] = 9
    out, path = _check_along(rd, "serpentine, to the end", dirs, dem, pits)
    assert int(path.sum()) == h * w > 65535 and (out == 5).all()
    pits.ravel()[stop] = 1
    dem.ravel()[stop] = 2
    out, path = _check_along(rd, "serpentine, two pits", dirs, dem, pits)
    assert int((out == 2).sum()) == h * w - 2 * h * w // 3 and int((out == 5).sum()) == 2 * h * w // 3


# ---- invariants at 2000 x 2000 -------------------------------------------------------------------------------------------
def test_breach_invariants_2000(rd):
    import torch
    import torch.nn.functional as F

    n = 2000
    z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(z, 77)
    inf = float("inf")

    def shifted(a, k, fill):
        """a's value at every cell's neighbour k"""
        p = F.pad(a[None, None].float() if a.dtype != torch.float32 else a[None, None], (1, 1, 1, 1), value=fill)[0, 0]
        return p[1 + bm.DY[k]:n + 1 + bm.DY[k], 1 + bm.DX[k]:n + 1 + bm.DX[k]]

    interior = torch.zeros((n, n), dtype=torch.bool, device="cuda")
    interior[1:-1, 1:-1] = True
    top = torch.finfo(torch.float32).max
    lo = torch.full_like(z, top)
    for k in range(1, 9):
        lo = torch.minimum(lo, shifted(z, k, inf))
    d1 = torch.where(interior & (z < lo), lo, z)
    lo2 = torch.full_like(z, top)
    for k in range(1, 9):
        before = bm.DY[k] < 0 or (bm.DY[k] == 0 and bm.DX[k] < 0)
        lo2 = torch.minimum(lo2, shifted(d1 if before else z, k, inf))
    pit = interior & (z <= lo2)
    out = z.clone()
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    path = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.breach_depressions_dev(out, dirs=dirs, path=path)
    st = rd.breach_stats()
    print("2000 x 2000 stats", st)
    assert st["unresolved"] == 0 and st["pits"] == int(pit.sum())
    best = torch.where(pit, d1, torch.full_like(d1, inf))
    for k in range(1, 9):                                          # the children: neighbours whose direction points back
        child = (shifted(dirs, k, 0) == bm.INV[k]) & (shifted(path, k, 0) == 1)
        ok = shifted(out, k, inf)
        best = torch.minimum(best, torch.where(child & (ok <= d1), ok, torch.full_like(d1, inf)))
    assert bool(((path == 1) == (best < inf)).all())
    assert bool((out == torch.where(best < inf, best, d1)).all())
    assert bool((out <= d1).all())
    assert not rd.has_depressions(out.cpu().numpy())
