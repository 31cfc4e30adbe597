"""Golden vectors of the reference's d8_upslope_cells (methods/d8_methods.hpp:144-236).  Run in the build container only
(it needs the reference tree); the tests read what it writes.

    python tests/golden/make_golden_upslope.py [--small] [--s2] --ref /path/to/reference

upslope_ref_wrap.cpp (beside this file: an extern "C" entry of our own over the UNMODIFIED reference header) is compiled
into a temporary directory outside the repository with the flags of oracle/Makefile.

* ref_upslope.npz     -- (--small) small cases, inputs beside outputs: <case>/dirs, <case>/nodata, <case>/lines (k x 4:
                         x0 y0 x1 y1) and <case>/up<i>, the reference's raster of line i.  See small_cases().  Only lines
                         for which the reference stays inside the raster: asserted with the line model
                         (tests/upslope_model.py) BEFORE the reference is called, so no golden rests on undefined behaviour.
* ref_s2_upslope.npz  -- (--s2) 10000 x 10000 G(seed=3), the reference's fill -> barnes_flat_resolution_d8 directions:
                         upslope cells of (i) the single cell with the largest d8_flow_accum and (ii) one long shallow line,
                         as band digests of the whole output (digest.py) with the count of 1-cells and the reference's
                         wall time.
"""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from digest import BAND_ROWS, band_digests_np, save_golden  # noqa: E402
from richdem_amd.synth import fractal_dem  # noqa: E402
import upslope_model as um  # noqa: E402


def build_ref(ref: str) -> ctypes.CDLL:
    """the flags of oracle/Makefile; the object lives in a temporary directory outside the repository"""
    out = os.path.join(tempfile.mkdtemp(prefix="upslope_ref_"), "liburef.so")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fopenmp", "-DNDEBUG", "-DRICHDEM_NO_PROGRESS",
                           "-I" + os.path.join(ref, "include"), "-shared", "-fPIC",
                           os.path.join(HERE, "upslope_ref_wrap.cpp"), "-o", out], stderr=subprocess.DEVNULL)
    return ctypes.CDLL(out)


def ref_upslope(L, dirs, nodata, x0, y0, x1, y1):
    dirs = np.ascontiguousarray(dirs, np.uint8)
    h, w = dirs.shape
    assert um.line((h, w), x0, y0, x1, y1) is not None, ("the reference would leave the raster", (w, h), (x0, y0, x1, y1))
    out = np.empty((h, w), np.uint8)
    nd = L.uref_d8_upslope_cells(dirs.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint8(nodata), w, h, int(x0), int(y0), int(x1),
                                 int(y1), out.ctypes.data_as(ctypes.c_void_p))
    assert nd == 255
    return out


def lines_for(h, w, rng):
    """a single point, a horizontal run, slopes below and above 1 in both signs, swapped end points, x0 == x1 with
    y0 != y1 -- those of them the reference keeps inside a raster of this shape"""
    xm, ym = w // 2, h // 2
    cand = [(xm, ym, xm, ym), (0, 0, 0, 0), (w - 1, h - 1, w - 1, h - 1),
            (0, ym, w - 1, ym), (w - 1, ym, 0, ym),                               # horizontal, and swapped
            (1, 1, w - 2, 1 + (h - 2) // 3), (1, h - 2, w - 2, h - 2 - (h - 2) // 3),   # shallow, both signs
            (w - 2, 1 + (h - 2) // 3, 1, 1),                                      # shallow, swapped
            (1, 0, min(w - 2, 1 + h // 4), h - 1), (1, h - 1, min(w - 2, 1 + h // 4), 0),   # steep, both signs
            (xm - 1 if xm else 0, 1 if h > 1 else 0, xm - 1 if xm else 0, h - 1),  # x0 == x1, y0 != y1
            (0, 0, w - 2, h - 1), (0, h - 1, w - 2, 0)]                           # about the diagonal
    for _ in range(3):
        cand.append(tuple(int(v) for v in (rng.integers(0, w), rng.integers(0, h), rng.integers(0, w), rng.integers(0, h))))
    out = []
    for c in cand:
        if um.line((h, w), *c) is not None and c not in out:
            out.append(c)
    return out


def small_cases(ref: str):
    """name -> (dirs uint8, nodata)"""
    import oracle
    oracle.build()
    R = oracle.ref
    assert R.available
    c = {}
    for f in sorted(glob.glob(f"{ref}/tests/flow_accum/*.d8")):              # the reference's own direction fixtures
        dirs, nd = oracle.read_ascii_grid(f, np.int32)
        c["fa_" + os.path.basename(f)[:-3]] = (dirs.astype(np.uint8), int(nd) & 0xFF)
    assert len(c) == 24
    rng = np.random.default_rng(41)
    for k, (w, h) in enumerate(((64, 64), (65, 129), (200, 130), (1, 37), (37, 1), (300, 257))):
        z = fractal_dem(w, h, 50 + k)
        c[f"frac_{w}x{h}"] = (R.flat_resolution(R.fill(z, 8), np.float32(-9999.0)), 255)
        zh = z.copy()                                                          # the same with NoData holes
        for _ in range(4):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            zh[y:y + 1 + h // 9, x:x + 1 + w // 9] = -9999.0
        c[f"holes_{w}x{h}"] = (R.flat_resolution(R.fill(zh, 8), np.float32(-9999.0)), 255)
    # hand-made: a direction loop inside one tile, a loop across a tile edge, NO_FLOW and NoData cells under the lines
    base = R.flat_resolution(R.fill(fractal_dem(140, 100, 60), 8), np.float32(-9999.0))
    lp = base.copy()
    lp[20, 20], lp[20, 21], lp[21, 21], lp[21, 20] = 5, 7, 1, 3              # E, S, W, N: a loop in tile (0, 0)
    c["loop_in_tile"] = (lp, 255)
    lp = base.copy()
    lp[50, 63], lp[50, 64], lp[51, 64], lp[51, 63] = 5, 7, 1, 3              # the same across columns 63 | 64
    lp[63, 30], lp[64, 30] = 7, 3                                            # a two-cell loop across rows 63 | 64
    c["loop_across_tiles"] = (lp, 255)
    nf = base.copy()
    nf[50, 10:130:7] = 0                                                      # NO_FLOW cells and a NoData run on row 50
    nf[50, 60:70] = 255
    nf[30:40, 100] = 255
    c["noflow_nodata"] = (nf, 255)
    return c


def small(L, ref):
    g = {}
    rng = np.random.default_rng(42)
    nlines = 0
    for name, (dirs, nodata) in small_cases(ref).items():
        h, w = dirs.shape
        lines = lines_for(h, w, rng)
        if name == "loop_in_tile":
            lines += [(20, 20, 20, 20), (18, 20, 24, 20)]                      # a seed on the loop; a line through it
        if name == "loop_across_tiles":
            lines += [(64, 50, 64, 50), (30, 63, 30, 63), (60, 51, 66, 51)]
        if name == "noflow_nodata":
            lines += [(5, 50, 135, 50), (100, 35, 100, 35)]                    # a line over NoData and NO_FLOW cells
        g[name + "/dirs"] = dirs
        g[name + "/nodata"] = np.uint8(nodata)
        g[name + "/lines"] = np.array(lines, np.int32).reshape(-1, 4)
        for i, ln in enumerate(lines):
            g[f"{name}/up{i}"] = ref_upslope(L, dirs, nodata, *ln)
        nlines += len(lines)
    save_golden(os.path.join(HERE, "ref_upslope.npz"), **g)
    print("wrote ref_upslope.npz", len(g), "arrays", nlines, "lines", flush=True)


def big_dem(n, seed):
    z = np.empty((n, n), np.float32)
    for y0 in range(0, n, 2000):
        z[y0:y0 + 2000] = fractal_dem(n, min(2000, n - y0), seed, y0=y0)
    return z


def s2(L, n=10000, seed=3):
    import oracle
    oracle.build()
    R = oracle.ref
    assert R.available
    z = big_dem(n, seed)
    dirs = R.flat_resolution(R.fill(z, 8), np.float32(-9999.0))
    del z
    acc = R.d8_flow_accum(dirs, 255, np.float64)
    my, mx = (int(v) for v in np.unravel_index(int(np.argmax(acc)), acc.shape))
    g = {"size": np.int64(n), "seed": np.int64(seed), "band_rows": np.int64(BAND_ROWS), "dirs": band_digests_np(dirs),
         "mouth": np.array([mx, my], np.int64), "mouth_accum": np.float64(acc[my, mx]),
         "line": np.array([n // 10, n // 2 - n // 20, n - n // 10, n // 2 + n // 20], np.int64)}
    del acc
    for tag, ln in (("mouth", (mx, my, mx, my)), ("line", tuple(int(v) for v in g["line"]))):
        t0 = time.perf_counter()
        up = ref_upslope(L, dirs, 255, *ln)
        g["ref_seconds/" + tag] = np.float64(round(time.perf_counter() - t0, 3))
        g["up_" + tag] = band_digests_np(up)
        g["ones_" + tag] = np.int64((up == 1).sum())
        g["twos_" + tag] = np.int64((up == 2).sum())
        print(tag, ln, float(g["ref_seconds/" + tag]), int(g["ones_" + tag]), flush=True)
    save_golden(os.path.join(HERE, "ref_s2_upslope.npz"), **g)
    print("wrote ref_s2_upslope.npz", flush=True)


if __name__ == "__main__":
    ref = sys.argv[sys.argv.index("--ref") + 1] if "--ref" in sys.argv else os.environ.get("RICHDEM_REFERENCE")
    if not ref:
        raise SystemExit("give the reference tree: --ref /path/to/reference (or RICHDEM_REFERENCE)")
    lib = build_ref(ref)
    todo = [a for a in ("--small", "--s2") if a in sys.argv] or ["--small"]
    if "--small" in todo:
        small(lib, ref)
    if "--s2" in todo:
        s2(lib)
