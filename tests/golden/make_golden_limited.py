"""Golden vectors of the reference's MoveWaterIntoPits (depressions/fill_spill_merge.hpp:226-318), the descent that
saturates cells on the way down, on the flow directions of its GetDepressionHierarchy<T, D8>.  Run in the build container
only (it needs the reference tree); the tests read what it writes.

    python tests/golden/make_golden_limited.py --ref /path/to/reference

limited_ref_wrap.cpp (beside this file: an extern "C" entry of our own over the UNMODIFIED reference headers) is compiled
into a temporary directory outside the repository with the flags of oracle/Makefile.  The border ring is labelled OCEAN,
everything else NO_DEP.

* ref_limited.npz -- `cases`, the case names; per case <case>/flowdirs (int8: the reference's), <case>/label (uint32) and,
                     per water table k in 0..3, <case>/w<k>/before (int16: wtd in units of 2^-10), <case>/w<k>/after
                     (float64: the reference's wtd after the descent) and <case>/w<k>/water_vol (float64, one per
                     depression, the ocean's first).

Inputs: five of make_golden_dephier.py's tie-free generators (asserted distinct).  Water tables, multiples of 2^-10 of at
most 16 in magnitude, so that every sum of them is exact in any order: all positive; all <= 0; mixed sparse (nine cells in
ten 0); mixed dense.  The border ring is not treated specially, but cell (0, 0) is: the reference compares the ADDRESS of
the downstream neighbour with NO_FLOW (fill_spill_merge.hpp:282-292, both 0), so a cell that flows into raster index 0 is
taken for a pit and cell 0 itself is never released and keeps its water.  Every table is <= 0 at cell 0, where standing
or not makes no difference, and the tests cut the links into cell 0 before they run the model: there the two coincide.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from digest import save_golden  # noqa: E402
from make_golden_dephier import distinct_fractal, perm_case  # noqa: E402

OCEAN, NO_DEP = 0, 0xFFFFFFFF
SUFFIX = {np.dtype(np.int32): "i32", np.dtype(np.float32): "f32"}
CASES = {"frac_f32_40x30": lambda: distinct_fractal(40, 30, 701), "frac_f32_65x129": lambda: distinct_fractal(65, 129, 702),
         "frac_f32_129x65": lambda: distinct_fractal(129, 65, 706), "perm_i32_65x129": lambda: perm_case(np.int32, 65, 129, 704),
         "perm_i32_200x130": lambda: perm_case(np.int32, 200, 130, 705)}
SEEDS = {"frac_f32_40x30": 701, "frac_f32_65x129": 702, "frac_f32_129x65": 706, "perm_i32_65x129": 704, "perm_i32_200x130": 705}
UNIT = 1024
MAXK = 16 * UNIT        # |wtd| <= 16


def build_ref(ref: str) -> ctypes.CDLL:
    """the flags of oracle/Makefile; the object lives in a temporary directory outside the repository"""
    out = os.path.join(tempfile.mkdtemp(prefix="limited_ref_"), "liblimref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fopenmp", "-DNDEBUG", "-DRICHDEM_NO_PROGRESS",
                           "-I" + os.path.join(ref, "include"), "-shared", "-fPIC",
                           os.path.join(HERE, "limited_ref_wrap.cpp"), "-o", out], stderr=subprocess.DEVNULL)
    return ctypes.CDLL(out)


def water_tables(shape, seed):
    """int16 [4, h, w], in units of 2^-10"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(1, MAXK + 1, shape)
    neg = -rng.integers(0, MAXK + 1, shape)
    dense = rng.integers(-MAXK, MAXK + 1, shape)
    sparse = np.where(rng.random(shape) < 0.1, rng.integers(-MAXK, MAXK + 1, shape), 0)
    t = np.stack([pos, neg, sparse, dense]).astype(np.int16)
    t[:, 0, 0] = -np.abs(t[:, 0, 0])                 # (see the module's docstring)
    return t


def main(ref):
    L = build_ref(ref)
    g = {"cases": np.array(list(CASES))}
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for name, make in CASES.items():
        dem = np.ascontiguousarray(make())
        assert np.unique(dem).size == dem.size, "the reference needs pairwise distinct elevations"
        h, w = dem.shape
        label = np.full((h, w), NO_DEP, np.uint32)
        label[0, :] = label[-1, :] = label[:, 0] = label[:, -1] = OCEAN
        dirs = np.zeros((h, w), np.int8)
        before = water_tables((h, w), SEEDS[name])
        wtd = before.astype(np.float64) / UNIT
        stride = h * w + 1
        vol = np.zeros((4, stride), np.float64)
        n = getattr(L, "limref_" + SUFFIX[dem.dtype])(p(dem), w, h, p(label), p(dirs), p(wtd), 4, p(vol), stride)
        assert 1 <= n <= stride
        assert dirs.min() >= 0 and dirs.max() <= 8 and label.max() < n
        g[name + "/flowdirs"], g[name + "/label"] = dirs, label
        for k in range(4):
            assert (wtd[k] <= 0).all()
            g[f"{name}/w{k}/before"], g[f"{name}/w{k}/after"], g[f"{name}/w{k}/water_vol"] = before[k], wtd[k], vol[k, :n].copy()
            print(name, "table", k, "depressions", n, "cells with a deficit left", int(np.count_nonzero(wtd[k] < 0)), "water in pits",
                  float(vol[k, :n].sum()), "in the ocean", float(vol[k, 0]), flush=True)
    path = os.path.join(HERE, "ref_limited.npz")
    save_golden(path, **g)
    assert not os.path.exists(path[:-4] + ".part1.npz"), "ref_limited.npz is one file"
    print("wrote ref_limited.npz", len(g), "arrays", os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    ref = sys.argv[sys.argv.index("--ref") + 1] if "--ref" in sys.argv else os.environ.get("RICHDEM_REFERENCE")
    if not ref:
        raise SystemExit("give the reference tree: --ref /path/to/reference (or RICHDEM_REFERENCE)")
    main(ref)
