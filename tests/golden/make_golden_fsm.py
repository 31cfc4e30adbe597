"""Golden vectors of the reference's FillSpillMerge (depressions/fill_spill_merge.hpp) on top of its
GetDepressionHierarchy<T, D8>.  Run in the build container only (it needs the reference tree); the tests read what it
writes.

    python tests/golden/make_golden_fsm.py --ref /path/to/reference

fsm_ref_wrap.cpp (beside this file: an extern "C" entry of our own over the UNMODIFIED reference headers) is compiled into
a temporary directory outside the repository with the flags of oracle/Makefile.  The border ring is labelled OCEAN,
everything else NO_DEP.

* ref_fsm.npz -- <case>/dem, <case>/seed, and per water k in 0..3 <case>/w<k>/water and <case>/w<k>/wtd (float64, the
                 DEM's shape: the water handed in and the reference's final wtd), <case>/w<k>/max_diff (the largest
                 |wtd - depth of tests/fsm_model.py| over ALL cells, measured here) and `cases`, the case names.

Inputs: five of make_golden_dephier.py's tie-free generators (asserted distinct).  Waters, each 0 on the border ring (the
reference app's own precondition: the reference leaves water standing on an ocean corner cell otherwise) and rounded to
a multiple of 2^-10, so that every sum of them is exact in any order: uniform span * 1e-4, span * 3e-3 and span * 0.05,
and span * 0.2 on 1 % of the cells, where span is the DEM's elevation range.
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
import dephier_model as dm  # noqa: E402
import fsm_model as fm  # noqa: E402
from make_golden_dephier import distinct_fractal, perm_case  # noqa: E402

OCEAN, NO_DEP = 0, 0xFFFFFFFF
SUFFIX = {np.dtype(np.int32): "i32", np.dtype(np.float32): "f32"}
CASES = {"frac_f32_40x30": lambda: distinct_fractal(40, 30, 701), "frac_f32_65x129": lambda: distinct_fractal(65, 129, 702),
         "frac_f32_300x257": lambda: distinct_fractal(300, 257, 703), "perm_i32_65x129": lambda: perm_case(np.int32, 65, 129, 704),
         "perm_i32_200x130": lambda: perm_case(np.int32, 200, 130, 705)}
SEEDS = {"frac_f32_40x30": 701, "frac_f32_65x129": 702, "frac_f32_300x257": 703, "perm_i32_65x129": 704, "perm_i32_200x130": 705}


def build_ref(ref: str) -> ctypes.CDLL:
    """the flags of oracle/Makefile; the object lives in a temporary directory outside the repository"""
    out = os.path.join(tempfile.mkdtemp(prefix="fsm_ref_"), "libfsmref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fopenmp", "-DNDEBUG", "-DRICHDEM_NO_PROGRESS",
                           "-I" + os.path.join(ref, "include"), "-shared", "-fPIC",
                           os.path.join(HERE, "fsm_ref_wrap.cpp"), "-o", out], stderr=subprocess.DEVNULL)
    return ctypes.CDLL(out)


def dyadic(v):
    """v rounded to a multiple of 2^-10, at least one unit"""
    return max(round(float(v) * 1024.0), 1) / 1024.0


def waters(dem, seed):
    span = float(dem.max()) - float(dem.min())
    out = []
    for f in (1e-4, 3e-3, 0.05):
        out.append(np.full(dem.shape, dyadic(span * f), np.float64))
    w = np.zeros(dem.size, np.float64)
    w[np.random.default_rng(seed).choice(dem.size, dem.size // 100, replace=False)] = dyadic(span * 0.2)
    out.append(w.reshape(dem.shape))
    for w in out:
        w[0, :] = w[-1, :] = w[:, 0] = w[:, -1] = 0.0
    return out


def ref_fsm(L, dem, water):
    dem = np.ascontiguousarray(dem)
    h, w = dem.shape
    label = np.full((h, w), NO_DEP, np.uint32)
    label[0, :] = label[-1, :] = label[:, 0] = label[:, -1] = OCEAN
    wtd = np.ascontiguousarray(water, dtype=np.float64).copy()
    k = getattr(L, "fsmref_" + SUFFIX[dem.dtype])(dem.ctypes.data_as(ctypes.c_void_p), w, h, label.ctypes.data_as(ctypes.c_void_p),
                                                  wtd.ctypes.data_as(ctypes.c_void_p))
    assert k >= 1
    return wtd


def main(ref):
    L = build_ref(ref)
    g = {"cases": np.array(list(CASES))}
    for name, make in CASES.items():
        dem = make()
        assert np.unique(dem).size == dem.size, "the reference needs pairwise distinct elevations"
        g[name + "/dem"], g[name + "/seed"] = dem, np.int64(SEEDS[name])
        labels, table = dm.hierarchy(dem, 8)
        for k, water in enumerate(waters(dem, SEEDS[name])):
            wtd = ref_fsm(L, dem, water)
            r = fm.fill_spill_merge(dem, labels, table, water)
            diff = float(np.abs(wtd - r["depth"]).max())
            g[f"{name}/w{k}/water"], g[f"{name}/w{k}/wtd"], g[f"{name}/w{k}/max_diff"] = water, wtd, np.float64(diff)
            print(name, "water", k, "lakes", r["lakes"], "full", r["full_lakes"], "wet cells", int(np.count_nonzero(wtd > 0)),
                  "max |wtd - model|", diff, "bit-equal" if np.array_equal(wtd, r["depth"]) else "", flush=True)
    save_golden(os.path.join(HERE, "ref_fsm.npz"), **g)
    print("wrote ref_fsm.npz", len(g), "arrays", os.path.getsize(os.path.join(HERE, "ref_fsm.npz")), "bytes", flush=True)


if __name__ == "__main__":
    ref = sys.argv[sys.argv.index("--ref") + 1] if "--ref" in sys.argv else os.environ.get("RICHDEM_REFERENCE")
    if not ref:
        raise SystemExit("give the reference tree: --ref /path/to/reference (or RICHDEM_REFERENCE)")
    main(ref)
