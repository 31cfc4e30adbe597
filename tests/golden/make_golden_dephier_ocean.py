"""Golden vectors of the reference's GetDepressionHierarchy, FillSpillMerge and BucketFillFromEdges for a CALLER-GIVEN
OCEAN: a label raster in which any set of cells is OCEAN.  Run in the build container only (it needs the reference tree);
the tests read what it writes.

    python tests/golden/make_golden_dephier_ocean.py --ref /path/to/reference

dephier_ref_wrap.cpp, fsm_ref_wrap.cpp and bucketfill_ref_wrap.cpp (beside this file: extern "C" entries of our own over
the UNMODIFIED reference headers) are compiled into a temporary directory outside the repository with the flags of
oracle/Makefile.  The cells of the mask are labelled OCEAN, everything else NO_DEP.

* ref_dephier_ocean.npz -- `cases` (names <raster>/<mask kind>), `fsm_cases`, and
    <raster>/dem, <raster>/seed
    <raster>/<kind>/mask (uint8) and per topology t in (8, 4) <raster>/<kind>/t<t>/labels, /u32, /f64: the rows of
        make_golden_dephier.py
    <raster>/<kind>/w<k>/water, /wtd (fsm_cases only, k in 0..3): the water handed in (0 on ocean cells, as the
        reference app does) and the reference's final wtd, D8
    <raster>/bucket/check (uint8: 1 below the raster's 25 % quantile), and per t <raster>/bucket/t<t>/mask: the
        reference's BucketFillFromEdges of check == 1 into an empty mask (the `bucket` mask kind is the D8 one)
    <raster>/bucket_wall/t<t>/mask_in, /mask: the same with a pre-set wall (row h // 2 and column w // 3)

Mask kinds: ring (the border ring), quantile (every cell below the 25 % quantile, anywhere), bucket (the bucket fill of
that set from the edges), onecell (ONE interior cell, no ring), ringhole (the ring and an interior 20 x 15 hole; 8 x 6 on
the 40 x 30 raster), scatter (2 % random cells, no ring), nodata (a hole of equal values -- -9999, 65535 for u16 -- marked
ocean, and the left column only).

Inputs: make_golden_dephier.py's tie-free generators; the seed of a raster is the first one for which the share of
internal nodes that ties dissolve in the canonical form stays below 5 % for EVERY mask kind, both topologies and both
trees (the reference's and the model's).  FSM cases use the quantile, onecell and ringhole masks only: on a scattered mask
one run of 32 differed in one leaf (unexplained); every stored combination is asserted bit-equal
between the reference and tests/fsm_model.py on the model's masked hierarchy.
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
import dephier_ocean_model as om  # noqa: E402
import fsm_model as fm  # noqa: E402
from make_golden_dephier import SUFFIX, distinct_fractal, perm_case, to_contract  # noqa: E402
from make_golden_fsm import waters  # noqa: E402

OCEAN, NO_DEP = 0, 0xFFFFFFFF
KINDS = ("ring", "quantile", "bucket", "onecell", "ringhole", "scatter", "nodata")
FSM_KINDS = ("quantile", "onecell", "ringhole")
RASTERS = {"perm_u16_40x30": lambda s: perm_case(np.uint16, 40, 30, s), "perm_i32_65x129": lambda s: perm_case(np.int32, 65, 129, s),
           "frac_f32_65x129": lambda s: distinct_fractal(65, 129, s), "frac_f32_200x130": lambda s: distinct_fractal(200, 130, s)}
FSM_RASTERS = ("perm_i32_65x129", "frac_f32_200x130")


def build(ref: str, src: str) -> ctypes.CDLL:
    """the flags of oracle/Makefile; the object lives in a temporary directory outside the repository"""
    out = os.path.join(tempfile.mkdtemp(prefix="ocean_ref_"), "lib" + src[:-4] + ".so")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fopenmp", "-DNDEBUG", "-DRICHDEM_NO_PROGRESS",
                           "-I" + os.path.join(ref, "include"), "-shared", "-fPIC", os.path.join(HERE, src), "-o", out],
                          stderr=subprocess.DEVNULL)
    return ctypes.CDLL(out)


def ref_bucket(LB, check, value, mask, topology):
    check = np.ascontiguousarray(check)
    out = np.ascontiguousarray(mask, dtype=np.uint8).copy()
    h, w = check.shape
    suf = "u8" if check.dtype == np.uint8 else SUFFIX[check.dtype]
    fn = getattr(LB, "bfref_" + suf)
    fn.restype = ctypes.c_long
    ct = {"u8": ctypes.c_uint8, "u16": ctypes.c_uint16, "i32": ctypes.c_int32, "f32": ctypes.c_float}[suf]
    fn(check.ctypes.data_as(ctypes.c_void_p), w, h, topology, ct(value), out.ctypes.data_as(ctypes.c_void_p))
    return out


def ref_hierarchy(LD, dem, mask, topology):
    dem = np.ascontiguousarray(dem)
    h, w = dem.shape
    label = np.where(mask != 0, OCEAN, NO_DEP).astype(np.uint32)
    cap = 2 * h * w + 2
    u = np.zeros((cap, 7), np.uint32)
    f = np.zeros((cap, 3), np.float64)
    k = getattr(LD, "dhref_" + SUFFIX[dem.dtype])(dem.ctypes.data_as(ctypes.c_void_p), w, h, topology,
                                                  label.ctypes.data_as(ctypes.c_void_p), cap,
                                                  u.ctypes.data_as(ctypes.c_void_p), f.ctypes.data_as(ctypes.c_void_p))
    assert k >= 1
    return label, u[:k].copy(), f[:k].copy()


def ref_fsm(LF, dem, mask, water):
    dem = np.ascontiguousarray(dem)
    h, w = dem.shape
    label = np.where(mask != 0, OCEAN, NO_DEP).astype(np.uint32)
    wtd = np.ascontiguousarray(water, dtype=np.float64).copy()
    k = getattr(LF, "fsmref_" + SUFFIX[dem.dtype])(dem.ctypes.data_as(ctypes.c_void_p), w, h, label.ctypes.data_as(ctypes.c_void_p),
                                                   wtd.ctypes.data_as(ctypes.c_void_p))
    assert k >= 1
    return wtd


def sea_check(dem):
    """uint8: 1 on the cells below the raster's 25 % quantile"""
    q = np.sort(dem.ravel())[dem.size // 4]
    return (dem < q).astype(np.uint8)


def masks_of(LB, dem, seed):
    """kind -> (dem for that kind, mask): the nodata kind changes the DEM (a hole of equal values)"""
    h, w = dem.shape
    sea = sea_check(dem)
    ring = om.ring_mask(dem.shape)
    out = {"ring": (dem, ring), "quantile": (dem, sea.copy()),
           "bucket": (dem, ref_bucket(LB, sea, 1, np.zeros_like(sea), 8))}
    one = np.zeros_like(ring)
    one[h // 2, w // 2] = 1
    out["onecell"] = (dem, one)
    hw, hh = (20, 15) if w >= 60 else (8, 6)
    y0, x0 = h // 3, w // 4
    hole = ring.copy()
    hole[y0:y0 + hh, x0:x0 + hw] = 1
    out["ringhole"] = (dem, hole)
    sc = np.zeros(dem.size, np.uint8)
    sc[np.random.default_rng(seed + 7).choice(dem.size, max(dem.size // 50, 1), replace=False)] = 1
    out["scatter"] = (dem, sc.reshape(h, w))
    nd = np.zeros_like(ring)
    nd[y0:y0 + hh, x0:x0 + hw] = 1
    holed = dem.copy()
    holed[nd != 0] = 65535 if dem.dtype == np.uint16 else -9999
    nd[:, 0] = 1
    out["nodata"] = (holed, nd)
    assert tuple(out) == KINDS
    return out


def tie_shares(LD, dem, mask):
    out, refs = [], {}
    for t in (8, 4):
        label, u, f = refs[t] = ref_hierarchy(LD, dem, mask, t)
        r = to_contract(label, u, f)
        _, tab = om.hierarchy(dem, t, mask)
        for par, lc, rc, pit, lvl, cells, vol in ((r["parent"], r["lchild"], r["rchild"], r["pit_cell"], r["level"], r["cells"], r["volume"]),
                                                  tuple(tab[k] for k in ("parent", "lchild", "rchild", "pit_cell", "level", "cells", "volume"))):
            _, dissolved = dm.canonical(par, lc, rc, pit, lvl, cells, vol)
            out.append((dissolved, int(np.count_nonzero(np.asarray(lc) != dm.NONE))))
    return out, refs


def main(ref):
    LD, LF, LB = build(ref, "dephier_ref_wrap.cpp"), build(ref, "fsm_ref_wrap.cpp"), build(ref, "bucketfill_ref_wrap.cpp")
    g, cases, fsm_cases = {}, [], []
    for k, (name, make) in enumerate(RASTERS.items()):
        for seed in range(1000 * (k + 1), 1000 * (k + 1) + 200):
            dem = make(seed)
            assert np.unique(dem).size == dem.size, "the reference needs pairwise distinct elevations"
            found, ok = {}, True
            for kind, (d, mask) in masks_of(LB, dem, seed).items():
                shares, refs = tie_shares(LD, d, mask)
                if not all(x < 0.05 * max(i, 1) for x, i in shares):
                    ok = False
                    break
                found[kind] = (d, mask, refs, shares)
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed below the cap on ties")
        g[name + "/dem"], g[name + "/seed"] = dem, np.int64(seed)
        for kind, (d, mask, refs, shares) in found.items():
            cases.append(f"{name}/{kind}")
            g[f"{name}/{kind}/mask"] = mask
            for t in (8, 4):
                g[f"{name}/{kind}/t{t}/labels"], g[f"{name}/{kind}/t{t}/u32"], g[f"{name}/{kind}/t{t}/f64"] = refs[t]
            print(name, kind, "seed", seed, "ocean cells", int(mask.sum()), "depressions", [len(refs[t][1]) - 1 for t in (8, 4)],
                  "(dissolved, internal)", shares, flush=True)
        # the bucket fill itself, both topologies, into an empty mask and against a pre-set wall
        sea = sea_check(dem)
        g[name + "/bucket/check"] = sea
        wall = np.zeros_like(sea)
        wall[dem.shape[0] // 2, :] = 1
        wall[:, dem.shape[1] // 3] = 1
        for t in (8, 4):
            g[f"{name}/bucket/t{t}/mask"] = ref_bucket(LB, sea, 1, np.zeros_like(sea), t)
            g[f"{name}/bucket_wall/t{t}/mask_in"], g[f"{name}/bucket_wall/t{t}/mask"] = wall, ref_bucket(LB, sea, 1, wall, t)
        if name in FSM_RASTERS:
            for kind in FSM_KINDS:
                d, mask = found[kind][0], found[kind][1]
                labels, table = om.hierarchy(d, 8, mask)
                fsm_cases.append(f"{name}/{kind}")
                for j, water in enumerate(waters(d, seed)):
                    water = np.where(mask != 0, 0.0, water)
                    wtd = ref_fsm(LF, d, mask, water)
                    r = fm.fill_spill_merge(d, labels, table, water)
                    assert np.array_equal(wtd, r["depth"]), (name, kind, j, float(np.abs(wtd - r["depth"]).max()))
                    g[f"{name}/{kind}/w{j}/water"], g[f"{name}/{kind}/w{j}/wtd"] = water, wtd
                    print(name, kind, "water", j, "lakes", r["lakes"], "full", r["full_lakes"], "bit-equal", flush=True)
    g["cases"], g["fsm_cases"] = np.array(cases), np.array(fsm_cases)
    path = os.path.join(HERE, "ref_dephier_ocean.npz")
    save_golden(path, **g)
    print("wrote ref_dephier_ocean.npz", len(g), "arrays", os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    ref = sys.argv[sys.argv.index("--ref") + 1] if "--ref" in sys.argv else os.environ.get("RICHDEM_REFERENCE")
    if not ref:
        raise SystemExit("give the reference tree: --ref /path/to/reference (or RICHDEM_REFERENCE)")
    main(ref)
