"""Golden vectors of the reference's CompleteBreaching_Lindsay2016<Topology::D8> (depressions/Lindsay2016.hpp:48-178) on the
rasters of tests/breach_cases.py.  Run in the build container only (it needs the reference tree); the tests read what it
writes.

    python tests/golden/make_golden_breach.py --ref /path/to/reference

breach_ref_wrap.cpp (beside this file: an extern "C" entry of our own over the UNMODIFIED reference header) is compiled into
a temporary directory outside the repository with the flags of oracle/Makefile.

* ref_breach.npz -- `cases`, the case names; per case <case>/out (the breached DEM, in full), <case>/shape and, for rasters of
                    at most 400 cells, <case>/dem (the input; the others are rebuilt from breach_cases.py's seeds).

Every case is checked here to stay within 40 breadth-first rings per plateau (the tie order's passes stay far under their
bound) and against the serial model of tests/breach_model.py.
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

import breach_cases as bc  # noqa: E402
import breach_model as bm  # noqa: E402
from digest import save_golden  # noqa: E402


def build_ref(ref: str) -> ctypes.CDLL:
    """the flags of oracle/Makefile; the object lives in a temporary directory outside the repository"""
    out = os.path.join(tempfile.mkdtemp(prefix="breach_ref_"), "libbreachref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fopenmp", "-DNDEBUG", "-DRICHDEM_NO_PROGRESS",
                           "-I" + os.path.join(ref, "include"), "-shared", "-fPIC",
                           os.path.join(HERE, "breach_ref_wrap.cpp"), "-o", out], stderr=subprocess.DEVNULL)
    return ctypes.CDLL(out)


def absent_value(dem):
    """a NoData value the raster does not hold"""
    for v in (-9999, 7, 77, 33, 101):
        fits = dem.dtype.kind == "f" or np.iinfo(dem.dtype).min <= v <= np.iinfo(dem.dtype).max
        if fits and not (dem == dem.dtype.type(v)).any():
            return dem.dtype.type(v)
    raise AssertionError("no absent value")


def main(ref):
    L = build_ref(ref)
    g = {"cases": np.array(list(bc.CASES))}
    ctype = {"u8": ctypes.c_uint8, "i8": ctypes.c_int8, "u16": ctypes.c_uint16, "i16": ctypes.c_int16, "u32": ctypes.c_uint32,
             "i32": ctypes.c_int32, "f32": ctypes.c_float}
    for name, make in bc.CASES.items():
        dem = np.ascontiguousarray(make())
        h, w = dem.shape
        s = bc.SUFFIX[dem.dtype.name]
        depth = bc.plateau_depth(dem)
        assert depth <= 40, (name, depth)
        out = dem.copy()
        getattr(L, "breachref_" + s)(out.ctypes.data_as(ctypes.c_void_p), w, h, ctype[s](absent_value(dem)))
        model = bm.breach_serial(dem)
        assert np.array_equal(out, model), name
        g[name + "/out"], g[name + "/shape"] = out, np.array([h, w])
        if dem.size <= 400:
            g[name + "/dem"] = dem
        print(name, dem.dtype, (h, w), "plateau depth", depth, "cells changed", int(np.count_nonzero(out != dem)), flush=True)
    path = os.path.join(HERE, "ref_breach.npz")
    save_golden(path, **g)
    assert not os.path.exists(path[:-4] + ".part1.npz"), "ref_breach.npz is one file"
    print("wrote ref_breach.npz", len(g), "arrays", os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    ref = sys.argv[sys.argv.index("--ref") + 1] if "--ref" in sys.argv else os.environ.get("RICHDEM_REFERENCE")
    if not ref:
        raise SystemExit("give the reference tree: --ref /path/to/reference (or RICHDEM_REFERENCE)")
    main(ref)
