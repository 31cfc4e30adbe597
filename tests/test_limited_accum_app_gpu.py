"""apps/rd_d8_limited_accumulation on native raster files: its outputs and the sums it prints equal the Python entry's, with
and without the optional rasters, for float32 and float64."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_limited_accum_shim_gpu import limited_case  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "rd_d8_limited_accumulation")
KEYS = ("supplied", "left", "kept_pos", "kept_neg")


def run(*args):
    if not os.path.exists(APP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "apps"), "rd_d8_limited_accumulation"], check=True, capture_output=True)
    return subprocess.run([APP, *map(str, args)], capture_output=True, text=True, timeout=300)


def sums(r):
    lines = dict(line.split() for line in r.stdout.strip().splitlines())
    return {k: float(lines[k]) for k in KEYS}


def test_rd_d8_limited_accumulation_app_equals_the_python_layer(rd, tmp_path):
    dirs, supply, cap, fac = limited_case(rd, 11)
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    d, s, c, f, o, k = (str(tmp_path / n) for n in ("dirs", "supply", "cap", "fac", "out", "kept"))
    rd.SaveNative(d, rd.rdarray(dirs, no_data=255, geotransform=gt))
    rd.SaveNative(s, rd.rdarray(supply, no_data=-9999, geotransform=gt))
    rd.SaveNative(c, rd.rdarray(cap, no_data=-9999))
    rd.SaveNative(f, rd.rdarray(fac, no_data=-9999))
    r = run(d, s, c, f, o, k)
    assert r.returncode == 0, r.stdout + r.stderr
    exp = rd.d8_flow_accum_limited(dirs, supply, -9999.0, cap, fac)
    for name, key in ((o, "out"), (k, "kept")):
        got = rd.LoadNative(name, np.float64)
        assert got.no_data == -1.0 and tuple(got.geotransform) == gt
        assert np.array_equal(np.asarray(got), exp[key]) and (exp[key][dirs == 255] == -1.0).all()
    assert sums(r) == exp["result"] and (dirs == 255).any() and (exp["kept"][dirs != 255] > 0).any()
    os.remove(k)
    r = run(d, s, "-", "-", o, "-")                                      # no limits, out alone
    assert r.returncode == 0 and not os.path.exists(k), r.stdout + r.stderr
    exp = rd.d8_flow_accum_limited(dirs, supply, -9999.0)
    assert np.array_equal(np.asarray(rd.LoadNative(o, np.float64)), exp["out"]) and sums(r) == exp["result"]
    for name, a in ((s, supply), (c, cap)):
        rd.SaveNative(name, rd.rdarray(a.astype(np.float64), no_data=-9999))
    r = run(d, s, c, "-", "-", k, "f64")
    assert r.returncode == 0, r.stdout + r.stderr
    exp = rd.d8_flow_accum_limited(dirs, supply.astype(np.float64), -9999.0, cap.astype(np.float64))
    assert np.array_equal(np.asarray(rd.LoadNative(k, np.float64)), exp["kept"]) and sums(r) == exp["result"]
    assert run(d, s, c, "-", "-", "-", "f64").returncode != 0            # nothing to write
    assert run(d, s, c, "-", o, k, "i32").returncode != 0                # float supplies only
    assert run(d, s, o).returncode != 0                                  # usage
    rd.SaveNative(c, rd.rdarray(cap[:5].astype(np.float64), no_data=-9999))
    assert run(d, s, c, "-", o, k, "f64").returncode != 0                # sizes differ
