"""apps/rd_upslope_extreme on native raster files: its two outputs equal the Python entry's, for both modes and for an
integer element type."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "rd_upslope_extreme")


def run(*args):
    if not os.path.exists(APP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "apps"), "rd_upslope_extreme"], check=True, capture_output=True)
    return subprocess.run([APP, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_rd_upslope_extreme_app_equals_the_python_layer(rd, tmp_path):
    from richdem_amd.synth import fractal_dem

    filled = rd.FillDepressions(fractal_dem(70, 193, seed=11))
    filled[40:43, 50:56] = -9999
    dirs = rd.barnes_flat_resolution_d8(filled, -9999)
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    d, v, vi, out = str(tmp_path / "dirs"), str(tmp_path / "vals"), str(tmp_path / "ints"), str(tmp_path / "out")
    rd.SaveNative(d, rd.rdarray(dirs, no_data=255, geotransform=gt))
    rd.SaveNative(v, rd.rdarray(filled, no_data=-9999, geotransform=gt))
    for which in ("max", "min"):
        r = run(d, v, out, which)
        assert r.returncode == 0, r.stdout + r.stderr
        exp = rd.d8_upslope_extreme(dirs, filled, which, -9999.0)
        got_e, got_a = rd.LoadNative(out + "_extreme", np.float32), rd.LoadNative(out + "_at_cell", np.uint32)
        assert got_e.no_data == -9999 and got_a.no_data == 0xFFFFFFFF and tuple(got_e.geotransform) == gt and tuple(got_a.geotransform) == gt
        assert np.array_equal(np.asarray(got_e).view(np.uint32), exp["extreme"].view(np.uint32))
        assert np.array_equal(np.asarray(got_a), exp["at_cell"]) and (exp["at_cell"] == 0xFFFFFFFF).any()
    ints = (np.arange(dirs.size, dtype=np.int64).reshape(dirs.shape) * 7919 % 1000 - 500).astype(np.int16)
    rd.SaveNative(vi, rd.rdarray(ints, no_data=-500))
    r = run(d, vi, out, "min", "i16")
    assert r.returncode == 0, r.stdout + r.stderr
    exp = rd.d8_upslope_extreme(dirs, ints, "min", -500)
    assert np.array_equal(np.asarray(rd.LoadNative(out + "_extreme", np.int16)), exp["extreme"])
    assert np.array_equal(np.asarray(rd.LoadNative(out + "_at_cell", np.uint32)), exp["at_cell"])
    assert run(d, v, out, "max", "f64").returncode != 0                  # 64-bit values are not supported
    assert run(d, v, out, "largest").returncode != 0                     # usage
    assert run(d, v, out).returncode != 0
    rd.SaveNative(v, rd.rdarray(filled[:5], no_data=-9999))
    assert run(d, v, out, "max").returncode != 0                         # sizes differ
