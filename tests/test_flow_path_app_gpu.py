"""apps/rd_flow_distance on native raster files: its output equals the Python entry's, with and without a channel raster,
in the units of the directions' geotransform."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "rd_flow_distance")


def run(*args):
    if not os.path.exists(APP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "apps"), "rd_flow_distance"], check=True, capture_output=True)
    return subprocess.run([APP, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_rd_flow_distance_app_equals_the_python_layer(rd, tmp_path):
    from richdem_amd.synth import fractal_dem

    dem = fractal_dem(150, 130, seed=11)
    filled = rd.FillDepressions(dem)
    filled[40:43, 50:56] = -9999
    dirs = rd.barnes_flat_resolution_d8(filled, -9999)
    chan = rd.d8_channels(rd.d8_flow_accum(dirs), 20.0)
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    d, c, out = str(tmp_path / "dirs"), str(tmp_path / "chan"), str(tmp_path / "dist")
    rd.SaveNative(d, rd.rdarray(dirs, no_data=255, geotransform=gt))
    rd.SaveNative(c, rd.rdarray(chan, no_data=0, geotransform=gt))
    r = run(d, out)
    assert r.returncode == 0, r.stdout + r.stderr
    got = rd.LoadNative(out, np.float64)
    exp = rd.d8_flow_distance(dirs, 255, None, (10.0, 20.0))
    assert got.no_data == -1 and tuple(got.geotransform) == gt
    assert np.array_equal(np.asarray(got).view(np.uint64), exp.view(np.uint64)) and (exp == -1).any() and exp.max() > 100
    r = run(d, out, c)
    assert r.returncode == 0, r.stdout + r.stderr
    exp = rd.d8_flow_distance(dirs, 255, chan, (10.0, 20.0))
    assert np.array_equal(np.asarray(rd.LoadNative(out, np.float64)).view(np.uint64), exp.view(np.uint64))
    assert (exp[chan != 0] == 0).all() and (exp > 0).any()
    rd.SaveNative(c, rd.rdarray(chan[:5], no_data=0))
    assert run(d, out, c).returncode != 0                               # sizes differ
    assert run(d).returncode != 0                                       # usage
