"""apps/rd_longest_flow_path on native raster files: its outputs equal the Python entry's, with one, two and three output
rasters."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "rd_longest_flow_path")


def run(*args):
    if not os.path.exists(APP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "apps"), "rd_longest_flow_path"], check=True, capture_output=True)
    return subprocess.run([APP, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_rd_longest_flow_path_app_equals_the_python_layer(rd, tmp_path):
    from richdem_amd.synth import fractal_dem

    filled = rd.FillDepressions(fractal_dem(70, 193, seed=11))
    filled[40:43, 50:56] = -9999
    dirs = rd.barnes_flat_resolution_d8(filled, -9999)
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    d, ln, fc, bp = (str(tmp_path / k) for k in ("dirs", "length", "from_cell", "on_basin_path"))
    rd.SaveNative(d, rd.rdarray(dirs, no_data=255, geotransform=gt))
    exp = rd.d8_longest_flow_path(dirs, cell=(10.0, -20.0), want=("from_cell", "length", "on_basin_path"))
    assert (exp["from_cell"] == 0xFFFFFFFF).any() and exp["on_basin_path"].any()
    for outs in ((ln,), (ln, fc), (ln, fc, bp)):
        for f in (ln, fc, bp):
            if os.path.exists(f):
                os.remove(f)
        r = run(d, *outs)
        assert r.returncode == 0, r.stdout + r.stderr
        got = rd.LoadNative(ln, np.float64)
        assert got.no_data == -1 and tuple(got.geotransform) == gt
        assert np.array_equal(np.asarray(got).view(np.uint64), exp["length"].view(np.uint64))
        if len(outs) >= 2:
            got = rd.LoadNative(fc, np.uint32)
            assert got.no_data == 0xFFFFFFFF and tuple(got.geotransform) == gt and np.array_equal(np.asarray(got), exp["from_cell"])
        if len(outs) == 3:
            got = rd.LoadNative(bp, np.uint8)
            assert got.no_data == 0 and np.array_equal(np.asarray(got), exp["on_basin_path"])
        assert os.path.exists(fc) == (len(outs) >= 2) and os.path.exists(bp) == (len(outs) == 3)
    assert run(d).returncode != 0                                        # usage
    assert run(d, ln, fc, bp, "more").returncode != 0
    assert run(str(tmp_path / "missing"), ln).returncode != 0
