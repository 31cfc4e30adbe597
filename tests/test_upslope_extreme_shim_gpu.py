"""The upslope-extreme part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::d8_upslope_extreme):
tests/cpp/extreme_shim_test checks the side effects (size, geotransform, projection, NoData) and hand-known answers, and
on native raster files it equals the Python layer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "extreme_shim_test")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.extreme"] + (["-B"] if force else []) + ["extreme_shim_test"],
                              stdout=subprocess.DEVNULL)


def test_extreme_shim_compiles_and_links(rd):
    _build(force=True)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_extreme_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["max", "min"])
def test_extreme_shim_equals_the_python_layer(rd, tmp_path, which):
    from richdem_amd.synth import fractal_dem

    _build()
    filled = rd.FillDepressions(fractal_dem(70, 193, seed=12))
    filled[60:63, 20:26] = -9999
    dirs = rd.barnes_flat_resolution_d8(filled, -9999)
    d, v, out = str(tmp_path / "dirs"), str(tmp_path / "vals"), str(tmp_path / "out")
    rd.SaveNative(d, rd.rdarray(dirs, no_data=255))
    rd.SaveNative(v, rd.rdarray(filled, no_data=-9999))
    r = subprocess.run([EXE, d, v, out, which], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "written" in r.stdout, r.stdout + r.stderr
    exp = rd.d8_upslope_extreme(dirs, filled, which, -9999.0)
    got_e, got_a = rd.LoadNative(out + "_extreme", np.float32), rd.LoadNative(out + "_at_cell", np.uint32)
    assert got_e.no_data == -9999 and got_a.no_data == 0xFFFFFFFF
    assert np.array_equal(np.asarray(got_e).view(np.uint32), exp["extreme"].view(np.uint32))
    assert np.array_equal(np.asarray(got_a), exp["at_cell"]) and (exp["at_cell"] == 0xFFFFFFFF).any()
    assert (exp["at_cell"] != np.arange(dirs.size, dtype=np.uint32).reshape(dirs.shape)).any()
