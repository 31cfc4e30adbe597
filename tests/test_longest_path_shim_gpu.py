"""The longest-flow-path part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::d8_longest_flow_path):
tests/cpp/longest_shim_test checks the side effects (size, geotransform, projection, NoData) and hand-known answers, and
on a native raster file it equals the Python layer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "longest_shim_test")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.longest"] + (["-B"] if force else []) + ["longest_shim_test"],
                              stdout=subprocess.DEVNULL)


def test_longest_shim_compiles_and_links(rd):
    _build(force=True)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_longest_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


@pytest.mark.gpu
def test_longest_shim_equals_the_python_layer(rd, tmp_path):
    from richdem_amd.synth import fractal_dem

    _build()
    filled = rd.FillDepressions(fractal_dem(70, 193, seed=12))
    filled[60:63, 20:26] = -9999
    dirs = rd.barnes_flat_resolution_d8(filled, -9999)
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    d, out = str(tmp_path / "dirs"), str(tmp_path / "out")
    rd.SaveNative(d, rd.rdarray(dirs, no_data=255, geotransform=gt))
    r = subprocess.run([EXE, d, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "written" in r.stdout, r.stdout + r.stderr
    exp = rd.d8_longest_flow_path(dirs, cell=(10.0, 20.0), want=("from_cell", "length", "on_basin_path"))
    got_l, got_f = rd.LoadNative(out + "_length", np.float64), rd.LoadNative(out + "_from_cell", np.uint32)
    got_p = rd.LoadNative(out + "_on_basin_path", np.uint8)
    assert got_l.no_data == -1 and got_f.no_data == 0xFFFFFFFF and got_p.no_data == 0 and tuple(got_l.geotransform) == gt
    assert np.array_equal(np.asarray(got_l).view(np.uint64), exp["length"].view(np.uint64))
    assert np.array_equal(np.asarray(got_f), exp["from_cell"]) and (exp["from_cell"] == 0xFFFFFFFF).any()
    assert np.array_equal(np.asarray(got_p), exp["on_basin_path"]) and exp["on_basin_path"].any()
    assert (exp["from_cell"] != np.arange(dirs.size, dtype=np.uint32).reshape(dirs.shape)).any()
