"""The limited-accumulation part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::d8_flow_accum_limited):
tests/cpp/limited_shim_test checks the side effects (size, geotransform, projection, NoData) and hand-known answers, and on
native raster files it equals the Python layer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "limited_shim_test")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.limited"] + (["-B"] if force else []) + ["limited_shim_test"],
                              stdout=subprocess.DEVNULL)


def test_limited_shim_compiles_and_links(rd):
    _build(force=True)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_limited_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


def limited_case(rd, seed):
    """directions with a NoData island, and dyadic float32 supply, capacity and factor rasters: every partial sum is exact"""
    from richdem_amd.synth import fractal_dem

    filled = rd.FillDepressions(fractal_dem(70, 193, seed=seed))
    filled[60:63, 20:26] = -9999
    dirs = rd.barnes_flat_resolution_d8(filled, -9999)
    rng = np.random.default_rng(seed)
    supply = (rng.integers(-1023, 1024, dirs.shape) / 1024.0).astype(np.float32)
    supply[5:9, 5:9] = -9999
    cap = (rng.integers(0, 4096, dirs.shape) / 512.0).astype(np.float32)
    cap[rng.random(dirs.shape) < 0.5] = np.nan
    fac = rng.choice(np.array([1.0, 0.0, 0.5], np.float32), dirs.shape, p=[0.9, 0.07, 0.03])
    return dirs, supply, cap, fac


@pytest.mark.gpu
def test_limited_shim_equals_the_python_layer(rd, tmp_path):
    _build()
    dirs, supply, cap, fac = limited_case(rd, 12)
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    names = [str(tmp_path / n) for n in ("dirs", "supply", "cap", "fac", "res")]
    rd.SaveNative(names[0], rd.rdarray(dirs, no_data=255, geotransform=gt))
    rd.SaveNative(names[1], rd.rdarray(supply, no_data=-9999))
    rd.SaveNative(names[2], rd.rdarray(cap, no_data=-9999))
    rd.SaveNative(names[3], rd.rdarray(fac, no_data=-9999))
    r = subprocess.run([EXE] + names, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "written" in r.stdout, r.stdout + r.stderr
    exp = rd.d8_flow_accum_limited(dirs, supply, -9999.0, cap, fac, nodata_out=-5.0)
    for k in ("out", "kept"):
        got = rd.LoadNative(names[4] + "_" + k, np.float64)
        assert got.no_data == -5.0 and tuple(got.geotransform) == gt
        assert np.array_equal(np.asarray(got), exp[k]) and (exp[k] == -5.0).any()
    part = dirs != 255
    assert (exp["kept"][part] > 0).any() and (exp["kept"][part] < 0).any() and (exp["out"][part] > 1).any()
    sums = [float(x) for x in r.stdout.split()[1:5]]
    assert sums == [exp["result"][k] for k in ("supplied", "left", "kept_pos", "kept_neg")] and sums[0] == sums[1] + sums[2] + sums[3]
