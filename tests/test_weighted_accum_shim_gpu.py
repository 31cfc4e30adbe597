"""The weighted-accumulation part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::d8_flow_accum_weighted,
rdgpu::d8_total_upstream_length): tests/cpp/weighted_shim_test checks the side effects (size, geotransform, projection,
NoData) and hand-known answers, and on native raster files it equals the Python layer."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "weighted_shim_test")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.weighted"] + (["-B"] if force else []) + ["weighted_shim_test"],
                              stdout=subprocess.DEVNULL)


def test_weighted_shim_compiles_and_links(rd):
    _build(force=True)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_weighted_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


@pytest.mark.gpu
def test_weighted_shim_equals_the_python_layer(rd, tmp_path):
    from richdem_amd.synth import fractal_dem

    _build()
    filled = rd.FillDepressions(fractal_dem(70, 193, seed=12))
    filled[60:63, 20:26] = -9999
    dirs = rd.barnes_flat_resolution_d8(filled, -9999)
    wts = (np.random.default_rng(3).integers(-4096, 4096, dirs.shape) / 64.0).astype(np.float32)   # every partial sum is exact
    wts[5:9, 5:9] = -9999
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    d, v, out = str(tmp_path / "dirs"), str(tmp_path / "wts"), str(tmp_path / "out")
    rd.SaveNative(d, rd.rdarray(dirs, no_data=255, geotransform=gt))
    rd.SaveNative(v, rd.rdarray(wts, no_data=-9999))
    r = subprocess.run([EXE, d, v, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "written" in r.stdout, r.stdout + r.stderr
    exp = rd.d8_flow_accum_weighted(dirs, wts, -9999.0, sum_nodata=-5.0)
    got = rd.LoadNative(out + "_sum", np.float64)
    assert got.no_data == -5.0 and tuple(got.geotransform) == gt
    assert np.array_equal(np.asarray(got).view(np.uint64), exp.view(np.uint64)) and (exp == -5.0).any()
    assert (exp[dirs != 255] != wts[dirs != 255]).any()
    tl = rd.d8_total_upstream_length(dirs, 10.0, 20.0)
    length = rd.LoadNative(out + "_length", np.float64)
    assert length.no_data == -1.0 and np.array_equal(np.asarray(length).view(np.uint64), tl["length"].view(np.uint64))
    for k, name in enumerate(("_nx", "_ny", "_nd")):
        plane = rd.LoadNative(out + name, np.uint32)
        assert plane.no_data == 0xFFFFFFFF and np.array_equal(np.asarray(plane), tl["steps"][k])
    assert tl["steps"][:, dirs != 255].any() and (tl["length"] == -1.0).any()
