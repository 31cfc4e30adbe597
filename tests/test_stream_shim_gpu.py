"""The channel-network part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::d8_channels, rdgpu::d8_stream_order)
and the app built on it (apps/rd_stream_order): tests/cpp/streams_shim_test checks the side effects and hand-known
answers; the app's raster equals the Python layer's on a fractal forest."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "streams_shim_test")
APP = os.path.join(ROOT, "apps", "rd_stream_order")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.streams"] + (["-B"] if force else []) + ["streams_shim_test"],
                              stdout=subprocess.DEVNULL)
    if force or not os.path.exists(APP):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps")] + (["-B"] if force else []) + ["rd_stream_order"],
                              stdout=subprocess.DEVNULL)


def test_stream_shim_and_app_compile_and_link(rd):
    _build(force=True)
    assert os.path.exists(EXE) and os.path.exists(APP)


@pytest.mark.gpu
def test_stream_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


@pytest.mark.gpu
def test_rd_stream_order_app_equals_the_python_layer(rd, tmp_path):
    from richdem_amd.synth import fractal_dem

    _build()
    dem = fractal_dem(150, 130, seed=11)
    dirs = rd.barnes_flat_resolution_d8(rd.FillDepressions(dem), -9999)
    acc = rd.d8_flow_accum(dirs)
    rd.SaveNative(str(tmp_path / "dirs"), rd.rdarray(dirs, no_data=255))
    rd.SaveNative(str(tmp_path / "acc"), rd.rdarray(acc, no_data=-1))
    r = subprocess.run([APP, str(tmp_path / "dirs"), str(tmp_path / "acc"), "20", str(tmp_path / "order")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.asarray(rd.LoadNative(str(tmp_path / "order"), np.uint8))
    exp = rd.d8_stream_order(dirs, 255, rd.d8_channels(acc, 20.0))
    assert got.dtype == np.uint8 and np.array_equal(got, exp) and exp.max() >= 2
    r = subprocess.run([APP, str(tmp_path / "dirs")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
