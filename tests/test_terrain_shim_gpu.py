"""The TerrainAttribute part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::TA_*): tests/cpp/terrain_shim_test checks
the reference's side effects -- output resized, geotransform / projection copied, the output's NoData kept, SPI / CTI NoData
-1 -- and its exceptions, an empty geotransform included."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_terrain_shim_compiles_and_links(rd):
    subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.terrain", "-B", "terrain_shim_test"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(CPP, "terrain_shim_test"))


@pytest.mark.gpu
def test_terrain_shim_runs_on_gpu(rd):
    exe = os.path.join(CPP, "terrain_shim_test")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.terrain", "terrain_shim_test"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
