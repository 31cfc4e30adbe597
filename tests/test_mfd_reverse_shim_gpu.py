"""The reverse-accumulation part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::FlowReverseAccumulation,
rdgpu::DinfReverseAccumulation[_flats], rdgpu::DinfUpslopeDependence[_flats]): tests/cpp/mfd_reverse_shim_test checks the
side effects (size, geotransform, projection, NoData) and hand-known answers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "mfd_reverse_shim_test")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.mfdrev"] + (["-B"] if force else [])
                              + ["mfd_reverse_shim_test"], stdout=subprocess.DEVNULL)


def test_mfd_reverse_shim_compiles_and_links(rd):
    _build(force=True)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_mfd_reverse_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
