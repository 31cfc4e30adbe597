"""rdgpu::FillSpillMerge of the C++ shim (include/rdgpu/richdem_gpu.hpp) on top of rdgpu::DepressionHierarchy:
tests/cpp/fsm_shim_test checks conservation, hand-known depths and the side effects."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "fsm_shim_test")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.fsm"] + (["-B"] if force else []) + ["fsm_shim_test"],
                              stdout=subprocess.DEVNULL)


def test_fsm_shim_compiles_and_links(rd):
    _build(force=True)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_fsm_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
