"""The breaching part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::BreachDepressions,
rdgpu::CompleteBreaching_Lindsay2016, rdgpu::d8_breach_along) and apps/rd_depressions_breach: tests/cpp/breach_shim_test
checks hand-known answers, the side effects and what is refused; on native raster files shim and app equal the compiled
reference's golden.  pyrichdem.BreachDepressions and _richdem.rdBreachDepressionsD8 stay bound and raising."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "breach_shim_test")
APP = os.path.join(ROOT, "apps", "rd_depressions_breach")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.breach"] + (["-B"] if force else []) + ["breach_shim_test"],
                              stdout=subprocess.DEVNULL)
    if force or not os.path.exists(APP):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "rd_depressions_breach"], stdout=subprocess.DEVNULL)


def test_breach_shim_and_app_compile_and_link(rd):
    _build(force=True)
    assert os.path.exists(EXE) and os.path.exists(APP)
    r = subprocess.run([APP], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "breaching" in r.stderr


@pytest.mark.gpu
def test_breach_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


@pytest.mark.gpu
def test_breach_shim_and_app_equal_the_reference(rd, tmp_path):
    import breach_cases as bc
    from digest import load_golden

    _build()
    name = "q_i16_130x129"
    dem = bc.CASES[name]()
    exp = load_golden(os.path.join(ROOT, "tests", "golden", "ref_breach.npz"))[name + "/out"]
    src = str(tmp_path / "dem")
    rd.SaveNative(src, rd.rdarray(dem, no_data=-9999))
    for cmd, out in (([EXE, src], "shim"), ([APP, src], "app")):
        dst = str(tmp_path / out)
        tail = [dst] if out == "shim" else [dst, "COMPLETE", "i16"]
        r = subprocess.run(cmd + tail, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = rd.LoadNative(dst, np.int16)
        assert got.no_data == -9999 and np.array_equal(np.asarray(got), exp)
    r = subprocess.run([APP, src, str(tmp_path / "x"), "SELECTIVE", "i16"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and not os.path.exists(str(tmp_path / "x"))
