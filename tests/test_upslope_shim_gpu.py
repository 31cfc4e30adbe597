"""The upslope part of the C++ shim (include/rdgpu/richdem_gpu.hpp: rdgpu::d8_upslope_cells, d8_catchments, d8_outlets).
tests/cpp/upslope_shim_test checks the reference's side effects (output resized, NoData 255, geotransform / projection
copied, other element types) on a raster whose answers are known by hand, and in --batch mode runs every golden case of
tests/golden/ref_upslope.npz through rdgpu::d8_upslope_cells: equal to the compiled reference's raster on every cell."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from digest import load_golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "upslope_shim_test")


def _build(force=False):
    if force or not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.upslope"] + (["-B"] if force else []) + ["upslope_shim_test"],
                              stdout=subprocess.DEVNULL)


def test_upslope_shim_compiles_and_links(rd):
    _build(force=True)
    assert os.path.exists(EXE)


def test_upslope_shim_binds_to_the_reference_array2d():
    """the same calls compile against richdem::Array2D<T> from the unmodified reference tree, where it exists"""
    ref = os.environ.get("RICHDEM_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "include", "richdem")):
        pytest.skip("reference tree not present on this box")
    subprocess.check_call(["make", "-C", CPP, "-f", "Makefile.upslope", "check_richdem", "REF=" + ref], stdout=subprocess.DEVNULL)


@pytest.mark.gpu
def test_upslope_shim_runs_on_gpu(rd):
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


@pytest.mark.gpu
def test_upslope_shim_every_golden_case_equals_the_reference(rd, tmp_path):
    _build()
    g = load_golden(os.path.join(GOLDEN, "ref_upslope.npz"))
    cases = sorted({k.split("/")[0] for k in g})
    jobs, lines = [], []
    for c in cases:
        dirs = g[c + "/dirs"]
        h, w = dirs.shape
        src = tmp_path / (c + ".dirs")
        dirs.tofile(src)
        for i, ln in enumerate(g[c + "/lines"]):
            dst = tmp_path / f"{c}.up{i}"
            lines.append(f"{src} {w} {h} {int(g[c + '/nodata'])} {int(ln[0])} {int(ln[1])} {int(ln[2])} {int(ln[3])} {dst}")
            jobs.append((c, i, dst))
    manifest = tmp_path / "jobs.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([EXE, "--batch", str(manifest)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(jobs)} jobs done" in r.stdout
    for c, i, dst in jobs:
        exp = g[f"{c}/up{i}"]
        got = np.fromfile(dst, np.uint8).reshape(exp.shape)
        assert np.array_equal(got, exp), (c, i, int((got != exp).sum()))
        assert np.array_equal(np.fromfile(tmp_path / (c + ".dirs"), np.uint8).reshape(exp.shape), g[c + "/dirs"])
