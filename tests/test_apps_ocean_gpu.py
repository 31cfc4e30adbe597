"""apps/rd_depression_hierarchy and apps/rd_fill_spill_merge end to end on a small native raster with a NoData hole and a
sea level: file -> Array2D -> rdgpu:: calls -> files, compared with the Python calls on the same raster."""
import os
import subprocess

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
SEA = -5.0


def run(app, *args):
    exe = os.path.join(ROOT, "apps", app)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "apps")], check=True, capture_output=True)
    return subprocess.run(["timeout", "-k", "10", "120", exe, *map(str, args)], capture_output=True, text=True)


def coast(dtype=np.float32):
    """a fractal whose lowest quarter is a sea of one level (with lakes of that level inland), and a NoData hole"""
    z = fractal_dem(97, 70, 17).astype(np.float64)
    z = np.where(z < np.quantile(z, 0.25), SEA, np.floor(z * 8.0) / 8.0)
    z[30:38, 40:52] = -9999
    return z.astype(dtype)


def test_rd_depression_hierarchy(rd, tmp_path):
    z = coast()
    src, prefix = str(tmp_path / "dem.rd"), str(tmp_path / "out")
    rd.SaveNative(src, rd.rdarray(z, no_data=-9999, geotransform=(500.0, 10.0, 0.0, 800.0, 0.0, -10.0)))
    r = run("rd_depression_hierarchy", src, prefix, SEA)
    assert r.returncode == 0, r.stderr
    ocean = ((z == -9999) | (z == np.float32(SEA))).astype(np.uint8)       # the app's rule: anywhere, no bucket fill
    labels, tab = rd.depression_hierarchy(z, 8, ocean=ocean)
    assert len(tab) > 20
    got = rd.LoadNative(prefix + "-label", np.uint32)
    assert np.array_equal(np.asarray(got), (labels + 1).astype(np.uint32)) and got.no_data == 0
    assert tuple(got.geotransform) == (500.0, 10.0, 0.0, 800.0, 0.0, -10.0)
    lines = open(prefix + "-graph.csv").read().split("\n")
    assert lines[0] == "parent,child,oceanlink" and lines[-1] == "" and len(lines) == len(tab) + 2
    for i, line in enumerate(lines[1:-1]):
        root = tab["parent"][i] == NONE
        up = tab["geolink"][i] if root else tab["parent"][i]
        assert line == f"{0 if up == NONE else int(up) + 1},{i + 1},{int(root)}"
    # an integer raster through the type argument; f64 is refused by the engine
    zi = coast(np.int32)
    rd.SaveNative(src, rd.rdarray(zi, no_data=-9999))
    assert run("rd_depression_hierarchy", src, prefix, SEA, "i32").returncode == 0
    li, _ = rd.depression_hierarchy(zi, 8, ocean=((zi == -9999) | (zi == int(SEA))).astype(np.uint8))
    assert np.array_equal(np.asarray(rd.LoadNative(prefix + "-label", np.uint32)), (li + 1).astype(np.uint32))
    assert run("rd_depression_hierarchy", src, prefix, SEA, "f64").returncode == 1
    assert run("rd_depression_hierarchy", src, prefix).returncode != 0                    # the syntax line
    rd.SaveNative(src, rd.rdarray(np.full((5, 5), 3.0, np.float32), no_data=-9999))
    r = run("rd_depression_hierarchy", src, prefix, SEA)                                  # no ocean cells
    assert r.returncode == 1 and "no ocean cells" in r.stderr


def test_rd_fill_spill_merge(rd, tmp_path):
    z = coast()
    src, prefix = str(tmp_path / "dem.rd"), str(tmp_path / "out")
    rd.SaveNative(src, rd.rdarray(z, no_data=-9999))
    ocean = rd.ocean_mask(z, ocean_level=SEA, nodata=-9999)                # the app's rule: bucket fill from the edges + NoData
    inland = (z == np.float32(SEA)) & (ocean == 0)
    assert inland.any() and ocean[30:38, 40:52].all()                      # lakes at sea level stay land
    labels, tab = rd.depression_hierarchy(z, 8, ocean=ocean)
    for args, water in ((("--swl", 0.375), np.full(z.shape, 0.375)),
                        (("--swf", str(tmp_path / "water.rd")), np.random.default_rng(2).integers(0, 64, z.shape) / 32.0)):
        if args[0] == "--swf":
            rd.SaveNative(args[1], rd.rdarray(water, no_data=-1))
        r = run("rd_fill_spill_merge", src, prefix, SEA, *args)
        assert r.returncode == 0, r.stderr
        depth, res = rd.fill_spill_merge(z, labels, tab, np.where(ocean != 0, 0.0, water))
        wtd = rd.LoadNative(prefix + "-wtd", np.float64)
        assert np.array_equal(np.asarray(wtd), depth) and wtd.no_data == -9999 and (np.asarray(wtd)[ocean != 0] == 0).all()
        assert res["standing"] > 0 and res["ocean"] > 0
        hsh = np.asarray(rd.LoadNative(prefix + "-hydrologic-surface-height", np.float64))
        assert np.array_equal(hsh, np.where(z == -9999, depth, depth + z.astype(np.float64)))
    assert run("rd_fill_spill_merge", src, prefix, SEA).returncode != 0                   # no water given
    assert run("rd_fill_spill_merge", src, prefix, SEA, "--what", 1).returncode != 0
