"""apps/rd_terrain_property (the reference app's argument order and algorithm numbers, native raster files): a round trip
whose output file is byte-equal to api.terrain_attribute's result saved with SaveNative."""
import os
import subprocess

import numpy as np
import pytest

from richdem_amd.synth import fractal_dem, fractal_dem_int

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("slope_riserun", "slope_percentage", "slope_degrees", "slope_radians", "aspect", "curvature",
         "planform_curvature", "profile_curvature")


def run(*args):
    exe = os.path.join(ROOT, "apps", "rd_terrain_property")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "apps")], check=True, capture_output=True)
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)


def test_rd_terrain_property_on_native_files(rd, tmp_path):
    z = fractal_dem(333, 222, 95).copy()
    z[40:44, 50:60] = -9999
    gt = (500.0, 10.0, 0.0, 800.0, 0.0, -20.0)
    src = rd.rdarray(z, no_data=-9999, geotransform=gt)
    dem, out, exp = str(tmp_path / "dem.rd"), str(tmp_path / "out.rd"), str(tmp_path / "exp.rd")
    rd.SaveNative(dem, src)
    for alg, name in enumerate(NAMES, 1):
        zscale = 2.5 if alg % 2 else 1.0
        r = run(dem, out, alg, zscale)
        assert r.returncode == 0, r.stderr
        got = rd.LoadNative(out, np.float32)
        want = rd.terrain_attribute(src, name, zscale=zscale, out_nodata=-9999)    # the result keeps the DEM's NoData
        assert got.no_data == -9999 and tuple(got.geotransform) == gt
        assert np.array_equal(np.asarray(got).view(np.int32), want.view(np.int32)), name
        rd.SaveNative(exp, rd.rdarray(want, meta_obj=src, no_data=-9999))
        assert open(out, "rb").read() == open(exp, "rb").read(), name
    zi = fractal_dem_int(100, 80, 96, 1.0, np.int16)
    rd.SaveNative(dem, rd.rdarray(zi, no_data=-32768, geotransform=gt))
    r = run(dem, out, 6, 1, "i16")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.asarray(rd.LoadNative(out, np.float32)),
                          rd.terrain_attribute(zi, "curvature", -32768, cell=(10.0, 20.0), out_nodata=-32768))
    assert run(dem, out, 9, 1, "i16").returncode == 1                  # unknown algorithm
    assert run(dem, out).returncode != 0                               # usage
