"""The numpy model of the terrain attributes (tests/terrain_model.py) against the COMPILED REFERENCE's outputs
(tests/golden/ref_terrain.npz, tests/golden/make_golden_terrain.py): bit for bit for rise/run, percentage and the three
curvatures -- only + - * / sqrt in IEEE double and one rounding to float32, correctly rounded on both sides -- and within
1 float32 ULP for the atan / atan2 / log attributes.  No cell is left out.  The C-ABI's argument errors are checked here
too: they return before any device call, so they need no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from digest import load_golden  # noqa: E402
import terrain_model as tm  # noqa: E402


def _golden():
    return load_golden(os.path.join(GOLDEN, "ref_terrain.npz"))


def _cases(g):
    return sorted({k.split("/")[0] for k in g})


CASES = _cases(_golden())


def test_the_golden_file_has_the_cases_the_kernel_must_survive():
    g = _golden()
    assert len(CASES) >= 20
    assert {g[c + "/dem"].dtype.name for c in CASES} == {"uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64",
                                                        "int64", "float32", "float64"}
    assert (g["level_f32/aspect"] == 270.0).all() and (g["level_f32/planform_curvature"] == 0.0).all()
    assert (g["level_f32/profile_curvature"] == 0.0).all()
    assert g["one_cell/dem"].shape == (1, 1) and g["one_row/dem"].shape[0] == 1 and g["one_column/dem"].shape[1] == 1
    assert np.isnan(g["nan_nodata_f32/nodata"][0]) and np.isnan(g["nan_nodata_f32/slope_riserun"]).any()
    assert g["big_i64/dem"].max() > 2**53 and g["big_u64/dem"].max() > 2**63
    assert any(g[c + "/params"][0] == 2.5 for c in CASES) and any(g[c + "/params"][1] != g[c + "/params"][2] for c in CASES)


@pytest.mark.parametrize("case", CASES)
def test_model_equals_the_reference(case):
    g = _golden()
    dem, nodata = g[case + "/dem"], g[case + "/nodata"][0]
    zscale, cx, cy, out_nd = g[case + "/params"]
    for a in tm.ATTRIBS:
        got = tm.terrain_attribute(dem, a, nodata, zscale, (cx, cy), out_nd)
        exp = g[case + "/" + a]
        if a in tm.ALGEBRAIC:
            assert tm.same_bits(got, exp), (case, a, int((got.view(np.int32) != exp.view(np.int32)).sum()))
        else:
            u = tm.ulps32(got, exp)
            assert u.max() <= 1, (case, a, int(u.max()), int((u > 0).sum()))
    for which in ("spi", "cti"):
        got = tm.spi_cti(which, g[case + "/acc"], g[case + "/acc_nodata"], g[case + "/slope_riserun"], out_nd, (cx, cy))
        u = tm.ulps32(got, g[case + "/" + which])
        assert u.max() <= 1, (case, which, int(u.max()))
        assert (got[g[case + "/acc"] == -1.0] == -1.0).all()


def test_invalid_attribute_name_raises_the_reference_message(rd):
    with pytest.raises(rd.RdgpuError, match="Invalid TerrainAttributes attribute. Valid attributes are: slope_riserun, "
                                            "slope_percentage, slope_degrees, slope_radians, aspect, curvature, "
                                            "planform_curvature, profile_curvature"):
        rd.terrain_attribute(np.zeros((4, 4), np.float32), "slope", -9999)
    with pytest.raises(rd.RdgpuError, match="Invalid TerrainAttributes"):
        rd.terrain_attributes(np.zeros((4, 4), np.float32), ["aspect", "spi"], -9999)


def test_capi_argument_errors_need_no_gpu(rd):
    L = rd.lib()
    dem = np.zeros((4, 4), np.float32)
    out = np.zeros((4, 4), np.float32)
    p, q = dem.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    f32, f64 = ctypes.c_float, ctypes.c_double

    def call(dem_p=p, w=4, h=4, cx=1.0, cy=1.0, attr=0, out_p=q, fn="rdgpu_terrain_attribute_f32"):
        nd = ctypes.c_uint64(0) if fn.endswith("u64") else f32(-9999)
        return getattr(L, fn)(dem_p, nd, w, h, f64(cx), f64(cy), f32(1.0), attr, out_p, f32(-9999))

    for kw, word in (({"attr": 8}, "attribute"), ({"attr": -1}, "attribute"), ({"cx": 0.0}, "cell length"),
                     ({"cy": float("nan")}, "cell length"), ({"cx": float("inf")}, "cell length"), ({"w": 0}, "positive"),
                     ({"h": -3}, "positive"), ({"dem_p": None}, "null"), ({"out_p": None}, "null")):
        for fn in ("rdgpu_terrain_attribute_f32", "rdgpu_terrain_attribute_u64"):
            assert call(fn=fn, **kw) == 2, kw                      # RDGPU_ERR_ARG
            assert word in L.rdgpu_last_error().decode(), (kw, L.rdgpu_last_error())
    outs = (ctypes.c_void_p * 8)()
    outs[0] = out.ctypes.data
    for mask, word in ((0, "attribute"), (256, "attribute"), (3, "null")):
        assert L.rdgpu_terrain_attributes_dev_f32(p, f32(-9999), 4, 4, f64(1), f64(1), f32(1), ctypes.c_uint(mask), outs,
                                                  f32(-9999), None) == 2
        assert word in L.rdgpu_last_error().decode()
    acc = np.ones((4, 4), np.float64)
    for fn in ("rdgpu_ta_spi", "rdgpu_ta_cti"):
        assert getattr(L, fn)(acc.ctypes.data_as(ctypes.c_void_p), f64(-1), p, f32(-9999), 4, 4, f64(0.0), f64(1.0), q) == 2
        assert "cell length" in L.rdgpu_last_error().decode()
        assert getattr(L, fn)(None, f64(-1), p, f32(-9999), 4, 4, f64(1.0), f64(1.0), q) == 2
    with pytest.raises(rd.RdgpuError, match="Couldn't calculate SPI! The input matricies were of unequal dimensions!"):
        rd.terrain_spi(np.ones((4, 4)), np.ones((4, 5), np.float32), -1.0, -9999.0)
    with pytest.raises(rd.RdgpuError, match="Couldn't calculate CTI! The input matricies were of unequal dimensions!"):
        rd.terrain_cti(np.ones((4, 4)), np.ones((3, 4), np.float32), -1.0, -9999.0)
