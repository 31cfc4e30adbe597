"""numpy float64 restatement of the reference's terrain attributes (include/richdem/methods/terrain_attributes.hpp), pinned
to the compiled reference by tests/test_terrain_model.py (tests/golden/ref_terrain.npz).  TEST INFRASTRUCTURE: it lets
the GPU tests use fresh random inputs where the reference does not exist.

Every operation is the reference's, in its order, in IEEE double (numpy forms no FMA): + - * / sqrt are correctly rounded,
so rise/run, percentage and the three curvatures are bit-equal to the reference's after the one rounding to float32; atan /
atan2 / log are numpy's against glibc's, within 1 float32 ULP.
"""
from __future__ import annotations

import numpy as np

ATTRIBS = ("slope_riserun", "slope_percentage", "slope_degrees", "slope_radians", "aspect", "curvature",
           "planform_curvature", "profile_curvature")
ALGEBRAIC = ("slope_riserun", "slope_percentage", "curvature", "planform_curvature", "profile_curvature")


def window(dem: np.ndarray, nodata, zscale: float):
    """a..i as float64 planes: a neighbour off the grid or == nodata (compared in the DEM's type) takes the centre's value,
    then everything is multiplied by zscale (a float promoted to double)"""
    h, w = dem.shape
    nd = dem.dtype.type(nodata)
    zs = np.float64(np.float32(zscale))
    ce = dem.astype(np.float64)
    out = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v = ce.copy()
            ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            src = dem[ys, xs]
            with np.errstate(invalid="ignore"):
                ok = src != nd
            v[yd, xd] = np.where(ok, src.astype(np.float64), ce[yd, xd])
            out.append(v * zs)
    return out   # a b c d e f g h i


def terrain_attribute(dem: np.ndarray, attrib: str, nodata, zscale: float = 1.0, cell=(1.0, 1.0), out_nodata=-9999.0):
    assert attrib in ATTRIBS
    cx, cy = np.float64(abs(cell[0])), np.float64(abs(cell[1]))
    a, b, c, d, e, f, g, h, i = window(dem, nodata, zscale)
    with np.errstate(all="ignore"):
        if attrib.startswith("slope") or attrib == "aspect":
            dzdx = ((c + 2 * f + i) - (a + 2 * d + g)) / 8 / cx
            dzdy = ((g + 2 * h + i) - (a + 2 * b + c)) / 8 / cy
            if attrib == "aspect":
                t = 180.0 / np.pi * np.arctan2(dzdy, -dzdx)
                r = np.where(t < 0, 90 - t, np.where(t > 90.0, 360.0 - t + 90.0, 90.0 - t))
            else:
                r = np.sqrt(dzdx * dzdx + dzdy * dzdy)
                if attrib == "slope_percentage":
                    r = r * 100
                elif attrib == "slope_radians":
                    r = np.arctan(r)
                elif attrib == "slope_degrees":
                    r = np.arctan(r) * 180 / np.pi
        else:
            L = cx
            D = ((d + f) / 2 - e) / L / L
            E = ((b + h) / 2 - e) / L / L
            F = (-a + c + g - i) / 4 / L / L
            G = (-d + f) / 2 / L
            H = (b - h) / 2 / L
            if attrib == "curvature":
                r = -2 * (D + E) * 100
            elif attrib == "planform_curvature":
                r = np.where((G == 0) & (H == 0), 0.0, -2 * (D * H * H + E * G * G - F * G * H) / (G * G + H * H) * 100)
            else:
                r = np.where((G == 0) & (H == 0), 0.0, 2 * (D * G * G + E * H * H + F * G * H) / (G * G + H * H) * 100)
        out = r.astype(np.float32)
        out[dem == dem.dtype.type(nodata)] = np.float32(out_nodata)
    return out


def spi_cti(which: str, acc: np.ndarray, acc_nodata, slope: np.ndarray, slope_nodata, cell=(1.0, 1.0)):
    area = np.float64(abs(cell[0] * cell[1]))
    with np.errstate(all="ignore"):
        s = slope.astype(np.float64) + 0.001
        q = acc.astype(np.float64) / area
        r = np.log(q * s if which == "spi" else q / s).astype(np.float32)
    r[(acc == np.float64(acc_nodata)) | (slope == np.float32(slope_nodata))] = np.float32(-1.0)
    return r


def ulps32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in float32 steps; cells that are NaN in both count 0, NaN in one only count 2**31"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2**31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2**31) - ib, ib)
    u = np.abs(ia - ib)
    na, nb = np.isnan(a), np.isnan(b)
    u[na & nb] = 0
    u[na ^ nb] = 2**31
    return u


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """bit equality of two float32 arrays, where a NaN equals any NaN (the payload and sign of a NaN are not arithmetic)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))
