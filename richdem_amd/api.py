"""Host-side mirror of the reference operator interface for the hot path, over the C-ABI.

Host arrays (numpy) go through the drop-in entry points ``rdgpu_<op>_<dtype>`` (H2D, compute, D2H into
the same buffer); HBM-resident torch tensors go through ``rdgpu_<op>_dev_<dtype>``.
"""
from __future__ import annotations

import ctypes
import os
import warnings

import numpy as np

from ._lib import RdgpuError, check, lib

_SUFFIX = {
    np.dtype(np.int8): "i8",
    np.dtype(np.uint8): "u8",
    np.dtype(np.int16): "i16",
    np.dtype(np.uint16): "u16",
    np.dtype(np.int32): "i32",
    np.dtype(np.uint32): "u32",
    np.dtype(np.float32): "f32",
    np.dtype(np.float64): "f64",
    np.dtype(np.int64): "i64",
    np.dtype(np.uint64): "u64",
}
_TOPO = {"D8": 8, "D4": 4, 8: 8, 4: 4}
_CT = {"i8": ctypes.c_int8, "u8": ctypes.c_uint8, "i16": ctypes.c_int16, "u16": ctypes.c_uint16, "i32": ctypes.c_int32,
       "u32": ctypes.c_uint32, "f32": ctypes.c_float, "f64": ctypes.c_double, "i64": ctypes.c_int64, "u64": ctypes.c_uint64}
_NP = {"i8": np.int8, "u8": np.uint8, "i16": np.int16, "u16": np.uint16, "i32": np.int32, "u32": np.uint32, "f32": np.float32,
       "f64": np.float64, "i64": np.int64, "u64": np.uint64}


def _scalar(s: str, nodata):
    """ctypes scalar of the DEM's element type from the user's no_data value, converted the way the reference's
    setNoData(double) does (a C cast to T: fractions truncate towards zero, out-of-range integers wrap as they do
    on x86-64): rdarray(int16_arr, no_data=-9999.0) works, and so does the common uint8 DEM with no_data=-9999.
    NaN / infinite values for an integer DEM are an error."""
    if s in ("f32", "f64"):
        return _CT[s](float(nodata))
    try:
        v = int(float(nodata))
    except (TypeError, ValueError, OverflowError):
        raise RdgpuError(f"no_data value {nodata!r} is not representable in the DEM's element type {_NP[s].__name__}") from None
    bits = 8 * np.dtype(_NP[s]).itemsize
    v &= (1 << bits) - 1
    if np.issubdtype(_NP[s], np.signedinteger) and v >= 1 << (bits - 1):
        v -= 1 << bits
    return _CT[s](v)


_ELEV_SUFFIX = dict(_SUFFIX)   # d8 directions, flat resolution, ResolveFlatsEpsilon, FA_D8 / FM_D8: every element type
_MFD_SUFFIX = {k: v for k, v in _SUFFIX.items() if v not in ("i64", "u64")}   # D-infinity and the MFD families
_ACC_SUFFIX = {np.dtype(np.int32): "i32", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}


def _suffix(dtype) -> str:
    try:
        return _SUFFIX[np.dtype(dtype)]
    except KeyError:
        raise RdgpuError(f"unsupported elevation dtype {dtype} (supported: {sorted(str(k) for k in _SUFFIX)})") from None


def _topo(topology) -> int:
    try:
        return _TOPO[topology]
    except KeyError:
        raise RdgpuError("Unknown topology!") from None  # depressions.hpp:19-20


def FillDepressions(dem: np.ndarray, epsilon: bool = False, in_place: bool = False, topology="D8", shards: int = 1,
                    nodata=-9999):
    """Fill all depressions of ``dem`` (reference: ``rd.FillDepressions``,
    wrappers/pyrichdem/richdem/__init__.py:381-422 -> FillDepressions<topo>, depressions.hpp:13-21; ``epsilon=True``
    -> PriorityFloodEpsilon_Barnes2014<topo>, depressions/Barnes2014.hpp:335-420, floating point only, ``nodata`` cells
    are left alone).  Returns the filled array (or None when ``in_place``).

    Ties (``epsilon=True`` only; the plain fill is exact for every input): the reference's result depends on the order
    in which ``std::priority_queue`` pops cells of EQUAL elevation -- a plateau or lake entered through several cells
    of one level gets its gradient from whichever pops first.  This engine returns the order-free surface
    ``E(c) = max(z(c), nextafter(min over neighbours E))``: identical to the reference when no two gradient sources
    share an elevation, a cell-wise lower bound of it otherwise (quantised / integer-valued DEMs).  The number of such
    sources is counted on the device (``epsilon_stats()["tie_sources"]``) and a ``RuntimeWarning`` is raised when it is
    not zero."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("FillDepressions: expected a 2-D numpy array")
    out = dem if in_place else dem.copy()
    if not out.flags["C_CONTIGUOUS"]:
        if in_place:
            raise RdgpuError("FillDepressions(in_place=True) needs a C-contiguous array")
        out = np.ascontiguousarray(out)
    h, w = out.shape
    if epsilon:
        if shards > 1:
            raise RdgpuError("FillDepressions(epsilon=True, shards=...): the epsilon fill is not sharded; use shards=1")
        if out.dtype not in (np.float32, np.float64):
            raise RdgpuError("Priority-Flood+Epsilon is only available for floating-point data types!")   # Barnes2014.hpp:424-451
        s = _suffix(out.dtype)
        check(getattr(lib(), f"rdgpu_fill_epsilon_{s}")(out.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h,
                                                        _topo(topology)), "rdgpu_fill_epsilon")
        ties = epsilon_stats()["tie_sources"]
        if ties:
            warnings.warn(f"FillDepressions(epsilon=True): {ties} gradient sources share their elevation with another one; "
                          "the reference's Priority-Flood+Epsilon resolves such ties by std::priority_queue's pop order, "
                          "this engine returns the order-free surface (a cell-wise lower bound of the reference's)",
                          RuntimeWarning, stacklevel=2)
        return None if in_place else out
    if shards > 1:   # the multi-GPU row-block protocol, shard after shard on one GPU
        if _suffix(out.dtype) in ("f64", "i64", "u64"):
            raise RdgpuError("FillDepressions(shards=...): the row-block shard engine takes the 32-bit element types")
        fn = getattr(lib(), f"rdgpu_fill_sharded_{_suffix(out.dtype)}")
        check(fn(out.ctypes.data_as(ctypes.c_void_p), w, h, _topo(topology), int(shards)), "rdgpu_fill_sharded")
    else:
        fn = getattr(lib(), f"rdgpu_fill_{_suffix(out.dtype)}")
        check(fn(out.ctypes.data_as(ctypes.c_void_p), w, h, _topo(topology)), "rdgpu_fill")
    return None if in_place else out


def has_depressions(dem: np.ndarray, topology="D8") -> bool:
    """HasDepressions<topo> (depressions/Barnes2014.hpp:44-103; apps/rd_depressions_has.cpp): True when the fill would
    raise at least one cell of ``dem``."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("has_depressions: expected a 2-D numpy array")
    dem = np.ascontiguousarray(dem)
    h, w = dem.shape
    if w == 0 or h == 0:
        return False
    out = ctypes.c_int(0)
    check(getattr(lib(), f"rdgpu_has_depressions_{_suffix(dem.dtype)}")(dem.ctypes.data_as(ctypes.c_void_p), w, h, _topo(topology),
                                                                          ctypes.byref(out)), "rdgpu_has_depressions")
    return bool(out.value)


def fill_wei2018(dem: np.ndarray, nodata=-9999, in_place: bool = False):
    """PriorityFlood_Wei2018 (depressions/Wei2018.hpp:154-202): the D8 fill in which NoData cells stay as they are and the
    data cells next to them drain like the raster's edge cells (InitPriorityQue, :14-50)."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("fill_wei2018: expected a 2-D numpy array")
    out = dem if in_place else dem.copy()
    if not out.flags["C_CONTIGUOUS"]:
        if in_place:
            raise RdgpuError("fill_wei2018(in_place=True) needs a C-contiguous array")
        out = np.ascontiguousarray(out)
    s = _suffix(out.dtype)
    h, w = out.shape
    if w and h:
        check(getattr(lib(), f"rdgpu_fill_wei2018_{s}")(out.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h),
              "rdgpu_fill_wei2018")
    return None if in_place else out


def fill_max_dep(dem: np.ndarray, max_dep_size: int, topology="D8", in_place: bool = False):
    """PriorityFlood_Barnes2014_max_dep<topo> (depressions/Barnes2014.hpp:844-931; rd_depressions_flood's third
    argument): only depressions of at most ``max_dep_size`` cells are filled."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("fill_max_dep: expected a 2-D numpy array")
    out = dem if in_place else dem.copy()
    if not out.flags["C_CONTIGUOUS"]:
        if in_place:
            raise RdgpuError("fill_max_dep(in_place=True) needs a C-contiguous array")
        out = np.ascontiguousarray(out)
    s = _suffix(out.dtype)
    if int(max_dep_size) < 0:
        raise RdgpuError("fill_max_dep: max_dep_size must not be negative")
    h, w = out.shape
    check(getattr(lib(), f"rdgpu_fill_max_dep_{s}")(out.ctypes.data_as(ctypes.c_void_p), w, h, _topo(topology),
                                                    ctypes.c_uint64(int(max_dep_size))), "rdgpu_fill_max_dep")
    st = max_dep_stats()   # (64-bit element types run on dense value ranks through the same engine: equal values, equal ranks)
    if st["tie_cluster_cells"]:   # (cells whose fate the order can actually decide; pockets with two candidates alone are common)
        warnings.warn(f"fill_max_dep: {st['tie_pockets']} of {st['pockets']} pockets can be flooded by two or more cells of their "
                      f"spill elevation; in their clusters ({st['tie_cluster_cells']} of {st['pocket_cells']} pocket cells) the "
                      "reference's grouping follows its heap's pop order, this engine's the lowest cell index", RuntimeWarning)
    return None if in_place else out


def watersheds(dem: np.ndarray, nodata=-9999, topology="D8", alter: bool = False):
    """PriorityFloodWatersheds_Barnes2014<topo> (depressions/Barnes2014.hpp:713-807): int32 watershed labels (1.. in the
    order the watersheds' first cells are flooded, -1 for NoData connected to the border); with ``alter`` also the filled
    DEM: returns labels, or (labels, filled)."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("watersheds: expected a 2-D numpy array")
    work = np.ascontiguousarray(dem).copy()
    s = _suffix(work.dtype)
    h, w = work.shape
    labels = np.empty((h, w), np.int32)
    check(getattr(lib(), f"rdgpu_watersheds_{s}")(work.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h, _topo(topology),
                                                  1 if alter else 0, labels.ctypes.data_as(ctypes.c_void_p)), "rdgpu_watersheds")
    return (labels, work) if alter else labels


def pf_flowdirs_dev(dem, nodata, dirs) -> None:
    """PriorityFloodFlowdirs_Barnes2014 of a contiguous 2-D CUDA tensor (8 / 16 / 32-bit element type) into a uint8 CUDA
    tensor of the same shape, on torch's current stream (the call synchronises: one read-back per nesting level)."""
    import torch

    h, w = _dev2d(dem, "pf_flowdirs_dev")
    if dirs.dtype != torch.uint8 or tuple(dirs.shape) != (h, w) or not dirs.is_contiguous() or not dirs.is_cuda:
        raise RdgpuError("pf_flowdirs_dev: dirs must be a contiguous uint8 CUDA tensor of the DEM's shape")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_pf_flowdirs_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                       ctypes.c_void_p(dirs.data_ptr()), _stream_ptr()), "rdgpu_pf_flowdirs_dev")


class _PfdStats(ctypes.Structure):
    _fields_ = [("levels", ctypes.c_uint32), ("twins", ctypes.c_uint32), ("unresolved", ctypes.c_uint64),
                ("tie_passes", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def pf_flowdirs_stats() -> dict:
    st = _PfdStats()
    check(lib().rdgpu_pf_flowdirs_get_stats(ctypes.byref(st)), "rdgpu_pf_flowdirs_get_stats")
    return {"levels": st.levels, "twins": st.twins, "unresolved": st.unresolved, "tie_passes": st.tie_passes}


def pf_flowdirs(dem: np.ndarray, nodata=-9999) -> np.ndarray:
    """PriorityFloodFlowdirs_Barnes2014 (depressions/Barnes2014.hpp:483-555): uint8 D8 directions in which every cell
    points at the neighbour the (non-raising) flood reached first; NoData cells 0.  Equal to the reference, equal
    elevations included: the reference's stable queue pops equal elevations in order of insertion, and that order is found
    as a fixed point -- the flood runs on the raster's unique ranks of (elevation, discovery time) until the ranks
    reproduce themselves (pf_flowdirs_stats(): "twins" cells with an equal elsewhere, "tie_passes" extra floods; a
    RuntimeWarning only if the passes ran out, "unresolved" != 0)."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("pf_flowdirs: expected a 2-D numpy array")
    dem = np.ascontiguousarray(dem)
    s = _suffix(dem.dtype)
    h, w = dem.shape
    out = np.empty((h, w), np.uint8)
    check(getattr(lib(), f"rdgpu_pf_flowdirs_{s}")(dem.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h,
                                                   out.ctypes.data_as(ctypes.c_void_p)), "rdgpu_pf_flowdirs")
    st = pf_flowdirs_stats()
    if st["unresolved"]:
        import warnings

        if os.environ.get("RDGPU_PFD_RANKS", "1")[:1] == "0":
            why = (f"ties at {st['unresolved']} cells were decided by neighbour number (RDGPU_PFD_RANKS=0, the fast path without the "
                   "reference's insertion order)")
        elif st["tie_passes"] == 0:
            why = "no tie-order pass ran (RDGPU_PFD_TIE_PASSES=0): equal cells were taken in a first-guess order"
        else:
            why = (f"the order of {st['unresolved']} of them among their equals was still moving when the tie-order passes were stopped "
                   f"after {st['tie_passes']} (RDGPU_PFD_TIE_PASSES / RDGPU_PFD_TIE_SECONDS)")
        warnings.warn(f"pf_flowdirs: {st['twins']} cells share their elevation with another cell and {why}: the result is the "
                      "reference's only where those ties do not decide", RuntimeWarning)
    return out


def pit_mask(dem: np.ndarray, nodata, topology="D8") -> np.ndarray:
    """uint8 mask of the cells lying in depressions: 1 = the fill would raise the cell, 0 = not, 3 = NoData
    (reference pit_mask<topo>, depressions/Barnes2014.hpp:593-676; apps/rd_depressions_mask.cpp)."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("pit_mask: expected a 2-D numpy array")
    dem = np.ascontiguousarray(dem)
    s = _suffix(dem.dtype)
    h, w = dem.shape
    out = np.empty((h, w), np.uint8)
    check(getattr(lib(), f"rdgpu_pit_mask_{s}")(dem.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h, _topo(topology),
                                                out.ctypes.data_as(ctypes.c_void_p)), "rdgpu_pit_mask")
    return out


def _elev(dem, who, mfd: bool = False):
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError(f"{who}: expected a 2-D numpy array")
    dem = np.ascontiguousarray(dem)
    try:
        return dem, (_MFD_SUFFIX if mfd else _ELEV_SUFFIX)[dem.dtype]
    except KeyError:
        raise RdgpuError(f"{who}: unsupported elevation dtype {dem.dtype}") from None


def d8_flow_directions(dem: np.ndarray, nodata) -> np.ndarray:
    """uint8 D8 directions (reference d8_flow_directions, flowmet/d8_flowdirs.hpp:96-123)."""
    dem, s = _elev(dem, "d8_flow_directions")
    h, w = dem.shape
    out = np.empty((h, w), np.uint8)
    fn = getattr(lib(), f"rdgpu_d8_flowdirs_{s}")
    check(fn(dem.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h, out.ctypes.data_as(ctypes.c_void_p)),
          "rdgpu_d8_flowdirs")
    return out


def barnes_flat_resolution_d8(dem: np.ndarray, nodata, alter: bool = False) -> np.ndarray:
    """Flat-resolved uint8 D8 directions (reference barnes_flat_resolution_d8(elev, flowdirs, alter=false),
    flats/flat_resolution.hpp:587-605)."""
    if alter:
        if not (isinstance(dem, np.ndarray) and dem.ndim == 2 and dem.flags["C_CONTIGUOUS"]):
            raise RdgpuError("barnes_flat_resolution_d8(alter=True): needs a C-contiguous 2-D array (it is altered in place)")
        h, w = dem.shape
        s = _suffix(dem.dtype)   # integer element types step towards zero, as the reference's nextafterf(e, 0) does
        out = np.empty((h, w), np.uint8)
        fn = getattr(lib(), f"rdgpu_flat_resolution_d8_alter_{s}")
        check(fn(dem.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h, out.ctypes.data_as(ctypes.c_void_p)),
              "rdgpu_flat_resolution_d8_alter")
        return out
    dem, s = _elev(dem, "barnes_flat_resolution_d8")
    h, w = dem.shape
    out = np.empty((h, w), np.uint8)
    fn = getattr(lib(), f"rdgpu_flat_resolution_d8_{s}")
    check(fn(dem.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h, out.ctypes.data_as(ctypes.c_void_p)),
          "rdgpu_flat_resolution_d8")
    return out


def resolve_flats(dem: np.ndarray, nodata):
    """(flat-resolved dirs, flat_mask, flat partition labels) -- exposes resolve_flats_barnes's
    intermediate arrays (flats/flat_resolution.hpp:447-517) for parity tests."""
    dem, s = _elev(dem, "resolve_flats")
    h, w = dem.shape
    dirs = np.empty((h, w), np.uint8)
    mask = np.empty((h, w), np.int32)
    labels = np.empty((h, w), np.int32)
    fn = getattr(lib(), f"rdgpu_resolve_flats_{s}")
    check(fn(dem.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h, dirs.ctypes.data_as(ctypes.c_void_p),
             mask.ctypes.data_as(ctypes.c_void_p), labels.ctypes.data_as(ctypes.c_void_p)), "rdgpu_resolve_flats")
    return dirs, mask, labels


def resolve_flats_epsilon(dem: np.ndarray, nodata, in_place: bool = False):
    """ResolveFlatsEpsilon (reference flats/flats.hpp:21-28, what ``rd.ResolveFlats`` calls): the DEM altered so
    that every flat with an outlet drains.  Returns the altered array (None when ``in_place``)."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("ResolveFlats: expected a 2-D numpy array")
    out = dem if in_place else dem.copy()
    if not out.flags["C_CONTIGUOUS"]:
        if in_place:
            raise RdgpuError("ResolveFlats(in_place=True) needs a C-contiguous array")
        out = np.ascontiguousarray(out)
    try:
        s = _ELEV_SUFFIX[out.dtype]
    except KeyError:
        raise RdgpuError(f"ResolveFlats: unsupported elevation dtype {out.dtype}") from None
    h, w = out.shape
    check(getattr(lib(), f"rdgpu_resolve_flats_epsilon_{s}")(out.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h),
          "rdgpu_resolve_flats_epsilon")
    return None if in_place else out


def d8_flow_accum(dirs: np.ndarray, nodata: int = 255, dtype=np.float64) -> np.ndarray:
    """Cells draining through each cell from uint8 D8 directions (reference d8_flow_accum,
    methods/d8_methods.hpp:47-139)."""
    if not isinstance(dirs, np.ndarray) or dirs.ndim != 2 or dirs.dtype != np.uint8:
        raise RdgpuError("d8_flow_accum: expected a 2-D uint8 array of D8 directions")
    dirs = np.ascontiguousarray(dirs)
    h, w = dirs.shape
    try:
        s = _ACC_SUFFIX[np.dtype(dtype)]
    except KeyError:
        raise RdgpuError(f"d8_flow_accum: unsupported accumulation dtype {dtype}") from None
    out = np.empty((h, w), dtype)
    fn = getattr(lib(), f"rdgpu_d8_flow_accum_{s}")
    check(fn(dirs.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint8(nodata), w, h, out.ctypes.data_as(ctypes.c_void_p)),
          "rdgpu_d8_flow_accum")
    return out


def dinf_flow_directions(dem: np.ndarray, nodata) -> np.ndarray:
    """float32 D-infinity angles (reference dinf_flow_directions, flowmet/dinf_flowdirs.hpp:128-152)."""
    dem, s = _elev(dem, "dinf_flow_directions", mfd=True)
    h, w = dem.shape
    out = np.empty((h, w), np.float32)
    check(getattr(lib(), f"rdgpu_dinf_flowdirs_{s}")(dem.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), w, h,
                                                     out.ctypes.data_as(ctypes.c_void_p)), "rdgpu_dinf_flowdirs")
    return out


# method name -> (kind, code).  Names and aliases as in the reference's Python wrapper
# (wrappers/pyrichdem/richdem/__init__.py:532-549, 693-710).
_METHODS = {
    "Tarboton": ("tarboton", None), "Dinf": ("tarboton", None),
    "D8": ("d8", None), "OCallaghanD8": ("d8", None),
    "Holmgren": ("mfd", 0), "Freeman": ("mfd", 1), "Quinn": ("mfd", 2),
    "D4": ("mfd", 3), "OCallaghanD4": ("mfd", 3),
}
_NEEDS_EXPONENT = ("Holmgren", "Freeman")
_RANDOM_METHODS = ("Rho8", "Rho4", "FairfieldLeymarieD8", "FairfieldLeymarieD4")
VALID_METHODS = ["Tarboton", "Dinf", "Quinn", "FairfieldLeymarieD8", "FairfieldLeymarieD4", "Rho8", "Rho4",
                 "OCallaghanD8", "OCallaghanD4", "D8", "D4", "Freeman", "Holmgren"]


def _method(who: str, method, exponent):
    if method in _RANDOM_METHODS:
        raise RdgpuError(f"{who}: {method} draws from the reference's process-global random engine in raster order; "
                         "its output cannot be reproduced by a parallel engine and is not provided")
    if method not in _METHODS:
        raise RdgpuError(f"Invalid {who} method. Valid methods are: " + ", ".join(VALID_METHODS))
    if method in _NEEDS_EXPONENT and exponent is None:
        raise RdgpuError(f'{who} method "{method}" requires an exponent!')
    kind, code = _METHODS[method]
    return kind, code, float(exponent) if (exponent is not None and method in _NEEDS_EXPONENT) else 1.0


def _flats_kind(who: str, method, kind: str, resolve_flats: bool) -> str:
    """the C-ABI family of a D-infinity call: across flats (``resolve_flats``) or plain; every other method refuses it"""
    if not resolve_flats:
        return kind
    if kind != "tarboton":
        raise RdgpuError(f'{who}: resolve_flats=True is available for "Dinf" / "Tarboton" only, not for method "{method}"')
    return "tarboton_flats"


def FlowProportions(dem: np.ndarray, method: str = "Dinf", nodata=-9999, exponent=None, *, resolve_flats: bool = False) -> np.ndarray:
    """[h, w, 9] float32 flow proportions (reference ``rd.FlowProportions`` -> FM_Tarboton / FM_D8 /
    FM_Holmgren / FM_Freeman / FM_Quinn / FM_D4, flowmet/*.hpp).  resolve_flats ("Dinf" / "Tarboton" only): the cells of
    drainable flats are routed over Barnes' flat mask (fm_tarboton_flats)."""
    kind, code, xp = _method("FlowProportions", method, exponent)
    kind = _flats_kind("FlowProportions", method, kind, resolve_flats)
    dem, s = _elev(dem, "FlowProportions", mfd=kind != "d8")
    h, w = dem.shape
    out = np.empty((h, w, 9), np.float32)
    pd, po = dem.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    if kind == "mfd":
        check(getattr(lib(), f"rdgpu_fm_mfd_{s}")(pd, _scalar(s, nodata), w, h, code, ctypes.c_double(xp), po), "rdgpu_fm_mfd")
    else:
        check(getattr(lib(), f"rdgpu_fm_{kind}_{s}")(pd, _scalar(s, nodata), w, h, po), "rdgpu_fm_" + kind)
    return out


def FlowAccumFromProps(props: np.ndarray, weights: np.ndarray | None = None) -> np.ndarray:
    """Generic accumulation over a 9-float proportions array (reference ``rd.FlowAccumFromProps`` ->
    FlowAccumulation, methods/flow_accumulation_generic.hpp:33-100)."""
    if not isinstance(props, np.ndarray) or props.ndim != 3 or props.shape[2] != 9:
        raise RdgpuError("FlowAccumFromProps: expected an [h, w, 9] array")
    props = np.ascontiguousarray(props, dtype=np.float32)
    h, w, _ = props.shape
    if weights is None:
        acc = np.ones((h, w), np.float64)
    else:
        if weights.shape != (h, w):
            raise RdgpuError("Accumulation array must have same dimensions as proportions array!")
        acc = np.ascontiguousarray(weights, dtype=np.float64).copy()
    check(lib().rdgpu_flow_accumulation_f64(props.ctypes.data_as(ctypes.c_void_p), w, h,
                                            acc.ctypes.data_as(ctypes.c_void_p)), "rdgpu_flow_accumulation_f64")
    return acc


def flow_accumulation_into(dem: np.ndarray, method, nodata, acc: np.ndarray, exponent=None, *, resolve_flats: bool = False) -> None:
    """FA_<method>(dem, acc): acc (float64, C-contiguous, dem's shape) holds the flow generated per cell on
    entry and the accumulation on return (methods/flow_accumulation.hpp:16-28).  resolve_flats: as FlowProportions."""
    kind, code, xp = _method("FlowAccumulation", method, exponent)
    kind = _flats_kind("FlowAccumulation", method, kind, resolve_flats)
    dem, s = _elev(dem, "FlowAccumulation", mfd=kind != "d8")
    h, w = dem.shape
    if acc.shape != dem.shape:                     # flow_accumulation_generic.hpp:42-43
        raise RdgpuError("Accumulation array must have same dimensions as proportions array!")
    if acc.dtype != np.float64 or not acc.flags["C_CONTIGUOUS"]:
        raise RdgpuError("Accumulation array must be of type 'float64'!")
    pd, pa = dem.ctypes.data_as(ctypes.c_void_p), acc.ctypes.data_as(ctypes.c_void_p)
    if kind == "mfd":
        check(getattr(lib(), f"rdgpu_fa_mfd_{s}")(pd, _scalar(s, nodata), w, h, code, ctypes.c_double(xp), pa), "rdgpu_fa_mfd")
    else:
        check(getattr(lib(), f"rdgpu_fa_{kind}_{s}")(pd, _scalar(s, nodata), w, h, pa), "rdgpu_fa_" + kind)


def FlowAccumulation(dem: np.ndarray, method: str = "D8", nodata=-9999, weights: np.ndarray | None = None, exponent=None, *,
                     resolve_flats: bool = False):
    """Flow accumulation (reference ``rd.FlowAccumulation(dem, method, exponent, weights)``,
    wrappers/pyrichdem/richdem/__init__.py:490-597 -> FA_D8 etc., methods/flow_accumulation.hpp:16-28).
    Returns float64 accumulation; NoData cells get -1.  resolve_flats: as FlowProportions."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("FlowAccumulation: expected a 2-D numpy array")
    if weights is None:
        kind, _, _ = _method("FlowAccumulation", method, exponent)
        _flats_kind("FlowAccumulation", method, kind, resolve_flats)
        if kind == "d8":                           # every cell generates 1 (__init__.py:560-563) and THIS code knows it:
            d, s = _elev(dem, "FlowAccumulation", mfd=False)   # the unit-weights entry neither reads nor uploads an array of ones
            acc = np.empty(d.shape, np.float64)
            check(getattr(lib(), f"rdgpu_fa_d8_unit_{s}")(d.ctypes.data_as(ctypes.c_void_p), _scalar(s, nodata), d.shape[1], d.shape[0],
                                                          acc.ctypes.data_as(ctypes.c_void_p)), "rdgpu_fa_d8_unit")
            return acc
        acc = np.ones(dem.shape, np.float64)
    else:
        if weights.shape != dem.shape:             # flow_accumulation_generic.hpp:42-43
            raise RdgpuError("Accumulation array must have same dimensions as proportions array!")
        acc = np.ascontiguousarray(weights, dtype=np.float64).copy()
    flow_accumulation_into(dem, method, nodata, acc, exponent, resolve_flats=resolve_flats)
    return acc


# ---- HBM-resident variants (torch tensors on the GPU) ---------------------------------------
def _torch_suffix(t) -> str:
    import torch

    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32",
         torch.float64: "f64", torch.int64: "i64"}
    if t.dtype not in m:
        raise RdgpuError(f"unsupported tensor dtype {t.dtype}")
    return m[t.dtype]


def _stream_ptr():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def fill_depressions_dev(dem, topology="D8") -> None:
    """In-place fill of a 2-D contiguous CUDA(HIP) tensor, on torch's current stream."""
    if not (dem.is_cuda and dem.dim() == 2 and dem.is_contiguous()):
        raise RdgpuError("fill_depressions_dev: expected a contiguous 2-D tensor on the GPU")
    h, w = dem.shape
    fn = getattr(lib(), f"rdgpu_fill_dev_{_torch_suffix(dem)}")
    check(fn(ctypes.c_void_p(dem.data_ptr()), w, h, _topo(topology), _stream_ptr()), "rdgpu_fill_dev")


def synth_dem_dev(out, seed: int, x0: int = 0, y0: int = 0, tilt: float = 0.0) -> None:
    """Fill a float32 CUDA tensor [h, w] with the seeded fractal DEM G(seed) (bench/test input)."""
    import torch

    if not (out.is_cuda and out.dim() == 2 and out.is_contiguous() and out.dtype == torch.float32):
        raise RdgpuError("synth_dem_dev: expected a contiguous 2-D float32 tensor on the GPU")
    h, w = out.shape
    check(
        lib().rdgpu_synth_dem_dev_f32(
            ctypes.c_void_p(out.data_ptr()), w, h, int(seed), int(x0), int(y0), ctypes.c_float(tilt), _stream_ptr()
        ),
        "rdgpu_synth_dem_dev_f32",
    )


def _dev2d(t, who, dtype=None):
    if not (t.is_cuda and t.dim() == 2 and t.is_contiguous()):
        raise RdgpuError(f"{who}: expected a contiguous 2-D tensor on the GPU")
    if dtype is not None and t.dtype != dtype:
        raise RdgpuError(f"{who}: expected dtype {dtype}, got {t.dtype}")
    return t.shape


def _torch_elev_suffix(t) -> str:
    import torch

    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32",
         torch.float64: "f64", torch.int64: "i64"}
    if t.dtype not in m:
        raise RdgpuError(f"unsupported tensor dtype {t.dtype}")
    return m[t.dtype]


def d8_flow_directions_dev(dem, nodata, dirs, flats: bool = False) -> None:
    """dirs (uint8 CUDA tensor) <- D8 directions of dem; flats=True also resolves flats
    (barnes_flat_resolution_d8, alter=false)."""
    import torch

    h, w = _dev2d(dem, "d8_flow_directions_dev")
    if _dev2d(dirs, "d8_flow_directions_dev", torch.uint8) != (h, w):
        raise RdgpuError("d8_flow_directions_dev: shape mismatch")
    s = _torch_elev_suffix(dem)
    name = f"rdgpu_flat_resolution_d8_dev_{s}" if flats else f"rdgpu_d8_flowdirs_dev_{s}"
    check(getattr(lib(), name)(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h, ctypes.c_void_p(dirs.data_ptr()),
                               _stream_ptr()), name)


def d8_flow_accum_dev(dirs, area, nodata: int = 255) -> None:
    import torch

    h, w = _dev2d(dirs, "d8_flow_accum_dev", torch.uint8)
    if _dev2d(area, "d8_flow_accum_dev") != (h, w):
        raise RdgpuError("d8_flow_accum_dev: shape mismatch")
    s = {torch.int32: "i32", torch.float32: "f32", torch.float64: "f64"}.get(area.dtype)
    if s is None:
        raise RdgpuError(f"d8_flow_accum_dev: unsupported accumulation dtype {area.dtype}")
    check(getattr(lib(), f"rdgpu_d8_flow_accum_dev_{s}")(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(nodata), w, h,
                                                         ctypes.c_void_p(area.data_ptr()), _stream_ptr()),
          "rdgpu_d8_flow_accum_dev")


def fa_d8_dev(dem, nodata, accum, unit_weights: bool = False) -> None:
    """accum (float64 CUDA tensor, pre-loaded with per-cell weights) <- FA_D8 accumulation.  unit_weights=True: the caller
    guarantees that every weight is 1 (accum is then output only; the engine does not read the weights to find out)."""
    import torch

    h, w = _dev2d(dem, "fa_d8_dev")
    if _dev2d(accum, "fa_d8_dev", torch.float64) != (h, w):
        raise RdgpuError("Accumulation array must have same dimensions as proportions array!")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_fa_d8_unit_dev_{s}" if unit_weights else f"rdgpu_fa_d8_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                 ctypes.c_void_p(accum.data_ptr()), _stream_ptr()), "rdgpu_fa_d8_dev")


def resolve_flats_epsilon_dev(dem, nodata) -> None:
    """In-place ResolveFlatsEpsilon (flats/flats.hpp:21-28) of a contiguous 2-D CUDA tensor, on torch's current stream."""
    h, w = _dev2d(dem, "resolve_flats_epsilon_dev")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_resolve_flats_epsilon_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                               _stream_ptr()), "rdgpu_resolve_flats_epsilon_dev")


class _FlatStats(ctypes.Structure):
    _fields_ = [("low", ctypes.c_uint64), ("high", ctypes.c_uint64), ("noflow", ctypes.c_uint64),
                ("away", ctypes.c_uint32), ("towards", ctypes.c_uint32)]


class _FlatAsyncStats(ctypes.Structure):
    _fields_ = [("visits", ctypes.c_uint64), ("launches", ctypes.c_uint32), ("failures", ctypes.c_uint32),
                ("live_tiles", ctypes.c_uint32), ("plane_repeats", ctypes.c_uint32)]


def flat_stats() -> dict:
    """rdgpu_flat_get_stats + rdgpu_flat_get_async_stats of the last flat resolution on this thread."""
    st = _FlatStats()
    check(lib().rdgpu_flat_get_stats(ctypes.byref(st)), "rdgpu_flat_get_stats")
    a = _FlatAsyncStats()
    check(lib().rdgpu_flat_get_async_stats(ctypes.byref(a)), "rdgpu_flat_get_async_stats")
    return {"low_edges": st.low, "high_edges": st.high, "noflow": st.noflow, "away": st.away, "towards": st.towards,
            "tail_visits": a.visits, "tail_live_tiles": a.live_tiles, "tail_launches": a.launches, "tail_failures": a.failures,
            "plane_repeats": a.plane_repeats}


def release_workspace() -> None:
    """Free the grow-only device workspace cached between calls (rdgpu_release_workspace)."""
    check(lib().rdgpu_release_workspace(), "rdgpu_release_workspace")


def fill_epsilon_dev(dem, nodata, topology="D8") -> None:
    """In-place PriorityFloodEpsilon of a contiguous 2-D float32 / float64 CUDA tensor, on torch's current stream."""
    import torch

    h, w = _dev2d(dem, "fill_epsilon_dev")
    if dem.dtype not in (torch.float32, torch.float64):
        raise RdgpuError("Priority-Flood+Epsilon is only available for floating-point data types!")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_fill_epsilon_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                        _topo(topology), _stream_ptr()), "rdgpu_fill_epsilon_dev")


def dinf_flow_directions_dev(dem, nodata, angles) -> None:
    """dinf_flow_directions (flowmet/dinf_flowdirs.hpp:128-152) of a contiguous 2-D CUDA tensor into a float32 CUDA tensor
    of the same shape, on torch's current stream."""
    import torch

    h, w = _dev2d(dem, "dinf_flow_directions_dev")
    if angles.dtype != torch.float32 or tuple(angles.shape) != (h, w) or not angles.is_contiguous() or not angles.is_cuda:
        raise RdgpuError("dinf_flow_directions_dev: angles must be a contiguous float32 CUDA tensor of the DEM's shape")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_dinf_flowdirs_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                         ctypes.c_void_p(angles.data_ptr()), _stream_ptr()), "rdgpu_dinf_flowdirs_dev")


def fa_tarboton_dev(dem, nodata, accum) -> None:
    """FA_Tarboton / FA_Dinfinity (methods/flow_accumulation.hpp:16-17): accum (float64 CUDA tensor, in: the cells' weights,
    out: the accumulation) from the DEM, on torch's current stream."""
    import torch

    h, w = _dev2d(dem, "fa_tarboton_dev")
    if accum.dtype != torch.float64 or tuple(accum.shape) != (h, w) or not accum.is_contiguous() or not accum.is_cuda:
        raise RdgpuError("fa_tarboton_dev: accum must be a contiguous float64 CUDA tensor of the DEM's shape")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_fa_tarboton_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                       ctypes.c_void_p(accum.data_ptr()), _stream_ptr()), "rdgpu_fa_tarboton_dev")


def flow_accumulation_rounds() -> int:
    """Launches of the work-list kernels (k_wl_buffer / k_wl_stack, csrc/mfd_worklist.hpp) in the last generic accumulation --
    FlowAccumFromProps, FA_Tarboton, FA_Holmgren / Freeman / Quinn / D4 and their _dev forms (rdgpu_flow_accumulation_rounds)."""
    r = ctypes.c_uint32()
    check(lib().rdgpu_flow_accumulation_rounds(ctypes.byref(r)), "rdgpu_flow_accumulation_rounds")
    return int(r.value)


def flow_accumulation_dev(props9, accum) -> None:
    """FlowAccumulation(Array3D<float>, Array2D<double>) (methods/flow_accumulation_generic.hpp:33-100): accum (float64 CUDA
    tensor [h, w], in: the cells' weights, out: the accumulation) from the float32 CUDA proportions tensor [h, w, 9], on
    torch's current stream."""
    import torch

    if not (props9.is_cuda and props9.dim() == 3 and props9.shape[2] == 9 and props9.is_contiguous()
            and props9.dtype == torch.float32):
        raise RdgpuError("flow_accumulation_dev: props9 must be a contiguous float32 CUDA tensor [h, w, 9]")
    h, w = int(props9.shape[0]), int(props9.shape[1])
    if accum.dtype != torch.float64 or tuple(accum.shape) != (h, w) or not accum.is_contiguous() or not accum.is_cuda:
        raise RdgpuError("flow_accumulation_dev: accum must be a contiguous float64 CUDA tensor of the proportions' shape")
    check(lib().rdgpu_flow_accumulation_dev_f64(ctypes.c_void_p(props9.data_ptr()), w, h, ctypes.c_void_p(accum.data_ptr()),
                                                _stream_ptr()), "rdgpu_flow_accumulation_dev_f64")


def fa_mfd_dev(dem, nodata, method, accum, exponent=None) -> None:
    """FA_Holmgren / FA_Freeman / FA_Quinn / FA_D4 (methods/flow_accumulation.hpp:18-20,28): accum (float64 CUDA tensor, in:
    the cells' weights, out: the accumulation) from the DEM, on torch's current stream."""
    import torch

    kind, code, xp = _method("fa_mfd_dev", method, exponent)
    if kind != "mfd":
        raise RdgpuError("fa_mfd_dev: method must be Holmgren, Freeman, Quinn or D4 (D8: fa_d8_dev, Dinf: fa_tarboton_dev)")
    h, w = _dev2d(dem, "fa_mfd_dev")
    if accum.dtype != torch.float64 or tuple(accum.shape) != (h, w) or not accum.is_contiguous() or not accum.is_cuda:
        raise RdgpuError("fa_mfd_dev: accum must be a contiguous float64 CUDA tensor of the DEM's shape")
    s = _torch_elev_suffix(dem)
    if s not in _MFD_SUFFIX.values():
        raise RdgpuError(f"fa_mfd_dev: unsupported elevation dtype {dem.dtype}")
    check(getattr(lib(), f"rdgpu_fa_mfd_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h, code,
                                                  ctypes.c_double(xp), ctypes.c_void_p(accum.data_ptr()), _stream_ptr()),
          "rdgpu_fa_mfd_dev")


class _MaxDepStats(ctypes.Structure):
    _fields_ = [("pockets", ctypes.c_uint64), ("tie_pockets", ctypes.c_uint64), ("tie_cluster_cells", ctypes.c_uint64),
                ("pocket_cells", ctypes.c_uint64)]


def max_dep_stats() -> dict:
    """Tie census of the calling thread's last max_dep fill: pockets, pockets that several cells of their spill elevation
    can flood (there the reference's heap order decides the grouping), and the cells of the clusters they touch."""
    st = _MaxDepStats()
    check(lib().rdgpu_fill_max_dep_get_stats(ctypes.byref(st)), "rdgpu_fill_max_dep_get_stats")
    return {k: int(getattr(st, k)) for k, _ in _MaxDepStats._fields_}


def fill_max_dep_ties_dev(dem, max_dep_size: int, tie_mask, topology="D8") -> None:
    """fill_max_dep_dev + the cells of tie-flagged pocket clusters as a uint8 CUDA tensor (1 = the reference's heap order can
    decide this cell, 0 = order free)."""
    import torch

    h, w = _dev2d(dem, "fill_max_dep_ties_dev")
    if tie_mask.dtype != torch.uint8 or tuple(tie_mask.shape) != (h, w) or not tie_mask.is_contiguous() or not tie_mask.is_cuda:
        raise RdgpuError("fill_max_dep_ties_dev: tie_mask must be a contiguous uint8 CUDA tensor of the DEM's shape")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_fill_max_dep_ties_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), w, h, _topo(topology),
                                                             ctypes.c_uint64(int(max_dep_size)), ctypes.c_void_p(tie_mask.data_ptr()),
                                                             _stream_ptr()), "rdgpu_fill_max_dep_ties_dev")


def fill_max_dep_dev(dem, max_dep_size: int, topology="D8") -> None:
    """In-place PriorityFlood_Barnes2014_max_dep of a contiguous 2-D CUDA tensor, on torch's current stream."""
    h, w = _dev2d(dem, "fill_max_dep_dev")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_fill_max_dep_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), w, h, _topo(topology),
                                                        ctypes.c_uint64(int(max_dep_size)), _stream_ptr()), "rdgpu_fill_max_dep_dev")


def watersheds_dev(dem, nodata, labels, topology="D8", alter: bool = False) -> None:
    """PriorityFloodWatersheds_Barnes2014 of a contiguous 2-D CUDA tensor into an int32 CUDA tensor of the same shape
    (``alter``: the DEM is filled in place), on torch's current stream."""
    import torch

    h, w = _dev2d(dem, "watersheds_dev")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (h, w) or not labels.is_contiguous() or not labels.is_cuda:
        raise RdgpuError("watersheds_dev: labels must be a contiguous int32 CUDA tensor of the DEM's shape")
    s = _torch_elev_suffix(dem)
    check(getattr(lib(), f"rdgpu_watersheds_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h, _topo(topology),
                                                      1 if alter else 0, ctypes.c_void_p(labels.data_ptr()), _stream_ptr()),
          "rdgpu_watersheds_dev")


class _EpsStats(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_uint32), ("attempts", ctypes.c_uint32), ("tile_relaxations", ctypes.c_uint64),
                ("slack", ctypes.c_uint64), ("max_lift", ctypes.c_uint64), ("tie_sources", ctypes.c_uint64)]


def epsilon_stats() -> dict:
    st = _EpsStats()
    check(lib().rdgpu_fill_epsilon_get_stats(ctypes.byref(st)), "rdgpu_fill_epsilon_get_stats")
    return {k: getattr(st, k) for k, _ in _EpsStats._fields_}


# ---- TerrainAttribute: slope, aspect, curvature, SPI, CTI (reference methods/terrain_attributes.hpp) ---------------------
#: the reference's attribute names (wrappers/pyrichdem/richdem/__init__.py TerrainAttribute), in RDGPU_TA_* id order
TERRAIN_ATTRIBUTES = ("slope_riserun", "slope_percentage", "slope_degrees", "slope_radians", "aspect", "curvature",
                      "planform_curvature", "profile_curvature")


def _ta_id(attrib) -> int:
    if attrib not in TERRAIN_ATTRIBUTES:
        raise RdgpuError("Invalid TerrainAttributes attribute. Valid attributes are: " + ", ".join(TERRAIN_ATTRIBUTES))
    return TERRAIN_ATTRIBUTES.index(attrib)


def _ta_meta(dem, nodata, cell):
    """an rdarray supplies no_data and, through its geotransform, the cell lengths |gt[1]|, |gt[5]|"""
    if nodata is None:
        nodata = getattr(dem, "no_data", None)
    if nodata is None:
        raise RdgpuError("terrain attributes: a no_data value is required (nodata=, or an rdarray input)")
    if cell is None:
        gt = getattr(dem, "geotransform", None)
        cell = (abs(float(gt[1])), abs(float(gt[5]))) if gt is not None and len(gt) == 6 else (1.0, 1.0)
    return nodata, (float(cell[0]), float(cell[1]))


def _ta_scalar(s: str, nodata):
    """_scalar, except that an integer no_data of an integer DEM is taken exactly (64-bit values above 2**53 do not survive
    the trip through a double that _scalar makes)"""
    if s not in ("f32", "f64") and isinstance(nodata, (int, np.integer)) and not isinstance(nodata, bool):
        bits = 8 * np.dtype(_NP[s]).itemsize
        v = int(nodata) & ((1 << bits) - 1)
        if np.issubdtype(_NP[s], np.signedinteger) and v >= 1 << (bits - 1):
            v -= 1 << bits
        return _CT[s](v)
    return _scalar(s, nodata)


def _ta_ids(attribs):
    ids = [_ta_id(a) for a in attribs]
    if not ids or len(set(ids)) != len(ids):
        raise RdgpuError("terrain_attributes: expected a non-empty list of distinct attribute names")
    return ids


def terrain_attributes(dem: np.ndarray, attribs, nodata=None, zscale: float = 1.0, cell=None, out_nodata=-9999) -> dict:
    """{name: float32 array} of several terrain attributes from ONE launch, one read of the DEM (reference TA_* of
    methods/terrain_attributes.hpp, each bit for bit what the single calls give)."""
    ids = _ta_ids(list(attribs))
    nodata, cell = _ta_meta(dem, nodata, cell)
    dem, s = _elev(np.asarray(dem), "terrain_attribute")
    h, w = dem.shape
    outs = {k: np.empty((h, w), np.float32) for k in ids}
    ptrs = (ctypes.c_void_p * len(TERRAIN_ATTRIBUTES))()
    for k, a in outs.items():
        ptrs[k] = a.ctypes.data
    mask = sum(1 << k for k in ids)
    check(getattr(lib(), f"rdgpu_terrain_attributes_{s}")(dem.ctypes.data_as(ctypes.c_void_p), _ta_scalar(s, nodata), w, h,
                                                          ctypes.c_double(cell[0]), ctypes.c_double(cell[1]),
                                                          ctypes.c_float(zscale), ctypes.c_uint(mask), ptrs,
                                                          ctypes.c_float(out_nodata)), "rdgpu_terrain_attributes")
    return {TERRAIN_ATTRIBUTES[k]: outs[k] for k in ids}


def terrain_attribute(dem: np.ndarray, attrib: str, nodata=None, zscale: float = 1.0, cell=None, out_nodata=-9999) -> np.ndarray:
    """float32 terrain attribute of ``dem`` (reference TerrainAttribute(dem, attrib, zscale)): ``attrib`` is one of
    TERRAIN_ATTRIBUTES; ``cell`` = (cellX, cellY), (1, 1) unless an rdarray's geotransform says otherwise; NoData cells get
    ``out_nodata`` (the reference's Python wrapper passes -9999)."""
    k = _ta_id(attrib)
    nodata, cell = _ta_meta(dem, nodata, cell)
    dem, s = _elev(np.asarray(dem), "terrain_attribute")
    h, w = dem.shape
    out = np.empty((h, w), np.float32)
    check(getattr(lib(), f"rdgpu_terrain_attribute_{s}")(dem.ctypes.data_as(ctypes.c_void_p), _ta_scalar(s, nodata), w, h,
                                                         ctypes.c_double(cell[0]), ctypes.c_double(cell[1]),
                                                         ctypes.c_float(zscale), k, out.ctypes.data_as(ctypes.c_void_p),
                                                         ctypes.c_float(out_nodata)), "rdgpu_terrain_attribute")
    return out


def _spi_cti(which, accum, slope, accum_nodata, slope_nodata, cell):
    if accum_nodata is None:
        accum_nodata = getattr(accum, "no_data", None)
    if slope_nodata is None:
        slope_nodata = getattr(slope, "no_data", None)
    if accum_nodata is None or slope_nodata is None:
        raise RdgpuError(f"terrain_{which}: the no_data values of the accumulation and of the slope are required")
    _, cell = _ta_meta(accum, accum_nodata, cell)
    accum, slope = np.asarray(accum), np.asarray(slope)
    if accum.ndim != 2 or slope.ndim != 2 or accum.shape != slope.shape:   # the reference's message
        raise RdgpuError(f"Couldn't calculate {which.upper()}! The input matricies were of unequal dimensions!")
    accum = np.ascontiguousarray(accum, np.float64)
    slope = np.ascontiguousarray(slope, np.float32)
    h, w = accum.shape
    out = np.empty((h, w), np.float32)
    check(getattr(lib(), f"rdgpu_ta_{which}")(accum.ctypes.data_as(ctypes.c_void_p), ctypes.c_double(accum_nodata),
                                              slope.ctypes.data_as(ctypes.c_void_p), ctypes.c_float(slope_nodata), w, h,
                                              ctypes.c_double(cell[0]), ctypes.c_double(cell[1]),
                                              out.ctypes.data_as(ctypes.c_void_p)), f"rdgpu_ta_{which}")
    return out


def terrain_spi(accum, slope, accum_nodata=None, slope_nodata=None, cell=None) -> np.ndarray:
    """log((accum / cellArea) * (slope + 0.001)) as float32 (reference TA_SPI); NoData in either input gives -1."""
    return _spi_cti("spi", accum, slope, accum_nodata, slope_nodata, cell)


def terrain_cti(accum, slope, accum_nodata=None, slope_nodata=None, cell=None) -> np.ndarray:
    """log((accum / cellArea) / (slope + 0.001)) as float32 (reference TA_CTI); NoData in either input gives -1."""
    return _spi_cti("cti", accum, slope, accum_nodata, slope_nodata, cell)


def _torch_ta_suffix(t) -> str:
    import torch

    m = {getattr(torch, n): s for n, s in (("uint16", "u16"), ("uint32", "u32"), ("uint64", "u64")) if hasattr(torch, n)}
    return m[t.dtype] if t.dtype in m else _torch_elev_suffix(t)


def terrain_attributes_dev(dem, attribs, nodata, outs, zscale: float = 1.0, cell=(1.0, 1.0), out_nodata=-9999) -> None:
    """outs[name] (float32 CUDA tensors of the DEM's shape) <- the attributes ``attribs`` of the CUDA tensor ``dem``, all
    from one launch on torch's current stream."""
    import torch

    ids = _ta_ids(list(attribs))
    h, w = _dev2d(dem, "terrain_attributes_dev")
    ptrs = (ctypes.c_void_p * len(TERRAIN_ATTRIBUTES))()
    for k in ids:
        o = outs[TERRAIN_ATTRIBUTES[k]]
        if _dev2d(o, "terrain_attributes_dev", torch.float32) != (h, w):
            raise RdgpuError("terrain_attributes_dev: shape mismatch")
        ptrs[k] = o.data_ptr()
    s = _torch_ta_suffix(dem)
    check(getattr(lib(), f"rdgpu_terrain_attributes_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _ta_scalar(s, nodata), w, h,
                                                              ctypes.c_double(cell[0]), ctypes.c_double(cell[1]),
                                                              ctypes.c_float(zscale), ctypes.c_uint(sum(1 << k for k in ids)),
                                                              ptrs, ctypes.c_float(out_nodata), _stream_ptr()),
          "rdgpu_terrain_attributes_dev")


def terrain_attribute_dev(dem, attrib: str, nodata, out, zscale: float = 1.0, cell=(1.0, 1.0), out_nodata=-9999) -> None:
    """out (float32 CUDA tensor) <- one terrain attribute of the CUDA tensor ``dem``, on torch's current stream."""
    import torch

    k = _ta_id(attrib)
    h, w = _dev2d(dem, "terrain_attribute_dev")
    if _dev2d(out, "terrain_attribute_dev", torch.float32) != (h, w):
        raise RdgpuError("terrain_attribute_dev: shape mismatch")
    s = _torch_ta_suffix(dem)
    check(getattr(lib(), f"rdgpu_terrain_attribute_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _ta_scalar(s, nodata), w, h,
                                                             ctypes.c_double(cell[0]), ctypes.c_double(cell[1]),
                                                             ctypes.c_float(zscale), k, ctypes.c_void_p(out.data_ptr()),
                                                             ctypes.c_float(out_nodata), _stream_ptr()),
          "rdgpu_terrain_attribute_dev")


def _spi_cti_dev(which, accum, slope, out, accum_nodata, slope_nodata, cell):
    import torch

    if accum.dim() != 2 or slope.dim() != 2 or tuple(accum.shape) != tuple(slope.shape):
        raise RdgpuError(f"Couldn't calculate {which.upper()}! The input matricies were of unequal dimensions!")
    h, w = _dev2d(accum, f"terrain_{which}_dev", torch.float64)
    _dev2d(slope, f"terrain_{which}_dev", torch.float32)
    if _dev2d(out, f"terrain_{which}_dev", torch.float32) != (h, w):
        raise RdgpuError(f"terrain_{which}_dev: shape mismatch")
    check(getattr(lib(), f"rdgpu_ta_{which}_dev")(ctypes.c_void_p(accum.data_ptr()), ctypes.c_double(accum_nodata),
                                                  ctypes.c_void_p(slope.data_ptr()), ctypes.c_float(slope_nodata), w, h,
                                                  ctypes.c_double(cell[0]), ctypes.c_double(cell[1]),
                                                  ctypes.c_void_p(out.data_ptr()), _stream_ptr()), f"rdgpu_ta_{which}_dev")


def terrain_spi_dev(accum, slope, out, accum_nodata=-1.0, slope_nodata=-9999.0, cell=(1.0, 1.0)) -> None:
    """out (float32) <- TA_SPI of a float64 accumulation and a float32 rise/run slope, CUDA tensors, current stream."""
    _spi_cti_dev("spi", accum, slope, out, accum_nodata, slope_nodata, cell)


def terrain_cti_dev(accum, slope, out, accum_nodata=-1.0, slope_nodata=-9999.0, cell=(1.0, 1.0)) -> None:
    """out (float32) <- TA_CTI of a float64 accumulation and a float32 rise/run slope, CUDA tensors, current stream."""
    _spi_cti_dev("cti", accum, slope, out, accum_nodata, slope_nodata, cell)


# ---- upslope cells, catchments, outlets (csrc/upslope.hip) -----------------------------------
def _dirs2d(dirs, who):
    if not isinstance(dirs, np.ndarray) or dirs.ndim != 2 or dirs.dtype != np.uint8:
        raise RdgpuError(f"{who}: expected a 2-D uint8 array of D8 directions")
    return np.ascontiguousarray(dirs)


def _seed_cells(seed_cells, w, h, who) -> np.ndarray:
    """flat indices, or an (n, 2) array of (x, y); a cell outside the raster is an error"""
    c = np.asarray(seed_cells)
    if c.size == 0:
        return np.zeros(0, np.uint32)
    if c.dtype.kind not in "iu":
        raise RdgpuError(f"{who}: seed cells must be integers")
    c = c.astype(np.int64)
    if c.ndim == 2 and c.shape[1] == 2:
        if ((c[:, 0] < 0) | (c[:, 0] >= w) | (c[:, 1] < 0) | (c[:, 1] >= h)).any():
            raise RdgpuError(f"{who}: a seed cell lies outside the raster")
        c = c[:, 1] * w + c[:, 0]
    elif c.ndim != 1:
        raise RdgpuError(f"{who}: seed cells are flat indices or an (n, 2) array of (x, y)")
    if ((c < 0) | (c >= w * h)).any():
        raise RdgpuError(f"{who}: a seed cell lies outside the raster")
    return np.ascontiguousarray(c, np.uint32)


def d8_upslope_line(shape, x0: int, y0: int, x1: int, y1: int) -> np.ndarray:
    """Flat indices of the cells the reference's d8_upslope_cells marks for the line (x0,y0)-(x1,y1) on a raster of
    shape (height, width), in its order (rdgpu_d8_upslope_line: host code, no GPU).  Raises where the line would leave
    the raster."""
    h, w = int(shape[0]), int(shape[1])
    n = ctypes.c_uint32(0)
    fn = lib().rdgpu_d8_upslope_line
    check(fn(w, h, int(x0), int(y0), int(x1), int(y1), None, ctypes.c_uint32(0), ctypes.byref(n)), "rdgpu_d8_upslope_line")
    cells = np.empty(n.value, np.uint32)
    check(fn(w, h, int(x0), int(y0), int(x1), int(y1), cells.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(n.value),
             ctypes.byref(n)), "rdgpu_d8_upslope_line")
    return cells


def d8_upslope_cells(dirs: np.ndarray, x0: int, y0: int, x1: int, y1: int, nodata: int = 255) -> np.ndarray:
    """uint8 raster: 2 on the line's cells, 1 on every cell that drains through one, 255 elsewhere (reference
    d8_upslope_cells, methods/d8_methods.hpp:144-236)."""
    dirs = _dirs2d(dirs, "d8_upslope_cells")
    h, w = dirs.shape
    out = np.empty((h, w), np.uint8)
    check(lib().rdgpu_d8_upslope_cells(dirs.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint8(nodata), w, h, int(x0), int(y0),
                                       int(x1), int(y1), out.ctypes.data_as(ctypes.c_void_p)), "rdgpu_d8_upslope_cells")
    return out


def d8_catchments(dirs: np.ndarray, seed_cells, seed_labels, unreached: int = 0, nodata: int = 255) -> np.ndarray:
    """int32 raster: the label of the first seed on every cell's flow path, `unreached` where there is none.  seed_cells:
    flat indices or an (n, 2) array of (x, y); of two entries for one cell the first wins."""
    dirs = _dirs2d(dirs, "d8_catchments")
    h, w = dirs.shape
    cells = _seed_cells(seed_cells, w, h, "d8_catchments")
    labels = np.ascontiguousarray(np.asarray(seed_labels).reshape(-1), np.int32)
    if labels.size != cells.size:
        raise RdgpuError("d8_catchments: one label per seed cell")
    out = np.empty((h, w), np.int32)
    check(lib().rdgpu_d8_catchments(dirs.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint8(nodata), w, h,
                                    cells.ctypes.data_as(ctypes.c_void_p), labels.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.c_uint32(cells.size), ctypes.c_int32(unreached),
                                    out.ctypes.data_as(ctypes.c_void_p)), "rdgpu_d8_catchments")
    return out


def d8_outlets(dirs: np.ndarray, nodata: int = 255) -> np.ndarray:
    """uint32 raster: the flat index of the cell every cell finally drains to (one id per drainage basin); 0xFFFFFFFF on
    NoData cells and on cells that drain into a direction loop."""
    dirs = _dirs2d(dirs, "d8_outlets")
    h, w = dirs.shape
    out = np.empty((h, w), np.uint32)
    check(lib().rdgpu_d8_outlets(dirs.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint8(nodata), w, h,
                                 out.ctypes.data_as(ctypes.c_void_p)), "rdgpu_d8_outlets")
    return out


def d8_upslope_cells_dev(dirs, x0: int, y0: int, x1: int, y1: int, out, nodata: int = 255) -> None:
    """out (uint8 CUDA tensor) <- d8_upslope_cells of dirs (uint8 CUDA tensor), on torch's current stream."""
    import torch

    h, w = _dev2d(dirs, "d8_upslope_cells_dev", torch.uint8)
    if _dev2d(out, "d8_upslope_cells_dev", torch.uint8) != (h, w):
        raise RdgpuError("d8_upslope_cells_dev: shape mismatch")
    check(lib().rdgpu_d8_upslope_cells_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(nodata), w, h, int(x0), int(y0),
                                           int(x1), int(y1), ctypes.c_void_p(out.data_ptr()), _stream_ptr()),
          "rdgpu_d8_upslope_cells_dev")


def d8_catchments_dev(dirs, seed_cells, seed_labels, out, unreached: int = 0, nodata: int = 255) -> None:
    """out (int32 CUDA tensor) <- catchments; seed_cells (int32 CUDA tensor of flat indices, read as unsigned) and
    seed_labels (int32 CUDA tensor) stay on the device."""
    import torch

    h, w = _dev2d(dirs, "d8_catchments_dev", torch.uint8)
    if _dev2d(out, "d8_catchments_dev", torch.int32) != (h, w):
        raise RdgpuError("d8_catchments_dev: shape mismatch")
    for t in (seed_cells, seed_labels):
        if not (t.is_cuda and t.dim() == 1 and t.is_contiguous() and t.dtype == torch.int32):
            raise RdgpuError("d8_catchments_dev: seeds are contiguous 1-D int32 tensors on the GPU")
    if seed_cells.numel() != seed_labels.numel():
        raise RdgpuError("d8_catchments_dev: one label per seed cell")
    check(lib().rdgpu_d8_catchments_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(nodata), w, h,
                                        ctypes.c_void_p(seed_cells.data_ptr()), ctypes.c_void_p(seed_labels.data_ptr()),
                                        ctypes.c_uint32(seed_cells.numel()), ctypes.c_int32(unreached),
                                        ctypes.c_void_p(out.data_ptr()), _stream_ptr()), "rdgpu_d8_catchments_dev")


def d8_outlets_dev(dirs, out, nodata: int = 255) -> None:
    """out (int32 CUDA tensor, holding the uint32 flat indices bit for bit: -1 is "none") <- outlets of dirs."""
    import torch

    h, w = _dev2d(dirs, "d8_outlets_dev", torch.uint8)
    if _dev2d(out, "d8_outlets_dev", torch.int32) != (h, w):
        raise RdgpuError("d8_outlets_dev: shape mismatch")
    check(lib().rdgpu_d8_outlets_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(nodata), w, h,
                                     ctypes.c_void_p(out.data_ptr()), _stream_ptr()), "rdgpu_d8_outlets_dev")


# ---- channel network and Strahler stream order (csrc/streams.hip) ----------------------------
STREAM_KINDS = {"none": 0, "head": 1, "junction": 2, "order_step": 3, "mouth": 4, "plain": 5}


def _mask2d(mask, shape, who):
    if mask is None:
        return None
    if not isinstance(mask, np.ndarray) or mask.dtype != np.uint8 or mask.shape != tuple(shape):
        raise RdgpuError(f"{who}: the channel mask is a uint8 array of the directions' shape")
    return np.ascontiguousarray(mask)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def d8_channels(accum: np.ndarray, threshold: float, accum_nodata: float = -1.0) -> np.ndarray:
    """uint8 mask: 1 where accum is not accum_nodata and accum >= threshold (float64 accumulation, as d8_flow_accum's)."""
    if not isinstance(accum, np.ndarray) or accum.ndim != 2 or accum.dtype != np.float64:
        raise RdgpuError("d8_channels: expected a 2-D float64 accumulation raster")
    accum = np.ascontiguousarray(accum)
    h, w = accum.shape
    out = np.empty((h, w), np.uint8)
    check(lib().rdgpu_d8_channels_f64(_ptr(accum), ctypes.c_double(accum_nodata), ctypes.c_double(threshold), w, h, _ptr(out)),
          "rdgpu_d8_channels_f64")
    return out


def d8_stream_order(dirs: np.ndarray, dir_nodata: int = 255, channels: np.ndarray | None = None) -> np.ndarray:
    """uint8 raster: the Strahler order of every channel cell (channels=None: every cell with a direction), 0 elsewhere,
    255 on the cells of a direction loop (include/rdgpu.h states the definition)."""
    dirs = _dirs2d(dirs, "d8_stream_order")
    chan = _mask2d(channels, dirs.shape, "d8_stream_order")
    h, w = dirs.shape
    out = np.empty((h, w), np.uint8)
    check(lib().rdgpu_d8_stream_order(_ptr(dirs), ctypes.c_uint8(dir_nodata), w, h, _ptr(chan), _ptr(out)), "rdgpu_d8_stream_order")
    return out


def d8_stream_links(dirs: np.ndarray, order: np.ndarray, dir_nodata: int = 255, channels: np.ndarray | None = None) -> np.ndarray:
    """uint8 raster of STREAM_KINDS: head, junction, order step (never, by the definition), mouth, plain; 0 off the channels."""
    dirs = _dirs2d(dirs, "d8_stream_links")
    chan = _mask2d(channels, dirs.shape, "d8_stream_links")
    order = _mask2d(order, dirs.shape, "d8_stream_links")
    if order is None:
        raise RdgpuError("d8_stream_links: the order raster is required")
    h, w = dirs.shape
    out = np.empty((h, w), np.uint8)
    check(lib().rdgpu_d8_stream_links(_ptr(dirs), ctypes.c_uint8(dir_nodata), w, h, _ptr(chan), _ptr(order), _ptr(out)),
          "rdgpu_d8_stream_links")
    return out


def d8_stream_order_stats() -> dict:
    """of this thread's last stream-order call: levels and node rounds per level enqueued, kernel launches"""
    v = [ctypes.c_int(0) for _ in range(3)]
    check(lib().rdgpu_d8_stream_order_get_stats(*[ctypes.byref(x) for x in v]), "rdgpu_d8_stream_order_get_stats")
    return {"levels": v[0].value, "rounds_per_level": v[1].value, "launches": v[2].value}


def _dev_mask(t, shape, who):
    import torch

    if t is None:
        return None
    if _dev2d(t, who, torch.uint8) != shape:
        raise RdgpuError(f"{who}: shape mismatch")
    return ctypes.c_void_p(t.data_ptr())


def d8_channels_dev(accum, threshold: float, out, accum_nodata: float = -1.0) -> None:
    """out (uint8 CUDA tensor) <- the channel mask of a float64 CUDA accumulation, on torch's current stream."""
    import torch

    h, w = _dev2d(accum, "d8_channels_dev", torch.float64)
    if _dev2d(out, "d8_channels_dev", torch.uint8) != (h, w):
        raise RdgpuError("d8_channels_dev: shape mismatch")
    check(lib().rdgpu_d8_channels_dev_f64(ctypes.c_void_p(accum.data_ptr()), ctypes.c_double(accum_nodata), ctypes.c_double(threshold),
                                          w, h, ctypes.c_void_p(out.data_ptr()), _stream_ptr()), "rdgpu_d8_channels_dev_f64")


def d8_stream_order_dev(dirs, out, dir_nodata: int = 255, channels=None) -> None:
    """out (uint8 CUDA tensor) <- the stream order of dirs (uint8 CUDA tensor), channels an optional uint8 CUDA mask."""
    import torch

    h, w = _dev2d(dirs, "d8_stream_order_dev", torch.uint8)
    if _dev2d(out, "d8_stream_order_dev", torch.uint8) != (h, w):
        raise RdgpuError("d8_stream_order_dev: shape mismatch")
    check(lib().rdgpu_d8_stream_order_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), w, h,
                                          _dev_mask(channels, (h, w), "d8_stream_order_dev"), ctypes.c_void_p(out.data_ptr()),
                                          _stream_ptr()), "rdgpu_d8_stream_order_dev")


def d8_stream_links_dev(dirs, order, out, dir_nodata: int = 255, channels=None) -> None:
    """out (uint8 CUDA tensor) <- the kinds of the channel cells of dirs / channels / order (uint8 CUDA tensors)."""
    import torch

    h, w = _dev2d(dirs, "d8_stream_links_dev", torch.uint8)
    if _dev2d(out, "d8_stream_links_dev", torch.uint8) != (h, w) or _dev2d(order, "d8_stream_links_dev", torch.uint8) != (h, w):
        raise RdgpuError("d8_stream_links_dev: shape mismatch")
    check(lib().rdgpu_d8_stream_links_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), w, h,
                                          _dev_mask(channels, (h, w), "d8_stream_links_dev"), ctypes.c_void_p(order.data_ptr()),
                                          ctypes.c_void_p(out.data_ptr()), _stream_ptr()), "rdgpu_d8_stream_links_dev")


# ---- flow distance, drainage cell and HAND (csrc/flowpath.hip) --------------------------------
_PATH_WANT = ("to_cell", "steps", "dist")
_HAND_SUFFIX = {k: v for k, v in _SUFFIX.items() if v not in ("i64", "u64")}


def _cell2(cell, who):
    try:
        cx, cy = float(cell[0]), float(cell[1])
    except (TypeError, ValueError, IndexError):
        raise RdgpuError(f"{who}: cell is a pair (cell_x, cell_y)") from None
    return ctypes.c_double(cx), ctypes.c_double(cy)


def _want(want, who):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _PATH_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_PATH_WANT}")
    return want


def d8_flow_path(dirs: np.ndarray, dir_nodata: int = 255, channels: np.ndarray | None = None, cell=(1.0, 1.0),
                 dist_nodata: float = -1.0, want=("to_cell", "dist")) -> dict:
    """The drainage cell of every cell and the way to it (include/rdgpu.h states the definition): a dict with the planes
    named in `want` -- "to_cell" (uint32 flat index, 0xFFFFFFFF for none), "steps" (uint32 [3, h, w]: along x, along y,
    diagonal) and "dist" (float64, dist_nodata for none).  channels=None: the drainage cell is the outlet."""
    dirs = _dirs2d(dirs, "d8_flow_path")
    chan = _mask2d(channels, dirs.shape, "d8_flow_path")
    want = _want(want, "d8_flow_path")
    cx, cy = _cell2(cell, "d8_flow_path")
    h, w = dirs.shape
    out = {}
    if "to_cell" in want:
        out["to_cell"] = np.empty((h, w), np.uint32)
    if "steps" in want:
        out["steps"] = np.empty((3, h, w), np.uint32)
    if "dist" in want:
        out["dist"] = np.empty((h, w), np.float64)
    check(lib().rdgpu_d8_flow_path(_ptr(dirs), ctypes.c_uint8(dir_nodata), w, h, _ptr(chan), cx, cy, _ptr(out.get("to_cell")),
                                   _ptr(out.get("steps")), _ptr(out.get("dist")), ctypes.c_double(dist_nodata)),
          "rdgpu_d8_flow_path")
    return out


def d8_flow_distance(dirs: np.ndarray, dir_nodata: int = 255, channels: np.ndarray | None = None, cell=(1.0, 1.0),
                     dist_nodata: float = -1.0) -> np.ndarray:
    """float64 raster: the length of every cell's flow path to its drainage cell -- the outlet, or with `channels` the
    first channel cell -- in the units of `cell`; dist_nodata where there is none."""
    return d8_flow_path(dirs, dir_nodata, channels, cell, dist_nodata, want=("dist",))["dist"]


def d8_hand(dem: np.ndarray, dirs: np.ndarray, dem_nodata, dir_nodata: int = 255, channels: np.ndarray | None = None,
            out_nodata: float = -9999.0) -> np.ndarray:
    """float64 raster: height above the nearest drainage, dem[c] - dem[drainage cell of c]; out_nodata where there is no
    drainage cell or one of the two elevations is dem_nodata.  Not clamped."""
    dirs = _dirs2d(dirs, "d8_hand")
    chan = _mask2d(channels, dirs.shape, "d8_hand")
    if not isinstance(dem, np.ndarray) or dem.shape != dirs.shape or dem.dtype not in _HAND_SUFFIX:
        raise RdgpuError("d8_hand: the DEM is an array of the directions' shape, element types int8 .. uint32, float32, float64")
    dem = np.ascontiguousarray(dem)
    s = _HAND_SUFFIX[dem.dtype]
    h, w = dirs.shape
    out = np.empty((h, w), np.float64)
    check(getattr(lib(), f"rdgpu_d8_hand_{s}")(_ptr(dirs), ctypes.c_uint8(dir_nodata), _ptr(dem), _scalar(s, dem_nodata), w, h,
                                               _ptr(chan), _ptr(out), ctypes.c_double(out_nodata)), "rdgpu_d8_hand")
    return out


def _dev_plane(t, shape, dtype, who):
    if t is None:
        return None
    if tuple(_dev_nd(t, who, dtype)) != tuple(shape):
        raise RdgpuError(f"{who}: shape mismatch")
    return ctypes.c_void_p(t.data_ptr())


def _dev_nd(t, who, dtype):
    if not (t.is_cuda and t.is_contiguous()):
        raise RdgpuError(f"{who}: expected a contiguous tensor on the GPU")
    if t.dtype != dtype:
        raise RdgpuError(f"{who}: expected dtype {dtype}, got {t.dtype}")
    return t.shape


def d8_flow_path_dev(dirs, dir_nodata: int = 255, channels=None, cell=(1.0, 1.0), dist_nodata: float = -1.0, to_cell=None,
                     steps=None, dist=None) -> None:
    """The planes given (CUDA tensors: to_cell int32 [h, w] holding the uint32 indices bit for bit, -1 is "none"; steps
    int32 [3, h, w] likewise; dist float64 [h, w]) <- d8_flow_path of dirs (uint8 CUDA tensor), on torch's current
    stream and without synchronising it.  At least one plane must be given."""
    import torch

    h, w = _dev2d(dirs, "d8_flow_path_dev", torch.uint8)
    if to_cell is None and steps is None and dist is None:
        raise RdgpuError("d8_flow_path_dev: no output requested")
    cx, cy = _cell2(cell, "d8_flow_path_dev")
    check(lib().rdgpu_d8_flow_path_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), w, h,
                                       _dev_mask(channels, (h, w), "d8_flow_path_dev"), cx, cy,
                                       _dev_plane(to_cell, (h, w), torch.int32, "d8_flow_path_dev"),
                                       _dev_plane(steps, (3, h, w), torch.int32, "d8_flow_path_dev"),
                                       _dev_plane(dist, (h, w), torch.float64, "d8_flow_path_dev"), ctypes.c_double(dist_nodata),
                                       _stream_ptr()), "rdgpu_d8_flow_path_dev")


def d8_flow_distance_dev(dirs, dist, dir_nodata: int = 255, channels=None, cell=(1.0, 1.0), dist_nodata: float = -1.0) -> None:
    """dist (float64 CUDA tensor) <- d8_flow_distance of dirs (uint8 CUDA tensor), channels an optional uint8 CUDA mask."""
    d8_flow_path_dev(dirs, dir_nodata, channels, cell, dist_nodata, dist=dist)


def d8_hand_dev(dem, dirs, dem_nodata, out, dir_nodata: int = 255, channels=None, out_nodata: float = -9999.0) -> None:
    """out (float64 CUDA tensor) <- d8_hand of dem (CUDA tensor, any element type torch has of int8 .. uint32, float32,
    float64) and dirs (uint8 CUDA tensor)."""
    import torch

    h, w = _dev2d(dirs, "d8_hand_dev", torch.uint8)
    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32", torch.float64: "f64"}
    for name, s in (("uint16", "u16"), ("uint32", "u32")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if dem.dtype not in m:
        raise RdgpuError(f"d8_hand_dev: unsupported elevation dtype {dem.dtype}")
    if _dev2d(dem, "d8_hand_dev") != (h, w) or _dev2d(out, "d8_hand_dev", torch.float64) != (h, w):
        raise RdgpuError("d8_hand_dev: shape mismatch")
    s = m[dem.dtype]
    check(getattr(lib(), f"rdgpu_d8_hand_dev_{s}")(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata),
                                                   ctypes.c_void_p(dem.data_ptr()), _scalar(s, dem_nodata), w, h,
                                                   _dev_mask(channels, (h, w), "d8_hand_dev"), ctypes.c_void_p(out.data_ptr()),
                                                   ctypes.c_double(out_nodata), _stream_ptr()), "rdgpu_d8_hand_dev")


# ---- stream reaches: reach labels, per-reach table, reach catchments (csrc/reaches.hip) ----------
REACH_DTYPE = np.dtype([("top_cell", np.uint32), ("bottom_cell", np.uint32), ("down", np.uint32), ("up", np.uint32),
                        ("cells", np.uint32), ("catchment_cells", np.uint32), ("steps", np.uint32, (3,)), ("order", np.uint32),
                        ("length", np.float64)])   # rdgpu_reach
_REACH_WANT = ("reach", "catchment", "table")


def d8_stream_reaches(dirs: np.ndarray, dir_nodata: int = 255, channels: np.ndarray | None = None, order: np.ndarray | None = None,
                      cell=(1.0, 1.0), want=_REACH_WANT) -> dict:
    """The reaches of the channel network -- the stretches between heads and junctions -- (include/rdgpu.h states the
    definitions): a dict with "count" (N) and what `want` names of "reach" (uint32: the label 1..N of a channel cell's
    reach, 0 elsewhere), "catchment" (uint32: the label of the reach a cell drains through, 0 for none) and "table"
    (``REACH_DTYPE`` [N]; ``table[i]`` describes label ``i + 1``).  Labels ascend with the raster index of the reach's
    bottom cell.  channels=None: every cell with a direction is a channel cell; order: an optional uint8 stream-order raster
    copied into the records.  With "table": two calls, the sizing call (no raster pass beyond the classification), then
    the one that fills it."""
    who = "d8_stream_reaches"
    dirs = _dirs2d(dirs, who)
    chan = _mask2d(channels, dirs.shape, who)
    if order is not None and (not isinstance(order, np.ndarray) or order.dtype != np.uint8 or order.shape != dirs.shape):
        raise RdgpuError(f"{who}: the order raster is a uint8 array of the directions' shape")
    order = None if order is None else np.ascontiguousarray(order)
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(k not in _REACH_WANT for k in want):
        raise RdgpuError(f"{who}: want names some of {_REACH_WANT}")
    cx, cy = _cell2(cell, who)
    h, w = dirs.shape
    count = ctypes.c_uint32(0)

    def call(reach, catchment, table):
        check(lib().rdgpu_d8_stream_reaches(_ptr(dirs), ctypes.c_uint8(dir_nodata), w, h, _ptr(chan), _ptr(order), cx, cy, _ptr(reach),
                                            _ptr(catchment), None if table is None or len(table) == 0 else _ptr(table),
                                            ctypes.c_uint32(0 if table is None else len(table)), ctypes.byref(count)),
              "rdgpu_d8_stream_reaches")
        return int(count.value)

    out = {}
    if "table" in want:
        out["table"] = np.zeros(call(None, None, None), REACH_DTYPE)
    if "reach" in want:
        out["reach"] = np.empty((h, w), np.uint32)
    if "catchment" in want:
        out["catchment"] = np.empty((h, w), np.uint32)
    n = out["count"] = call(out.get("reach"), out.get("catchment"), out.get("table"))
    if "table" in want and n != len(out["table"]):
        raise RdgpuError(f"{who}: the count changed between the two calls ({len(out['table'])} -> {n})")
    return out


def d8_stream_reaches_dev(dirs, dir_nodata: int = 255, channels=None, order=None, cell=(1.0, 1.0), reach=None, catchment=None,
                          table=None):
    """The same on HBM-resident tensors, on torch's current stream and without synchronising it: dirs, channels and order
    uint8 CUDA tensors; reach and catchment int32 CUDA tensors [h, w] holding the uint32 labels bit for bit, or ``None``;
    table a contiguous CUDA tensor of any element type holding 48 bytes per record (its capacity is its size in bytes
    // 48; ``.cpu().numpy().view(REACH_DTYPE)`` reads it) or ``None``.  Returns a one-element int32 CUDA tensor that holds
    the number of reaches once the stream gets there."""
    import torch

    who = "d8_stream_reaches_dev"
    h, w = _dev2d(dirs, who, torch.uint8)
    cx, cy = _cell2(cell, who)
    cap = 0
    if table is not None:
        if not (table.is_cuda and table.is_contiguous()):
            raise RdgpuError(f"{who}: expected a contiguous table tensor on the GPU")
        cap = table.numel() * table.element_size() // REACH_DTYPE.itemsize
    count = torch.zeros(1, dtype=torch.int32, device=dirs.device)
    check(lib().rdgpu_d8_stream_reaches_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), w, h,
                                            _dev_mask(channels, (h, w), who), _dev_mask(order, (h, w), who), cx, cy,
                                            _dev_plane(reach, (h, w), torch.int32, who), _dev_plane(catchment, (h, w), torch.int32, who),
                                            None if cap == 0 else ctypes.c_void_p(table.data_ptr()), ctypes.c_uint32(cap),
                                            ctypes.c_void_p(count.data_ptr()), _stream_ptr()), "rdgpu_d8_stream_reaches_dev")
    return count


# ---- depression inventory: labels and one record per depression of the fill -------------------------------------
DEPRESSION_DTYPE = np.dtype([("first_cell", np.uint32), ("pit_cell", np.uint32), ("outlet_cell", np.uint32), ("cells", np.uint32),
                             ("level", np.float64), ("pit_elevation", np.float64), ("volume", np.float64)])   # rdgpu_depression


def depressions_into(dem: np.ndarray, labels: np.ndarray | None, table: np.ndarray | None, topology="D8") -> int:
    """One call of ``rdgpu_depressions_<T>``: ``labels`` (int32, the DEM's shape) and the first ``len(table)`` records of
    ``table`` (``DEPRESSION_DTYPE``) are written where given; returns the number of depressions, whatever the capacity."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("depressions: expected a 2-D numpy array")
    dem = np.ascontiguousarray(dem)
    s = _suffix(dem.dtype)
    h, w = dem.shape
    if labels is not None and not (isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (h, w)
                                   and labels.flags["C_CONTIGUOUS"]):
        raise RdgpuError("depressions: labels must be a C-contiguous int32 array of the DEM's shape")
    if table is not None and not (isinstance(table, np.ndarray) and table.dtype == DEPRESSION_DTYPE and table.ndim == 1
                                  and table.flags["C_CONTIGUOUS"]):
        raise RdgpuError("depressions: table must be a C-contiguous 1-D array of DEPRESSION_DTYPE")
    count = ctypes.c_uint32(0)
    check(getattr(lib(), f"rdgpu_depressions_{s}")(dem.ctypes.data_as(ctypes.c_void_p), w, h, _topo(topology),
                                                   None if labels is None else labels.ctypes.data_as(ctypes.c_void_p),
                                                   None if table is None or len(table) == 0 else table.ctypes.data_as(ctypes.c_void_p),
                                                   ctypes.c_uint32(0 if table is None else len(table)), ctypes.byref(count)),
          "rdgpu_depressions")
    return int(count.value)


def depressions(dem: np.ndarray, topology="D8", labels: bool = True):
    """The depressions ``FillDepressions(dem, topology=...)`` fills: ``(labels, table)``.  ``labels`` (int32; ``None`` when
    not asked for) is 0 on cells the fill leaves alone and 1..N on its lakes, numbered by their lowest raster index;
    ``table[i]`` (``DEPRESSION_DTYPE``) describes label ``i + 1``: first, pit and outlet cell (raster indices), cells,
    level, pit elevation and volume (elevation units x cells).  NoData is an elevation like any other.  Two calls: the
    sizing call, then the one that fills the table."""
    n = depressions_into(dem, None, None, topology)
    lab = np.empty(dem.shape, np.int32) if labels else None
    table = np.zeros(n, DEPRESSION_DTYPE)
    got = depressions_into(dem, lab, table, topology)
    if got != n:
        raise RdgpuError(f"depressions: the count changed between the two calls ({n} -> {got})")
    return lab, table


def depressions_dev(dem, labels, table, topology="D8"):
    """The same on HBM-resident tensors, on torch's current stream: ``labels`` an int32 CUDA tensor of the DEM's shape or
    ``None``; ``table`` a contiguous CUDA tensor of any element type holding 40 bytes per record (its capacity is its size
    in bytes // 40; ``.cpu().numpy().view(DEPRESSION_DTYPE)`` reads it) or ``None``.  Returns a one-element int32 CUDA
    tensor that holds the number of depressions once the stream gets there."""
    import torch

    h, w = _dev2d(dem, "depressions_dev")
    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32", torch.float64: "f64",
         torch.int64: "i64"}
    for name, s in (("uint16", "u16"), ("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if dem.dtype not in m:
        raise RdgpuError(f"depressions_dev: unsupported elevation dtype {dem.dtype}")
    if labels is not None and tuple(_dev2d(labels, "depressions_dev", torch.int32)) != (h, w):
        raise RdgpuError("depressions_dev: shape mismatch")
    cap = 0
    if table is not None:
        if not (table.is_cuda and table.is_contiguous()):
            raise RdgpuError("depressions_dev: expected a contiguous table tensor on the GPU")
        cap = table.numel() * table.element_size() // DEPRESSION_DTYPE.itemsize
    count = torch.zeros(1, dtype=torch.int32, device=dem.device)
    check(getattr(lib(), f"rdgpu_depressions_dev_{m[dem.dtype]}")(
        ctypes.c_void_p(dem.data_ptr()), w, h, _topo(topology), None if labels is None else ctypes.c_void_p(labels.data_ptr()),
        None if cap == 0 else ctypes.c_void_p(table.data_ptr()), ctypes.c_uint32(cap), ctypes.c_void_p(count.data_ptr()),
        _stream_ptr()), "rdgpu_depressions_dev")
    return count


# ---- depression hierarchy: merge tree, leaf labels, levels and volumes (csrc/dephier.hip) ------------------------
DEPHIER_NONE = 0xFFFFFFFF
DEPHIER_NODE_DTYPE = np.dtype([("parent", np.uint32), ("lchild", np.uint32), ("rchild", np.uint32), ("pit_cell", np.uint32),
                               ("inside_cell", np.uint32), ("outside_cell", np.uint32), ("geolink", np.uint32),
                               ("cells", np.uint32), ("level", np.float64), ("pit_elevation", np.float64),
                               ("volume", np.float64)])   # rdgpu_dephier_node


class _DephierStats(ctypes.Structure):   # rdgpu_dephier_stats
    _fields_ = [("cell_pairs", ctypes.c_uint64), ("edges_raw", ctypes.c_uint64), ("edges_reduced", ctypes.c_uint64),
                ("pits", ctypes.c_uint32),
                ("nodes", ctypes.c_uint32), ("roots", ctypes.c_uint32), ("builder", ctypes.c_uint32),
                ("builder_rounds", ctypes.c_uint32), ("jump_rounds", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("lift_planes", ctypes.c_uint32)]


DEPHIER_BUILDERS = {1: "host_kruskal"}


def dephier_stats() -> dict:
    """``rdgpu_dephier_get_stats``: the counts of the calling thread's last hierarchy call; ``builder`` by name."""
    st = _DephierStats()
    check(lib().rdgpu_dephier_get_stats(ctypes.byref(st)), "rdgpu_dephier_get_stats")
    out = {k: int(getattr(st, k)) for k, _ in _DephierStats._fields_}
    out["builder"] = DEPHIER_BUILDERS.get(out["builder"], "none")
    return out


def _ocean_host(ocean, shape, who):
    """The ocean mask as a C-contiguous uint8 array of the DEM's shape (bool is taken as it is; non-zero means ocean)."""
    if not isinstance(ocean, np.ndarray) or ocean.shape != tuple(shape) or ocean.dtype not in (np.dtype(np.uint8), np.dtype(bool)):
        raise RdgpuError(f"{who}: ocean must be a uint8 or bool array of the DEM's shape")
    return np.ascontiguousarray(ocean).view(np.uint8)


def depression_hierarchy_into(dem: np.ndarray, labels: np.ndarray | None, table: np.ndarray | None, topology=8, ocean=None):
    """One call of ``rdgpu_depression_hierarchy_<T>`` (``rdgpu_depression_hierarchy_ocean_<T>`` when ``ocean``, a uint8 or
    bool mask of the DEM's shape, is given): ``labels`` (int32, the DEM's shape) and the first ``len(table)`` records of
    ``table`` (``DEPHIER_NODE_DTYPE``) are written where given; returns ``(nodes, leaves)``."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("depression_hierarchy: expected a 2-D numpy array")
    dem = np.ascontiguousarray(dem)
    s = _suffix(dem.dtype)
    h, w = dem.shape
    if labels is not None and not (isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (h, w)
                                   and labels.flags["C_CONTIGUOUS"]):
        raise RdgpuError("depression_hierarchy: labels must be a C-contiguous int32 array of the DEM's shape")
    if table is not None and not (isinstance(table, np.ndarray) and table.dtype == DEPHIER_NODE_DTYPE and table.ndim == 1
                                  and table.flags["C_CONTIGUOUS"]):
        raise RdgpuError("depression_hierarchy: table must be a C-contiguous 1-D array of DEPHIER_NODE_DTYPE")
    count, leaves = ctypes.c_uint32(0), ctypes.c_uint32(0)
    outs = (None if labels is None else labels.ctypes.data_as(ctypes.c_void_p),
            None if table is None or len(table) == 0 else table.ctypes.data_as(ctypes.c_void_p),
            ctypes.c_uint32(0 if table is None else len(table)), ctypes.byref(count), ctypes.byref(leaves))
    if ocean is None:
        check(getattr(lib(), f"rdgpu_depression_hierarchy_{s}")(
            dem.ctypes.data_as(ctypes.c_void_p), w, h, _topo(topology), *outs), "rdgpu_depression_hierarchy")
    else:
        ocean = _ocean_host(ocean, (h, w), "depression_hierarchy")
        check(getattr(lib(), f"rdgpu_depression_hierarchy_ocean_{s}")(
            dem.ctypes.data_as(ctypes.c_void_p), w, h, _topo(topology), ocean.ctypes.data_as(ctypes.c_void_p), *outs),
            "rdgpu_depression_hierarchy_ocean")
    return int(count.value), int(leaves.value)


def depression_hierarchy(dem: np.ndarray, topology=8, labels: bool = True, ocean=None):
    """The depression hierarchy of ``dem`` (reference: ``GetDepressionHierarchy``; the contract, which fixes every tie, is
    in ``include/rdgpu.h``): ``(labels, table)``.  The ocean is the border ring, or, when ``ocean`` (a uint8 or bool mask
    of the DEM's shape, see ``ocean_mask``) is given, exactly its non-zero cells: the ring is then land unless the mask
    says otherwise, and a mask without any ocean cell is an error.  ``labels`` (int32; ``None`` when not
    asked for) is the leaf depression a cell descends to, -1 where it drains into the ocean.  ``table``
    (``DEPHIER_NODE_DTYPE``): the binary merge tree, leaves first (by ascending pit index), then the merged depressions in
    the order they form; parent / children (``DEPHIER_NONE``: root / leaf), pit cell, the spill pair, ``geolink``, and the
    cells, level and volume of the node filled to its spill level.  Two calls: the sizing call, then the one that fills
    the table."""
    n, _ = depression_hierarchy_into(dem, None, None, topology, ocean)
    lab = np.empty(dem.shape, np.int32) if labels else None
    table = np.zeros(n, DEPHIER_NODE_DTYPE)
    got, _ = depression_hierarchy_into(dem, lab, table, topology, ocean)
    if got != n:
        raise RdgpuError(f"depression_hierarchy: the count changed between the two calls ({n} -> {got})")
    return lab, table


def depression_hierarchy_dev(dem, labels, table, topology=8, ocean=None):
    """The same on HBM-resident tensors, on torch's current stream: ``labels`` an int32 CUDA tensor of the DEM's shape or
    ``None``; ``table`` a contiguous CUDA tensor of any element type holding 56 bytes per record (its capacity is its size
    in bytes // 56; ``.cpu().numpy().view(DEPHIER_NODE_DTYPE)`` reads it) or ``None``; ``ocean`` a uint8 or bool CUDA tensor
    of the DEM's shape or ``None`` (the border ring).  Returns a two-element int32 CUDA tensor: the number of nodes and of
    leaves."""
    import torch

    h, w = _dev2d(dem, "depression_hierarchy_dev")
    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32", torch.float64: "f64",
         torch.int64: "i64"}
    for name, s in (("uint16", "u16"), ("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if dem.dtype not in m:
        raise RdgpuError(f"depression_hierarchy_dev: unsupported elevation dtype {dem.dtype}")
    if labels is not None and tuple(_dev2d(labels, "depression_hierarchy_dev", torch.int32)) != (h, w):
        raise RdgpuError("depression_hierarchy_dev: shape mismatch")
    cap = 0
    if table is not None:
        if not (table.is_cuda and table.is_contiguous()):
            raise RdgpuError("depression_hierarchy_dev: expected a contiguous table tensor on the GPU")
        cap = table.numel() * table.element_size() // DEPHIER_NODE_DTYPE.itemsize
    counts = torch.zeros(2, dtype=torch.int32, device=dem.device)
    outs = (None if labels is None else ctypes.c_void_p(labels.data_ptr()),
            None if cap == 0 else ctypes.c_void_p(table.data_ptr()), ctypes.c_uint32(cap), ctypes.c_void_p(counts.data_ptr()),
            ctypes.c_void_p(counts.data_ptr() + 4), _stream_ptr())
    if ocean is None:
        check(getattr(lib(), f"rdgpu_depression_hierarchy_dev_{m[dem.dtype]}")(
            ctypes.c_void_p(dem.data_ptr()), w, h, _topo(topology), *outs), "rdgpu_depression_hierarchy_dev")
    else:
        if ocean.dtype not in (torch.uint8, torch.bool) or tuple(_dev2d(ocean, "depression_hierarchy_dev")) != (h, w):
            raise RdgpuError("depression_hierarchy_dev: ocean must be a uint8 or bool CUDA tensor of the DEM's shape")
        check(getattr(lib(), f"rdgpu_depression_hierarchy_ocean_dev_{m[dem.dtype]}")(
            ctypes.c_void_p(dem.data_ptr()), w, h, _topo(topology), ctypes.c_void_p(ocean.data_ptr()), *outs),
            "rdgpu_depression_hierarchy_ocean_dev")
    return counts


# ---- bucket fill from the edges, and the ocean mask built with it (csrc/bucketfill.hip) ---------------------------
_check_rc = check   # (the raster argument below is called `check`, as in the reference)


def _check_scalar(s: str, value):
    """ctypes scalar of the raster's element type for an equality test against `value`: floating types round it as a C
    cast does; for an integer raster None when no element can equal it (NaN, a fraction, out of range)."""
    if s in ("f32", "f64"):
        return _CT[s](float(value))
    if isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_)):
        v = int(value)                       # (exact: a 64-bit integer need not survive a trip through float)
    else:
        try:
            f = float(value)
            if not np.isfinite(f) or f != int(f):
                return None
            v = int(f)
        except (TypeError, ValueError, OverflowError):
            return None
    info = np.iinfo(_NP[s])
    return _CT[s](v) if info.min <= v <= info.max else None


def bucket_fill_from_edges(check: np.ndarray, check_value, mask: np.ndarray | None = None, topology=8):
    """``BucketFillFromEdges`` (reference: misc/misc_methods.hpp; the contract is in ``include/rdgpu.h``): the cells with
    ``check == check_value`` and ``mask == 0`` that are connected, through such cells, to one of them on the border ring
    get ``mask = 1``.  ``mask`` (uint8 or bool, the raster's shape; all zero when left out) is not modified: returns
    ``(new mask as uint8, number of bytes set)``.  A ``check_value`` no element can equal sets nothing."""
    if not isinstance(check, np.ndarray) or check.ndim != 2:
        raise RdgpuError("bucket_fill_from_edges: expected a 2-D numpy array")
    check_a = np.ascontiguousarray(check)
    s = _suffix(check_a.dtype)
    h, w = check_a.shape
    out = np.zeros((h, w), np.uint8) if mask is None else _ocean_host(mask, (h, w), "bucket_fill_from_edges").copy()
    topo = _topo(topology)
    v = _check_scalar(s, check_value)
    if v is None:
        return out, 0
    filled = ctypes.c_uint64(0)
    _check_rc(getattr(lib(), f"rdgpu_bucket_fill_from_edges_{s}")(
        check_a.ctypes.data_as(ctypes.c_void_p), w, h, topo, v, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(filled)),
        "rdgpu_bucket_fill_from_edges")
    return out, int(filled.value)


def bucket_fill_from_edges_dev(check, check_value, mask, topology=8):
    """The same on HBM-resident tensors, on torch's current stream: ``mask`` (a uint8 or bool CUDA tensor of the raster's
    shape) is updated in place.  Returns a one-element int64 CUDA tensor: the number of bytes set."""
    import torch

    h, w = _dev2d(check, "bucket_fill_from_edges_dev")
    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32", torch.float64: "f64",
         torch.int64: "i64"}
    for name, s in (("uint16", "u16"), ("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if check.dtype not in m:
        raise RdgpuError(f"bucket_fill_from_edges_dev: unsupported dtype {check.dtype}")
    if mask.dtype not in (torch.uint8, torch.bool) or tuple(_dev2d(mask, "bucket_fill_from_edges_dev")) != (h, w):
        raise RdgpuError("bucket_fill_from_edges_dev: mask must be a uint8 or bool CUDA tensor of the raster's shape")
    topo = _topo(topology)
    filled = torch.zeros(1, dtype=torch.int64, device=check.device)
    v = _check_scalar(m[check.dtype], check_value)
    if v is None:
        return filled
    _check_rc(getattr(lib(), f"rdgpu_bucket_fill_from_edges_dev_{m[check.dtype]}")(
        ctypes.c_void_p(check.data_ptr()), w, h, topo, v, ctypes.c_void_p(mask.data_ptr()),
        ctypes.c_void_p(filled.data_ptr()), _stream_ptr()), "rdgpu_bucket_fill_from_edges_dev")
    return filled


def ocean_mask(dem: np.ndarray, ocean_level=None, nodata=None, border: bool = False, topology=8) -> np.ndarray:
    """An ocean mask for ``depression_hierarchy(..., ocean=)`` by the rule of the reference's Fill-Spill-Merge app: the
    cells equal to ``nodata`` (when given), the cells at ``ocean_level`` (when given) that the border reaches through such
    cells (``bucket_fill_from_edges``, which runs before the NoData cells are added, as in the app), and, with ``border``,
    the border ring.  uint8, the DEM's shape."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("ocean_mask: expected a 2-D numpy array")
    h, w = dem.shape
    if ocean_level is not None:
        mask, _ = bucket_fill_from_edges(dem, ocean_level, None, topology)
    else:
        _topo(topology)
        mask = np.zeros((h, w), np.uint8)
    if nodata is not None:
        v = _check_scalar(_suffix(dem.dtype), nodata)
        if v is not None:
            mask[dem == dem.dtype.type(v.value)] = 1
    if border:
        mask[0, :] = mask[-1, :] = 1
        mask[:, 0] = mask[:, -1] = 1
    return mask


# ---- fill-spill-merge: water routed through the depression hierarchy (csrc/fsm.hip) ------------------------------
class _FsmResult(ctypes.Structure):   # rdgpu_fsm_result
    _fields_ = [("water_in", ctypes.c_double), ("ocean", ctypes.c_double), ("standing", ctypes.c_double),
                ("lakes", ctypes.c_uint32), ("full_lakes", ctypes.c_uint32)]


class _FsmStats(ctypes.Structure):   # rdgpu_fsm_stats
    _fields_ = [("records", ctypes.c_uint64), ("host_ms", ctypes.c_double), ("nodes", ctypes.c_uint32),
                ("leaves", ctypes.c_uint32), ("lakes", ctypes.c_uint32), ("partial_lakes", ctypes.c_uint32),
                ("pours", ctypes.c_uint32), ("longest_pour", ctypes.c_uint32), ("shortcut_hits", ctypes.c_uint32),
                ("sort_bits", ctypes.c_uint32)]


FSM_RESULT_DTYPE = np.dtype([("water_in", np.float64), ("ocean", np.float64), ("standing", np.float64),
                             ("lakes", np.uint32), ("full_lakes", np.uint32)])   # rdgpu_fsm_result


def fsm_stats() -> dict:
    """``rdgpu_fsm_get_stats``: the counts of the calling thread's last fill-spill-merge call."""
    st = _FsmStats()
    check(lib().rdgpu_fsm_get_stats(ctypes.byref(st)), "rdgpu_fsm_get_stats")
    return {k: (float if k == "host_ms" else int)(getattr(st, k)) for k, _ in _FsmStats._fields_}


def fill_spill_merge(dem: np.ndarray, labels: np.ndarray, table: np.ndarray, water: np.ndarray, node_water: bool = True):
    """Fill-Spill-Merge (reference: ``FillSpillMerge`` with surface water only; the contract is in ``include/rdgpu.h``):
    ``water`` (float64 per cell, finite and >= 0) runs down into the leaf depressions of ``depression_hierarchy(dem)``,
    fills them, spills over their saddles and merges; what leaves the raster goes to the ocean.  ``labels`` and ``table``
    are that call's outputs, so one hierarchy serves any number of water scenarios.  Returns ``(depth, result)``:
    ``depth`` (float64, the DEM's shape) is the standing water per cell, ``result`` a dict with ``water_in``, ``ocean``,
    ``standing``, ``lakes``, ``full_lakes`` and, when asked for, ``node_water`` (float64 per node of ``table``)."""
    if not isinstance(dem, np.ndarray) or dem.ndim != 2:
        raise RdgpuError("fill_spill_merge: expected a 2-D numpy array")
    dem = np.ascontiguousarray(dem)
    s = _suffix(dem.dtype)
    h, w = dem.shape
    if not (isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (h, w)):
        raise RdgpuError("fill_spill_merge: labels must be an int32 array of the DEM's shape")
    if not (isinstance(table, np.ndarray) and table.dtype == DEPHIER_NODE_DTYPE and table.ndim == 1):
        raise RdgpuError("fill_spill_merge: table must be a 1-D array of DEPHIER_NODE_DTYPE")
    if not (isinstance(water, np.ndarray) and water.shape == (h, w)):
        raise RdgpuError("fill_spill_merge: water must be an array of the DEM's shape")
    labels, table = np.ascontiguousarray(labels), np.ascontiguousarray(table)
    water = np.ascontiguousarray(water, dtype=np.float64)
    depth = np.empty((h, w), np.float64)
    nw = np.zeros(len(table), np.float64) if node_water else None
    res = _FsmResult()
    check(getattr(lib(), f"rdgpu_fill_spill_merge_{s}")(
        dem.ctypes.data_as(ctypes.c_void_p), w, h, labels.ctypes.data_as(ctypes.c_void_p),
        table.ctypes.data_as(ctypes.c_void_p) if len(table) else None, ctypes.c_uint32(len(table)),
        water.ctypes.data_as(ctypes.c_void_p), depth.ctypes.data_as(ctypes.c_void_p),
        nw.ctypes.data_as(ctypes.c_void_p) if nw is not None and len(nw) else None, ctypes.byref(res)),
        "rdgpu_fill_spill_merge")
    out = {k: getattr(res, k) for k, _ in _FsmResult._fields_}
    if node_water:
        out["node_water"] = nw
    return depth, out


def fill_spill_merge_dev(dem, labels, table, count: int, water, depth, node_water=None):
    """The same on HBM-resident tensors, on torch's current stream: ``labels`` int32 and ``water`` / ``depth`` float64
    CUDA tensors of the DEM's shape, ``table`` the contiguous CUDA tensor ``depression_hierarchy_dev`` filled (56 bytes per
    record) holding ``count`` records, ``node_water`` a float64 CUDA tensor of ``count`` elements or ``None``.  ``depth``
    (and ``node_water``) are written; returns a 32-byte uint8 CUDA tensor, ``.cpu().numpy().view(FSM_RESULT_DTYPE)[0]``."""
    import torch

    h, w = _dev2d(dem, "fill_spill_merge_dev")
    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32", torch.float64: "f64",
         torch.int64: "i64"}
    for name, s in (("uint16", "u16"), ("uint32", "u32"), ("uint64", "u64")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if dem.dtype not in m:
        raise RdgpuError(f"fill_spill_merge_dev: unsupported elevation dtype {dem.dtype}")
    if tuple(_dev2d(labels, "fill_spill_merge_dev", torch.int32)) != (h, w) or \
            tuple(_dev2d(water, "fill_spill_merge_dev", torch.float64)) != (h, w) or \
            tuple(_dev2d(depth, "fill_spill_merge_dev", torch.float64)) != (h, w):
        raise RdgpuError("fill_spill_merge_dev: shape mismatch")
    count = int(count)
    if count:
        if not (table is not None and table.is_cuda and table.is_contiguous()
                and table.numel() * table.element_size() >= count * DEPHIER_NODE_DTYPE.itemsize):
            raise RdgpuError("fill_spill_merge_dev: expected a contiguous table tensor on the GPU holding count records")
    if node_water is not None and not (node_water.is_cuda and node_water.is_contiguous() and node_water.dtype == torch.float64
                                       and node_water.numel() >= count):
        raise RdgpuError("fill_spill_merge_dev: node_water must be a contiguous float64 CUDA tensor of count elements")
    res = torch.zeros(FSM_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dem.device)
    check(getattr(lib(), f"rdgpu_fill_spill_merge_dev_{m[dem.dtype]}")(
        ctypes.c_void_p(dem.data_ptr()), w, h, ctypes.c_void_p(labels.data_ptr()),
        ctypes.c_void_p(table.data_ptr()) if count else None, ctypes.c_uint32(count), ctypes.c_void_p(water.data_ptr()),
        ctypes.c_void_p(depth.data_ptr()), None if node_water is None or not count else ctypes.c_void_p(node_water.data_ptr()),
        ctypes.c_void_p(res.data_ptr()), _stream_ptr()), "rdgpu_fill_spill_merge_dev")
    return res


# ---- upslope extremes (csrc/extreme.hip) -------------------------------------------------------
_EXTREME_WANT = ("extreme", "at_cell")
_EXTREME_SUFFIX = {k: v for k, v in _SUFFIX.items() if v not in ("f64", "i64", "u64")}


def _which(which, who) -> int:
    m = {"max": 0, "min": 1, 0: 0, 1: 1}
    if isinstance(which, bool) or which not in m:
        raise RdgpuError(f"{who}: which is 'max' or 'min'")
    return m[which]


def d8_upslope_extreme(dirs: np.ndarray, values: np.ndarray, which="max", value_nodata=None, dir_nodata: int = 255,
                       want=("extreme", "at_cell")) -> dict:
    """The largest (which="max") or smallest ("min") value over everything that drains through each cell, the cell
    included, and where it sits (include/rdgpu.h states the definition): a dict with the planes named in `want` --
    "extreme" (the values' element type; value_nodata where nothing contributes) and "at_cell" (uint32 flat index, the
    lowest on a tie, 0xFFFFFFFF for none).  values: int8 .. uint32 or float32; cells equal to value_nodata and NaNs
    contribute nothing.  value_nodata=None: the array's own no_data (an rdarray), else an error."""
    who = "d8_upslope_extreme"
    dirs = _dirs2d(dirs, who)
    if not isinstance(values, np.ndarray) or values.shape != dirs.shape or values.dtype not in _EXTREME_SUFFIX:
        raise RdgpuError(f"{who}: the values are an array of the directions' shape, element types int8 .. uint32 or float32")
    w_ = _which(which, who)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _EXTREME_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_EXTREME_WANT}")
    if value_nodata is None:
        value_nodata = getattr(values, "no_data", None)
        if value_nodata is None:
            raise RdgpuError(f"{who}: value_nodata is not given and the values carry no no_data of their own")
    s = _EXTREME_SUFFIX[values.dtype]
    nd = _scalar(s, value_nodata)
    vals = np.ascontiguousarray(values)
    h, w = dirs.shape
    out = {}
    if "extreme" in want:
        out["extreme"] = np.empty((h, w), vals.dtype)
    if "at_cell" in want:
        out["at_cell"] = np.empty((h, w), np.uint32)
    check(getattr(lib(), f"rdgpu_d8_upslope_extreme_{s}")(_ptr(dirs), ctypes.c_uint8(dir_nodata), _ptr(vals), nd, w, h, w_,
                                                          _ptr(out.get("extreme")), _ptr(out.get("at_cell"))),
          "rdgpu_d8_upslope_extreme")
    return out


def d8_upslope_extreme_dev(dirs, values, which, value_nodata, extreme=None, at_cell=None, dir_nodata: int = 255) -> None:
    """The planes given (CUDA tensors: extreme of the values' dtype, at_cell int32 holding the uint32 indices bit for bit,
    -1 is "none") <- d8_upslope_extreme of dirs (uint8 CUDA tensor) and values (CUDA tensor of int8 .. uint32 as far as
    torch has them, or float32), on torch's current stream and without synchronising it.  At least one plane must be
    given."""
    import torch

    who = "d8_upslope_extreme_dev"
    h, w = _dev2d(dirs, who, torch.uint8)
    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32"}
    for name, s in (("uint16", "u16"), ("uint32", "u32")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if values.dtype not in m:
        raise RdgpuError(f"{who}: unsupported value dtype {values.dtype}")
    if _dev2d(values, who) != (h, w):
        raise RdgpuError(f"{who}: shape mismatch")
    if extreme is None and at_cell is None:
        raise RdgpuError(f"{who}: no output requested")
    s = m[values.dtype]
    check(getattr(lib(), f"rdgpu_d8_upslope_extreme_dev_{s}")(
        ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), ctypes.c_void_p(values.data_ptr()), _scalar(s, value_nodata),
        w, h, _which(which, who), _dev_plane(extreme, (h, w), values.dtype, who), _dev_plane(at_cell, (h, w), torch.int32, who),
        _stream_ptr()), "rdgpu_d8_upslope_extreme_dev")


# ---- depression breaching (csrc/breach.hip) -----------------------------------------------------
_BREACH_WANT = ("out", "path")


def _torch_breach_suffix(t, who) -> str:
    import torch

    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32"}
    for name, s in (("uint16", "u16"), ("uint32", "u32")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if t.dtype not in m:
        raise RdgpuError(f"{who}: unsupported dtype {t.dtype}")
    return m[t.dtype]


def d8_breach_along(dirs: np.ndarray, dem: np.ndarray, pits: np.ndarray, dir_nodata: int = 255, want=("out", "path")) -> dict:
    """The carve of depression breaching along GIVEN D8 directions (include/rdgpu.h states the definition): every pit (pits
    != 0) sends its level down the chain of links as far as the cells are not below it, and a cell ends at the least level
    that reached it.  A dict with the planes named in `want`: "out" (the DEM's element type, copies of cell values) and
    "path" (uint8: 1 where a pit's level reached the cell).  dem: int8 .. uint32 or float32 of the directions' shape."""
    who = "d8_breach_along"
    dirs = _dirs2d(dirs, who)
    if not isinstance(dem, np.ndarray) or dem.shape != dirs.shape or dem.dtype not in _EXTREME_SUFFIX:
        raise RdgpuError(f"{who}: the DEM is an array of the directions' shape, element types int8 .. uint32 or float32")
    if not isinstance(pits, np.ndarray) or pits.shape != dirs.shape or pits.dtype != np.uint8:
        raise RdgpuError(f"{who}: the pits are a uint8 array of the directions' shape")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _BREACH_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_BREACH_WANT}")
    s = _EXTREME_SUFFIX[dem.dtype]
    z, pm = np.ascontiguousarray(dem), np.ascontiguousarray(pits)
    h, w = dirs.shape
    out = {}
    if "out" in want:
        out["out"] = np.empty((h, w), z.dtype)
    if "path" in want:
        out["path"] = np.empty((h, w), np.uint8)
    check(getattr(lib(), f"rdgpu_d8_breach_along_{s}")(_ptr(dirs), ctypes.c_uint8(dir_nodata), _ptr(z), _ptr(pm), w, h,
                                                       _ptr(out.get("out")), _ptr(out.get("path"))), "rdgpu_d8_breach_along")
    return out


def d8_breach_along_dev(dirs, dem, pits, out=None, path=None, dir_nodata: int = 255) -> None:
    """The planes given (CUDA tensors: out of the DEM's dtype and not the DEM itself, path uint8) <- d8_breach_along of dirs
    and pits (uint8 CUDA tensors) and dem (CUDA tensor of int8 .. uint32 as far as torch has them, or float32), on torch's
    current stream and without synchronising it.  At least one plane must be given."""
    import torch

    who = "d8_breach_along_dev"
    h, w = _dev2d(dirs, who, torch.uint8)
    s = _torch_breach_suffix(dem, who)
    if _dev2d(dem, who) != (h, w) or _dev2d(pits, who, torch.uint8) != (h, w):
        raise RdgpuError(f"{who}: shape mismatch")
    if out is None and path is None:
        raise RdgpuError(f"{who}: no output requested")
    check(getattr(lib(), f"rdgpu_d8_breach_along_dev_{s}")(
        ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), ctypes.c_void_p(dem.data_ptr()), ctypes.c_void_p(pits.data_ptr()),
        w, h, _dev_plane(out, (h, w), dem.dtype, who), _dev_plane(path, (h, w), torch.uint8, who), _stream_ptr()),
        "rdgpu_d8_breach_along_dev")


class _BreachStats(ctypes.Structure):
    _fields_ = [("pits", ctypes.c_uint64), ("lowered", ctypes.c_uint64), ("raised", ctypes.c_uint64), ("unresolved", ctypes.c_uint64),
                ("twins", ctypes.c_uint32), ("tie_passes", ctypes.c_uint32)]


def breach_stats() -> dict:
    """of this thread's last breach_depressions / breach_depressions_dev: pits marked, cells raised by the pit pass, cells
    lowered by the carve, and the flood tree's twins / unresolved / tie_passes (pf_flowdirs_stats)"""
    st = _BreachStats()
    check(lib().rdgpu_breach_get_stats(ctypes.byref(st)), "rdgpu_breach_get_stats")
    return {"pits": st.pits, "lowered": st.lowered, "raised": st.raised, "unresolved": st.unresolved, "twins": st.twins,
            "tie_passes": st.tie_passes}


def _breach_warn(who):
    st = breach_stats()
    if st["unresolved"]:
        import warnings

        warnings.warn(f"{who}: the order of {st['unresolved']} of {st['twins']} equal cells was still moving when the tie-order passes "
                      f"of the flood's tree were stopped after {st['tie_passes']}: the result is the reference's only where those ties "
                      "do not decide", RuntimeWarning)


def breach_depressions(dem: np.ndarray, nodata=None, want=()):
    """CompleteBreaching_Lindsay2016<D8> (depressions/Lindsay2016.hpp:48-178): the breached copy of a 2-D array of int8 ..
    uint32 or float32, equal to the reference's, equal elevations included (breach_stats()["unresolved"] == 0; a
    RuntimeWarning otherwise).  nodata=None: the raster has no NoData; a raster that does hold its nodata value raises
    (code 3: breaching with NoData cells as outlets is not built).  want: "dirs" (uint8: the flood's tree, every interior
    cell pointing at the cell that pushed it) and / or "path" (uint8: 1 on the cells a walk carved or passed); with any of
    them the result is a dict with "out" and the planes named."""
    who = "breach_depressions"
    if not isinstance(dem, np.ndarray) or dem.ndim != 2 or dem.dtype not in _EXTREME_SUFFIX:
        raise RdgpuError(f"{who}: expected a 2-D numpy array of int8 .. uint32 or float32")
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(k not in ("dirs", "path") for k in want):
        raise RdgpuError(f"{who}: want names 'dirs' and / or 'path'")
    s = _EXTREME_SUFFIX[dem.dtype]
    work = np.ascontiguousarray(dem).copy()
    h, w = work.shape
    planes = {k: np.empty((h, w), np.uint8) for k in want}
    check(getattr(lib(), f"rdgpu_breach_d8_{s}")(_ptr(work), _scalar(s, 0 if nodata is None else nodata), 0 if nodata is None else 1,
                                                 w, h, _ptr(planes.get("dirs")), _ptr(planes.get("path"))), "rdgpu_breach_d8")
    _breach_warn(who)
    return dict(planes, out=work) if want else work


def breach_depressions_dev(dem, nodata=None, dirs=None, path=None) -> None:
    """breach_depressions in place on a contiguous 2-D CUDA tensor; dirs / path: optional uint8 CUDA tensors of its shape.
    On torch's current stream, which the call synchronises (the flood's tree is iterated from the host)."""
    import torch

    who = "breach_depressions_dev"
    h, w = _dev2d(dem, who)
    s = _torch_breach_suffix(dem, who)
    check(getattr(lib(), f"rdgpu_breach_d8_dev_{s}")(
        ctypes.c_void_p(dem.data_ptr()), _scalar(s, 0 if nodata is None else nodata), 0 if nodata is None else 1, w, h,
        _dev_plane(dirs, (h, w), torch.uint8, who), _dev_plane(path, (h, w), torch.uint8, who), _stream_ptr()), "rdgpu_breach_d8_dev")
    _breach_warn(who)


# ---- longest upstream flow path (csrc/longest.hip) ---------------------------------------------
_LONGEST_WANT = ("from_cell", "steps", "length", "on_basin_path")


def d8_longest_flow_path(dirs: np.ndarray, dir_nodata: int = 255, cell=(1.0, 1.0), length_nodata: float = -1.0,
                         want=("from_cell", "length")) -> dict:
    """The longest flow path that ends at every cell (include/rdgpu.h states the definition): a dict with the planes named
    in `want` -- "from_cell" (uint32 flat index of the path's head, the lowest on a tie, 0xFFFFFFFF for none), "steps"
    (uint32 [3, h, w]: along x, along y, diagonal), "length" (float64, length_nodata for none) and "on_basin_path" (uint8:
    1 on the longest path of every basin, from its head to the outlet)."""
    who = "d8_longest_flow_path"
    dirs = _dirs2d(dirs, who)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _LONGEST_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_LONGEST_WANT}")
    cx, cy = _cell2(cell, who)
    h, w = dirs.shape
    out = {}
    if "from_cell" in want:
        out["from_cell"] = np.empty((h, w), np.uint32)
    if "steps" in want:
        out["steps"] = np.empty((3, h, w), np.uint32)
    if "length" in want:
        out["length"] = np.empty((h, w), np.float64)
    if "on_basin_path" in want:
        out["on_basin_path"] = np.empty((h, w), np.uint8)
    check(lib().rdgpu_d8_longest_flow_path(_ptr(dirs), ctypes.c_uint8(dir_nodata), w, h, cx, cy, _ptr(out.get("from_cell")),
                                           _ptr(out.get("steps")), _ptr(out.get("length")), ctypes.c_double(length_nodata),
                                           _ptr(out.get("on_basin_path"))), "rdgpu_d8_longest_flow_path")
    return out


def d8_longest_flow_path_dev(dirs, dir_nodata: int = 255, cell=(1.0, 1.0), length_nodata: float = -1.0, from_cell=None, steps=None,
                             length=None, on_basin_path=None) -> None:
    """The planes given (CUDA tensors: from_cell int32 [h, w] holding the uint32 indices bit for bit, -1 is "none"; steps
    int32 [3, h, w] likewise; length float64 [h, w]; on_basin_path uint8 [h, w]) <- d8_longest_flow_path of dirs (uint8
    CUDA tensor), on torch's current stream and without synchronising it.  At least one plane must be given."""
    import torch

    who = "d8_longest_flow_path_dev"
    h, w = _dev2d(dirs, who, torch.uint8)
    if from_cell is None and steps is None and length is None and on_basin_path is None:
        raise RdgpuError(f"{who}: no output requested")
    cx, cy = _cell2(cell, who)
    check(lib().rdgpu_d8_longest_flow_path_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), w, h, cx, cy,
                                               _dev_plane(from_cell, (h, w), torch.int32, who),
                                               _dev_plane(steps, (3, h, w), torch.int32, who),
                                               _dev_plane(length, (h, w), torch.float64, who), ctypes.c_double(length_nodata),
                                               _dev_plane(on_basin_path, (h, w), torch.uint8, who), _stream_ptr()),
          "rdgpu_d8_longest_flow_path_dev")


# ---- weighted accumulation and total upstream length (csrc/accum_weighted.hip) ------------------
_WEIGHTED_SUFFIX = {k: v for k, v in _SUFFIX.items() if v not in ("i64", "u64")}
_TLEN_WANT = ("steps", "length")


def _sum_scalar(s: str, sum_nodata):
    return ctypes.c_double(float(sum_nodata)) if s in ("f32", "f64") else _scalar("i64", sum_nodata)


def d8_flow_accum_weighted(dirs: np.ndarray, weights: np.ndarray, weight_nodata, dir_nodata: int = 255, sum_nodata=-1) -> np.ndarray:
    """The sum of `weights` over everything that drains through each cell of a D8 direction raster, the cell included
    (include/rdgpu.h states the definition; direction loops carry nothing along their own links): int64 for int8 .. uint32
    weights (exact), float64 for float32 / float64 weights.  Cells whose weight equals weight_nodata, and NaNs, add
    nothing but pass on what they receive; sum_nodata where dirs == dir_nodata."""
    who = "d8_flow_accum_weighted"
    dirs = _dirs2d(dirs, who)
    if not isinstance(weights, np.ndarray) or weights.shape != dirs.shape or weights.dtype not in _WEIGHTED_SUFFIX:
        raise RdgpuError(f"{who}: the weights are an array of the directions' shape, element types int8 .. uint32, float32, float64")
    s = _WEIGHTED_SUFFIX[weights.dtype]
    wts = np.ascontiguousarray(weights)
    h, w = dirs.shape
    out = np.empty((h, w), np.float64 if s in ("f32", "f64") else np.int64)
    check(getattr(lib(), f"rdgpu_d8_flow_accum_weighted_{s}")(_ptr(dirs), ctypes.c_uint8(dir_nodata), _ptr(wts), _scalar(s, weight_nodata),
                                                              w, h, _ptr(out), _sum_scalar(s, sum_nodata)),
          "rdgpu_d8_flow_accum_weighted")
    return out


def d8_flow_accum_weighted_dev(dirs, weights, weight_nodata, out, dir_nodata: int = 255, sum_nodata=-1) -> None:
    """out (CUDA tensor: int64 for integer weights, float64 for float32 / float64 weights) <- d8_flow_accum_weighted of dirs
    (uint8 CUDA tensor) and weights (CUDA tensor of int8 .. uint32 as far as torch has them, float32 or float64), on torch's
    current stream and without synchronising it."""
    import torch

    who = "d8_flow_accum_weighted_dev"
    h, w = _dev2d(dirs, who, torch.uint8)
    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32", torch.float64: "f64"}
    for name, s in (("uint16", "u16"), ("uint32", "u32")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if weights.dtype not in m:
        raise RdgpuError(f"{who}: unsupported weight dtype {weights.dtype}")
    if _dev2d(weights, who) != (h, w):
        raise RdgpuError(f"{who}: shape mismatch")
    s = m[weights.dtype]
    if out is None:
        raise RdgpuError(f"{who}: no output given")
    check(getattr(lib(), f"rdgpu_d8_flow_accum_weighted_dev_{s}")(
        ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), ctypes.c_void_p(weights.data_ptr()), _scalar(s, weight_nodata),
        w, h, _dev_plane(out, (h, w), torch.float64 if s in ("f32", "f64") else torch.int64, who), _sum_scalar(s, sum_nodata),
        _stream_ptr()), "rdgpu_d8_flow_accum_weighted_dev")


def d8_total_upstream_length(dirs: np.ndarray, cell_x: float = 1.0, cell_y: float = 1.0, dir_nodata: int = 255,
                             want=("steps", "length"), length_nodata: float = -1.0) -> dict:
    """The total length of the links of the tree above every cell (TauDEM's tlen; include/rdgpu.h states the definition): a
    dict with the planes named in `want` -- "steps" (uint32 [3, h, w]: the links along x, along y and diagonal above the
    cell, 0xFFFFFFFF where dirs == dir_nodata) and "length" (float64, length_nodata there)."""
    who = "d8_total_upstream_length"
    dirs = _dirs2d(dirs, who)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _TLEN_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_TLEN_WANT}")
    cx, cy = _cell2((cell_x, cell_y), who)
    h, w = dirs.shape
    out = {}
    if "steps" in want:
        out["steps"] = np.empty((3, h, w), np.uint32)
    if "length" in want:
        out["length"] = np.empty((h, w), np.float64)
    check(lib().rdgpu_d8_total_upstream_length(_ptr(dirs), ctypes.c_uint8(dir_nodata), w, h, cx, cy, _ptr(out.get("steps")),
                                               _ptr(out.get("length")), ctypes.c_double(length_nodata)),
          "rdgpu_d8_total_upstream_length")
    return out


def d8_total_upstream_length_dev(dirs, cell_x: float = 1.0, cell_y: float = 1.0, dir_nodata: int = 255, steps=None, length=None,
                                 length_nodata: float = -1.0) -> None:
    """The planes given (CUDA tensors: steps int32 [3, h, w] holding the uint32 counts bit for bit, -1 where
    dirs == dir_nodata; length float64 [h, w]) <- d8_total_upstream_length of dirs (uint8 CUDA tensor), on torch's current
    stream and without synchronising it.  At least one plane must be given."""
    import torch

    who = "d8_total_upstream_length_dev"
    h, w = _dev2d(dirs, who, torch.uint8)
    if steps is None and length is None:
        raise RdgpuError(f"{who}: no output requested")
    cx, cy = _cell2((cell_x, cell_y), who)
    check(lib().rdgpu_d8_total_upstream_length_dev(ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), w, h, cx, cy,
                                                   _dev_plane(steps, (3, h, w), torch.int32, who),
                                                   _dev_plane(length, (h, w), torch.float64, who), ctypes.c_double(length_nodata),
                                                   _stream_ptr()), "rdgpu_d8_total_upstream_length_dev")


# ---- limited accumulation: losses, decay and capacity (csrc/accum_limited.hip) -------------------
_LIMITED_WANT = ("out", "kept")


class rdgpu_limited_result(ctypes.Structure):
    _fields_ = [("supplied", ctypes.c_double), ("left", ctypes.c_double), ("kept_pos", ctypes.c_double),
                ("kept_neg", ctypes.c_double)]


def _limited_want(want, who):
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(k not in _LIMITED_WANT for k in want):
        raise RdgpuError(f"{who}: want names planes of {_LIMITED_WANT}")
    return want


def d8_flow_accum_limited(dirs: np.ndarray, supply: np.ndarray, supply_nodata, capacity=None, factor=None, dir_nodata: int = 255,
                          nodata_out: float = -1.0, want=("out", "kept")) -> dict:
    """D8 accumulation in which a cell passes on out = min(max(factor * total, 0), max(capacity, 0)) of the total that
    reached it (its own supply included) and keeps the rest (include/rdgpu.h states the definition): a negative supply is
    a storage deficit that inflow fills first, `factor` a decay, `capacity` a transport limit; both are optional rasters
    of the supply's type (float32 or float64), NaN meaning "none here".  Returns a dict with the planes named in `want`
    ("out", "kept": float64, nodata_out where dirs == dir_nodata; `want` may be empty) and "result": the sums supplied,
    left (the out of the cells without a link), kept_pos and kept_neg, with supplied = left + kept_pos + kept_neg."""
    who = "d8_flow_accum_limited"
    dirs = _dirs2d(dirs, who)
    if not isinstance(supply, np.ndarray) or supply.shape != dirs.shape or supply.dtype not in (np.float32, np.float64):
        raise RdgpuError(f"{who}: the supply is a float32 or float64 array of the directions' shape")
    s = _SUFFIX[supply.dtype]
    planes = [np.ascontiguousarray(supply)]
    for name, a in (("capacity", capacity), ("factor", factor)):
        if a is not None and (not isinstance(a, np.ndarray) or a.shape != dirs.shape or a.dtype != supply.dtype):
            raise RdgpuError(f"{who}: {name} is an array of the supply's shape and element type, or None")
        planes.append(None if a is None else np.ascontiguousarray(a))
    want = _limited_want(want, who)
    h, w = dirs.shape
    res = {k: np.empty((h, w), np.float64) for k in want}
    r = rdgpu_limited_result()
    check(getattr(lib(), f"rdgpu_d8_flow_accum_limited_{s}")(_ptr(dirs), ctypes.c_uint8(dir_nodata), _ptr(planes[0]),
                                                             _scalar(s, supply_nodata), _ptr(planes[1]), _ptr(planes[2]), w, h,
                                                             _ptr(res.get("out")), _ptr(res.get("kept")), ctypes.c_double(nodata_out),
                                                             ctypes.byref(r)), "rdgpu_d8_flow_accum_limited")
    res["result"] = {k: getattr(r, k) for k, _ in rdgpu_limited_result._fields_}
    return res


def d8_flow_accum_limited_dev(dirs, supply, supply_nodata, capacity=None, factor=None, dir_nodata: int = 255, out=None, kept=None,
                              nodata_out: float = -1.0, result=None) -> None:
    """The planes given (float64 CUDA tensors out, kept [h, w]; result: a float64 CUDA tensor of 4 elements that receives
    supplied, left, kept_pos, kept_neg) <- d8_flow_accum_limited of dirs (uint8 CUDA tensor), supply and the optional
    capacity and factor (CUDA tensors, all float32 or all float64), on torch's current stream and without synchronising
    it.  At least one of out, kept, result must be given; what is not given is not written."""
    import torch

    who = "d8_flow_accum_limited_dev"
    h, w = _dev2d(dirs, who, torch.uint8)
    m = {torch.float32: "f32", torch.float64: "f64"}
    if supply.dtype not in m:
        raise RdgpuError(f"{who}: unsupported supply dtype {supply.dtype}")
    if _dev2d(supply, who) != (h, w):
        raise RdgpuError(f"{who}: shape mismatch")
    for a in (capacity, factor):
        if a is not None and (a.dtype != supply.dtype or _dev2d(a, who) != (h, w)):
            raise RdgpuError(f"{who}: capacity and factor have the supply's shape and element type")
    if out is None and kept is None and result is None:
        raise RdgpuError(f"{who}: no output requested")
    s = m[supply.dtype]
    check(getattr(lib(), f"rdgpu_d8_flow_accum_limited_dev_{s}")(
        ctypes.c_void_p(dirs.data_ptr()), ctypes.c_uint8(dir_nodata), ctypes.c_void_p(supply.data_ptr()), _scalar(s, supply_nodata),
        ctypes.c_void_p(capacity.data_ptr()) if capacity is not None else None,
        ctypes.c_void_p(factor.data_ptr()) if factor is not None else None, w, h,
        _dev_plane(out, (h, w), torch.float64, who), _dev_plane(kept, (h, w), torch.float64, who), ctypes.c_double(nodata_out),
        _dev_plane(result, (4,), torch.float64, who), _stream_ptr()), "rdgpu_d8_flow_accum_limited_dev")


# ---- flow distance and drop (HAND) down to the stop cells over D-infinity / MFD proportions (csrc/mfd_distance.hip) ----
_DIST_WANT = ("dist", "drop")
_DIST_STAT = {"ave": 0, "min": 1, "max": 2}


def _dist_stat(stat, who) -> int:
    if isinstance(stat, str):
        if stat not in _DIST_STAT:
            raise RdgpuError(f"{who}: stat is one of {tuple(_DIST_STAT)}")
        return _DIST_STAT[stat]
    return int(stat)   # the C-ABI's numbering; it rejects what is outside 0..2


def _dist_want(want, who):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _DIST_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_DIST_WANT}")
    return want


def _props3(props, who):
    if not isinstance(props, np.ndarray) or props.ndim != 3 or props.shape[2] != 9 or props.dtype != np.float32:
        raise RdgpuError(f"{who}: expected a float32 proportions array [h, w, 9]")
    return np.ascontiguousarray(props)


def _dist_planes(want, h, w):
    return {k: np.empty((h, w), np.float64) for k in _DIST_WANT if k in want}


def mfd_distance_down(props: np.ndarray, chan: np.ndarray | None = None, elev: np.ndarray | None = None, stat="ave",
                      strict: bool = True, cell=(1.0, 1.0), out_nodata: float = -1.0, want=("dist",)) -> dict:
    """Distance ("dist") and drop ("drop", needs elev) down to the stop cells over a proportions array [h, w, 9]
    (include/rdgpu.h states the definition): a dict with the float64 planes named in `want`.  chan: an optional uint8 mask
    of the stop cells (None: the cells without receivers); stat "ave" / "min" / "max" combines a cell's receivers; strict:
    every receiver must reach a stop cell; out_nodata where there is no value.  elev of any real dtype is taken as float64."""
    who = "mfd_distance_down"
    props = _props3(props, who)
    h, w = props.shape[:2]
    chan = _mask2d(chan, (h, w), who)
    want = _dist_want(want, who)
    if elev is not None:
        if not isinstance(elev, np.ndarray) or elev.shape != (h, w):
            raise RdgpuError(f"{who}: elev is an array of the proportions' raster shape")
        elev = np.ascontiguousarray(elev, dtype=np.float64)
    cx, cy = _cell2(cell, who)
    out = _dist_planes(want, h, w)
    check(lib().rdgpu_mfd_distance_down(_ptr(props), w, h, _ptr(chan), _ptr(elev), _dist_stat(stat, who), int(bool(strict)), cx, cy,
                                        _ptr(out.get("dist")), _ptr(out.get("drop")), ctypes.c_double(out_nodata)),
          "rdgpu_mfd_distance_down")
    return out


def _dinf_distance_down(who, dem, nodata, chan, stat, strict, cell, out_nodata, want) -> dict:
    dem, s = _elev(dem, who, mfd=True)
    h, w = dem.shape
    chan = _mask2d(chan, (h, w), who)
    want = _dist_want(want, who)
    cx, cy = _cell2(cell, who)
    out = _dist_planes(want, h, w)
    check(getattr(lib(), f"rdgpu_{who}_{s}")(_ptr(dem), _scalar(s, nodata), w, h, _ptr(chan), _dist_stat(stat, who), int(bool(strict)),
                                             cx, cy, _ptr(out.get("dist")), _ptr(out.get("drop")), ctypes.c_double(out_nodata)),
          "rdgpu_" + who)
    return out


def dinf_distance_down(dem: np.ndarray, nodata, chan: np.ndarray | None = None, stat="ave", strict: bool = True, cell=(1.0, 1.0),
                       out_nodata: float = -1.0, want=("dist",)) -> dict:
    """mfd_distance_down over the D-infinity proportions of dem (FM_Tarboton, never materialised), elevations the DEM's."""
    return _dinf_distance_down("dinf_distance_down", dem, nodata, chan, stat, strict, cell, out_nodata, want)


def dinf_distance_down_flats(dem: np.ndarray, nodata, chan: np.ndarray | None = None, stat="ave", strict: bool = True,
                             cell=(1.0, 1.0), out_nodata: float = -1.0, want=("dist",)) -> dict:
    """dinf_distance_down over the proportions of fm_tarboton_flats: the drainable flats of dem pass flow on."""
    return _dinf_distance_down("dinf_distance_down_flats", dem, nodata, chan, stat, strict, cell, out_nodata, want)


def dinf_hand(dem: np.ndarray, nodata, chan: np.ndarray, stat="ave", strict: bool = True, out_nodata: float = -9999.0) -> np.ndarray:
    """float64 raster: height above the drainage reached over the D-infinity proportions of dem -- the "drop" plane of
    dinf_distance_down with the channel mask chan.  Not clamped."""
    return dinf_distance_down(dem, nodata, chan, stat, strict, (1.0, 1.0), out_nodata, want=("drop",))["drop"]


def dinf_hand_flats(dem: np.ndarray, nodata, chan: np.ndarray, stat="ave", strict: bool = True, out_nodata: float = -9999.0) -> np.ndarray:
    """dinf_hand over the proportions of fm_tarboton_flats."""
    return dinf_distance_down_flats(dem, nodata, chan, stat, strict, (1.0, 1.0), out_nodata, want=("drop",))["drop"]


def mfd_distance_rounds() -> int:
    """Work-list launches of the last mfd_distance_down / dinf_distance_down / dinf_hand call or _dev form, or of the last
    mfd_distance_up / dinf_distance_up call or _dev form: whichever came last."""
    r = ctypes.c_uint32(0)
    check(lib().rdgpu_mfd_distance_rounds(ctypes.byref(r)), "rdgpu_mfd_distance_rounds")
    return r.value


def _torch_mfd_suffix(t, who) -> str:
    import torch

    m = {torch.int8: "i8", torch.uint8: "u8", torch.int16: "i16", torch.int32: "i32", torch.float32: "f32", torch.float64: "f64"}
    for name, s in (("uint16", "u16"), ("uint32", "u32")):
        if hasattr(torch, name):
            m[getattr(torch, name)] = s
    if t.dtype not in m:
        raise RdgpuError(f"{who}: unsupported elevation dtype {t.dtype}")
    return m[t.dtype]


def mfd_distance_down_dev(props, chan=None, elev=None, stat="ave", strict: bool = True, cell=(1.0, 1.0), out_nodata: float = -1.0,
                          dist=None, drop=None) -> None:
    """The planes given (float64 CUDA tensors [h, w]) <- mfd_distance_down of props (float32 CUDA tensor [h, w, 9]), chan
    an optional uint8 CUDA mask, elev a float64 CUDA tensor; on torch's current stream and without synchronising it.  At
    least one plane must be given."""
    import torch

    who = "mfd_distance_down_dev"
    if not (props.is_cuda and props.dim() == 3 and props.shape[2] == 9 and props.is_contiguous() and props.dtype == torch.float32):
        raise RdgpuError(f"{who}: expected a contiguous float32 tensor [h, w, 9] on the GPU")
    h, w = props.shape[:2]
    if dist is None and drop is None:
        raise RdgpuError(f"{who}: no output requested")
    cx, cy = _cell2(cell, who)
    check(lib().rdgpu_mfd_distance_down_dev(ctypes.c_void_p(props.data_ptr()), w, h, _dev_mask(chan, (h, w), who),
                                            _dev_plane(elev, (h, w), torch.float64, who), _dist_stat(stat, who), int(bool(strict)),
                                            cx, cy, _dev_plane(dist, (h, w), torch.float64, who),
                                            _dev_plane(drop, (h, w), torch.float64, who), ctypes.c_double(out_nodata), _stream_ptr()),
          "rdgpu_mfd_distance_down_dev")


def _dinf_distance_down_dev(who, entry, dem, nodata, chan, stat, strict, cell, out_nodata, dist, drop) -> None:
    import torch

    h, w = _dev2d(dem, who)
    s = _torch_mfd_suffix(dem, who)
    if dist is None and drop is None:
        raise RdgpuError(f"{who}: no output requested")
    cx, cy = _cell2(cell, who)
    check(getattr(lib(), f"{entry}_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h, _dev_mask(chan, (h, w), who),
                                         _dist_stat(stat, who), int(bool(strict)), cx, cy,
                                         _dev_plane(dist, (h, w), torch.float64, who), _dev_plane(drop, (h, w), torch.float64, who),
                                         ctypes.c_double(out_nodata), _stream_ptr()), entry)


def dinf_distance_down_dev(dem, nodata, chan=None, stat="ave", strict: bool = True, cell=(1.0, 1.0), out_nodata: float = -1.0,
                           dist=None, drop=None) -> None:
    """The planes given (float64 CUDA tensors) <- dinf_distance_down of dem (CUDA tensor of any element type torch has of
    int8 .. uint32, float32, float64), on torch's current stream.  At least one plane must be given."""
    _dinf_distance_down_dev("dinf_distance_down_dev", "rdgpu_dinf_distance_down_dev", dem, nodata, chan, stat, strict, cell,
                            out_nodata, dist, drop)


def dinf_distance_down_flats_dev(dem, nodata, chan=None, stat="ave", strict: bool = True, cell=(1.0, 1.0), out_nodata: float = -1.0,
                                 dist=None, drop=None) -> None:
    """dinf_distance_down_dev over the proportions of fm_tarboton_flats."""
    _dinf_distance_down_dev("dinf_distance_down_flats_dev", "rdgpu_dinf_distance_down_flats_dev", dem, nodata, chan, stat, strict,
                            cell, out_nodata, dist, drop)


def dinf_hand_dev(dem, nodata, chan, out, stat="ave", strict: bool = True, out_nodata: float = -9999.0) -> None:
    """out (float64 CUDA tensor) <- dinf_hand of dem and the uint8 CUDA channel mask chan."""
    dinf_distance_down_dev(dem, nodata, chan, stat, strict, (1.0, 1.0), out_nodata, drop=out)


def dinf_hand_flats_dev(dem, nodata, chan, out, stat="ave", strict: bool = True, out_nodata: float = -9999.0) -> None:
    """out (float64 CUDA tensor) <- dinf_hand_flats of dem and the uint8 CUDA channel mask chan."""
    dinf_distance_down_flats_dev(dem, nodata, chan, stat, strict, (1.0, 1.0), out_nodata, drop=out)


# ---- flow distance and rise up to the sources over D-infinity / MFD proportions (csrc/mfd_distance_up.hip) ----
_DISTUP_WANT = ("dist", "rise")


def _distup_want(want, who):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _DISTUP_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_DISTUP_WANT}")
    return want


def _distup_stat(stat, who) -> int:
    s = _dist_stat(stat, who)
    if s not in (0, 1, 2):
        raise RdgpuError(f"{who}: stat is one of {tuple(_DIST_STAT)} or 0..2")
    return s


def _min_share(min_share, who):
    """min_share as the float32 the engine compares with; negative or not finite is refused here as it is there"""
    try:
        v = np.float32(min_share)
    except (TypeError, ValueError):
        raise RdgpuError(f"{who}: min_share is a number") from None
    if not np.isfinite(v) or v < 0:
        raise RdgpuError(f"{who}: min_share must be finite and >= 0")
    return ctypes.c_float(float(v))


def _cell2_checked(cell, who):
    cx, cy = _cell2(cell, who)
    if not (np.isfinite(cx.value) and np.isfinite(cy.value)) or cx.value == 0 or cy.value == 0:
        raise RdgpuError(f"{who}: cell sizes must be finite and non-zero")
    return cx, cy


def mfd_distance_up(props: np.ndarray, elev: np.ndarray | None = None, stat="ave", min_share: float = 0.0, cell=(1.0, 1.0),
                    out_nodata: float = -1.0, want=("dist",)) -> dict:
    """Distance ("dist") and rise ("rise", needs elev) up to the sources over a proportions array [h, w, 9]
    (include/rdgpu.h states the definition): a dict with the float64 planes named in `want`.  stat "ave" / "min" / "max"
    combines a cell's donors (longest, shortest or share-weighted mean way up to the ridge); min_share: only shares above
    it are links (TauDEM's proportion threshold; 0: the accumulation's graph); out_nodata where there is no value.  elev of
    any real dtype is taken as float64."""
    who = "mfd_distance_up"
    props = _props3(props, who)
    h, w = props.shape[:2]
    want = _distup_want(want, who)
    if elev is not None:
        if not isinstance(elev, np.ndarray) or elev.shape != (h, w):
            raise RdgpuError(f"{who}: elev is an array of the proportions' raster shape")
        elev = np.ascontiguousarray(elev, dtype=np.float64)
    elif "rise" in want:
        raise RdgpuError(f"{who}: rise needs the elevations")
    st, ms = _distup_stat(stat, who), _min_share(min_share, who)
    cx, cy = _cell2_checked(cell, who)
    out = {k: np.empty((h, w), np.float64) for k in _DISTUP_WANT if k in want}
    check(lib().rdgpu_mfd_distance_up(_ptr(props), w, h, _ptr(elev), st, ms, cx, cy, _ptr(out.get("dist")), _ptr(out.get("rise")),
                                      ctypes.c_double(out_nodata)), "rdgpu_mfd_distance_up")
    return out


def _dinf_distance_up(who, dem, nodata, stat, min_share, cell, out_nodata, want) -> dict:
    dem, s = _elev(dem, who, mfd=True)
    h, w = dem.shape
    want = _distup_want(want, who)
    st, ms = _distup_stat(stat, who), _min_share(min_share, who)
    cx, cy = _cell2_checked(cell, who)
    nd = _scalar(s, nodata)
    out = {k: np.empty((h, w), np.float64) for k in _DISTUP_WANT if k in want}
    check(getattr(lib(), f"rdgpu_{who}_{s}")(_ptr(dem), nd, w, h, st, ms, cx, cy, _ptr(out.get("dist")), _ptr(out.get("rise")),
                                             ctypes.c_double(out_nodata)), "rdgpu_" + who)
    return out


def dinf_distance_up(dem: np.ndarray, nodata, stat="ave", min_share: float = 0.0, cell=(1.0, 1.0), out_nodata: float = -1.0,
                     want=("dist",)) -> dict:
    """mfd_distance_up over the D-infinity proportions of dem (FM_Tarboton, never materialised), elevations the DEM's."""
    return _dinf_distance_up("dinf_distance_up", dem, nodata, stat, min_share, cell, out_nodata, want)


def dinf_distance_up_flats(dem: np.ndarray, nodata, stat="ave", min_share: float = 0.0, cell=(1.0, 1.0), out_nodata: float = -1.0,
                           want=("dist",)) -> dict:
    """dinf_distance_up over the proportions of fm_tarboton_flats: the drainable flats of dem pass flow on."""
    return _dinf_distance_up("dinf_distance_up_flats", dem, nodata, stat, min_share, cell, out_nodata, want)


def mfd_distance_up_dev(props, elev=None, stat="ave", min_share: float = 0.0, cell=(1.0, 1.0), out_nodata: float = -1.0, dist=None,
                        rise=None) -> None:
    """The planes given (float64 CUDA tensors [h, w]) <- mfd_distance_up of props (float32 CUDA tensor [h, w, 9]), elev a
    float64 CUDA tensor; on torch's current stream and without synchronising it.  At least one plane must be given."""
    import torch

    who = "mfd_distance_up_dev"
    if not (props.is_cuda and props.dim() == 3 and props.shape[2] == 9 and props.is_contiguous() and props.dtype == torch.float32):
        raise RdgpuError(f"{who}: expected a contiguous float32 tensor [h, w, 9] on the GPU")
    h, w = props.shape[:2]
    if dist is None and rise is None:
        raise RdgpuError(f"{who}: no output requested")
    if rise is not None and elev is None:
        raise RdgpuError(f"{who}: rise needs the elevations")
    st, ms = _distup_stat(stat, who), _min_share(min_share, who)
    cx, cy = _cell2_checked(cell, who)
    pe, pd, pr = (_dev_plane(t, (h, w), torch.float64, who) for t in (elev, dist, rise))
    check(lib().rdgpu_mfd_distance_up_dev(ctypes.c_void_p(props.data_ptr()), w, h, pe, st, ms, cx, cy, pd, pr,
                                          ctypes.c_double(out_nodata), _stream_ptr()), "rdgpu_mfd_distance_up_dev")


def _dinf_distance_up_dev(who, entry, dem, nodata, stat, min_share, cell, out_nodata, dist, rise) -> None:
    import torch

    h, w = _dev2d(dem, who)
    s = _torch_mfd_suffix(dem, who)
    if dist is None and rise is None:
        raise RdgpuError(f"{who}: no output requested")
    st, ms = _distup_stat(stat, who), _min_share(min_share, who)
    cx, cy = _cell2_checked(cell, who)
    pd, pr = (_dev_plane(t, (h, w), torch.float64, who) for t in (dist, rise))
    check(getattr(lib(), f"{entry}_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h, st, ms, cx, cy, pd, pr,
                                         ctypes.c_double(out_nodata), _stream_ptr()), entry)


def dinf_distance_up_dev(dem, nodata, stat="ave", min_share: float = 0.0, cell=(1.0, 1.0), out_nodata: float = -1.0, dist=None,
                         rise=None) -> None:
    """The planes given (float64 CUDA tensors) <- dinf_distance_up of dem (CUDA tensor of any element type torch has of
    int8 .. uint32, float32, float64), on torch's current stream.  At least one plane must be given."""
    _dinf_distance_up_dev("dinf_distance_up_dev", "rdgpu_dinf_distance_up_dev", dem, nodata, stat, min_share, cell, out_nodata,
                          dist, rise)


def dinf_distance_up_flats_dev(dem, nodata, stat="ave", min_share: float = 0.0, cell=(1.0, 1.0), out_nodata: float = -1.0,
                               dist=None, rise=None) -> None:
    """dinf_distance_up_dev over the proportions of fm_tarboton_flats."""
    _dinf_distance_up_dev("dinf_distance_up_flats_dev", "rdgpu_dinf_distance_up_flats_dev", dem, nodata, stat, min_share, cell,
                          out_nodata, dist, rise)


# ---- reverse accumulation and upslope dependence over D-infinity / MFD proportions (csrc/mfd_reverse.hip) ----
_REV_WANT = ("racc", "wmax")


def _rev_want(want, who):
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _REV_WANT for k in want):
        raise RdgpuError(f"{who}: want names at least one of {_REV_WANT}")
    return want


def _rev_inputs(weights, dest, weight_nodata, want, shape, who):
    """the weights as float64, the mask, weight_nodata as a double (None: a NaN, "no NoData value")"""
    dest = _mask2d(dest, shape, who)
    if weights is not None:
        if not isinstance(weights, np.ndarray) or weights.shape != tuple(shape):
            raise RdgpuError(f"{who}: weights is an array of the raster's shape")
        weights = np.ascontiguousarray(weights, dtype=np.float64)
    elif dest is None:
        raise RdgpuError(f"{who}: neither weights nor dest given")
    elif "wmax" in want:
        raise RdgpuError(f"{who}: wmax needs the weights")
    return weights, dest, ctypes.c_double(float("nan") if weight_nodata is None else float(weight_nodata))


def mfd_reverse_accum(props: np.ndarray, weights: np.ndarray | None = None, dest: np.ndarray | None = None, weight_nodata=None,
                      out_nodata: float = -1.0, want=("racc",)) -> dict:
    """Reverse accumulation ("racc": the weights summed over everything downslope of a cell, by the shares) and the largest
    weight downslope ("wmax", needs weights) over a proportions array [h, w, 9] (include/rdgpu.h states the definition): a
    dict with the float64 planes named in `want`, in that order.  dest: an optional uint8 mask of absorbing cells; weights
    of any real dtype are taken as float64, cells equal to weight_nodata (None: no such value) and NaNs do not contribute;
    without weights the weight is 1 on dest and 0 elsewhere (the upslope dependence).  out_nodata where there is no value."""
    who = "mfd_reverse_accum"
    props = _props3(props, who)
    h, w = props.shape[:2]
    want = _rev_want(want, who)
    weights, dest, wnd = _rev_inputs(weights, dest, weight_nodata, want, (h, w), who)
    out = {k: np.empty((h, w), np.float64) for k in want}
    check(lib().rdgpu_mfd_reverse_accum(_ptr(props), w, h, _ptr(weights), wnd, _ptr(dest), _ptr(out.get("racc")),
                                        _ptr(out.get("wmax")), ctypes.c_double(out_nodata)), "rdgpu_mfd_reverse_accum")
    return out


def mfd_upslope_dependence(props: np.ndarray, dest: np.ndarray, out_nodata: float = -1.0) -> np.ndarray:
    """float64 raster: the fraction of every cell's flow that reaches the cells of the uint8 mask dest over the proportions
    (TauDEM's DinfUpDependence): mfd_reverse_accum's "racc" without weights."""
    if dest is None:
        raise RdgpuError("mfd_upslope_dependence: dest is required")
    return mfd_reverse_accum(props, None, dest, None, out_nodata, ("racc",))["racc"]


def _dinf_reverse_accum(who, dem, nodata, weights, dest, weight_nodata, out_nodata, want) -> dict:
    dem, s = _elev(dem, who, mfd=True)
    h, w = dem.shape
    want = _rev_want(want, who)
    weights, dest, wnd = _rev_inputs(weights, dest, weight_nodata, want, (h, w), who)
    out = {k: np.empty((h, w), np.float64) for k in want}
    check(getattr(lib(), f"rdgpu_{who}_{s}")(_ptr(dem), _scalar(s, nodata), w, h, _ptr(weights), wnd, _ptr(dest),
                                             _ptr(out.get("racc")), _ptr(out.get("wmax")), ctypes.c_double(out_nodata)),
          "rdgpu_" + who)
    return out


def dinf_reverse_accum(dem: np.ndarray, nodata, weights: np.ndarray | None = None, dest: np.ndarray | None = None,
                       weight_nodata=None, out_nodata: float = -1.0, want=("racc",)) -> dict:
    """mfd_reverse_accum over the D-infinity proportions of dem (FM_Tarboton, never materialised)."""
    return _dinf_reverse_accum("dinf_reverse_accum", dem, nodata, weights, dest, weight_nodata, out_nodata, want)


def dinf_reverse_accum_flats(dem: np.ndarray, nodata, weights: np.ndarray | None = None, dest: np.ndarray | None = None,
                             weight_nodata=None, out_nodata: float = -1.0, want=("racc",)) -> dict:
    """dinf_reverse_accum over the proportions of fm_tarboton_flats: the drainable flats of dem pass flow on."""
    return _dinf_reverse_accum("dinf_reverse_accum_flats", dem, nodata, weights, dest, weight_nodata, out_nodata, want)


def dinf_upslope_dependence(dem: np.ndarray, nodata, dest: np.ndarray, out_nodata: float = -1.0) -> np.ndarray:
    """mfd_upslope_dependence over the D-infinity proportions of dem."""
    if dest is None:
        raise RdgpuError("dinf_upslope_dependence: dest is required")
    return dinf_reverse_accum(dem, nodata, None, dest, None, out_nodata, ("racc",))["racc"]


def dinf_upslope_dependence_flats(dem: np.ndarray, nodata, dest: np.ndarray, out_nodata: float = -1.0) -> np.ndarray:
    """dinf_upslope_dependence over the proportions of fm_tarboton_flats."""
    if dest is None:
        raise RdgpuError("dinf_upslope_dependence_flats: dest is required")
    return dinf_reverse_accum_flats(dem, nodata, None, dest, None, out_nodata, ("racc",))["racc"]


def _rev_dev_args(weights, dest, weight_nodata, racc, wmax, shape, who):
    import torch

    if racc is None and wmax is None:
        raise RdgpuError(f"{who}: no output requested")
    if weights is None and dest is None:
        raise RdgpuError(f"{who}: neither weights nor dest given")
    if wmax is not None and weights is None:
        raise RdgpuError(f"{who}: wmax needs the weights")
    return (_dev_plane(weights, shape, torch.float64, who), ctypes.c_double(float("nan") if weight_nodata is None else float(weight_nodata)),
            _dev_mask(dest, shape, who), _dev_plane(racc, shape, torch.float64, who), _dev_plane(wmax, shape, torch.float64, who))


def mfd_reverse_accum_dev(props, weights=None, dest=None, weight_nodata=None, out_nodata: float = -1.0, racc=None, wmax=None) -> None:
    """The planes given (float64 CUDA tensors [h, w]) <- mfd_reverse_accum of props (float32 CUDA tensor [h, w, 9]), weights
    an optional float64 CUDA tensor, dest an optional uint8 CUDA mask; on torch's current stream and without synchronising
    it.  At least one plane must be given."""
    import torch

    who = "mfd_reverse_accum_dev"
    if not (props.is_cuda and props.dim() == 3 and props.shape[2] == 9 and props.is_contiguous() and props.dtype == torch.float32):
        raise RdgpuError(f"{who}: expected a contiguous float32 tensor [h, w, 9] on the GPU")
    h, w = props.shape[:2]
    pw, wnd, pd, pa, pm = _rev_dev_args(weights, dest, weight_nodata, racc, wmax, (h, w), who)
    check(lib().rdgpu_mfd_reverse_accum_dev(ctypes.c_void_p(props.data_ptr()), w, h, pw, wnd, pd, pa, pm, ctypes.c_double(out_nodata),
                                            _stream_ptr()), "rdgpu_mfd_reverse_accum_dev")


def _dinf_reverse_accum_dev(who, entry, dem, nodata, weights, dest, weight_nodata, out_nodata, racc, wmax) -> None:
    h, w = _dev2d(dem, who)
    s = _torch_mfd_suffix(dem, who)
    pw, wnd, pd, pa, pm = _rev_dev_args(weights, dest, weight_nodata, racc, wmax, (h, w), who)
    check(getattr(lib(), f"{entry}_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h, pw, wnd, pd, pa, pm,
                                         ctypes.c_double(out_nodata), _stream_ptr()), entry)


def dinf_reverse_accum_dev(dem, nodata, weights=None, dest=None, weight_nodata=None, out_nodata: float = -1.0, racc=None,
                           wmax=None) -> None:
    """The planes given (float64 CUDA tensors) <- dinf_reverse_accum of dem (CUDA tensor of any element type torch has of
    int8 .. uint32, float32, float64), on torch's current stream.  At least one plane must be given."""
    _dinf_reverse_accum_dev("dinf_reverse_accum_dev", "rdgpu_dinf_reverse_accum_dev", dem, nodata, weights, dest, weight_nodata,
                            out_nodata, racc, wmax)


def dinf_reverse_accum_flats_dev(dem, nodata, weights=None, dest=None, weight_nodata=None, out_nodata: float = -1.0, racc=None,
                                 wmax=None) -> None:
    """dinf_reverse_accum_dev over the proportions of fm_tarboton_flats."""
    _dinf_reverse_accum_dev("dinf_reverse_accum_flats_dev", "rdgpu_dinf_reverse_accum_flats_dev", dem, nodata, weights, dest,
                            weight_nodata, out_nodata, racc, wmax)


# ---- D-infinity across flats (include/rdgpu.h "D-infinity across flats") ---------------------------------------
class _DinfFlatsStats(ctypes.Structure):
    _fields_ = [("noflow_cells", ctypes.c_uint64), ("patched_cells", ctypes.c_uint64), ("fallback_cells", ctypes.c_uint64),
                ("unresolved_cells", ctypes.c_uint64)]


def dinf_flats_stats() -> dict:
    """The counts of this thread's last *_flats call (rdgpu_dinf_flats_get_stats; waits for that call's stream)."""
    st = _DinfFlatsStats()
    check(lib().rdgpu_dinf_flats_get_stats(ctypes.byref(st)), "rdgpu_dinf_flats_get_stats")
    return {k: int(getattr(st, k)) for k, _ in _DinfFlatsStats._fields_}


def fm_tarboton_flats(dem: np.ndarray, nodata) -> np.ndarray:
    """[h, w, 9] float32: FM_Tarboton's proportions with the cells of drainable flats routed over Barnes' flat mask.  The
    DEM is not altered."""
    return FlowProportions(dem, "Dinf", nodata=nodata, resolve_flats=True)


def fa_tarboton_flats(dem: np.ndarray, nodata, weights: np.ndarray | None = None) -> np.ndarray:
    """float64 accumulation over the proportions of fm_tarboton_flats (never materialised); NoData cells get -1."""
    return FlowAccumulation(dem, "Dinf", nodata=nodata, weights=weights, resolve_flats=True)


def fm_tarboton_flats_dev(dem, nodata, props9) -> None:
    """props9 (contiguous float32 CUDA tensor [h, w, 9]) <- fm_tarboton_flats of the CUDA tensor dem, on torch's current
    stream."""
    import torch

    who = "fm_tarboton_flats_dev"
    h, w = _dev2d(dem, who)
    if props9.dtype != torch.float32 or tuple(props9.shape) != (h, w, 9) or not props9.is_contiguous() or not props9.is_cuda:
        raise RdgpuError(f"{who}: props9 must be a contiguous float32 CUDA tensor [h, w, 9] of the DEM's raster shape")
    s = _torch_mfd_suffix(dem, who)
    check(getattr(lib(), f"rdgpu_fm_tarboton_flats_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                             ctypes.c_void_p(props9.data_ptr()), _stream_ptr()),
          "rdgpu_fm_tarboton_flats_dev")


def fa_tarboton_flats_dev(dem, nodata, accum) -> None:
    """fa_tarboton_dev over the proportions of fm_tarboton_flats: accum (float64 CUDA tensor) in: the cells' weights, out:
    the accumulation."""
    import torch

    who = "fa_tarboton_flats_dev"
    h, w = _dev2d(dem, who)
    if accum.dtype != torch.float64 or tuple(accum.shape) != (h, w) or not accum.is_contiguous() or not accum.is_cuda:
        raise RdgpuError(f"{who}: accum must be a contiguous float64 CUDA tensor of the DEM's shape")
    s = _torch_mfd_suffix(dem, who)
    check(getattr(lib(), f"rdgpu_fa_tarboton_flats_dev_{s}")(ctypes.c_void_p(dem.data_ptr()), _scalar(s, nodata), w, h,
                                                             ctypes.c_void_p(accum.data_ptr()), _stream_ptr()),
          "rdgpu_fa_tarboton_flats_dev")
