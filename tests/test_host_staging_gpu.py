"""The host door of every product against its device door (csrc/common.hpp: HostStage).

A host entry stages the caller's arrays in the workspace's named buffers, runs the driver its `_dev` twin runs and copies
the results down.  What such staging can get wrong -- a wrong element count, one buffer name shared by two live planes, a
stale tail in a pooled buffer that is larger than the call needs, a plane written that was not asked for -- shows as a
difference between the two doors, so every product is run through both on the same input and compared bit for bit.

Every product runs 67 x 131 (h x w) first: more than one 64-cell tile each way, neither side a multiple of 4, so every
per-cell plane has a ragged tail.  Then 9 x 5 in the same process: each pooled buffer is then larger than the call needs
and still holds the earlier call's bytes.  Typed entries run a 1-byte and an 8-byte element type (where the entry has no
8-byte type, its widest).  Every host call gets an input no earlier call has seen (a new seed), and the compared results
stay alive until the assertion, so a short download cannot pass on recycled memory."""
import ctypes
import itertools
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(67, 131), (9, 5)]   # (height, width), in this order
FILL = 0x5A                    # the sentinel byte
_SEED = itertools.count(1)


@pytest.fixture(scope="module")
def api(rd):
    from richdem_amd import api as a

    return a


def _nodata(dtype):
    return 255 if np.dtype(dtype) == np.uint8 else -9999


def _dem(shape, dtype):
    """a fresh DEM with pits, flats (few distinct levels) and some NoData cells"""
    rng = np.random.default_rng(next(_SEED))
    h, w = shape
    z = rng.integers(0, 9, (h, w)) + (np.add.outer(np.arange(h), np.arange(w)) // 7)
    z = z.astype(dtype)
    z[rng.random((h, w)) < 0.02] = _nodata(dtype)
    return z


def _dirs(api, shape):
    """fresh flat-resolved D8 directions (with NoData cells and a few cells without a direction)"""
    return api.barnes_flat_resolution_d8(_dem(shape, np.uint8), 255)


def _values(shape, dtype):
    rng = np.random.default_rng(next(_SEED))
    return rng.integers(0, 200, shape).astype(dtype)


def _mask(shape, p=0.1):
    rng = np.random.default_rng(next(_SEED))
    return (rng.random(shape) < p).astype(np.uint8)


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _empty(shape, dtype):
    """a device tensor filled with the sentinel byte"""
    import torch

    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    t = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32,
           np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)]
    return t.view(tdt).reshape(tuple(shape))


def _down(t, dtype=None):
    import torch

    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what   # bit for bit: NaNs and signed zeros included


def _stream(api):
    return api._stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ok(api, rc, what):
    api.check(rc, what)


# ---- fills -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_fill_and_its_other_outputs(api, dtype):
    L = api.lib()
    for shape in SHAPES:
        h, w = shape
        s, nd = api._suffix(dtype), _nodata(dtype)
        dem = _dem(shape, dtype)
        host = api.FillDepressions(dem)
        t = _up(dem)
        api.fill_depressions_dev(t)
        _same(host, _down(t), "fill")

        dem = _dem(shape, dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host = api.fill_max_dep(dem, 6)
        t = _up(dem)
        api.fill_max_dep_dev(t, 6)
        _same(host, _down(t), "fill_max_dep")

        dem = _dem(shape, dtype)
        host = api.pit_mask(dem, nd)
        t, m = _up(dem), _empty(shape, np.uint8)
        _ok(api, getattr(L, f"rdgpu_pit_mask_dev_{s}")(_p(t), api._scalar(s, nd), w, h, 8, _p(m), _stream(api)), "pit_mask_dev")
        _same(host, _down(m), "pit_mask")
        _same(dem, _down(t), "pit_mask: the DEM")

        for alter in (False, True):
            dem = _dem(shape, dtype)
            host = api.watersheds(dem, nd, alter=alter)
            t, lab = _up(dem), _empty(shape, np.int32)
            api.watersheds_dev(t, nd, lab, alter=alter)
            _same(host[0] if alter else host, _down(lab), "watersheds: labels")
            _same(host[1] if alter else dem, _down(t), "watersheds: the DEM")

        dem = _dem(shape, dtype)
        host = api.fill_wei2018(dem, nd)
        t = _up(dem)
        _ok(api, getattr(L, f"rdgpu_fill_wei2018_dev_{s}")(_p(t), api._scalar(s, nd), w, h, _stream(api)), "fill_wei2018_dev")
        _same(host, _down(t), "fill_wei2018")

        dem = _dem(shape, dtype)
        host = api.has_depressions(dem)
        t, flag = _up(dem), ctypes.c_int(-1)
        _ok(api, getattr(L, f"rdgpu_has_depressions_dev_{s}")(_p(t), w, h, 8, ctypes.byref(flag), _stream(api)), "has_depressions_dev")
        assert host == bool(flag.value)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])   # (the epsilon fill has floating-point entries only)
def test_fill_epsilon(api, dtype):
    for shape in SHAPES:
        dem = _dem(shape, dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host = api.FillDepressions(dem, epsilon=True, nodata=-9999)
        t = _up(dem)
        api.fill_epsilon_dev(t, -9999)
        _same(host, _down(t), "fill_epsilon")


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_pf_flowdirs(api, dtype):
    for shape in SHAPES:
        dem = _dem(shape, dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host = api.pf_flowdirs(dem, _nodata(dtype))
        t, d = _up(dem), _empty(shape, np.uint8)
        api.pf_flowdirs_dev(t, _nodata(dtype), d)
        _same(host, _down(d), "pf_flowdirs")


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_depressions(api, dtype):
    for shape in SHAPES:
        dem = _dem(shape, dtype)
        lab, table = api.depressions(dem)
        n = len(table)
        t, dl, dt = _up(dem), _empty(shape, np.int32), _empty((max(n, 1) * api.DEPRESSION_DTYPE.itemsize,), np.uint8)
        count = api.depressions_dev(t, dl, dt)
        assert int(_down(count)[0]) == n
        _same(lab, _down(dl), "depressions: labels")
        _same(table, _down(dt).view(api.DEPRESSION_DTYPE)[:n], "depressions: table")
        # the table alone, and cut short: the records that fit, the count whatever the capacity
        short = np.frombuffer(bytearray([FILL]) * (api.DEPRESSION_DTYPE.itemsize * (n // 2 + 1)), api.DEPRESSION_DTYPE)
        assert api.depressions_into(_dem_copy(dem), None, short) == n
        k = min(n, len(short))
        _same(short[:k], table[:k], "depressions: short table")
        assert bytes(short[k:].tobytes()) == bytes([FILL]) * (api.DEPRESSION_DTYPE.itemsize * (len(short) - k))


def _dem_copy(dem):
    return dem.copy()


# ---- directions, flats, D8 accumulation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_flow_directions_and_flats(api, dtype):
    L = api.lib()
    for shape in SHAPES:
        h, w = shape
        s, nd = api._suffix(dtype), _nodata(dtype)
        for flats in (False, True):
            dem = _dem(shape, dtype)
            host = api.barnes_flat_resolution_d8(dem, nd) if flats else api.d8_flow_directions(dem, nd)
            t, d = _up(dem), _empty(shape, np.uint8)
            api.d8_flow_directions_dev(t, nd, d, flats=flats)
            _same(host, _down(d), "flat resolution" if flats else "d8 directions")

        dem = _dem(shape, dtype)
        work = dem.copy()
        host = api.barnes_flat_resolution_d8(work, nd, alter=True)
        t, d = _up(dem), _empty(shape, np.uint8)
        _ok(api, getattr(L, f"rdgpu_flat_resolution_d8_alter_dev_{s}")(_p(t), api._scalar(s, nd), w, h, _p(d), _stream(api)), "alter_dev")
        _same(host, _down(d), "flat resolution, alter: directions")
        _same(work, _down(t), "flat resolution, alter: the DEM")

        dem = _dem(shape, dtype)
        host = api.resolve_flats_epsilon(dem, nd)
        t = _up(dem)
        api.resolve_flats_epsilon_dev(t, nd)
        _same(host, _down(t), "ResolveFlatsEpsilon")

        # rdgpu_resolve_flats: directions only, + mask, + labels, all -- a plane left out is null, the others do not move
        dem = _dem(shape, dtype)
        fn = getattr(L, f"rdgpu_resolve_flats_{s}")

        def call(want_mask, want_labels):
            d = np.full(shape, FILL, np.uint8)
            m = np.full(shape, FILL, np.int32) if want_mask else None
            lab = np.full(shape, FILL, np.int32) if want_labels else None
            _ok(api, fn(_hp(dem), api._scalar(s, nd), w, h, _hp(d), _hp(m), _hp(lab)), "rdgpu_resolve_flats")
            return d, m, lab

        d_all, m_all, l_all = call(True, True)
        d_only, _, _ = call(False, False)
        d_m, m_m, _ = call(True, False)
        d_l, _, l_l = call(False, True)
        t, d = _up(dem), _empty(shape, np.uint8)
        api.d8_flow_directions_dev(t, nd, d, flats=True)
        _same(d_only, _down(d), "resolve_flats, directions only")
        _same(d_all, d_only, "resolve_flats: directions")
        _same(d_m, d_all, "resolve_flats + mask: directions")
        _same(d_l, d_all, "resolve_flats + labels: directions")
        _same(m_m, m_all, "resolve_flats: mask")
        _same(l_l, l_all, "resolve_flats: labels")


@pytest.mark.parametrize("dtype", [np.int32, np.float32, np.float64])
def test_d8_flow_accum(api, dtype):
    for shape in SHAPES:
        dirs = _dirs(api, shape)
        host = api.d8_flow_accum(dirs, 255, dtype)
        a = _empty(shape, dtype)
        api.d8_flow_accum_dev(_up(dirs), a)
        _same(host, _down(a), "d8_flow_accum")


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_fa_d8_in_out_and_output_only(api, dtype):
    for shape in SHAPES:
        nd = _nodata(dtype)
        dem = _dem(shape, dtype)
        wts = _values(shape, np.float64) / 4.0
        host = api.FlowAccumulation(dem, "D8", nodata=nd, weights=wts)
        a = _up(wts)
        api.fa_d8_dev(_up(dem), nd, a)
        _same(host, _down(a), "fa_d8, caller weights")

        dem = _dem(shape, dtype)
        host = api.FlowAccumulation(dem, "D8", nodata=nd)   # declared ones: the array is output only, nothing is uploaded
        a = _empty(shape, np.float64)
        api.fa_d8_dev(_up(dem), nd, a, unit_weights=True)
        _same(host, _down(a), "fa_d8, declared ones")

        # FM_D8 has no device door: the same input gives the same bytes from a workspace that has held nothing else
        dem = _dem(shape, dtype)
        first = api.FlowProportions(dem, "D8", nodata=nd)
        api.release_workspace()
        _same(first, api.FlowProportions(dem.copy(), "D8", nodata=nd), "fm_d8")


# ---- D-infinity and MFD --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_dinf_and_mfd(api, dtype):
    """The accumulation of the MFD family runs through both doors with method D4, whose proportions are 0 or 1: with the
    weights used here (multiples of 1/4) every sum is exact in whatever order the device adds.  Holmgren and Quinn go through
    both doors for their proportions only: their accumulation adds fractional shares with double atomics in the order the
    hardware takes them, and two calls of ONE door on one input already differ (67 x 131, four calls each, on the commit
    before the staging helper and after it alike: 80 to 250 of 8777 cells, by at most 2 units in the last place -- host
    against host, device against device and host against device the same), so no comparison of two calls can ask for equal
    bits there.  D-infinity's accumulation (at most two receivers a cell) repeated itself in every one of those runs."""
    L = api.lib()
    for shape in SHAPES:
        h, w = shape
        s, nd = api._suffix(dtype), _nodata(dtype)
        dem = _dem(shape, dtype)
        host = api.dinf_flow_directions(dem, nd)
        a = _empty(shape, np.float32)
        api.dinf_flow_directions_dev(_up(dem), nd, a)
        _same(host, _down(a), "dinf_flow_directions")

        for flats in (False, True):
            dem = _dem(shape, dtype)
            wts = _values(shape, np.float64) / 4.0
            host = api.FlowAccumulation(dem, "Dinf", nodata=nd, weights=wts, resolve_flats=flats)
            a = _up(wts)
            (api.fa_tarboton_flats_dev if flats else api.fa_tarboton_dev)(_up(dem), nd, a)
            _same(host, _down(a), "fa_tarboton" + ("_flats" if flats else ""))

        dem = _dem(shape, dtype)
        host = api.FlowProportions(dem, "Dinf", nodata=nd, resolve_flats=True)
        p = _empty((h, w, 9), np.float32)
        api.fm_tarboton_flats_dev(_up(dem), nd, p)
        _same(host, _down(p), "fm_tarboton_flats")

        # FM_Tarboton has no device door: its proportions carry the device door of the accumulation
        dem = _dem(shape, dtype)
        props = api.FlowProportions(dem, "Dinf", nodata=nd)
        wts = _values(shape, np.float64) / 4.0
        host = api.FlowAccumFromProps(props, wts)
        a = _up(wts)
        api.flow_accumulation_dev(_up(props), a)
        _same(host, _down(a), "FlowAccumFromProps")
        b = _up(wts)
        api.fa_tarboton_dev(_up(dem), nd, b)
        _same(host, _down(b), "fm_tarboton + accumulation against fa_tarboton_dev")

        for method, xp, code in (("Holmgren", 4.0, 0), ("Quinn", None, 2), ("D4", None, 3)):
            dem = _dem(shape, dtype)
            host = api.FlowProportions(dem, method, nodata=nd, exponent=xp)
            p = _empty((h, w, 9), np.float32)
            t = _up(dem)
            _ok(api, getattr(L, f"rdgpu_fm_mfd_dev_{s}")(_p(t), api._scalar(s, nd), w, h, code, ctypes.c_double(xp or 1.0), _p(p),
                                                         _stream(api)), "fm_mfd_dev")
            _same(host, _down(p), "fm_mfd " + method)
            if method != "D4":   # (see the docstring: their accumulation does not repeat itself bit for bit)
                continue
            wts = _values(shape, np.float64) / 4.0
            host = api.FlowAccumulation(dem, method, nodata=nd, weights=wts, exponent=xp)
            a = _up(wts)
            api.fa_mfd_dev(_up(dem), nd, method, a, exponent=xp)
            _same(host, _down(a), "fa_mfd " + method)


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_mfd_distance(api, dtype):
    for shape in SHAPES:
        nd = _nodata(dtype)
        for want in (("dist",), ("drop",), ("dist", "drop")):
            dem = _dem(shape, dtype)
            chan = _mask(shape)
            for flats in (False, True):
                host = (api.dinf_distance_down_flats if flats else api.dinf_distance_down)(dem, nd, chan, "ave", False, (2.0, 3.0), -1.0, want)
                planes = {k: _empty(shape, np.float64) for k in want}
                (api.dinf_distance_down_flats_dev if flats else api.dinf_distance_down_dev)(_up(dem), nd, _up(chan), "ave", False,
                                                                                            (2.0, 3.0), -1.0, **planes)
                assert set(host) == set(want)
                for k in want:
                    _same(host[k], _down(planes[k]), f"dinf_distance_down{'_flats' if flats else ''}: {k} of {want}")
            # over a proportions array, elevations of the element type under test
            props = api.FlowProportions(_dem(shape, dtype), "Freeman", nodata=nd, exponent=1.5)
            elev = _values(shape, np.float64)
            chan = _mask(shape) if "drop" in want else None
            host = api.mfd_distance_down(props, chan, elev, "max", True, (1.0, 1.0), -1.0, want)
            planes = {k: _empty(shape, np.float64) for k in want}
            api.mfd_distance_down_dev(_up(props), None if chan is None else _up(chan), _up(elev), "max", True, (1.0, 1.0), -1.0, **planes)
            for k in want:
                _same(host[k], _down(planes[k]), f"mfd_distance_down: {k} of {want}")


# ---- terrain -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_terrain(api, dtype):
    L = api.lib()
    names = api.TERRAIN_ATTRIBUTES
    for shape in SHAPES:
        h, w = shape
        s, nd = api._suffix(dtype), _nodata(dtype)
        dem = _dem(shape, dtype)
        host = api.terrain_attribute(dem, "aspect", nd, 2.0, (3.0, 5.0))          # a mask of one plane
        a = _empty(shape, np.float32)
        api.terrain_attribute_dev(_up(dem), "aspect", nd, a, 2.0, (3.0, 5.0))
        _same(host, _down(a), "terrain_attribute")

        dem = _dem(shape, dtype)
        host = api.terrain_attributes(dem, names, nd, 2.0, (3.0, 5.0))            # every plane
        outs = {k: _empty(shape, np.float32) for k in names}
        api.terrain_attributes_dev(_up(dem), names, nd, outs, 2.0, (3.0, 5.0))
        for k in names:
            _same(host[k], _down(outs[k]), "terrain_attributes: " + k)

        # several planes of the eight: a pointer is given for every plane, the ones outside the mask are not written
        some = (1, 4, 7)
        planes = [np.full(shape, FILL, np.uint8).repeat(4, axis=1).view(np.float32) for _ in names]
        ptrs = (ctypes.c_void_p * len(names))(*[p.ctypes.data for p in planes])
        _ok(api, getattr(L, f"rdgpu_terrain_attributes_{s}")(_hp(dem), api._ta_scalar(s, nd), w, h, ctypes.c_double(3.0),
                                                             ctypes.c_double(5.0), ctypes.c_float(2.0),
                                                             ctypes.c_uint(sum(1 << k for k in some)), ptrs, ctypes.c_float(-9999)),
            "rdgpu_terrain_attributes")
        for k, name in enumerate(names):
            if k in some:
                _same(planes[k], host[name], "terrain_attributes, three planes: " + name)
            else:
                assert (planes[k].view(np.uint8) == FILL).all(), name + " was not requested but written"

        for which in ("spi", "cti"):
            acc, slope = _values(shape, np.float64) + 1.0, _values(shape, np.float32) / 16
            acc[0, 0], slope[-1, -1] = -1.0, -9999.0
            host = getattr(api, "terrain_" + which)(acc, slope, -1.0, -9999.0, (2.0, 3.0))
            a = _empty(shape, np.float32)
            getattr(api, f"terrain_{which}_dev")(_up(acc), _up(slope), a, -1.0, -9999.0, (2.0, 3.0))
            _same(host, _down(a), which)


# ---- the D8 forest engines -------------------------------------------------------------------------------------------------
def test_upslope(api):
    for shape in SHAPES:
        h, w = shape
        dirs = _dirs(api, shape)
        host = api.d8_upslope_cells(dirs, 1, 1, w - 2, h - 2)
        a = _empty(shape, np.uint8)
        api.d8_upslope_cells_dev(_up(dirs), 1, 1, w - 2, h - 2, a)
        _same(host, _down(a), "d8_upslope_cells")

        dirs = _dirs(api, shape)
        rng = np.random.default_rng(next(_SEED))
        cells = rng.choice(h * w, 7, replace=False).astype(np.uint32)
        labels = np.arange(10, 17, dtype=np.int32)
        host = api.d8_catchments(dirs, cells, labels, unreached=-3)
        a = _empty(shape, np.int32)
        api.d8_catchments_dev(_up(dirs), _up(cells.view(np.int32)), _up(labels), a, unreached=-3)
        _same(host, _down(a), "d8_catchments")
        a = _empty(shape, np.int32)
        api.d8_catchments_dev(_up(dirs), _up(cells.view(np.int32))[:0].contiguous(), _up(labels)[:0].contiguous(), a, unreached=-3)
        _same(api.d8_catchments(dirs, cells[:0], labels[:0], unreached=-3), _down(a), "d8_catchments, no seeds")

        dirs = _dirs(api, shape)
        host = api.d8_outlets(dirs)
        a = _empty(shape, np.uint32)
        api.d8_outlets_dev(_up(dirs), a)
        _same(host, _down(a, np.uint32), "d8_outlets")


def test_streams(api):
    for shape in SHAPES:
        acc = _values(shape, np.float64)
        acc[0, 0] = -1.0
        host = api.d8_channels(acc, 150.0)
        a = _empty(shape, np.uint8)
        api.d8_channels_dev(_up(acc), 150.0, a)
        _same(host, _down(a), "d8_channels")

        for with_chan in (False, True):
            dirs = _dirs(api, shape)
            chan = _mask(shape, 0.5) if with_chan else None
            dchan = None if chan is None else _up(chan)
            order = api.d8_stream_order(dirs, 255, chan)
            a = _empty(shape, np.uint8)
            api.d8_stream_order_dev(_up(dirs), a, 255, dchan)
            _same(order, _down(a), "d8_stream_order")
            host = api.d8_stream_links(dirs, order, 255, chan)
            a = _empty(shape, np.uint8)
            api.d8_stream_links_dev(_up(dirs), _up(order), a, 255, dchan)
            _same(host, _down(a), "d8_stream_links")


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_flow_path_and_hand(api, dtype):
    for shape in SHAPES:
        h, w = shape
        tshape = {"to_cell": (shape, np.uint32), "steps": ((3, h, w), np.uint32), "dist": (shape, np.float64)}
        dirs, chan = _dirs(api, shape), _mask(shape)
        full = api.d8_flow_path(dirs, 255, chan, (2.0, 3.0), -7.0, want=("to_cell", "steps", "dist"))
        for want in (("to_cell",), ("steps",), ("dist",), ("to_cell", "steps", "dist")):   # each plane alone, then all
            host = api.d8_flow_path(dirs, 255, chan, (2.0, 3.0), -7.0, want=want)
            planes = {k: _empty(*tshape[k]) for k in want}
            api.d8_flow_path_dev(_up(dirs), 255, _up(chan), (2.0, 3.0), -7.0, **planes)
            assert set(host) == set(want)
            for k in want:
                _same(host[k], _down(planes[k], tshape[k][1]), f"d8_flow_path: {k} of {want}")
                _same(host[k], full[k], f"d8_flow_path: {k} alone against all")

        for with_chan in (False, True):
            dirs, dem = _dirs(api, shape), _dem(shape, dtype)
            chan = _mask(shape) if with_chan else None
            host = api.d8_hand(dem, dirs, _nodata(dtype), 255, chan)
            a = _empty(shape, np.float64)
            api.d8_hand_dev(_up(dem), _up(dirs), _nodata(dtype), a, 255, None if chan is None else _up(chan))
            _same(host, _down(a), "d8_hand")


def test_stream_reaches(api):
    rec = api.REACH_DTYPE
    for shape in SHAPES:
        dirs, chan = _dirs(api, shape), _mask(shape, 0.4)
        order = api.d8_stream_order(dirs, 255, chan)
        full = api.d8_stream_reaches(dirs, 255, chan, order, (2.0, 3.0))
        n = full["count"]
        assert n == len(full["table"])
        for want in (("table",), ("table", "reach"), ("table", "catchment"), ("reach",), ("table", "reach", "catchment")):
            host = api.d8_stream_reaches(dirs, 255, chan, order, (2.0, 3.0), want=want)
            assert set(host) == set(want) | {"count"} and host["count"] == n
            planes = {k: _empty(shape, np.uint32) for k in want if k != "table"}
            table = _empty((max(n, 1) * rec.itemsize,), np.uint8) if "table" in want else None
            count = api.d8_stream_reaches_dev(_up(dirs), 255, _up(chan), _up(order), (2.0, 3.0), table=table, **planes)
            assert int(_down(count)[0]) == n
            for k in planes:
                _same(host[k], _down(planes[k], np.uint32), f"d8_stream_reaches: {k} of {want}")
                _same(host[k], full[k], f"d8_stream_reaches: {k} of {want} against all")
            if table is not None:
                _same(host["table"], _down(table).view(rec)[:n], f"d8_stream_reaches: table of {want}")
                _same(host["table"], full["table"], f"d8_stream_reaches: table of {want} against all")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])   # (float32 is the widest type the entry has)
def test_upslope_extreme(api, dtype):
    for shape in SHAPES:
        dirs, vals = _dirs(api, shape), _values(shape, dtype)
        full = api.d8_upslope_extreme(dirs, vals, "min", 3)
        for want in (("extreme",), ("at_cell",), ("extreme", "at_cell")):
            host = api.d8_upslope_extreme(dirs, vals, "min", 3, want=want)
            planes = {k: _empty(shape, dtype if k == "extreme" else np.uint32) for k in want}
            api.d8_upslope_extreme_dev(_up(dirs), _up(vals), "min", 3, **planes)
            for k in want:
                _same(host[k], _down(planes[k], host[k].dtype), f"d8_upslope_extreme: {k} of {want}")
                _same(host[k], full[k], f"d8_upslope_extreme: {k} alone against all")


def test_longest_flow_path(api):
    for shape in SHAPES:
        h, w = shape
        tshape = {"from_cell": (shape, np.uint32), "steps": ((3, h, w), np.uint32), "length": (shape, np.float64),
                  "on_basin_path": (shape, np.uint8)}
        dirs = _dirs(api, shape)
        full = api.d8_longest_flow_path(dirs, 255, (2.0, 3.0), -7.0, want=tuple(tshape))
        for want in (("from_cell",), ("steps",), ("length",), ("on_basin_path",), tuple(tshape)):
            host = api.d8_longest_flow_path(dirs, 255, (2.0, 3.0), -7.0, want=want)
            planes = {k: _empty(*tshape[k]) for k in want}
            api.d8_longest_flow_path_dev(_up(dirs), 255, (2.0, 3.0), -7.0, **planes)
            assert set(host) == set(want)
            for k in want:
                _same(host[k], _down(planes[k], tshape[k][1]), f"d8_longest_flow_path: {k} of {want}")
                _same(host[k], full[k], f"d8_longest_flow_path: {k} alone against all")


@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_weighted_accumulation_and_upstream_length(api, dtype):
    for shape in SHAPES:
        h, w = shape
        dirs, wts = _dirs(api, shape), _values(shape, dtype)
        host = api.d8_flow_accum_weighted(dirs, wts, 7, 255, -2)
        a = _empty(shape, host.dtype)
        api.d8_flow_accum_weighted_dev(_up(dirs), _up(wts), 7, a, 255, -2)
        _same(host, _down(a), "d8_flow_accum_weighted")

        tshape = {"steps": ((3, h, w), np.uint32), "length": (shape, np.float64)}
        dirs = _dirs(api, shape)
        full = api.d8_total_upstream_length(dirs, 2.0, 3.0)
        for want in (("steps",), ("length",), ("steps", "length")):
            host = api.d8_total_upstream_length(dirs, 2.0, 3.0, want=want)
            planes = {k: _empty(*tshape[k]) for k in want}
            api.d8_total_upstream_length_dev(_up(dirs), 2.0, 3.0, **planes)
            for k in want:
                _same(host[k], _down(planes[k], tshape[k][1]), f"d8_total_upstream_length: {k} of {want}")
                _same(host[k], full[k], f"d8_total_upstream_length: {k} alone against all")


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_keep_their_text_and_leave_nothing_behind(api):
    """Rejected on the host before any GPU work: the caller's arrays are untouched, the next valid call succeeds."""
    L = api.lib()
    shape = (9, 5)
    h, w = shape

    def refused(rc, text):
        assert rc == 2, rc                                         # RDGPU_ERR_ARG
        assert L.rdgpu_last_error().decode() == text

    acc, slope = _values(shape, np.float64) + 1.0, _values(shape, np.float32)
    out = np.full(shape, FILL, np.uint8).repeat(4, axis=1).view(np.float32)
    args = (ctypes.c_double(-1.0), _hp(slope), ctypes.c_float(-9999.0), w, h, ctypes.c_double(1.0), ctypes.c_double(1.0))
    refused(L.rdgpu_ta_spi(_hp(acc), ctypes.c_double(-1.0), None, ctypes.c_float(-9999.0), w, h, ctypes.c_double(1.0), ctypes.c_double(1.0),
                           _hp(out)), "rdgpu_ta_spi / _cti: null pointer")
    refused(L.rdgpu_ta_spi(_hp(acc), ctypes.c_double(-1.0), _hp(slope), ctypes.c_float(-9999.0), w, 0, ctypes.c_double(1.0),
                           ctypes.c_double(1.0), _hp(out)), "rdgpu_ta_spi / _cti: width and height must be positive")
    refused(L.rdgpu_ta_spi(_hp(acc), ctypes.c_double(-1.0), _hp(slope), ctypes.c_float(-9999.0), w, h, ctypes.c_double(0.0),
                           ctypes.c_double(1.0), _hp(out)), "rdgpu_ta_spi / _cti: the cell lengths must be finite and non-zero")
    assert (out.view(np.uint8) == FILL).all()
    del args
    host = api.terrain_spi(acc, slope, -1.0, -9999.0)
    a = _empty(shape, np.float32)
    api.terrain_spi_dev(_up(acc), _up(slope), a)
    _same(host, _down(a), "spi after the refused calls")

    dirs = _dirs(api, shape)
    dist = np.full(shape, FILL, np.uint8).repeat(8, axis=1).view(np.float64)
    one = ctypes.c_double(1.0)
    refused(L.rdgpu_d8_flow_path(_hp(dirs), ctypes.c_uint8(255), w, h, None, one, one, None, None, None, ctypes.c_double(-1.0)),
            "rdgpu_d8_flow_path: no output requested")
    refused(L.rdgpu_d8_flow_path(None, ctypes.c_uint8(255), w, h, None, one, one, None, None, _hp(dist), ctypes.c_double(-1.0)),
            "rdgpu_d8_flow_path: null pointer")
    assert (dist.view(np.uint8) == FILL).all()
    host = api.d8_flow_distance(dirs)
    a = _empty(shape, np.float64)
    api.d8_flow_distance_dev(_up(dirs), a)
    _same(host, _down(a), "flow distance after the refused calls")

    dem = _dem(shape, np.float64)
    kept = dem.copy()
    refused(L.rdgpu_fill_f64(_hp(dem), w, h, 5), "rdgpu_fill: topology must be 8 or 4")
    refused(L.rdgpu_fill_f64(None, w, h, 8), "rdgpu_fill: null DEM pointer")
    _same(dem, kept, "the DEM of a refused fill")
    host = api.FillDepressions(dem)
    t = _up(dem)
    api.fill_depressions_dev(t)
    _same(host, _down(t), "fill after the refused calls")
