"""GPU parity tests: the directions-only flat resolution where its level planes end (csrc/flat_planes.inc keeps the two
breadth-first level fields as 16 bit planes per 64 x 64 tile; include/rdgpu.h: the plane engine "steps aside by itself when a
level does not fit 16 bits" and the call is repeated on the int engine).

The rasters (flat_depth_cases.py; checked on the CPU in test_flat_depth_model.py) are serpentine channels whose towards-lower
levels end at exactly D.  D sweeps 0xFEF0 .. 0x10110 -- every point at which a 16-bit encoding can end (0xFFFF = the "not
reached" pattern, 0x10000 = the first level that wraps, one 256-level segment of a visit below them) -- and far beyond, with
the channel inside one tile column or crossing a tile seam every 64 levels, at vertical and at horizontal seams, and with the
seams moved against the levels.  Every assertion on directions is byte equality with the oracle on every cell.

Which engine ran is asserted too (flat_stats()["plane_repeats"]): planes alone up to D = 0xFE00, the repeat on ints from
D = 0x10000 on -- without that, a limit set far too low would pass every equality test."""
import time

import numpy as np
import pytest

import flat_depth_cases as fc

pytestmark = pytest.mark.gpu


def assert_same_dirs(got, exp, dem, what):
    if np.array_equal(got, exp):
        return
    bad = got != exp
    missing = int((bad & (got == 0)).sum())
    first = np.argwhere(bad)[:4].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} directions differ ({missing} missing, {int(bad.sum()) - missing} wrong), "
                         f"{int((bad & (dem == fc.CHANNEL)).sum())} in the channel; first {first} "
                         f"got {[int(got[tuple(p)]) for p in first]} exp {[int(exp[tuple(p)]) for p in first]}")


def assert_engine(depth, stats, what):
    """The plane engine alone up to 0xFE00; a repeat on ints from 0x10000 on (no 16-bit word holds such a level, and
    0xFFFF is taken); in between either is right."""
    r = stats["plane_repeats"]
    assert r in (0, 1), (what, stats)
    if depth <= 0xFE00:
        assert r == 0, (what, stats)
    if depth >= 0x10000:
        assert r == 1, (what, stats)


def run_case(rd, case, what=""):
    dem, exp = fc.build(case), fc.expected(case)
    t0 = time.perf_counter()
    got = rd.barnes_flat_resolution_d8(dem, fc.NODATA)
    ms = (time.perf_counter() - t0) * 1e3
    st = rd.flat_stats()
    name = fc.case_id(case) + what
    print(f"{name}: {dem.shape[0]} x {dem.shape[1]}, {ms:.1f} ms, plane_repeats {st['plane_repeats']}, "
          f"rounds towards {st['towards']}, tail visits {st['tail_visits']}")
    assert_same_dirs(got, exp, dem, name)
    assert_engine(case[3], st, name)


@pytest.mark.parametrize("case", fc.SWEEP, ids=fc.case_id)
def test_depth_sweep(rd, orc, case):
    """The channel ends inside a tile at depth D."""
    run_case(rd, case)


@pytest.mark.parametrize("case", fc.SEAMS, ids=fc.case_id)
def test_seam_sweep(rd, orc, case):
    """The channel runs 600 levels past 0x10000, crossing a seam about every 64 levels; the eight shifts put a crossing at
    every residue of 8 within the window where an edge level would read as "not reached" or wrap."""
    run_case(rd, case)


@pytest.mark.parametrize("switch", ["RDGPU_FLAT_ASYNC=0", "RDGPU_FLAT_ASYNC=100000", "RDGPU_FLAT_STATIC=0"])
@pytest.mark.parametrize("case", fc.SCHEDULE_CASES, ids=fc.case_id)
def test_schedules(rd, orc, monkeypatch, case, switch):
    """Rounds to the end, the asynchronous tail from the first batch on, the towards search in host-decided batches."""
    monkeypatch.setenv(*switch.split("="))
    run_case(rd, case, " " + switch)


@pytest.mark.parametrize("case", fc.ROUTE_CASES, ids=fc.case_id)
def test_device_entry_on_a_side_stream(rd, orc, case):
    import torch

    dem, exp = fc.build(case), fc.expected(case)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        z = torch.from_numpy(dem).cuda(non_blocking=True)
        z2 = z + 0                                              # (queued work the call must come after)
        dirs = torch.empty(z.shape, dtype=torch.uint8, device="cuda")
        rd.d8_flow_directions_dev(z2, fc.NODATA, dirs, flats=True)
        st = rd.flat_stats()
        out = dirs + 0                                          # (... and work that must come after it)
    side.synchronize()
    assert_same_dirs(out.cpu().numpy(), exp, dem, fc.case_id(case))
    assert np.array_equal(z2.cpu().numpy(), dem), "the input tensor was changed"
    assert_engine(case[3], st, fc.case_id(case))


def canon(labels):
    """Canonical partition ids: 1 + lowest cell index of each label (0 stays 0)."""
    flat = labels.ravel()
    ids, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    out = (first + 1)[inv.ravel()]
    out[flat == 0] = 0
    return out.reshape(labels.shape).astype(labels.dtype)


@pytest.mark.parametrize("case", fc.ROUTE_CASES, ids=fc.case_id)
def test_masks_and_labels_on_the_int_engine(rd, orc, case):
    dem, exp = fc.build(case), fc.expected(case)
    dirs, mask, labels = rd.resolve_flats(dem, fc.NODATA)
    _, emask, elabels = orc.port.resolve_flats(dem, fc.NODATA)
    assert_same_dirs(dirs, exp, dem, fc.case_id(case))
    assert int(emask.max()) == 2 * case[3]
    assert np.array_equal(mask, emask), "flat_mask differs"
    assert np.array_equal(labels, canon(elabels)), "flat partition differs"


@pytest.mark.parametrize("case", fc.ROUTE_CASES, ids=fc.case_id)
def test_three_row_blocks(rd, orc, case):
    import torch

    from richdem_amd.sharded import flat_resolution_blocks

    dem, exp = fc.build(case), fc.expected(case)
    got, _ = flat_resolution_blocks(torch.from_numpy(dem).cuda(), fc.NODATA, 3)
    assert_same_dirs(got.cpu().numpy(), exp, dem, fc.case_id(case))
