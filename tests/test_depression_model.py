"""The model of the depression inventory (tests/depression_model.py) on hand-written rasters whose answers are written out
here, and the no-GPU checks that the library and the package carry the feature."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depression_model import HAND, depressions_model  # noqa: E402

# per case and topology: the labelled cells (raster index -> label) and the records
# (first_cell, pit_cell, outlet_cell, cells, level, pit_elevation, volume)
EXPECTED = {
    ("single_pit", 8): ({4: 1}, [(4, 4, 0, 1, 5.0, 1.0, 4.0)]),
    ("single_pit", 4): ({4: 1}, [(4, 4, 1, 1, 5.0, 1.0, 4.0)]),
    # the two pits touch only diagonally: ONE depression under D8, TWO under D4
    ("diagonal_pits", 8): ({5: 1, 10: 1}, [(5, 5, 0, 2, 9.0, 1.0, 15.0)]),
    ("diagonal_pits", 4): ({5: 1, 10: 2}, [(5, 5, 1, 1, 9.0, 1.0, 8.0), (10, 10, 6, 1, 9.0, 2.0, 7.0)]),
    # a lake of 15 cells with two pits (2 and 1): one depression, its pit is the deeper one
    ("nested_pit", 8): ({c: 1 for r in (1, 2, 3) for c in range(7 * r + 1, 7 * r + 6)}, [(8, 18, 0, 15, 9.0, 1.0, 80.0)]),
    ("nested_pit", 4): ({c: 1 for r in (1, 2, 3) for c in range(7 * r + 1, 7 * r + 6)}, [(8, 18, 1, 15, 9.0, 1.0, 80.0)]),
    # two cells of the lowest elevation: the lower index is the pit
    ("equal_lowest", 8): ({5: 1, 6: 1}, [(5, 5, 0, 2, 7.0, 2.0, 10.0)]),
    ("equal_lowest", 4): ({5: 1, 6: 1}, [(5, 5, 1, 2, 7.0, 2.0, 10.0)]),
    # two rim cells at the spill level (5 and 9): the lower index is the outlet
    ("two_rim_cells", 8): ({6: 1, 7: 1, 8: 1}, [(6, 6, 5, 3, 5.0, 3.0, 6.0)]),
    ("two_rim_cells", 4): ({6: 1, 7: 1, 8: 1}, [(6, 6, 5, 3, 5.0, 3.0, 6.0)]),
    ("flat", 8): ({}, []),
    ("flat", 4): ({}, []),
    # the upper lake (cell 8) stands at 6, the lip (cell 9) is at that level and un-raised; the lower lake (cell 10) at 4
    ("cascade", 8): ({8: 1, 10: 2}, [(8, 8, 9, 1, 6.0, 2.0, 4.0), (10, 10, 17, 1, 4.0, 1.0, 3.0)]),
    ("cascade", 4): ({8: 1, 10: 2}, [(8, 8, 9, 1, 6.0, 2.0, 4.0), (10, 10, 17, 1, 4.0, 1.0, 3.0)]),
}


@pytest.mark.parametrize("name,topo", sorted(EXPECTED))
def test_model_on_hand_written_rasters(orc, name, topo):
    for dtype in (np.int32, np.float32):
        dem = np.array(HAND[name], dtype)
        labels, table = depressions_model(orc, dem, topo)
        cells, records = EXPECTED[(name, topo)]
        exp = np.zeros(dem.size, np.int32)
        for c, l in cells.items():
            exp[c] = l
        assert np.array_equal(labels.ravel(), exp)
        assert [tuple(r) for r in table.tolist()] == records


def test_every_case_has_an_answer():
    assert {n for n, _ in EXPECTED} == set(HAND)


def test_library_exports_the_depression_entries(rd):
    L = rd.lib()
    for s in ("u8", "i8", "i16", "u16", "i32", "u32", "f32", "f64", "i64", "u64"):
        for stem in ("rdgpu_depressions_", "rdgpu_depressions_dev_"):
            assert isinstance(getattr(L, stem + s), ctypes._CFuncPtr), stem + s


def test_package_has_depressions(rd):
    assert callable(rd.depressions) and callable(rd.depressions_dev)
    assert rd.DEPRESSION_DTYPE.itemsize == 40
    assert rd.DEPRESSION_DTYPE.names == ("first_cell", "pit_cell", "outlet_cell", "cells", "level", "pit_elevation", "volume")
