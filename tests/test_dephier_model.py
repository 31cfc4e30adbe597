"""The model of the depression hierarchy (tests/dephier_model.py: the contract of include/rdgpu.h in numpy / Python)
against the COMPILED REFERENCE's GetDepressionHierarchy (tests/golden/ref_dephier.npz, make_golden_dephier.py) in canonical
form, on rasters worked by hand, and against the definition of cells and volume taken literally.  No GPU.

The reference orders outlets that share their saddle cell arbitrarily, so both trees are compared after dropping every
internal node whose own level equals the level it was created at; nothing else is left out, and on the golden inputs such
nodes are fewer than 5 % of the internal nodes (asserted here and in the recipe)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from digest import load_golden  # noqa: E402
import dephier_model as dm  # noqa: E402

G = load_golden(os.path.join(GOLDEN, "ref_dephier.npz"))
CASES = sorted({k.split("/")[0] for k in G})
NONE = dm.NONE
NO_DEP = 0xFFFFFFFF


def _ref(name, t):
    """the reference's rows in the contract's conventions (make_golden_dephier.to_contract, restated: no import of the recipe)"""
    label, u, f = G[f"{name}/t{t}/labels"], G[f"{name}/t{t}/u32"], G[f"{name}/t{t}/f64"]

    def shift(a):
        a = a.astype(np.int64)
        return np.where(a == NO_DEP, NONE, a - 1)

    ocean_parent = (u[1:, 6] & 1).astype(bool)
    return {"labels": label.astype(np.int64) - 1, "parent": np.where(ocean_parent, NONE, shift(u[1:, 0])),
            "lchild": shift(u[1:, 1]), "rchild": shift(u[1:, 2]), "pit_cell": u[1:, 3].astype(np.int64), "level": f[1:, 0],
            "cells": (u[1:, 6] >> 1).astype(np.int64), "volume": f[1:, 2]}


def test_the_cases_are_the_ones_asked_for():
    shapes = {G[c + "/dem"].shape for c in CASES}
    assert shapes == {(30, 40), (129, 65), (130, 200), (257, 300)}
    assert {G[c + "/dem"].dtype for c in CASES} == {np.dtype(np.uint16), np.dtype(np.int32), np.dtype(np.float32)}
    for c in CASES:
        z = G[c + "/dem"]
        assert np.unique(z).size == z.size, c


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("name", CASES)
def test_model_equals_the_reference_in_canonical_form(name, t):
    dem = G[name + "/dem"]
    r = _ref(name, t)
    labels, tab = dm.hierarchy(dem, t)
    # labels: the reference's label translated through its pit cells; OCEAN is -1
    P = int(np.count_nonzero(tab["lchild"] == NONE)) if len(tab) else 0
    leaf_of_pit = {int(tab["pit_cell"][i]): i for i in range(P)}
    rl = r["labels"].ravel()
    trans = np.array([-1 if v < 0 else leaf_of_pit[int(r["pit_cell"][v])] for v in rl], np.int64)
    assert np.array_equal(trans, labels.ravel().astype(np.int64))
    assert P == int(np.count_nonzero(r["lchild"] == NONE))    # the same leaves
    mine, d_mine = dm.canonical(tab["parent"], tab["lchild"], tab["rchild"], tab["pit_cell"], tab["level"], tab["cells"],
                                tab["volume"])
    ref, d_ref = dm.canonical(r["parent"], r["lchild"], r["rchild"], r["pit_cell"], r["level"], r["cells"], r["volume"])
    # (the numbers of nodes may differ by the ties: two depressions that reach the outside over one saddle cell are two
    # roots in one order and one dissolved node above them in the other)
    for d, internal in ((d_mine, len(tab) - P), (d_ref, len(r["parent"]) - P)):
        assert d < 0.05 * max(internal, 1), (d_mine, d_ref, internal)
    # volumes: exact for the integer inputs; the f32 inputs are multiples of one power of two, so the reference's double
    # arithmetic is exact on them as well and the bound cells * 2^-52 * exact is met with nothing to spare
    assert mine == ref


@pytest.mark.parametrize("t", [8, 4])
@pytest.mark.parametrize("name", ["perm_u16_40x30", "perm_f32_40x30", "frac_f32_65x129"])
def test_cells_and_volume_are_their_definition(name, t):
    dem = G[name + "/dem"]
    labels, tab = dm.hierarchy(dem, t)
    for m, (cells, vol) in enumerate(dm.brute_cells_volume(dem, labels, tab)):
        assert tab["cells"][m] == cells and Fraction(float(tab["volume"][m])) == Fraction(float(vol)), m


def _check_tree(tab):
    P = int(np.count_nonzero(tab["lchild"] == NONE))
    for m in range(len(tab)):
        assert (tab["lchild"][m] == NONE) == (tab["rchild"][m] == NONE) == (m < P)
        if m >= P:
            a, b = int(tab["lchild"][m]), int(tab["rchild"][m])
            assert a < m and b < m and tab["parent"][a] == m and tab["parent"][b] == m
            assert tab["level"][a] == tab["level"][b] <= tab["level"][m]
            assert tab["pit_cell"][m] == tab["pit_cell"][a]
    return P


def test_two_pits_and_one_saddle():
    # cells of row 1:  7  8  9 10 11 12 13
    z = np.array([[9, 9, 9, 8, 9, 9, 9],
                  [9, 1, 6, 4, 7, 2, 9],
                  [9, 9, 9, 9, 9, 9, 9]], np.int32)
    lab, tab = dm.hierarchy(z, 4)
    # D4: cell 9 (6) descends to 8 (1); cell 10 (4) is a pit; cell 11 (7) descends to 12 (2), its lowest neighbour
    assert lab[1].tolist() == [-1, 0, 0, 1, 2, 2, -1]
    assert _check_tree(tab) == 3 and len(tab) == 5
    # edges by key: (6; 9, 10) joins leaves 0 and 1 into node 3; (7; 11, 10) joins leaf 2 and node 3 into node 4;
    # (8; 3, 10) makes node 4 a root
    assert tab["parent"].tolist() == [3, 3, 4, 4, NONE]
    assert (tab["lchild"][3], tab["rchild"][3]) == (0, 1) and (tab["lchild"][4], tab["rchild"][4]) == (3, 2)
    assert tab["level"].tolist() == [6, 6, 7, 7, 8]
    assert tab["inside_cell"].tolist() == [9, 10, 11, 10, 10] and tab["outside_cell"].tolist() == [10, 9, 10, 11, 3]
    assert tab["geolink"].tolist() == [1, 0, 1, 2, NONE]
    assert tab["pit_cell"].tolist() == [8, 10, 12, 8, 8] and tab["pit_elevation"].tolist() == [1, 4, 2, 1, 1]
    assert tab["cells"].tolist() == [2, 1, 2, 3, 5]          # the saddle cells count where dem == level: the reference's <=
    assert tab["volume"].tolist() == [5 + 0, 2, 0 + 5, 6 + 1 + 3, 7 + 2 + 4 + 1 + 6]


def test_three_basins_sharing_one_saddle_cell_have_a_fixed_order():
    # cell 12 (value 5) is the higher cell of the lowest edge between each two of the three basins (pits 6, 8 and 17)
    z = np.array([[9, 9, 9, 9, 9],
                  [9, 1, 9, 2, 9],
                  [9, 9, 5, 9, 9],
                  [9, 9, 3, 9, 9],
                  [9, 9, 9, 9, 9]], np.int32)
    lab, tab = dm.hierarchy(z, 8)
    assert lab.ravel()[[6, 8, 12, 17]].tolist() == [0, 1, 0, 2]          # the saddle descends to its lowest neighbour, 6
    assert _check_tree(tab) == 3 and len(tab) == 5
    # the two edges with hi = 12 come by ascending lo: (5; 12, 8) before (5; 12, 17)
    assert tab["parent"].tolist() == [3, 3, 4, 4, NONE]
    assert (tab["lchild"][3], tab["rchild"][3]) == (0, 1) and (tab["lchild"][4], tab["rchild"][4]) == (3, 2)
    assert tab["level"].tolist() == [5, 5, 5, 5, 9]
    assert tab["inside_cell"].tolist() == [12, 8, 17, 12, 6] and tab["outside_cell"].tolist() == [8, 12, 12, 17, 0]
    assert tab["geolink"].tolist() == [1, 0, 0, 2, NONE]
    kept, dissolved = dm.canonical(tab["parent"], tab["lchild"], tab["rchild"], tab["pit_cell"], tab["level"], tab["cells"],
                                   tab["volume"])
    assert dissolved == 1 and len(kept) == 4                 # node 3: created at 5, spills at 5


def test_a_pit_next_to_the_border_ring():
    z = np.array([[5, 5, 5, 5],
                  [5, 1, 3, 5],
                  [5, 5, 5, 4]], np.uint8)
    lab, tab = dm.hierarchy(z, 8)
    assert lab.tolist() == [[-1, -1, -1, -1], [-1, 0, 0, -1], [-1, -1, -1, -1]]
    assert len(tab) == 1 and tab["parent"][0] == NONE and tab["lchild"][0] == NONE
    # the lowest edge to the outside: hi = cell 11 (4), its only neighbour in the leaf is cell 6
    assert (tab["inside_cell"][0], tab["outside_cell"][0], tab["geolink"][0]) == (6, 11, NONE)
    assert (tab["level"][0], tab["cells"][0], tab["volume"][0], tab["pit_cell"][0]) == (4, 2, 3 + 1, 5)
    lab4, tab4 = dm.hierarchy(z, 4)
    assert (tab4["inside_cell"][0], tab4["outside_cell"][0], tab4["level"][0]) == (5, 1, 5)   # hi = 1: lowest index at 5


def test_a_plateau_of_equal_values():
    z = np.full((5, 6), 7, np.int16)
    z[1:4, 1:5] = 2                                         # twelve equal cells: ties go to the lower index
    lab, tab = dm.hierarchy(z, 8)
    # cell 7 is the pit; every other plateau cell points at its lowest-index neighbour
    assert (lab[1:4, 1:5] == 0).all() and len(tab) == 1
    assert (tab["pit_cell"][0], tab["level"][0], tab["cells"][0], tab["volume"][0]) == (7, 7, 12, 60)
    assert (tab["inside_cell"][0], tab["outside_cell"][0]) == (7, 0)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 7), (6, 8)])
def test_an_all_equal_raster_and_rasters_without_interior(shape):
    z = np.full(shape, 3, np.float32)     # (the interior of an all-equal raster descends by index to the border ring)
    lab, tab = dm.hierarchy(z, 8)
    assert len(tab) == 0 and (lab == -1).all()
