#!/usr/bin/env python3
"""Makes tests/golden/pairs_list_cap.npz: rasters (50 rows of 100, float32) whose pair tile (0, 0) has an exact number of
boundary cells by tests/pairs_model.py -- the capacity of the pair pass's list (LIST_CAP, csrc/fill.hip) and one more,
and 1 024 and 1 025, each for D8 and for D4; no descent tile has more than NT_CAP nodes.  `<topo>_<n + 1>` is `<topo>_<n>`
with ONE cell changed.

    python tests/tools/make_pairs_list_cap.py

A seeded hill climb from smoothed white noise: one cell of the tile at a time is set to the mean of its four neighbours
or to a new random value, kept when the count moves towards the target."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pairs_model as pmod  # noqa: E402

H, W = 50, 100


def count(z, topo):
    ptr, lab = pmod.forest(z, topo)
    bc, nd = pmod.boundary_cells(lab, topo), pmod.nodes(ptr, z.shape)
    return int(bc[0, 0]), int(bc.max()), int(nd.max())


def start(seed, alpha=0.45):
    rng = np.random.default_rng(seed)
    a = rng.random((H + 2, W + 2))
    s = sum(a[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    return ((1 - alpha) * s + alpha * a[1:-1, 1:-1]).astype(np.float32)


def climb(z, topo, target, rng, one_cell=False):
    z = z.copy()
    c, _, _ = count(z, topo)
    for _ in range(200000):
        if c == target:
            return z
        y, x = int(rng.integers(1, pmod.TH - 1)), int(rng.integers(1, pmod.TW - 1))
        old = z[y, x]
        z[y, x] = np.float32((z[y - 1, x] + z[y + 1, x] + z[y, x - 1] + z[y, x + 1]) / 4) if rng.random() < 0.5 else np.float32(rng.random())
        c2, mx, nd = count(z, topo)
        ok = mx == c2 and nd <= pmod.NT_CAP and (c2 == target if one_cell else abs(c2 - target) < abs(c - target))
        if ok:
            c = c2
        else:
            z[y, x] = old
    raise SystemExit(f"no raster with {target} boundary cells found (D{topo})")


def main():
    out = {}
    for topo in (8, 4):
        rng = np.random.default_rng(100 + topo)
        z = start(7)
        c, mx, nd = count(z, topo)
        assert c == mx > 1025 and nd <= pmod.NT_CAP, (topo, c, mx, nd)
        for target in (1024, pmod.LIST_CAP):
            z = climb(z, topo, target, rng)
            out[f"d{topo}_{target}"] = z.copy()
            out[f"d{topo}_{target + 1}"] = climb(z, topo, target + 1, rng, one_cell=True)
            assert int((out[f"d{topo}_{target}"] != out[f"d{topo}_{target + 1}"]).sum()) == 1
    for k, z in out.items():
        print(k, count(z, int(k[1])))
    np.savez_compressed(pmod.GOLDEN, **out)
    print(pmod.GOLDEN, os.path.getsize(pmod.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
