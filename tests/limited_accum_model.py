"""A plain Python model of the limited D8 accumulation (include/rdgpu.h, "limited accumulation on the D8 direction forest"):
in-degrees over the links and a Kahn queue, serial, with fractions.Fraction totals, so that nothing is ever rounded and
"exact" has a meaning.  A cell the queue never releases lies on a direction loop: its out is 0 and it keeps what reached
it.  Factors and capacities must be finite or NaN (+inf is allowed for a capacity): a Fraction has no infinity.
The forest helpers are tests/weighted_accum_model.py's; the hand-written rasters in tests/test_limited_accum_model.py pin
this file."""
import math
import os
import sys
from collections import deque
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weighted_accum_model as wm  # noqa: E402


def limited(dirs, supply, supply_nodata, capacity=None, factor=None, dir_nodata=255, nodata_out=-1.0):
    """a dict: "out", "kept" float64 [h, w] (the exact values rounded to double once; nodata_out where a cell does not
    participate), "out_exact", "kept_exact" (flat lists of Fraction, None there), "loop" (bool [h, w]), "link" (flat list,
    -1: none), "part" (flat list), and "result": the four sums of the contract as exact Fractions"""
    assert supply.shape == dirs.shape
    h, w = dirs.shape
    n = h * w
    part, link, _ = wm.links(dirs, dir_nodata)
    con = wm.contributes(supply, supply_nodata)
    sv = np.ascontiguousarray(supply).ravel().astype(np.float64).tolist()        # exact
    cap = None if capacity is None else np.ascontiguousarray(capacity).ravel().astype(np.float64).tolist()
    fac = None if factor is None else np.ascontiguousarray(factor).ravel().astype(np.float64).tolist()
    total = [Fraction(sv[c]) if part[c] and con[c] else Fraction(0) for c in range(n)]
    supplied = sum((total[c] for c in range(n) if part[c]), Fraction(0))

    def node(c, t):
        a = t
        if fac is not None and not math.isnan(fac[c]):
            a = Fraction(fac[c]) * t
        a = max(a, Fraction(0))
        if cap is not None and not math.isnan(cap[c]) and cap[c] != math.inf:
            a = min(a, max(Fraction(cap[c]), Fraction(0)))
        return a

    indeg = [0] * n
    for c in range(n):
        if link[c] >= 0:
            indeg[link[c]] += 1
    out = [None] * n
    queue = deque(c for c in range(n) if part[c] and indeg[c] == 0)
    while queue:
        c = queue.popleft()
        out[c] = node(c, total[c])
        t = link[c]
        if t < 0:
            continue
        total[t] += out[c]
        indeg[t] -= 1
        if indeg[t] == 0:
            queue.append(t)
    loop = [part[c] and out[c] is None for c in range(n)]
    kept = [None] * n
    for c in range(n):
        if part[c]:
            if loop[c]:
                out[c] = Fraction(0)
            kept[c] = total[c] - out[c]
    res = {"supplied": supplied,
           "left": sum((out[c] for c in range(n) if part[c] and link[c] < 0), Fraction(0)),
           "kept_pos": sum((kept[c] for c in range(n) if part[c] and kept[c] > 0), Fraction(0)),
           "kept_neg": sum((kept[c] for c in range(n) if part[c] and kept[c] < 0), Fraction(0))}
    assert res["supplied"] == res["left"] + res["kept_pos"] + res["kept_neg"]    # the mass balance, exactly

    def plane(v):
        return np.array([float(v[c]) if part[c] else float(nodata_out) for c in range(n)], np.float64).reshape(h, w)

    return {"out": plane(out), "kept": plane(kept), "out_exact": out, "kept_exact": kept,
            "loop": np.array(loop, bool).reshape(h, w), "link": link, "part": part, "result": res}


def bound(dirs, supply, supply_nodata, dir_nodata=255):
    """per cell (flat list of Fraction): the contract's bound g * (sum of |s| over T(v)), g = k u / (1 - k u), u = 2^-53,
    k the cells of T(v) -- EVERY cell of T(v), not only the contributing ones: a cell that adds nothing still rounds
    what it passes on when there is a factor"""
    h, w = dirs.shape
    part, link, _ = wm.links(dirs, dir_nodata)
    con = wm.contributes(supply, supply_nodata)
    sv = np.ascontiguousarray(supply).ravel().astype(np.float64).tolist()
    start = [(abs(Fraction(sv[c])) if part[c] and con[c] else Fraction(0), 1 if part[c] else 0) for c in range(h * w)]
    acc = wm._kahn(part, link, start, lambda a, b: (a[0] + b[0], a[1] + b[1]))
    u = Fraction(1, 2**53)
    return [k * u / (1 - k * u) * mag for mag, k in acc]


# ---- for the cross-check against the reference's MoveWaterIntoPits (tests/golden/ref_limited.npz) -----------------------
def reference_cases():
    """yields (name, dirs uint8, label, [(supply float64, wtd after, water_vol)] per water table) of make_golden_limited.py.
    The reference takes a cell that flows into raster index 0 for a pit (its NO_FLOW test is on the neighbour's address,
    fill_spill_merge.hpp:282-292): those links are cut here, and every table is <= 0 at cell 0."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_limited.npz")) as g:
        for name in g["cases"].tolist():
            dirs = g[name + "/flowdirs"].astype(np.uint8)
            _, link, _ = wm.links(dirs)
            flat = dirs.reshape(-1)
            for c, t in enumerate(link):
                if t == 0:
                    flat[c] = 0
            tables = [(g[f"{name}/w{k}/before"].astype(np.float64) / 1024.0, g[f"{name}/w{k}/after"], g[f"{name}/w{k}/water_vol"])
                      for k in range(4)]
            yield name, dirs, g[name + "/label"], tables


def per_label_left(out, link, label, count):
    """float64 [count]: the out (float64 [h, w], multiples of 2^-10) of the cells without a link, summed per label in
    integers: exactly"""
    units = np.round(out * 1024.0).astype(np.int64)
    assert np.array_equal(units / 1024.0, out)
    acc = np.zeros(count, np.int64)
    ends = np.array(link).reshape(out.shape) < 0
    np.add.at(acc, label[ends].astype(np.int64), units[ends])
    return acc / 1024.0
