#!/usr/bin/env python3
"""The longest upstream flow path at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of
d8_longest_flow_path -- `length` alone, `from_cell + length`, and all four planes -- on the flat-resolved directions of
G(seed=3), cells of 30 x 10.5.  The yardsticks are measured in the same run, before and after: the two products this one
composes, d8_flow_path (steps + dist, no mask) and d8_upslope_extreme_f32 (both planes, the filled DEM as the values), and
d8_outlets.  Writes profiles/longest_path_bench.json (--out): per line the ms (median of the repeats, min / max as the
spread), the algorithmic bytes per cell (inputs read once, outputs written once), GB/s at that traffic and the fraction of
the 8 TB/s HBM peak; the ratios to the sum of the two composed products and to d8_outlets; then the per-kernel times of one
profiled call of each line and the kernel that dominates it.  A failure stops the run: nothing is launched after it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
CELL = (30.0, 10.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longest_path_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    cells = n * n
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    torch.cuda.synchronize()
    cell32 = torch.empty((n, n), dtype=torch.int32, device="cuda")
    steps = torch.empty((3, n, n), dtype=torch.int32, device="cuda")
    f64 = torch.empty((n, n), dtype=torch.float64, device="cuda")
    ext = torch.empty((n, n), dtype=torch.float32, device="cuda")
    mask = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    res = {"size": n, "cell": CELL, "launches_per_repeat": args.launches, "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK,
           "lines": {}, "kernels": {}, "dominant_kernel": {}}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.launches)
        return sorted(ms)

    def line(name, fn, bytes_per_cell):
        ms = timed(fn)
        med = ms[len(ms) // 2]
        bps = cells * bytes_per_cell / (med * 1e-3)
        res["lines"][name] = {"ms": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                              "bytes_per_cell": bytes_per_cell, "GB_per_s": round(bps / 1e9, 1),
                              "fraction_of_hbm_peak": round(bps / HBM_PEAK, 4)}
        print(name, res["lines"][name], flush=True)
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        k = {k: {"ms": round(v[0], 4), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}
        res["kernels"][name] = k
        res["dominant_kernel"][name] = max(k, key=lambda x: k[x]["ms"])
        print(" ", k, flush=True)

    # bytes per cell: directions 1 in (extremes: the f32 values 4 more); cell planes 4, steps 12, float64 planes 8, the mask 1 out
    products = (
        ("d8_outlets", lambda: rd.d8_outlets_dev(dirs, cell32), 5),
        ("d8_flow_path:steps+dist", lambda: rd.d8_flow_path_dev(dirs, cell=CELL, steps=steps, dist=f64), 21),
        ("d8_upslope_extreme_f32:max:extreme+at_cell",
         lambda: rd.d8_upslope_extreme_dev(dirs, Z, "max", -9999.0, extreme=ext, at_cell=cell32), 13),
        ("d8_longest_flow_path:length", lambda: rd.d8_longest_flow_path_dev(dirs, cell=CELL, length=f64), 9),
        ("d8_longest_flow_path:from_cell+length", lambda: rd.d8_longest_flow_path_dev(dirs, cell=CELL, from_cell=cell32, length=f64), 13),
        ("d8_longest_flow_path:all",
         lambda: rd.d8_longest_flow_path_dev(dirs, cell=CELL, from_cell=cell32, steps=steps, length=f64, on_basin_path=mask), 26),
        ("d8_upslope_extreme_f32:max:extreme+at_cell:again",
         lambda: rd.d8_upslope_extreme_dev(dirs, Z, "max", -9999.0, extreme=ext, at_cell=cell32), 13),
        ("d8_flow_path:steps+dist:again", lambda: rd.d8_flow_path_dev(dirs, cell=CELL, steps=steps, dist=f64), 21),
        ("d8_outlets:again", lambda: rd.d8_outlets_dev(dirs, cell32), 5))
    for name, fn, bpc in products:
        line(name, fn, bpc)
        if name == "d8_longest_flow_path:all":
            res["lines"][name]["cells_on_a_basin_main_path"] = int(mask.sum(dtype=torch.int64).item())
            res["lines"][name]["cells_whose_head_is_another_cell"] = int(
                (cell32.view(-1) != torch.arange(cells, dtype=torch.int32, device="cuda")).sum().item())
    L = res["lines"]
    both = lambda k: min(L[k]["ms"], L[k + ":again"]["ms"])  # noqa: E731
    outlets = both("d8_outlets")
    parents = both("d8_flow_path:steps+dist") + both("d8_upslope_extreme_f32:max:extreme+at_cell")
    res["flow_path_plus_extreme_ms"] = round(parents, 4)
    mine = {k: v for k, v in L.items() if k.startswith("d8_longest_flow_path")}
    res["ms_over_flow_path_plus_extreme_ms"] = {k: round(v["ms"] / parents, 3) for k, v in mine.items()}
    res["ms_over_d8_outlets_ms"] = {k: round(v["ms"] / outlets, 3) for k, v in mine.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))


if __name__ == "__main__":
    main()
