#!/usr/bin/env python3
"""Terrain attributes at 40000 x 40000 float32, HBM resident: HIP-event time per launch of rise/run, degrees, aspect, profile
curvature and of the fused launches {rise/run, aspect, curvature} and all eight, with d8_flow_directions (the same stencil
shape, 5 B/cell) timed IN THE SAME RUN as the yardstick.  Writes profiles/terrain_bench.json (--out): per line
the ms (median of the repeats, with min / max as the run-to-run spread), GB/s at 4 * (1 + k) B/cell for k outputs and the
fraction of the 8 TB/s HBM peak.  A failure stops the run: nothing is launched after it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    names = rd.TERRAIN_ATTRIBUTES
    planes = {a: torch.empty((n, n), dtype=torch.float32, device="cuda") for a in names}
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    cells = n * n
    res = {"size": n, "dtype": "float32", "launches_per_repeat": args.launches, "repeats": args.repeats,
           "hbm_peak_bytes_per_s": HBM_PEAK, "lines": {}}

    def timed(fn):
        for _ in range(3):
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

    line("d8_flow_directions", lambda: rd.d8_flow_directions_dev(Z, -9999.0, dirs), 5)
    for a in ("slope_riserun", "slope_degrees", "aspect", "profile_curvature"):
        line(a, lambda a=a: rd.terrain_attribute_dev(Z, a, -9999.0, planes[a]), 8)
    three = ("slope_riserun", "aspect", "curvature")
    line("fused:slope_riserun+aspect+curvature", lambda: rd.terrain_attributes_dev(Z, three, -9999.0, planes), 4 * 4)
    line("fused:all_eight", lambda: rd.terrain_attributes_dev(Z, names, -9999.0, planes), 4 * 9)
    for a in names:
        if a not in res["lines"]:
            line(a, lambda a=a: rd.terrain_attribute_dev(Z, a, -9999.0, planes[a]), 8)
    line("d8_flow_directions:again", lambda: rd.d8_flow_directions_dev(Z, -9999.0, dirs), 5)
    L = res["lines"]
    singles = sum(L[a]["ms"] for a in names)
    res["sum_of_eight_single_launches_ms"] = round(singles, 4)
    res["fused_all_eight_over_sum_of_singles"] = round(L["fused:all_eight"]["ms"] / singles, 4)
    res["riserun_fraction_over_flowdirs_fraction"] = round(
        L["slope_riserun"]["fraction_of_hbm_peak"] / max(L["d8_flow_directions"]["fraction_of_hbm_peak"],
                                                        L["d8_flow_directions:again"]["fraction_of_hbm_peak"]), 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "lines"}))


if __name__ == "__main__":
    main()
