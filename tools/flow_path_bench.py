#!/usr/bin/env python3
"""Flow-path products at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of d8_flow_path -- dist alone
without a channel mask, to_cell + dist with channels at >= 100 and at >= 10 000 cells of accumulation -- and of d8_hand
(float32 DEM) at the >= 100 threshold, with d8_outlets (the same three-stage structure, 4 B/cell out) and d8_flow_accum
(u8 -> f64) on the same directions as the yardsticks, measured before and after.  Directions: the engine's fill -> flat
resolution of G(seed=3).  Writes profiles/flow_path_bench.json (--out): per line the ms (median of the repeats, min / max
as the spread), the algorithmic bytes per cell (inputs read once, outputs written once), GB/s at that traffic and the
fraction of the 8 TB/s HBM peak, the ratio to d8_outlets, then the per-kernel times of one profiled call of each line.
A failure stops the run: nothing is launched after it."""
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
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_path_bench.json"))
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
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, area)
    chans = {}
    for thr in (1e2, 1e4):
        chans[thr] = torch.empty((n, n), dtype=torch.uint8, device="cuda")
        rd.d8_channels_dev(area, thr, chans[thr])
    out32 = torch.empty((n, n), dtype=torch.int32, device="cuda")
    dist = torch.empty((n, n), dtype=torch.float64, device="cuda")
    res = {"size": n, "launches_per_repeat": args.launches, "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK,
           "lines": {}, "kernels": {}}

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
        res["kernels"][name] = {k: {"ms": round(v[0], 4), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels"][name], flush=True)

    # bytes per cell: directions 1 (+ mask 1) in; to_cell 4, dist 8, hand 8 out; the f32 DEM 4 in and one gathered read 4
    products = (("d8_flow_accum_f64", lambda: rd.d8_flow_accum_dev(dirs, area), 9),
                ("d8_outlets", lambda: rd.d8_outlets_dev(dirs, out32), 5),
                ("d8_flow_path:dist", lambda: rd.d8_flow_path_dev(dirs, dist=dist), 9),
                ("d8_flow_path:to_cell+dist:threshold_100",
                 lambda: rd.d8_flow_path_dev(dirs, 255, chans[1e2], to_cell=out32, dist=dist), 14),
                ("d8_flow_path:to_cell+dist:threshold_10000",
                 lambda: rd.d8_flow_path_dev(dirs, 255, chans[1e4], to_cell=out32, dist=dist), 14),
                ("d8_hand_f32:threshold_100", lambda: rd.d8_hand_dev(Z, dirs, -9999.0, dist, 255, chans[1e2]), 18),
                ("d8_outlets:again", lambda: rd.d8_outlets_dev(dirs, out32), 5),
                ("d8_flow_accum_f64:again", lambda: rd.d8_flow_accum_dev(dirs, area), 9))
    for name, fn, bpc in products:
        line(name, fn, bpc)
        if name.startswith("d8_flow_path:to_cell"):
            res["lines"][name]["cells_with_a_drainage_cell"] = int((out32 != -1).sum().item())
    L = res["lines"]
    outlets = min(L["d8_outlets"]["ms"], L["d8_outlets:again"]["ms"])
    acc = min(L["d8_flow_accum_f64"]["ms"], L["d8_flow_accum_f64:again"]["ms"])
    res["ms_over_d8_outlets_ms"] = {k: round(v["ms"] / outlets, 3) for k, v in L.items() if k.startswith(("d8_flow_path", "d8_hand"))}
    res["ms_over_flow_accum_ms"] = {k: round(v["ms"] / acc, 3) for k, v in L.items() if k.startswith(("d8_flow_path", "d8_hand"))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))


if __name__ == "__main__":
    main()
