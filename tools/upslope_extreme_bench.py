#!/usr/bin/env python3
"""Upslope extremes at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of d8_upslope_extreme -- `extreme`
alone, `at_cell` alone and both for the maximum, both for the minimum -- on the flat-resolved directions of G(seed=3) with
the float32 filled DEM as the values, with d8_outlets and d8_flow_accum (u8 -> f64) on the same directions as the
yardsticks, measured before and after.  Writes profiles/upslope_extreme_bench.json (--out): per line the ms (median of the
repeats, min / max as the spread), the algorithmic bytes per cell (inputs read once, outputs written once), GB/s at that
traffic and the fraction of the 8 TB/s HBM peak, the ratio to d8_outlets, then the per-kernel times of one profiled call
of each line.  A failure stops the run: nothing is launched after it."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upslope_extreme_bench.json"))
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
    out32 = torch.empty((n, n), dtype=torch.int32, device="cuda")
    ext = torch.empty((n, n), dtype=torch.float32, device="cuda")
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

    # bytes per cell: directions 1 and the f32 values 4 in; extreme 4, at_cell 4 out
    products = (("d8_flow_accum_f64", lambda: rd.d8_flow_accum_dev(dirs, area), 9),
                ("d8_outlets", lambda: rd.d8_outlets_dev(dirs, out32), 5),
                ("d8_upslope_extreme:max:extreme", lambda: rd.d8_upslope_extreme_dev(dirs, Z, "max", -9999.0, extreme=ext), 9),
                ("d8_upslope_extreme:max:at_cell", lambda: rd.d8_upslope_extreme_dev(dirs, Z, "max", -9999.0, at_cell=out32), 9),
                ("d8_upslope_extreme:max:extreme+at_cell",
                 lambda: rd.d8_upslope_extreme_dev(dirs, Z, "max", -9999.0, extreme=ext, at_cell=out32), 13),
                ("d8_upslope_extreme:min:extreme+at_cell",
                 lambda: rd.d8_upslope_extreme_dev(dirs, Z, "min", -9999.0, extreme=ext, at_cell=out32), 13),
                ("d8_outlets:again", lambda: rd.d8_outlets_dev(dirs, out32), 5),
                ("d8_flow_accum_f64:again", lambda: rd.d8_flow_accum_dev(dirs, area), 9))
    for name, fn, bpc in products:
        line(name, fn, bpc)
        if name.endswith("extreme+at_cell"):
            idx_differs = int((out32.view(-1) != torch.arange(cells, dtype=torch.int32, device="cuda")).sum().item())
            res["lines"][name]["cells_whose_extreme_sits_elsewhere"] = idx_differs
    L = res["lines"]
    outlets = min(L["d8_outlets"]["ms"], L["d8_outlets:again"]["ms"])
    acc = min(L["d8_flow_accum_f64"]["ms"], L["d8_flow_accum_f64:again"]["ms"])
    res["ms_over_d8_outlets_ms"] = {k: round(v["ms"] / outlets, 3) for k, v in L.items() if k.startswith("d8_upslope_extreme")}
    res["ms_over_flow_accum_ms"] = {k: round(v["ms"] / acc, 3) for k, v in L.items() if k.startswith("d8_upslope_extreme")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))


if __name__ == "__main__":
    main()
