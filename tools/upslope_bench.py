#!/usr/bin/env python3
"""Upslope products at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of d8_outlets, d8_catchments with
1 and with 65 536 seeds and d8_upslope_cells at the main river's mouth, with d8_flow_accum (u8 -> f64) on the same
directions as the yardstick.  Directions: the engine's fill -> flat resolution of G(seed=3).  Writes
profiles/upslope_bench.json (--out): per line the ms (median of the repeats, min / max as the spread), GB/s at the
product's floor traffic (5 B/cell for the 4-byte outputs, 2 B/cell for upslope cells, 9 B/cell for the f64 accumulation)
and the fraction of the 8 TB/s HBM peak, then the per-kernel times of one profiled call of each product.  A failure stops
the run: nothing is launched after it."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upslope_bench.json"))
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
    del Z
    torch.cuda.empty_cache()
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, area)
    m = int(torch.argmax(area.view(-1)).item())
    mx, my = m % n, m // n
    out32 = torch.empty((n, n), dtype=torch.int32, device="cuda")
    out8 = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)
    seeds1 = torch.tensor([m], dtype=torch.int32, device="cuda")
    labels1 = torch.tensor([1], dtype=torch.int32, device="cuda")
    seeds64k = torch.randint(0, cells, (65536,), generator=gen, device="cuda").to(torch.int32)
    labels64k = torch.arange(1, 65537, dtype=torch.int32, device="cuda")
    res = {"size": n, "launches_per_repeat": args.launches, "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK,
           "mouth": [mx, my], "mouth_accum": float(area.view(-1)[m].item()), "lines": {}, "kernels_ms": {}}

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
        res["kernels_ms"][name] = {k: round(v[0], 4) for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels_ms"][name], flush=True)

    products = (("d8_flow_accum_f64", lambda: rd.d8_flow_accum_dev(dirs, area), 9),
                ("d8_outlets", lambda: rd.d8_outlets_dev(dirs, out32), 5),
                ("d8_catchments:1_seed", lambda: rd.d8_catchments_dev(dirs, seeds1, labels1, out32), 5),
                ("d8_catchments:65536_seeds", lambda: rd.d8_catchments_dev(dirs, seeds64k, labels64k, out32), 5),
                ("d8_upslope_cells:mouth", lambda: rd.d8_upslope_cells_dev(dirs, mx, my, mx, my, out8), 2),
                ("d8_flow_accum_f64:again", lambda: rd.d8_flow_accum_dev(dirs, area), 9))
    for name, fn, bpc in products:
        line(name, fn, bpc)
    L = res["lines"]
    res["outlets_ms_over_flow_accum_ms"] = round(L["d8_outlets"]["ms"] / min(L["d8_flow_accum_f64"]["ms"],
                                                                              L["d8_flow_accum_f64:again"]["ms"]), 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels_ms")}))


if __name__ == "__main__":
    main()
