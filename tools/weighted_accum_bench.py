#!/usr/bin/env python3
"""Weighted D8 accumulation and total upstream length at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of
d8_flow_accum_weighted with u8, i32, f32 and f64 weights and of d8_total_upstream_length (`length` alone, and with `steps`)
on the flat-resolved directions of G(seed=3), alternated with the yardsticks measured in the same run: d8_flow_accum
(u8 -> f64) on the same directions, fa_d8_dev with non-unit weights (the same walk behind a direction pass of its own, on
FM_D8 directions of the filled DEM, which end at every lake: the new f64 call is timed on such directions too), and
flow_accumulation_dev on the MATERIALISED proportions of the same directions with
the same f64 weights -- until now the only route to this result.  The proportions take 36 B per cell, so that route runs at
--generic-size (default 20000), next to the new f64 call at that size, and its output is compared with the new call's
(integer-valued weights: equality).  For that comparison alone the border codes are zeroed first: the generic engine, like the reference, counts the
dependencies of interior cells only.  fa_d8_dev and flow_accumulation_dev take their weights in the output array, so each
call is preceded by a device copy of the weights, which is timed alone as well.
Writes profiles/weighted_accum_bench.json (--out): per line the ms (median of the repeats, min / max as the spread), the
algorithmic bytes per cell (inputs read once, outputs written once), GB/s at that traffic and the fraction of the 8 TB/s
HBM peak, then the per-kernel times of one profiled call of each line.  A failure stops the run: nothing is launched after
it."""
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
    ap.add_argument("--generic-size", type=int, default=20000)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_accum_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    res = {"size": args.size, "generic_size": args.generic_size, "launches_per_repeat": args.launches, "repeats": args.repeats,
           "hbm_peak_bytes_per_s": HBM_PEAK, "lines": {}, "kernels": {}}

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

    def line(name, fn, bytes_per_cell, cells, profile=True):
        ms = timed(fn)
        med = ms[len(ms) // 2]
        bps = cells * bytes_per_cell / (med * 1e-3)
        res["lines"][name] = {"ms": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                              "bytes_per_cell": bytes_per_cell, "GB_per_s": round(bps / 1e9, 1),
                              "fraction_of_hbm_peak": round(bps / HBM_PEAK, 4)}
        print(name, res["lines"][name], flush=True)
        if not profile:
            return
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels"][name] = {k: {"ms": round(v[0], 4), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels"][name], flush=True)

    def scene(n, zero_border=False):
        """the filled DEM of G(seed=3), its flat-resolved directions, integer-valued weights"""
        Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
        rd.synth_dem_dev(Z, seed=3)
        rd.fill_depressions_dev(Z)
        dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
        rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
        if zero_border:
            for edge in (dirs[0, :], dirs[-1, :], dirs[:, 0], dirs[:, -1]):
                edge[edge != 255] = 0
        w8 = (torch.arange(n, device="cuda", dtype=torch.int32)[:, None] * 7 + torch.arange(n, device="cuda", dtype=torch.int32)[None, :] * 13) % 9 + 1
        return Z, dirs, w8.to(torch.uint8)

    # ---- the generic route, at the size its proportions fit ------------------------------------------------------------
    g = args.generic_size
    if g:
        Z, dirs, w8 = scene(g, zero_border=True)
        w64 = w8.to(torch.float64)
        props = torch.zeros((g, g, 9), dtype=torch.float32, device="cuda")
        props[..., 0] = torch.where(dirs == 255, -2.0, torch.where((dirs >= 1) & (dirs <= 8), 0.0, -1.0))
        for c in range(1, 9):
            props[..., c] = (dirs == c).to(torch.float32)
        acc = torch.empty((g, g), dtype=torch.float64, device="cuda")
        new = torch.empty((g, g), dtype=torch.float64, device="cuda")

        def generic():
            acc.copy_(w64)
            rd.flow_accumulation_dev(props, acc)

        cells = g * g
        line(f"weights_copy_f64@{g}", lambda: acc.copy_(w64), 16, cells, profile=False)
        line(f"d8_flow_accum_weighted:f64@{g}", lambda: rd.d8_flow_accum_weighted_dev(dirs, w64, -9999.0, new), 17, cells)
        line(f"flow_accumulation_dev:props9@{g}", generic, 52, cells)
        line(f"d8_flow_accum_weighted:f64@{g}:again", lambda: rd.d8_flow_accum_weighted_dev(dirs, w64, -9999.0, new), 17, cells)
        generic()
        rd.d8_flow_accum_weighted_dev(dirs, w64, -9999.0, new)
        torch.cuda.synchronize()
        res["generic_equals_weighted_cells_differing"] = int((acc != new).sum().item())
        print("generic route vs the new call, cells differing:", res["generic_equals_weighted_cells_differing"], flush=True)
        if res["generic_equals_weighted_cells_differing"]:
            raise SystemExit("the generic route and d8_flow_accum_weighted differ")
        L = res["lines"]
        newms = min(L[f"d8_flow_accum_weighted:f64@{g}"]["ms"], L[f"d8_flow_accum_weighted:f64@{g}:again"]["ms"])
        copy = L[f"weights_copy_f64@{g}"]["ms"]
        gl = L[f"flow_accumulation_dev:props9@{g}"]
        res["generic_route"] = {"new_f64_ms": newms, "generic_ms_min_less_copy": round(gl["ms_min"] - copy, 4),
                                "generic_ms_median_less_copy": round(gl["ms"] - copy, 4),
                                "new_is_not_slower": bool(newms <= gl["ms_min"] - copy)}
        print(res["generic_route"], flush=True)
        del Z, dirs, w8, w64, props, acc, new
        torch.cuda.empty_cache()
        rd.release_workspace()

    # ---- the new calls and the D8 yardsticks ---------------------------------------------------------------------------
    n = args.size
    cells = n * n
    Z, dirs, w8 = scene(n)
    torch.cuda.synchronize()
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    w64 = w8.to(torch.float64)
    sum_i = torch.empty((n, n), dtype=torch.int64, device="cuda")
    sum_f = sum_i.view(torch.float64)
    lakes = torch.empty((n, n), dtype=torch.uint8, device="cuda")

    def fa_d8():
        area.copy_(w64)
        rd.fa_d8_dev(Z, -9999.0, area)

    def weighted(wts, out):
        return lambda: rd.d8_flow_accum_weighted_dev(dirs, wts, 0, out)

    line("d8_flow_accum_f64", lambda: rd.d8_flow_accum_dev(dirs, area), 9, cells)
    line("weights_copy_f64", lambda: area.copy_(w64), 16, cells, profile=False)
    line("fa_d8_dev:non_unit", fa_d8, 20, cells)
    line("d8_flow_accum_weighted:u8", weighted(w8, sum_i), 10, cells)
    ref = sum_i.clone()
    line("d8_flow_accum_weighted:f64", weighted(w64, sum_f), 17, cells)
    res["f64_equals_u8_cells_differing"] = int((sum_f != ref.to(torch.float64)).sum().item())
    wts = w8.to(torch.int32)
    line("d8_flow_accum_weighted:i32", weighted(wts, sum_i), 13, cells)
    res["i32_equals_u8_cells_differing"] = int((sum_i != ref).sum().item())
    wts = w8.to(torch.float32)
    line("d8_flow_accum_weighted:f32", weighted(wts, sum_f), 13, cells)
    del wts, ref
    # the same call on the directions fa_d8_dev walks: those of the filled DEM WITHOUT flat resolution, which end at every lake
    rd.d8_flow_directions_dev(Z, -9999.0, lakes, flats=False)
    line("d8_flow_accum_weighted:f64:unresolved_directions", lambda: rd.d8_flow_accum_weighted_dev(lakes, w64, 0, sum_f), 17, cells)
    line("fa_d8_dev:non_unit:again", fa_d8, 20, cells)
    line("d8_flow_accum_f64:again", lambda: rd.d8_flow_accum_dev(dirs, area), 9, cells)
    del w64, sum_f, sum_i, lakes
    torch.cuda.empty_cache()
    length = torch.empty((n, n), dtype=torch.float64, device="cuda")
    line("d8_total_upstream_length:length", lambda: rd.d8_total_upstream_length_dev(dirs, 30.0, 30.0, length=length), 9, cells)
    steps = torch.empty((3, n, n), dtype=torch.int32, device="cuda")
    line("d8_total_upstream_length:steps+length",
         lambda: rd.d8_total_upstream_length_dev(dirs, 30.0, 30.0, steps=steps, length=length), 21, cells)
    rd.d8_flow_accum_dev(dirs, area)
    part = dirs != 255
    links = steps.to(torch.int64).sum(dim=0)
    res["steps_sum_equals_area_minus_1_cells_differing"] = int(((links.to(torch.float64) != area - 1.0) & part).sum().item())
    L = res["lines"]
    acc = min(L["d8_flow_accum_f64"]["ms"], L["d8_flow_accum_f64:again"]["ms"])
    copy = L["weights_copy_f64"]["ms"]
    fa = min(L["fa_d8_dev:non_unit"]["ms"], L["fa_d8_dev:non_unit:again"]["ms"]) - copy
    new = [k for k in L if k.startswith("d8_flow_accum_weighted") and "@" not in k or k.startswith("d8_total")]
    res["fa_d8_dev_non_unit_ms_less_copy"] = round(fa, 4)
    res["ms_over_flow_accum_ms"] = {k: round(L[k]["ms"] / acc, 3) for k in new}
    res["ms_over_fa_d8_non_unit_ms"] = {k: round(L[k]["ms"] / fa, 3) for k in new}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))


if __name__ == "__main__":
    main()
