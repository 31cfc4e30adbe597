#!/usr/bin/env python3
"""Limited D8 accumulation at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of d8_flow_accum_limited_dev
(f64 rasters) on the flat-resolved directions of G(seed=3) with no limits, with a capacity raster, with a factor raster, with
both, and with `out` alone in place of both planes, next to the yardstick d8_flow_accum_weighted_dev with the same f64
supply.  The lines ALTERNATE: after one warm-up call of each, every round times one call of each line in turn, --repeats
rounds (default 5); the JSON holds the median with min and max as the spread, the algorithmic bytes per cell (inputs read
once, outputs written once), GB/s at that traffic and the fraction of the 8 TB/s HBM peak, the per-kernel times of one
profiled call of each line, and each line's ratio to the yardstick beside the ratio of their algorithmic bytes.
The supply is non-negative and integer-valued, so the call with no limits must equal the yardstick on every cell: checked.
Writes profiles/limited_accum_bench.json (--out).  A failure stops the run: nothing is launched after it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
YARDSTICK = "d8_flow_accum_weighted:f64"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limited_accum_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    cells = n * n
    res = {"size": n, "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK, "lines": {}, "kernels": {}}
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    del Z
    torch.cuda.empty_cache()
    ix = torch.arange(n, device="cuda", dtype=torch.int32)
    pattern = ix[:, None] * 7 + ix[None, :] * 13
    supply = (pattern % 9 + 1).to(torch.float64)
    cap = (pattern % 61 + 4).to(torch.float64)               # 4 .. 64: binds wherever more than a few cells drain
    fac = torch.where(pattern % 5 == 0, 0.5, 1.0).to(torch.float64)
    del pattern, ix
    out = torch.empty((n, n), dtype=torch.float64, device="cuda")
    kept = torch.empty((n, n), dtype=torch.float64, device="cuda")
    ref = torch.empty((n, n), dtype=torch.float64, device="cuda")
    result = torch.zeros(4, dtype=torch.float64, device="cuda")

    def limited(c, f, o, k, r=None):
        return lambda: rd.d8_flow_accum_limited_dev(dirs, supply, 0.0, c, f, out=o, kept=k, result=r)

    # name -> (call, algorithmic bytes per cell: directions 1, every f64 raster read or written 8)
    lines = {
        YARDSTICK: (lambda: rd.d8_flow_accum_weighted_dev(dirs, supply, 0.0, ref), 17),
        "d8_flow_accum_limited:none": (limited(None, None, out, kept), 25),
        "d8_flow_accum_limited:capacity": (limited(cap, None, out, kept), 33),
        "d8_flow_accum_limited:factor": (limited(None, fac, out, kept), 33),
        "d8_flow_accum_limited:both": (limited(cap, fac, out, kept), 41),
        "d8_flow_accum_limited:none:out_alone": (limited(None, None, out, None), 17),
        "d8_flow_accum_limited:both:out_alone": (limited(cap, fac, out, None), 33),
        "d8_flow_accum_limited:both:with_result": (limited(cap, fac, out, kept, result), 41),
    }
    for fn, _ in lines.values():                             # the warm-up
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in lines}
    for _ in range(args.repeats):
        for name, (fn, _) in lines.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    for name, (fn, bpc) in lines.items():
        t = sorted(ms[name])
        med = t[len(t) // 2]
        bps = cells * bpc / (med * 1e-3)
        res["lines"][name] = {"ms": round(med, 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4), "bytes_per_cell": bpc,
                              "GB_per_s": round(bps / 1e9, 1), "fraction_of_hbm_peak": round(bps / HBM_PEAK, 4)}
        print(name, res["lines"][name], flush=True)
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels"][name] = {k: {"ms": round(v[0], 4), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels"][name], flush=True)
    # no limits, supplies >= 0: the yardstick's sums, and nothing kept
    lines[YARDSTICK][0]()
    lines["d8_flow_accum_limited:none"][0]()
    torch.cuda.synchronize()
    part = dirs != 255
    res["none_equals_weighted_cells_differing"] = int((out != ref).sum().item())
    res["none_kept_nonzero_cells"] = int(((kept != 0) & part).sum().item())
    lines["d8_flow_accum_limited:both:with_result"][0]()
    torch.cuda.synchronize()
    r = result.cpu().tolist()
    res["both_result"] = dict(zip(("supplied", "left", "kept_pos", "kept_neg"), r))
    res["both_balance_residual"] = r[0] - (r[1] + r[2] + r[3])
    res["both_cells_clamped_or_decayed"] = int(((kept > 0) & part).sum().item())
    if res["none_equals_weighted_cells_differing"] or res["none_kept_nonzero_cells"]:
        raise SystemExit("the call with no limits and d8_flow_accum_weighted differ")
    L = res["lines"]
    yard = L[YARDSTICK]
    res["ms_over_yardstick_ms"] = {k: round(L[k]["ms"] / yard["ms"], 3) for k in L if k != YARDSTICK}
    res["bytes_over_yardstick_bytes"] = {k: round(L[k]["bytes_per_cell"] / yard["bytes_per_cell"], 3) for k in L if k != YARDSTICK}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))


if __name__ == "__main__":
    main()
