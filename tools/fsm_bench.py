#!/usr/bin/env python3
"""Fill-Spill-Merge at 40000 x 40000 (f32, G(seed=3), HBM resident) in ONE run from one build: HIP-event time per call of
rdgpu_fill_spill_merge_dev_f32 on the hierarchy of the bench's DEM, for three uniform waters -- span * 1e-4, span * 3e-3 and
span * 0.05 on every interior cell, span the DEM's elevation range, each rounded to a multiple of 2^-10 -- and, for the
ratio, of rdgpu_depression_hierarchy_dev_f32, rdgpu_depressions_dev_f32 and rdgpu_fill_dev_f32 on the same DEM.  The pour
runs on the host between two waits for the stream; the events bracket the whole call, the host time included.  Writes
profiles/fsm_bench.json (--out): per line the ms (median of the repeats after a warm-up, min / max as the spread); per water
the records sorted, the lakes, the longest pour, the shortcut hits and the host pass's share of the call; the ratios to the
three yardsticks; then the per-stage times of one profiled call of each line ("fsm.host_pass" is the host stage: the two
transfers, the checks, the pour and the lake tops), stamped with the git SHA.  A failure stops the run: nothing is launched
after it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dephier_bench import git_sha  # noqa: E402

WATERS = (("span_1e-4", 1e-4), ("span_3e-3", 3e-3), ("span_0.05", 0.05))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsm_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z0 = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z0, seed=3)
    span = float(Z0.max()) - float(Z0.min())
    Z = torch.empty_like(Z0)
    labels = torch.empty((n, n), dtype=torch.int32, device="cuda")
    nodes, leaves = (int(v) for v in rd.depression_hierarchy_dev(Z0, None, None).cpu())   # the sizing call
    htable = torch.empty(max(nodes, 1) * rd.DEPHIER_NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    rd.depression_hierarchy_dev(Z0, labels, htable)
    lakes = int(rd.depressions_dev(Z0, None, None).item())
    itable = torch.empty((max(lakes, 1), 5), dtype=torch.float64, device="cuda")
    water = torch.empty((n, n), dtype=torch.float64, device="cuda")
    depth = torch.empty_like(water)
    res = {"git_sha": git_sha(), "size": n, "dtype": "f32", "seed": 3, "repeats": args.repeats, "span": span, "nodes": nodes,
           "leaves": leaves, "depressions": lakes, "waters": {}, "lines": {}, "kernels_ms": {}}
    print("span:", span, "nodes:", nodes, "leaves:", leaves, "lakes:", lakes, flush=True)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def line(name, fn, before=lambda: None):
        before()
        once(fn)                                                                  # the warm-up
        ms = []
        for _ in range(args.repeats):
            before()
            ms.append(once(fn))
        ms.sort()
        res["lines"][name] = {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}
        print(name, res["lines"][name], flush=True)
        before()
        torch.cuda.synchronize()
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels_ms"][name] = {k: round(v[0], 4) for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels_ms"][name], flush=True)

    for name, f in WATERS:
        v = max(round(span * f * 1024.0), 1) / 1024.0
        water.fill_(v)
        water[0, :] = 0
        water[-1, :] = 0
        water[:, 0] = 0
        water[:, -1] = 0
        key = "fill_spill_merge_dev_f32:" + name
        out = {}
        line(key, lambda: out.update(r=rd.fill_spill_merge_dev(Z0, labels, htable, nodes, water, depth)))
        r = out["r"].cpu().numpy().view(rd.FSM_RESULT_DTYPE)[0]
        st = rd.fsm_stats()
        ms = res["lines"][key]["ms"]
        res["waters"][name] = {"water_per_cell": v, "water_in": float(r["water_in"]), "ocean": float(r["ocean"]),
                               "standing": float(r["standing"]), "lakes": int(r["lakes"]), "full_lakes": int(r["full_lakes"]),
                               "records": st["records"], "longest_pour": st["longest_pour"], "shortcut_hits": st["shortcut_hits"],
                               "pours": st["pours"], "sort_bits": st["sort_bits"], "host_ms": round(st["host_ms"], 3),
                               "host_share": round(res["kernels_ms"][key].get("fsm.host_pass", 0.0) / ms, 4)}
        print(" ", res["waters"][name], flush=True)
    line("depression_hierarchy_dev_f32:labels", lambda: rd.depression_hierarchy_dev(Z0, labels, htable))
    line("depressions_dev_f32:labels", lambda: rd.depressions_dev(Z0, labels, itable))
    line("fill_dev_f32", lambda: rd.fill_depressions_dev(Z), before=lambda: Z.copy_(Z0))
    L = res["lines"]
    for name, _ in WATERS:
        key = "fill_spill_merge_dev_f32:" + name
        for other, short in (("depression_hierarchy_dev_f32:labels", "hierarchy"), ("depressions_dev_f32:labels", "depressions"),
                             ("fill_dev_f32", "fill")):
            res[f"{key}/{short}"] = round(L[key]["ms"] / L[other]["ms"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels_ms")}))


if __name__ == "__main__":
    main()
