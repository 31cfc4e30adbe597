#!/usr/bin/env python3
"""The depression hierarchy with a caller-given ocean, and BucketFillFromEdges, at 40000 x 40000 (f32, G(seed=3), HBM
resident: the DEM of tools/dephier_bench.py) in ONE run from one build.  HIP-event time per call, the host time of the
hierarchy's builder included.

(a) Hierarchy, labels written: the entry without a mask (the yardstick), ocean = NULL, the ring mask, and a sea mask -- the
    DEM with everything below its 25 % quantile set to that quantile, the mask the bucket fill of that level from the
    edges.  The four lines are timed in alternation, `repeats` rounds after one warm-up round, so that a drift of the
    machine falls on all of them alike; per line the median, min and max, and `spread_ms` = max - min of the yardstick.
(b) Bucket fill on that sea, on a raster whose every cell is eligible, and on a one-cell-wide serpentine channel; beside
    them d8_flow_directions on the DEM, a one-pass yardstick; the launches of one profiled call of each input.  Every
    timed fill starts from a zeroed mask, the memset inside the timed interval.

Writes profiles/dephier_ocean_bench.json (--out), stamped with the git SHA.  A failure stops the run: nothing is launched
after it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def git_sha():
    if os.environ.get("RDGPU_GIT_SHA"):
        return os.environ["RDGPU_GIT_SHA"]
    try:
        with open(os.path.join(ROOT, ".gitsha")) as f:
            return f.read().strip()
    except OSError:
        pass
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dephier_ocean_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z0 = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z0, seed=3)
    labels = torch.empty((n, n), dtype=torch.int32, device="cuda")
    # the sea: the 25 % quantile of a strided sample of the DEM; everything below it becomes that level
    sample = Z0.flatten()[::max(Z0.numel() // (1 << 22), 1)]
    q = float(torch.quantile(sample[:1 << 22], 0.25))
    Zsea = torch.clamp(Z0, min=q)
    sea = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    sea_cells = int(rd.bucket_fill_from_edges_dev(Zsea, q, sea).cpu()[0])
    ring = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    ring[0, :] = ring[-1, :] = 1
    ring[:, 0] = ring[:, -1] = 1
    nodes = {"plain": int(rd.depression_hierarchy_dev(Z0, None, None).cpu()[0]),
             "sea": int(rd.depression_hierarchy_dev(Zsea, None, None, ocean=sea).cpu()[0])}
    htable = torch.empty(max(nodes.values()) * rd.DEPHIER_NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    res = {"git_sha": git_sha(), "size": n, "dtype": "f32", "seed": 3, "repeats": args.repeats, "sea_level": q, "sea_cells": sea_cells,
           "nodes": nodes, "hierarchy": {}, "bucket_fill": {}, "kernels_ms": {}}
    print("sea level", q, "sea cells", sea_cells, "nodes", nodes, flush=True)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def profiled(name, fn):
        torch.cuda.synchronize()
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        tot = {k: v for k, v in rd.profile_totals().items() if v[1]}
        res["kernels_ms"][name] = {k: round(v[0], 4) for k, v in tot.items()}
        return tot

    def summary(ms):
        ms = sorted(ms)
        return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}

    # (a) the four hierarchy lines in alternation
    hier = (("entry_without_mask", lambda: rd.depression_hierarchy_dev(Z0, labels, htable)),
            ("ocean_null", lambda: rd.depression_hierarchy_dev(Z0, labels, htable, ocean=None)),
            ("ring_mask", lambda: rd.depression_hierarchy_dev(Z0, labels, htable, ocean=ring)),
            ("sea_mask", lambda: rd.depression_hierarchy_dev(Zsea, labels, htable, ocean=sea)))
    times = {name: [] for name, _ in hier}
    for r in range(args.repeats + 1):
        for name, fn in hier:
            ms = timed(fn)
            if r:                                                                 # round 0 is the warm-up
                times[name].append(ms)
    for name, fn in hier:
        res["hierarchy"][name] = summary(times[name])
        print(name, res["hierarchy"][name], flush=True)
    y = res["hierarchy"]["entry_without_mask"]
    res["hierarchy"]["spread_ms"] = round(y["ms_max"] - y["ms_min"], 3)
    for name in ("ocean_null", "ring_mask", "sea_mask"):
        res["hierarchy"][name + "/entry_without_mask"] = round(res["hierarchy"][name]["ms"] / y["ms"], 4)
    for name, fn in hier[2:]:
        profiled("hierarchy:" + name, fn)

    # (b) the bucket fill
    del labels, htable
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    mask = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    full = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    serp = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    serp[1:n - 1:2, 1:n - 1] = 1
    serp[2:n - 2:4, n - 2] = 1
    serp[4:n - 2:4, 1] = 1
    serp[0, 1] = 1

    def fill(check, value):
        def run():
            mask.zero_()
            return rd.bucket_fill_from_edges_dev(check, value, mask)
        return run

    lines = (("d8_flow_directions", lambda: rd.d8_flow_directions_dev(Z0, -9999.0, dirs)),
             ("bucket_fill:sea", fill(Zsea, q)), ("bucket_fill:all_eligible", fill(full, 0)), ("bucket_fill:serpentine", fill(serp, 1)))
    times = {name: [] for name, _ in lines}
    for r in range(args.repeats + 1):
        for name, fn in lines:
            ms = timed(fn)
            if r:
                times[name].append(ms)
    for name, fn in lines:
        res["bucket_fill"][name] = summary(times[name])
        if name.startswith("bucket_fill"):
            res["bucket_fill"][name]["filled"] = int(fn().cpu()[0])
            tot = profiled(name, fn)
            res["bucket_fill"][name]["launches"] = int(sum(v[1] for k, v in tot.items() if k.startswith("bucketfill.")))
        print(name, res["bucket_fill"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernels_ms"}))


if __name__ == "__main__":
    main()
