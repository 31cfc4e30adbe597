#!/usr/bin/env python3
"""What would a coarse lower bound of the filled surface let the fill's pair pass (k_pairs16) skip, and what would it cost?

    make -C richdem_amd/csrc probe
    RDGPU_LIB=richdem_amd/librdgpu_probe.so python tools/probes/coarse_flood.py [--size 40000] [--out FILE]

For CB in --blocks: the raster of CB x CB block minima of the bench DEM is filled with the library's own fill (LB).  A path of
cells to the border maps to a path of blocks whose maximum is not larger, so LB(block(c)) <= W(c), the filled surface, and
an interior 64 x 64 descent tile whose blocks all have LB above the tile's largest cell lies wholly under one lake:
"flagged".  Measured here:

  (a) the flagged share, the census of tiles that the filled surface shows to be wholly under one lake, flagged <= census
      and LB <= W on every block, and the time of the coarse fill alone (best of --reps, its input restored outside the clock);
  (b) the launch time of the pair pass (the library's HIP-event profiler, "fill.scan") with exactly the flagged tiles
      handed to it as `skip` (rdgpu_probe_pairs_skip, probe build only), against the same fill without.  Nothing replaces
      the skipped tiles' pairs, so the rounds of such a fill do not finish and the surface is not written: only the
      kernel's time counts.

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

TILE = 64   # the descent tile's edge (csrc/fill.hip: DW, DH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--blocks", type=int, nargs="+", default=[64, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--part", choices=["a", "ab"], default="ab", help="a: the shares and the coarse fill's time only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    L = rd.lib()
    if not hasattr(L, "rdgpu_probe_pairs_skip"):
        raise SystemExit("not a probe build: set RDGPU_LIB to librdgpu_probe.so (make -C richdem_amd/csrc probe)")
    n = args.size
    if n % TILE or any(TILE % cb for cb in args.blocks):
        raise SystemExit("--size must be a multiple of 64 and every block size a divisor of 64 (whole blocks and tiles only)")
    nt = n // TILE
    sync = torch.cuda.synchronize
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=args.seed)
    W = Z.clone()
    rd.fill_depressions_dev(W)
    sync()
    stats0 = rd.fill_stats()

    def pool(a, k, op):   # k x k blocks of a square raster whose edge is a multiple of k
        m = a.shape[0] // k
        return getattr(a.view(m, k, m, k), op)(dim=(1, 3))

    tile_max = pool(Z, TILE, "amax")
    interior = torch.zeros((nt, nt), dtype=torch.bool, device="cuda")
    interior[1:-1, 1:-1] = True   # (a tile that touches the raster's border row or column is not interior)
    wmin, wmax = pool(W, TILE, "amin"), pool(W, TILE, "amax")
    census = interior & (wmin == wmax) & (wmin > tile_max)
    wblock = {cb: pool(W, cb, "amin") for cb in args.blocks}   # (W is scratch from here on)
    out = {"size": n, "seed": args.seed, "tiles": nt * nt, "census_tiles": int(census.sum()),
           "census_share": round(float(census.sum()) / (nt * nt), 4), "pair_records": stats0["edge_records"], "blocks": {}}

    def scan_times(skip, reps):
        """per fill: the launches' times of that fill, from the library's profiler"""
        runs = []
        assert L.rdgpu_probe_pairs_skip(ctypes.c_void_p(skip.data_ptr() if skip is not None else 0)) == 0
        try:
            for _ in range(reps):
                W.copy_(Z)
                sync()
                rd.profile_reset()
                rd.profile_enable(True)
                err = None
                try:
                    rd.fill_depressions_dev(W)
                    sync()
                except rd.RdgpuError as e:   # (expected with skipped tiles: basins without a pair never hook)
                    err = str(e)
                rd.profile_enable(False)
                tot = rd.profile_totals()
                runs.append({"scan_ms": tot["fill.scan"][0], "edge_round_ms": tot.get("fill.edge_round", (0.0, 0))[0],
                             "pair_records": rd.fill_stats()["edge_records"], "error": err})
        finally:
            assert L.rdgpu_probe_pairs_skip(ctypes.c_void_p(0)) == 0
        return runs

    if args.part == "ab":
        base = scan_times(None, args.reps)
        out["pairs_no_skip"] = {"runs": base, "scan_ms_fastest": min(r["scan_ms"] for r in base)}

    for cb in args.blocks:
        m0 = pool(Z, cb, "amin").contiguous()
        m = m0.clone()
        rd.fill_depressions_dev(m)   # workspace growth: not timed
        sync()
        cst = rd.fill_stats()
        times = []
        for _ in range(args.reps):
            m.copy_(m0)
            sync()
            t0 = time.perf_counter()
            rd.fill_depressions_dev(m)
            sync()
            times.append((time.perf_counter() - t0) * 1e3)
        lb_le_w = bool((m <= wblock[cb]).all())
        k = TILE // cb
        flag = interior & ((pool(m, k, "amin") if k > 1 else m) > tile_max)
        nflag = int(flag.sum())
        res = out["blocks"][str(cb)] = {
            "coarse_raster": list(m.shape), "coarse_fill_ms_runs": [round(t, 3) for t in times], "coarse_fill_ms_best": round(min(times), 3),
            "coarse_fill_stats": {kk: cst[kk] for kk in ("basins", "rounds", "edge_records", "host_syncs", "dissolved_pits")},
            "lb_le_w_on_every_block": lb_le_w, "flagged_tiles": nflag, "flagged_share": round(nflag / (nt * nt), 4),
            "flagged_of_census": round(nflag / max(1, int(census.sum())), 4), "flagged_subset_of_census": bool((flag & ~census).sum() == 0)}
        if args.part == "ab":
            skipped = scan_times(flag.to(torch.uint8).contiguous().view(-1), args.reps)
            fast = min(r["scan_ms"] for r in skipped)
            saving = out["pairs_no_skip"]["scan_ms_fastest"] - fast
            res.update({"pairs_with_skip": {"runs": skipped, "scan_ms_fastest": fast}, "saving_ms": round(saving, 3),
                        "saving_minus_coarse_fill_ms": round(saving - min(times), 3)})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
