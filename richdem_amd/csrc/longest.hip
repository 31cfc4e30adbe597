// longest.hip -- the longest upstream flow path of every cell of a D8 direction forest: the HEAD (the cell upstream that is
// farthest away along the flow), the steps and the length from it, and the main path of every basin (TauDEM's plen,
// WhiteboxTools' MaxUpslopeFlowpathLength / LongestFlowpath).  The contract is in include/rdgpu.h.
//
// For u upstream of v the steps from u to v are steps(u) - steps(v), so the cell of U(v) farthest from v is the one with the
// greatest distance D to the OUTLET: an upslope maximum of a fixed per-cell value, closed downstream as extreme.hip closes
// its keys.  D is a double, so value and cell index no longer fit the one 64-bit word extreme.hip pushes; they are closed
// one after the other.
//   flow-path engine   the three step planes of every cell (flow_path_device without a mask) into scratch; D is evaluated
//                      from them where it is needed, with the engine's own d8_path_length: the same bits.
//   k_forest_links     the node links (d8_forest.hpp).  This buffer is only read afterwards: both closures start their
//                      doubling from it.
//   CLOSURE 1, the value.  key = bits(D) + 1, monotone as an unsigned integer because D is finite and >= 0; 0 is "no
//   contribution", which D == 0.0 at an outlet must not be.  Cells without a path have no key.
//   k_lp_tile<KEYS>    own keys closed in the tile (ds_max_rtn_u64 over doubled pointers), exits raise their node.
//   k_forest_round     ceil(log2(nodes)) + 1 gated rounds over the 64-bit keys, pointers doubled between two buffers.
//                      nkey[i] is then the greatest key that ENTERS the tile at border cell i.
//   CLOSURE 2, the index.  M(c), the closed key of cell c, never falls downstream.  A link c -> t is KEPT iff
//   M(t) == M(c) != 0 and CUT otherwise; a pointer doubled over kept links only has equal M all the way along it, so a
//   push over it carries a cell of U(target) that holds the target's maximum, and nothing else ever arrives.  A cell starts
//   with 0xFFFFFFFF - cell iff its own key equals its M (never 0: cell <= 0xFFFEFFFF); the pushes are 32-bit maxima, so
//   the lowest index wins.
//   k_lp_tile<HEADS>   M rebuilt in the tile (own keys + nkey of the tile's border slots, closed), kept links, indices
//                      closed in LDS (ds_max_rtn_u32); an exit raises nidx of its node iff nkey there equals its own M.
//   k_lp_cut           the kept node links: i -> n iff nkey[n] == nkey[i] != 0.
//   k_forest_round     the same gated rounds over the kept links and the 32-bit indices.
//   k_lp_tile<WRITE>   as HEADS, with nidx of a border slot joining its cell's start iff nkey there equals the cell's M;
//                      every cell decoded: the head's steps gathered, the cell's own subtracted, the planes written.
//   k_lp_basin         on_basin_path = from_cell[v] == from_cell[to_cell[v]] in a pass of its own: the outlet's head is
//                      written by another block.  It reads two planes (from_cell, and the engine's to_cell kept in
//                      scratch) and gathers one word.  The alternative, a third closure that brings head(outlet) back UP
//                      the forest, would have cost a pull-style node table and one more tile pass.
//
// Races and termination: d8_forest.hpp's argument, for both closures (kept links form a sub-forest; the words are 64-bit
// keys, then 32-bit indices).  M is final before closure 2 reads it (kernel order on the stream; a barrier in the tile), so
// which links are kept does not depend on timing.  Cells on or draining into a direction loop have no path, hence no key
// and no index; nothing with a key lies upstream of them, so they raise nothing and receive nothing, their links are cut
// (M == 0), and the rounds over them end on the flag.
//
// No host synchronisation in the device driver; the flow-path engine's launches + 3 memsets + 5 + 2 rounds launches (+ 1
// for on_basin_path), fixed by the raster's size.
// LDS per block: 4752 B staged directions + 8448 B pointers + 33792 B keys (closure 2's indices overlay them) = 46992 B:
// three blocks per CU.
// Scratch: 12 B per cell for the step planes, the flow-path engine's 2.5, and per node three pointer buffers, a key and an
// index (24 B; 256 nodes per 4096 cells: 1.5 B per cell); on_basin_path keeps to_cell (4 B per cell) and, where from_cell
// is not requested, from_cell (4 more).
#include "d8_forest.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>

namespace rdgpu {

typedef unsigned long long lpkey_t;

constexpr uint32_t LP_NONE = 0xFFFFFFFFu;   // no path (the flow-path engine's steps), no head, no kept link
enum { LP_KEYS = 0, LP_HEADS = 1, LP_WRITE = 2 };

struct LpTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(8)));
  uint16_t lp[LT * LPS];
  union {
    lpkey_t key[LT * LPS];    // closure 1, per cell: the greatest key known to reach it
    uint32_t idx[LT * LPS];   // closure 2, per cell: the best index known to reach it (after the keys have been read)
  } __attribute__((aligned(8)));
};

// the node links closure 2 keeps, from the un-doubled links and the closed node keys
__global__ __launch_bounds__(NTHR) void k_lp_cut(const uint32_t *__restrict__ nxt0, const lpkey_t *__restrict__ nkey,
                                                 uint32_t *__restrict__ dst, uint32_t nnodes) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;   // (nnodes: a multiple of NTHR)
  if (i >= nnodes) return;
  const uint32_t n = nxt0[i];
  uint32_t keep = LP_NONE;
  if (n < nnodes) {
    const lpkey_t k = nkey[i];
    if (k != 0 && nkey[n] == k) keep = n;
  }
  dst[i] = keep;
}

// ---- the two closures inside a tile ------------------------------------------------------------------------------------------
// LP_KEYS:  keys = the cells' own; closed in the tile; a cell whose link leaves the tile raises the key of its node.
// LP_HEADS: keys = own and the node keys of the tile's border slots, closed: M.  Indices over the kept links, closed; a
//           cell whose link leaves the tile raises the index of its node iff the node's key is its M.
// LP_WRITE: as LP_HEADS, the node indices of the border slots joining in; every cell decoded and written.
// flag_out: a node word was raised (LP_KEYS, LP_HEADS).
template <int MODE>
__global__ __launch_bounds__(NTHR, 3) void k_lp_tile(const uint8_t *__restrict__ dirs, uint8_t nodata, const uint32_t *__restrict__ sfp,
                                                     int w, int h, uint32_t tilesX, uint32_t ntiles, double cx, double cy, double diag,
                                                     lpkey_t *nkey, uint32_t *nidx, uint32_t *flag_out,
                                                     uint32_t *__restrict__ from_cell, uint32_t *__restrict__ steps,
                                                     double *__restrict__ length, double length_nodata) {
  __shared__ LpTile S;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  const size_t plane = (size_t)w * h;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, S.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // the steps to the outlet are read once per cell by the cell's own thread; no path: no key
  lpkey_t own[FOREST_RPT];
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
    own[j] = 0;
    if (gx < w && gy < h) {
      const size_t g = (size_t)gy * w + gx;
      const uint32_t nx = sfp[g];
      if (nx != LP_NONE)
        own[j] = (lpkey_t)__double_as_longlong(d8_path_length(nx, sfp[plane + g], sfp[2 * plane + g], cx, cy, diag)) + 1ull;
    }
  }
  __syncthreads();
  uint32_t p[FOREST_RPT];
  uint32_t exitmask = 0;
  bool keyed = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int kind = forest_link(S.sd, nodata, lx, ly, tx, ty);
    lpkey_t k = own[j];   // (0 on NoData cells: they have no path)
    if (MODE != LP_KEYS && kind >= 0) {
      const int slot = border_slot(lx, ly);
      if (slot >= 0) {
        const lpkey_t nk = nkey[(size_t)t * TILE_SLOTS + slot];
        k = nk > k ? nk : k;
      }
    }
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : self;   // an end cell points at itself
    exitmask |= (kind == 2 ? 1u : 0u) << j;
    S.lp[self] = (uint16_t)p[j];
    S.key[self] = k;
    keyed |= k != 0;
  }
  forest_close(S.lp, p, keyed, lx, ly0, [&](uint32_t self, uint32_t to) { return forest_push_max(S.key, self, to); });
  if (MODE == LP_KEYS) {
    forest_push_exits(S.sd, nodata, S.key, exitmask, lx, ly0, x0, y0, tilesX, nkey, flag_out);
    return;
  }
  // closure 2.  M of the cell and of its target, the kept link and the cell's start, all read before the indices
  // overwrite the keys
  lpkey_t m[FOREST_RPT];
  uint32_t start[FOREST_RPT];
  bool headed = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int kind = forest_link(S.sd, nodata, lx, ly, tx, ty);
    m[j] = S.key[self];
    p[j] = (kind == 1 && m[j] != 0 && S.key[ty * LPS + tx] == m[j]) ? (uint32_t)(ty * LPS + tx) : self;
    uint32_t k = 0;
    if (m[j] != 0) {   // (the cell has a path, so it lies in the raster)
      if (own[j] == m[j]) k = LP_NONE - ((uint32_t)(y0 + ly) * (uint32_t)w + (uint32_t)(x0 + lx));
      if (MODE == LP_WRITE) {
        const int slot = border_slot(lx, ly);
        if (slot >= 0 && nkey[(size_t)t * TILE_SLOTS + slot] == m[j]) {
          const uint32_t nk = nidx[(size_t)t * TILE_SLOTS + slot];
          k = nk > k ? nk : k;
        }
      }
    }
    start[j] = k;
    headed |= k != 0;
  }
  __syncthreads();   // the keys have been read for the last time
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const uint32_t self = (uint32_t)((ly0 + 4 * j) * LPS + lx);
    S.lp[self] = (uint16_t)p[j];
    S.idx[self] = start[j];
  }
  forest_close(S.lp, p, headed, lx, ly0, [&](uint32_t self, uint32_t to) { return forest_push_max(S.idx, self, to); });
  if (MODE == LP_HEADS) {
    bool pushed = false;
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      if (!(exitmask >> j & 1u)) continue;
      const int ly = ly0 + 4 * j;
      const uint32_t k = S.idx[ly * LPS + lx];
      if (k == 0) continue;
      int tx, ty;
      forest_link(S.sd, nodata, lx, ly, tx, ty);
      const uint32_t n = tile_node(x0 + tx, y0 + ty, tilesX);
      if (nkey[n] != m[j]) continue;   // the link is cut: something farther away enters that cell from elsewhere
      atomicMax(&nidx[n], k);
      pushed = true;
    }
    if (__any(pushed) && (threadIdx.x & 63) == 0) *flag_out = 1;
  } else {
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      const int ly = ly0 + 4 * j, gx = x0 + lx, gy = y0 + ly;
      if (gx >= w || gy >= h) continue;
      const uint32_t k = S.idx[ly * LPS + lx];
      const size_t g = (size_t)gy * w + gx;
      uint32_t fc = LP_NONE, nx = LP_NONE, ny = LP_NONE, nd = LP_NONE;
      if (k != 0) {   // (every cell with a path has a head: itself, if nothing else)
        fc = LP_NONE - k;
        if (steps || length) {
          nx = sfp[fc] - sfp[g];
          ny = sfp[plane + fc] - sfp[plane + g];
          nd = sfp[2 * plane + fc] - sfp[2 * plane + g];
        }
      }
      if (from_cell) from_cell[g] = fc;
      if (steps) { steps[g] = nx; steps[plane + g] = ny; steps[2 * plane + g] = nd; }
      if (length) length[g] = fc == LP_NONE ? length_nodata : d8_path_length(nx, ny, nd, cx, cy, diag);
    }
  }
}

__global__ __launch_bounds__(NTHR) void k_lp_basin(const uint32_t *__restrict__ from_cell, const uint32_t *__restrict__ to_cell, uint64_t n,
                                                   uint8_t *__restrict__ on_basin_path) {
  const uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i >= n) return;
  const uint32_t tc = to_cell[i];
  on_basin_path[i] = (tc != LP_NONE && from_cell[i] == from_cell[tc]) ? 1 : 0;
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
static void lp_check_args(const void *dirs, int w, int h, double cx, double cy, const void *from_cell, const void *steps,
                          const void *length, const void *on_basin_path, const char *who) {
  if (!dirs) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  if (!from_cell && !steps && !length && !on_basin_path) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  check_forest_dims(w, h, who);
  check_cell_lengths(cx, cy, who);
}

// arguments checked by the caller
static void longest_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, double cx, double cy, uint32_t *d_from_cell,
                           uint32_t *d_steps, double *d_length, double length_nodata, uint8_t *d_on_basin_path, hipStream_t s) {
  cx = std::fabs(cx);
  cy = std::fabs(cy);
  const double diag = std::sqrt(cx * cx + cy * cy);   // (the flow-path engine's expression)
  const uint64_t n = (uint64_t)w * h;
  const ForestDims fd(w, h);
  const uint32_t tilesX = fd.tilesX, ntiles = fd.ntiles, nnodes = (uint32_t)fd.nnodes;
  const int rounds = forest_rounds(nnodes);
  Workspace &ws = Workspace::get();
  uint32_t *sfp = ws.buf<uint32_t>("longest.steps", 3 * n);
  uint32_t *tc = d_on_basin_path ? ws.buf<uint32_t>("longest.to_cell", n) : nullptr;
  uint32_t *fc = d_from_cell ? d_from_cell : d_on_basin_path ? ws.buf<uint32_t>("longest.from_cell", n) : nullptr;
  uint32_t *nxt0 = ws.buf<uint32_t>("longest.nxt", nnodes);
  uint32_t *pp[2] = {ws.buf<uint32_t>("longest.nxt_a", nnodes), ws.buf<uint32_t>("longest.nxt_b", nnodes)};
  lpkey_t *nkey = ws.buf<lpkey_t>("longest.nkey", nnodes);
  uint32_t *nidx = ws.buf<uint32_t>("longest.nidx", nnodes);
  // flags, per closure c = 0, 1 at c * (rounds + 1): [0] the tile pass raised a node word | [1 + r] round r raised one
  uint32_t *flags = ws.buf<uint32_t>("longest.flags", 2 * ((size_t)rounds + 1));
  flow_path_device(d_dirs, nodata, w, h, nullptr, cx, cy, tc, sfp, nullptr, 0.0, s);   // (lp_check_args covers its checks)
  RD_HIP(hipMemsetAsync(flags, 0, 2 * ((size_t)rounds + 1) * sizeof(uint32_t), s));
  RD_HIP(hipMemsetAsync(nkey, 0, (size_t)nnodes * sizeof(lpkey_t), s));
  RD_HIP(hipMemsetAsync(nidx, 0, (size_t)nnodes * sizeof(uint32_t), s));
  const uint32_t rgrid = std::min<uint32_t>(ntiles, 2048u);
  uint32_t *const f1 = flags, *const f2 = flags + rounds + 1;
  RD_LAUNCH("longest.links", k_forest_links, dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, w, h, tilesX, ntiles, nxt0);
  RD_LAUNCH("longest.keys", (k_lp_tile<LP_KEYS>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, (const uint32_t *)sfp, w, h,
            tilesX, ntiles, cx, cy, diag, nkey, nidx, f1, (uint32_t *)nullptr, (uint32_t *)nullptr, (double *)nullptr, 0.0);
  for (int r = 0; r < rounds; r++)   // (round 0 reads the kept buffer; every round writes every word of its target)
    RD_LAUNCH("longest.key_round", (k_forest_round<lpkey_t>), dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)(r ? pp[(r + 1) & 1] : nxt0),
              pp[r & 1], nkey, nnodes, (const uint32_t *)(f1 + r), f1 + r + 1);
  RD_LAUNCH("longest.heads", (k_lp_tile<LP_HEADS>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, (const uint32_t *)sfp, w, h,
            tilesX, ntiles, cx, cy, diag, nkey, nidx, f2, (uint32_t *)nullptr, (uint32_t *)nullptr, (double *)nullptr, 0.0);
  RD_LAUNCH("longest.cut", k_lp_cut, dim3(nnodes / NTHR), dim3(NTHR), 0, s, (const uint32_t *)nxt0, (const lpkey_t *)nkey, pp[1], nnodes);
  for (int r = 0; r < rounds; r++)
    RD_LAUNCH("longest.head_round", (k_forest_round<uint32_t>), dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)pp[(r + 1) & 1], pp[r & 1],
              nidx, nnodes, (const uint32_t *)(f2 + r), f2 + r + 1);
  RD_LAUNCH("longest.write", (k_lp_tile<LP_WRITE>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, (const uint32_t *)sfp, w, h,
            tilesX, ntiles, cx, cy, diag, nkey, nidx, (uint32_t *)nullptr, fc, d_steps, d_length, length_nodata);
  if (d_on_basin_path)
    RD_LAUNCH("longest.basin", k_lp_basin, dim3((uint32_t)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, (const uint32_t *)fc,
              (const uint32_t *)tc, n, d_on_basin_path);
}

// host rasters: staged in the workspace, as d8_flow_path's
static void longest_host(const uint8_t *dirs, uint8_t nodata, int w, int h, double cx, double cy, uint32_t *from_cell, uint32_t *steps,
                         double *length, double length_nodata, uint8_t *on_basin_path, const char *who) {
  lp_check_args(dirs, w, h, cx, cy, from_cell, steps, length, on_basin_path, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  uint32_t *df = st.out("host.longest.from_cell", from_cell, n);
  uint32_t *dst = st.out("host.longest.steps", steps, 3 * n);
  double *dl = st.out("host.longest.length", length, n);
  uint8_t *db = st.out("host.longest.on_basin_path", on_basin_path, n);
  longest_device(dd, nodata, w, h, cx, cy, df, dst, dl, length_nodata, db, nullptr);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

extern "C" int rdgpu_d8_longest_flow_path(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, double cell_x, double cell_y,
                                          uint32_t *from_cell, uint32_t *steps, double *length, double length_nodata,
                                          uint8_t *on_basin_path) {
  return guarded([&] {
    longest_host(dirs, dir_nodata, width, height, cell_x, cell_y, from_cell, steps, length, length_nodata, on_basin_path,
                 "rdgpu_d8_longest_flow_path");
  });
}
extern "C" int rdgpu_d8_longest_flow_path_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, double cell_x,
                                              double cell_y, uint32_t *d_from_cell, uint32_t *d_steps, double *d_length,
                                              double length_nodata, uint8_t *d_on_basin_path, void *hip_stream) {
  return guarded([&] {
    lp_check_args(d_dirs, width, height, cell_x, cell_y, d_from_cell, d_steps, d_length, d_on_basin_path,
                  "rdgpu_d8_longest_flow_path_dev");
    longest_device(d_dirs, dir_nodata, width, height, cell_x, cell_y, d_from_cell, d_steps, d_length, length_nodata, d_on_basin_path,
                   (hipStream_t)hip_stream);
  });
}
