// flowpath.hip -- sums along the D8 direction forest: the drainage cell of every cell, the steps to it (along x, along y,
// diagonal), the flow distance made of them, and HAND (height above the nearest drainage).  The contract is in
// include/rdgpu.h.
//
// upslope.hip brings the IDENTITY of a path's end back up the path; here a payload comes with it, the three step counts.
// Same three stages, and the race argument redone for the payload:
//   1. k_fp_tile   every 64 x 64 tile on its own: the directions staged in LDS, every cell pointer-jumped to the in-tile
//                  end of its path -- a stop cell, a cell whose path ends, or an EXIT (a cell whose target lies in another
//                  tile).  Pointer, end flag, the kind of end and the three counts (an in-tile path has at most 4095
//                  steps: 12 bits each) are ONE 64-bit LDS word, loaded and stored whole.  The jumps run in place, as
//                  k_up_tile's: whichever word of cell q a racing lane reads, old or new, it says "q's path reaches cell
//                  r after these steps", pointer and counts from the same store, so own counts + q's counts are the steps
//                  to r.  (A pointer from one store and counts from another would be wrong; that is why it is one word.)
//                  Only the tile's 252 border cells publish a node: RESOLVED with the drainage cell and the counts to it,
//                  or the node of the neighbouring tile's border cell its exit flows to, with the counts up to there.
//   2. k_fp_round  pointer doubling over the nodes.  A node is a link word and four payload words (20 bytes), too wide
//                  to be replaced whole, so the rounds go from one buffer to the other.  An open node adds the payload of
//                  the node it points to and takes that node's link.  A node resolved in round r exists in round r's
//                  target buffer only (FRESH); round r + 1 copies it across and marks it DONE in both, after which no
//                  round touches it beyond reading its link.  (That mark is the one store into the source buffer: FRESH
//                  and DONE both read as "resolved, payload valid here".)  ceil(log2(nodes)) + 1 rounds are enqueued; a
//                  round whose predecessor left nothing open returns at once on a device-side flag.  A node open in both
//                  buffers after the last round lies on, or flows into, a direction loop.
//   3. k_fp_final  every tile again: the in-tile ends recomputed in LDS, the answers of the tile's exits (node of the
//                  target + the exit's own step) gathered by one thread per border cell into a table that overlays the
//                  staged directions, every requested plane written once.
//   k_fp_hand      dem[c] - dem[to_cell[c]] in a pass of its own, from a to_cell plane kept in scratch.
// No host synchronisation in the device drivers; 1 memset + 2 + rounds launches (+ 1 for HAND), fixed by the raster's size.
// LDS per block: 4752 B staged directions (later the 4096 B exit table) + 33792 B words = 38544 B (38800 with the
// block-wide OR's scratch): four blocks per CU.  58 VGPRs in both tile kernels, 20 in the rounds.
// Scratch: two buffers of 20 B per node, 256 nodes per 4096 cells: 2.5 B per cell (+ 4 B per cell for HAND's to_cell).
#include "d8_forest.hpp"

#include <cmath>
#include <string>

namespace rdgpu {

constexpr uint32_t FP_NONE = 0xFFFFFFFFu;
// a tile word: bits 0..14 a cell's table index | bit 15: that cell is the END of the path | 16..27 steps along x |
// 28..39 along y | 40..51 diagonal | 52..53 (end words only) the kind of end.  A word that is no end has kind 0, so the
// kind arrives with the sum.  On a loop the counts overflow upwards, away from the pointer; such words never get FP_END.
constexpr unsigned long long FP_END = 0x8000ull, FP_CELL = 0x7FFFull, FP_PTR = 0xFFFFull;
constexpr int FP_SX = 16, FP_SY = 28, FP_SD = 40, FP_SK = 52;
enum { FP_K_NONE = 0, FP_K_SELF = 1, FP_K_EXIT = 2 };   // the end has no drainage cell | is the drainage cell | leaves the tile
// a node's link: the node it points to, or
constexpr uint32_t FP_DONE = 0xFFFFFFFFu, FP_FRESH = 0xFFFFFFFEu;   // resolved in both buffers | in this buffer only

struct FpTile {   // a tile's LDS state
  uint8_t sd[SDH * SDW] __attribute__((aligned(16)));   // staged directions (tile_front.hpp); k_fp_final: the exits' answers
  unsigned long long lw[LT * LPS];                      // per cell: its word
};
static_assert(sizeof(uint4) * TILE_SLOTS <= SDH * SDW, "the exit table overlays the staged directions");

// one step in direction d (1..8) as a tile word's counts: 1, 5 along x; 3, 7 along y; the even codes diagonal
__device__ __forceinline__ int fp_plane(uint32_t d) { return (d & 1u) ? ((d & 2u) ? 1 : 0) : 2; }
__device__ __forceinline__ unsigned long long fp_step(uint32_t d) { return 1ull << (FP_SX + 12 * fp_plane(d)); }

__device__ __forceinline__ unsigned long long fp_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void fp_store(unsigned long long *p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the word of a cell whose word is a, followed through the cell it points to, whose word is q
__device__ __forceinline__ unsigned long long fp_hop(unsigned long long a, unsigned long long q) {
  return (q & FP_PTR) | ((a & ~FP_PTR) + (q & ~FP_PTR));
}

// Stages the tile and pointer-jumps every cell to the in-tile end of its path: p[j] is the word of the thread's cell
// (lx, ly0 + 4 j); with FP_END it names the end, the steps to it and its kind; without, the path runs into a direction
// loop inside the tile (the flag, not "points to itself", marks an end: d8_forest.hpp).
__device__ __forceinline__ void fp_tile_ends(FpTile &T, const uint8_t *__restrict__ dirs, const uint8_t *__restrict__ chan,
                                             uint8_t nodata, int w, int h, int x0, int y0, unsigned long long (&p)[FOREST_RPT]) {
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, T.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t stopmask = 0;   // the mask is read once per cell, by the cell's own thread: no LDS copy
  if (chan) {
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
      if (gx < w && gy < h && chan[(size_t)gy * w + gx] != 0) stopmask |= 1u << j;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const unsigned long long self = (unsigned long long)(ly * LPS + lx);
    const uint32_t d = T.sd[(ly + 1) * SDW + SDO + lx];
    // where a path simply ends: without a mask that cell is the drainage cell, with one the path has met no stop cell
    const unsigned long long ends = self | FP_END | ((unsigned long long)(chan ? FP_K_NONE : FP_K_SELF) << FP_SK);
    unsigned long long v;
    if (d == nodata) {   // (cells outside the raster are staged as NoData)
      v = self | FP_END | ((unsigned long long)FP_K_NONE << FP_SK);
    } else if (stopmask >> j & 1u) {
      v = self | FP_END | ((unsigned long long)FP_K_SELF << FP_SK);
    } else if (d - 1u >= 8u) {
      v = ends;
    } else {
      const int tx = lx + d8dx((int)d), ty = ly + d8dy((int)d), gx = x0 + tx, gy = y0 + ty;
      if (gx < 0 || gy < 0 || gx >= w || gy >= h || T.sd[(ty + 1) * SDW + SDO + tx] == nodata) v = ends;
      else if (tx >= 0 && tx < LT && ty >= 0 && ty < LT) v = (unsigned long long)(ty * LPS + tx) | fp_step(d);
      else v = self | FP_END | ((unsigned long long)FP_K_EXIT << FP_SK);
    }
    p[j] = v;
    T.lw[ly * LPS + lx] = v;
  }
  __syncthreads();
  // two hops per trip: a trip at least triples the distance covered, twelve trips cover any loop-free path of 4096 cells;
  // what still moves then runs round a direction loop
#pragma unroll 1
  for (int it = 0; it < 12; it++) {
    bool moving = false;
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      unsigned long long a = p[j];
      if (!(a & FP_END)) {
        a = fp_hop(a, fp_load(&T.lw[a & FP_CELL]));
        if (!(a & FP_END)) a = fp_hop(a, fp_load(&T.lw[a & FP_CELL]));
        p[j] = a;
        fp_store(&T.lw[(ly0 + 4 * j) * LPS + lx], a);
        moving |= !(a & FP_END);
      }
    }
    if (!__syncthreads_or(moving)) break;
  }
  __syncthreads();
}

__global__ __launch_bounds__(NTHR, 4) void k_fp_tile(const uint8_t *__restrict__ dirs, const uint8_t *__restrict__ chan, uint8_t nodata,
                                                     int w, int h, uint32_t tilesX, uint32_t ntiles, uint32_t *__restrict__ link,
                                                     uint4 *__restrict__ val) {
  __shared__ FpTile T;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  unsigned long long p[FOREST_RPT];
  fp_tile_ends(T, dirs, chan, nodata, w, h, x0, y0, p);
  // what a path that ENTERS the tile at a border cell comes to, one border cell per thread
  const int slot = (int)threadIdx.x;
  uint32_t l = FP_FRESH;
  uint4 v = make_uint4(FP_NONE, 0u, 0u, 0u);   // (the four spare slots; a path into an in-tile loop; an end without a drainage cell)
  if (slot < BORDER_SLOTS) {
    int bx, by;
    border_cell(slot, bx, by);
    const unsigned long long a = T.lw[by * LPS + bx];
    const int kind = (int)(a >> FP_SK) & 3;
    if ((a & FP_END) && kind != FP_K_NONE) {
      const int e = (int)(a & FP_CELL), ey = e / LPS, ex = e - ey * LPS;
      v.y = (uint32_t)(a >> FP_SX) & 0xFFFu;
      v.z = (uint32_t)(a >> FP_SY) & 0xFFFu;
      v.w = (uint32_t)(a >> FP_SD) & 0xFFFu;
      if (kind == FP_K_SELF) {
        v.x = (uint32_t)(y0 + ey) * (uint32_t)w + (uint32_t)(x0 + ex);
      } else {   // the exit's own step belongs to this node: the node it flows to counts from the target cell on
        const uint32_t d = T.sd[(ey + 1) * SDW + SDO + ex];
        const int pl = fp_plane(d);
        v.y += pl == 0; v.z += pl == 1; v.w += pl == 2;
        v.x = 0u;
        l = tile_node(x0 + ex + d8dx((int)d), y0 + ey + d8dy((int)d), tilesX);
      }
    }
  }
  link[(size_t)t * TILE_SLOTS + slot] = l;
  val[(size_t)t * TILE_SLOTS + slot] = v;
}

// One doubling round from (ls, vs) into (ld, vd).  flags[r]: round r left a node open.
__global__ __launch_bounds__(NTHR) void k_fp_round(uint32_t *ls, const uint4 *vs, uint32_t *__restrict__ ld, uint4 *__restrict__ vd,
                                                   uint64_t nnodes, uint32_t *flags, int r) {
  if (r > 0 && flags[r - 1] == 0) return;
  const uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x;
  bool open = false;
  if (i < nnodes) {
    const uint32_t l = ls[i];
    if (l == FP_FRESH) {   // resolved by the round before (or by the tile pass): bring the other buffer up to date, once
      vd[i] = vs[i];
      ld[i] = FP_DONE;
      ls[i] = FP_DONE;     // (whoever reads this link meanwhile takes FRESH and DONE alike)
    } else if (l != FP_DONE) {
      const uint4 a = vs[i];
      const uint32_t l2 = ls[l];
      const uint4 b = vs[l];
      open = l2 < FP_FRESH;
      vd[i] = make_uint4(open ? 0u : b.x, a.y + b.y, a.z + b.z, a.w + b.w);
      ld[i] = open ? l2 : FP_FRESH;
    }
  }
  if (__any(open) && (threadIdx.x & 63) == 0) flags[r] = 1;
}

__global__ __launch_bounds__(NTHR, 4) void k_fp_final(const uint8_t *__restrict__ dirs, const uint8_t *__restrict__ chan, uint8_t nodata,
                                                      int w, int h, uint32_t tilesX, uint32_t ntiles, const uint32_t *__restrict__ link_a,
                                                      const uint4 *__restrict__ val_a, const uint32_t *__restrict__ link_b,
                                                      const uint4 *__restrict__ val_b, uint32_t *__restrict__ to_cell,
                                                      uint32_t *__restrict__ steps, double *__restrict__ dist, double cx, double cy,
                                                      double diag, double dist_nodata) {
  __shared__ FpTile T;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  unsigned long long p[FOREST_RPT];
  fp_tile_ends(T, dirs, chan, nodata, w, h, x0, y0, p);
  // the exits' answers, one border cell per thread: a node is resolved in at least one of the two buffers, or not at all
  const int slot = (int)threadIdx.x;
  uint4 ans = make_uint4(FP_NONE, 0u, 0u, 0u);
  if (slot < BORDER_SLOTS) {
    int bx, by;
    border_cell(slot, bx, by);
    const unsigned long long self = (unsigned long long)(by * LPS + bx);
    const unsigned long long a = T.lw[self];
    if ((a & FP_PTR) == (self | FP_END) && ((int)(a >> FP_SK) & 3) == FP_K_EXIT) {
      const uint32_t d = T.sd[(by + 1) * SDW + SDO + bx];
      const uint32_t nid = tile_node(x0 + bx + d8dx((int)d), y0 + by + d8dy((int)d), tilesX);
      const uint4 *src = val_a;
      uint32_t l = link_a[nid];
      if (l < FP_FRESH) { l = link_b[nid]; src = val_b; }
      if (l >= FP_FRESH) {
        ans = src[nid];
        const int pl = fp_plane(d);
        ans.y += pl == 0; ans.z += pl == 1; ans.w += pl == 2;
      }
    }
  }
  __syncthreads();   // the staged directions have been read for the last time
  uint4 *const exits = reinterpret_cast<uint4 *>(T.sd);
  exits[slot] = ans;
  __syncthreads();
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t plane = (size_t)w * h;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
    if (gx >= w || gy >= h) continue;
    const unsigned long long a = p[j];
    uint32_t tc = FP_NONE, nx = FP_NONE, ny = FP_NONE, nd = FP_NONE;
    const int kind = (int)(a >> FP_SK) & 3;
    if ((a & FP_END) && kind != FP_K_NONE) {   // (no end flag: into a direction loop inside the tile)
      const int e = (int)(a & FP_CELL), ey = e / LPS, ex = e - ey * LPS;
      const uint32_t ax = (uint32_t)(a >> FP_SX) & 0xFFFu, ay = (uint32_t)(a >> FP_SY) & 0xFFFu, ad = (uint32_t)(a >> FP_SD) & 0xFFFu;
      if (kind == FP_K_SELF) {
        tc = (uint32_t)(y0 + ey) * (uint32_t)w + (uint32_t)(x0 + ex);
        nx = ax; ny = ay; nd = ad;
      } else {
        const uint4 b = exits[border_slot(ex, ey)];
        if (b.x != FP_NONE) { tc = b.x; nx = ax + b.y; ny = ay + b.z; nd = ad + b.w; }
      }
    }
    const size_t g = (size_t)gy * w + gx;
    if (to_cell) to_cell[g] = tc;
    if (steps) { steps[g] = nx; steps[plane + g] = ny; steps[2 * plane + g] = nd; }
    if (dist) dist[g] = tc == FP_NONE ? dist_nodata : d8_path_length(nx, ny, nd, cx, cy, diag);
  }
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_fp_hand(const T *__restrict__ dem, T dem_nodata, const uint32_t *__restrict__ to_cell,
                                                  uint64_t n, double *__restrict__ hand, double out_nodata) {
  const uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i >= n) return;
  const uint32_t tc = to_cell[i];
  double v = out_nodata;
  if (tc != FP_NONE) {
    const T a = dem[i], b = dem[tc];
    if (a != dem_nodata && b != dem_nodata) v = __dsub_rn((double)a, (double)b);
  }
  hand[i] = v;
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
static void fp_check_dims(const void *dirs, int w, int h, const char *who) {
  if (!dirs) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_forest_dims(w, h, who);
}
static void fp_check_path_args(const void *dirs, int w, int h, double cx, double cy, const void *to_cell, const void *steps,
                               const void *dist, const char *who) {
  fp_check_dims(dirs, w, h, who);
  if (!to_cell && !steps && !dist) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  check_cell_lengths(cx, cy, who);
}

// arguments checked by the caller (declared in d8_forest.hpp: longest.hip runs it too)
void flow_path_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, const uint8_t *d_chan, double cx, double cy,
                      uint32_t *d_to_cell, uint32_t *d_steps, double *d_dist, double dist_nodata, hipStream_t s) {
  cx = std::fabs(cx);
  cy = std::fabs(cy);
  const double diag = std::sqrt(cx * cx + cy * cy);
  const ForestDims fd(w, h);
  const uint32_t tilesX = fd.tilesX, ntiles = fd.ntiles;
  const uint64_t nnodes = fd.nnodes;
  Workspace &ws = Workspace::get();
  uint32_t *link[2] = {ws.buf<uint32_t>("flowpath.link_a", nnodes), ws.buf<uint32_t>("flowpath.link_b", nnodes)};
  uint4 *val[2] = {ws.buf<uint4>("flowpath.val_a", nnodes), ws.buf<uint4>("flowpath.val_b", nnodes)};
  const int rounds = forest_rounds(nnodes);
  uint32_t *flags = ws.buf<uint32_t>("flowpath.flags", (size_t)rounds);
  RD_HIP(hipMemsetAsync(flags, 0, (size_t)rounds * sizeof(uint32_t), s));
  RD_LAUNCH("flowpath.tile", k_fp_tile, dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, d_chan, nodata, w, h, tilesX, ntiles, link[0],
            val[0]);
  const uint32_t ngrid = (uint32_t)((nnodes + NTHR - 1) / NTHR);
  for (int r = 0; r < rounds; r++)   // (round 0 writes every word of the second buffer)
    RD_LAUNCH("flowpath.round", k_fp_round, dim3(ngrid), dim3(NTHR), 0, s, link[r & 1], (const uint4 *)val[r & 1], link[(r + 1) & 1],
              val[(r + 1) & 1], nnodes, flags, r);
  RD_LAUNCH("flowpath.final", k_fp_final, dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, d_chan, nodata, w, h, tilesX, ntiles,
            (const uint32_t *)link[0], (const uint4 *)val[0], (const uint32_t *)link[1], (const uint4 *)val[1], d_to_cell, d_steps,
            d_dist, cx, cy, diag, dist_nodata);
}

static void hand_check(const void *dirs, const void *dem, const void *hand, int w, int h, const char *who) {
  fp_check_dims(dirs, w, h, who);
  if (!dem || !hand) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
}

// arguments checked by the caller (hand_check)
template <class T>
static void hand_device(const uint8_t *d_dirs, uint8_t nodata, const T *d_dem, T dem_nodata, int w, int h, const uint8_t *d_chan,
                        double *d_hand, double out_nodata, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  uint32_t *tc = Workspace::get().buf<uint32_t>("flowpath.to_cell", n);
  flow_path_device(d_dirs, nodata, w, h, d_chan, 1.0, 1.0, tc, nullptr, nullptr, 0.0, s);
  RD_LAUNCH("flowpath.hand", (k_fp_hand<T>), dim3((uint32_t)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, d_dem, dem_nodata,
            (const uint32_t *)tc, n, d_hand, out_nodata);
}

// host rasters: staged in the workspace, as d8_flow_accum's
static void flow_path_host(const uint8_t *dirs, uint8_t nodata, int w, int h, const uint8_t *chan, double cx, double cy,
                           uint32_t *to_cell, uint32_t *steps, double *dist, double dist_nodata, const char *who) {
  fp_check_path_args(dirs, w, h, cx, cy, to_cell, steps, dist, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  const uint8_t *dc = st.in("host.flowpath.chan", chan, n);
  uint32_t *dt = st.out("host.flowpath.to_cell", to_cell, n);
  uint32_t *dst = st.out("host.flowpath.steps", steps, 3 * n);
  double *ddi = st.out("host.flowpath.dist", dist, n);
  flow_path_device(dd, nodata, w, h, dc, cx, cy, dt, dst, ddi, dist_nodata, nullptr);
  st.finish();
}

template <class T>
static void hand_host(const uint8_t *dirs, uint8_t nodata, const T *dem, T dem_nodata, int w, int h, const uint8_t *chan, double *hand,
                      double out_nodata, const char *who) {
  hand_check(dirs, dem, hand, w, h, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  const uint8_t *dc = st.in("host.flowpath.chan", chan, n);
  const T *dz = st.in("host.flowpath.dem", dem, n);
  double *dh = st.out("host.flowpath.dist", hand, n);
  hand_device<T>(dd, nodata, dz, dem_nodata, w, h, dc, dh, out_nodata, nullptr);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

extern "C" int rdgpu_d8_flow_path(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan, double cell_x,
                                  double cell_y, uint32_t *to_cell, uint32_t *steps, double *dist, double dist_nodata) {
  return guarded([&] {
    flow_path_host(dirs, dir_nodata, width, height, chan, cell_x, cell_y, to_cell, steps, dist, dist_nodata, "rdgpu_d8_flow_path");
  });
}
extern "C" int rdgpu_d8_flow_path_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, const uint8_t *d_chan,
                                      double cell_x, double cell_y, uint32_t *d_to_cell, uint32_t *d_steps, double *d_dist,
                                      double dist_nodata, void *hip_stream) {
  return guarded([&] {
    fp_check_path_args(d_dirs, width, height, cell_x, cell_y, d_to_cell, d_steps, d_dist, "rdgpu_d8_flow_path_dev");
    flow_path_device(d_dirs, dir_nodata, width, height, d_chan, cell_x, cell_y, d_to_cell, d_steps, d_dist, dist_nodata,
                     (hipStream_t)hip_stream);
  });
}

#define RD_DEFINE_HAND(SUF, T)                                                                                                       \
  extern "C" int rdgpu_d8_hand_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const T *dem, T dem_nodata, int width, int height,    \
                                     const uint8_t *chan, double *hand, double out_nodata) {                                         \
    return guarded([&] {                                                                                                             \
      hand_host<T>(dirs, dir_nodata, dem, dem_nodata, width, height, chan, hand, out_nodata, "rdgpu_d8_hand_" #SUF);                 \
    });                                                                                                                              \
  }                                                                                                                                  \
  extern "C" int rdgpu_d8_hand_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const T *d_dem, T dem_nodata, int width,         \
                                         int height, const uint8_t *d_chan, double *d_hand, double out_nodata, void *hip_stream) {   \
    return guarded([&] {                                                                                                             \
      hand_check(d_dirs, d_dem, d_hand, width, height, "rdgpu_d8_hand_dev_" #SUF);                                                   \
      hand_device<T>(d_dirs, dir_nodata, d_dem, dem_nodata, width, height, d_chan, d_hand, out_nodata, (hipStream_t)hip_stream);     \
    });                                                                                                                              \
  }
RD_DEFINE_HAND(i8, int8_t)
RD_DEFINE_HAND(u8, uint8_t)
RD_DEFINE_HAND(i16, int16_t)
RD_DEFINE_HAND(u16, uint16_t)
RD_DEFINE_HAND(i32, int32_t)
RD_DEFINE_HAND(u32, uint32_t)
RD_DEFINE_HAND(f32, float)
RD_DEFINE_HAND(f64, double)
#undef RD_DEFINE_HAND
