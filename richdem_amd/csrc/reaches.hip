// reaches.hip -- the reaches of the D8 channel network: reach labels, one record per reach, the catchment of every
// reach.  The contract is in include/rdgpu.h.
//
// A reach is known by its BOTTOM (a channel cell without a channel target, or whose channel target is a junction), and
// walking down from any channel cell that has a reach stays inside that reach until its bottom.  So with the bottoms as
// the stop mask, the flow-path engine's to_cell is, for every cell of the raster, the bottom of the reach it drains
// through -- catchments and reach labels are one gather away, and loops need no case of their own (a loop without a
// junction holds no bottom: to_cell is "none" on it and on what drains into it).
//   k_rc_classify  every 64 x 64 tile: directions and mask staged as ONE byte per cell with a halo of 2 (the bottom test
//                  reads the children of the target), then per cell the bottom mask (a byte plane, the flow-path
//                  engine's chan) and the cell's class (channel, top, the kind of its step, its channel children).
//                  (A pass without LDS, every cell reading its 3 x 3 and its target's from global memory, took 42 ms at
//                  40000 x 40000 with channels at >= 100 cells of accumulation, where this one takes 5.3.)
//   k_rc_rank      the bottom plane in raster order, four cells per lane: a wavefront holds a block of 256 cells and
//                  writes the rank of each among the block's bottoms (a byte) and the block's count.
//   hipcub scan    over the block counts (one word per 256 cells): label = 1 + base[c >> 8] + rank_in_block[c], which is
//                  the rank of the bottom in raster order.  base[blocks] = N.
//   flow_path_device   to_cell over the bottoms, into the catchment plane (or the reach plane, or scratch).
//   k_rc_records   bottoms write bottom_cell and down and clear the counts (`cells` starts at 1 on a mouth, the one cell
//                  of a reach without a step); tops write top_cell, up and order.  Different fields: no ordering needed.
//   k_rc_count     every 64 x 64 tile: to_cell -> label in place, the reach plane, and the per-label counts
//                  (catchment cells, steps by kind), four 16-bit counts in one 64-bit word.  Equal labels are summed
//                  first along the wavefront's row (runs of equal labels: a segmented shuffle sum), then in an LDS hash
//                  table of the tile (one ds_add_u64 per run), and one global add per label, tile and non-zero count.
//                  One reach may own the whole raster (every run of a tile lands on one LDS word: at most 64 adds per
//                  row) and a tile may hold 4096 reaches (what finds no slot within RC_PROBES goes to global memory
//                  directly: such labels are many, so their addresses do not collide).  Integer adds: exact in any order.
//   k_rc_finish    per record: cells += steps, length from the final steps; *count = N.
// No host synchronisation in the device driver.  Scratch: 3 bytes per cell (bottom mask, class, rank in block), 8 bytes
// per 256 cells, the flow-path engine's 2.5 per cell, and 4 per cell for to_cell only when no label plane is requested.
#include "d8_forest.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

namespace rdgpu {

static_assert(sizeof(rdgpu_reach) == 48 && offsetof(rdgpu_reach, steps) == 24 && offsetof(rdgpu_reach, length) == 40,
              "ten 32-bit words and a double, no padding");

constexpr uint32_t RC_NONE = 0xFFFFFFFFu;
// a cell's class byte: bit 0 channel cell | bit 1 top | bits 2..3 its step (0: no channel target, 1 along x, 2 along y,
// 3 diagonal) | bits 4..7 its channel children (0..8)
constexpr uint32_t RC_CHAN = 1u, RC_TOP = 2u;
constexpr int RC_STEP = 2, RC_UP = 4;
constexpr int RC_BLOCK_LOG = 8;   // the rank blocks: 256 cells in raster order, one wavefront of k_rc_rank
constexpr int RC_CPT = 4;         // cells per thread of the two streaming kernels, their bytes moved as one word
static_assert((1 << RC_BLOCK_LOG) == 64 * RC_CPT, "a bottom's rank in its block is a byte, a block is one wavefront");
// the tile's hash table of k_rc_count
constexpr int RC_HASH_LOG = 10, RC_HASH = 1 << RC_HASH_LOG, RC_PROBES = 8;
// a count word: catchment cells | steps along x << 16 | along y << 32 | diagonal << 48 (a tile has 4096 cells)
constexpr int RC_SX = 16;

__device__ __forceinline__ int rc_opposite(int m) { return ((m + 3) & 7) + 1; }

// k_rc_classify's window: the tile with a halo of 2 (the bottom test reads the children of the target), one byte per cell:
// the code 1..8 of a channel cell, 0 for a channel cell without one, RC_OFF for what is no channel cell or off the raster
constexpr int RC_HALO = 2, RC_WW = LT + 2 * RC_HALO;
constexpr uint32_t RC_OFF = 0x80u;

// the channel children of the window cell at index `at`
__device__ __forceinline__ int rc_children(const uint8_t *sc, int at) {
  int n = 0;
#pragma unroll
  for (int m = 1; m <= 8; m++) n += sc[at + d8dy(m) * RC_WW + d8dx(m)] == (uint32_t)rc_opposite(m) ? 1 : 0;
  return n;
}

__global__ __launch_bounds__(NTHR) void k_rc_classify(const uint8_t *__restrict__ dirs, const uint8_t *__restrict__ chan, uint8_t nodata,
                                                      int w, int h, uint32_t tilesX, uint32_t ntiles, uint8_t *__restrict__ bot,
                                                      uint8_t *__restrict__ info) {
  __shared__ uint8_t sc[RC_WW * RC_WW];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  for (int i = (int)threadIdx.x; i < RC_WW * RC_WW; i += NTHR) {
    const int ly = i / RC_WW, lx = i - ly * RC_WW;
    const int gx = x0 - RC_HALO + lx, gy = y0 - RC_HALO + ly;
    uint32_t v = RC_OFF;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const size_t c = (size_t)gy * w + gx;
      if (!chan || chan[c] != 0) {   // (the directions are read on channel cells only)
        const uint32_t d = dirs[c];
        if (d != nodata) v = d - 1u < 8u ? d : 0u;
      }
    }
    sc[i] = (uint8_t)v;
  }
  __syncthreads();
  const int lx = threadIdx.x & (LT - 1), ly0 = (int)(threadIdx.x >> 6);
  const int gx = x0 + lx;
  if (gx >= w) return;
#pragma unroll 2
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j, gy = y0 + ly;
    if (gy >= h) break;
    const int at = (ly + RC_HALO) * RC_WW + lx + RC_HALO;
    const uint32_t d = sc[at];
    uint32_t inf = 0;
    bool bottom = false;
    if (d != RC_OFF) {
      const int k = rc_children(sc, at);
      uint32_t step = 0;
      bottom = true;   // (a mouth, unless it has a channel target)
      if (d != 0) {
        const int to = at + d8dy((int)d) * RC_WW + d8dx((int)d);
        if (sc[to] != RC_OFF) {
          step = (d & 1u) ? ((d & 2u) ? 2u : 1u) : 3u;   // codes 1, 5 along x; 3, 7 along y; the even ones diagonal
          bottom = rc_children(sc, to) >= 2;
        }
      }
      inf = RC_CHAN | (k != 1 ? RC_TOP : 0u) | (step << RC_STEP) | ((uint32_t)k << RC_UP);
    }
    const size_t g = (size_t)gy * w + gx;
    bot[g] = bottom ? 1 : 0;
    info[g] = (uint8_t)inf;
  }
}

// RC_CPT consecutive cells per thread, their bytes moved as one word: a wavefront is one rank block.  wrank <- the rank of
// every cell among the bottoms of its block, in raster order; bcount <- the block's bottoms.
__global__ __launch_bounds__(NTHR) void k_rc_rank(const uint8_t *__restrict__ bot, uint64_t n, uint8_t *__restrict__ wrank,
                                                  uint32_t *__restrict__ bcount) {
  const uint64_t q = (uint64_t)blockIdx.x * NTHR + threadIdx.x, c0 = q * RC_CPT;
  const bool whole = c0 + RC_CPT <= n;
  uint32_t botw = 0;
  if (whole) {   // (the workspace's planes are aligned)
    botw = *reinterpret_cast<const uint32_t *>(bot + c0);
  } else {
    for (int k = 0; k < RC_CPT && c0 + k < n; k++) botw |= (uint32_t)bot[c0 + k] << (8 * k);
  }
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < RC_CPT; k++) {
    const unsigned long long b = __ballot((botw >> (8 * k) & 1u) != 0);
    before += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    total += (uint32_t)__popcll(b);
  }
  uint32_t rankw = 0;
#pragma unroll
  for (int k = 0; k < RC_CPT; k++) {
    rankw |= (before & 0xFFu) << (8 * k);   // (of a bottom: at most 255 before it)
    before += botw >> (8 * k) & 1u;
  }
  if (whole) {
    *reinterpret_cast<uint32_t *>(wrank + c0) = rankw;
  } else {
    for (int k = 0; k < RC_CPT && c0 + k < n; k++) wrank[c0 + k] = (uint8_t)(rankw >> (8 * k));
  }
  if (lane == 0 && ((q >> 6) << RC_BLOCK_LOG) < n) bcount[q >> 6] = total;
}

// the label of the bottom cell b
__device__ __forceinline__ uint32_t rc_label(const uint32_t *__restrict__ base, const uint8_t *__restrict__ wrank, uint32_t b) {
  return 1u + base[b >> RC_BLOCK_LOG] + wrank[b];
}

// the record fields that the cell i, of class inf, knows
__device__ __forceinline__ void rc_record_cell(uint32_t i, uint32_t inf, const uint8_t *__restrict__ dirs, int w,
                                               const uint8_t *__restrict__ order, const uint8_t *__restrict__ bot,
                                               const uint8_t *__restrict__ wrank, const uint32_t *__restrict__ base,
                                               const uint32_t *__restrict__ tc, rdgpu_reach *table, uint32_t cap) {
  if (bot[i]) {
    const uint32_t l0 = rc_label(base, wrank, i) - 1u;
    if (l0 < cap) {
      rdgpu_reach &r = table[l0];
      const bool step = (inf >> RC_STEP & 3u) != 0;
      uint32_t down = 0;
      if (step) {   // (its target is a channel cell inside the raster, a junction: the top of a reach)
        const int d = (int)dirs[i];
        const uint32_t below = tc[(size_t)((int64_t)i + (int64_t)d8dy(d) * w + d8dx(d))];
        if (below != RC_NONE) down = rc_label(base, wrank, below);
      }
      r.bottom_cell = i;
      r.down = down;
      r.cells = step ? 0u : 1u;
      r.catchment_cells = 0;
      r.steps[0] = r.steps[1] = r.steps[2] = 0;
      r.length = 0.0;
    }
  }
  if (inf & RC_TOP) {
    const uint32_t b = tc[i];
    if (b != RC_NONE) {
      const uint32_t l0 = rc_label(base, wrank, b) - 1u;
      if (l0 < cap) {
        rdgpu_reach &r = table[l0];
        r.top_cell = i;
        r.up = inf >> RC_UP;
        r.order = order ? order[i] : 0u;
      }
    }
  }
}

// RC_CPT cells per thread: a class word of 0 holds no channel cell
__global__ __launch_bounds__(NTHR) void k_rc_records(const uint8_t *__restrict__ dirs, int w, uint64_t n, const uint8_t *__restrict__ order,
                                                     const uint8_t *__restrict__ bot, const uint8_t *__restrict__ info,
                                                     const uint8_t *__restrict__ wrank, const uint32_t *__restrict__ base,
                                                     const uint32_t *__restrict__ tc, rdgpu_reach *table, uint32_t cap) {
  const uint64_t c0 = ((uint64_t)blockIdx.x * NTHR + threadIdx.x) * RC_CPT;
  if (c0 >= n) return;
  uint32_t infw = 0;
  if (c0 + RC_CPT <= n) {
    infw = *reinterpret_cast<const uint32_t *>(info + c0);
  } else {
    for (int k = 0; k < RC_CPT && c0 + k < n; k++) infw |= (uint32_t)info[c0 + k] << (8 * k);
  }
  if (infw == 0) return;
#pragma unroll
  for (int k = 0; k < RC_CPT; k++) {
    const uint32_t inf = infw >> (8 * k) & 0xFFu;
    if (inf & RC_CHAN) rc_record_cell((uint32_t)c0 + k, inf, dirs, w, order, bot, wrank, base, tc, table, cap);
  }
}

__device__ __forceinline__ void rc_global_add(rdgpu_reach *table, uint32_t cap, uint32_t label, unsigned long long v) {
  if (label - 1u >= cap) return;
  rdgpu_reach &r = table[label - 1u];
  const uint32_t c = (uint32_t)v & 0xFFFFu, sx = (uint32_t)(v >> RC_SX) & 0xFFFFu, sy = (uint32_t)(v >> 2 * RC_SX) & 0xFFFFu,
                 sd = (uint32_t)(v >> 3 * RC_SX);
  if (c) atomicAdd(&r.catchment_cells, c);
  if (sx) atomicAdd(&r.steps[0], sx);
  if (sy) atomicAdd(&r.steps[1], sy);
  if (sd) atomicAdd(&r.steps[2], sd);
}

// tc holds to_cell on entry; where it is one of the two planes it leaves as that plane
__global__ __launch_bounds__(NTHR) void k_rc_count(const uint8_t *__restrict__ info, const uint8_t *__restrict__ wrank,
                                                   const uint32_t *__restrict__ base, const uint32_t *tc, int w, int h, uint32_t tilesX,
                                                   uint32_t ntiles, uint32_t *reach, uint32_t *catchment, rdgpu_reach *table,
                                                   uint32_t cap) {
  __shared__ uint32_t keys[RC_HASH];
  __shared__ unsigned long long vals[RC_HASH];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  const bool counting = table != nullptr && cap != 0;   // (uniform)
  if (counting) {
    for (int k = (int)threadIdx.x; k < RC_HASH; k += NTHR) { keys[k] = 0; vals[k] = 0; }
    __syncthreads();
  }
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int gx = x0 + lx;
#pragma unroll 4
  for (int j = 0; j < FOREST_RPT; j++) {
    const int gy = y0 + ly0 + 4 * j;   // (uniform over the wavefront: a row of the tile)
    if (gy >= h) break;
    uint32_t label = 0;
    unsigned long long v = 0;
    if (gx < w) {
      const size_t g = (size_t)gy * w + gx;
      const uint32_t b = tc[g], inf = info[g];
      if (b != RC_NONE) {
        label = rc_label(base, wrank, b);
        const uint32_t step = inf >> RC_STEP & 3u;
        v = 1ull | (step ? 1ull << (RC_SX * step) : 0ull);
      }
      if (catchment) catchment[g] = label;
      if (reach) reach[g] = (inf & RC_CHAN) ? label : 0u;
    }
    if (!counting) continue;
    // the runs of equal labels along the row: summed into their first lane
    const uint32_t left = __shfl_up(label, 1);
    const bool head = lx == 0 || left != label;
    const unsigned long long heads = __ballot(head);
    const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lx) - 1ull));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long ov = __shfl_down(v, d);
      const uint32_t orun = __shfl_down(run, d);
      if (lx + d < 64 && orun == run) v += ov;
    }
    if (head && label != 0) {
      uint32_t s = (label * 0x9E3779B1u) >> (32 - RC_HASH_LOG);
      bool placed = false;
      for (int k = 0; k < RC_PROBES && !placed; k++) {
        const uint32_t old = atomicCAS(&keys[s], 0u, label);
        if (old == 0u || old == label) {
          atomicAdd(&vals[s], v);
          placed = true;
        }
        s = (s + 1u) & (uint32_t)(RC_HASH - 1);
      }
      if (!placed) rc_global_add(table, cap, label, v);
    }
  }
  if (!counting) return;
  __syncthreads();
  for (int k = (int)threadIdx.x; k < RC_HASH; k += NTHR)
    if (keys[k] != 0) rc_global_add(table, cap, keys[k], vals[k]);
}

// base[nblocks] is N
__global__ __launch_bounds__(NTHR) void k_rc_finish(const uint32_t *__restrict__ base, uint32_t nblocks, rdgpu_reach *table, uint32_t cap,
                                                    double cx, double cy, double diag, uint32_t *count) {
  const uint32_t N = base[nblocks];
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i == 0) *count = N;
  if (i >= N || i >= cap) return;
  rdgpu_reach &r = table[i];
  r.cells += r.steps[0] + r.steps[1] + r.steps[2];
  r.length = d8_path_length(r.steps[0], r.steps[1], r.steps[2], cx, cy, diag);
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
static void rc_check_args(const void *dirs, int w, int h, double cx, double cy, const void *table, uint32_t capacity, const void *count,
                          const char *who) {
  if (!dirs || !count) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  if (!table && capacity) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null table with a non-zero capacity");
  check_forest_dims(w, h, who);
  check_cell_lengths(cx, cy, who);
}

// arguments checked by the caller
static void stream_reaches_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, const uint8_t *d_chan, const uint8_t *d_order,
                                  double cx, double cy, uint32_t *d_reach, uint32_t *d_catchment, rdgpu_reach *d_table,
                                  uint32_t capacity, uint32_t *d_count, hipStream_t s) {
  cx = std::fabs(cx);
  cy = std::fabs(cy);
  const double diag = std::sqrt(cx * cx + cy * cy);
  const uint64_t n = (uint64_t)w * h;
  const uint32_t nblocks = (uint32_t)((n + (1u << RC_BLOCK_LOG) - 1) >> RC_BLOCK_LOG);   // the rank blocks
  const uint32_t cap = d_table ? (uint32_t)std::min<uint64_t>(capacity, n) : 0u;   // (there are no more reaches than cells)
  Workspace &ws = Workspace::get();
  uint8_t *bot = ws.buf<uint8_t>("reaches.bottom", n), *info = ws.buf<uint8_t>("reaches.info", n);
  uint8_t *wrank = ws.buf<uint8_t>("reaches.rank", n);
  uint32_t *bcount = ws.buf<uint32_t>("reaches.bcount", (size_t)nblocks + 1), *base = ws.buf<uint32_t>("reaches.base", (size_t)nblocks + 1);
  RD_HIP(hipMemsetAsync(bcount + nblocks, 0, sizeof(uint32_t), s));
  const ForestDims fd(w, h);
  const uint32_t sgrid = (uint32_t)((n + (uint64_t)NTHR * RC_CPT - 1) / ((uint64_t)NTHR * RC_CPT));   // the streaming kernels
  RD_LAUNCH("reaches.classify", k_rc_classify, dim3(xcd_grid(fd.ntiles)), dim3(NTHR), 0, s, d_dirs, d_chan, nodata, w, h, fd.tilesX,
            fd.ntiles, bot, info);
  RD_LAUNCH("reaches.rank", k_rc_rank, dim3(sgrid), dim3(NTHR), 0, s, (const uint8_t *)bot, n, wrank, bcount);
  size_t tb = 0;
  RD_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, bcount, base, (int)(nblocks + 1), s));
  void *tmp = ws.buf("reaches.scan_tmp", tb);
  {
    Profiler &pf = Profiler::get();
    if (pf.enabled) pf.begin("reaches.scan", s);
    RD_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, bcount, base, (int)(nblocks + 1), s));
    if (pf.enabled) pf.end(s);
  }
  if (d_reach || d_catchment || cap) {
    uint32_t *tc = d_catchment ? d_catchment : d_reach ? d_reach : ws.buf<uint32_t>("reaches.to_cell", n);
    flow_path_device(d_dirs, nodata, w, h, bot, 1.0, 1.0, tc, nullptr, nullptr, 0.0, s);
    if (cap)
      RD_LAUNCH("reaches.records", k_rc_records, dim3(sgrid), dim3(NTHR), 0, s, d_dirs, w, n, d_order, (const uint8_t *)bot,
                (const uint8_t *)info, (const uint8_t *)wrank, (const uint32_t *)base, (const uint32_t *)tc, d_table, cap);
    RD_LAUNCH("reaches.count", k_rc_count, dim3(xcd_grid(fd.ntiles)), dim3(NTHR), 0, s, (const uint8_t *)info, (const uint8_t *)wrank,
              (const uint32_t *)base, (const uint32_t *)tc, w, h, fd.tilesX, fd.ntiles, d_reach, d_catchment, d_table, cap);
  }
  RD_LAUNCH("reaches.finish", k_rc_finish, dim3(std::max(1u, (cap + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, (const uint32_t *)base, nblocks,
            d_table, cap, cx, cy, diag, d_count);
}

// host rasters: staged in the workspace, as d8_flow_accum's
static void stream_reaches_host(const uint8_t *dirs, uint8_t nodata, int w, int h, const uint8_t *chan, const uint8_t *order, double cx,
                                double cy, uint32_t *reach, uint32_t *catchment, rdgpu_reach *table, uint32_t capacity, uint32_t *count,
                                const char *who) {
  rc_check_args(dirs, w, h, cx, cy, table, capacity, count, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  const uint8_t *dc = st.in("host.reaches.chan", chan, n);
  const uint8_t *dor = st.in("host.reaches.order", order, n);
  uint32_t *dn = st.out("host.reaches.count", count, 1);
  uint32_t *dr = st.out("host.reaches.reach", reach, n);
  uint32_t *dca = st.out("host.reaches.catchment", catchment, n);
  const uint32_t cap = table ? (uint32_t)std::min<uint64_t>(capacity, n) : 0u;
  rdgpu_reach *dt = cap ? Workspace::get().buf<rdgpu_reach>("host.reaches.table", cap) : nullptr;   // (fetched: cut to the count)
  stream_reaches_device(dd, nodata, w, h, dc, dor, cx, cy, dr, dca, dt, cap, dn, nullptr);
  st.finish();
  st.fetch(table, dt, std::min(*count, cap));
}

}  // namespace rdgpu

using namespace rdgpu;

extern "C" int rdgpu_d8_stream_reaches(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan,
                                       const uint8_t *order, double cell_x, double cell_y, uint32_t *reach, uint32_t *catchment,
                                       rdgpu_reach *table, uint32_t capacity, uint32_t *count) {
  return guarded([&] {
    stream_reaches_host(dirs, dir_nodata, width, height, chan, order, cell_x, cell_y, reach, catchment, table, capacity, count,
                        "rdgpu_d8_stream_reaches");
  });
}
extern "C" int rdgpu_d8_stream_reaches_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, const uint8_t *d_chan,
                                           const uint8_t *d_order, double cell_x, double cell_y, uint32_t *d_reach,
                                           uint32_t *d_catchment, rdgpu_reach *d_table, uint32_t capacity, uint32_t *d_count,
                                           void *hip_stream) {
  return guarded([&] {
    rc_check_args(d_dirs, width, height, cell_x, cell_y, d_table, capacity, d_count, "rdgpu_d8_stream_reaches_dev");
    stream_reaches_device(d_dirs, dir_nodata, width, height, d_chan, d_order, cell_x, cell_y, d_reach, d_catchment, d_table, capacity,
                          d_count, (hipStream_t)hip_stream);
  });
}
