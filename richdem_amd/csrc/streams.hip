// streams.hip -- the channel network on the D8 direction forest: channel mask from an accumulation threshold, Strahler
// stream order, and the classification of channel cells (heads, junctions, mouths).  The contract is in include/rdgpu.h.
//
// The order is not additive, but "order >= k + 1" is a reachability question: with S_k the channel cells of order >= k,
//   S_1     = every channel cell
//   J_k     = the cells with at least two channel children in S_k
//   S_{k+1} = J_k and everything downstream of it (inside the channel mask)
// and order(v) = max { k : v in S_k }.  A level k is therefore "mark the junctions of S_k, close the marks downstream",
// and the closure is what the link forest of accum.hip / upslope.hip is built for, run with marks instead of sums:
//   k_so_init    order <- 1 on channel cells, 0 elsewhere: from here on "order != 0" IS the channel mask.
//   k_so_links   the node links of the channel paths, as d8_forest.hpp's k_forest_links with the channel mask.  What has
//                no end after 4096 steps runs into a loop inside the tile, and the cell it has reached lies ON the loop --
//                the jump is a rotation of the loop, so every loop cell is reached by one: those get 255.
//   loops across tiles: the same argument on the nodes (k_so_round without marks, ping-pong buffers so that every node
//                covers the same distance; k_so_loopmark marks what the unfinished nodes have reached), then
//                k_so_close<SO_LOOPS> writes 255 along the in-tile paths below the marked entries.
//   per level k = 1 .. floor(log2(cells)) (order k needs 2^(k-1) heads, so no more levels can matter):
//     k_so_close<SO_SEED>   J_k from the staged 66 x 66 window of directions and orders, closed downstream INSIDE the tile
//                           by mark pushing over doubled pointers in LDS; a marked exit marks the node it flows to.
//     k_so_round            the node marks pushed over doubled node pointers: round r pushes by 2^r, and a round that
//                           marked nothing new proves the marks closed -- every later round returns at once.
//     k_so_close<SO_WRITE>  J_k again plus the marked entries, closed in the tile, order <- k + 1 on what is marked.
//   A level returns at once (a device-side flag, no host synchronisation) when the level before it found no junction, and
//   a tile is skipped at level k when it holds no cell of order k (tmax: S_{k+1} lies inside S_k).
// Loop cells are children of loop cells only, so 255 never enters a finite order; their tributaries are ordinary trees.
#include "d8_forest.hpp"

#include <algorithm>
#include <cmath>
#include <string>

namespace rdgpu {

constexpr uint32_t SO_ORDER_LOOP = 255u;
enum { SO_LOOPS = 0, SO_SEED = 1, SO_WRITE = 2 };

struct SoTile {   // a tile's LDS state
  uint8_t sd[SDH * SDW] __attribute__((aligned(4)));   // staged directions (tile_front.hpp)
  uint8_t so[SDH * SDW] __attribute__((aligned(4)));   // staged orders, same layout (0 outside the raster)
  uint16_t lp[LT * LPS];                               // per cell: a cell further down its in-tile channel path
  uint8_t mk[LT * LPS];                                // per cell: marked
};

__device__ __forceinline__ int so_opposite(int m) { return ((m + 3) & 7) + 1; }

// the channel link of the channel cell (lx, ly): 0 none (its tree ends here), 1 to (tx, ty) inside the tile, 2 to (tx, ty)
// in another tile.  A target that is no channel cell, or lies off the raster (staged as order 0), ends the tree.
__device__ __forceinline__ int so_link(const SoTile &T, int lx, int ly, int &tx, int &ty) {
  const uint32_t d = T.sd[(ly + 1) * SDW + SDO + lx];
  tx = lx; ty = ly;
  if (d - 1u >= 8u) return 0;
  tx = lx + d8dx((int)d); ty = ly + d8dy((int)d);
  if (T.so[(ty + 1) * SDW + SDO + tx] == 0) return 0;
  return (tx >= 0 && tx < LT && ty >= 0 && ty < LT) ? 1 : 2;
}

// the number of channel children of (lx, ly) whose order is at least k (loop cells excluded)
__device__ __forceinline__ int so_children(const SoTile &T, int lx, int ly, uint32_t k) {
  int n = 0;
#pragma unroll
  for (int m = 1; m <= 8; m++) {
    const int at = (ly + 1 + d8dy(m)) * SDW + SDO + lx + d8dx(m);
    const uint32_t o = T.so[at];
    n += (o >= k && o != SO_ORDER_LOOP && T.sd[at] == (uint32_t)so_opposite(m)) ? 1 : 0;
  }
  return n;
}

// ---- element-wise ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_so_channels(const double *__restrict__ accum, double nodata, double threshold, uint64_t n,
                                                      uint8_t *__restrict__ chan) {
  const uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i >= n) return;
  const double a = accum[i];
  chan[i] = (a != nodata && a >= threshold) ? 1 : 0;
}

__global__ __launch_bounds__(NTHR) void k_so_init(const uint8_t *__restrict__ dirs, uint8_t nodata, const uint8_t *__restrict__ chan,
                                                  uint64_t n, uint8_t *__restrict__ order) {
  const uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i >= n) return;
  order[i] = (dirs[i] != nodata && (!chan || chan[i] != 0)) ? 1 : 0;
}

// ---- the link forest of the channel cells, and the loops inside a tile ------------------------------------------------------
__global__ __launch_bounds__(NTHR, 5) void k_so_links(const uint8_t *__restrict__ dirs, uint8_t nodata, uint8_t *order, int w, int h,
                                                      uint32_t tilesX, uint32_t ntiles, uint32_t *__restrict__ nxt0,
                                                      uint8_t *__restrict__ tmax) {
  __shared__ SoTile T;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, T.sd);
  stage_dirs_rows(order, w, h, x0, y0, (uint8_t)0, T.so);
  __syncthreads();
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t p[FOREST_RPT];
  bool chan_here = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty, kind = 0;
    if (T.so[(ly + 1) * SDW + SDO + lx] != 0) {
      chan_here = true;
      kind = so_link(T, lx, ly, tx, ty);
    }
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : (self | FOREST_END);
    T.lp[self] = (uint16_t)p[j];
    T.mk[self] = 0;
  }
  const bool any_chan = __syncthreads_or(chan_here);
  forest_jump_sync(T.lp, p, lx, ly0);
  bool loop_here = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++)
    if (!(p[j] & FOREST_END)) { T.mk[p[j]] = 1; loop_here = true; }
  if (__syncthreads_or(loop_here)) {
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      const int ly = ly0 + 4 * j;
      if (T.mk[ly * LPS + lx]) order[(size_t)(y0 + ly) * w + (x0 + lx)] = (uint8_t)SO_ORDER_LOOP;   // (a channel cell: inside the raster)
    }
  }
  // the node a path that ENTERS the tile at a border cell leaves it to, one border cell per thread
  const int slot = (int)threadIdx.x;
  uint32_t word = FOREST_NONE;
  if (any_chan && slot < BORDER_SLOTS) {
    int bx, by, tx, ty;
    border_cell(slot, bx, by);
    const uint32_t rp = T.lp[by * LPS + bx], root = rp & FOREST_CELL;
    if (T.so[(by + 1) * SDW + SDO + bx] != 0 && (rp & FOREST_END)) {
      const int ry = (int)root / LPS, rx = (int)root - ry * LPS;
      if (so_link(T, rx, ry, tx, ty) == 2) word = tile_node(x0 + tx, y0 + ty, tilesX);
    }
  }
  nxt0[(size_t)t * TILE_SLOTS + slot] = word;
  if (threadIdx.x == 0) tmax[t] = any_chan ? 1 : 0;
}

// One doubling round over the nodes, from src into dst (never in place: every node covers the same distance), a tile's
// 256 nodes per block trip.  With marks: a marked node marks the node it points to; flag_out: something new was marked.
// Without: flag_out: a node is still unfinished.  Tiles without a cell of order k take no part (their words in dst stay
// stale: they are read only through nodes that cannot be marked, and an index is checked before it is followed).
__global__ __launch_bounds__(NTHR) void k_so_round(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint8_t *nmark,
                                                   uint32_t ntiles, const uint8_t *__restrict__ tmax, uint32_t k,
                                                   const uint32_t *__restrict__ gate, uint32_t *flag_out) {
  if (*gate == 0) return;
  const uint32_t nnodes = ntiles * (uint32_t)TILE_SLOTS;
  bool flag = false;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    if (tmax[t] < k) continue;
    const uint32_t i = t * (uint32_t)TILE_SLOTS + threadIdx.x;
    const uint32_t n = src[i];
    uint32_t n2 = FOREST_NONE;
    if (n < nnodes) {
      n2 = src[n];
      if (nmark) {
        if (nmark[i] && !nmark[n]) { nmark[n] = 1; flag = true; }
      } else {
        flag |= n2 < nnodes;
      }
    }
    dst[i] = n2;
  }
  if (__any(flag) && (threadIdx.x & 63) == 0) *flag_out = 1;
}

// what an unfinished node has reached after the last round lies on a loop, and every node of a loop is reached by one
__global__ __launch_bounds__(NTHR) void k_so_loopmark(const uint32_t *__restrict__ last, uint32_t nnodes, uint8_t *nmark,
                                                      const uint8_t *__restrict__ tmax, const uint32_t *__restrict__ gate) {
  if (*gate == 0) return;
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= nnodes || tmax[i / (uint32_t)TILE_SLOTS] == 0) return;   // (a tile without channel cells took no part in the rounds)
  const uint32_t n = last[i];
  if (n < nnodes) nmark[n] = 1;
}

// SO_LOOPS: marks = the entries on a loop across tiles; 255 on what lies below them in the tile.
// SO_SEED:  marks = J_k; closed in the tile; a marked exit marks its node.  lvl_out: there is a junction at this level.
// SO_WRITE: marks = J_k and the marked entries; closed in the tile; order <- k + 1.
template <int MODE>
__global__ __launch_bounds__(NTHR, 5) void k_so_close(const uint8_t *__restrict__ dirs, uint8_t nodata, uint8_t *order, int w, int h,
                                                      uint32_t tilesX, uint32_t ntiles, uint32_t k, uint8_t *nmark, uint8_t *tmax,
                                                      const uint32_t *__restrict__ gate, uint32_t *lvl_out, uint32_t *exit_out) {
  __shared__ SoTile T;
  if (gate && *gate == 0) return;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  if (tmax[t] < k) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, T.sd);
  stage_dirs_rows(order, w, h, x0, y0, (uint8_t)0, T.so);
  __syncthreads();
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t p[FOREST_RPT];
  uint32_t exitmask = 0;
  bool seeded = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    const uint32_t o = T.so[(ly + 1) * SDW + SDO + lx];
    int tx, ty, kind = 0;
    bool seed = false;
    if (o != 0) {
      kind = so_link(T, lx, ly, tx, ty);
      if (MODE != SO_LOOPS) seed = o != SO_ORDER_LOOP && so_children(T, lx, ly, k) >= 2;
      if (MODE != SO_SEED) {
        const int slot = border_slot(lx, ly);
        if (slot >= 0 && nmark[(size_t)t * TILE_SLOTS + slot]) seed = true;
      }
    }
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : self;
    exitmask |= (kind == 2 ? 1u : 0u) << j;
    T.lp[self] = (uint16_t)p[j];
    T.mk[self] = seed ? 1 : 0;
    seeded |= seed;
  }
  // the marks pushed down the in-tile paths (a marked cell pushes to itself at an end: nothing new)
  const auto mark = [&](uint32_t self, uint32_t to) {
    if (!T.mk[self] || T.mk[to]) return false;
    T.mk[to] = 1;
    return true;
  };
  if (!forest_close(T.lp, p, seeded, lx, ly0, mark)) return;
  if (MODE == SO_SEED && threadIdx.x == 0) *lvl_out = 1;
  bool done = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    if (!T.mk[ly * LPS + lx]) continue;
    if (MODE == SO_SEED) {
      if (exitmask >> j & 1u) {
        int tx, ty;
        so_link(T, lx, ly, tx, ty);
        nmark[tile_node(x0 + tx, y0 + ty, tilesX)] = 1;
        done = true;
      }
    } else {
      const uint32_t o = T.so[(ly + 1) * SDW + SDO + lx];
      if (MODE == SO_LOOPS) {
        order[(size_t)(y0 + ly) * w + (x0 + lx)] = (uint8_t)SO_ORDER_LOOP;
      } else if (o != SO_ORDER_LOOP) {
        order[(size_t)(y0 + ly) * w + (x0 + lx)] = (uint8_t)(k + 1);
        done = true;
      }
    }
  }
  if (MODE != SO_LOOPS && __syncthreads_or(done) && threadIdx.x == 0) {
    if (MODE == SO_SEED) *exit_out = 1;
    else tmax[t] = (uint8_t)(k + 1);
  }
}

// ---- the kinds of channel cells: one 3 x 3 pass ---------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_so_kinds(const uint8_t *__restrict__ dirs, uint8_t nodata, int w, int h,
                                                   const uint8_t *__restrict__ chan, const uint8_t *__restrict__ order,
                                                   uint8_t *__restrict__ kind) {
  const uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i >= (uint64_t)w * h) return;
  const int x = (int)(i % (uint32_t)w), y = (int)(i / (uint32_t)w);
  auto is_chan = [&](int cx, int cy) {
    if (cx < 0 || cy < 0 || cx >= w || cy >= h) return false;
    const size_t c = (size_t)cy * w + cx;
    return dirs[c] != nodata && (!chan || chan[c] != 0);
  };
  uint8_t out = 0;
  if (is_chan(x, y)) {
    int children = 0;
    uint32_t child_order = 0;
    for (int m = 1; m <= 8; m++) {
      const int cx = x + d8dx(m), cy = y + d8dy(m);
      if (is_chan(cx, cy) && dirs[(size_t)cy * w + cx] == (uint32_t)so_opposite(m)) {
        children++;
        child_order = order[(size_t)cy * w + cx];
      }
    }
    const uint32_t d = dirs[i];
    const bool target_chan = d - 1u < 8u && is_chan(x + d8dx((int)d), y + d8dy((int)d));
    out = children == 0 ? RDGPU_STREAM_HEAD
          : children >= 2 ? RDGPU_STREAM_JUNCTION
          : child_order != order[i] ? RDGPU_STREAM_ORDER_STEP
          : !target_chan ? RDGPU_STREAM_MOUTH
                         : RDGPU_STREAM_PLAIN;
  }
  kind[i] = out;
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
static thread_local int so_last_levels = 0, so_last_rounds = 0, so_last_launches = 0;

// the argument checks of an entry's two doors (host pointers, device pointers): thrown before anything is staged
static void so_check_args(bool pointers, int w, int h, const char *who) {
  if (!pointers) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_forest_dims(w, h, who);
}
static void so_check_channels_args(const void *accum, const void *chan, int w, int h, double threshold, const char *who) {
  so_check_args(accum && chan, w, h, who);
  if (!std::isfinite(threshold)) throw Error(RDGPU_ERR_ARG, std::string(who) + ": the threshold must be finite");
}

// arguments checked by the caller (so_check_args), here and in the two drivers below
static void stream_order_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, const uint8_t *d_chan, uint8_t *d_order,
                                hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  const ForestDims fd(w, h);
  const uint32_t tilesX = fd.tilesX, ntiles = fd.ntiles, nnodes = (uint32_t)fd.nnodes;
  const int rounds = forest_rounds(nnodes);
  int levels = 0;   // order k needs 2^(k-1) heads: levels 1 .. floor(log2(cells))
  while ((2ull << levels) <= n) levels++;
  if (levels > 30) levels = 30;
  Workspace &ws = Workspace::get();
  uint32_t *nxt0 = ws.buf<uint32_t>("streams.nxt0", nnodes);
  uint32_t *pp[2] = {ws.buf<uint32_t>("streams.nxt_a", nnodes), ws.buf<uint32_t>("streams.nxt_b", nnodes)};
  uint8_t *nmark = ws.buf<uint8_t>("streams.nmark", nnodes);
  uint8_t *tmax = ws.buf<uint8_t>("streams.tmax", ntiles);
  // flags: [0] always 1 | per level l = 0 (the loops) .. levels: [1 + l * stride] junctions at this level,
  // [+1] a marked exit, [+2 + r] round r marked something new (left something unfinished)
  const size_t stride = (size_t)rounds + 2, nflags = 1 + (size_t)(levels + 1) * stride;
  uint32_t *flags = ws.buf<uint32_t>("streams.flags", nflags);
  RD_HIP(hipMemsetAsync(flags, 0, nflags * sizeof(uint32_t), s));
  RD_HIP(hipMemsetAsync(flags, 1, 1, s));
  const uint32_t egrid = (uint32_t)((n + NTHR - 1) / NTHR), rgrid = std::min<uint32_t>(ntiles, 2048u);
  int launches = 0;
  auto round = [&](int l, int r, uint8_t *marks, uint32_t k) {
    uint32_t *f = flags + 1 + (size_t)l * stride;
    RD_LAUNCH(marks ? "streams.push" : "streams.round", k_so_round, dim3(rgrid), dim3(NTHR), 0, s,
              (const uint32_t *)(r == 0 ? nxt0 : pp[(r - 1) & 1]), pp[r & 1], marks, ntiles, (const uint8_t *)tmax, k,
              (const uint32_t *)(r == 0 ? (marks ? f + 1 : flags) : f + 2 + (r - 1)), f + 2 + r);
    launches++;
  };
  RD_LAUNCH("streams.init", k_so_init, dim3(egrid), dim3(NTHR), 0, s, d_dirs, nodata, d_chan, n, d_order);
  RD_LAUNCH("streams.links", k_so_links, dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_order, w, h, tilesX, ntiles,
            nxt0, tmax);
  launches += 2;
  // loops across tiles
  RD_HIP(hipMemsetAsync(nmark, 0, nnodes, s));
  for (int r = 0; r < rounds; r++) round(0, r, nullptr, 1u);
  const uint32_t *loop_gate = flags + 1 + 2 + (rounds - 1);
  RD_LAUNCH("streams.loopmark", k_so_loopmark, dim3((nnodes + NTHR - 1) / NTHR), dim3(NTHR), 0, s,
            (const uint32_t *)pp[(rounds - 1) & 1], nnodes, nmark, (const uint8_t *)tmax, loop_gate);
  RD_LAUNCH("streams.loops", (k_so_close<SO_LOOPS>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_order, w, h, tilesX,
            ntiles, 1u, nmark, tmax, loop_gate, (uint32_t *)nullptr, (uint32_t *)nullptr);
  launches += 2;
  for (int k = 1; k <= levels; k++) {
    uint32_t *f = flags + 1 + (size_t)k * stride;
    const uint32_t *before = k == 1 ? flags : f - stride;   // the level before found a junction
    RD_HIP(hipMemsetAsync(nmark, 0, nnodes, s));
    RD_LAUNCH("streams.seed", (k_so_close<SO_SEED>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_order, w, h, tilesX,
              ntiles, (uint32_t)k, nmark, tmax, before, f, f + 1);
    for (int r = 0; r < rounds; r++) round(k, r, nmark, (uint32_t)k);
    RD_LAUNCH("streams.write", (k_so_close<SO_WRITE>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_order, w, h,
              tilesX, ntiles, (uint32_t)k, nmark, tmax, (const uint32_t *)f, (uint32_t *)nullptr, (uint32_t *)nullptr);
    launches += 2;
  }
  so_last_levels = levels;
  so_last_rounds = rounds;
  so_last_launches = launches;
}

static void channels_device(const double *d_accum, double nodata, double threshold, int w, int h, uint8_t *d_chan, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  RD_LAUNCH("streams.channels", k_so_channels, dim3((uint32_t)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, d_accum, nodata, threshold,
            n, d_chan);
}

static void stream_links_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, const uint8_t *d_chan, const uint8_t *d_order,
                                uint8_t *d_kind, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  RD_LAUNCH("streams.kinds", k_so_kinds, dim3((uint32_t)((n + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, d_dirs, nodata, w, h, d_chan,
            d_order, d_kind);
}

}  // namespace rdgpu

using namespace rdgpu;

// host rasters: staged in the workspace, as d8_flow_accum's
extern "C" int rdgpu_d8_stream_order(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan,
                                     uint8_t *order) {
  return guarded([&] {
    so_check_args(dirs && order, width, height, "rdgpu_d8_stream_order");
    const size_t n = (size_t)width * height;
    HostStage st;
    const uint8_t *dd = st.in("host.dirs", dirs, n);
    const uint8_t *dc = st.in("host.streams.chan", chan, n);
    uint8_t *dout = st.out("host.streams.order", order, n);
    stream_order_device(dd, dir_nodata, width, height, dc, dout, nullptr);
    st.finish();
  });
}
extern "C" int rdgpu_d8_stream_order_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, const uint8_t *d_chan,
                                         uint8_t *d_order, void *hip_stream) {
  return guarded([&] {
    so_check_args(d_dirs && d_order, width, height, "rdgpu_d8_stream_order_dev");
    stream_order_device(d_dirs, dir_nodata, width, height, d_chan, d_order, (hipStream_t)hip_stream);
  });
}
extern "C" int rdgpu_d8_stream_order_get_stats(int *levels, int *rounds_per_level, int *launches) {
  if (levels) *levels = so_last_levels;
  if (rounds_per_level) *rounds_per_level = so_last_rounds;
  if (launches) *launches = so_last_launches;
  return RDGPU_OK;
}

extern "C" int rdgpu_d8_channels_f64(const double *accum, double accum_nodata, double threshold, int width, int height,
                                     uint8_t *chan) {
  return guarded([&] {
    so_check_channels_args(accum, chan, width, height, threshold, "rdgpu_d8_channels_f64");
    const size_t n = (size_t)width * height;
    HostStage st;
    const double *da = st.in("host.streams.accum", accum, n);
    uint8_t *dc = st.out("host.streams.chan", chan, n);
    channels_device(da, accum_nodata, threshold, width, height, dc, nullptr);
    st.finish();
  });
}
extern "C" int rdgpu_d8_channels_dev_f64(const double *d_accum, double accum_nodata, double threshold, int width, int height,
                                         uint8_t *d_chan, void *hip_stream) {
  return guarded([&] {
    so_check_channels_args(d_accum, d_chan, width, height, threshold, "rdgpu_d8_channels_dev_f64");
    channels_device(d_accum, accum_nodata, threshold, width, height, d_chan, (hipStream_t)hip_stream);
  });
}

extern "C" int rdgpu_d8_stream_links(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan,
                                     const uint8_t *order, uint8_t *kind) {
  return guarded([&] {
    so_check_args(dirs && order && kind, width, height, "rdgpu_d8_stream_links");
    const size_t n = (size_t)width * height;
    HostStage st;
    const uint8_t *dd = st.in("host.dirs", dirs, n);
    const uint8_t *dc = st.in("host.streams.chan", chan, n);
    const uint8_t *dord = st.in("host.streams.order", order, n);
    uint8_t *dk = st.out("host.streams.kind", kind, n);
    stream_links_device(dd, dir_nodata, width, height, dc, dord, dk, nullptr);
    st.finish();
  });
}
extern "C" int rdgpu_d8_stream_links_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, const uint8_t *d_chan,
                                         const uint8_t *d_order, uint8_t *d_kind, void *hip_stream) {
  return guarded([&] {
    so_check_args(d_dirs && d_order && d_kind, width, height, "rdgpu_d8_stream_links_dev");
    stream_links_device(d_dirs, dir_nodata, width, height, d_chan, d_order, d_kind, (hipStream_t)hip_stream);
  });
}
