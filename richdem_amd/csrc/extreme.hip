// extreme.hip -- the largest or smallest value found upstream of every cell of a D8 direction forest, and the cell it sits
// at (TauDEM's "D8 extreme upslope value").  The contract is in include/rdgpu.h.
//
// streams.hip closes boolean marks downstream over doubled pointers, first in LDS, then over the border nodes; a boolean
// OR is an idempotent reduction, and so is a maximum.  Here the mark is an ordered KEY, one 64-bit word
//   key = ord(value) << 32 | (0xFFFFFFFF - cell)
// with ord a monotone map of T onto uint32 (~ord for the minimum), so that in both modes the answer is an unsigned 64-bit
// maximum in which the lowest cell index wins a tie without further work.  cell <= 0xFFFEFFFF, so the low word of a real
// key is never 0 and key == 0 means "no contribution"; value and cell are decoded from the key, nothing is gathered.
//   k_ex_links         every 64 x 64 tile once: each cell pointer-jumped (synchronously) to the in-tile end of its path; a
//                      border cell publishes the node its path leaves the tile to (one word per border cell, 256 slots per
//                      tile), or NONE: the path ends in the tile or runs into a loop inside it.
//   k_ex_close<SEED>   the cells' own keys, closed downstream INSIDE the tile by key pushing over doubled pointers in LDS;
//                      every cell whose link leaves the tile raises the key of the node it flows to.
//   k_ex_round         the node keys pushed over doubled node pointers (ping-pong buffers, every node covers the same
//                      distance): nkey[nxt[i]] <- max(nkey[nxt[i]], nkey[i]).  ceil(log2(nodes)) + 1 rounds are enqueued;
//                      a round returns at once on a device-side flag when its predecessor raised nothing.
//   k_ex_close<WRITE>  own keys plus the node keys of the tile's own border slots, closed in the tile; every cell decoded
//                      and the requested planes written once.
// The keys must be PUSHED (a cell does not know its children's pointers), so the pull-style engines do not fit.
//
// Termination.  A closure round r: every cell reads the pointer q = lp[p] of the cell p it points to, barrier, raises
// key[p] to its own key (one ds_max_rtn_u64), stores q.  Pointers double synchronously, so before round r a pointer covers
// 2^r links (or stops at the path's end), and the cells holding a key >= K form, per source of such a key, a run along the
// path that starts at the source and is at least 2^r - 1 links long (exactly that without the races: pushes of one round
// race with each other, and a key raised early in a round may be pushed on in the same round.  That is harmless: keys only
// grow, a push is idempotent, and what arrives early is a key that flows there anyway).  A round pushes every run on by
// 2^r.  If a run ended at a cell x whose successor holds less, the cell 2^r - 1 links above x is in the run and pushes to
// that successor: the round raises a key.  So a round that raises nothing proves the closure, for every level set of the
// key at once.  On a direction loop the equal jumps rotate it; 12 rounds cover 4095 links, every path and every loop a
// tile can hold, and ceil(log2(nodes)) + 1 rounds every chain or loop of nodes.  Nothing is special-cased for loops.
//
// No host synchronisation in the device driver; 2 memsets + 3 + rounds launches, fixed by the raster's size.
// LDS per block: 4752 B staged directions + 8448 B pointers + 33792 B keys = 46992 B: three blocks per CU.
// Scratch: two pointer buffers and one key per node, 16 B; 256 nodes per 4096 cells: 1 B per cell.
#include "common.hpp"
#include "tile_front.hpp"

#include <algorithm>
#include <string>
#include <type_traits>

namespace rdgpu {

typedef unsigned long long exkey_t;

constexpr uint32_t EX_NONE = 0xFFFFFFFFu;
constexpr uint32_t EX_END = 0x8000u, EX_CELL = 0x7FFFu;   // k_ex_links' tile pointers: | EX_END when the cell is the END of the path
constexpr int EX_RPT = LT / 4;                            // rows (cells) per thread of a tile pass
constexpr int EX_JUMPS = 12;                              // 2^12 = 4096 cells: any path or loop inside a tile
enum { EX_SEED = 0, EX_WRITE = 1 };

struct ExLinkTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(4)));   // staged directions (tile_front.hpp)
  uint16_t lp[LT * LPS];                               // per cell: a cell further down its in-tile path
};
struct ExTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(8)));
  uint16_t lp[LT * LPS];
  exkey_t key[LT * LPS] __attribute__((aligned(8)));   // per cell: the best key known to reach it
};

// ord: T onto uint32, monotone.  f32: the IEEE total order on the non-NaN values, -inf < ... < -0 < +0 < ... < +inf.
template <class T>
__device__ __forceinline__ uint32_t ex_ord(T v) {
  if constexpr (std::is_same<T, float>::value) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  } else if constexpr (std::is_signed<T>::value) {
    return (uint32_t)(int32_t)v ^ 0x80000000u;
  } else {
    return (uint32_t)v;
  }
}
// the bits of the T that ord maps to o, zero-extended
template <class T>
__device__ __forceinline__ uint32_t ex_unord(uint32_t o) {
  if constexpr (std::is_same<T, float>::value) return (o >> 31) ? o ^ 0x80000000u : ~o;
  else if constexpr (std::is_signed<T>::value) return o ^ 0x80000000u;
  else return o;
}
template <class T>
__device__ __forceinline__ bool ex_contributes(T v, T nodata) {
  if constexpr (std::is_same<T, float>::value) return v == v && v != nodata;   // (-0 == +0; a NaN never contributes)
  else return v != nodata;
}
template <class T>
__device__ __forceinline__ void ex_store_bits(T *p, uint32_t bits) {
  if constexpr (sizeof(T) == 4) *reinterpret_cast<uint32_t *>(p) = bits;
  else if constexpr (sizeof(T) == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)bits;
  else *reinterpret_cast<uint8_t *>(p) = (uint8_t)bits;
}
template <class T>
__device__ __forceinline__ uint32_t ex_bits(T v) {
  if constexpr (std::is_same<T, float>::value) return __float_as_uint(v);
  else if constexpr (sizeof(T) == 4) return (uint32_t)v;
  else if constexpr (sizeof(T) == 2) return (uint32_t)(uint16_t)v;
  else return (uint32_t)(uint8_t)v;
}

// the link of the cell (lx, ly) of the staged tile: -1 the cell does not participate (NoData, or outside the raster: staged
// as NoData), 0 none (its tree ends here: no direction, or a target that is off the raster or NoData), 1 to (tx, ty) inside
// the tile, 2 to (tx, ty) in another tile
__device__ __forceinline__ int ex_link(const uint8_t *sd, uint8_t nodata, int lx, int ly, int &tx, int &ty) {
  const uint32_t d = sd[(ly + 1) * SDW + SDO + lx];
  tx = lx; ty = ly;
  if (d == nodata) return -1;
  if (d - 1u >= 8u) return 0;
  tx = lx + d8dx((int)d); ty = ly + d8dy((int)d);
  if (sd[(ty + 1) * SDW + SDO + tx] == nodata) return 0;
  return (tx >= 0 && tx < LT && ty >= 0 && ty < LT) ? 1 : 2;
}
__device__ __forceinline__ uint32_t ex_node(int gx, int gy, uint32_t tilesX) {
  return ((uint32_t)(gy / LT) * tilesX + (uint32_t)(gx / LT)) * 256u + (uint32_t)border_slot(gx % LT, gy % LT);
}
__device__ __forceinline__ void ex_border_cell(int slot, int &bx, int &by) {
  bx = slot < LT ? slot : slot < 2 * LT ? slot - LT : slot < 3 * LT - 2 ? 0 : LT - 1;
  by = slot < LT ? 0 : slot < 2 * LT ? LT - 1 : slot < 3 * LT - 2 ? slot - 2 * LT + 1 : slot - (3 * LT - 2) + 1;
}

// ---- the link forest of the border cells -------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR, 5) void k_ex_links(const uint8_t *__restrict__ dirs, uint8_t nodata, int w, int h, uint32_t tilesX,
                                                      uint32_t ntiles, uint32_t *__restrict__ nxt0) {
  __shared__ ExLinkTile T;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, T.sd);
  __syncthreads();
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t p[EX_RPT], q[EX_RPT];
#pragma unroll
  for (int j = 0; j < EX_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int kind = ex_link(T.sd, nodata, lx, ly, tx, ty);
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : (self | EX_END);
    T.lp[self] = (uint16_t)p[j];
  }
  __syncthreads();
  // synchronous doubling: after round r a pointer without EX_END covers exactly 2^(r+1) cells
#pragma unroll 1
  for (int it = 0; it < EX_JUMPS; it++) {
    bool moving = false;
#pragma unroll
    for (int j = 0; j < EX_RPT; j++) q[j] = (p[j] & EX_END) ? p[j] : T.lp[p[j]];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EX_RPT; j++) {
      p[j] = q[j];
      moving |= !(q[j] & EX_END);
      T.lp[(ly0 + 4 * j) * LPS + lx] = (uint16_t)q[j];
    }
    if (!__syncthreads_or(moving)) break;
  }
  // the node a path that ENTERS the tile at a border cell leaves it to, one border cell per thread (a pointer without
  // EX_END after the last round: into a loop inside the tile)
  const int slot = (int)threadIdx.x;
  uint32_t word = EX_NONE;
  if (slot < 4 * LT - 4) {
    int bx, by, tx, ty;
    ex_border_cell(slot, bx, by);
    const uint32_t rp = T.lp[by * LPS + bx], root = rp & EX_CELL;
    if (rp & EX_END) {
      const int ry = (int)root / LPS, rx = (int)root - ry * LPS;
      if (ex_link(T.sd, nodata, rx, ry, tx, ty) == 2) word = ex_node(x0 + tx, y0 + ty, tilesX);
    }
  }
  nxt0[(size_t)t * 256 + slot] = word;
}

// ---- one doubling round over the nodes ---------------------------------------------------------------------------------
// From src into dst (never in place: every node covers the same distance); a node raises the key of the node it points to
// (one global_atomic_umax_x2).  flag_out: a key was raised.
__global__ __launch_bounds__(NTHR) void k_ex_round(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, exkey_t *nkey,
                                                   uint32_t nnodes, const uint32_t *__restrict__ gate, uint32_t *flag_out) {
  if (*gate == 0) return;
  bool flag = false;
  for (uint32_t i = blockIdx.x * NTHR + threadIdx.x; i < nnodes; i += gridDim.x * NTHR) {   // (nnodes: a multiple of NTHR)
    const uint32_t n = src[i];
    uint32_t n2 = EX_NONE;
    if (n < nnodes) {
      n2 = src[n];
      const exkey_t k = __hip_atomic_load(&nkey[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k != 0) flag |= atomicMax(&nkey[n], k) < k;
    }
    dst[i] = n2;
  }
  if (__any(flag) && (threadIdx.x & 63) == 0) *flag_out = 1;
}

// ---- the closure inside a tile ---------------------------------------------------------------------------------------------
// EX_SEED:  keys = the cells' own; closed in the tile; a cell whose link leaves the tile raises the node it flows to.
//           exit_out: a node key was raised.
// EX_WRITE: keys = the cells' own and the node keys of the tile's border slots; closed in the tile; decoded and written.
template <class T, int MODE>
__global__ __launch_bounds__(NTHR, 3) void k_ex_close(const uint8_t *__restrict__ dirs, uint8_t nodata, const T *__restrict__ values,
                                                      T value_nodata, int w, int h, uint32_t tilesX, uint32_t ntiles, uint32_t flip,
                                                      exkey_t *nkey, uint32_t *exit_out, T *__restrict__ extreme,
                                                      uint32_t *__restrict__ at_cell) {
  __shared__ ExTile S;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, S.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // the values are read once per cell by the cell's own thread: no LDS copy
  exkey_t own[EX_RPT];
#pragma unroll
  for (int j = 0; j < EX_RPT; j++) {
    const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
    own[j] = 0;
    if (gx < w && gy < h) {
      const uint32_t cell = (uint32_t)gy * (uint32_t)w + (uint32_t)gx;
      const T v = values[cell];
      if (ex_contributes<T>(v, value_nodata)) own[j] = ((exkey_t)(ex_ord<T>(v) ^ flip) << 32) | (exkey_t)(0xFFFFFFFFu - cell);
    }
  }
  __syncthreads();
  uint32_t p[EX_RPT], q[EX_RPT];
  uint32_t exitmask = 0;
  bool keyed = false;
#pragma unroll
  for (int j = 0; j < EX_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int kind = ex_link(S.sd, nodata, lx, ly, tx, ty);
    exkey_t k = kind >= 0 ? own[j] : 0;   // (a cell that does not participate contributes nothing)
    if (MODE == EX_WRITE && kind >= 0) {
      const int slot = border_slot(lx, ly);
      if (slot >= 0) {
        const exkey_t nk = nkey[(size_t)t * 256 + slot];
        k = nk > k ? nk : k;
      }
    }
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : self;   // an end cell points at itself
    exitmask |= (kind == 2 ? 1u : 0u) << j;
    S.lp[self] = (uint16_t)p[j];
    S.key[self] = k;
    keyed |= k != 0;
  }
  if (__syncthreads_or(keyed)) {
    // the keys pushed down the in-tile paths: round r pushes by 2^r; a round that raises nothing has closed them
#pragma unroll 1
    for (int it = 0; it < EX_JUMPS; it++) {
      bool fresh = false;
#pragma unroll
      for (int j = 0; j < EX_RPT; j++) q[j] = S.lp[p[j]];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < EX_RPT; j++) {
        const uint32_t self = (uint32_t)((ly0 + 4 * j) * LPS + lx);
        if (p[j] != self) {
          const exkey_t k = __hip_atomic_load(&S.key[self], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (k != 0) fresh |= atomicMax(&S.key[p[j]], k) < k;
        }
        S.lp[self] = (uint16_t)q[j];
      }
      if (!__syncthreads_or(fresh)) break;
#pragma unroll
      for (int j = 0; j < EX_RPT; j++) p[j] = q[j];
    }
  }
  if (MODE == EX_SEED) {
    bool pushed = false;
#pragma unroll
    for (int j = 0; j < EX_RPT; j++) {
      if (!(exitmask >> j & 1u)) continue;
      const int ly = ly0 + 4 * j;
      const exkey_t k = S.key[ly * LPS + lx];
      if (k == 0) continue;
      int tx, ty;
      ex_link(S.sd, nodata, lx, ly, tx, ty);
      atomicMax(&nkey[ex_node(x0 + tx, y0 + ty, tilesX)], k);   // (the target participates: inside the raster)
      pushed = true;
    }
    if (__any(pushed) && (threadIdx.x & 63) == 0) *exit_out = 1;
  } else {
    const uint32_t nd_bits = ex_bits<T>(value_nodata);
#pragma unroll
    for (int j = 0; j < EX_RPT; j++) {
      const int ly = ly0 + 4 * j, gx = x0 + lx, gy = y0 + ly;
      if (gx >= w || gy >= h) continue;
      const exkey_t k = S.key[ly * LPS + lx];
      const size_t g = (size_t)gy * w + gx;
      if (extreme) ex_store_bits<T>(extreme + g, k != 0 ? ex_unord<T>((uint32_t)(k >> 32) ^ flip) : nd_bits);
      if (at_cell) at_cell[g] = k != 0 ? 0xFFFFFFFFu - (uint32_t)k : EX_NONE;
    }
  }
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
static void ex_check_args(const void *dirs, const void *values, int w, int h, int which, const void *extreme, const void *at_cell,
                          const char *who) {
  if (!dirs || !values) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  if (!extreme && !at_cell) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  if (which != RDGPU_EXTREME_MAX && which != RDGPU_EXTREME_MIN)
    throw Error(RDGPU_ERR_ARG, std::string(who) + ": which must be RDGPU_EXTREME_MAX or RDGPU_EXTREME_MIN");
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, std::string(who) + ": width and height must be positive");
  if ((uint64_t)w * (uint64_t)h > 0xFFFF0000ull) throw Error(RDGPU_ERR_ARG, std::string(who) + ": raster too large");
}

// arguments checked by the caller
template <class T>
static void extreme_device(const uint8_t *d_dirs, uint8_t nodata, const T *d_values, T value_nodata, int w, int h, int which,
                           T *d_extreme, uint32_t *d_at_cell, hipStream_t s) {
  const uint32_t tilesX = (w + LT - 1) / LT, ntiles = tilesX * ((h + LT - 1) / LT);
  const uint32_t nnodes = ntiles * 256u;   // (at most 0xFFFF0000 cells: below 2^29 nodes)
  int rounds = 1;
  while ((1ull << (rounds - 1)) < nnodes) rounds++;   // ceil(log2(nodes)) + 1
  Workspace &ws = Workspace::get();
  uint32_t *pp[2] = {ws.buf<uint32_t>("extreme.nxt_a", nnodes), ws.buf<uint32_t>("extreme.nxt_b", nnodes)};
  exkey_t *nkey = ws.buf<exkey_t>("extreme.nkey", nnodes);
  // flags: [0] the seed pass raised a node key | [1 + r] round r raised one
  uint32_t *flags = ws.buf<uint32_t>("extreme.flags", (size_t)rounds + 1);
  RD_HIP(hipMemsetAsync(flags, 0, ((size_t)rounds + 1) * sizeof(uint32_t), s));
  RD_HIP(hipMemsetAsync(nkey, 0, (size_t)nnodes * sizeof(exkey_t), s));
  const uint32_t flip = which == RDGPU_EXTREME_MIN ? 0xFFFFFFFFu : 0u;
  const uint32_t rgrid = std::min<uint32_t>(ntiles, 2048u);
  RD_LAUNCH("extreme.links", k_ex_links, dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, w, h, tilesX, ntiles, pp[0]);
  RD_LAUNCH("extreme.seed", (k_ex_close<T, EX_SEED>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_values, value_nodata,
            w, h, tilesX, ntiles, flip, nkey, flags, (T *)nullptr, (uint32_t *)nullptr);
  for (int r = 0; r < rounds; r++)
    RD_LAUNCH("extreme.round", k_ex_round, dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)pp[r & 1], pp[(r + 1) & 1], nkey, nnodes,
              (const uint32_t *)(flags + r), flags + r + 1);
  RD_LAUNCH("extreme.write", (k_ex_close<T, EX_WRITE>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_values,
            value_nodata, w, h, tilesX, ntiles, flip, nkey, (uint32_t *)nullptr, d_extreme, d_at_cell);
}

// host rasters: staged in the workspace, as d8_flow_accum's
template <class T>
static void extreme_host(const uint8_t *dirs, uint8_t nodata, const T *values, T value_nodata, int w, int h, int which, T *extreme,
                         uint32_t *at_cell, const char *who) {
  ex_check_args(dirs, values, w, h, which, extreme, at_cell, who);
  const size_t n = (size_t)w * h;
  Workspace &ws = Workspace::get();
  uint8_t *dd = ws.buf<uint8_t>("host.dirs", n);
  T *dv = ws.buf<T>("host.extreme.values", n);
  T *de = extreme ? ws.buf<T>("host.extreme.extreme", n) : nullptr;
  uint32_t *da = at_cell ? ws.buf<uint32_t>("host.extreme.at_cell", n) : nullptr;
  RD_HIP(hipMemcpy(dd, dirs, n, hipMemcpyHostToDevice));
  RD_HIP(hipMemcpy(dv, values, n * sizeof(T), hipMemcpyHostToDevice));
  extreme_device<T>(dd, nodata, dv, value_nodata, w, h, which, de, da, nullptr);
  RD_HIP(hipStreamSynchronize(nullptr));
  if (extreme) RD_HIP(hipMemcpy(extreme, de, n * sizeof(T), hipMemcpyDeviceToHost));
  if (at_cell) RD_HIP(hipMemcpy(at_cell, da, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_DEFINE_EXTREME(SUF, T)                                                                                                    \
  extern "C" int rdgpu_d8_upslope_extreme_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const T *values, T value_nodata, int width, \
                                                int height, int which, T *extreme, uint32_t *at_cell) {                              \
    return guarded([&] {                                                                                                             \
      extreme_host<T>(dirs, dir_nodata, values, value_nodata, width, height, which, extreme, at_cell,                                \
                      "rdgpu_d8_upslope_extreme_" #SUF);                                                                             \
    });                                                                                                                              \
  }                                                                                                                                  \
  extern "C" int rdgpu_d8_upslope_extreme_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const T *d_values, T value_nodata,    \
                                                    int width, int height, int which, T *d_extreme, uint32_t *d_at_cell,             \
                                                    void *hip_stream) {                                                              \
    return guarded([&] {                                                                                                             \
      ex_check_args(d_dirs, d_values, width, height, which, d_extreme, d_at_cell, "rdgpu_d8_upslope_extreme_dev_" #SUF);             \
      extreme_device<T>(d_dirs, dir_nodata, d_values, value_nodata, width, height, which, d_extreme, d_at_cell,                      \
                        (hipStream_t)hip_stream);                                                                                    \
    });                                                                                                                              \
  }
RD_DEFINE_EXTREME(i8, int8_t)
RD_DEFINE_EXTREME(u8, uint8_t)
RD_DEFINE_EXTREME(i16, int16_t)
RD_DEFINE_EXTREME(u16, uint16_t)
RD_DEFINE_EXTREME(i32, int32_t)
RD_DEFINE_EXTREME(u32, uint32_t)
RD_DEFINE_EXTREME(f32, float)
#undef RD_DEFINE_EXTREME
