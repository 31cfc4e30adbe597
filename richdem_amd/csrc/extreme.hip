// extreme.hip -- the largest or smallest value found upstream of every cell of a D8 direction forest, and the cell it sits
// at (TauDEM's "D8 extreme upslope value").  The contract is in include/rdgpu.h.
//
// streams.hip closes boolean marks downstream over doubled pointers, first in LDS, then over the border nodes; a boolean
// OR is an idempotent reduction, and so is a maximum.  Here the mark is an ordered KEY, one 64-bit word
//   key = ord(value) << 32 | (0xFFFFFFFF - cell)
// with ord a monotone map of T onto uint32 (~ord for the minimum), so that in both modes the answer is an unsigned 64-bit
// maximum in which the lowest cell index wins a tie without further work.  cell <= 0xFFFEFFFF, so the low word of a real
// key is never 0 and key == 0 means "no contribution"; value and cell are decoded from the key, nothing is gathered.
//   k_forest_links     the node links (d8_forest.hpp).
//   k_ex_close<SEED>   the cells' own keys, closed downstream INSIDE the tile by key pushing over doubled pointers in LDS;
//                      every cell whose link leaves the tile raises the key of the node it flows to.
//   k_forest_round     the node keys pushed over doubled node pointers (ping-pong buffers).  ceil(log2(nodes)) + 1 rounds
//                      are enqueued; a round returns at once on a device-side flag when its predecessor raised nothing.
//   k_ex_close<WRITE>  own keys plus the node keys of the tile's own border slots, closed in the tile; every cell decoded
//                      and the requested planes written once.
// Why the keys are pushed, and why a round that raises nothing ends a closure: d8_forest.hpp.
//
// No host synchronisation in the device driver; 2 memsets + 3 + rounds launches, fixed by the raster's size.
// LDS per block: 4752 B staged directions + 8448 B pointers + 33792 B keys = 46992 B: three blocks per CU.
// Scratch: two pointer buffers and one key per node, 16 B; 256 nodes per 4096 cells: 1 B per cell.
#include "d8_forest.hpp"

#include <algorithm>
#include <string>
#include <type_traits>

namespace rdgpu {

typedef unsigned long long exkey_t;

constexpr uint32_t EX_NONE = 0xFFFFFFFFu;   // at_cell: nothing upstream contributes
enum { EX_SEED = 0, EX_WRITE = 1 };

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
  exkey_t own[FOREST_RPT];
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
    own[j] = 0;
    if (gx < w && gy < h) {
      const uint32_t cell = (uint32_t)gy * (uint32_t)w + (uint32_t)gx;
      const T v = values[cell];
      if (ex_contributes<T>(v, value_nodata)) own[j] = ((exkey_t)(ex_ord<T>(v) ^ flip) << 32) | (exkey_t)(0xFFFFFFFFu - cell);
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
    exkey_t k = kind >= 0 ? own[j] : 0;   // (a cell that does not participate contributes nothing)
    if (MODE == EX_WRITE && kind >= 0) {
      const int slot = border_slot(lx, ly);
      if (slot >= 0) {
        const exkey_t nk = nkey[(size_t)t * TILE_SLOTS + slot];
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
  if (MODE == EX_SEED) {
    forest_push_exits(S.sd, nodata, S.key, exitmask, lx, ly0, x0, y0, tilesX, nkey, exit_out);
  } else {
    const uint32_t nd_bits = ex_bits<T>(value_nodata);
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
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
  check_forest_dims(w, h, who);
}

// arguments checked by the caller
template <class T>
static void extreme_device(const uint8_t *d_dirs, uint8_t nodata, const T *d_values, T value_nodata, int w, int h, int which,
                           T *d_extreme, uint32_t *d_at_cell, hipStream_t s) {
  const ForestDims fd(w, h);
  const uint32_t tilesX = fd.tilesX, ntiles = fd.ntiles, nnodes = (uint32_t)fd.nnodes;
  const int rounds = forest_rounds(nnodes);
  Workspace &ws = Workspace::get();
  uint32_t *pp[2] = {ws.buf<uint32_t>("extreme.nxt_a", nnodes), ws.buf<uint32_t>("extreme.nxt_b", nnodes)};
  exkey_t *nkey = ws.buf<exkey_t>("extreme.nkey", nnodes);
  // flags: [0] the seed pass raised a node key | [1 + r] round r raised one
  uint32_t *flags = ws.buf<uint32_t>("extreme.flags", (size_t)rounds + 1);
  RD_HIP(hipMemsetAsync(flags, 0, ((size_t)rounds + 1) * sizeof(uint32_t), s));
  RD_HIP(hipMemsetAsync(nkey, 0, (size_t)nnodes * sizeof(exkey_t), s));
  const uint32_t flip = which == RDGPU_EXTREME_MIN ? 0xFFFFFFFFu : 0u;
  const uint32_t rgrid = std::min<uint32_t>(ntiles, 2048u);
  RD_LAUNCH("extreme.links", k_forest_links, dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, w, h, tilesX, ntiles, pp[0]);
  RD_LAUNCH("extreme.seed", (k_ex_close<T, EX_SEED>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_values, value_nodata,
            w, h, tilesX, ntiles, flip, nkey, flags, (T *)nullptr, (uint32_t *)nullptr);
  for (int r = 0; r < rounds; r++)
    RD_LAUNCH("extreme.round", (k_forest_round<exkey_t>), dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)pp[r & 1], pp[(r + 1) & 1],
              nkey, nnodes, (const uint32_t *)(flags + r), flags + r + 1);
  RD_LAUNCH("extreme.write", (k_ex_close<T, EX_WRITE>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_values,
            value_nodata, w, h, tilesX, ntiles, flip, nkey, (uint32_t *)nullptr, d_extreme, d_at_cell);
}

// host rasters: staged in the workspace, as d8_flow_accum's
template <class T>
static void extreme_host(const uint8_t *dirs, uint8_t nodata, const T *values, T value_nodata, int w, int h, int which, T *extreme,
                         uint32_t *at_cell, const char *who) {
  ex_check_args(dirs, values, w, h, which, extreme, at_cell, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  const T *dv = st.in("host.extreme.values", values, n);
  T *de = st.out("host.extreme.extreme", extreme, n);
  uint32_t *da = st.out("host.extreme.at_cell", at_cell, n);
  extreme_device<T>(dd, nodata, dv, value_nodata, w, h, which, de, da, nullptr);
  st.finish();
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
