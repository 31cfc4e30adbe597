// accum_weighted.hip -- the sum of a weight raster over each cell's drainage area on a GIVEN D8 direction raster, and the
// total upstream length (TauDEM's tlen) made of three such sums.  The contract is in include/rdgpu.h.
//
// accum.hip's "last arriver continues" walk (its header explains the scheme) with three differences: the directions are
// the caller's and are read with the caller's dir_nodata; the weights are read in their own type W, once, by the tile
// pre-walk; and the totals are int64 for integer weights (unsigned long long on the device: the adds wrap like two's
// complement), double for float weights.
//   k_aw_prewalk<W, ACC, SRC>  every 64 x 64 tile in LDS: the cells' own weights (0 where a cell does not contribute),
//                              the pending words, and every walk that stays among the tile's interior cells; writes the
//                              totals so far, sum_nodata where dirs == dir_nodata, and the pending words.
//   k_aw_walk<ACC>             raster-wide: a lane takes a source, adds its total to the cell it flows to with one
//                              returning 64-bit atomic, then decrements that cell's pending word; the lane whose
//                              decrement was the last goes on from there.
//   k_aw_length                the total upstream length: the three step counts out of two sums, and the length.
// A pending word is (inflows in total << 12) | (link << 8) | inflows still to arrive.  `link` is the cell's code where its
// link EXISTS (code 1..8, target in the raster and participating) and 0 otherwise, so the walk never looks at the
// directions again and never touches a cell that does not participate.  The count byte AW_SRC marks a cell that is
// complete and still has to pass its total on, AW_NODATA a cell that does not participate (at most 8 arrivals decrement a
// count: neither ever reads as 1).  A cell on a direction loop never completes: one of its inflows is the loop's own
// link, which nothing ever walks, so it keeps its own weight plus what its tributaries brought.  Nothing is
// special-cased for loops.
//
// LDS per pre-walk block: 4752 B staged directions + 16384 B pending words + 32768 B totals = 53904 B: three blocks per CU.
// Scratch: one pending word per cell, 4 B; the upstream length 16 B per cell more (two sums).
#include "d8_forest.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>

namespace rdgpu {

constexpr uint32_t AW_SRC = 0xFEu, AW_NODATA = 0xF0u;
constexpr uint32_t AW_CHUNK = 8192;   // cells per wavefront of the walk
// where the pre-walk takes a cell's weight from
enum { AW_WEIGHTS = 0,   // the weight raster
       AW_AXIS = 1,      // 1 where the cell's link runs along x, 1 << 32 where it runs along y
       AW_DIAG = 2 };    // 1 where the cell's link is diagonal

template <class W>
__device__ __forceinline__ bool aw_contributes(W v, W nodata) {
  if constexpr (std::is_floating_point<W>::value) return v == v && v != nodata;   // (-0 == +0; a NaN never contributes)
  else return v != nodata;
}
// exact in both accumulators: every W fits int64, and every f32 is a double
template <class W, class ACC>
__device__ __forceinline__ ACC aw_widen(W v) {
  if constexpr (std::is_floating_point<ACC>::value) return (ACC)v;
  else return (ACC)(long long)v;
}
// the weight of a cell whose link is `link` (0: none) when the weights are step counts
template <class ACC, int SRC>
__device__ __forceinline__ ACC aw_step_weight(uint32_t link) {
  if (link == 0) return (ACC)0;
  if (SRC == AW_DIAG) return (ACC)((link & 1u) ? 0 : 1);
  return (link & 1u) ? ((link & 2u) ? (ACC)1 << 32 : (ACC)1) : (ACC)0;   // 1, 5 along x; 3, 7 along y
}

template <class ACC>
struct AwTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(8)));
  uint32_t lc[LT * LT];
  ACC lt[LT * LT] __attribute__((aligned(8)));
};

template <class W, class ACC, int SRC>
__global__ __launch_bounds__(NTHR, 3) void k_aw_prewalk(const uint8_t *__restrict__ dirs, uint8_t nodata,
                                                        const W *__restrict__ weights, W weight_nodata, int w, int h,
                                                        uint32_t tilesX, uint32_t ntiles, uint32_t *__restrict__ pending,
                                                        ACC *__restrict__ sum, ACC sum_nodata) {
  __shared__ AwTile<ACC> S;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, S.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  ACC own[FOREST_RPT];
  if (SRC == AW_WEIGHTS) {
    W wv[FOREST_RPT];
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {   // the weights in their own type: all loads in flight together
      const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
      wv[j] = (gx < w && gy < h) ? weights[(size_t)gy * w + gx] : weight_nodata;
    }
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) own[j] = aw_contributes<W>(wv[j], weight_nodata) ? aw_widen<W, ACC>(wv[j]) : (ACC)0;
  }
  __syncthreads();
  uint32_t srcmask = 0;
#pragma unroll 4
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j, o = (ly + 1) * SDW + SDO + lx;
    uint32_t v = AW_NODATA;
    ACC own_j = (ACC)0;
    if (S.sd[o] != nodata) {   // (cells outside the raster are staged as NoData)
      uint32_t k = 0;
#pragma unroll
      for (int m = 1; m <= 8; m++) {
        const uint8_t d = S.sd[o + d8dy(m) * SDW + d8dx(m)];
        if (d != nodata && d == (m <= 4 ? m + 4 : m - 4)) k++;   // neighbour m participates and points at this cell
      }
      int tx, ty;
      const uint32_t link = forest_link(S.sd, nodata, lx, ly, tx, ty) > 0 ? S.sd[o] : 0u;
      v = (k << 12) | (link << 8) | k;
      if (k == 0) srcmask |= 1u << j;
      if constexpr (SRC == AW_WEIGHTS) own_j = own[j];
      else own_j = aw_step_weight<ACC, SRC>(link);
    }
    S.lc[ly * LT + lx] = v;
    S.lt[ly * LT + lx] = own_j;
  }
  __syncthreads();
  {
    // a lane whose walk has ended takes its next source in the same trip.  LDS executes a wavefront's operations in
    // order and the adds and decrements are atomics on the one LDS, so the last decrementer's read comes after every
    // other arriver's add.
    uint32_t m = srcmask;
    bool active = false;
    int cx = 0, cy = 0;
    ACC v = (ACC)0;
    for (;;) {
      if (!active && m) {
        cx = lx; cy = ly0 + 4 * (__ffs((int)m) - 1);
        m &= m - 1;
        v = S.lt[cy * LT + cx];
        active = true;
      }
      if (!__any(active || m != 0)) break;
      if (active) {
        const uint32_t d = (S.lc[cy * LT + cx] >> 8) & 15u;
        bool stalled = false, cont = false;
        if (d != 0) {
          const int tx = cx + d8dx((int)d), ty = cy + d8dy((int)d);
          if (tx >= 1 && tx < LT - 1 && ty >= 1 && ty < LT - 1) {
            atomicAdd(&S.lt[ty * LT + tx], v);
            const uint32_t old = atomicSub(&S.lc[ty * LT + tx], 1u);
            if ((old & 0xFFu) == 1) {
              v = __hip_atomic_load(&S.lt[ty * LT + tx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              cx = tx; cy = ty;
              cont = true;
            }
          } else {
            stalled = true;   // a border cell of this tile or a cell of another: the raster-wide walk goes on from here
          }
        }
        // only this lane writes the word of the cell it stands on: the cell is complete, nothing arrives there any more
        if (stalled) S.lc[cy * LT + cx] = (S.lc[cy * LT + cx] & ~0xFFu) | AW_SRC;
        active = cont;
      }
    }
  }
  __syncthreads();
#pragma unroll 4
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j, gx = x0 + lx, gy = y0 + ly;
    if (gx >= w || gy >= h) continue;
    const size_t g = (size_t)gy * w + gx;
    const uint32_t v = S.lc[ly * LT + lx];
    pending[g] = v;
    sum[g] = v != AW_NODATA ? S.lt[ly * LT + lx] : sum_nodata;
  }
}

// the raster-wide walk (k_acc_walk_f64's, with the link in the pending word final: no look at the raster's edge or at a
// NoData target here)
template <class ACC>
__global__ __launch_bounds__(NTHR) void k_aw_walk(uint32_t *pending, ACC *sum, int w, uint64_t n) {
  const uint64_t wave = ((uint64_t)blockIdx.x * NTHR + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  uint64_t next = wave * AW_CHUNK;
  const uint64_t end = next + AW_CHUNK < n ? next + AW_CHUNK : n;
  if (next >= n) return;
  bool active = false;
  uint32_t c = 0, d = 0;
  ACC v = (ACC)0;
  for (;;) {
    const unsigned long long idle = __ballot(!active);
    if (next < end && idle) {
      const uint64_t my = next + (uint64_t)__popcll(idle & ((1ull << lane) - 1ull));
      if (!active && my < end) {
        // sources only; a source's word and total are never written by anyone else
        const uint32_t p = pending[my];
        if ((p & 0xFFu) == AW_SRC) { active = true; c = (uint32_t)my; v = sum[my]; d = (p >> 8) & 15u; }
      }
      next += (uint64_t)__popcll(idle);
    } else if (idle == ~0ull) {
      break;
    }
    if (active) {
      // d is 1..8 and its target lies in the raster and participates (the pre-walk wrote 0 otherwise)
      const uint32_t t = (uint32_t)((int64_t)c + (int64_t)d8dy((int)d) * w + d8dx((int)d));
      // Both steps are device-scope atomic read-modify-writes executed at the memory side: the RETURNING add has
      // completed there before the decrement is issued, and the last arriver's decrement is ordered after every other
      // arriver's decrement, hence after their adds.
      const ACC prev = atomicAdd(&sum[t], v);
      asm volatile("s_waitcnt vmcnt(0)" ::"v"(prev) : "memory");   // the add has returned
      const uint32_t old = __hip_atomic_fetch_sub(&pending[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      d = (old >> 8) & 15u;
      if ((old & 0xFFu) != 1 || d == 0) {
        active = false;   // not the last arriver, or t's tree ends at t
      } else {
        // t's only inflow (the common case): the add returned t's own weight, so its total is known without a third round
        // trip; at a confluence the final total is read back at the memory side
        v = ((old >> 12) & 15u) == 1 ? prev + v : atomicAdd(&sum[t], (ACC)0);
        c = t;
      }
    }
  }
}

// steps and length of the total upstream length.  axis = nx | ny << 32 and diag = nd are the sums of the links' kinds over
// T(v), v's own link among them: it is taken off here (the link is still in v's pending word).
__global__ __launch_bounds__(NTHR) void k_aw_length(const uint32_t *__restrict__ pending, const unsigned long long *__restrict__ axis,
                                                    const unsigned long long *__restrict__ diagsum, uint64_t n, double cx, double cy,
                                                    double diag, uint32_t *__restrict__ steps, double *__restrict__ length,
                                                    double length_nodata) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t p = pending[c];
    uint32_t nx = 0xFFFFFFFFu, ny = 0xFFFFFFFFu, nd = 0xFFFFFFFFu;
    const bool part = (p & 0xFFu) != AW_NODATA;
    if (part) {
      const uint32_t link = (p >> 8) & 15u;
      const unsigned long long a = axis[c] - aw_step_weight<unsigned long long, AW_AXIS>(link);
      nx = (uint32_t)a;
      ny = (uint32_t)(a >> 32);
      nd = (uint32_t)(diagsum[c] - aw_step_weight<unsigned long long, AW_DIAG>(link));
    }
    if (steps) {
      steps[c] = nx;
      steps[n + c] = ny;
      steps[2 * n + c] = nd;
    }
    if (length) length[c] = part ? d8_path_length(nx, ny, nd, cx, cy, diag) : length_nodata;
  }
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
// arguments checked by the caller
template <class W, class ACC, int SRC>
static void aw_accumulate(const uint8_t *d_dirs, uint8_t nodata, const W *d_weights, W weight_nodata, int w, int h, uint32_t *pending,
                          ACC *d_sum, ACC sum_nodata, hipStream_t s) {
  const ForestDims fd(w, h);
  const uint64_t n = (uint64_t)w * h;
  RD_LAUNCH("accum_weighted.prewalk", (k_aw_prewalk<W, ACC, SRC>), dim3(xcd_grid(fd.ntiles)), dim3(NTHR), 0, s, d_dirs, nodata,
            d_weights, weight_nodata, w, h, fd.tilesX, fd.ntiles, pending, d_sum, sum_nodata);
  RD_LAUNCH("accum_weighted.walk", (k_aw_walk<ACC>), dim3((uint32_t)(((n + AW_CHUNK - 1) / AW_CHUNK + 3) / 4)), dim3(NTHR), 0, s,
            pending, d_sum, w, n);
}

template <class W>
struct AwSum {
  typedef typename std::conditional<std::is_floating_point<W>::value, double, int64_t>::type S;
  typedef typename std::conditional<std::is_floating_point<W>::value, double, unsigned long long>::type ACC;
};

static void aw_check_args(const void *dirs, const void *weights, const void *sum, int w, int h, const char *who) {
  if (!dirs || !weights || !sum) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_forest_dims(w, h, who);
}

template <class W>
static void weighted_device(const uint8_t *d_dirs, uint8_t nodata, const W *d_weights, W weight_nodata, int w, int h,
                            typename AwSum<W>::S *d_sum, typename AwSum<W>::S sum_nodata, hipStream_t s) {
  typedef typename AwSum<W>::ACC ACC;
  uint32_t *pending = Workspace::get().buf<uint32_t>("accum_weighted.pending", (size_t)w * h);
  aw_accumulate<W, ACC, AW_WEIGHTS>(d_dirs, nodata, d_weights, weight_nodata, w, h, pending, reinterpret_cast<ACC *>(d_sum),
                                    (ACC)sum_nodata, s);
}

// host rasters: staged in the workspace, as d8_flow_accum's
template <class W>
static void weighted_host(const uint8_t *dirs, uint8_t nodata, const W *weights, W weight_nodata, int w, int h,
                          typename AwSum<W>::S *sum, typename AwSum<W>::S sum_nodata, const char *who) {
  typedef typename AwSum<W>::S S;
  aw_check_args(dirs, weights, sum, w, h, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  const W *dw = st.in("host.accum_weighted.weights", weights, n);
  S *ds = st.out("host.accum_weighted.sum", sum, n);
  weighted_device<W>(dd, nodata, dw, weight_nodata, w, h, ds, sum_nodata, nullptr);
  st.finish();
}

static void tlen_check_args(const void *dirs, int w, int h, double cx, double cy, const void *steps, const void *length,
                            const char *who) {
  if (!dirs) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  if (!steps && !length) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  check_forest_dims(w, h, who);
  check_cell_lengths(cx, cy, who);
}

// arguments checked by the caller
static void tlen_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, double cx, double cy, uint32_t *d_steps, double *d_length,
                        double length_nodata, hipStream_t s) {
  typedef unsigned long long ull;
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  uint32_t *pending = ws.buf<uint32_t>("accum_weighted.pending", n);
  ull *axis = ws.buf<ull>("accum_weighted.axis", n), *diagsum = ws.buf<ull>("accum_weighted.diag", n);
  // (the second accumulation rewrites the pending words: the same links, the counts of a finished walk)
  aw_accumulate<uint8_t, ull, AW_AXIS>(d_dirs, nodata, nullptr, 0, w, h, pending, axis, 0ull, s);
  aw_accumulate<uint8_t, ull, AW_DIAG>(d_dirs, nodata, nullptr, 0, w, h, pending, diagsum, 0ull, s);
  cx = std::fabs(cx);
  cy = std::fabs(cy);
  const double diag = std::sqrt(cx * cx + cy * cy);
  RD_LAUNCH("accum_weighted.length", k_aw_length, dim3((uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u)), dim3(NTHR), 0,
            s, (const uint32_t *)pending, (const ull *)axis, (const ull *)diagsum, n, cx, cy, diag, d_steps, d_length, length_nodata);
}

static void tlen_host(const uint8_t *dirs, uint8_t nodata, int w, int h, double cx, double cy, uint32_t *steps, double *length,
                      double length_nodata, const char *who) {
  tlen_check_args(dirs, w, h, cx, cy, steps, length, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  uint32_t *dst = st.out("host.accum_weighted.steps", steps, 3 * n);
  double *dl = st.out("host.accum_weighted.length", length, n);
  tlen_device(dd, nodata, w, h, cx, cy, dst, dl, length_nodata, nullptr);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_DEFINE_WEIGHTED(SUF, W, S)                                                                                                  \
  extern "C" int rdgpu_d8_flow_accum_weighted_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const W *weights, W weight_nodata,       \
                                                    int width, int height, S *sum, S sum_nodata) {                                    \
    return guarded([&] {                                                                                                               \
      weighted_host<W>(dirs, dir_nodata, weights, weight_nodata, width, height, sum, sum_nodata,                                      \
                       "rdgpu_d8_flow_accum_weighted_" #SUF);                                                                          \
    });                                                                                                                                \
  }                                                                                                                                    \
  extern "C" int rdgpu_d8_flow_accum_weighted_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const W *d_weights,                \
                                                        W weight_nodata, int width, int height, S *d_sum, S sum_nodata,               \
                                                        void *hip_stream) {                                                            \
    return guarded([&] {                                                                                                               \
      aw_check_args(d_dirs, d_weights, d_sum, width, height, "rdgpu_d8_flow_accum_weighted_dev_" #SUF);                               \
      weighted_device<W>(d_dirs, dir_nodata, d_weights, weight_nodata, width, height, d_sum, sum_nodata, (hipStream_t)hip_stream);    \
    });                                                                                                                                \
  }
RD_DEFINE_WEIGHTED(i8, int8_t, int64_t)
RD_DEFINE_WEIGHTED(u8, uint8_t, int64_t)
RD_DEFINE_WEIGHTED(i16, int16_t, int64_t)
RD_DEFINE_WEIGHTED(u16, uint16_t, int64_t)
RD_DEFINE_WEIGHTED(i32, int32_t, int64_t)
RD_DEFINE_WEIGHTED(u32, uint32_t, int64_t)
RD_DEFINE_WEIGHTED(f32, float, double)
RD_DEFINE_WEIGHTED(f64, double, double)
#undef RD_DEFINE_WEIGHTED

extern "C" int rdgpu_d8_total_upstream_length(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, double cell_x,
                                              double cell_y, uint32_t *steps, double *length, double length_nodata) {
  return guarded([&] {
    tlen_host(dirs, dir_nodata, width, height, cell_x, cell_y, steps, length, length_nodata, "rdgpu_d8_total_upstream_length");
  });
}
extern "C" int rdgpu_d8_total_upstream_length_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, double cell_x,
                                                  double cell_y, uint32_t *d_steps, double *d_length, double length_nodata,
                                                  void *hip_stream) {
  return guarded([&] {
    tlen_check_args(d_dirs, width, height, cell_x, cell_y, d_steps, d_length, "rdgpu_d8_total_upstream_length_dev");
    tlen_device(d_dirs, dir_nodata, width, height, cell_x, cell_y, d_steps, d_length, length_nodata, (hipStream_t)hip_stream);
  });
}
