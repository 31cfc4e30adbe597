// accum_limited.hip -- D8 accumulation with a per-cell limit on what a cell passes on: a storage deficit (a negative
// supply), a decay factor, a transport capacity.  The contract is in include/rdgpu.h.
//
// accum_weighted.hip's "last arriver continues" walk (accum.hip's header explains the scheme) with the same pending word
// ((inflows in total << 12) | (link << 8) | inflows still to arrive; AL_SRC / AL_NODATA in the count byte) and one
// difference: when a lane completes a cell, that cell's TOTAL is final, and what the lane adds to the next cell is
// AlLimits::out(total), not the total.  The totals stay in the accumulator plane; k_al_finish evaluates the same function
// on them once more for the planes the caller reads, so the value passed on and the `out` written are the same double
// (one multiply, two compares, no fused operation: the library is built with -ffp-contract=off).
//   k_al_prewalk<W, CAP, FAC>  every 64 x 64 tile in LDS: supplies, pending words, every walk among the tile's interior
//                              cells; the block's contributing supplies into result->supplied.
//   k_al_walk<W, CAP, FAC>     raster-wide, one returning f64 atomic add and one decrement per step.
//   k_al_finish<W, CAP, FAC>   out, kept and the three other sums of result from the totals.  A cell whose count byte
//                              is neither 0 nor AL_SRC nor AL_NODATA never completed: it lies on a loop.
// capacity and factor are read from global memory where a cell completes (each cell completes at most once, so at most
// one read per cell and plane over the two walks, one more in the finish): LDS stays at the linear walk's 53904 B (+ 32 B
// for the block sum), three blocks per CU.  The raster-wide walk issues the loads for the TARGET ahead of its two atomics,
// so they add no round trip to a step.  CAP / FAC are compile-time: a call without a limit runs kernels without the loads.
// Scratch: one pending word per cell, 4 B; 8 B more for the totals when neither plane is requested.
#include "d8_forest.hpp"

#include <algorithm>
#include <string>

namespace rdgpu {

constexpr uint32_t AL_SRC = 0xFEu, AL_NODATA = 0xF0u;
constexpr uint32_t AL_CHUNK = 8192;   // cells per wavefront of the walk

// the limits of one cell, and the node function
template <class W, bool CAP, bool FAC>
struct AlLimits {
  double c = 0.0, f = 0.0;
  __device__ __forceinline__ void load(const W *__restrict__ cap, const W *__restrict__ fac, size_t g) {
    if constexpr (CAP) c = (double)cap[g];
    if constexpr (FAC) f = (double)fac[g];
  }
  // min(max(factor * total, 0), max(capacity, 0)); a NaN factor is 1, a NaN capacity no limit.  Compares, not fmax / fmin:
  // a NaN product and -0.0 both give +0.0.
  __device__ __forceinline__ double out(double total) const {
    double a = total;
    if constexpr (FAC) {
      if (f == f) a = __dmul_rn(f, total);
    }
    a = a > 0.0 ? a : 0.0;
    if constexpr (CAP) {
      if (c == c) {
        const double lim = c > 0.0 ? c : 0.0;
        a = a < lim ? a : lim;
      }
    }
    return a;
  }
};

__device__ __forceinline__ double al_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct AlTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(8)));
  uint32_t lc[LT * LT];
  double lt[LT * LT] __attribute__((aligned(8)));
  double red[NTHR / 64];
};

template <class W, bool CAP, bool FAC>
__global__ __launch_bounds__(NTHR, 3) void k_al_prewalk(const uint8_t *__restrict__ dirs, uint8_t nodata,
                                                        const W *__restrict__ supply, W supply_nodata,
                                                        const W *__restrict__ cap, const W *__restrict__ fac, int w, int h,
                                                        uint32_t tilesX, uint32_t ntiles, uint32_t *__restrict__ pending,
                                                        double *__restrict__ total, double nodata_out,
                                                        rdgpu_limited_result *result) {
  __shared__ AlTile S;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, S.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double own[FOREST_RPT];
  {
    W sv[FOREST_RPT];
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {   // the supplies in their own type: all loads in flight together
      const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
      sv[j] = (gx < w && gy < h) ? supply[(size_t)gy * w + gx] : supply_nodata;
    }
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) own[j] = (sv[j] == sv[j] && sv[j] != supply_nodata) ? (double)sv[j] : 0.0;
  }
  __syncthreads();
  uint32_t srcmask = 0;
  double supplied = 0.0;
#pragma unroll 4
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j, o = (ly + 1) * SDW + SDO + lx;
    uint32_t v = AL_NODATA;
    double own_j = 0.0;
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
      own_j = own[j];
      supplied += own_j;
    }
    S.lc[ly * LT + lx] = v;
    S.lt[ly * LT + lx] = own_j;
  }
  if (result) {   // (uniform)
    supplied = al_wave_sum(supplied);
    if ((threadIdx.x & 63) == 0) S.red[threadIdx.x >> 6] = supplied;
  }
  __syncthreads();
  if (result && threadIdx.x == 0) {
    double b = S.red[0];
#pragma unroll
    for (int i = 1; i < NTHR / 64; i++) b += S.red[i];
    atomicAdd(&result->supplied, b);
  }
  {
    // accum_weighted.hip's in-tile walk: v is the TOTAL of the cell the lane stands on, complete and final; what it adds to
    // the next cell is that cell's out.  The limits of a participating cell are read at its raster index: in bounds.
    uint32_t m = srcmask;
    bool active = false;
    int cx = 0, cy = 0;
    double v = 0.0;
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
            AlLimits<W, CAP, FAC> lim;
            lim.load(cap, fac, (size_t)(y0 + cy) * w + (x0 + cx));
            atomicAdd(&S.lt[ty * LT + tx], lim.out(v));
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
        if (stalled) S.lc[cy * LT + cx] = (S.lc[cy * LT + cx] & ~0xFFu) | AL_SRC;
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
    total[g] = v != AL_NODATA ? S.lt[ly * LT + lx] : nodata_out;
  }
}

// the raster-wide walk (k_aw_walk's).  v is the total of the cell c the lane stands on and lim that cell's limits; the
// limits of the target are requested before the two atomics and have arrived with the add's return.
template <class W, bool CAP, bool FAC>
__global__ __launch_bounds__(NTHR) void k_al_walk(uint32_t *pending, double *total, const W *__restrict__ cap,
                                                  const W *__restrict__ fac, int w, uint64_t n) {
  const uint64_t wave = ((uint64_t)blockIdx.x * NTHR + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  uint64_t next = wave * AL_CHUNK;
  const uint64_t end = next + AL_CHUNK < n ? next + AL_CHUNK : n;
  if (next >= n) return;
  bool active = false;
  uint32_t c = 0, d = 0;
  double v = 0.0;
  AlLimits<W, CAP, FAC> lim;
  for (;;) {
    const unsigned long long idle = __ballot(!active);
    if (next < end && idle) {
      const uint64_t my = next + (uint64_t)__popcll(idle & ((1ull << lane) - 1ull));
      if (!active && my < end) {
        // sources only; a source's word and total are never written by anyone else
        const uint32_t p = pending[my];
        if ((p & 0xFFu) == AL_SRC) {
          active = true; c = (uint32_t)my; v = total[my]; d = (p >> 8) & 15u;
          lim.load(cap, fac, my);
        }
      }
      next += (uint64_t)__popcll(idle);
    } else if (idle == ~0ull) {
      break;
    }
    if (active) {
      // d is 1..8 and its target lies in the raster and participates (the pre-walk wrote 0 otherwise)
      const uint32_t t = (uint32_t)((int64_t)c + (int64_t)d8dy((int)d) * w + d8dx((int)d));
      AlLimits<W, CAP, FAC> tl;
      tl.load(cap, fac, t);
      const double o = lim.out(v);
      // Both steps are device-scope atomic read-modify-writes executed at the memory side: the RETURNING add has
      // completed there before the decrement is issued, and the last arriver's decrement is ordered after every other
      // arriver's decrement, hence after their adds.
      const double prev = atomicAdd(&total[t], o);
      asm volatile("s_waitcnt vmcnt(0)" ::"v"(prev) : "memory");   // the add has returned
      const uint32_t old = __hip_atomic_fetch_sub(&pending[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      d = (old >> 8) & 15u;
      if ((old & 0xFFu) != 1 || d == 0) {
        active = false;   // not the last arriver, or t's tree ends at t
      } else {
        // t's only inflow (the common case): the add returned t's own supply, so its total is prev + o, the sum the
        // memory side formed; at a confluence the final total is read back there
        v = ((old >> 12) & 15u) == 1 ? prev + o : atomicAdd(&total[t], 0.0);
        c = t;
        lim = tl;
      }
    }
  }
}

// out, kept and result's left / kept_pos / kept_neg from the totals.  acc may be `out` or `kept` itself: a thread reads
// its cell's total before it writes either plane.
template <class W, bool CAP, bool FAC>
__global__ __launch_bounds__(NTHR) void k_al_finish(const uint32_t *__restrict__ pending, const double *acc,
                                                    const W *__restrict__ cap, const W *__restrict__ fac, uint64_t n, double *out,
                                                    double *kept, double nodata_out, rdgpu_limited_result *result) {
  __shared__ double red[3][NTHR / 64];
  double left = 0.0, kpos = 0.0, kneg = 0.0;
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t p = pending[c], cnt = p & 0xFFu;
    double o = nodata_out, k = nodata_out;
    if (cnt != AL_NODATA) {
      const double tot = acc[c];
      if (cnt == 0 || cnt == AL_SRC) {
        AlLimits<W, CAP, FAC> lim;
        lim.load(cap, fac, c);
        o = lim.out(tot);
        k = __dsub_rn(tot, o);
        if (((p >> 8) & 15u) == 0) left += o;
      } else {   // on a loop: never complete
        o = 0.0;
        k = tot;
      }
      if (k > 0.0) kpos += k;
      else if (k < 0.0) kneg += k;
    }
    if (out) out[c] = o;
    if (kept) kept[c] = k;
  }
  if (!result) return;   // (uniform)
  left = al_wave_sum(left);
  kpos = al_wave_sum(kpos);
  kneg = al_wave_sum(kneg);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = left;
    red[1][threadIdx.x >> 6] = kpos;
    red[2][threadIdx.x >> 6] = kneg;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double b = red[threadIdx.x][0];
#pragma unroll
    for (int i = 1; i < NTHR / 64; i++) b += red[threadIdx.x][i];
    double *dst = threadIdx.x == 0 ? &result->left : threadIdx.x == 1 ? &result->kept_pos : &result->kept_neg;
    if (b != 0.0) atomicAdd(dst, b);
  }
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
static void al_check_args(const void *dirs, const void *supply, const void *out, const void *kept, const void *result, int w, int h,
                          const char *who) {
  if (!dirs || !supply) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  if (!out && !kept && !result) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  check_forest_dims(w, h, who);
}

template <class W, bool CAP, bool FAC>
static void al_launch(const uint8_t *d_dirs, uint8_t nodata, const W *d_supply, W supply_nodata, const W *d_cap, const W *d_fac, int w,
                      int h, uint32_t *pending, double *acc, double *d_out, double *d_kept, double nodata_out,
                      rdgpu_limited_result *d_result, hipStream_t s) {
  const ForestDims fd(w, h);
  const uint64_t n = (uint64_t)w * h;
  RD_LAUNCH("accum_limited.prewalk", (k_al_prewalk<W, CAP, FAC>), dim3(xcd_grid(fd.ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_supply,
            supply_nodata, d_cap, d_fac, w, h, fd.tilesX, fd.ntiles, pending, acc, nodata_out, d_result);
  RD_LAUNCH("accum_limited.walk", (k_al_walk<W, CAP, FAC>), dim3((uint32_t)(((n + AL_CHUNK - 1) / AL_CHUNK + 3) / 4)), dim3(NTHR), 0, s,
            pending, acc, d_cap, d_fac, w, n);
  RD_LAUNCH("accum_limited.finish", (k_al_finish<W, CAP, FAC>), dim3((uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u)),
            dim3(NTHR), 0, s, (const uint32_t *)pending, (const double *)acc, d_cap, d_fac, n, d_out, d_kept, nodata_out, d_result);
}

// arguments checked by the caller.  The totals are accumulated in a plane the caller gave where there is one.
template <class W>
static void limited_device(const uint8_t *d_dirs, uint8_t nodata, const W *d_supply, W supply_nodata, const W *d_cap, const W *d_fac,
                           int w, int h, double *d_out, double *d_kept, double nodata_out, rdgpu_limited_result *d_result,
                           hipStream_t s) {
  const size_t n = (size_t)w * h;
  Workspace &ws = Workspace::get();
  uint32_t *pending = ws.buf<uint32_t>("accum_limited.pending", n);
  double *acc = d_kept ? d_kept : d_out ? d_out : ws.buf<double>("accum_limited.total", n);
  if (d_result) RD_HIP(hipMemsetAsync(d_result, 0, sizeof(rdgpu_limited_result), s));
#define RD_AL_GO(CAP, FAC)                                                                                                             \
  al_launch<W, CAP, FAC>(d_dirs, nodata, d_supply, supply_nodata, d_cap, d_fac, w, h, pending, acc, d_out, d_kept, nodata_out,        \
                         d_result, s)
  if (d_cap && d_fac) RD_AL_GO(true, true);
  else if (d_cap) RD_AL_GO(true, false);
  else if (d_fac) RD_AL_GO(false, true);
  else RD_AL_GO(false, false);
#undef RD_AL_GO
}

// host rasters: staged in the workspace, as d8_flow_accum_weighted's
template <class W>
static void limited_host(const uint8_t *dirs, uint8_t nodata, const W *supply, W supply_nodata, const W *cap, const W *fac, int w, int h,
                         double *out, double *kept, double nodata_out, rdgpu_limited_result *result, const char *who) {
  al_check_args(dirs, supply, out, kept, result, w, h, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  const W *dsup = st.in("host.accum_limited.supply", supply, n);
  const W *dcap = st.in("host.accum_limited.capacity", cap, n);
  const W *dfac = st.in("host.accum_limited.factor", fac, n);
  double *dout = st.out("host.accum_limited.out", out, n);
  double *dkept = st.out("host.accum_limited.kept", kept, n);
  rdgpu_limited_result *dres = st.out("host.accum_limited.result", result, 1);
  limited_device<W>(dd, nodata, dsup, supply_nodata, dcap, dfac, w, h, dout, dkept, nodata_out, dres, nullptr);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_DEFINE_LIMITED(SUF, W)                                                                                                      \
  extern "C" int rdgpu_d8_flow_accum_limited_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const W *supply, W supply_nodata,         \
                                                   const W *capacity, const W *factor, int width, int height, double *out,            \
                                                   double *kept, double nodata_out, rdgpu_limited_result *result) {                   \
    return guarded([&] {                                                                                                               \
      limited_host<W>(dirs, dir_nodata, supply, supply_nodata, capacity, factor, width, height, out, kept, nodata_out, result,        \
                      "rdgpu_d8_flow_accum_limited_" #SUF);                                                                            \
    });                                                                                                                                \
  }                                                                                                                                    \
  extern "C" int rdgpu_d8_flow_accum_limited_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const W *d_supply, W supply_nodata, \
                                                       const W *d_capacity, const W *d_factor, int width, int height, double *d_out,  \
                                                       double *d_kept, double nodata_out, rdgpu_limited_result *d_result,             \
                                                       void *hip_stream) {                                                             \
    return guarded([&] {                                                                                                               \
      al_check_args(d_dirs, d_supply, d_out, d_kept, d_result, width, height, "rdgpu_d8_flow_accum_limited_dev_" #SUF);               \
      limited_device<W>(d_dirs, dir_nodata, d_supply, supply_nodata, d_capacity, d_factor, width, height, d_out, d_kept, nodata_out,  \
                        d_result, (hipStream_t)hip_stream);                                                                            \
    });                                                                                                                                \
  }
RD_DEFINE_LIMITED(f32, float)
RD_DEFINE_LIMITED(f64, double)
#undef RD_DEFINE_LIMITED
