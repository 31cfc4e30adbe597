// mfd_reverse.hip -- reverse accumulation, largest weight downslope and upslope dependence over D-infinity / MFD
// proportions: a quantity summed or maximised over everything that lies DOWNSLOPE of a cell, weighted by the shares
// (the transpose of the accumulation; TauDEM's DinfRevAccum and DinfUpDependence are the products meant).
//
//  * rdgpu_mfd_reverse_accum[_dev]              any 9-float proportions array (PropsAcc)
//  * rdgpu_dinf_reverse_accum[_dev]_<T>         D-infinity from a DEM in compact form (DinfAcc, 5 B/cell)
//  * rdgpu_dinf_reverse_accum_flats[_dev]_<T>   the same with the cells of drainable flats patched from the flat mask (mfd.hip)
//
// include/rdgpu.h states the definition.  The graph and the direction are those of mfd_distance.hip: a cell is decided
// once every receiver is decided.  One uint32 per cell is counter and state at once: the number of receivers still
// undecided while the cell waits (1..8), afterwards RV_RESOLVED (decided, has a maximum) or RV_EMPTY (decided, no
// contributing weight at or below it), RV_NODATA off the data.  Where wmax is not requested the distinction is not kept:
// every decided cell is RV_RESOLVED and no thread reads a receiver's state.  A work list holds DECIDED cells.  Its thread
// decrements the counter of every donor of its cell with a returning agent-scope atomic; the thread that takes a counter
// to zero is the only one that ever computes that donor: it reads the values (and states) of the donor's receivers,
// combines them in the fixed order n = 1..8, publishes the donor and continues inline with it (mfd_worklist.hpp).
// Nothing waits: a cycle of positive shares leaves its counters above zero, the lists run empty and the finalize gives
// those cells out_nodata.
//
// Visibility between workgroups is mfd_distance.hip's: a cell's values and then its state are published with
// relaxed agent-scope atomic stores; the wavefront drains them (s_waitcnt vmcnt(0)) before its next counter decrement;
// every read of another cell's state or value in the work-list kernels is a relaxed agent-scope atomic load, which
// bypasses the L1.  The read-only inputs (proportions, weights, mask) are read plainly.  The output planes themselves
// hold the values while the lists run.
#include "mfd_worklist.hpp"

namespace rdgpu {

extern uint32_t g_dist_rounds;   // mfd_distance.hip: rdgpu_mfd_distance_rounds reports the last call of any of the three engines

constexpr uint32_t RV_NODATA = 0xFFFFFFFFu, RV_RESOLVED = 0xFFFFFFFEu, RV_EMPTY = 0xFFFFFFFDu;

struct RevArgs {
  const uint8_t *dest;   // nullable: absorbing cells
  const double *wgt;     // nullable: then dest is given and the weight is 1.0 on absorbing cells, 0.0 elsewhere
  double wnd;            // the weights' NoData value (a NaN: none)
  double *racc, *wmax;   // nullable, not both; wmax only with wgt
  int w, h;
};

__device__ __forceinline__ uint32_t rv_ld_state(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double rv_ld_value(const double *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the weight of the data cell c and whether it contributes
__device__ __forceinline__ bool rv_weight(const RevArgs &g, uint64_t c, double &wc) {
  if (!g.wgt) {
    wc = g.dest[c] != 0 ? 1.0 : 0.0;
    return true;
  }
  wc = g.wgt[c];
  return !(wc == g.wnd) && !(wc != wc);
}

// counters, the final values and state of the cells with R(c) empty (edge cells, absorbing cells, cells without
// receivers), and the flags of the first work list
template <class ACC>
__global__ __launch_bounds__(NTHR) void k_rev_init(ACC a, RevArgs g, uint32_t *st, uint8_t *ready) {
  const int w = g.w, h = g.h;
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    uint32_t s = RV_NODATA;
    uint8_t rdy = 0;
    if (!a.nodata(c)) {
      uint32_t k = 0;
      const bool absorbing = g.dest && g.dest[c] != 0;
      if (!absorbing && x >= 1 && y >= 1 && x < w - 1 && y < h - 1) {   // a cell on the raster's edge has no receivers
#pragma unroll
        for (int m = 1; m <= 8; m++)
          if (a.share(c, m) > 0 && !a.nodata((uint64_t)(y + mdy(m)) * w + (x + mdx(m)))) k++;
      }
      if (k == 0) {
        double wc;
        const bool con = rv_weight(g, c, wc);
        if (g.racc) g.racc[c] = con ? wc : 0.0;
        if (g.wmax && con) g.wmax[c] = wc;
        s = (con || !g.wmax) ? RV_RESOLVED : RV_EMPTY;
        rdy = 1;
      } else s = k;
    }
    st[c] = s;
    ready[c] = rdy;
  }
}

// The donor d, whose last receiver has just been decided, by the thread that took its counter to zero.
template <class ACC>
__device__ __forceinline__ void rev_decide(const ACC &a, const RevArgs &g, uint32_t *st, uint32_t d) {
  const int w = g.w;
  const int x = (int)(d % (uint32_t)w), y = (int)(d / (uint32_t)w);   // interior
  float p[8];
  bool rec[8];
#pragma unroll
  for (int n = 1; n <= 8; n++) p[n - 1] = a.share(d, n);
#pragma unroll
  for (int n = 1; n <= 8; n++) rec[n - 1] = p[n - 1] > 0 && !a.nodata((uint64_t)(y + mdy(n)) * w + (x + mdx(n)));
  uint32_t rs[8];
  double va[8], vm[8];
#pragma unroll
  for (int n = 1; n <= 8; n++) {   // all loads in flight together
    const uint64_t r = (uint64_t)(y + mdy(n)) * w + (x + mdx(n));
    rs[n - 1] = RV_NODATA;
    va[n - 1] = 0.0;
    if (!rec[n - 1]) continue;
    vm[n - 1] = 0.0;
    if (!rec[n - 1]) continue;
    if (g.racc) va[n - 1] = rv_ld_value(&g.racc[r]);
    if (g.wmax) {   // (the value of an RV_EMPTY receiver is not yet written and is not used)
      rs[n - 1] = rv_ld_state(&st[r]);
      vm[n - 1] = rv_ld_value(&g.wmax[r]);
    }
  }
  double wc;
  const bool con = rv_weight(g, d, wc);
  bool has = con;
  if (g.racc) {
    double S = con ? wc : 0.0;
#pragma unroll
    for (int n = 1; n <= 8; n++)
      if (rec[n - 1]) S = S + (double)p[n - 1] * va[n - 1];
    __hip_atomic_store(&g.racc[d], S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (g.wmax) {
    double M = wc;
#pragma unroll
    for (int n = 1; n <= 8; n++) {
      if (rs[n - 1] != RV_RESOLVED) continue;
      if (!has || vm[n - 1] > M) {
        M = vm[n - 1];
        has = true;
      }
    }
    if (has) __hip_atomic_store(&g.wmax[d], M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else has = true;
  __hip_atomic_store(&st[d], has ? RV_RESOLVED : RV_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One step for the decided cell c: the counters of its donors go down; the donors completed by this thread are decided
// and published.  Returns them as a mask of neighbour numbers (bit m - 1: the neighbour m of c).
template <class ACC>
__device__ __forceinline__ uint32_t rev_step(const ACC &a, const RevArgs &g, uint32_t *st, uint32_t c) {
  const int w = g.w, h = g.h;
  const int x = (int)(c % (uint32_t)w), y = (int)(c / (uint32_t)w);
  bool don[8];
#pragma unroll
  for (int m = 1; m <= 8; m++) {   // the donors: interior, non-absorbing data cells with a positive share towards c
    const int dx = x + mdx(m), dy = y + mdy(m);
    bool is = false;
    if (dx >= 1 && dy >= 1 && dx < w - 1 && dy < h - 1) {
      const uint64_t d = (uint64_t)dy * w + dx;
      is = !a.nodata(d) && a.share(d, m <= 4 ? m + 4 : m - 4) > 0 && !(g.dest && g.dest[d] != 0);
    }
    don[m - 1] = is;
  }
  // what this wavefront has published so far (the cell c among it, and the cells on its stack) is drained before any counter
  // is decremented: whoever takes a counter to zero afterwards reads final states and values at the memory side
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t old[8];
#pragma unroll
  for (int m = 1; m <= 8; m++)
    if (don[m - 1])
      old[m - 1] = __hip_atomic_fetch_sub(&st[(uint64_t)(y + mdy(m)) * w + (x + mdx(m))], 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
  uint32_t done = 0;
#pragma unroll
  for (int m = 1; m <= 8; m++)
    if (don[m - 1] && old[m - 1] == 1u) done |= 1u << (m - 1);
  for (uint32_t rest = done; rest;) {
    const int m = __builtin_ctz(rest) + 1;
    rest &= rest - 1u;
    rev_decide<ACC>(a, g, st, (uint32_t)(y + mdy(m)) * (uint32_t)w + (uint32_t)(x + mdx(m)));
  }
  return done;
}

// the work list's step (mfd_worklist.hpp)
template <class ACC>
struct RevStep {
  ACC a;
  RevArgs g;
  uint32_t *st;
  __device__ __forceinline__ int width() const { return g.w; }
  __device__ __forceinline__ uint32_t operator()(uint32_t c, bool) const { return rev_step<ACC>(a, g, st, c); }
};

__global__ __launch_bounds__(NTHR) void k_rev_finalize(const uint32_t *__restrict__ st, double *racc, double *wmax,
                                                       double out_nodata, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t s = st[c];
    if (s == RV_RESOLVED) continue;
    if (racc && s != RV_EMPTY) racc[c] = out_nodata;   // undecided (a counter above zero) and NoData cells
    if (wmax) wmax[c] = out_nodata;                    // those, and decided cells without a maximum
  }
}

// in: the proportions or the DEM
static void check_args(const char *who, const void *in, int w, int h, const void *weights, const void *dest, const void *racc,
                       const void *wmax, uint64_t max_cells = 0xFFFF0000ull) {
  if (!in) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_dims(w, h, who, max_cells);
  if (!racc && !wmax) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  if (wmax && !weights) throw Error(RDGPU_ERR_ARG, std::string(who) + ": wmax needs the weights");
  if (!weights && !dest) throw Error(RDGPU_ERR_ARG, std::string(who) + ": neither weights nor dest given");
}

// The scratch planes are the accumulation's (same sizes, never in use at the same time: one call per device at a time).
template <class ACC>
static void mfd_reverse(ACC a, int w, int h, const double *d_wgt, double wnd, const uint8_t *d_dest, double *d_racc, double *d_wmax,
                        double out_nodata, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  uint32_t *st = ws.buf<uint32_t>("mfd.pending", n);
  uint8_t *ready = ws.buf<uint8_t>("mfd.ready", n);
  RevArgs g;
  g.dest = d_dest;
  g.wgt = d_wgt;
  g.wnd = wnd;
  g.racc = d_racc;
  g.wmax = d_wmax;
  g.w = w;
  g.h = h;
  g_dist_rounds = 0;
  RD_LAUNCH("mfdrev.init", (k_rev_init<ACC>), dim3(sgrid(n)), dim3(NTHR), 0, s, a, g, st, ready);
  // the switch between the buffer kernel and the stack kernel is the distance engines' (mfd_distance.hip says why)
  const char *se = getenv("RDGPU_MFD_DISTANCE_STACK_BELOW");
  const uint32_t stack_below = se ? (uint32_t)strtoul(se, nullptr, 10) : (1u << 22);
  g_dist_rounds = worklist_run(ready, n, RevStep<ACC>{a, g, st}, "mfdrev.round", "mfdrev.stack", stack_below,
                               "rdgpu mfd reverse accumulation did not terminate", s);
  RD_LAUNCH("mfdrev.finalize", k_rev_finalize, dim3(sgrid(n)), dim3(NTHR), 0, s, (const uint32_t *)st, d_racc, d_wmax, out_nodata,
            n);
}

// the proportions from the DEM (tarboton: with or without the flats patched), then the engine
template <class T>
static void dinf_reverse(TarbotonFn<T> tarboton, const T *d_dem, T nodata, int w, int h, const double *d_wgt, double wnd,
                         const uint8_t *d_dest, double *d_racc, double *d_wmax, double out_nodata, hipStream_t s) {
  const DinfAcc a = tarboton(d_dem, nodata, w, h, s);
  mfd_reverse<DinfAcc>(a, w, h, d_wgt, wnd, d_dest, d_racc, d_wmax, out_nodata, s);
}

}  // namespace rdgpu

using namespace rdgpu;

extern "C" int rdgpu_mfd_reverse_accum_dev(const float *d_props9, int w, int h, const double *d_weights, double weight_nodata,
                                           const uint8_t *d_dest, double *d_racc, double *d_wmax, double out_nodata, void *st) {
  return guarded([&] {
    check_args("rdgpu_mfd_reverse_accum", d_props9, w, h, d_weights, d_dest, d_racc, d_wmax);
    mfd_reverse<PropsAcc>(PropsAcc{d_props9}, w, h, d_weights, weight_nodata, d_dest, d_racc, d_wmax, out_nodata, (hipStream_t)st);
  });
}
extern "C" int rdgpu_mfd_reverse_accum(const float *props9, int w, int h, const double *weights, double weight_nodata,
                                       const uint8_t *dest, double *racc, double *wmax, double out_nodata) {
  return guarded([&] {
    check_args("rdgpu_mfd_reverse_accum", props9, w, h, weights, dest, racc, wmax);
    const size_t n = (size_t)w * h;
    HostStage hs;
    const float *dp = hs.in("host.props", props9, n * 9);
    const double *dw = hs.in("host.mfdrev.weights", weights, n);
    const uint8_t *dd = hs.in("host.mfdrev.dest", dest, n);
    double *da = hs.out("host.mfdrev.racc", racc, n), *dm = hs.out("host.mfdrev.wmax", wmax, n);
    mfd_reverse<PropsAcc>(PropsAcc{dp}, w, h, dw, weight_nodata, dd, da, dm, out_nodata, nullptr);
    hs.finish();
  });
}

#define RD_DINF_REV_API(FL, ACCESSOR, MAXC, SUF, T)                                                                       \
  extern "C" int rdgpu_dinf_reverse_accum##FL##_dev_##SUF(const T *d_dem, T nodata, int w, int h, const double *d_weights, \
                                                          double weight_nodata, const uint8_t *d_dest, double *d_racc,    \
                                                          double *d_wmax, double out_nodata, void *st) {                  \
    return guarded([&] {                                                                                                  \
      check_args("rdgpu_dinf_reverse_accum" #FL, d_dem, w, h, d_weights, d_dest, d_racc, d_wmax, MAXC);                   \
      dinf_reverse<T>(ACCESSOR<T>, d_dem, nodata, w, h, d_weights, weight_nodata, d_dest, d_racc, d_wmax, out_nodata,     \
                      (hipStream_t)st);                                                                                   \
    });                                                                                                                   \
  }                                                                                                                       \
  extern "C" int rdgpu_dinf_reverse_accum##FL##_##SUF(const T *dem, T nodata, int w, int h, const double *weights,        \
                                                      double weight_nodata, const uint8_t *dest, double *racc, double *wmax, \
                                                      double out_nodata) {                                                \
    return guarded([&] {                                                                                                  \
      check_args("rdgpu_dinf_reverse_accum" #FL, dem, w, h, weights, dest, racc, wmax, MAXC);                             \
      const size_t n = (size_t)w * h;                                                                                     \
      HostStage hs;                                                                                                       \
      const T *d = hs.in("host.dem", dem, n);                                                                             \
      const double *dw = hs.in("host.mfdrev.weights", weights, n);                                                        \
      const uint8_t *dd = hs.in("host.mfdrev.dest", dest, n);                                                             \
      double *da = hs.out("host.mfdrev.racc", racc, n), *dm = hs.out("host.mfdrev.wmax", wmax, n);                        \
      dinf_reverse<T>(ACCESSOR<T>, d, nodata, w, h, dw, weight_nodata, dd, da, dm, out_nodata, nullptr);                  \
      hs.finish();                                                                                                        \
    });                                                                                                                   \
  }
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, u8, uint8_t)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u8, uint8_t)
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, i16, int16_t)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i16, int16_t)
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, u16, uint16_t)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u16, uint16_t)
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, i32, int32_t)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i32, int32_t)
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, u32, uint32_t)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u32, uint32_t)
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, f32, float)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, f32, float)
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, f64, double)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, f64, double)
RD_DINF_REV_API(, tarboton_device, 0xFFFF0000ull, i8, int8_t)
RD_DINF_REV_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i8, int8_t)
