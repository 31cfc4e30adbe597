// mfd_distance_up.hip -- flow distance and rise UP to the sources (the ridge) over D-infinity / MFD proportions.
//
//  * rdgpu_mfd_distance_up[_dev]            any 9-float proportions array (PropsAcc)
//  * rdgpu_dinf_distance_up[_dev]_<T>       D-infinity from a DEM in compact form (DinfAcc, 5 B/cell), elevations the DEM's
//  * rdgpu_dinf_distance_up_flats[_dev]_<T> the same with the cells of drainable flats patched from the flat mask (mfd.hip)
//
// include/rdgpu.h states the definition.  This is the distance engine (mfd_distance.hip) run in the accumulation's
// direction: a cell is final once every DONOR is final.  One uint32 per cell counts the donors still undecided (NoData:
// 0xFFFFFFFF); zero means decided.  A work list holds DECIDED cells.  Its thread decrements the counter of every receiver
// of its cell with a returning agent-scope atomic; the thread that takes a counter to zero is the only one that ever
// computes that receiver: it reads the shares of the eight neighbours towards it and the values of those that are donors,
// combines them in the fixed order m = 1..8, publishes the receiver and continues inline with it.  Further receivers it
// completed in the same step go to the wavefront's LDS stack or to the next launch's list (mfd_worklist.hpp).  Nothing
// waits: a cycle of links leaves its counters above zero, the lists run empty and the finalize gives those cells and
// everything downstream of them out_nodata.
//
// Visibility between workgroups is the down engine's: a cell's values are published with relaxed agent-scope atomic
// stores; the wavefront drains them (s_waitcnt vmcnt(0)) before its next counter decrement; every read of another cell's
// value in the work-list kernels is a relaxed agent-scope atomic load, which bypasses the L1.  A reader only ever looks at
// a donor after the decrement that followed that donor's drain, so it needs no fence.  The output planes themselves hold
// the values while the lists run.
#include "mfd_worklist.hpp"

#include <cmath>

namespace rdgpu {

extern uint32_t g_dist_rounds;   // mfd_distance.hip: rdgpu_mfd_distance_rounds reports the last call of either direction

constexpr uint32_t UP_NODATA = 0xFFFFFFFFu;

struct UpArgs {
  const double *elev;    // nullable unless rise
  double *dist, *rise;   // nullable, not both
  double lx, ly, ld;     // the increment along x, along y, diagonal
  float min_share;       // a link needs a share above it
  int stat;
  int w, h;
};

__device__ __forceinline__ int up_opp(int m) { return m <= 4 ? m + 4 : m - 4; }
__device__ __forceinline__ double up_ld_value(const double *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the share of the link from the neighbour m of (x, y) into (x, y), or 0 where there is no such link: donors are data
// cells off the raster's edge whose share towards the cell is above min_share (min_share >= 0: a link's share is positive)
template <class ACC>
__device__ __forceinline__ float up_link(const ACC &a, const UpArgs &g, int x, int y, int m) {
  const int dx = x + mdx(m), dy = y + mdy(m);
  if (dx < 1 || dy < 1 || dx >= g.w - 1 || dy >= g.h - 1) return 0.0f;
  const uint64_t d = (uint64_t)dy * g.w + dx;
  if (a.nodata(d)) return 0.0f;
  const float p = a.share(d, up_opp(m));
  return p > g.min_share ? p : 0.0f;
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_distup_elev(const T *__restrict__ z, double *__restrict__ e, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) e[c] = (double)z[c];
}

// the donor counters, the zeros of the sources and the flags of the first work list
template <class ACC>
__global__ __launch_bounds__(NTHR) void k_distup_init(ACC a, UpArgs g, uint32_t *cnt, uint8_t *ready) {
  const int w = g.w;
  const uint64_t n = (uint64_t)w * g.h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    uint32_t k = UP_NODATA;
    uint8_t rdy = 0;
    if (!a.nodata(c)) {
      k = 0;
#pragma unroll
      for (int m = 1; m <= 8; m++)
        if (up_link<ACC>(a, g, x, y, m) > 0.0f) k++;
      if (k == 0) {   // a source
        rdy = 1;
        if (g.dist) g.dist[c] = 0.0;
        if (g.rise) g.rise[c] = 0.0;
      }
    }
    cnt[c] = k;
    ready[c] = rdy;
  }
}

// The receiver r, whose last donor has just been decided, by the thread that took its counter to zero.  r may lie on the
// raster's edge: up_link checks the bounds of its neighbours.
template <class ACC>
__device__ __forceinline__ void up_decide(const ACC &a, const UpArgs &g, uint32_t r) {
  const int w = g.w;
  const int x = (int)(r % (uint32_t)w), y = (int)(r / (uint32_t)w);
  float p[8];
#pragma unroll
  for (int m = 1; m <= 8; m++) p[m - 1] = up_link<ACC>(a, g, x, y, m);
  double vd[8], vh[8];
  int ncon = 0;
  const double zr = g.rise ? g.elev[r] : 0.0;
#pragma unroll
  for (int m = 1; m <= 8; m++) {
    vd[m - 1] = 0.0;
    vh[m - 1] = 0.0;
    if (!(p[m - 1] > 0.0f)) continue;
    ncon++;
    const uint64_t d = (uint64_t)(y + mdy(m)) * w + (x + mdx(m));
    if (g.dist) vd[m - 1] = up_ld_value(&g.dist[d]) + ((m == 1 || m == 5) ? g.lx : (m == 3 || m == 7) ? g.ly : g.ld);
    if (g.rise) vh[m - 1] = up_ld_value(&g.rise[d]) + (g.elev[d] - zr);
  }
  double qd = 0.0, qh = 0.0;
  if (g.stat == 0 && ncon > 1) {
    double nd = 0.0, nh = 0.0, den = 0.0;
#pragma unroll
    for (int m = 1; m <= 8; m++) {
      if (!(p[m - 1] > 0.0f)) continue;
      const double pm = (double)p[m - 1];
      nd += pm * vd[m - 1];
      nh += pm * vh[m - 1];
      den += pm;
    }
    qd = nd / den;
    qh = nh / den;
  } else {
    bool first = true;
#pragma unroll
    for (int m = 1; m <= 8; m++) {
      if (!(p[m - 1] > 0.0f)) continue;
      if (first) { qd = vd[m - 1]; qh = vh[m - 1]; first = false; continue; }
      if (g.stat == 1) {
        if (vd[m - 1] < qd) qd = vd[m - 1];
        if (vh[m - 1] < qh) qh = vh[m - 1];
      } else {
        if (vd[m - 1] > qd) qd = vd[m - 1];
        if (vh[m - 1] > qh) qh = vh[m - 1];
      }
    }
  }
  if (g.dist) __hip_atomic_store(&g.dist[r], qd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (g.rise) __hip_atomic_store(&g.rise[r], qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One step for the decided cell c: the counters of its receivers go down; the receivers completed by this thread are
// decided and published.  Returns them as a mask of neighbour numbers (bit n - 1: the neighbour n of c).
template <class ACC>
__device__ __forceinline__ uint32_t up_step(const ACC &a, const UpArgs &g, uint32_t *cnt, uint32_t c) {
  const int w = g.w, h = g.h;
  const int x = (int)(c % (uint32_t)w), y = (int)(c / (uint32_t)w);
  if (x == 0 || y == 0 || x == w - 1 || y == h - 1) return 0;   // a cell on the raster's edge is never a donor
  bool rcv[8];
#pragma unroll
  for (int n = 1; n <= 8; n++)   // the links out of c: a share above min_share into a data cell (c is interior: in bounds)
    rcv[n - 1] = a.share(c, n) > g.min_share && !a.nodata((uint64_t)(y + mdy(n)) * w + (x + mdx(n)));
  // what this wavefront has published so far (the cell c among it, and the cells on its stack) is drained before any counter
  // is decremented: whoever takes a counter to zero afterwards reads final values at the memory side
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t old[8];
#pragma unroll
  for (int n = 1; n <= 8; n++)
    if (rcv[n - 1])
      old[n - 1] = __hip_atomic_fetch_sub(&cnt[(uint64_t)(y + mdy(n)) * w + (x + mdx(n))], 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
  uint32_t done = 0;
#pragma unroll
  for (int n = 1; n <= 8; n++)
    if (rcv[n - 1] && old[n - 1] == 1u) done |= 1u << (n - 1);
  for (uint32_t rest = done; rest;) {
    const int n = __builtin_ctz(rest) + 1;
    rest &= rest - 1u;
    up_decide<ACC>(a, g, (uint32_t)(y + mdy(n)) * (uint32_t)w + (uint32_t)(x + mdx(n)));
  }
  return done;
}

// the work list's step (mfd_worklist.hpp); the step itself never reads c's values, the thread that decides a receiver does
template <class ACC>
struct UpStep {
  ACC a;
  UpArgs g;
  uint32_t *cnt;
  __device__ __forceinline__ int width() const { return g.w; }
  __device__ __forceinline__ uint32_t operator()(uint32_t c, bool) const { return up_step<ACC>(a, g, cnt, c); }
};

__global__ __launch_bounds__(NTHR) void k_distup_finalize(const uint32_t *__restrict__ cnt, double *dist, double *rise,
                                                          double out_nodata, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride)
    if (cnt[c] != 0u) {   // undecided (a counter above zero) and NoData cells
      if (dist) dist[c] = out_nodata;
      if (rise) rise[c] = out_nodata;
    }
}

struct UpParams {
  int stat;
  float min_share;
  double cell_x, cell_y;
};

// in: the proportions or the DEM
static void check_up_args(const char *who, const void *in, int w, int h, bool have_elev, int stat, float min_share, double cx,
                          double cy, const void *dist, const void *rise, uint64_t max_cells = 0xFFFF0000ull) {
  if (!in) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_dims(w, h, who, max_cells);
  if (!dist && !rise) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  if (rise && !have_elev) throw Error(RDGPU_ERR_ARG, std::string(who) + ": rise needs the elevations");
  if (stat < 0 || stat > 2) throw Error(RDGPU_ERR_ARG, std::string(who) + ": stat must be 0 (average), 1 (minimum) or 2 (maximum)");
  if (!std::isfinite(min_share) || min_share < 0) throw Error(RDGPU_ERR_ARG, std::string(who) + ": min_share must be finite and >= 0");
  if (!std::isfinite(cx) || !std::isfinite(cy) || cx == 0 || cy == 0)
    throw Error(RDGPU_ERR_ARG, std::string(who) + ": cell sizes must be finite and non-zero");
}

// The scratch planes are the accumulation's (same sizes, never in use at the same time: one call per device at a time).
template <class ACC>
static void mfd_distance_up(ACC a, int w, int h, const double *d_elev, const UpParams &pr, double *d_dist, double *d_rise,
                            double out_nodata, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  uint32_t *cnt = ws.buf<uint32_t>("mfd.pending", n);
  uint8_t *ready = ws.buf<uint8_t>("mfd.ready", n);
  UpArgs g;
  g.elev = d_rise ? d_elev : nullptr;
  g.dist = d_dist;
  g.rise = d_rise;
  g.lx = std::fabs(pr.cell_x);
  g.ly = std::fabs(pr.cell_y);
  g.ld = std::sqrt(g.lx * g.lx + g.ly * g.ly);
  g.min_share = pr.min_share;
  g.stat = pr.stat;
  g.w = w;
  g.h = h;
  g_dist_rounds = 0;
  RD_LAUNCH("mfddistup.init", (k_distup_init<ACC>), dim3(sgrid(n)), dim3(NTHR), 0, s, a, g, cnt, ready);
  // the distance engines' switch between the two work-list kernels (mfd_distance.hip says how it was chosen)
  const char *se = getenv("RDGPU_MFD_DISTANCE_STACK_BELOW");
  const uint32_t stack_below = se ? (uint32_t)strtoul(se, nullptr, 10) : (1u << 22);
  g_dist_rounds = worklist_run(ready, n, UpStep<ACC>{a, g, cnt}, "mfddistup.round", "mfddistup.stack", stack_below,
                               "rdgpu mfd distance up did not terminate", s);
  RD_LAUNCH("mfddistup.finalize", k_distup_finalize, dim3(sgrid(n)), dim3(NTHR), 0, s, (const uint32_t *)cnt, d_dist, d_rise,
            out_nodata, n);
}

// the elevations of a DEM as doubles (exact for every element type); a float64 DEM is used as it is
template <class T>
static const double *up_elev_plane(const T *d_z, uint64_t n, hipStream_t s) {
  if constexpr (std::is_same<T, double>::value) return d_z;
  else {
    double *e = Workspace::get().buf<double>("mfddist.elev", n);
    RD_LAUNCH("mfddistup.elev", (k_distup_elev<T>), dim3(sgrid(n)), dim3(NTHR), 0, s, d_z, e, n);
    return e;
  }
}

// the proportions from the DEM (tarboton: with or without the flats patched), then the distances
template <class T>
static void dinf_distance_up(TarbotonFn<T> tarboton, const T *d_dem, T nodata, int w, int h, const UpParams &pr, double *d_dist,
                             double *d_rise, double out_nodata, hipStream_t s) {
  const DinfAcc a = tarboton(d_dem, nodata, w, h, s);
  const double *e = d_rise ? up_elev_plane<T>(d_dem, (uint64_t)w * h, s) : nullptr;
  mfd_distance_up<DinfAcc>(a, w, h, e, pr, d_dist, d_rise, out_nodata, s);
}

}  // namespace rdgpu

using namespace rdgpu;

extern "C" int rdgpu_mfd_distance_up_dev(const float *d_props9, int w, int h, const double *d_elev, int stat, float min_share,
                                         double cell_x, double cell_y, double *d_dist, double *d_rise, double out_nodata,
                                         void *st) {
  return guarded([&] {
    check_up_args("rdgpu_mfd_distance_up", d_props9, w, h, d_elev != nullptr, stat, min_share, cell_x, cell_y, d_dist, d_rise);
    mfd_distance_up<PropsAcc>(PropsAcc{d_props9}, w, h, d_elev, UpParams{stat, min_share, cell_x, cell_y}, d_dist, d_rise,
                              out_nodata, (hipStream_t)st);
  });
}
extern "C" int rdgpu_mfd_distance_up(const float *props9, int w, int h, const double *elev, int stat, float min_share,
                                     double cell_x, double cell_y, double *dist, double *rise, double out_nodata) {
  return guarded([&] {
    check_up_args("rdgpu_mfd_distance_up", props9, w, h, elev != nullptr, stat, min_share, cell_x, cell_y, dist, rise);
    const size_t n = (size_t)w * h;
    HostStage hs;
    const float *dp = hs.in("host.props", props9, n * 9);
    const double *de = hs.in("host.mfddist.elev", rise ? elev : nullptr, n);   // (read for the rise only)
    double *dd = hs.out("host.mfddist.dist", dist, n), *dr = hs.out("host.mfddist.drop", rise, n);
    mfd_distance_up<PropsAcc>(PropsAcc{dp}, w, h, de, UpParams{stat, min_share, cell_x, cell_y}, dd, dr, out_nodata, nullptr);
    hs.finish();
  });
}

#define RD_DINF_DISTUP_API(FL, ACCESSOR, MAXC, SUF, T)                                                                    \
  extern "C" int rdgpu_dinf_distance_up##FL##_dev_##SUF(const T *d_dem, T nodata, int w, int h, int stat, float min_share, \
                                                        double cell_x, double cell_y, double *d_dist, double *d_rise,     \
                                                        double out_nodata, void *st) {                                    \
    return guarded([&] {                                                                                                  \
      check_up_args("rdgpu_dinf_distance_up" #FL, d_dem, w, h, true, stat, min_share, cell_x, cell_y, d_dist, d_rise, MAXC); \
      dinf_distance_up<T>(ACCESSOR<T>, d_dem, nodata, w, h, UpParams{stat, min_share, cell_x, cell_y}, d_dist, d_rise,    \
                          out_nodata, (hipStream_t)st);                                                                   \
    });                                                                                                                   \
  }                                                                                                                       \
  extern "C" int rdgpu_dinf_distance_up##FL##_##SUF(const T *dem, T nodata, int w, int h, int stat, float min_share,      \
                                                    double cell_x, double cell_y, double *dist, double *rise,             \
                                                    double out_nodata) {                                                  \
    return guarded([&] {                                                                                                  \
      check_up_args("rdgpu_dinf_distance_up" #FL, dem, w, h, true, stat, min_share, cell_x, cell_y, dist, rise, MAXC);    \
      const size_t n = (size_t)w * h;                                                                                     \
      HostStage hs;                                                                                                       \
      const T *d = hs.in("host.dem", dem, n);                                                                             \
      double *dd = hs.out("host.mfddist.dist", dist, n), *dr = hs.out("host.mfddist.drop", rise, n);                      \
      dinf_distance_up<T>(ACCESSOR<T>, d, nodata, w, h, UpParams{stat, min_share, cell_x, cell_y}, dd, dr, out_nodata, nullptr); \
      hs.finish();                                                                                                        \
    });                                                                                                                   \
  }
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, u8, uint8_t)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u8, uint8_t)
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, i16, int16_t)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i16, int16_t)
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, u16, uint16_t)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u16, uint16_t)
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, i32, int32_t)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i32, int32_t)
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, u32, uint32_t)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u32, uint32_t)
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, f32, float)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, f32, float)
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, f64, double)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, f64, double)
RD_DINF_DISTUP_API(, tarboton_device, 0xFFFF0000ull, i8, int8_t)
RD_DINF_DISTUP_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i8, int8_t)
