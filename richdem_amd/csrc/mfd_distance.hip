// mfd_distance.hip -- flow distance and drop (HAND) DOWN to the stop cells over D-infinity / MFD proportions.
//
//  * rdgpu_mfd_distance_down[_dev]          any 9-float proportions array (PropsAcc)
//  * rdgpu_dinf_distance_down[_dev]_<T>     D-infinity from a DEM in compact form (DinfAcc, 5 B/cell), elevations the DEM's
//  * rdgpu_dinf_distance_down_flats[_dev]_<T>  the same with the cells of drainable flats patched from the flat mask (mfd.hip)
//  * rdgpu_mfd_distance_rounds              work-list launches of the last call
//
// include/rdgpu.h states the definition.  The graph is the accumulation's (mfd.hip) run the other way: a cell is final
// once every receiver is final.  One uint32 per cell is counter and state at once: the number of receivers still
// undecided while the cell waits (1..8), afterwards ST_RESOLVED or ST_DEAD, ST_NODATA off the data.  A work list holds
// DECIDED cells.  Its thread decrements the counter of every donor of its cell with a returning agent-scope atomic; the
// thread that takes a counter to zero is the only one that ever computes that donor: it reads the state and the values
// of the donor's receivers, combines them in the fixed order n = 1..8, publishes the donor and continues inline with
// it.  Further donors it completed in the same step go to the wavefront's LDS stack or to the next launch's list: the
// work list is the accumulation's (mfd_worklist.hpp).  Nothing waits: a cycle of positive shares leaves its counters
// above zero, the lists run empty and the finalize gives those cells out_nodata.
//
// Visibility between workgroups (per-XCD L2s are not coherent, a CU's L1 is never refreshed by another CU's stores): a
// cell's values and state are published with relaxed agent-scope atomic stores (write-through, at most 8 B each); the
// wavefront drains them (s_waitcnt vmcnt(0)) before its next counter decrement; every read of another cell's state or
// value in the work-list kernels is a relaxed agent-scope atomic load, which bypasses the L1.  A reader only ever looks
// at a cell after the decrement that followed that cell's drain, so it needs no fence.  The output planes themselves
// hold the values while the lists run.
#include "mfd_worklist.hpp"

#include <cmath>

namespace rdgpu {

constexpr uint32_t ST_NODATA = 0xFFFFFFFFu, ST_RESOLVED = 0xFFFFFFFEu, ST_DEAD = 0xFFFFFFFDu;

struct DistArgs {
  const uint8_t *chan;   // nullable: stop cells are the cells without receivers
  const double *elev;    // nullable unless drop
  double *dist, *drop;   // nullable, not both
  double lx, ly, ld;     // the increment along x, along y, diagonal
  int stat, strict;
  int w, h;
};

__device__ __forceinline__ uint32_t ld_state(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_value(const double *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_dist_elev(const T *__restrict__ z, double *__restrict__ e, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) e[c] = (double)z[c];
}

// counters, the final state of stop cells and of cells without receivers, and the flags of the first work list
template <class ACC>
__global__ __launch_bounds__(NTHR) void k_dist_init(ACC a, DistArgs g, uint32_t *st, uint8_t *ready) {
  const int w = g.w, h = g.h;
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    uint32_t s = ST_NODATA;
    uint8_t rdy = 0;
    if (!a.nodata(c)) {
      uint32_t k = 0;
      if (x >= 1 && y >= 1 && x < w - 1 && y < h - 1) {   // a cell on the raster's edge has no receivers
#pragma unroll
        for (int m = 1; m <= 8; m++)
          if (a.share(c, m) > 0 && !a.nodata((uint64_t)(y + mdy(m)) * w + (x + mdx(m)))) k++;
      }
      const bool stop = g.chan ? g.chan[c] != 0 : k == 0;
      if (stop) {
        s = ST_RESOLVED;
        if (g.dist) g.dist[c] = 0.0;
        if (g.drop) g.drop[c] = 0.0;
      } else s = k ? k : ST_DEAD;
      rdy = k == 0 || stop;
    }
    st[c] = s;
    ready[c] = rdy;
  }
}

// The donor d, whose last receiver has just been decided, by the thread that took its counter to zero.
template <class ACC>
__device__ __forceinline__ void dist_decide(const ACC &a, const DistArgs &g, uint32_t *st, uint32_t d) {
  const int w = g.w;
  const int x = (int)(d % (uint32_t)w), y = (int)(d / (uint32_t)w);   // interior
  float p[8];
  uint32_t rs[8];
#pragma unroll
  for (int n = 1; n <= 8; n++) p[n - 1] = a.share(d, n);
#pragma unroll
  for (int n = 1; n <= 8; n++) {
    const uint64_t r = (uint64_t)(y + mdy(n)) * w + (x + mdx(n));
    rs[n - 1] = (p[n - 1] > 0 && !a.nodata(r)) ? ld_state(&st[r]) : ST_NODATA;
  }
  double vd[8], vh[8];
  int nrec = 0, ncon = 0;
  const double zd = g.drop ? g.elev[d] : 0.0;
#pragma unroll
  for (int n = 1; n <= 8; n++) {
    vd[n - 1] = 0.0;
    vh[n - 1] = 0.0;
    if (rs[n - 1] == ST_NODATA) continue;
    nrec++;
    if (rs[n - 1] != ST_RESOLVED) continue;
    ncon++;
    const uint64_t r = (uint64_t)(y + mdy(n)) * w + (x + mdx(n));
    if (g.dist) vd[n - 1] = ld_value(&g.dist[r]) + ((n == 1 || n == 5) ? g.lx : (n == 3 || n == 7) ? g.ly : g.ld);
    if (g.drop) vh[n - 1] = ld_value(&g.drop[r]) + (zd - g.elev[r]);
  }
  const bool resolved = g.strict ? ncon == nrec : ncon >= 1;
  if (resolved) {
    double qd = 0.0, qh = 0.0;
    if (g.stat == 0 && ncon > 1) {
      double nd = 0.0, nh = 0.0, den = 0.0;
#pragma unroll
      for (int n = 1; n <= 8; n++) {
        if (rs[n - 1] != ST_RESOLVED) continue;
        const double pn = (double)p[n - 1];
        nd += pn * vd[n - 1];
        nh += pn * vh[n - 1];
        den += pn;
      }
      qd = nd / den;
      qh = nh / den;
    } else {
      bool first = true;
#pragma unroll
      for (int n = 1; n <= 8; n++) {
        if (rs[n - 1] != ST_RESOLVED) continue;
        if (first) { qd = vd[n - 1]; qh = vh[n - 1]; first = false; continue; }
        if (g.stat == 1) {
          if (vd[n - 1] < qd) qd = vd[n - 1];
          if (vh[n - 1] < qh) qh = vh[n - 1];
        } else {
          if (vd[n - 1] > qd) qd = vd[n - 1];
          if (vh[n - 1] > qh) qh = vh[n - 1];
        }
      }
    }
    if (g.dist) __hip_atomic_store(&g.dist[d], qd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g.drop) __hip_atomic_store(&g.drop[d], qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(&st[d], resolved ? ST_RESOLVED : ST_DEAD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One step for the decided cell c: the counters of its donors go down; the donors completed by this thread are decided
// and published.  Returns them as a mask of neighbour numbers (bit m - 1: the neighbour m of c).
template <class ACC>
__device__ __forceinline__ uint32_t dist_step(const ACC &a, const DistArgs &g, uint32_t *st, uint32_t c) {
  const int w = g.w, h = g.h;
  const int x = (int)(c % (uint32_t)w), y = (int)(c / (uint32_t)w);
  bool don[8];
#pragma unroll
  for (int m = 1; m <= 8; m++) {   // the donors: interior, non-stop data cells with a positive share towards c
    const int dx = x + mdx(m), dy = y + mdy(m);
    bool is = false;
    if (dx >= 1 && dy >= 1 && dx < w - 1 && dy < h - 1) {
      const uint64_t d = (uint64_t)dy * w + dx;
      is = !a.nodata(d) && a.share(d, m <= 4 ? m + 4 : m - 4) > 0 && !(g.chan && g.chan[d] != 0);
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
    dist_decide<ACC>(a, g, st, (uint32_t)(y + mdy(m)) * (uint32_t)w + (uint32_t)(x + mdx(m)));
  }
  return done;
}

// the work list's step (mfd_worklist.hpp); a cell's state and values are read at the memory side wherever it comes from
template <class ACC>
struct DistStep {
  ACC a;
  DistArgs g;
  uint32_t *st;
  __device__ __forceinline__ int width() const { return g.w; }
  __device__ __forceinline__ uint32_t operator()(uint32_t c, bool) const { return dist_step<ACC>(a, g, st, c); }
};

__global__ __launch_bounds__(NTHR) void k_dist_finalize(const uint32_t *__restrict__ st, double *dist, double *drop,
                                                        double out_nodata, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride)
    if (st[c] != ST_RESOLVED) {   // DEAD, undecided (a counter above zero) and NoData cells
      if (dist) dist[c] = out_nodata;
      if (drop) drop[c] = out_nodata;
    }
}

uint32_t g_dist_rounds = 0;   // mfd_distance_up.hip sets it too: the last call of either direction

struct DistParams {
  int stat, strict;
  double cell_x, cell_y;
};

// in: the proportions or the DEM
static void check_args(const char *who, const void *in, int w, int h, bool have_elev, int stat, double cx, double cy, const void *dist,
                       const void *drop, uint64_t max_cells = 0xFFFF0000ull) {
  if (!in) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_dims(w, h, who, max_cells);
  if (!dist && !drop) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  if (drop && !have_elev) throw Error(RDGPU_ERR_ARG, std::string(who) + ": drop needs the elevations");
  if (stat < 0 || stat > 2) throw Error(RDGPU_ERR_ARG, std::string(who) + ": stat must be 0 (average), 1 (minimum) or 2 (maximum)");
  if (!std::isfinite(cx) || !std::isfinite(cy) || cx == 0 || cy == 0)
    throw Error(RDGPU_ERR_ARG, std::string(who) + ": cell sizes must be finite and non-zero");
}

// The scratch planes are the accumulation's (same sizes, never in use at the same time: one call per device at a time).
template <class ACC>
static void mfd_distance(ACC a, int w, int h, const uint8_t *d_chan, const double *d_elev, const DistParams &pr, double *d_dist,
                         double *d_drop, double out_nodata, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  uint32_t *st = ws.buf<uint32_t>("mfd.pending", n);
  uint8_t *ready = ws.buf<uint8_t>("mfd.ready", n);
  DistArgs g;
  g.chan = d_chan;
  g.elev = d_drop ? d_elev : nullptr;
  g.dist = d_dist;
  g.drop = d_drop;
  g.lx = std::fabs(pr.cell_x);
  g.ly = std::fabs(pr.cell_y);
  g.ld = std::sqrt(g.lx * g.lx + g.ly * g.ly);
  g.stat = pr.stat;
  g.strict = pr.strict != 0;
  g.w = w;
  g.h = h;
  g_dist_rounds = 0;
  RD_LAUNCH("mfddist.init", (k_dist_init<ACC>), dim3(sgrid(n)), dim3(NTHR), 0, s, a, g, st, ready);
  // Long lists go through the buffer kernel (their by-products are processed next launch, densely packed), short ones through
  // the stack kernel, which finishes what is reachable from its list in one launch.  RDGPU_MFD_DISTANCE_STACK_BELOW sets the
  // list length of the switch (0: never the stack; 4294967295: always).  Where every cell drains, channels at >= 100 cells
  // (dist + drop; ms at 6000^2 / 16000^2 / 40000^2): never 77 / 261 / 1103, 2^20 16.5 / 132 / 858, 2^22 16.5 / 112 / 797,
  // 2^24 38 / 118 / 746, 2^26 38 / 116 / 795-810, always 38 / 271 / 1696 -- a first list of stop cells that goes to the stack
  // kernel, and any wavefront that works off its own by-products, runs at a few active lanes.
  const char *se = getenv("RDGPU_MFD_DISTANCE_STACK_BELOW");
  const uint32_t stack_below = se ? (uint32_t)strtoul(se, nullptr, 10) : (1u << 22);
  g_dist_rounds = worklist_run(ready, n, DistStep<ACC>{a, g, st}, "mfddist.round", "mfddist.stack", stack_below,
                               "rdgpu mfd distance did not terminate", s);
  RD_LAUNCH("mfddist.finalize", k_dist_finalize, dim3(sgrid(n)), dim3(NTHR), 0, s, (const uint32_t *)st, d_dist, d_drop,
            out_nodata, n);
}

// the elevations of a DEM as doubles (exact for every element type); a float64 DEM is used as it is
template <class T>
static const double *elev_plane(const T *d_z, uint64_t n, hipStream_t s) {
  if constexpr (std::is_same<T, double>::value) return d_z;
  else {
    double *e = Workspace::get().buf<double>("mfddist.elev", n);
    RD_LAUNCH("mfddist.elev", (k_dist_elev<T>), dim3(sgrid(n)), dim3(NTHR), 0, s, d_z, e, n);
    return e;
  }
}

// the proportions from the DEM (tarboton: with or without the flats patched), then the distances: what the two doors of a DEM
// entry run, on the caller's stream or on the null stream
template <class T>
static void dinf_distance(TarbotonFn<T> tarboton, const T *d_dem, T nodata, int w, int h, const uint8_t *d_chan, const DistParams &pr,
                          double *d_dist, double *d_drop, double out_nodata, hipStream_t s) {
  const DinfAcc a = tarboton(d_dem, nodata, w, h, s);
  const double *e = d_drop ? elev_plane<T>(d_dem, (uint64_t)w * h, s) : nullptr;
  mfd_distance<DinfAcc>(a, w, h, d_chan, e, pr, d_dist, d_drop, out_nodata, s);
}

}  // namespace rdgpu

using namespace rdgpu;

extern "C" int rdgpu_mfd_distance_down_dev(const float *d_props9, int w, int h, const uint8_t *d_chan, const double *d_elev,
                                           int stat, int strict, double cell_x, double cell_y, double *d_dist, double *d_drop,
                                           double out_nodata, void *st) {
  return guarded([&] {
    check_args("rdgpu_mfd_distance_down", d_props9, w, h, d_elev != nullptr, stat, cell_x, cell_y, d_dist, d_drop);
    mfd_distance<PropsAcc>(PropsAcc{d_props9}, w, h, d_chan, d_elev, DistParams{stat, strict, cell_x, cell_y}, d_dist, d_drop,
                           out_nodata, (hipStream_t)st);
  });
}
extern "C" int rdgpu_mfd_distance_down(const float *props9, int w, int h, const uint8_t *chan, const double *elev, int stat,
                                       int strict, double cell_x, double cell_y, double *dist, double *drop, double out_nodata) {
  return guarded([&] {
    check_args("rdgpu_mfd_distance_down", props9, w, h, elev != nullptr, stat, cell_x, cell_y, dist, drop);
    const size_t n = (size_t)w * h;
    HostStage hs;
    const float *dp = hs.in("host.props", props9, n * 9);
    const double *de = hs.in("host.mfddist.elev", drop ? elev : nullptr, n);   // (read for the drop only)
    const uint8_t *dc = hs.in("host.mfddist.chan", chan, n);
    double *dd = hs.out("host.mfddist.dist", dist, n), *dr = hs.out("host.mfddist.drop", drop, n);
    mfd_distance<PropsAcc>(PropsAcc{dp}, w, h, dc, de, DistParams{stat, strict, cell_x, cell_y}, dd, dr, out_nodata, nullptr);
    hs.finish();
  });
}
extern "C" int rdgpu_mfd_distance_rounds(uint32_t *rounds) {
  if (!rounds) return RDGPU_ERR_ARG;
  *rounds = g_dist_rounds;
  return RDGPU_OK;
}

#define RD_DINF_DIST_API(FL, ACCESSOR, MAXC, SUF, T)                                                                      \
  extern "C" int rdgpu_dinf_distance_down##FL##_dev_##SUF(const T *d_dem, T nodata, int w, int h, const uint8_t *d_chan, int stat, \
                                                    int strict, double cell_x, double cell_y, double *d_dist, double *d_drop, \
                                                    double out_nodata, void *st) {                                        \
    return guarded([&] {                                                                                                  \
      check_args("rdgpu_dinf_distance_down" #FL, d_dem, w, h, true, stat, cell_x, cell_y, d_dist, d_drop, MAXC);          \
      dinf_distance<T>(ACCESSOR<T>, d_dem, nodata, w, h, d_chan, DistParams{stat, strict, cell_x, cell_y}, d_dist, d_drop, \
                       out_nodata, (hipStream_t)st);                                                                      \
    });                                                                                                                   \
  }                                                                                                                       \
  extern "C" int rdgpu_dinf_distance_down##FL##_##SUF(const T *dem, T nodata, int w, int h, const uint8_t *chan, int stat, \
                                                int strict, double cell_x, double cell_y, double *dist, double *drop,     \
                                                double out_nodata) {                                                      \
    return guarded([&] {                                                                                                  \
      check_args("rdgpu_dinf_distance_down" #FL, dem, w, h, true, stat, cell_x, cell_y, dist, drop, MAXC);                \
      const size_t n = (size_t)w * h;                                                                                     \
      HostStage hs;                                                                                                       \
      const T *d = hs.in("host.dem", dem, n);                                                                             \
      const uint8_t *dc = hs.in("host.mfddist.chan", chan, n);                                                            \
      double *dd = hs.out("host.mfddist.dist", dist, n), *dr = hs.out("host.mfddist.drop", drop, n);                      \
      dinf_distance<T>(ACCESSOR<T>, d, nodata, w, h, dc, DistParams{stat, strict, cell_x, cell_y}, dd, dr, out_nodata, nullptr); \
      hs.finish();                                                                                                        \
    });                                                                                                                   \
  }
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, u8, uint8_t)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u8, uint8_t)
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, i16, int16_t)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i16, int16_t)
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, u16, uint16_t)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u16, uint16_t)
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, i32, int32_t)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i32, int32_t)
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, u32, uint32_t)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, u32, uint32_t)
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, f32, float)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, f32, float)
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, f64, double)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, f64, double)
RD_DINF_DIST_API(, tarboton_device, 0xFFFF0000ull, i8, int8_t)
RD_DINF_DIST_API(_flats, tarboton_flats_device, FLATS_MAX_CELLS, i8, int8_t)
