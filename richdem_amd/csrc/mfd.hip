// mfd.hip -- D-infinity flow directions / proportions and the generic (multiple-receiver) flow accumulation.
//
//  * rdgpu_dinf_flowdirs_*        replaces dinf_flow_directions / dinf_FlowDir
//                                 (reference include/richdem/flowmet/dinf_flowdirs.hpp:128-152, :45-115)
//  * rdgpu_fm_tarboton_*          replaces FM_Tarboton = FM_Dinfinity (flowmet/Tarboton1997.hpp:14-144):
//                                 the 9-float-per-cell proportions array (common/Array3D.hpp:203-206)
//  * rdgpu_flow_accumulation_f64  replaces FlowAccumulation(const Array3D<float>&, Array2D<double>&)
//                                 (methods/flow_accumulation_generic.hpp:33-100) for any proportions array
//  * rdgpu_fa_tarboton_*          replaces FA_Tarboton / FA_Dinfinity (methods/flow_accumulation.hpp:16-17)
//                                 without materialising the 36 B/cell array: 5 B/cell (receiver, share)
//  * rdgpu_fm_tarboton_flats_*    the same two with the cells of drainable flats patched from Barnes' flat mask
//    rdgpu_fa_tarboton_flats_*    (k_tarboton_flats; no reference counterpart, DESIGN.md "D-infinity across flats")
//
// The slope/angle arithmetic is done in double with atan2/sqrt exactly as written in the reference
// (-ffp-contract=off: no FMA contraction); device libm may differ from glibc in the last ulp of atan2, so
// these outputs are compared with a tolerance (north_star: <= 1 ULP in f32), not bit for bit.
//
// Accumulation: "last arriver continues" generalised to several receivers.  A completed cell pushes
// share*total to each receiver with a returning device-scope atomic add and decrements the receiver's
// pending-donor count; the receivers it completed are the work list's to continue with (mfd_worklist.hpp).
// f64 sums in a different order than the reference's FIFO: exact for integer-valued flows, f64 rounding
// otherwise.
#include "flats.hpp"
#include "flowdirs.hpp"
#include "mfd_worklist.hpp"

#include <climits>

namespace rdgpu {

// ------------------------------------------------------------------------------------------
// D-infinity per cell, on the 3 x 3 window of elevations (rows y-1, y, y+1; columns x-1, x, x+1).
// Both kernels are LDS-tiled stencils (r04: 64 x 32 tiles + halo, the window slides down a column in registers, as
// flowdirs.hip does): one thread per cell with sixteen neighbour loads and their 64-bit addresses was 36 ms at 40000^2.
// The reference takes atan2 of every facet and then branches on the angle.  Which branch it takes follows from the two
// slopes alone except within rounding of the thresholds (s1, s2 are differences of elevations, never -0.0):
// r < 0 <=> s2 < 0; r > atan2(1, 1) <=> s1 <= 0 or s2 > s1.  So the angle is computed ONCE, for the facet that wins (the
// steepest-facet comparison only needs s), and per facet only where s2 / s1 is within a margin of a threshold.  Results are
// the reference's bit for bit (tests/test_s2_dinf_gpu.py: every band of the 10000^2 raster).
// ------------------------------------------------------------------------------------------
constexpr int DTW = 64, DTH = 32, DLW_ = DTW + 2, DLH_ = DTH + 2;

template <class T>
__device__ __forceinline__ void dinf_stage(const T *__restrict__ z, int w, int h, int x0, int y0, T *sz) {
  constexpr int IPT = (DLH_ * DLW_ + NTHR - 1) / NTHR;
  T zv[IPT];
#pragma unroll
  for (int r = 0; r < IPT; r++) {   // clamped addresses: a cell outside the raster is never used as a neighbour
    const int i = min((int)threadIdx.x + r * NTHR, DLH_ * DLW_ - 1);
    const int ly = i / DLW_, lx = i - ly * DLW_;
    const int gx = min(max(x0 - 1 + lx, 0), w - 1), gy = min(max(y0 - 1 + ly, 0), h - 1);
    zv[r] = z[(size_t)gy * w + gx];
  }
#pragma unroll
  for (int r = 0; r < IPT; r++) {
    const int i = (int)threadIdx.x + r * NTHR;
    if (i < DLH_ * DLW_) sz[i] = zv[r];
  }
}

// dinf_FlowDir, flowmet/dinf_flowdirs.hpp:45-115 (facet tables :21-27), interior data cell; win[r][c]
template <class T>
__device__ __forceinline__ float dinf_cell(const T (&win)[3][3]) {
  constexpr int dy_e1[8] = {0, -1, -1, 0, 0, 1, 1, 0}, dx_e1[8] = {1, 0, 0, -1, -1, 0, 0, 1};
  constexpr int dy_e2[8] = {-1, -1, -1, -1, 1, 1, 1, 1}, dx_e2[8] = {1, 1, -1, -1, -1, -1, 1, 1};
  constexpr double ac[8] = {0., 1., 1., 2., 2., 3., 3., 4.}, af[8] = {1., -1., 1., -1., 1., -1., 1., -1.};
  int nmax = -1;
  double smax = 0, rmax = 0, w1 = 0, w2 = 0;   // w1, w2: the winning facet's slopes when its angle is still owed
  bool owed = false;
  const double e0 = (double)win[1][1];
  const double quarter = atan2(1.0, 1.0);
#pragma unroll
  for (int k = 0; k < 8; k++) {                                      // :68-96
    const double e1 = (double)win[1 + dy_e1[k]][1 + dx_e1[k]];
    const double e2 = (double)win[1 + dy_e2[k]][1 + dx_e2[k]];
    const double s1 = (e0 - e1) / 1.0, s2 = (e1 - e2) / 1.0;
    int branch;   // 0: r < 0; 1: r > quarter; 2: in between (r = atan2(s2, s1))
    if (s2 < 0) branch = 0;
    else if (s1 <= 0) branch = (s1 == 0 && s2 == 0) ? 2 : 1;        // atan2(+0, +0) = 0; otherwise r >= pi / 2
    else {
      const double lo = s1 * (1.0 - 0x1p-40), hi = s1 * (1.0 + 0x1p-40);
      if (s2 > hi) branch = 1;
      else if (s2 < lo) branch = 2;
      else branch = atan2(s2, s1) > quarter ? 1 : 2;                 // within rounding of the threshold: as the reference does
    }
    double s;
    if (branch == 0) s = s1;
    else if (branch == 1) s = (e0 - e2) / sqrt(2.0);
    else s = sqrt(s1 * s1 + s2 * s2);
    if (s > smax) {
      smax = s; nmax = k;
      rmax = branch == 1 ? quarter : 0.0;
      owed = branch == 2;
      w1 = s1; w2 = s2;
    }
  }
  if (owed) rmax = atan2(w2, w1);
  double rg = 0;                                                     // NO_FLOW
  if (nmax != -1) rg = af[nmax] * rmax + ac[nmax] * M_PI / 2;
  return (float)rg;
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_dinf_dirs(const T *__restrict__ z, T nodata, float *__restrict__ out, int w,
                                                    int h, uint32_t tilesX, uint32_t ntiles) {
  __shared__ T sz[DLH_ * DLW_];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * DTW, y0 = (int)(t / tilesX) * DTH;
  dinf_stage<T>(z, w, h, x0, y0, sz);
  __syncthreads();
  const int lx = threadIdx.x & (DTW - 1), yb = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (DTH / 4);
  const int gx = x0 + lx;
  T win[3][3];
#pragma unroll
  for (int e = 0; e < 3; e++) { win[0][e] = sz[yb * DLW_ + lx + e]; win[1][e] = sz[(yb + 1) * DLW_ + lx + e]; }
#pragma unroll 2
  for (int j = 0; j < DTH / 4; j++) {
    const int gy = y0 + yb + j;
#pragma unroll
    for (int e = 0; e < 3; e++) win[2][e] = sz[(yb + j + 2) * DLW_ + lx + e];
    float a;
    if (win[1][1] == nodata) a = -1.0f;                                  // dinf_NO_DATA, :147-148
    else if (gx == 0 || gy == 0 || gx == w - 1 || gy == h - 1) {         // :46-63
      double e;
      if (gx == 0 && gy == 0) e = 3 * M_PI / 4;
      else if (gx == 0 && gy == h - 1) e = 5 * M_PI / 4;
      else if (gx == w - 1 && gy == 0) e = 1 * M_PI / 4;
      else if (gx == w - 1 && gy == h - 1) e = 7 * M_PI / 4;
      else if (gx == 0) e = 4 * M_PI / 4;
      else if (gx == w - 1) e = 0 * M_PI / 4;
      else if (gy == 0) e = 2 * M_PI / 4;
      else e = 6 * M_PI / 4;
      a = (float)e;
    } else a = dinf_cell<T>(win);
    if (gx < w && gy < h) out[(size_t)gy * w + gx] = a;
#pragma unroll
    for (int e = 0; e < 3; e++) { win[0][e] = win[1][e]; win[1][e] = win[2][e]; }
  }
}

// ------------------------------------------------------------------------------------------
// FM_Tarboton, flowmet/Tarboton1997.hpp:14-144 in compact form: rcv = first receiver n (0 none, 255
// NoData), share = proportion to neighbour n, share2 = proportion to neighbour nwrap(n + 1).  Interior data cell;
// win[r][c] as above.
// ------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void tarboton_cell(const T (&win)[3][3], T nodata, int &rcv, float &share, float &share2) {
  constexpr int dy_e1[9] = {0, 0, -1, -1, 0, 0, 1, 1, 0}, dx_e1[9] = {0, -1, 0, 0, 1, 1, 0, 0, -1};
  constexpr int dy_e2[9] = {0, -1, -1, -1, -1, 1, 1, 1, 1}, dx_e2[9] = {0, -1, -1, 1, 1, 1, 1, -1, -1};
  constexpr double af[9] = {0, -1., 1., -1., 1., -1., 1., -1., 1.};
  const float dang = (float)atan2(1.0, 1.0);
  rcv = 0;
  share = 0.0f;
  share2 = 0.0f;
  int nmax = -1;
  double smax = 0, w1 = 0, w2 = 0;
  float rmax = 0;
  bool owed = false;
  const double e0 = (double)win[1][1];
#pragma unroll
  for (int n = 1; n <= 8; n++) {                                       // :56-92
    const T v1 = win[1 + dy_e1[n]][1 + dx_e1[n]], v2 = win[1 + dy_e2[n]][1 + dx_e2[n]];
    if (v1 == nodata || v2 == nodata) continue;
    const double e1 = (double)v1, e2 = (double)v2;
    const double s1 = (e0 - e1) / 1.0, s2 = (e1 - e2) / 1.0;
    // which of the reference's three branches (:83-91) the angle r = atan2(s2, s1) falls into follows from the slopes except
    // within a margin of the two thresholds (there: atan2, as the reference); the angle itself is only needed for the
    // facet that wins
    int branch;   // 0: r < 1e-7; 1: r > dang - 1e-7; 2: in between
    if (s2 < 0) branch = 0;
    else if (s1 <= 0) branch = (s1 == 0 && s2 == 0) ? 0 : 1;            // atan2(+0, +0) = 0; otherwise r >= pi / 2
    else if (s2 < s1 * 0.99e-7) branch = 0;                             // tan(1e-7) = 1.0000000000000033e-7
    else if (s2 > s1) branch = 1;                                       // tan(dang - 1e-7) = 0.99999984...
    else if (s2 > s1 * 1.01e-7 && s2 < s1 * 0.9999995) branch = 2;
    else {
      const double r = atan2(s2, s1);
      branch = r < 1e-7 ? 0 : r > dang - 1e-7 ? 1 : 2;
    }
    double s;
    if (branch == 0) s = s1;
    else if (branch == 1) s = (e0 - e2) / sqrt(2.0);
    else s = sqrt(s1 * s1 + s2 * s2);
    if (s > smax) {
      smax = s; nmax = n;
      rmax = branch == 1 ? dang : 0.0f;
      owed = branch == 2;
      w1 = s1; w2 = s2;
    }
  }
  if (nmax == -1) return;
  if (owed) rmax = (float)atan2(w2, w1);
  if (af[nmax] == 1 && rmax == 0) rmax = dang;                          // :99-104
  else if (af[nmax] == 1 && rmax == dang) rmax = 0;
  else if (af[nmax] == 1) rmax = (float)(M_PI / 4 - rmax);
  const int nxt = nmax + 1 == 9 ? 1 : nmax + 1;
  if (rmax == 0) { rcv = nmax; share = 1.0f; }                          // :106-113
  else if (rmax == dang) { rcv = nxt; share = 1.0f; }
  else {
    rcv = nmax | 0x10;                            // 0x10: two receivers
    share = (float)(rmax / (M_PI / 4.));          // props(x,y,nmax), :111
    share2 = (float)(1 - rmax / (M_PI / 4.));     // props(x,y,nwrap(nmax+1)), :112
  }
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_tarboton(const T *__restrict__ z, T nodata, uint8_t *__restrict__ rcv,
                                                   float *__restrict__ sh1, float *__restrict__ sh2, int w, int h,
                                                   uint32_t tilesX, uint32_t ntiles) {
  __shared__ T sz[DLH_ * DLW_];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * DTW, y0 = (int)(t / tilesX) * DTH;
  dinf_stage<T>(z, w, h, x0, y0, sz);
  __syncthreads();
  const int lx = threadIdx.x & (DTW - 1), yb = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (DTH / 4);
  const int gx = x0 + lx;
  T win[3][3];
#pragma unroll
  for (int e = 0; e < 3; e++) { win[0][e] = sz[yb * DLW_ + lx + e]; win[1][e] = sz[(yb + 1) * DLW_ + lx + e]; }
#pragma unroll 2
  for (int j = 0; j < DTH / 4; j++) {
    const int gy = y0 + yb + j;
#pragma unroll
    for (int e = 0; e < 3; e++) win[2][e] = sz[(yb + j + 2) * DLW_ + lx + e];
    int r = 0;
    float p = 0.0f, q = 0.0f;
    if (win[1][1] == nodata) r = 255;                                                     // :44-47
    else if (!(gx == 0 || gy == 0 || gx == w - 1 || gy == h - 1)) tarboton_cell<T>(win, nodata, r, p, q);   // :49-50: edges never flow
    if (gx < w && gy < h) {
      const size_t c = (size_t)gy * w + gx;
      rcv[c] = (uint8_t)r;
      sh1[c] = p;
      sh2[c] = q;
    }
#pragma unroll
    for (int e = 0; e < 3; e++) { win[0][e] = win[1][e]; win[1][e] = win[2][e]; }
  }
}

__global__ __launch_bounds__(NTHR) void k_tarboton_props(const uint8_t *__restrict__ rcv, const float *__restrict__ sh1,
                                                         const float *__restrict__ sh2, float *__restrict__ props,
                                                         uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    float p[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};   // NO_FLOW_GEN, :25
    const int rr = rcv[c], r = rr & 0xF;
    if (rr == 255) p[0] = -2.0f;                         // NO_DATA_GEN, :45
    else if (r >= 1) {
      p[0] = 0.0f;                                       // HAS_FLOW_GEN, :97
      p[r] = sh1[c];
      if (rr & 0x10) p[r == 8 ? 1 : r + 1] = sh2[c];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) props[9 * c + k] = p[k];
  }
}

// ------------------------------------------------------------------------------------------
// D-infinity across flats (DESIGN.md "D-infinity across flats"): the cells FM_Tarboton leaves without flow inside a
// drainable flat get their receivers from Barnes' flat mask instead of the elevations.  Runs over k_tarboton's tiles after
// k_tarboton, the D8 directions and resolve_flats_device (flats.hpp), and writes the patched cells only.
//   patched: d8 == NO_FLOW and the cell's flat has a low edge (label != 0) -- such a cell is interior and has rcv == 0;
//   its window: the 3 x 3 mask values, every neighbour of another flat (or of none) replaced by FLAT_OTHER, which goes to
//   tarboton_cell as the NoData value: the facet rule, thresholds and facet order are FM_Tarboton's;
//   no descending facet: everything to the first neighbour n = 1..8 of the same flat with a smaller mask value;
//   none either: the cell stays without flow and is counted.
// A tile whose interior data cells all have a receiver costs its rcv bytes: one block-wide vote, then the block leaves.
// ------------------------------------------------------------------------------------------
constexpr int32_t FLAT_OTHER = INT32_MIN;   // flat_mask values are >= 0
enum { FC_NOFLOW = 0, FC_PATCHED = 1, FC_FALLBACK = 2, FC_UNRESOLVED = 3, FC_N = 4 };

__global__ __launch_bounds__(NTHR) void k_tarboton_flats(uint8_t *__restrict__ rcv, float *__restrict__ sh1,
                                                         float *__restrict__ sh2, const uint8_t *__restrict__ d8,
                                                         const int32_t *__restrict__ M, const uint32_t *__restrict__ L,
                                                         const int32_t *__restrict__ fh, int w, int h, uint32_t tilesX,
                                                         uint32_t ntiles, unsigned long long *counts) {
  __shared__ int32_t sm[DLH_ * DLW_];    // flat_mask with a one-cell halo
  __shared__ uint32_t sg[DLH_ * DLW_];   // the group: L + 1 where the cell's flat has a low edge, else 0 (k_flat_labels_out)
  __shared__ uint32_t scnt[FC_N];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * DTW, y0 = (int)(t / tilesX) * DTH;
  const int lx = threadIdx.x & (DTW - 1), yb = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (DTH / 4);
  const int gx = x0 + lx;
  if (threadIdx.x < FC_N) scnt[threadIdx.x] = 0;
  uint32_t open = 0;   // bit j: the thread's cell of row yb + j is an interior data cell without flow
  if (gx >= 1 && gx < w - 1) {
#pragma unroll
    for (int j = 0; j < DTH / 4; j++) {
      const int gy = y0 + yb + j;
      if (gy >= 1 && gy < h - 1 && rcv[(size_t)gy * w + gx] == 0) open |= 1u << j;
    }
  }
  if (!__syncthreads_or(open != 0)) return;
  uint32_t cnt[FC_N] = {(uint32_t)__builtin_popcount(open), 0, 0, 0};
  if (L) {   // (null: no flat of the raster has an outlet -- nothing to patch, the cells are counted)
    constexpr int IPT = (DLH_ * DLW_ + NTHR - 1) / NTHR;
    int32_t mv[IPT];
    uint32_t lv[IPT];
#pragma unroll
    for (int r = 0; r < IPT; r++) {   // clamped addresses: a patched cell is interior, its window lies inside the raster
      const int i = min((int)threadIdx.x + r * NTHR, DLH_ * DLW_ - 1);
      const int ly = i / DLW_, sx = i - ly * DLW_;
      const size_t c = (size_t)min(max(y0 - 1 + ly, 0), h - 1) * w + min(max(x0 - 1 + sx, 0), w - 1);
      mv[r] = M[c];
      lv[r] = L[c];
    }
#pragma unroll
    for (int r = 0; r < IPT; r++) lv[r] = fh[lv[r]] >= 0 ? lv[r] + 1u : 0u;
#pragma unroll
    for (int r = 0; r < IPT; r++) {
      const int i = (int)threadIdx.x + r * NTHR;
      if (i < DLH_ * DLW_) { sm[i] = mv[r]; sg[i] = lv[r]; }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t rest = open; rest; rest &= rest - 1u) {
      const int j = __builtin_ctz(rest);
      const size_t c = (size_t)(y0 + yb + j) * w + gx;
      const int li = (yb + j + 1) * DLW_ + lx + 1;
      const uint32_t g0 = sg[li];
      if (g0 == 0 || d8[c] != 0) continue;
      cnt[FC_PATCHED]++;
      int32_t win[3][3];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int e = 0; e < 3; e++) {
          const int k = li + (r - 1) * DLW_ + (e - 1);
          win[r][e] = sg[k] == g0 ? sm[k] : FLAT_OTHER;
        }
      int r = 0;
      float p = 0.0f, q = 0.0f;
      tarboton_cell<int32_t>(win, FLAT_OTHER, r, p, q);
      if (r == 0) {
#pragma unroll
        for (int n = 8; n >= 1; n--) {   // (descending: the first n in 1..8 wins)
          const int32_t v = win[1 + mdy(n)][1 + mdx(n)];
          if (v != FLAT_OTHER && v < win[1][1]) r = n;
        }
        if (r == 0) { cnt[FC_UNRESOLVED]++; continue; }
        p = 1.0f;
        cnt[FC_FALLBACK]++;
      }
      rcv[c] = (uint8_t)r;
      sh1[c] = p;
      sh2[c] = q;
    }
  }
#pragma unroll
  for (int k = 0; k < FC_N; k++) {   // per wavefront, per block, one atomic per block and counter
    uint32_t v = cnt[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&scnt[k], v);
  }
  __syncthreads();
  if (threadIdx.x < FC_N && scnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

constexpr uint32_t PEND_NODATA = 0xFFFFFFFFu;

// deps, flow_accumulation_generic.hpp:47-58 (donors are interior cells only), + the initial ready flags :61-64
template <class ACC>
__global__ __launch_bounds__(NTHR) void k_mfd_init(ACC a, uint32_t *pending, uint8_t *ready, int w, int h) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    uint32_t k = PEND_NODATA;
    uint8_t rdy = 0;
    if (!a.nodata(c)) {
      k = 0;
#pragma unroll
      for (int m = 1; m <= 8; m++) {
        const int dx = x + mdx(m), dy = y + mdy(m);
        if (dx < 1 || dy < 1 || dx >= w - 1 || dy >= h - 1) continue;   // donors: interior cells
        const uint64_t d = (uint64_t)dy * w + dx;
        if (a.nodata(d)) continue;
        if (a.share(d, m <= 4 ? m + 4 : m - 4) > 0) k++;
      }
      rdy = k == 0;
    }
    pending[c] = k;
    ready[c] = rdy;
  }
}

// The work list's step (mfd_worklist.hpp) for the COMPLETED cell c: its total goes to the receivers -- all returning adds
// in flight together, one wait, then all counter decrements together: two memory round trips per cell however many
// receivers it has.  Returns the receivers whose counter this thread took to zero: they are complete.
template <class ACC>
struct AccStep {
  ACC a;
  uint32_t *pending;
  double *acc;
  int w, h;
  __device__ __forceinline__ int width() const { return w; }
  __device__ __forceinline__ uint32_t operator()(uint32_t c, bool from_list) const {
    // the total: final since an earlier launch (or a source), or just completed: then read at the memory side
    const double v = from_list ? acc[c] : atomicAdd(&acc[c], 0.0);
    const int x = (int)(c % (uint32_t)w), y = (int)(c / (uint32_t)w);
    if (x == 0 || y == 0 || x == w - 1 || y == h - 1) return 0;   // edge cells never pass flow on (FM_*: :49-50)
    float p[8];
    bool nd[8];
#pragma unroll
    for (int n = 1; n <= 8; n++) p[n - 1] = a.share(c, n);
#pragma unroll
    for (int n = 1; n <= 8; n++)   // flow_accumulation_generic.hpp:81-86
      nd[n - 1] = (p[n - 1] > 0) ? a.nodata((uint64_t)(y + mdy(n)) * w + (x + mdx(n))) : true;
    double prev = 0;
#pragma unroll
    for (int n = 1; n <= 8; n++)
      if (!nd[n - 1]) prev += atomicAdd(&acc[(uint64_t)(y + mdy(n)) * w + (x + mdx(n))], (double)p[n - 1] * v);   // :87
    // every add has returned (= was performed at the memory side) before any counter is decremented
    asm volatile("s_waitcnt vmcnt(0)" ::"v"(prev) : "memory");
    uint32_t old[8];
#pragma unroll
    for (int n = 1; n <= 8; n++)
      if (!nd[n - 1])
        old[n - 1] = __hip_atomic_fetch_sub(&pending[(uint64_t)(y + mdy(n)) * w + (x + mdx(n))], 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
    uint32_t done = 0;
#pragma unroll
    for (int n = 1; n <= 8; n++)
      if (!nd[n - 1] && old[n - 1] == 1u) done |= 1u << (n - 1);
    return done;
  }
};

template <class ACC>
__global__ __launch_bounds__(NTHR) void k_mfd_nodata(ACC a, double *acc, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride)
    if (a.nodata(c)) acc[c] = -1.0;                                     // ACCUM_NO_DATA, :95-97
}

static uint32_t g_mfd_rounds = 0;

template <class ACC>
static void mfd_accumulate(ACC a, int w, int h, double *d_acc, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  uint32_t *pending = ws.buf<uint32_t>("mfd.pending", n);
  uint8_t *ready = ws.buf<uint8_t>("mfd.ready", n);
  RD_LAUNCH("mfd.init", (k_mfd_init<ACC>), dim3(sgrid(n)), dim3(NTHR), 0, s, a, pending, ready, w, h);
  g_mfd_rounds = 0;
  // Long lists go through the buffer kernel (their by-products are processed next launch, densely packed: a wavefront
  // that works off its own by-products runs at a few active lanes -- S3's filled DEM, 223 launches: 256 ms, one stacked
  // launch 492); once a list is short the launches are what costs (S3 where every cell drains: 2614 launches, 7.2 s) and
  // the stack kernel finishes everything that is left.  RDGPU_MFD_STACK_BELOW sets the list length of the switch (0: never).
  const char *se = getenv("RDGPU_MFD_STACK_BELOW");
  const uint32_t stack_below = se ? (uint32_t)strtoul(se, nullptr, 10) : (1u << 22);
  g_mfd_rounds = worklist_run(ready, n, AccStep<ACC>{a, pending, d_acc, w, h}, "mfd.round", "mfd.round", stack_below,
                              "rdgpu flow accumulation did not terminate", s);
  RD_LAUNCH("mfd.nodata", (k_mfd_nodata<ACC>), dim3(sgrid(n)), dim3(NTHR), 0, s, a, d_acc, n);
}

// ------------------------------------------------------------------------------------------
// FM_Holmgren (flowmet/Holmgren1994.hpp:14-88), FM_Quinn (= Holmgren, x = 1; Quinn1991.hpp:13-17),
// FM_Freeman (Freeman1991.hpp:14-86), FM_D4 = FM_OCallaghan<D4> (OCallaghan1984.hpp:13-77, :86) into the
// reference's 9-float proportions layout.  The arithmetic is written as in the reference (rise in the
// element type's promoted type, gradient and pow in double, Holmgren sums the STORED floats, Freeman the
// doubles, the normalisation multiplies float by double); pow comes from the device libm, so proportions
// are specified to <= 1 ULP (f32) like D-infinity.  FM_D4 keeps the reference's slot numbering: it
// stores the chosen D4 neighbour n = 1..4 (left, up, right, down) in slot n, and FlowAccumulation then reads
// slot n with the D8 offsets -- reproduced as is, because that is what FA_D4 returns.
// ------------------------------------------------------------------------------------------
// pow() as the reference's libm returns it, to the extent the f32 proportions can see: glibc's pow is exact
// whenever x^y is representable, and with short-mantissa gradients (differences of float elevations) and an
// integer exponent, x^y often IS representable and lands exactly on a float rounding tie -- where the device
// libm's last-bit error would flip the stored float.  Integer exponents up to 64 are therefore evaluated by
// binary powering in double-double (one final rounding); everything else goes to the device pow (<= 1 ulp).
struct dd { double hi, lo; };
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
  const double p = a.hi * b.hi;
  double e = __builtin_fma(a.hi, b.hi, -p);
  e += a.hi * b.lo + a.lo * b.hi;
  const double hi = p + e;
  return dd{hi, e - (hi - p)};
}
__device__ __forceinline__ double pow_ref(double x, double y) {
  if (y == 1.0) return x;
  if (y >= 2.0 && y <= 64.0 && y == (double)(int)y) {
    int n = (int)y;
    dd r{1.0, 0.0}, b{x, 0.0};
    for (;;) {
      if (n & 1) r = dd_mul(r, b);
      n >>= 1;
      if (!n) break;
      b = dd_mul(b, b);
    }
    return r.hi;
  }
  return pow(x, y);
}

enum { MFD_HOLMGREN = 0, MFD_FREEMAN = 1, MFD_QUINN = 2, MFD_D4 = 3 };

template <class T>
__global__ __launch_bounds__(NTHR) void k_fm_mfd(const T *__restrict__ z, T nodata, float *__restrict__ props, int w, int h,
                                                 int method, double xparam) {
  constexpr double SQ2 = 1.414213562373095048801688724209698078569671875376948;
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    float p[9];
#pragma unroll
    for (int k = 0; k < 9; k++) p[k] = -1.0f;
    const T e = z[c];
    if (e == nodata) {
      p[0] = -2.0f;
    } else if (x > 0 && y > 0 && x < w - 1 && y < h - 1) {
      if (method == MFD_D4) {
        int lowest_n = 0;
        T lowest = T();
#pragma unroll
        for (int k = 1; k <= 4; k++) {
          const int dx = k == 1 ? -1 : k == 3 ? 1 : 0, dy = k == 2 ? -1 : k == 4 ? 1 : 0;   // constants.hpp:54-55
          const T ne = z[(size_t)(y + dy) * w + (x + dx)];
          if (ne == nodata || ne >= e) continue;
          if (lowest_n == 0 || ne < lowest) { lowest = ne; lowest_n = k; }
        }
        if (lowest_n) { p[0] = 0.0f; p[lowest_n] = 1.0f; }
      } else {
        double C = 0;
#pragma unroll
        for (int k = 1; k <= 8; k++) {
          const T ne = z[(size_t)(y + mdy(k)) * w + (x + mdx(k))];
          if (ne == nodata) continue;
          if (ne < e) {
            const double rise = e - ne;
            const double run = (k & 1) ? 1.0 : SQ2;
            const double grad = rise / run;
            if (method == MFD_HOLMGREN) {
              p[k] = (float)pow_ref(grad * ((k & 1) ? 0.5 : 0.354), xparam);
              C += p[k];
            } else {
              const double cval = pow_ref(grad, xparam);
              p[k] = (float)cval;
              C += cval;
            }
          }
        }
        if (C > 0) {
          p[0] = 0.0f;
          C = 1 / C;
#pragma unroll
          for (int k = 1; k <= 8; k++) p[k] = p[k] > 0 ? (float)(p[k] * C) : 0.0f;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) props[c * 9 + k] = p[k];
  }
}

static void check_mfd_method(int method) {
  if (method < 0 || method > 3) throw Error(RDGPU_ERR_ARG, "rdgpu_fm_mfd: method must be 0 (Holmgren), 1 (Freeman), 2 (Quinn) or 3 (D4)");
}

// arguments checked by the caller (mfd_check_args, check_mfd_method)
template <class T>
static void fm_mfd_device(const T *d_z, T nodata, int w, int h, int method, double xparam, float *d_props, hipStream_t s) {
  if (method == MFD_QUINN) { method = MFD_HOLMGREN; xparam = 1.0; }
  RD_LAUNCH("mfd.fm_mfd", (k_fm_mfd<T>), dim3(sgrid((uint64_t)w * h)), dim3(NTHR), 0, s, d_z, nodata, d_props, w, h, method, xparam);
}

template <class T>
DinfAcc tarboton_device(const T *d_z, T nodata, int w, int h, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  uint8_t *rcv = ws.buf<uint8_t>("mfd.rcv", n);
  float *sh1 = ws.buf<float>("mfd.sh1", n), *sh2 = ws.buf<float>("mfd.sh2", n);
  {
    const uint32_t dtilesX = (w + DTW - 1) / DTW, dntiles = dtilesX * ((h + DTH - 1) / DTH);
    RD_LAUNCH("mfd.tarboton", (k_tarboton<T>), dim3(xcd_grid(dntiles)), dim3(NTHR), 0, s, d_z, nodata, rcv, sh1, sh2, w, h, dtilesX, dntiles);
  }
  return DinfAcc{rcv, sh1, sh2};
}
template DinfAcc tarboton_device<uint8_t>(const uint8_t *, uint8_t, int, int, hipStream_t);   // (mfd_distance.hip)
template DinfAcc tarboton_device<int8_t>(const int8_t *, int8_t, int, int, hipStream_t);
template DinfAcc tarboton_device<uint16_t>(const uint16_t *, uint16_t, int, int, hipStream_t);
template DinfAcc tarboton_device<int16_t>(const int16_t *, int16_t, int, int, hipStream_t);
template DinfAcc tarboton_device<uint32_t>(const uint32_t *, uint32_t, int, int, hipStream_t);
template DinfAcc tarboton_device<int32_t>(const int32_t *, int32_t, int, int, hipStream_t);
template DinfAcc tarboton_device<float>(const float *, float, int, int, hipStream_t);
template DinfAcc tarboton_device<double>(const double *, double, int, int, hipStream_t);

// the counts of the calling thread's last tarboton_flats_device: copied to pinned words of the thread's own on the call's stream
struct FlatsCounts {
  unsigned long long *host = nullptr;
  hipStream_t stream = nullptr;
  int device = 0;
  bool pending = false;
};
static thread_local FlatsCounts g_flats_counts;

template <class T>
DinfAcc tarboton_flats_device(const T *d_z, T nodata, int w, int h, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  const DinfAcc a = tarboton_device<T>(d_z, nodata, w, h, s);
  Workspace &ws = Workspace::get();
  uint8_t *d8 = ws.buf<uint8_t>("mfd.flats_d8", n);
  flowdirs_device<T>(d_z, nodata, w, h, d8, MODE_D8, s);
  int32_t *M, *fh;
  uint32_t *L;
  resolve_flats_device<T>(d_z, d8, w, h, &M, &L, &fh, s);
  unsigned long long *counts = ws.buf<unsigned long long>("mfd.flats_counts", FC_N);
  RD_HIP(hipMemsetAsync(counts, 0, FC_N * sizeof(unsigned long long), s));
  const uint32_t dtilesX = (w + DTW - 1) / DTW, dntiles = dtilesX * ((h + DTH - 1) / DTH);
  RD_LAUNCH("mfd.tarboton_flats", k_tarboton_flats, dim3(xcd_grid(dntiles)), dim3(NTHR), 0, s, const_cast<uint8_t *>(a.rcv),
            const_cast<float *>(a.sh1), const_cast<float *>(a.sh2), (const uint8_t *)d8, (const int32_t *)M, (const uint32_t *)L,
            (const int32_t *)fh, w, h, dtilesX, dntiles, counts);
  FlatsCounts &fc = g_flats_counts;
  if (!fc.host) RD_HIP(hipHostMalloc((void **)&fc.host, FC_N * sizeof(unsigned long long), hipHostMallocDefault));
  RD_HIP(hipGetDevice(&fc.device));
  fc.stream = s;
  fc.pending = true;
  RD_HIP(hipMemcpyAsync(fc.host, counts, FC_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  return a;
}
template DinfAcc tarboton_flats_device<uint8_t>(const uint8_t *, uint8_t, int, int, hipStream_t);   // (mfd_distance.hip)
template DinfAcc tarboton_flats_device<int8_t>(const int8_t *, int8_t, int, int, hipStream_t);
template DinfAcc tarboton_flats_device<uint16_t>(const uint16_t *, uint16_t, int, int, hipStream_t);
template DinfAcc tarboton_flats_device<int16_t>(const int16_t *, int16_t, int, int, hipStream_t);
template DinfAcc tarboton_flats_device<uint32_t>(const uint32_t *, uint32_t, int, int, hipStream_t);
template DinfAcc tarboton_flats_device<int32_t>(const int32_t *, int32_t, int, int, hipStream_t);
template DinfAcc tarboton_flats_device<float>(const float *, float, int, int, hipStream_t);
template DinfAcc tarboton_flats_device<double>(const double *, double, int, int, hipStream_t);

// ------------------------------------------------------------------------------------------
// The entry points.  Each product has a typed driver on device pointers and a stream; its `_dev` entry runs the driver on the
// caller's stream, its host entry stages the caller's arrays (HostStage) and runs the same driver on the null stream.
// ------------------------------------------------------------------------------------------
static void mfd_check_args(const void *in, const void *out, int w, int h, const char *who, uint64_t max_cells = 0xFFFF0000ull) {
  if (!in || !out) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_dims(w, h, who, max_cells);
}

template <class T>
static void dinf_flowdirs_device(const T *d_z, T nodata, int w, int h, float *d_out, hipStream_t s) {
  const uint32_t dtilesX = (w + DTW - 1) / DTW, dntiles = dtilesX * ((h + DTH - 1) / DTH);
  RD_LAUNCH("mfd.dinf_dirs", (k_dinf_dirs<T>), dim3(xcd_grid(dntiles)), dim3(NTHR), 0, s, d_z, nodata, d_out, w, h, dtilesX, dntiles);
}
// tarboton: tarboton_device, or tarboton_flats_device for the `_flats` entries
template <class T>
static void fm_tarboton_device(TarbotonFn<T> tarboton, const T *d_z, T nodata, int w, int h, float *d_props9, hipStream_t s) {
  const DinfAcc a = tarboton(d_z, nodata, w, h, s);
  const uint64_t n = (uint64_t)w * h;
  RD_LAUNCH("mfd.tarboton_props", k_tarboton_props, dim3(sgrid(n)), dim3(NTHR), 0, s, a.rcv, a.sh1, a.sh2, d_props9, n);
}
template <class T>
static void fa_tarboton_device(TarbotonFn<T> tarboton, const T *d_z, T nodata, int w, int h, double *d_accum, hipStream_t s) {
  const DinfAcc a = tarboton(d_z, nodata, w, h, s);
  mfd_accumulate<DinfAcc>(a, w, h, d_accum, s);
}
template <class T>
static void fa_mfd_device(const T *d_z, T nodata, int w, int h, int method, double xparam, double *d_accum, hipStream_t s) {
  float *p = Workspace::get().buf<float>("mfd.props", (uint64_t)w * h * 9);
  fm_mfd_device<T>(d_z, nodata, w, h, method, xparam, p, s);
  mfd_accumulate<PropsAcc>(PropsAcc{p}, w, h, d_accum, s);
}

// The host doors.  A DEM up, `per_cell` floats a cell down: run(device DEM, device planes) on the null stream.
template <class T, class Run>
static void host_dem_to_f32(const T *dem, int w, int h, const char *out_name, float *out, size_t per_cell, Run &&run) {
  const size_t n = (size_t)w * h;
  HostStage st;
  const T *d = st.in("host.dem", dem, n);
  float *o = st.out(out_name, out, n * per_cell);
  run(d, o);
  st.finish();
}
// A DEM up, the accumulation array both ways (the caller's flow generated per cell in, the accumulation out).
template <class T, class Run>
static void host_dem_accum(const T *dem, int w, int h, double *accum, Run &&run) {
  const size_t n = (size_t)w * h;
  HostStage st;
  const T *d = st.in("host.dem", dem, n);
  double *da = st.inout("host.area", accum, n);
  run(d, da);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_MFD_API(SUF, T)                                                                                      \
  extern "C" int rdgpu_dinf_flowdirs_dev_##SUF(const T *d_dem, T nodata, int w, int h, float *d_out, void *st) { \
    return guarded([&] {                                                                                        \
      mfd_check_args(d_dem, d_out, w, h, "rdgpu_dinf_flowdirs");                                                \
      dinf_flowdirs_device<T>(d_dem, nodata, w, h, d_out, (hipStream_t)st);                                     \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_dinf_flowdirs_##SUF(const T *dem, T nodata, int w, int h, float *out) {                  \
    return guarded([&] {                                                                                        \
      mfd_check_args(dem, out, w, h, "rdgpu_dinf_flowdirs");                                                    \
      host_dem_to_f32<T>(dem, w, h, "host.f32out", out, 1,                                                      \
                         [&](const T *d, float *o) { dinf_flowdirs_device<T>(d, nodata, w, h, o, nullptr); });  \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fm_tarboton_##SUF(const T *dem, T nodata, int w, int h, float *props9) {                 \
    return guarded([&] {                                                                                        \
      mfd_check_args(dem, props9, w, h, "rdgpu_fm_tarboton");                                                   \
      host_dem_to_f32<T>(dem, w, h, "host.props", props9, 9, [&](const T *d, float *p) {                        \
        fm_tarboton_device<T>(tarboton_device<T>, d, nodata, w, h, p, nullptr);                                 \
      });                                                                                                       \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fa_tarboton_dev_##SUF(const T *d_dem, T nodata, int w, int h, double *d_accum, void *st) { \
    return guarded([&] {                                                                                        \
      mfd_check_args(d_dem, d_accum, w, h, "rdgpu_fa_tarboton");                                                \
      fa_tarboton_device<T>(tarboton_device<T>, d_dem, nodata, w, h, d_accum, (hipStream_t)st);                 \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fa_tarboton_##SUF(const T *dem, T nodata, int w, int h, double *accum) {                 \
    return guarded([&] {                                                                                        \
      mfd_check_args(dem, accum, w, h, "rdgpu_fa_tarboton");                                                    \
      host_dem_accum<T>(dem, w, h, accum, [&](const T *d, double *da) {                                         \
        fa_tarboton_device<T>(tarboton_device<T>, d, nodata, w, h, da, nullptr);                                \
      });                                                                                                       \
    });                                                                                                         \
  }
RD_MFD_API(u8, uint8_t)
RD_MFD_API(i16, int16_t)
RD_MFD_API(u16, uint16_t)
RD_MFD_API(i32, int32_t)
RD_MFD_API(u32, uint32_t)
RD_MFD_API(f32, float)
RD_MFD_API(f64, double)
RD_MFD_API(i8, int8_t)

// D-infinity across flats: FM_Tarboton / FA_Tarboton with the cells of drainable flats patched from the flat mask
#define RD_MFD_FLATS_API(SUF, T)                                                                                \
  extern "C" int rdgpu_fm_tarboton_flats_dev_##SUF(const T *d_dem, T nodata, int w, int h, float *d_props9, void *st) { \
    return guarded([&] {                                                                                        \
      mfd_check_args(d_dem, d_props9, w, h, "rdgpu_fm_tarboton_flats", FLATS_MAX_CELLS);                        \
      fm_tarboton_device<T>(tarboton_flats_device<T>, d_dem, nodata, w, h, d_props9, (hipStream_t)st);          \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fm_tarboton_flats_##SUF(const T *dem, T nodata, int w, int h, float *props9) {           \
    return guarded([&] {                                                                                        \
      mfd_check_args(dem, props9, w, h, "rdgpu_fm_tarboton_flats", FLATS_MAX_CELLS);                            \
      host_dem_to_f32<T>(dem, w, h, "host.props", props9, 9, [&](const T *d, float *p) {                        \
        fm_tarboton_device<T>(tarboton_flats_device<T>, d, nodata, w, h, p, nullptr);                           \
      });                                                                                                       \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fa_tarboton_flats_dev_##SUF(const T *d_dem, T nodata, int w, int h, double *d_accum, void *st) { \
    return guarded([&] {                                                                                        \
      mfd_check_args(d_dem, d_accum, w, h, "rdgpu_fa_tarboton_flats", FLATS_MAX_CELLS);                         \
      fa_tarboton_device<T>(tarboton_flats_device<T>, d_dem, nodata, w, h, d_accum, (hipStream_t)st);           \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fa_tarboton_flats_##SUF(const T *dem, T nodata, int w, int h, double *accum) {           \
    return guarded([&] {                                                                                        \
      mfd_check_args(dem, accum, w, h, "rdgpu_fa_tarboton_flats", FLATS_MAX_CELLS);                             \
      host_dem_accum<T>(dem, w, h, accum, [&](const T *d, double *da) {                                         \
        fa_tarboton_device<T>(tarboton_flats_device<T>, d, nodata, w, h, da, nullptr);                          \
      });                                                                                                       \
    });                                                                                                         \
  }
RD_MFD_FLATS_API(u8, uint8_t)
RD_MFD_FLATS_API(i8, int8_t)
RD_MFD_FLATS_API(u16, uint16_t)
RD_MFD_FLATS_API(i16, int16_t)
RD_MFD_FLATS_API(u32, uint32_t)
RD_MFD_FLATS_API(i32, int32_t)
RD_MFD_FLATS_API(f32, float)
RD_MFD_FLATS_API(f64, double)

extern "C" int rdgpu_dinf_flats_get_stats(rdgpu_dinf_flats_stats *out) {
  return guarded([&] {
    if (!out) throw Error(RDGPU_ERR_ARG, "rdgpu_dinf_flats_get_stats: null pointer");
    *out = rdgpu_dinf_flats_stats{0, 0, 0, 0};
    FlatsCounts &fc = g_flats_counts;
    if (!fc.host) return;   // no call on this thread yet
    if (fc.pending) {
      int cur = 0;
      RD_HIP(hipGetDevice(&cur));
      if (cur != fc.device) RD_HIP(hipSetDevice(fc.device));
      const hipError_t e = hipStreamSynchronize(fc.stream);
      if (cur != fc.device) (void)hipSetDevice(cur);
      RD_HIP(e);
      fc.pending = false;
    }
    out->noflow_cells = fc.host[FC_NOFLOW];
    out->patched_cells = fc.host[FC_PATCHED];
    out->fallback_cells = fc.host[FC_FALLBACK];
    out->unresolved_cells = fc.host[FC_UNRESOLVED];
  });
}

#define RD_MFD2_API(SUF, T)                                                                                    \
  extern "C" int rdgpu_fm_mfd_dev_##SUF(const T *d_dem, T nodata, int w, int h, int method, double xparam,      \
                                        float *d_props9, void *st) {                                            \
    return guarded([&] {                                                                                        \
      mfd_check_args(d_dem, d_props9, w, h, "rdgpu_fm_mfd");                                                    \
      check_mfd_method(method);                                                                                 \
      fm_mfd_device<T>(d_dem, nodata, w, h, method, xparam, d_props9, (hipStream_t)st);                         \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fm_mfd_##SUF(const T *dem, T nodata, int w, int h, int method, double xparam,            \
                                    float *props9) {                                                            \
    return guarded([&] {                                                                                        \
      mfd_check_args(dem, props9, w, h, "rdgpu_fm_mfd");                                                        \
      check_mfd_method(method);                                                                                 \
      host_dem_to_f32<T>(dem, w, h, "host.props", props9, 9, [&](const T *d, float *p) {                        \
        fm_mfd_device<T>(d, nodata, w, h, method, xparam, p, nullptr);                                          \
      });                                                                                                       \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fa_mfd_dev_##SUF(const T *d_dem, T nodata, int w, int h, int method, double xparam,      \
                                        double *d_accum, void *st) {                                            \
    return guarded([&] {                                                                                        \
      mfd_check_args(d_dem, d_accum, w, h, "rdgpu_fa_mfd");                                                     \
      check_mfd_method(method);                                                                                 \
      fa_mfd_device<T>(d_dem, nodata, w, h, method, xparam, d_accum, (hipStream_t)st);                          \
    });                                                                                                         \
  }                                                                                                             \
  extern "C" int rdgpu_fa_mfd_##SUF(const T *dem, T nodata, int w, int h, int method, double xparam,            \
                                    double *accum) {                                                            \
    return guarded([&] {                                                                                        \
      mfd_check_args(dem, accum, w, h, "rdgpu_fa_mfd");                                                         \
      check_mfd_method(method);                                                                                 \
      host_dem_accum<T>(dem, w, h, accum, [&](const T *d, double *da) {                                         \
        fa_mfd_device<T>(d, nodata, w, h, method, xparam, da, nullptr);                                         \
      });                                                                                                       \
    });                                                                                                         \
  }
RD_MFD2_API(u8, uint8_t)
RD_MFD2_API(i16, int16_t)
RD_MFD2_API(u16, uint16_t)
RD_MFD2_API(i32, int32_t)
RD_MFD2_API(u32, uint32_t)
RD_MFD2_API(f32, float)
RD_MFD2_API(f64, double)
RD_MFD2_API(i8, int8_t)

// FlowAccumulation(const Array3D<float>&, Array2D<double>&), methods/flow_accumulation_generic.hpp:33-100
extern "C" int rdgpu_flow_accumulation_dev_f64(const float *d_props9, int w, int h, double *d_accum, void *st) {
  return guarded([&] {
    mfd_check_args(d_props9, d_accum, w, h, "rdgpu_flow_accumulation");
    mfd_accumulate<PropsAcc>(PropsAcc{d_props9}, w, h, d_accum, (hipStream_t)st);
  });
}
extern "C" int rdgpu_flow_accumulation_f64(const float *props9, int w, int h, double *accum) {
  return guarded([&] {
    mfd_check_args(props9, accum, w, h, "rdgpu_flow_accumulation");
    const size_t n = (size_t)w * h;
    HostStage st;
    const float *dp = st.in("host.props", props9, n * 9);
    double *da = st.inout("host.area", accum, n);
    mfd_accumulate<PropsAcc>(PropsAcc{dp}, w, h, da, nullptr);
    st.finish();
  });
}
extern "C" int rdgpu_flow_accumulation_rounds(uint32_t *rounds) {
  if (!rounds) return RDGPU_ERR_ARG;
  *rounds = g_mfd_rounds;
  return RDGPU_OK;
}
