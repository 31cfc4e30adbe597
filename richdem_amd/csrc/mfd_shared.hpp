// mfd_shared.hpp -- what the engines on D-infinity / MFD proportions share: the neighbour numbering, the two proportions
// accessors, the ready-flag compaction and the compact D-infinity form from a DEM (mfd.hip: accumulation;
// mfd_distance.hip: distance and drop down to the stop cells).
#pragma once

#include "common.hpp"

#include <algorithm>

namespace rdgpu {

constexpr int NTHR = 256;
static inline uint32_t sgrid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u); }

__device__ __forceinline__ int mdx(int n) { return (n == 1 || n == 2 || n == 8) ? -1 : (n >= 4 && n <= 6) ? 1 : 0; }
__device__ __forceinline__ int mdy(int n) { return (n >= 2 && n <= 4) ? -1 : (n >= 6 && n <= 8) ? 1 : 0; }

// ------------------------------------------------------------------------------------------
// proportions accessors
// ------------------------------------------------------------------------------------------
struct PropsAcc {   // the reference's Array3D<float>
  const float *props;
  __device__ __forceinline__ bool nodata(uint64_t c) const { return props[9 * c] == -2.0f; }
  __device__ __forceinline__ float share(uint64_t c, int n) const { return props[9 * c + n]; }
};
struct DinfAcc {    // compact D-infinity form
  const uint8_t *rcv;
  const float *sh1, *sh2;
  __device__ __forceinline__ bool nodata(uint64_t c) const { return rcv[c] == 255; }
  __device__ __forceinline__ float share(uint64_t c, int n) const {
    const int rr = rcv[c], r = rr & 0xF;
    if (rr == 255 || r < 1 || r > 8) return -1.0f;
    if (n == r) return sh1[c];
    if ((rr & 0x10) && n == (r == 8 ? 1 : r + 1)) return sh2[c];
    return -1.0f;
  }
};

// FM_Tarboton in compact form into workspace planes (mfd.hip): 5 B/cell, the 36 B/cell array is never materialised
template <class T>
DinfAcc tarboton_device(const T *d_z, T nodata, int w, int h, hipStream_t s);

// ---- ready flags -> work list (count / scan / fill; flags are cleared) ------------------------------
constexpr int CPB = 4096;
static __global__ __launch_bounds__(NTHR) void k_rdy_count(const uint8_t *__restrict__ f, uint64_t n, uint32_t *counts) {
  __shared__ uint32_t ws[NTHR / 64];
  const uint64_t base = (uint64_t)blockIdx.x * CPB;
  uint32_t cnt = 0;
#pragma unroll 4
  for (int j = 0; j < CPB / NTHR; j++) {
    const uint64_t c = base + (uint64_t)j * NTHR + threadIdx.x;
    if (c < n && f[c]) cnt++;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
static __global__ __launch_bounds__(1024) void k_rdy_scan(uint32_t *counts, uint32_t m, uint32_t *total) {
  __shared__ uint32_t part[1024];
  const uint32_t chunk = (m + 1023u) / 1024u;
  const uint32_t lo = threadIdx.x * chunk, hi = min(lo + chunk, m);
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i++) s += counts[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    uint32_t v = (threadIdx.x >= (uint32_t)o) ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t v = counts[i];
    counts[i] = run;
    run += v;
  }
  if (threadIdx.x == 1023) *total = part[1023];
}
static __global__ __launch_bounds__(NTHR) void k_rdy_fill(uint8_t *f, uint64_t n, const uint32_t *__restrict__ offsets,
                                                          uint32_t *__restrict__ out) {
  __shared__ uint32_t ws[NTHR / 64];
  const uint64_t base = (uint64_t)blockIdx.x * CPB;
  uint32_t run = offsets[blockIdx.x];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = 0; j < CPB / NTHR; j++) {
    const uint64_t c = base + (uint64_t)j * NTHR + threadIdx.x;
    const bool hit = c < n && f[c];
    if (hit) f[c] = 0;
    const unsigned long long bal = __ballot(hit);
    const uint32_t rank = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) ws[wv] = __popcll(bal);
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NTHR / 64; k++) {
      const uint32_t v = ws[k];
      if (k < wv) woff += v;
      tot += v;
    }
    if (hit) out[run + woff + rank] = (uint32_t)c;
    run += tot;
    __syncthreads();
  }
}

static inline void check_dims(int w, int h, const char *who) {
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, std::string(who) + ": width and height must be positive");
  if ((uint64_t)w * (uint64_t)h > 0xFFFF0000ull) throw Error(RDGPU_ERR_ARG, std::string(who) + ": raster too large");
}

template <class T>
static void host_dem(const T *dem, int w, int h, T **d) {
  const size_t n = (size_t)w * h;
  *d = Workspace::get().buf<T>("host.dem", n);
  RD_HIP(hipMemcpy(*d, dem, n * sizeof(T), hipMemcpyHostToDevice));
}

}  // namespace rdgpu
