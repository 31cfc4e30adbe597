// bucketfill.hip -- BucketFillFromEdges on the device (include/rdgpu.h, "bucket fill from the edges"; DESIGN.md section
// 3e).  Reference counterpart: misc/misc_methods.hpp (BucketFill, BucketFillFromEdges): a queue flood from the border
// cells over the cells with check == check_value that are not yet set.  Here the ELIGIBLE cells are labelled by a
// union-find in a fixed number of launches -- four, whatever the shape of the region; rounds of propagation would need as
// many launches as the longest channel has cells:
//   k_bf_init    parent[c] = the head of c's horizontal run of eligible cells inside its 64-cell wavefront segment (a
//                ballot and bit operations), BF_NONE on cells that are not eligible.
//   k_bf_union   unions of run heads across segment seams and with the row above (N; NW and NE under D8): the larger
//                root is hooked under the smaller by a compare-and-swap, retried from where the swap found it.
//   k_bf_mark    every eligible cell is pointed at its root; every eligible ring cell sets bit 31 of its root's word
//                (free below 2^31-65536 cells).
//   k_bf_write   mask[c] = 1 where the root's word carries the bit; the count of bytes set.
// Words other workgroups write during a launch are read and written with agent-scope atomics (the per-XCD L2s are not
// coherent).  A parent is always a smaller index than its child, so every walk ends and no thread waits for another.
#include "common.hpp"
#include "fill_shared.hpp"

namespace rdgpu {

constexpr uint32_t BF_NONE = 0xFFFFFFFFu, BF_MARK = 0x80000000u, BF_IDX = 0x7FFFFFFFu;

__device__ __forceinline__ uint32_t bf_ld(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void bf_st(uint32_t *p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the run heads of one 64-cell segment: an eligible cell whose left neighbour is not eligible, lies in the row before
// (rowstart: the cells with x == 0) or in the segment before
__device__ __forceinline__ unsigned long long bf_heads(unsigned long long elig, unsigned long long rowstart) {
  return elig & ~((elig << 1) & ~rowstart);
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_bf_init(const T *__restrict__ check, const uint8_t *__restrict__ mask,
                                                  uint32_t *__restrict__ par, int w, uint64_t n, T value) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  const int lane = (int)(threadIdx.x & 63u);
  for (uint64_t base = (uint64_t)blockIdx.x * NTHR + (threadIdx.x & ~63u); base < n; base += stride) {   // (wave-uniform)
    const uint64_t c = base + lane;
    const bool valid = c < n;
    const bool e = valid && check[c] == value && mask[c] == 0;
    const unsigned long long eb = __ballot(e), rs = __ballot(valid && c % (uint64_t)w == 0);
    if (!valid) continue;
    const unsigned long long hd = bf_heads(eb, rs) & (~0ull >> (63 - lane));   // the heads at or before this lane
    par[c] = e ? (uint32_t)base + (uint32_t)(63 - __builtin_clzll(hd | 1ull)) : BF_NONE;
  }
}

// the root of x (k_bf_union: no word carries BF_MARK yet), halving the path on the way: x is not a root when its word is
// rewritten and never becomes one again, and the new value is one of its ancestors whatever others have written meanwhile
__device__ __forceinline__ uint32_t bf_find(uint32_t *par, uint32_t x) {
  uint32_t p = bf_ld(&par[x]);
  while (p != x) {
    const uint32_t g = bf_ld(&par[p]);
    if (g != p) bf_st(&par[x], g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void bf_union(uint32_t *par, uint32_t a, uint32_t b) {
  if (bf_ld(&par[a]) == bf_ld(&par[b])) return;   // (an open sea: most unions find their two ends under one root)
  for (;;) {
    a = bf_find(par, a);
    b = bf_find(par, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    uint32_t seen = a;
    if (__hip_atomic_compare_exchange_strong(&par[a], &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return;
    a = seen;   // somebody hooked a first: go on from the parent it was given (smaller than a)
  }
}

template <int TOPO>
__global__ __launch_bounds__(NTHR) void k_bf_union(uint32_t *par, int w, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  const int lane = (int)(threadIdx.x & 63u);
  for (uint64_t base = (uint64_t)blockIdx.x * NTHR + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint64_t c = base + lane;
    const bool valid = c < n;
    const bool e = valid && bf_ld(&par[c]) != BF_NONE;
    const int x = valid ? (int)(c % (uint64_t)w) : 1;
    const unsigned long long eb = __ballot(e), rs = __ballot(valid && x == 0);
    if (!e) continue;
    const bool head = (bf_heads(eb, rs) >> lane) & 1ull;
    const uint32_t cc = (uint32_t)c;
    // the run goes on in the segment before
    if (lane == 0 && x > 0 && bf_ld(&par[c - 1]) != BF_NONE) bf_union(par, cc, cc - 1u);
    if (c < (uint64_t)w) continue;   // (the first row)
    // the row above: one union per run up there that touches this run, made by the first cell of the contact
    const uint32_t u = cc - (uint32_t)w;
    const bool eu = bf_ld(&par[u]) != BF_NONE;
    if (TOPO == 4) {
      if (eu && (head || bf_ld(&par[u - 1u]) == BF_NONE)) bf_union(par, cc, u);   // (not a head: x > 0)
    } else {
      if (head) {
        if (eu) bf_union(par, cc, u);
        else if (x > 0 && bf_ld(&par[u - 1u]) != BF_NONE) bf_union(par, cc, u - 1u);
      }
      if (!eu && x + 1 < w && bf_ld(&par[u + 1u]) != BF_NONE) bf_union(par, cc, u + 1u);
    }
  }
}

__global__ __launch_bounds__(NTHR) void k_bf_mark(uint32_t *par, int w, int h) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t p = bf_ld(&par[c]);
    if (p == BF_NONE) continue;
    uint32_t r = (uint32_t)c, word = p;
    while ((word & BF_IDX) != r) {
      r = word & BF_IDX;
      word = bf_ld(&par[r]);
    }
    if (r != (uint32_t)c && p != r) bf_st(&par[c], r);   // (c is no root: nobody marks its word)
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    if ((x == 0 || y == 0 || x == w - 1 || y == h - 1) && !(word & BF_MARK))
      __hip_atomic_fetch_or(&par[r], BF_MARK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(NTHR) void k_bf_write(const uint32_t *__restrict__ par, uint8_t *__restrict__ mask, uint64_t n,
                                                   unsigned long long *filled) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  uint32_t mine = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    uint32_t word = par[c];
    if (word == BF_NONE) continue;
    uint32_t r = (uint32_t)c;
    while ((word & BF_IDX) != r) {
      r = word & BF_IDX;
      word = par[r];
    }
    if (word & BF_MARK) {
      mask[c] = 1;
      mine++;
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(filled, (unsigned long long)mine);
}

static void check_bucket_args(const void *check, int w, int h, int topology, const void *mask) {
  if (!check || !mask) throw Error(RDGPU_ERR_ARG, "rdgpu_bucket_fill_from_edges: null check or mask pointer");
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, "rdgpu_bucket_fill_from_edges: width and height must be positive");
  if (topology != 8 && topology != 4) throw Error(RDGPU_ERR_ARG, "rdgpu_bucket_fill_from_edges: topology must be 8 or 4");
  if ((uint64_t)w * (uint64_t)h > 0x7FFF0000ull)
    throw Error(RDGPU_ERR_ARG, "rdgpu_bucket_fill_from_edges: raster has more than 2^31-65536 cells");
}

template <class T>
static void bucket_device(const T *d_check, int w, int h, int topology, T value, uint8_t *d_mask, uint64_t *d_filled,
                          hipStream_t s) {
  check_bucket_args(d_check, w, h, topology, d_mask);
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  const uint32_t rgrid = (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u);
  uint32_t *par = ws.buf<uint32_t>("bucketfill.parent", n);
  unsigned long long *filled = d_filled ? reinterpret_cast<unsigned long long *>(d_filled)
                                        : ws.buf<unsigned long long>("bucketfill.filled", 1);
  RD_HIP(hipMemsetAsync(filled, 0, sizeof(unsigned long long), s));
  RD_LAUNCH("bucketfill.init", (k_bf_init<T>), dim3(rgrid), dim3(NTHR), 0, s, d_check, (const uint8_t *)d_mask, par, w, n, value);
  if (topology == 8) RD_LAUNCH("bucketfill.union", (k_bf_union<8>), dim3(rgrid), dim3(NTHR), 0, s, par, w, n);
  else RD_LAUNCH("bucketfill.union", (k_bf_union<4>), dim3(rgrid), dim3(NTHR), 0, s, par, w, n);
  RD_LAUNCH("bucketfill.mark", k_bf_mark, dim3(rgrid), dim3(NTHR), 0, s, par, w, h);
  RD_LAUNCH("bucketfill.write", k_bf_write, dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)par, d_mask, n, filled);
}

template <class T>
static void bucket_host(const T *check, int w, int h, int topology, T value, uint8_t *mask, uint64_t *filled) {
  check_bucket_args(check, w, h, topology, mask);
  const size_t n = (size_t)w * h;
  HostStage st;
  const T *d = st.in("host.dem", check, n);
  uint8_t *dm = st.inout("bucketfill.host.mask", mask, n);
  uint64_t *df = st.out("bucketfill.host.filled", filled, 1);
  bucket_device<T>(d, w, h, topology, value, dm, df, nullptr);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_BUCKET_API(SUF, T)                                                                                         \
  extern "C" int rdgpu_bucket_fill_from_edges_##SUF(const T *check, int w, int h, int topology, T check_value,        \
                                                    uint8_t *mask, uint64_t *filled) {                                \
    return guarded([&] { bucket_host<T>(check, w, h, topology, check_value, mask, filled); });                        \
  }                                                                                                                   \
  extern "C" int rdgpu_bucket_fill_from_edges_dev_##SUF(const T *d_check, int w, int h, int topology, T check_value,  \
                                                        uint8_t *d_mask, uint64_t *d_filled, void *stream) {          \
    return guarded([&] { bucket_device<T>(d_check, w, h, topology, check_value, d_mask, d_filled, (hipStream_t)stream); }); \
  }
RD_BUCKET_API(u8, uint8_t)
RD_BUCKET_API(i8, int8_t)
RD_BUCKET_API(i16, int16_t)
RD_BUCKET_API(u16, uint16_t)
RD_BUCKET_API(i32, int32_t)
RD_BUCKET_API(u32, uint32_t)
RD_BUCKET_API(f32, float)
RD_BUCKET_API(f64, double)
RD_BUCKET_API(i64, int64_t)
RD_BUCKET_API(u64, uint64_t)
