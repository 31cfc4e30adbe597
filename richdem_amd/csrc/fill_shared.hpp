// fill_shared.hpp -- the pieces of the fill engine (fill.hip) that other files of the library build on: the buffers that
// outlive the local phase, the union-find over basins, and the kernel that finds the cell a pocket is flooded from
// (max_dep in fill.hip, the depression inventory in depressions.hip).
#pragma once

#include "common.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace rdgpu {

constexpr int NTHR = 256;     // 4 wavefronts

static inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// Device buffers that outlive the local phase.
struct FillBuffers {
  uint32_t *lab = nullptr, *cur = nullptr, *acc = nullptr, *tid = nullptr;
  uint32_t B = 0;
  bool trivial = false;   // nothing to raise (no interior, or no pits)
  // the compact-label local phase of a row-block shard (r04): no 32-bit label per cell, but the 16-bit slots, the tiles'
  // node bases and counts, node -> basin (curN), and per node its level (lvl) and watershed terminal (nodeW)
  bool compact = false;
  uint16_t *lab16 = nullptr;
  uint32_t *tile_base = nullptr, *tile_count = nullptr, *curN = nullptr, *lvl = nullptr, *nodeW = nullptr;
  unsigned long long *counters = nullptr;
  uint32_t rcap = 0, nstripes = 0, nnmax = 0;
};

struct BufAlloc {   // where persistent buffers come from: the shared workspace, or owned hipMalloc
  bool owned;
  std::vector<void *> *owned_list;
  bool shard_ws = false;   // workspace buffers under their own names ("shard." + name): the one cached shard
  template <class U>
  U *get(const char *name, size_t count) {
    if (!owned && shard_ws) return Workspace::get().buf<U>((std::string("shard.") + name).c_str(), count);
    if (!owned) return Workspace::get().buf<U>(name, count);
    void *p = nullptr;
    RD_HIP(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(U)));
    owned_list->push_back(p);
    return static_cast<U *>(p);
  }
};

inline void check_fill_args(const void *p, int w, int h, int topology) {
  if (!p) throw Error(RDGPU_ERR_ARG, "rdgpu_fill: null DEM pointer");
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, "rdgpu_fill: width and height must be positive");
  if (topology != 8 && topology != 4) throw Error(RDGPU_ERR_ARG, "rdgpu_fill: topology must be 8 or 4");  // depressions.hpp:19-20
}

// Phases 1-4 of the fill (descent forest, basins, Boruvka rounds) of a whole raster on workspace buffers: fb.lab[cell] =
// basin (fb.B = the outside), fb.acc[basin] = the key of its filled level; fb.trivial: nothing to raise.  Defined in fill.hip
// for u8, i8, i16, u16, i32, u32 and f32.  (It waits for the stream a few times: the round loop is driven from the host.)
template <class T>
void fill_local_phase_plain(const T *d_z, int w, int h, int topology, FillBuffers &fb, hipStream_t s);

// The depression inventory (depressions.hip) of an f64 raster runs on its dense value ranks (fill64.hip):
// depressions_f64_device ranks the raster and hands over to depressions_on_ranks (d_uniq[rank] = the value's 64-bit key).
void depressions_f64_device(const double *d_z, int w, int h, int topology, int32_t *d_labels, rdgpu_depression *d_table,
                            uint32_t capacity, uint32_t *d_count, hipStream_t s);
void depressions_on_ranks(const uint32_t *d_rk, const uint64_t *d_uniq, const double *d_vals, int w, int h, int topology,
                          int32_t *d_labels, rdgpu_depression *d_table, uint32_t capacity, uint32_t *d_count, hipStream_t s);

// ---- union-find over basins (pockets; see the comment above k_md_pockets in fill.hip) ----------------------------------
__device__ __forceinline__ uint32_t md_find(uint32_t *par, uint32_t x) {
  uint32_t p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return x;
}
__device__ __forceinline__ void md_unite(uint32_t *par, uint32_t a, uint32_t b) {
  for (;;) {
    a = md_find(par, a);
    b = md_find(par, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }   // hook the larger root under the smaller: acyclic under any interleaving
    const uint32_t old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

template <class T, int TOPO, int PASS>
__global__ __launch_bounds__(NTHR) void k_md_spawn(const T *__restrict__ z, const uint32_t *__restrict__ lab,
                                                   const uint32_t *__restrict__ acc, uint32_t *par, uint32_t *spawn, int w,
                                                   int h, uint32_t B) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t b = lab[c];
    const uint32_t kz = Key32<T>::to(z[c]);
    if (b != B && acc[b] > kz) continue;   // raised cells are flooded, they do not flood
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    uint32_t first = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (TOPO == 4 && (k & 1)) continue;
      const int dx[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dy[8] = {0, -1, -1, -1, 0, 1, 1, 1};
      const int xx = x + dx[k], yy = y + dy[k];
      if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
      const size_t q = (size_t)yy * w + xx;
      const uint32_t bq = lab[q];
      if (bq == B) continue;
      const uint32_t L = acc[bq];
      if (L != kz || !(L > Key32<T>::to(z[q]))) continue;   // a raised neighbour filled to exactly this cell's elevation
      const uint32_t r = md_find(par, bq);
      if (PASS == 0) {
        if ((uint32_t)c < __hip_atomic_load(&spawn[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&spawn[r], (uint32_t)c);
      } else if (__hip_atomic_load(&spawn[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)c) {
        if (first == 0xFFFFFFFFu) first = r;
        else md_unite(par, first, r);        // the pockets this cell floods are one run
      }
    }
  }
}

}  // namespace rdgpu
