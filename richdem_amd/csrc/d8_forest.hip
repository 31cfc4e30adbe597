// d8_forest.hip -- the two kernels the key-pushing engines on the D8 link forest launch as they are (extreme.hip,
// longest.hip).  d8_forest.hpp explains the forest.
#include "d8_forest.hpp"

namespace rdgpu {

struct ForestLinkTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(4)));   // staged directions (tile_front.hpp)
  uint16_t lp[LT * LPS];                               // per cell: a cell further down its in-tile path
};

__global__ __launch_bounds__(NTHR, 5) void k_forest_links(const uint8_t *__restrict__ dirs, uint8_t nodata, int w, int h,
                                                          uint32_t tilesX, uint32_t ntiles, uint32_t *__restrict__ nxt0) {
  __shared__ ForestLinkTile T;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, T.sd);
  __syncthreads();
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t p[FOREST_RPT];
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int kind = forest_link(T.sd, nodata, lx, ly, tx, ty);
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : (self | FOREST_END);
    T.lp[self] = (uint16_t)p[j];
  }
  __syncthreads();
  forest_jump_sync(T.lp, p, lx, ly0);
  // the node a path that ENTERS the tile at a border cell leaves it to, one border cell per thread (a pointer without
  // FOREST_END after the last trip: into a loop inside the tile)
  const int slot = (int)threadIdx.x;
  uint32_t word = FOREST_NONE;
  if (slot < BORDER_SLOTS) {
    int bx, by, tx, ty;
    border_cell(slot, bx, by);
    const uint32_t rp = T.lp[by * LPS + bx], root = rp & FOREST_CELL;
    if (rp & FOREST_END) {
      const int ry = (int)root / LPS, rx = (int)root - ry * LPS;
      if (forest_link(T.sd, nodata, rx, ry, tx, ty) == 2) word = tile_node(x0 + tx, y0 + ty, tilesX);
    }
  }
  nxt0[(size_t)t * TILE_SLOTS + slot] = word;
}

template <class K>
__global__ __launch_bounds__(NTHR) void k_forest_round(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, K *nval,
                                                       uint32_t nnodes, const uint32_t *__restrict__ gate, uint32_t *flag_out) {
  if (*gate == 0) return;
  bool flag = false;
  for (uint32_t i = blockIdx.x * NTHR + threadIdx.x; i < nnodes; i += gridDim.x * NTHR) {   // (nnodes: a multiple of NTHR)
    const uint32_t n = src[i];
    uint32_t n2 = FOREST_NONE;
    if (n < nnodes) {
      n2 = src[n];
      const K k = __hip_atomic_load(&nval[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k != 0) flag |= atomicMax(&nval[n], k) < k;
    }
    dst[i] = n2;
  }
  if (__any(flag) && (threadIdx.x & 63) == 0) *flag_out = 1;
}
template __global__ void k_forest_round<unsigned long long>(const uint32_t *__restrict__, uint32_t *__restrict__, unsigned long long *,
                                                            uint32_t, const uint32_t *__restrict__, uint32_t *);
template __global__ void k_forest_round<uint32_t>(const uint32_t *__restrict__, uint32_t *__restrict__, uint32_t *, uint32_t,
                                                  const uint32_t *__restrict__, uint32_t *);

}  // namespace rdgpu
