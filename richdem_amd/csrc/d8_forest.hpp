// d8_forest.hpp -- what the engines on the D8 link forest share (upslope.hip, streams.hip, flowpath.hip, extreme.hip,
// longest.hip; accum.hip for the size check).  The node numbering itself is in tile_front.hpp.
//
// The forest.  Every 64 x 64 tile is worked on alone; what crosses tiles goes over the NODES, one per border cell (256
// slots per tile).  A node's link is the node of the neighbouring tile's border cell that the path entering the tile at
// this border cell leaves it to, or FOREST_NONE: the path ends in the tile or runs into a loop inside it.
//
// Tile pointers.  Inside a tile a cell holds a 16-bit pointer to a cell further down its in-tile path.  A FLAG
// (FOREST_END), not "points to itself", marks that the cell pointed to is the END of the path: three hops round a loop of
// three cells come back to the start.  forest_jump_sync doubles the pointers SYNCHRONOUSLY (read, barrier, store), so
// that every cell covers the same distance: after trip r a pointer without the flag covers exactly 2^(r+1) cells, and
// what has no end after FOREST_JUMPS trips runs round a loop inside the tile -- the cell it has reached lies ON the loop.
// (upslope.hip and flowpath.hip jump asynchronously, two hops in place; their race arguments are their own.)
//
// Pushing (extreme.hip, longest.hip, streams.hip).  A word per cell -- a mark, a key, an index -- that only grows is
// closed DOWNSTREAM: first inside the tile (forest_close), the exits raise the node they flow to (forest_push_exits), then
// over the nodes (k_forest_round), then in the tile again with the node words of its border slots joining in.  The words
// must be pushed (a cell does not know its children's pointers), so the pull-style rounds of upslope.hip and flowpath.hip
// do not fit.  Every word that changes is changed by one idempotent update (an atomic maximum, a byte store of 1); the
// only words too wide for that are the doubled pointers: in LDS they double synchronously, over the nodes from one buffer
// into the other.
//
// Termination of a closure.  Round r: every cell reads the pointer q = lp[p] of the cell p it points to, barrier, pushes
// its word to p, stores q.  Before round r a pointer covers 2^r links (or stops at the path's end), and the cells holding
// a word >= K form, per source of such a word, a run along the path that starts at the source and is at least 2^r - 1 links
// long (exactly that without the races: pushes of one round race with each other, and a word raised early in a round may
// be pushed on in the same round.  That is harmless: words only grow, a push is idempotent, and what arrives early flows
// there anyway).  A round pushes every run on by 2^r.  If a run ended at a cell x whose successor holds less, the cell
// 2^r - 1 links above x is in the run and pushes to that successor: the round raises a word.  So a round that raises
// nothing proves the closure, for every level set of the word at once.  On a direction loop the equal jumps rotate it;
// FOREST_JUMPS = 12 rounds cover 4095 links, every path and every loop a tile can hold, and ceil(log2(nodes)) + 1 rounds
// (forest_rounds) every chain or loop of nodes.  Nothing is special-cased for loops.
#pragma once

#include "common.hpp"
#include "tile_front.hpp"

#include <cmath>
#include <string>

namespace rdgpu {

constexpr uint32_t FOREST_NONE = 0xFFFFFFFFu;   // a node's link: none
// a tile pointer: the table index of a cell (ly * LPS + lx) | FOREST_END when that cell is the END of the path
constexpr uint32_t FOREST_END = 0x8000u, FOREST_CELL = 0x7FFFu;
constexpr int FOREST_RPT = LT / 4;     // rows (cells) per thread of a tile pass
constexpr int FOREST_JUMPS = 12;       // 2^12 = 4096 cells: any path or loop inside a tile

// ---- device functions (in the header: the library is built without relocatable device code) ----------------------------
// the link of the cell (lx, ly) of the staged tile: -1 the cell does not participate (NoData, or outside the raster: staged
// as NoData), 0 none (its tree ends here: no direction, or a target that is off the raster or NoData), 1 to (tx, ty) inside
// the tile, 2 to (tx, ty) in another tile.  These are the links of the flow-path engine without a mask.
__device__ __forceinline__ int forest_link(const uint8_t *sd, uint8_t nodata, int lx, int ly, int &tx, int &ty) {
  const uint32_t d = sd[(ly + 1) * SDW + SDO + lx];
  tx = lx; ty = ly;
  if (d == nodata) return -1;
  if (d - 1u >= 8u) return 0;
  tx = lx + d8dx((int)d); ty = ly + d8dy((int)d);
  if (sd[(ty + 1) * SDW + SDO + tx] == nodata) return 0;
  return (tx >= 0 && tx < LT && ty >= 0 && ty < LT) ? 1 : 2;
}

// Doubles the tile pointers in lp synchronously; every thread holds the pointers of its own cells (lx, ly0 + 4 j) in p[]
// (an end: self | FOREST_END).  To be called behind a barrier; ends behind one.
__device__ __forceinline__ void forest_jump_sync(uint16_t *lp, uint32_t (&p)[FOREST_RPT], int lx, int ly0) {
  uint32_t q[FOREST_RPT];
#pragma unroll 1
  for (int it = 0; it < FOREST_JUMPS; it++) {
    bool moving = false;
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) q[j] = (p[j] & FOREST_END) ? p[j] : lp[p[j]];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      p[j] = q[j];
      moving |= !(q[j] & FOREST_END);
      lp[(ly0 + 4 * j) * LPS + lx] = (uint16_t)q[j];
    }
    if (!__syncthreads_or(moving)) break;
  }
}

// Closes the cells' words down the pointers in lp (no end flag here: an end cell points at itself), which every thread
// holds in p[] for its own cells: round r pushes by 2^r; a round that raises nothing has closed them.  push(self, to)
// pushes the word of the cell `self` to the cell `to` and tells whether that raised it.  any: this thread has a word to
// push; returns whether any thread of the block has (if none, nothing is done).  Ends behind a barrier.
template <class Push>
__device__ __forceinline__ bool forest_close(uint16_t *lp, uint32_t (&p)[FOREST_RPT], bool any, int lx, int ly0, Push push) {
  if (!__syncthreads_or(any)) return false;
  uint32_t q[FOREST_RPT];
#pragma unroll 1
  for (int it = 0; it < FOREST_JUMPS; it++) {
    bool fresh = false;
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) q[j] = lp[p[j]];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      const uint32_t self = (uint32_t)((ly0 + 4 * j) * LPS + lx);
      fresh |= push(self, p[j]);
      lp[self] = (uint16_t)q[j];
    }
    if (!__syncthreads_or(fresh)) break;
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) p[j] = q[j];
  }
  return true;
}
// the push of a key or an index (0: none) in the LDS table W: one ds_max_rtn_u64 / _u32
template <class K>
__device__ __forceinline__ bool forest_push_max(K *W, uint32_t self, uint32_t to) {
  if (to == self) return false;
  const K k = __hip_atomic_load(&W[self], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return k != 0 && atomicMax(&W[to], k) < k;
}

// After a closure of keys: every cell whose link leaves the tile (its bit in exitmask) raises the key of the node it flows
// to (one global_atomic_umax_x2).  flag_out: a node key was raised.
__device__ __forceinline__ void forest_push_exits(const uint8_t *sd, uint8_t nodata, const unsigned long long *key, uint32_t exitmask,
                                                  int lx, int ly0, int x0, int y0, uint32_t tilesX, unsigned long long *nkey,
                                                  uint32_t *flag_out) {
  bool pushed = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    if (!(exitmask >> j & 1u)) continue;
    const int ly = ly0 + 4 * j;
    const unsigned long long k = key[ly * LPS + lx];
    if (k == 0) continue;
    int tx, ty;
    forest_link(sd, nodata, lx, ly, tx, ty);
    atomicMax(&nkey[tile_node(x0 + tx, y0 + ty, tilesX)], k);   // (the target participates: inside the raster)
    pushed = true;
  }
  if (__any(pushed) && (threadIdx.x & 63) == 0) *flag_out = 1;
}

// The length of a path of nx steps along x, ny along y and nd diagonal: two roundings per term, never a fused
// multiply-add, so that a numpy model reproduces it bit for bit.  longest.hip orders cells by the bits of this value and
// subtracts what the flow-path engine wrote: both evaluate it here.
__device__ __forceinline__ double d8_path_length(uint32_t nx, uint32_t ny, uint32_t nd, double cx, double cy, double diag) {
  return __dadd_rn(__dadd_rn(__dmul_rn((double)nx, cx), __dmul_rn((double)ny, cy)), __dmul_rn((double)nd, diag));
}

// ---- kernels (d8_forest.hip) ---------------------------------------------------------------------------------------------
// Every 64 x 64 tile once: each cell pointer-jumped to the in-tile end of its path; a border cell publishes its node's link
// (nxt0: one word per slot).
__global__ void k_forest_links(const uint8_t *__restrict__ dirs, uint8_t nodata, int w, int h, uint32_t tilesX, uint32_t ntiles,
                               uint32_t *__restrict__ nxt0);
// One doubling round over the nodes, from src into dst (never in place: every node covers the same distance); a node
// raises the word of the node it points to: nval[src[i]] <- max(nval[src[i]], nval[i]) (one global_atomic_umax[_x2]).
// Returns at once when *gate == 0: the round before raised nothing.  flag_out: a word was raised.
template <class K>
__global__ void k_forest_round(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, K *nval, uint32_t nnodes,
                               const uint32_t *__restrict__ gate, uint32_t *flag_out);
extern template __global__ void k_forest_round<unsigned long long>(const uint32_t *__restrict__, uint32_t *__restrict__,
                                                                   unsigned long long *, uint32_t, const uint32_t *__restrict__,
                                                                   uint32_t *);
extern template __global__ void k_forest_round<uint32_t>(const uint32_t *__restrict__, uint32_t *__restrict__, uint32_t *, uint32_t,
                                                         const uint32_t *__restrict__, uint32_t *);

// ---- host ------------------------------------------------------------------------------------------------------------------
// cells are indexed with 32 bits, and the values from 0xFFFF0000 up are kept for "none" and its like
inline void check_forest_dims(int w, int h, const char *who) {
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, std::string(who) + ": width and height must be positive");
  if ((uint64_t)w * (uint64_t)h > 0xFFFF0000ull) throw Error(RDGPU_ERR_ARG, std::string(who) + ": raster too large");
}
inline void check_cell_lengths(double cx, double cy, const char *who) {
  if (!std::isfinite(cx) || !std::isfinite(cy) || cx == 0 || cy == 0)
    throw Error(RDGPU_ERR_ARG, std::string(who) + ": the cell lengths must be finite and non-zero");
}
// the tiles and nodes of a w x h raster (nnodes: a multiple of NTHR)
struct ForestDims {
  uint32_t tilesX, ntiles;
  uint64_t nnodes;
  ForestDims(int w, int h) : tilesX((w + LT - 1) / LT), ntiles(tilesX * ((h + LT - 1) / LT)), nnodes((uint64_t)ntiles * TILE_SLOTS) {}
};
// ceil(log2(nodes)) + 1 doubling rounds cover every chain or loop of nodes
inline int forest_rounds(uint64_t nnodes) {
  int rounds = 1;
  while ((1ull << (rounds - 1)) < nnodes) rounds++;
  return rounds;
}

// the flow-path engine (flowpath.hip), as rdgpu_d8_flow_path_dev behind its argument checks; longest.hip runs it first
void flow_path_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, const uint8_t *d_chan, double cx, double cy,
                      uint32_t *d_to_cell, uint32_t *d_steps, double *d_dist, double dist_nodata, hipStream_t s);

}  // namespace rdgpu
