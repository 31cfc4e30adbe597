// tile_front.hpp -- the common front end of the 64 x 64 tile passes over a D8 direction raster (accum.hip and the engines
// of d8_forest.hpp): the staged directions, the byte tables of the eight directions and the numbering of a tile's border
// cells.
#pragma once

#include "common.hpp"

namespace rdgpu {

constexpr int NTHR = 256;

// D8 neighbour offsets, numbering 234/105/876 (reference common/constants.hpp:44-45)
__device__ __forceinline__ int d8dx(int n) { return (n == 1 || n == 2 || n == 8) ? -1 : (n >= 4 && n <= 6) ? 1 : 0; }
__device__ __forceinline__ int d8dy(int n) { return (n >= 2 && n <= 4) ? -1 : (n >= 6 && n <= 8) ? 1 : 0; }

// the tile passes work on LT x LT tiles; a tile's 4 LT - 4 border cells are numbered top row, bottom row, left column,
// right column (the link forest's nodes: 256 slots per tile).  This numbering is a data format: every engine on the forest
// reads and writes node tables laid out by it.
constexpr int LT = 64;
constexpr int TILE_SLOTS = 256;           // a tile's nodes, the spare ones included
constexpr int BORDER_SLOTS = 4 * LT - 4;  // the slots that stand for a border cell
static_assert(BORDER_SLOTS <= TILE_SLOTS && TILE_SLOTS == NTHR, "one border cell per thread, one node word per thread");
__device__ __forceinline__ int border_slot(int lx, int ly) {
  if (ly == 0) return lx;
  if (ly == LT - 1) return LT + lx;
  if (lx == 0) return 2 * LT + (ly - 1);
  if (lx == LT - 1) return 2 * LT + (LT - 2) + (ly - 1);
  return -1;
}
// the inverse: the cell of slot < BORDER_SLOTS.  (Through two locals: assigned straight to the references, accum.hip's
// hand-tuned kernels come out of the compiler with another block layout than with the expressions written in place.)
__device__ __forceinline__ void border_cell(int slot, int &bx, int &by) {
  const int x = slot < LT ? slot : slot < 2 * LT ? slot - LT : slot < 3 * LT - 2 ? 0 : LT - 1;
  const int y = slot < LT ? 0 : slot < 2 * LT ? LT - 1 : slot < 3 * LT - 2 ? slot - 2 * LT + 1 : slot - (3 * LT - 2) + 1;
  bx = x; by = y;
}
// the node of the raster cell (gx, gy), a border cell of its tile
__device__ __forceinline__ uint32_t tile_node(int gx, int gy, uint32_t tilesX) {
  return ((uint32_t)(gy / LT) * tilesX + (uint32_t)(gx / LT)) * (uint32_t)TILE_SLOTS + (uint32_t)border_slot(gx % LT, gy % LT);
}

// The pointer tables of the tile passes are gathered at random by all 64 lanes; with rows of 64 two-byte entries every row
// starts on the same LDS bank, so lanes that point at neighbouring columns of DIFFERENT rows -- the usual case: flow
// converges -- collide.  Rows of LPS = 66 entries shift the banks by one per row (r03e: SQ_LDS_BANK_CONFLICT was 57 % of
// k_acc_link_tile's LDS cycles, 44 % of k_acc_link_final_sums').  A cell's table index is ly * LPS + lx.
constexpr int LPS = LT + 2;
// ---- the tile passes' common front end (r04d) ---------------------------------------------------------------------
// The staged directions: rows of SDW = 72 bytes with the tile's first column at byte SDO = 4, so that an interior tile is
// staged with aligned 32-bit LDS stores from 32-bit global loads (one byte per load and a division per byte made the
// staging a fifth of k_acc_link_tile's instructions).  Cells outside the raster read as `fill`.
constexpr int SDW = 72, SDO = 4, SDH = LT + 2;
__device__ __forceinline__ void stage_dirs_rows(const uint8_t *__restrict__ dirs, int w, int h, int x0, int y0, uint8_t fill,
                                                uint8_t *sd) {
  if (y0 >= 1 && y0 + LT < h && x0 + LT <= w) {   // (block-uniform) every row of the window lies in the raster
    constexpr int NQ = SDH * (LT / 4), QPT = (NQ + NTHR - 1) / NTHR;
    uint32_t v[QPT];
#pragma unroll
    for (int r = 0; r < QPT; r++) {
      const int i = (int)threadIdx.x + r * NTHR;
      if (i < NQ) __builtin_memcpy(&v[r], dirs + (size_t)(y0 - 1 + (i >> 4)) * w + (x0 + 4 * (i & 15)), 4);   // (any alignment)
    }
#pragma unroll
    for (int r = 0; r < QPT; r++) {
      const int i = (int)threadIdx.x + r * NTHR;
      if (i < NQ) *reinterpret_cast<uint32_t *>(sd + (i >> 4) * SDW + SDO + 4 * (i & 15)) = v[r];
    }
    if (threadIdx.x < 2 * SDH) {   // the two ring columns
      const int ly = (int)threadIdx.x >> 1, side = (int)threadIdx.x & 1;
      const int gx = side ? x0 + LT : x0 - 1;
      sd[ly * SDW + (side ? SDO + LT : SDO - 1)] = (gx >= 0 && gx < w) ? dirs[(size_t)(y0 - 1 + ly) * w + gx] : fill;
    }
  } else {
    for (int i = (int)threadIdx.x; i < SDH * SDH; i += NTHR) {
      const int ly = i / SDH, lx = i - ly * SDH;
      const int gx = x0 - 1 + lx, gy = y0 - 1 + ly;
      sd[ly * SDW + SDO - 1 + lx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? dirs[(size_t)gy * w + gx] : fill;
    }
  }
}
// Per direction 1..8 (index e = d - 1), one byte each, looked up with v_perm_b32 (selector bytes 0..3 pick from the second
// operand, 4..7 from the first, 0x0c gives 0): the target's offset in the staged rows (+73), in the pointer table (+67), and
// which side of the tile it can leave through (1: left, 2: right, 4: top, 8: bottom).
__device__ __forceinline__ uint32_t d8_byte(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
constexpr uint32_t D8_SD_LO = 0x02010048u, D8_SD_HI = 0x9091924Au;   // (dy * SDW + dx) + SDW + 1
constexpr uint32_t D8_LP_LO = 0x02010042u, D8_LP_HI = 0x84858644u;   // (dy * LPS + dx) + LPS + 1
constexpr uint32_t D8_FL_LO = 0x06040501u, D8_FL_HI = 0x09080A02u;
static_assert(SDW == 72 && LPS == 66, "the byte tables above");

}  // namespace rdgpu
