// fill.hip -- depression filling on MI355X: descent forest -> basins -> one raster pass -> Boruvka rounds on a pair list.
//
// Replaces FillDepressions<D8/D4> (reference include/richdem/depressions/depressions.hpp:13-21,
// i.e. PriorityFlood_Zhou2016, depressions/Zhou2016.hpp:126-191, and PriorityFlood_Barnes2014<D4>,
// depressions/Barnes2014.hpp:230-304).  The reference is a serial priority-queue sweep; its
// RESULT is the unique surface
//        W(c) = min over paths c -> raster border of (max elevation on the path)
// (SURVEY.md section 0), computed with comparisons and copies only.  This file computes the same
// surface with a GPU-shaped algorithm (see DESIGN.md section 3 for the proof sketch):
//
//   1. k_descent      every cell points at its lowest (key, index) neighbour if that is lower than
//                     itself in the (key, index) total order; border cells drain "OUT".  Paths are
//                     compressed inside a 64x64 tile in LDS, and pits get dense basin ids 0..B-1.
//   2. k_tile_label   lab[c] = basin of c (B = the outside): the few distinct pointers of a tile are chased
//                     to their pits once per tile (k_chase / k_label_cells: fallback for very long chains).
//                     W(c) = max(z(c), L[basin(c)]) with L = minimax pass height basin -> outside.
//   3. rounds of      round 1: k_scan<EMIT> (the one raster pass: the lowest pass of every PAIR of adjacent
//                     components, reduced per tile and appended to a list; each component's lowest pass to a
//                     different component = one 64-bit atomicMin of (pass height << 32 | neighbour component));
//                     rounds 2..: k_edge_round on the pair list (raster k_scan passes as overflow fallback);
//                     k_hook (hook every component along its lowest pass; mutual pairs keep the
//                     smaller id as root), k_chase_links (pointer jumping carrying the path
//                     maximum), k_update_basins (compact labels: k_settle_basins, once), k_compact_roots.  This is Boruvka's contraction:
//                     the number of live components at least halves per round.
//   4. k_finalize     z(c) <- max(z(c), acc[lab[c]]).
//
// All elevation work is on order-preserving 32-bit keys (common.hpp Key32), so it is exact for
// u8/i16/u16/i32/u32/f32.  HBM-bound integer/compare work: no MFMA anywhere.
#include "common.hpp"
#include "fill_shared.hpp"

#include <algorithm>
#include <cstdlib>
#include <numeric>
#include <vector>

struct rdgpu_fill_shard;

namespace rdgpu {

constexpr int TW = 64;        // tile width  (cells)  = one wavefront per tile row
constexpr int TH = 32;        // tile height (cells)
constexpr int LW = TW + 2;    // LDS row stride incl. 1-cell halo (66 words: conflict-free rows)
constexpr int LH = TH + 2;
constexpr uint32_t OUTP = 0xFFFFFFFFu;  // descent pointer of a border cell: drains off the raster
// Component ids carry CLOSED in the top bit when the component never hooks again: the outside (B) and,
// in a row-block shard, the frozen terminal basins of the cut rows (Barnes 2016 tile protocol).
constexpr uint32_t CLOSED = 0x80000000u;
constexpr uint32_t NO_TID = 0xFFFFFFFFu;   // tid[b]: basin b is not a cut-row terminal

static thread_local rdgpu_fill_stats g_stats;   // (per host thread: one thread per device may be inside the library)

// ------------------------------------------------------------------------------------------
// 1. descent pointers, path-compressed inside the tile
// A 64x64 tile (+1 halo) of keys is staged in LDS; every cell picks its descent target; pointers that
// stay inside the tile are chased to their tile-local root with LDS pointer jumping, so what reaches
// HBM already points at a pit, at OUT, or at the first cell OUTSIDE the tile on the cell's path.  The
// global chase (k_chase) then hops tile to tile instead of cell to cell.
// ------------------------------------------------------------------------------------------
constexpr int DW = 64, DH = 64, DLW = DW + 2, DLH = DH + 2;
constexpr uint32_t LAB_PEND = 0x80000000u;   // lab word not resolved yet: LAB_PEND | next cell on the path (OUTP: off the raster)
constexpr uint16_t LTERM_BASE = 0xF000u;   // local pointers >= this: the cell is terminal within the tile (low 4 bits: code)

// Four consecutive cells of a row starting at column gx in one load.  ALIGNED: the raster width is a multiple of 4
// and its base is aligned, so every quad of every row is naturally aligned (the case the compiler may assume and
// the fastest one: the 40000-wide bench DEM).  Otherwise the hardware still takes any element-aligned address for a
// 16 / 8 / 4-byte load (3 % slower when the data happens to be aligned), and the last quad of a row may hang over
// its end: those cells read as `fill`.
template <class U>
struct Quad { U v[4]; };
template <class U, bool ALIGNED>
__device__ __forceinline__ Quad<U> load_quad(const U *__restrict__ row, int gx, int w, U fill) {
  Quad<U> q;
  if (ALIGNED) {
    struct alignas(4 * sizeof(U)) AQ { U v[4]; };
    const AQ a = *reinterpret_cast<const AQ *>(row + gx);
#pragma unroll
    for (int e = 0; e < 4; e++) q.v[e] = a.v[e];
  } else if (gx + 3 < w) {
    __builtin_memcpy(&q, row + gx, sizeof(q));
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) q.v[e] = gx + e < w ? row[gx + e] : fill;
  }
  return q;
}
// A point in the code that arithmetic on a loaded float quad cannot move above (no instruction): the compare-free float key starts
// with a floating-point add, which the compiler otherwise places right behind the quad's load, together with the wait for it.
template <class U>
__device__ __forceinline__ void keys_after_loads(Quad<U> &q) {
  if constexpr (std::is_same<U, float>::value) {
#pragma unroll
    for (int e = 0; e < 4; e++) asm volatile("" : "+v"(q.v[e]));
  }
}

template <class T, int TOPO, bool VEC>
__global__ __launch_bounds__(NTHR) void k_descent(const T *__restrict__ z, uint32_t *__restrict__ lab,
                                                  uint32_t *pit_counter,
                                                  int w, int h, uint32_t tilesX, uint32_t ntiles, int open_top,
                                                  int open_bottom, const uint8_t *__restrict__ outlet) {
  // outlet (optional): cells that drain like border cells (rdgpu_fill_outlets_dev_*, pfdirs.hip)
  __shared__ uint32_t sk[DLH * DLW];
  __shared__ uint16_t lp[DH * DW];
  __shared__ uint32_t wtot[NTHR / 64];
  __shared__ uint32_t pbase;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * DW, y0 = (int)(t / tilesX) * DH;
  {
    // interior columns with quad loads (VEC: naturally aligned quads, else any width -- see load_quad); all
    // loads of the thread are issued before the first is consumed (one memory round trip, not one per trip)
    constexpr int NQ = DLH * (DW / 4), QPT = (NQ + NTHR - 1) / NTHR;
    Quad<T> zq[QPT];   // four cells per load: 16 / 8 / 4 bytes for 4- / 2- / 1-byte elevations
    bool okq[QPT];
#pragma unroll
    for (int r = 0; r < QPT; r++) {
      const int i = threadIdx.x + r * NTHR;
      const int ly = i / (DW / 4), q = i - ly * (DW / 4);
      const int gx = x0 + 4 * q, gy = y0 - 1 + ly;
      okq[r] = i < NQ && gy >= 0 && gy < h && gx < w;
      if (okq[r]) zq[r] = load_quad<T, VEC>(z + (size_t)gy * w, gx, w, T());
    }
#pragma unroll
    for (int r = 0; r < QPT; r++) {
      const int i = threadIdx.x + r * NTHR;
      if (i >= NQ) continue;
      const int ly = i / (DW / 4), q = i - ly * (DW / 4);
      const int o = ly * DLW + 1 + 4 * q;
#pragma unroll
      for (int e = 0; e < 4; e++) sk[o + e] = (okq[r] && x0 + 4 * q + e < w) ? Key32<T>::to(zq[r].v[e]) : 0xFFFFFFFFu;
    }
    for (int i = threadIdx.x; i < 2 * DLH; i += NTHR) {   // halo columns
      const int ly = i >> 1, lxh = (i & 1) ? DLW - 1 : 0;
      const int gx = x0 - 1 + lxh, gy = y0 - 1 + ly;
      uint32_t kk = 0xFFFFFFFFu;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) kk = Key32<T>::to(z[(size_t)gy * w + gx]);
      sk[ly * DLW + lxh] = kk;
    }
  }
  __syncthreads();
  // a wavefront owns a band of DH/4 consecutive rows, one column per lane; the 3x3 window of keys slides
  // down the column in registers (3 LDS reads per cell instead of 9)
  const int lx = threadIdx.x & (DW - 1), ly0 = (threadIdx.x >> 6) * (DH / 4);
  const int gx = x0 + lx;
  // local pointers.  A cell whose target stays in the tile stores the target's local index (12 bits); a cell
  // that is terminal within the tile stores LTERM_BASE | code, code = 0 its own root (pit / cut-row terminal),
  // 1..8 the descent neighbour (outside the tile) in raster order, 9 = drains off the raster -- so the global
  // pointer of a terminal never has to be recomputed from the keys.
  {
    uint32_t k0[3], k1[3], k2[3];
#pragma unroll
    for (int e = 0; e < 3; e++) { k0[e] = sk[ly0 * DLW + lx + e]; k1[e] = sk[(ly0 + 1) * DLW + lx + e]; }
#pragma unroll 4
    for (int j = 0; j < DH / 4; j++) {
      const int ly = ly0 + j, gy = y0 + ly;
#pragma unroll
      for (int e = 0; e < 3; e++) k2[e] = sk[(ly + 2) * DLW + lx + e];
      // Branch-free: every case is computed and the pointer is chosen by selects (the nested ifs compiled into five
      // levels of exec-mask branches per cell; this kernel is bound by instruction issue).
      // lowest (key, index) neighbour: visited in increasing index order and compared with strict '<', so the lowest
      // index wins among equal keys; a neighbour of EQUAL key is taken only if its index is lower.  q packs the
      // neighbour's 3x3 position n with its row n / 3 (bits 4-5) and column n % 3 (bits 6-7).
#define RD_Q(n) ((n) | (((n) / 3) << 4) | (((n) % 3) << 6))
      const uint32_t kc = k1[1];
      uint32_t bk, q;
      if (TOPO == 8) {
        bk = k0[0]; q = RD_Q(0);
        { const bool t = k0[1] < bk; bk = t ? k0[1] : bk; q = t ? RD_Q(1) : q; }
        { const bool t = k0[2] < bk; bk = t ? k0[2] : bk; q = t ? RD_Q(2) : q; }
        { const bool t = k1[0] < bk; bk = t ? k1[0] : bk; q = t ? RD_Q(3) : q; }
        { const bool t = k1[2] < bk; bk = t ? k1[2] : bk; q = t ? RD_Q(5) : q; }
        { const bool t = k2[0] < bk; bk = t ? k2[0] : bk; q = t ? RD_Q(6) : q; }
        { const bool t = k2[1] < bk; bk = t ? k2[1] : bk; q = t ? RD_Q(7) : q; }
        { const bool t = k2[2] < bk; bk = t ? k2[2] : bk; q = t ? RD_Q(8) : q; }
      } else {
        bk = k0[1]; q = RD_Q(1);
        { const bool t = k1[0] < bk; bk = t ? k1[0] : bk; q = t ? RD_Q(3) : q; }
        { const bool t = k1[2] < bk; bk = t ? k1[2] : bk; q = t ? RD_Q(5) : q; }
        { const bool t = k2[1] < bk; bk = t ? k2[1] : bk; q = t ? RD_Q(7) : q; }
      }
#undef RD_Q
      const int n = (int)(q & 15u);
      const bool drains = (bk < kc) | ((bk == kc) & (n < 4));
      const int tx = lx + (int)(q >> 6 & 3u) - 1, ty = ly + (int)(q >> 4 & 3u) - 1;
      const bool inside = (tx >= 0) & (tx < DW) & (ty >= 0) & (ty < DH);
      const uint16_t ldrain = inside ? (uint16_t)(ty * DW + tx) : (uint16_t)(LTERM_BASE | (uint16_t)(n < 4 ? n + 1 : n));
      const bool incell = (gx < w) & (gy < h);
      bool border = (gx == 0) | (gx == w - 1) | ((gy == 0) & !open_top) | ((gy == h - 1) & !open_bottom);   // true border
      if (outlet) border |= incell && outlet[(size_t)gy * w + gx] != 0;
      const bool cutrow = (gy == 0) | (gy == h - 1);   // (not a border: the cut row of a row-block shard, a frozen terminal)
      const uint16_t l = !incell ? LTERM_BASE : border ? (uint16_t)(LTERM_BASE | 9) : (cutrow | !drains) ? LTERM_BASE : ldrain;
      lp[ly * DW + lx] = l;
#pragma unroll
      for (int e = 0; e < 3; e++) { k0[e] = k1[e]; k1[e] = k2[e]; }
    }
  }
  __syncthreads();
  // pointer jumping inside the tile; any value ever stored is an ancestor, so races are harmless.
  // A cell whose parent is a tile root is finished for good, so only the still-active cells (bit mask
  // per thread) are revisited: integer VALU + LDS issue, not HBM, bounds this kernel.
  // Every trip reads all of the thread's pointers, then all of their targets' pointers: two batches of
  // independent LDS reads (the latency of a dependent read chain per cell was what bounded this loop).
  // Two hops per trip (c -> p -> q -> r): the barrier, not the LDS reads, is what a trip costs, and the hop distance
  // triples instead of doubling per trip.
  // A cell is finished for good once its pointer names a tile root (or it is one itself); a ROW of the wavefront's band
  // whose 64 cells are all finished is skipped with one scalar test -- this loop is instruction-issue bound (r02a SQ
  // counters: 2.4 k VALU instructions per wavefront, half of them here), and after two or three trips most rows are done.
  uint32_t act = 0;   // bit j: the cell of row ly0 + j may still move
#pragma unroll
  for (int j = 0; j < DH / 4; j++) act |= (lp[(ly0 + j) * DW + lx] < LTERM_BASE ? 1u : 0u) << j;
  for (int it = 0; it < 12; it++) {
    int still = 0;
#pragma unroll
    for (int g = 0; g < DH / 16; g++) {   // groups of four rows: batched LDS reads inside, one scalar test outside
      if (__ballot((act >> (4 * g)) & 15u) == 0ull) continue;   // wave uniform
      uint16_t pv[4], qv[4], rv[4];
#pragma unroll
      for (int e = 0; e < 4; e++) pv[e] = lp[(ly0 + 4 * g + e) * DW + lx];
#pragma unroll
      for (int e = 0; e < 4; e++) qv[e] = lp[pv[e] < LTERM_BASE ? pv[e] : (ly0 + 4 * g + e) * DW + lx];
#pragma unroll
      for (int e = 0; e < 4; e++) rv[e] = lp[qv[e] < LTERM_BASE ? qv[e] : (ly0 + 4 * g + e) * DW + lx];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int j = 4 * g + e;
        if (pv[e] < LTERM_BASE && qv[e] < LTERM_BASE) {
          // q is not the tile root of the path yet?  then r is a cell further down: jump there and come back
          const bool more = rv[e] < LTERM_BASE;
          lp[(ly0 + j) * DW + lx] = more ? rv[e] : qv[e];
          if (more) still = 1;
          else act &= ~(1u << j);
        } else {
          act &= ~(1u << j);
        }
      }
    }
    if (!__syncthreads_or(still)) break;
  }
  // Pits (and a shard's cut-row terminals) -- the cells that are their own root -- get their dense basin id here:
  // ONE counter add per tile (ids are dense but not in raster order -- nothing depends on their order, the filled
  // surface is unique).
  uint32_t pitmask = 0;
#pragma unroll 4
  for (int j = 0; j < DH / 4; j++) {
    const int ly = ly0 + j, gy = y0 + ly;
    if (gx < w && gy < h && lp[ly * DW + lx] == LTERM_BASE) pitmask |= 1u << j;
  }
  const uint32_t mine = (uint32_t)__popc(pitmask);
  uint32_t incl = mine;   // inclusive prefix over the wavefront
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if ((threadIdx.x & 63) >= o) incl += v;
  }
  if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    pbase = tot ? atomicAdd(pit_counter, tot) : 0;
  }
  __syncthreads();
  uint32_t id = pbase + incl - mine;
  for (int k = 0; k < (int)(threadIdx.x >> 6); k++) id += wtot[k];
  uint32_t *pid = sk;   // the keys are no longer needed: basin id of the pit at local index i
  for (uint32_t m = pitmask; m; m &= m - 1) {
    const int j = __ffs((int)m) - 1;
    pid[(ly0 + j) * DW + lx] = id++;
  }
  __syncthreads();
  // One word per cell: its basin id when its path ends at a pit of this tile (final), LAB_PEND | the first cell
  // outside the tile on its path otherwise, OUTP when it drains off the raster.  k_tile_label resolves the rest.
#pragma unroll 4
  for (int j = 0; j < DH / 4; j++) {
    const int ly = ly0 + j, gy = y0 + ly;
    if (gx >= w || gy >= h) continue;
    const uint16_t p0 = lp[ly * DW + lx];
    const int r = p0 < LTERM_BASE ? (int)p0 : ly * DW + lx;   // the tile root of the cell's path (itself when it is one)
    const uint16_t p = lp[r];                                  // (its own entry again when the cell is a root: no branch)
    const int code = p & 15;
    const uint32_t basin = pid[r];                             // (only meaningful for code 0; any slot is readable)
    const int rx = r & (DW - 1), ry = r >> 6;
    const int n = code <= 4 ? code - 1 : code;   // 3x3 position of the root's descent neighbour (codes 1..8)
    const int nr = n >= 6 ? 2 : n >= 3 ? 1 : 0, nc = n - 3 * nr;
    const uint32_t pend = LAB_PEND | ((uint32_t)(y0 + ry + nr - 1) * (uint32_t)w + (uint32_t)(x0 + rx + nc - 1));
    lab[(size_t)gy * w + gx] = code == 9 ? OUTP : code == 0 ? basin : pend;
  }
}

// ------------------------------------------------------------------------------------------
// 2. labels.  After k_descent a word of lab[] is a basin id (final), LAB_PEND | next cell, or OUTP.  Every value ever
// stored in a word is the cell's basin, or a cell further down its path, or OUTP when the path leaves the raster --
// so concurrent in-place updates and stale cached reads are harmless.
// ------------------------------------------------------------------------------------------
// Fallback for pathologically long tile-to-tile chains: bounded hops per pass with path compression; the host
// repeats while flagged.  Resolves a word as soon as it meets a resolved one.
__global__ __launch_bounds__(NTHR) void k_chase(uint32_t *lab, uint32_t n, int maxhops, uint32_t *flag) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c64 = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c64 < n; c64 += stride) {
    const uint32_t c = (uint32_t)c64;
    uint32_t v = lab[c];
    if (!(v & LAB_PEND) || v == OUTP) continue;
    const uint32_t v0 = v;
    int hops = 0;
    bool unfinished = false;
    for (;;) {
      const uint32_t q = lab[v & ~LAB_PEND];
      v = q;
      if (!(q & LAB_PEND) || q == OUTP) break;
      if (++hops >= maxhops) { unfinished = true; break; }
    }
    if (v != v0) lab[c] = v;
    if (unfinished) *flag = 1;
  }
}

// Labels per tile: the unresolved cells of a 64x64 tile share a handful of distinct pointers (the ring cells its
// paths leave through), so the distinct values are collected in an LDS table, each is chased to a resolved word
// ONCE (tile-to-tile hops, global gathers), and the cells read their label from LDS; lab[c] = B for cells draining
// off the raster.  Cells whose path ends at a pit of their own tile were finished by k_descent and are not written.
// A chain longer than maxhops raises the flag and leaves (compressed) pending words: the host then falls back to the
// compressing passes.
constexpr int LT_SLOTS = 1024;
constexpr uint32_t LT_EMPTY = 0xFFFFFFFEu;

__device__ __forceinline__ uint32_t chase_to_label(const uint32_t *lab, uint32_t v, uint32_t B, int maxhops, uint32_t *flag) {
  int hops = 0;
  for (;;) {   // v: a pending word
    const uint32_t q = lab[v & ~LAB_PEND];
    if (q == OUTP) return B;
    if (!(q & LAB_PEND)) return q;
    v = q;
    if (++hops >= maxhops) { *flag = 1; return v; }
  }
}

__global__ __launch_bounds__(NTHR) void k_tile_label(uint32_t *lab, int w, int h, uint32_t tilesX, uint32_t ntiles,
                                                     uint32_t B, int maxhops, uint32_t *flag) {
  __shared__ uint32_t tkey[LT_SLOTS];
  __shared__ uint32_t tval[LT_SLOTS];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * DW, y0 = (int)(t / tilesX) * DH;
  for (int i = threadIdx.x; i < LT_SLOTS; i += NTHR) tkey[i] = LT_EMPTY;
  __syncthreads();
  const int lx = threadIdx.x & (DW - 1), ly0 = threadIdx.x >> 6;
  const int gx = x0 + lx;
  constexpr int CELLS = DH / 4;
  uint32_t pv[CELLS];
  int16_t sl[CELLS];   // table slot, -1: final already / outside the raster, -2: drains off the raster, -3: table full
#pragma unroll
  for (int j = 0; j < CELLS; j++) {   // all loads of the thread in flight together
    const int gy = y0 + ly0 + 4 * j;
    pv[j] = (gx < w && gy < h) ? lab[(size_t)gy * w + gx] : 0u;
  }
#pragma unroll
  for (int j = 0; j < CELLS; j++) {
    sl[j] = -1;
    const uint32_t p = pv[j];
    if (!(p & LAB_PEND)) continue;
    if (p == OUTP) { sl[j] = -2; continue; }
    if (j > 0 && sl[j - 1] >= 0 && pv[j - 1] == p) { sl[j] = sl[j - 1]; continue; }
    uint32_t slot = (p * 0x9E3779B1u) >> 22;
    int found = -3;
#pragma unroll 1
    for (int probe = 0; probe < 16; probe++) {
      uint32_t k = tkey[slot];
      if (k == LT_EMPTY) k = atomicCAS(&tkey[slot], LT_EMPTY, p);
      if (k == LT_EMPTY || k == p) { found = (int)slot; break; }
      slot = (slot + 1) & (LT_SLOTS - 1);
    }
    sl[j] = (int16_t)found;
  }
  __syncthreads();
  {
    // the thread's table slots are chased together: one gather per live chain and trip, all in flight at once
    constexpr int SPT = LT_SLOTS / NTHR;
    uint32_t p[SPT];
    uint32_t live = 0;
#pragma unroll
    for (int r = 0; r < SPT; r++) {
      p[r] = tkey[threadIdx.x + r * NTHR];   // a pending word (or LT_EMPTY)
      if (p[r] != LT_EMPTY) live |= 1u << r;
    }
    for (int hops = 0; live; hops++) {
      if (hops > maxhops) { *flag = 1; break; }   // the words stay pending (compressed): the fallback finishes them
      uint32_t q[SPT];
#pragma unroll
      for (int r = 0; r < SPT; r++) q[r] = (live >> r & 1u) ? lab[p[r] & ~LAB_PEND] : 0u;
#pragma unroll
      for (int r = 0; r < SPT; r++) {
        if (!(live >> r & 1u)) continue;
        if (q[r] == OUTP) { p[r] = B; live &= ~(1u << r); }
        else if (!(q[r] & LAB_PEND)) { p[r] = q[r]; live &= ~(1u << r); }
        else p[r] = q[r];
      }
    }
#pragma unroll
    for (int r = 0; r < SPT; r++) tval[threadIdx.x + r * NTHR] = p[r];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CELLS; j++) {
    if (sl[j] == -1) continue;
    const size_t c = (size_t)(y0 + ly0 + 4 * j) * w + gx;
    lab[c] = sl[j] >= 0 ? tval[sl[j]] : sl[j] == -2 ? B : chase_to_label(lab, pv[j], B, maxhops, flag);
  }
}

// ------------------------------------------------------------------------------------------
// 3. after the compressing fallback passes every word is a basin id or OUTP: lab[c] = B for the latter
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_label_cells(uint32_t *lab, uint32_t n, uint32_t B) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c64 = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c64 < n; c64 += stride)
    if (lab[c64] == OUTP) lab[c64] = B;
}

// Stream compaction helper: every thread of the (256-thread) block calls it; ONE global atomic per
// block (same-address atomics serialise at ~12 ns each on this chip, so per-wave appends of 10^7
// elements cost milliseconds).  Returns the output slot for threads with pred.
__device__ __forceinline__ uint32_t block_append(bool pred, uint32_t *counter) {
  __shared__ uint32_t wcnt[NTHR / 64];
  __shared__ uint32_t bbase;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(pred);
  if (lane == 0) wcnt[wv] = (uint32_t)__popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    bbase = tot ? atomicAdd(counter, tot) : 0;
  }
  __syncthreads();
  uint32_t off = bbase;
  for (int k = 0; k < wv; k++) off += wcnt[k];
  return off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}

// ------------------------------------------------------------------------------------------
// 4. Boruvka rounds
// tables (B+1 entries, index B = the outside): cur[b]  current root component of basin b
//                                              acc[b]  max pass key on b's path to cur[b]
//                                              best[r] (pass key << 32 | neighbour root), per root
//                                              link[r] (path max key << 32 | parent root), per root
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_init_tables(uint32_t *cur, uint32_t *acc, unsigned long long *link,
                                                      uint32_t *roots, uint32_t *nroots,
                                                      const uint32_t *__restrict__ tid, uint32_t B) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;   // grid covers whole waves past B
  bool open = false;
  if (i <= B) {
    const bool closed = i == B || (tid && tid[i] != NO_TID);
    cur[i] = closed ? (i | CLOSED) : i;
    acc[i] = 0;
    link[i] = (unsigned long long)i;
    open = !closed;
  }
  // live roots = basins that still have to hook (everything but the outside and frozen terminals).  Without
  // terminals that is simply 0..B-1: no compaction (one same-address atomic per block is 0.5 ms for 4e4 blocks)
  if (!tid) {
    if (i < B) roots[i] = i;
    if (i == 0) *nroots = B;
    return;
  }
  const uint32_t slot = block_append(open, nroots);
  if (open) roots[slot] = i;
}

// tid[basin] = terminal id of a cut-row cell's basin (top row: x, bottom row: w + x), NO_TID otherwise
__global__ __launch_bounds__(NTHR) void k_mark_terminals(const uint32_t *__restrict__ lab, uint32_t *tid, int w, int h,
                                                         int open_top, int open_bottom) {
  const int x = blockIdx.x * NTHR + threadIdx.x;
  if (x <= 0 || x >= w - 1) return;
  if (open_top) tid[lab[x]] = (uint32_t)x;
  if (open_bottom) tid[lab[(size_t)(h - 1) * w + x]] = (uint32_t)(w + x);
}

// (r06) dyn != nullptr in the round kernels below: the count is read from the device -- the rounds of a fill are enqueued
// without a host read-back between them, over grids the host sizes from upper bounds (grid-stride loops: a launch
// whose list turns out empty costs a few microseconds).
// (r07) The bodies of the round kernels are __device__ functions over (block index, block count) and NT threads per
// block: the __global__ kernels below are their full-width launches, k_rounds_tail runs them in ONE workgroup, round after
// round, once a round's lists are small.  A full-width round kernel returns at once when its gate says that the tail
// kernel takes the round: the live roots and the records entering it (cnt[0], cnt[1]: final before the round's first
// launch, and never growing from round to round) are both under the tail's thresholds.
struct TailGate {
  const uint32_t *cnt = nullptr;   // rc + 4 r of the round; nullptr: the round is never the tail's
  uint32_t roots = 0, recs = 0;
  __device__ __forceinline__ bool taken() const { return cnt && cnt[0] <= roots && cnt[1] <= recs; }
};

template <int NT>
__device__ __forceinline__ void best_reset_body(const uint32_t *roots, uint32_t nroots, unsigned long long *best,
                                                uint32_t blk, uint32_t nblk) {
  for (uint32_t i = blk * NT + threadIdx.x; i < nroots; i += nblk * NT) best[roots[i]] = ~0ull;
}
__global__ __launch_bounds__(NTHR) void k_best_reset(const uint32_t *__restrict__ roots, uint32_t nroots,
                                                     unsigned long long *best, const uint32_t *__restrict__ dyn = nullptr,
                                                     TailGate gate = TailGate()) {
  if (gate.taken()) return;
  if (dyn) nroots = *dyn;
  best_reset_body<NTHR>(roots, nroots, best, blockIdx.x, gridDim.x);
}

// One raster pass of a Boruvka round.  tiles_in == nullptr: all tiles (XCD-banded order); otherwise
// the list of tiles that still contained a component boundary last round (a tile without candidates can
// never produce one again: components only merge, open components only close).  Candidates of the same
// component are first reduced in an LDS table, so a tile issues ~one global atomic per component it
// touches instead of one per boundary cell.
constexpr int SC_SLOTS = 256;

// find-or-insert component C in the block's LDS table; -1 when its probe window is full
__device__ __forceinline__ int tab_slot(uint32_t *tab_id, uint32_t C) {
  uint32_t slot = (C * 0x9E3779B1u) >> 24;
#pragma unroll 1
  for (int probe = 0; probe < 8; probe++) {
    uint32_t id = tab_id[slot];
    if (id == 0xFFFFFFFFu) id = atomicCAS(&tab_id[slot], 0xFFFFFFFFu, C);
    if (id == 0xFFFFFFFFu || id == C) return (int)slot;
    slot = (slot + 1) & (SC_SLOTS - 1);
  }
  return -1;
}

// The component-pair list of the first round (EMIT).  A raster pass is only needed ONCE: while it looks for every
// component's lowest pass it also sees every pair of adjacent components, and the lowest pass of each PAIR is all the
// later rounds need.  The pairs of a tile are reduced in an LDS table and appended to a global list of
// (component, component, pass key) records; rounds 2.. contract that list (k_edge_round) instead of re-reading the
// raster.  The list is split into ESEG segments with their own fill counters: a single counter bumped once per
// tile would serialise (~12 ns per same-address atomic, 7.8e5 tiles).  A pair that finds no slot in the tile's table is
// appended on its own (pair_spill); a segment that runs full raises `overflow`, and the host falls back to raster
// passes for the remaining rounds.
constexpr int PT_SLOTS = 256, PT_PROBES = 16;
constexpr uint32_t ESEG = 8192;
struct EdgeOut {
  uint32_t *a, *b, *k;     // nseg segments of `segcap` records each
  uint32_t *segcount;      // fill count per segment
  uint32_t segcap;
  uint32_t segmask;        // nseg - 1 (nseg: a power of two <= ESEG)
  uint32_t *overflow;
  uint32_t seglimit = 0xFFFFFFFFu;   // k_pairs16: records a segment may take (<= segcap; smaller under RDGPU_FILL_EDGE_CAP)
};

template <int SLOTS = PT_SLOTS>
__device__ __forceinline__ uint32_t pair_home(uint32_t C, uint32_t D) {
  return (((C * 0x9E3779B1u) ^ (D * 0x85EBCA6Bu)) >> 16) & (SLOTS - 1);
}
// find-or-insert the pair (C, D) in the tile's LDS pair table and lower its pass key; false when the probe window is full
template <int SLOTS = PT_SLOTS>
__device__ __forceinline__ bool pair_insert(unsigned long long *pt_pair, uint32_t *pt_key, uint32_t C, uint32_t D, uint32_t key) {
  const unsigned long long pr = ((unsigned long long)C << 32) | D;
  uint32_t slot = pair_home<SLOTS>(C, D);
#pragma unroll 1
  for (int probe = 0; probe < PT_PROBES; probe++) {
    unsigned long long v = pt_pair[slot];
    if (v == ~0ull) {
      v = atomicCAS(&pt_pair[slot], ~0ull, pr);
      if (v == ~0ull) v = pr;
    }
    if (v == pr) {
      if (key < pt_key[slot]) atomicMin(&pt_key[slot], key);
      return true;
    }
    slot = (slot + 1) & (SLOTS - 1);
  }
  return false;
}

// A pair that found no slot in the tile's table goes straight to the tile's segment, one record per atomic: slow, but
// it keeps rasters with hundreds of basins per tile on the pair list (the records are only not merged per tile).
__device__ __forceinline__ void pair_spill(const EdgeOut &eo, unsigned long long *best, uint32_t seg,
                                           uint32_t lo, uint32_t hi, uint32_t key) {
  // (it bypasses the table the components' proposals are derived from, so it proposes on its own)

  const unsigned long long cl = ((unsigned long long)key << 32) | hi, ch = ((unsigned long long)key << 32) | lo;
  if (!(lo & CLOSED) && cl < best[lo]) atomicMin(&best[lo], cl);
  if (!(hi & CLOSED) && ch < best[hi]) atomicMin(&best[hi], ch);
  const uint32_t g = atomicAdd(&eo.segcount[seg], 1u);
  if (g < eo.segcap) {
    const size_t i = (size_t)seg * eo.segcap + g;
    eo.a[i] = lo; eo.b[i] = hi; eo.k[i] = key;
  } else {
    *eo.overflow = 1;
  }
}

template <class T, int TOPO, bool FIRST, bool VEC, bool EMIT>
__global__ __launch_bounds__(NTHR) void k_scan(const T *__restrict__ z, const uint32_t *__restrict__ lab,
                                               const uint32_t *__restrict__ cur, unsigned long long *best,
                                               int w, int h, uint32_t B, uint32_t tilesX, uint32_t ntiles,
                                               const uint32_t *__restrict__ tiles_in, uint32_t nwork,
                                               uint8_t *alive_out, EdgeOut eo) {
  __shared__ __attribute__((aligned(8))) uint32_t sk[LH * LW];
  __shared__ uint32_t sc[LH * LW];
  // The component table: in the pair pass it is only needed AFTER the pairs are reduced, when the keys are dead, so it
  // lives in sk's storage there (with the 256-slot pair table: 25.1 instead of 31.5 KB of LDS, a sixth block per CU).
  __shared__ uint32_t tab_id_s[EMIT ? 1 : SC_SLOTS];
  __shared__ unsigned long long tab_val_s[EMIT ? 1 : SC_SLOTS];
  __shared__ uint8_t tab_cross_s[EMIT ? 1 : SC_SLOTS];
  uint32_t *const tab_id = EMIT ? sk : tab_id_s;
  unsigned long long *const tab_val = EMIT ? reinterpret_cast<unsigned long long *>(sk + SC_SLOTS) : tab_val_s;
  uint8_t *const tab_cross = EMIT ? reinterpret_cast<uint8_t *>(sk + 3 * SC_SLOTS) : tab_cross_s;
  __shared__ uint16_t list[TW * TH];   // LDS offsets of the cells that touch another component
  __shared__ uint32_t nlist;
  __shared__ unsigned long long pt_pair[EMIT ? PT_SLOTS : 1];   // (smaller id << 32 | larger id), ~0 = empty
  __shared__ uint32_t pt_key[EMIT ? PT_SLOTS : 1];              // lowest pass key of the pair
  __shared__ uint32_t pt_n, pt_base, any_open;
  // XCD-banded order in every round; from round 2 on only the tiles that still held a component boundary last
  // round are launched (compacted list: a dead tile costs neither a block nor a flag load)
  const uint32_t wi = xcd_tile(blockIdx.x, nwork);
  if (wi >= nwork) return;
  const uint32_t t = tiles_in ? tiles_in[wi] : wi;
  const int x0 = (int)(t % tilesX) * TW, y0 = (int)(t / tilesX) * TH;
  if (!EMIT)
    for (int i = threadIdx.x; i < SC_SLOTS; i += NTHR) { tab_id[i] = 0xFFFFFFFFu; tab_val[i] = ~0ull; tab_cross[i] = 0; }
  if (EMIT)
    for (int i = threadIdx.x; i < PT_SLOTS; i += NTHR) { pt_pair[i] = ~0ull; pt_key[i] = 0xFFFFFFFFu; }
  if (threadIdx.x == 0) { nlist = 0; pt_n = 0; any_open = 0; }
  // FIRST: every basin is still its own component (only used when there are no frozen terminals)
#define RD_COMP(l) (FIRST ? ((l) == B ? (B | CLOSED) : (l)) : cur[(l)])
  {
    // Interior columns with quad loads (VEC: naturally aligned quads, else any width -- see load_quad),
    // the two halo columns with scalar loads.  The kernel is latency bound (SQ counters: waves parked ~75 % of
    // their cycles), so the loads are issued in two batches -- every z / label quad of this thread, then every
    // component gather -- instead of item by item: two dependent memory round trips per tile instead of six.
    constexpr int NQ = LH * (TW / 4);                 // 16-byte items of the tile incl. halo rows
    constexpr int QPT = (NQ + NTHR - 1) / NTHR;       // per thread
    Quad<T> zq[QPT];   // four cells per load: 16 / 8 / 4 bytes for 4- / 2- / 1-byte elevations
    Quad<uint32_t> lq[QPT];
    bool ok[QPT];
#pragma unroll
    for (int r = 0; r < QPT; r++) {
      const int i = threadIdx.x + r * NTHR;
      const int ly = i / (TW / 4), q = i - ly * (TW / 4);
      const int gx = x0 + 4 * q, gy = y0 - 1 + ly;
      ok[r] = i < NQ && gy >= 0 && gy < h && gx < w;
      if (ok[r]) {
        const size_t g = (size_t)gy * w + gx;
        zq[r] = load_quad<T, VEC>(z + (g - gx), gx, w, T());
        lq[r] = load_quad<uint32_t, VEC>(lab + (g - gx), gx, w, B);   // past the row end: the outside's label
      }
    }
    // halo columns: one cell per thread for the first 2 * LH threads
    const bool hcell = threadIdx.x < 2 * LH;
    const int hly = threadIdx.x >> 1, hlx = (threadIdx.x & 1) ? LW - 1 : 0;
    bool hok = false;
    T hz = T();
    uint32_t hl = 0;
    if (hcell) {
      const int gx = x0 - 1 + hlx, gy = y0 - 1 + hly;
      hok = gx >= 0 && gx < w && gy >= 0 && gy < h;
      if (hok) {
        hl = lab[(size_t)gy * w + gx];
        hz = z[(size_t)gy * w + gx];
      }
    }
    uint32_t cq[QPT][4];
#pragma unroll
    for (int r = 0; r < QPT; r++) {
      // branch-free: an absent quad reads the outside's entry (label B: cur[B] == B | CLOSED), so all gathers of
      // the thread are in flight together
      const uint32_t l[4] = {ok[r] ? lq[r].v[0] : B, ok[r] ? lq[r].v[1] : B, ok[r] ? lq[r].v[2] : B, ok[r] ? lq[r].v[3] : B};
#pragma unroll
      for (int e = 0; e < 4; e++) cq[r][e] = RD_COMP(l[e]);
    }
    const uint32_t hlsafe = hok ? hl : B;
    const uint32_t hc = RD_COMP(hlsafe);
#pragma unroll
    for (int r = 0; r < QPT; r++) {
      const int i = threadIdx.x + r * NTHR;
      if (i < NQ) {
        const int ly = i / (TW / 4), q = i - ly * (TW / 4);
        const int o = ly * LW + 1 + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; e++) { sk[o + e] = (ok[r] && x0 + 4 * q + e < w) ? Key32<T>::to(zq[r].v[e]) : 0u; sc[o + e] = cq[r][e]; }
      }
    }
    if (hcell) { sk[hly * LW + hlx] = hok ? Key32<T>::to(hz) : 0u; sc[hly * LW + hlx] = hc; }
  }
#undef RD_COMP
  __syncthreads();
  // Phase 1 -- detect: each wavefront walks a band of TH/4 consecutive rows, one column per lane, with
  // the 3x3 window of component ids carried in registers, and appends the cells that touch another
  // component to an LDS list.  Integer VALU is the bottleneck of this kernel (not HBM), and only
  // ~5-15% of the cells sit on a component boundary, so the expensive candidate evaluation (phase 2)
  // runs densely over that list instead of over every lane.
  const int lx = threadIdx.x & (TW - 1), band = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int ROWS = TH / 4;
  const int gx = x0 + lx;
  const int yb = band * ROWS;   // first tile row of the band
  {
    uint32_t c0[3], c1[3], c2[3];
    {
      const int o = yb * LW + lx;   // LDS row yb is the halo row above tile row yb
#pragma unroll
      for (int e = 0; e < 3; e++) { c0[e] = sc[o + e]; c1[e] = sc[o + LW + e]; }
    }
    unsigned long long bal[ROWS];   // per row: the lanes whose cell touches another component
    unsigned long long balive = 0;
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
      const int ly = yb + j, gy = y0 + ly;
      {
        const int o = (ly + 2) * LW + lx;
#pragma unroll
        for (int e = 0; e < 3; e++) c2[e] = sc[o + e];
      }
      const uint32_t C = c1[1];
      uint32_t d = (c0[1] ^ C) | (c1[0] ^ C) | (c1[2] ^ C) | (c2[1] ^ C);
      if (TOPO == 8) d |= (c0[0] ^ C) | (c0[2] ^ C) | (c2[0] ^ C) | (c2[2] ^ C);
      // closed: drains to the outside or to a frozen terminal -- never proposes
      bool hit = d != 0 && !(C & CLOSED) && gx < w && gy < h;
      if (EMIT) {
        // the pair pass lists the cells with a foreign E / SE / S / SW neighbour (open or closed: see phase 2);
        // "this tile holds a component boundary" keeps its meaning for the raster fallback
        balive |= __ballot(hit);
        uint32_t df = (c1[2] ^ C) | (c2[1] ^ C);
        if (TOPO == 8) df |= (c2[0] ^ C) | (c2[2] ^ C);
        hit = df != 0 && gx < w && gy < h;
      }
      bal[j] = __ballot(hit);
#pragma unroll
      for (int e = 0; e < 3; e++) { c0[e] = c1[e]; c1[e] = c2[e]; }
    }
    if (EMIT && balive && lane == 0) any_open = 1;
    // one list reservation per wavefront (a returning LDS atomic per row was a dependent chain of eight)
    uint32_t total = 0;
#pragma unroll
    for (int j = 0; j < ROWS; j++) total += (uint32_t)__popcll(bal[j]);
    if (total) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&nlist, total);
      base = __shfl(base, 0, 64);
#pragma unroll
      for (int j = 0; j < ROWS; j++) {
        if (bal[j] >> lane & 1ull)
          list[base + __popcll(bal[j] & ((1ull << lane) - 1ull))] = (uint16_t)((yb + j + 1) * LW + lx + 1);
        base += (uint32_t)__popcll(bal[j]);
      }
    }
  }
  // (no barrier needed between the detect phase and this: both only read sc)
  // components that also live outside this tile (seen on the halo ring) need the global atomic;
  // a component entirely inside the tile is reduced here completely and can use a plain store
  for (int i = threadIdx.x; !EMIT && i < 2 * LW + 2 * (LH - 2); i += NTHR) {   // (the pair pass always uses the atomic)
    int o;
    if (i < LW) o = i;
    else if (i < 2 * LW) o = (LH - 1) * LW + (i - LW);
    else { const int r = (i - 2 * LW) >> 1; o = (r + 1) * LW + (((i - 2 * LW) & 1) ? LW - 1 : 0); }
    const uint32_t C = sc[o];
    if (!(C & CLOSED)) {
      const int slot = tab_slot(tab_id, C);
      if (slot >= 0) tab_cross[slot] = 1;
    }
  }
  __syncthreads();
  const uint32_t nl = nlist;
  if (EMIT) {
    // Phase 2 (pair pass) -- every adjacent cell pair is recorded exactly once, by its earlier cell in raster order:
    // a listed cell looks at its E, SE, S, SW neighbours (D4: E, S) and the pair is stored as (smaller id, larger
    // id) with its pass height.  Up to two distinct neighbouring components are kept in registers and looked up
    // together: the common case -- the pair is already in its home slot with a pass at least as low -- costs one
    // LDS round trip for the whole cell.  The components' own lowest passes are derived from the pairs afterwards.
    constexpr int NF = TOPO == 8 ? 4 : 2;
    const int foff[4] = {1, TOPO == 8 ? LW + 1 : LW, LW, LW - 1};
    const uint32_t seg = t & eo.segmask;
    for (uint32_t i = threadIdx.x; i < nl; i += NTHR) {
      const int o = list[i];
      const uint32_t C = sc[o], kc = sk[o];
      uint32_t nD[NF], nH[NF];
#pragma unroll
      for (int e = 0; e < NF; e++) { nD[e] = sc[o + foff[e]]; nH[e] = sk[o + foff[e]]; }
      uint32_t pd[2] = {C, C}, pk[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};   // pd == C: unused
#pragma unroll
      for (int e = 0; e < NF; e++) {
        const uint32_t D = nD[e], hn = nH[e] > kc ? nH[e] : kc;   // pass height of the cell pair
        if (D != C && !(C & D & CLOSED)) {   // two closed components never merge
          if (pd[0] == C) pd[0] = D;
          if (D == pd[0]) pk[0] = hn < pk[0] ? hn : pk[0];
          else {
            if (pd[1] == C) pd[1] = D;
            if (D == pd[1]) pk[1] = hn < pk[1] ? hn : pk[1];
            else if (!pair_insert(pt_pair, pt_key, C < D ? C : D, C < D ? D : C, hn)) pair_spill(eo, best, seg, C < D ? C : D, C < D ? D : C, hn);
          }
        }
      }
      uint32_t ps[2], pq[2], lo[2], hi[2];
      unsigned long long pv[2];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        lo[j] = C < pd[j] ? C : pd[j];
        hi[j] = C < pd[j] ? pd[j] : C;
        ps[j] = pair_home(lo[j], hi[j]);
        pv[j] = pt_pair[ps[j]];
        pq[j] = pt_key[ps[j]];
      }
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (pd[j] != C) {
          const unsigned long long pr = ((unsigned long long)lo[j] << 32) | hi[j];
          if (pv[j] == pr) { if (pk[j] < pq[j]) atomicMin(&pt_key[ps[j]], pk[j]); }
          else if (!pair_insert(pt_pair, pt_key, lo[j], hi[j], pk[j])) pair_spill(eo, best, seg, lo[j], hi[j], pk[j]);
        }
      }
    }
    __syncthreads();
    // the keys are dead from here on: their storage becomes the component table (visible after the next barrier)
    for (int i = threadIdx.x; i < SC_SLOTS; i += NTHR) { tab_id[i] = 0xFFFFFFFFu; tab_val[i] = ~0ull; }
    // compact the occupied slots (`list` is free again)
    const int lane64 = threadIdx.x & 63;
    for (int i = threadIdx.x; i < PT_SLOTS; i += NTHR) {
      const bool occ = pt_pair[i] != ~0ull;
      const unsigned long long bal = __ballot(occ);
      uint32_t base = 0;
      if (lane64 == 0 && bal) base = atomicAdd(&pt_n, (uint32_t)__popcll(bal));
      base = __shfl(base, 0, 64);
      if (occ) list[base + __popcll(bal & ((1ull << lane64) - 1ull))] = (uint16_t)i;
    }
    __syncthreads();
    // reserve the tile's space in its segment with ONE atomic (its latency hides behind the loop below)
    const uint32_t tot = pt_n;
    if (threadIdx.x == 0) {
      uint32_t ob = 0xFFFFFFFFu;
      if (tot) {
        ob = atomicAdd(&eo.segcount[seg], tot);
        if (ob + tot > eo.segcap) { *eo.overflow = 1; ob = 0xFFFFFFFFu; }
      }
      pt_base = ob;
      alive_out[t] = any_open ? 1 : 0;
    }
    // every pair proposes its pass to its open sides, reduced per component in the LDS table
    for (uint32_t i = threadIdx.x; i < tot; i += NTHR) {
      const int sl = list[i];
      const unsigned long long pr = pt_pair[sl];
      const uint32_t lo = (uint32_t)(pr >> 32), hi = (uint32_t)pr, key = pt_key[sl];
      if (!(lo & CLOSED)) {
        const unsigned long long cand = ((unsigned long long)key << 32) | hi;
        const int slot = tab_slot(tab_id, lo);
        if (slot >= 0) atomicMin(&tab_val[slot], cand);
        else if (cand < best[lo]) atomicMin(&best[lo], cand);
      }
      if (!(hi & CLOSED)) {
        const unsigned long long cand = ((unsigned long long)key << 32) | lo;
        const int slot = tab_slot(tab_id, hi);
        if (slot >= 0) atomicMin(&tab_val[slot], cand);
        else if (cand < best[hi]) atomicMin(&best[hi], cand);
      }
    }
    __syncthreads();
    // (always the atomic: a pair of C with a cell above / left of it is recorded -- and proposed -- by the tile that
    // owns that earlier cell, so even a component entirely inside this tile can have another proposer)
    for (int i = threadIdx.x; i < SC_SLOTS; i += NTHR) {
      const uint32_t C = tab_id[i];
      if (C != 0xFFFFFFFFu) {
        const unsigned long long cand = tab_val[i];
        if (cand < best[C]) atomicMin(&best[C], cand);      // cheap (possibly stale) pre-check first
      }
    }
    const uint32_t ob = pt_base;
    if (ob != 0xFFFFFFFFu) {
      const size_t g0 = (size_t)seg * eo.segcap + ob;
      for (uint32_t i = threadIdx.x; i < tot; i += NTHR) {
        const int sl = list[i];
        const unsigned long long pr = pt_pair[sl];
        eo.a[g0 + i] = (uint32_t)(pr >> 32);
        eo.b[g0 + i] = (uint32_t)pr;
        eo.k[g0 + i] = pt_key[sl];
      }
    }
    return;
  }
  // Phase 2 -- evaluate the boundary cells densely
  for (uint32_t i = threadIdx.x; i < nl; i += NTHR) {
    const int o = list[i];
    const uint32_t C = sc[o], kc = sk[o];
    unsigned long long cand = ~0ull;
    // the ring of neighbours, read once: N, NE, E, SE, S, SW, W, NW (D4: N, E, S, W)
    constexpr int NNB = TOPO == 8 ? 8 : 4;
    const int noff[8] = {-LW, TOPO == 8 ? -LW + 1 : 1, TOPO == 8 ? 1 : LW, TOPO == 8 ? LW + 1 : -1, LW, LW - 1, -1, -LW - 1};
    uint32_t nD[NNB], nH[NNB];
#pragma unroll
    for (int e = 0; e < NNB; e++) { nD[e] = sc[o + noff[e]]; nH[e] = sk[o + noff[e]]; }
#pragma unroll
    for (int e = 0; e < NNB; e++) {
      nH[e] = nH[e] > kc ? nH[e] : kc;   // pass height of the cell pair
      const unsigned long long e_ = ((unsigned long long)(nD[e] != C ? nH[e] : 0xFFFFFFFFu) << 32) | nD[e];
      cand = e_ < cand ? e_ : cand;
    }
    // reduce per component in LDS; fall back to the global atomic when its probe window is full
    const int slot = tab_slot(tab_id, C);
    if (slot >= 0) atomicMin(&tab_val[slot], cand);
    else if (cand < best[C]) atomicMin(&best[C], cand);
  }
  const int any = nl != 0;
  __syncthreads();
  const int alive = any;
  for (int i = threadIdx.x; i < SC_SLOTS; i += NTHR) {
    const uint32_t C = tab_id[i];
    if (C != 0xFFFFFFFFu) {
      const unsigned long long cand = tab_val[i];
      if (cand == ~0ull) continue;   // only seen on the halo ring
      if (!tab_cross[i]) best[C] = cand;                       // nobody else proposes for C
      else if (cand < best[C]) atomicMin(&best[C], cand);      // cheap (possibly stale) pre-check first
    }
  }
  // NB: no global "alive tiles" counter here -- ~10^6 same-address atomics serialise at ~12 ns each
  // (that alone cost 9 ms per pass); k_compact_alive turns the flags into the next round's tile list
  if (threadIdx.x == 0) alive_out[t] = alive ? 1 : 0;
}

// One contraction round on the pair list: every record (a, b, key) is mapped to the current components of its two
// sides; a record inside one component (or between two closed ones) is dropped for good, the others propose
// (key << 32 | other side) to best[] exactly as the raster pass does, and are written to the next round's list as
// (current a, current b, key).  SEG: the input is the segmented list of the raster pass (one segment per block
// range: segcap is a multiple of the 2048 records a block covers); otherwise a dense list of n records.
constexpr int EPT = 8;
constexpr int DT_SLOTS = 4096;   // the dense rounds' pair table of a block (2048 records)
// The dense rounds (!SEG) first merge the records of a block per component pair in an LDS table -- after a few rounds
// most records of a block connect the same few large components, and without this the lists stop shrinking and
// thousands of lanes hit the same best[] entries with atomics.  (Merging per pair in the first list round was measured
// slower: 2.5 vs 1.4 ms -- its records are already merged per tile.)
template <bool SEG, int NT>
__device__ __forceinline__ void edge_round_body(const uint32_t *ea, const uint32_t *eb, const uint32_t *ek, uint32_t n,
                                                const uint32_t *segcount, uint32_t segcap, const uint32_t *cur,
                                                unsigned long long *best, uint32_t B, uint32_t *oa, uint32_t *ob, uint32_t *ok,
                                                uint32_t *ocount, uint32_t blk, uint32_t nblk) {
  constexpr bool DEDUP = !SEG;
  __shared__ uint32_t wtot[NT / 64];
  __shared__ uint32_t bbase, dn;
  __shared__ unsigned long long dt_pair[DEDUP ? DT_SLOTS : 1];
  __shared__ uint32_t dt_key[DEDUP ? DT_SLOTS : 1];
  __shared__ uint16_t dt_list[DEDUP ? DT_SLOTS : 1];
  for (size_t i0 = (size_t)blk * (NT * EPT); i0 < (size_t)n; i0 += (size_t)nblk * (NT * EPT)) {
  size_t lim = n;   // records of this block's range that exist
  if (SEG && NT == NTHR) {   // (a block's range lies in one segment; a wider workgroup's may not: per record below)
    const uint32_t seg = (uint32_t)(i0 / segcap);
    lim = (size_t)seg * segcap + segcount[seg];
    if (i0 >= lim) continue;
  }
  if (DEDUP) {
    for (int i = threadIdx.x; i < DT_SLOTS; i += NT) { dt_pair[i] = ~0ull; dt_key[i] = 0xFFFFFFFFu; }
    if (threadIdx.x == 0) dn = 0;
  }
  uint32_t a[EPT], b[EPT], k[EPT];
  bool ok_[EPT];
#pragma unroll
  for (int r = 0; r < EPT; r++) {
    const size_t i = i0 + (size_t)r * NT + threadIdx.x;
    ok_[r] = i < lim;
    if (SEG && NT != NTHR && ok_[r]) ok_[r] = i % segcap < segcount[i / segcap];
    a[r] = ok_[r] ? ea[i] : B;   // an absent record reads as (outside, outside): dead
    b[r] = ok_[r] ? eb[i] : B;
    k[r] = ok_[r] ? ek[i] : 0u;
  }
  uint32_t ca[EPT], cb[EPT];
#pragma unroll
  for (int r = 0; r < EPT; r++) { ca[r] = cur[a[r] & ~CLOSED]; cb[r] = cur[b[r] & ~CLOSED]; }
  bool live[EPT];
#pragma unroll
  for (int r = 0; r < EPT; r++) live[r] = ca[r] != cb[r] && !(ca[r] & cb[r] & CLOSED);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t nd = 0;
  if (DEDUP) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < EPT; r++) {
      if (live[r]) {
        const uint32_t lo = ca[r] < cb[r] ? ca[r] : cb[r], hi = ca[r] < cb[r] ? cb[r] : ca[r];
        if (pair_insert<DT_SLOTS>(dt_pair, dt_key, lo, hi, k[r])) live[r] = false;   // merged; else it stays a record of its own
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DT_SLOTS; i += NT) {
      const bool occ = dt_pair[i] != ~0ull;
      const unsigned long long bal = __ballot(occ);
      uint32_t base = 0;
      if (lane == 0 && bal) base = atomicAdd(&dn, (uint32_t)__popcll(bal));
      base = __shfl(base, 0, 64);
      if (occ) dt_list[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)i;
    }
    __syncthreads();
    nd = dn;
    for (uint32_t i = threadIdx.x; i < nd; i += NT) {
      const int sl = dt_list[i];
      const unsigned long long pr = dt_pair[sl];
      const uint32_t lo = (uint32_t)(pr >> 32), hi = (uint32_t)pr, key = dt_key[sl];
      const unsigned long long cl = ((unsigned long long)key << 32) | hi, ch = ((unsigned long long)key << 32) | lo;
      if (!(lo & CLOSED) && cl < best[lo]) atomicMin(&best[lo], cl);
      if (!(hi & CLOSED) && ch < best[hi]) atomicMin(&best[hi], ch);
    }
  }
  unsigned long long pa[EPT], pb[EPT];   // current best of either side (possibly stale: only a pre-check)
#pragma unroll
  for (int r = 0; r < EPT; r++) {
    pa[r] = (live[r] && !(ca[r] & CLOSED)) ? best[ca[r]] : 0ull;
    pb[r] = (live[r] && !(cb[r] & CLOSED)) ? best[cb[r]] : 0ull;
  }
#pragma unroll
  for (int r = 0; r < EPT; r++) {
    const unsigned long long candA = ((unsigned long long)k[r] << 32) | cb[r];
    const unsigned long long candB = ((unsigned long long)k[r] << 32) | ca[r];
    if (candA < pa[r]) atomicMin(&best[ca[r]], candA);
    if (candB < pb[r]) atomicMin(&best[cb[r]], candB);
  }
  // survivors -> next list, in order, one global atomic per block
  unsigned long long bal[EPT];
  uint32_t mine = 0;
#pragma unroll
  for (int r = 0; r < EPT; r++) { bal[r] = __ballot(live[r]); mine += (uint32_t)__popcll(bal[r]); }
  if (lane == 0) wtot[wv] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = nd;
    for (int q = 0; q < NT / 64; q++) tot += wtot[q];
    bbase = tot ? atomicAdd(ocount, tot) : 0;
  }
  __syncthreads();
  uint32_t off = bbase;
  if (DEDUP) {
    for (uint32_t i = threadIdx.x; i < nd; i += NT) {
      const int sl = dt_list[i];
      const unsigned long long pr = dt_pair[sl];
      oa[off + i] = (uint32_t)(pr >> 32); ob[off + i] = (uint32_t)pr; ok[off + i] = dt_key[sl];
    }
    off += nd;
  }
  for (int q = 0; q < wv; q++) off += wtot[q];
#pragma unroll
  for (int r = 0; r < EPT; r++) {
    if (live[r]) {
      const uint32_t g = off + (uint32_t)__popcll(bal[r] & ((1ull << lane) - 1ull));
      oa[g] = ca[r]; ob[g] = cb[r]; ok[g] = k[r];
    }
    off += (uint32_t)__popcll(bal[r]);
  }
  __syncthreads();   // (the next chunk of the block reuses the tables)
  }
}
template <bool SEG>
__global__ __launch_bounds__(NTHR) void k_edge_round(const uint32_t *__restrict__ ea, const uint32_t *__restrict__ eb,
                                                     const uint32_t *__restrict__ ek, uint32_t n,
                                                     const uint32_t *__restrict__ segcount, uint32_t segcap,
                                                     const uint32_t *__restrict__ cur, unsigned long long *best, uint32_t B,
                                                     uint32_t *oa, uint32_t *ob, uint32_t *ok, uint32_t *ocount,
                                                     const uint32_t *__restrict__ dyn = nullptr, TailGate gate = TailGate()) {
  if (gate.taken()) return;
  if (dyn) n = *dyn;   // (the dense rounds: the record count the round before left on the device)
  edge_round_body<SEG, NTHR>(ea, eb, ek, n, segcount, segcap, cur, best, B, oa, ob, ok, ocount, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(NTHR) void k_sum_segments(const uint32_t *__restrict__ segcount, uint32_t nseg, uint32_t *total,
                                                       uint32_t *total2 = nullptr) {
  __shared__ uint32_t part[NTHR];
  uint32_t v = 0;
  for (uint32_t i = threadIdx.x; i < nseg; i += NTHR) v += segcount[i];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int st = NTHR / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *total = part[0];
    if (total2) *total2 = part[0];
  }
}

// alive flags -> list of tiles for the next round (roughly ascending: blocks append in launch order) + count
__global__ __launch_bounds__(NTHR) void k_compact_alive(const uint8_t *__restrict__ alive, uint32_t ntiles,
                                                        uint32_t *list, uint32_t *count) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  const bool hit = i < ntiles && alive[i] != 0;
  const uint32_t slot = block_append(hit, count);
  if (hit) list[slot] = i;
}

template <int NT>
__device__ __forceinline__ void hook_body(const uint32_t *roots, uint32_t nroots, const unsigned long long *best,
                                          unsigned long long *link, uint32_t blk, uint32_t nblk) {
  for (uint32_t i = blk * NT + threadIdx.x; i < nroots; i += nblk * NT) {
    const uint32_t r = roots[i];
    const unsigned long long b = best[r];
    const uint32_t t = (uint32_t)b;
    bool keep_root = false;
    if (b == ~0ull) keep_root = true;  // no neighbouring component (cannot happen on a connected raster)
    else if (!(t & CLOSED)) {
      // mutual lowest pass: the pair merges, the smaller id stays root (the pass heights agree
      // because both sides see the same cell pair).  Closed components never choose, so never mutual.
      keep_root = ((uint32_t)best[t] == r) && (r < t);
    }
    link[r] = keep_root ? (unsigned long long)r : b;
  }
}
__global__ __launch_bounds__(NTHR) void k_hook(const uint32_t *__restrict__ roots, uint32_t nroots,
                                               const unsigned long long *__restrict__ best,
                                               unsigned long long *link, const uint32_t *__restrict__ dyn = nullptr,
                                               TailGate gate = TailGate()) {
  if (gate.taken()) return;
  if (dyn) nroots = *dyn;
  hook_body<NTHR>(roots, nroots, best, link, blockIdx.x, gridDim.x);
}

// pointer jumping over this round's hook forest, carrying the path maximum in the high word.
template <int NT>
__device__ __forceinline__ void chase_links_body(const uint32_t *roots, uint32_t nroots, unsigned long long *link, int maxhops,
                                                 uint32_t *flag, uint32_t blk, uint32_t nblk) {
  for (uint32_t i = blk * NT + threadIdx.x; i < nroots; i += nblk * NT) {
    const uint32_t r = roots[i];
    unsigned long long l = __hip_atomic_load(&link[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t p = (uint32_t)l, m = (uint32_t)(l >> 32);
    if (p == r) continue;
    const uint32_t p0 = p;
    int hops = 0;
    bool unfinished = false;
    for (;;) {
      if (p & CLOSED) break;   // the outside / a frozen terminal: a root by definition
      const unsigned long long lp = __hip_atomic_load(&link[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t pp = (uint32_t)lp;
      if (pp == p) break;
      const uint32_t mm = (uint32_t)(lp >> 32);
      p = pp;
      m = mm > m ? mm : m;
      if (++hops >= maxhops) { unfinished = true; break; }
    }
    if (p != p0)
      __hip_atomic_store(&link[r], ((unsigned long long)m << 32) | p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (unfinished) *flag = 1;
  }
}
__global__ __launch_bounds__(NTHR) void k_chase_links(const uint32_t *__restrict__ roots, uint32_t nroots,
                                                      unsigned long long *link, int maxhops, uint32_t *flag,
                                                      const uint32_t *__restrict__ dyn = nullptr, TailGate gate = TailGate()) {
  if (gate.taken()) return;
  if (dyn) nroots = *dyn;
  chase_links_body<NTHR>(roots, nroots, link, maxhops, flag, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(NTHR) void k_update_basins(uint32_t *cur, uint32_t *acc,
                                                        const unsigned long long *__restrict__ link, uint32_t B,
                                                        const uint32_t *__restrict__ dyn = nullptr) {
  if (dyn && *dyn == 0u) return;   // (a round enqueued after the last: nothing hooked)
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  const uint32_t c = cur[b];
  if (c & CLOSED) return;
  const unsigned long long l = link[c];
  const uint32_t p = (uint32_t)l, m = (uint32_t)(l >> 32);
  if (p != c) {
    cur[b] = p;
    if (m > acc[b]) acc[b] = m;
  }
}

constexpr int RPT = 8;   // roots per thread: 2048 per block, so a round over 1e7 roots is 5e3 same-address atomics
// curw (the compact-label fill): cur[r] = parent of r for EVERY root of the round.  The next round's k_edge_round looks
// cur[] up for the ids in its records only, and those are this round's roots (round 2: basin ids, every open basin being a
// root of round 1) or closed ids, whose cur[] k_init_tables wrote for good.  All other entries of cur[] are stale until
// k_settle_basins.
template <int NT>
__device__ __forceinline__ void compact_roots_body(const uint32_t *roots_in, uint32_t nroots, const unsigned long long *link,
                                                   uint32_t *roots_out, uint32_t *counter, uint32_t *curw, uint32_t blk,
                                                   uint32_t nblk) {
  __shared__ uint32_t wtot[NT / 64];
  __shared__ uint32_t bbase;
  for (uint32_t i0 = blk * (NT * RPT); i0 < nroots; i0 += nblk * (NT * RPT)) {
  uint32_t r[RPT];
  bool ok[RPT];
#pragma unroll
  for (int q = 0; q < RPT; q++) {
    const uint32_t i = i0 + q * NT + threadIdx.x;
    ok[q] = i < nroots;
    r[q] = ok[q] ? roots_in[i] : 0u;
  }
  bool keep[RPT];
#pragma unroll
  for (int q = 0; q < RPT; q++) {
    const uint32_t p = ok[q] ? (uint32_t)link[r[q]] : 0u;
    keep[q] = ok[q] && p == r[q];
    if (curw && ok[q]) curw[r[q]] = p;   // (the parent as k_hook / k_chase_links left it: its CLOSED bit included)
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long bal[RPT];
  uint32_t mine = 0;
#pragma unroll
  for (int q = 0; q < RPT; q++) { bal[q] = __ballot(keep[q]); mine += (uint32_t)__popcll(bal[q]); }
  if (lane == 0) wtot[wv] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (int k = 0; k < NT / 64; k++) tot += wtot[k];
    bbase = tot ? atomicAdd(counter, tot) : 0;
  }
  __syncthreads();
  uint32_t off = bbase;
  for (int k = 0; k < wv; k++) off += wtot[k];
#pragma unroll
  for (int q = 0; q < RPT; q++) {
    if (keep[q]) roots_out[off + (uint32_t)__popcll(bal[q] & ((1ull << lane) - 1ull))] = r[q];
    off += (uint32_t)__popcll(bal[q]);
  }
  __syncthreads();   // (the next chunk of the block reuses wtot / bbase)
  }
}
__global__ __launch_bounds__(NTHR) void k_compact_roots(const uint32_t *__restrict__ roots_in, uint32_t nroots,
                                                        const unsigned long long *__restrict__ link,
                                                        uint32_t *roots_out, uint32_t *counter,
                                                        const uint32_t *__restrict__ dyn = nullptr, uint32_t *curw = nullptr,
                                                        TailGate gate = TailGate()) {
  if (gate.taken()) return;
  if (dyn) nroots = *dyn;
  compact_roots_body<NTHR>(roots_in, nroots, link, roots_out, counter, curw, blockIdx.x, gridDim.x);
}

// The basins' final components and levels, once, after the last round (the compact-label fill; the other paths update
// cur[] / acc[] in every round, k_update_basins).  link[r] of a root that died is never written again -- k_hook and
// k_chase_links run over the live roots only -- so after the rounds link[] is the whole merge forest, each word carrying the
// highest pass on its hop: cur[b] = the end of b's chain (a self-link or a closed parent), acc[b] = the highest pass on the
// way, which is what the per-round updates accumulated.  A basin that never hooked (a frozen terminal, the outside) keeps
// what k_init_tables wrote.  A chain has at most one hop per round with work; it is stored back shortened (any value ever
// stored is a valid continuation: concurrent walkers and stale reads are harmless).
__global__ __launch_bounds__(NTHR) void k_settle_basins(uint32_t *cur, uint32_t *acc, unsigned long long *link, uint32_t B,
                                                        int maxhops, uint32_t *flag) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  const unsigned long long l = __hip_atomic_load(&link[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t p = (uint32_t)l, m = (uint32_t)(l >> 32);
  if (p == b) return;
  const uint32_t p0 = p;
  int hops = 0;
  for (;;) {
    if (p & CLOSED) break;
    const unsigned long long lp = __hip_atomic_load(&link[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t pp = (uint32_t)lp;
    if (pp == p) break;
    const uint32_t mm = (uint32_t)(lp >> 32);
    p = pp;
    m = mm > m ? mm : m;
    if (++hops >= maxhops) { *flag = 1; break; }
  }
  if (p != p0)
    __hip_atomic_store(&link[b], ((unsigned long long)m << 32) | p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  cur[b] = p;
  acc[b] = m;
}

// The small rounds of the compact-label fill in ONE launch: a single workgroup runs best_reset -> edge_round -> hook ->
// chase -> compact round after round, __syncthreads() between the phases (no grid-wide barrier, no waiting on another
// block), the root and record lists ping-ponging by the round's parity as on the host.  It takes over at the first round of
// [rlo, rhi] whose gate holds (the full-width kernels of that round and of every later one have returned at once), runs until
// no live root is left or round rmax is done, and leaves rc[4 r] / rc[4 r + 1] as the full-width kernels would, plus the
// last round anybody ran in rc[2].  No gate holds: it does nothing, and the host enqueues more rounds.
constexpr int TAILT = 1024;
// Thresholds, measured at S3 (40000^2, 1.03e7 basins, ms per fill): 0 (no tail kernel) 15.37, 1024 roots 15.36, 4096 15.40,
// 16384 15.50, 131072 18.0 -- one workgroup pays ~20 us a round in dependent round trips whatever the round's size, which is
// what five launches of an almost empty round cost too, and it loses as soon as a round has more than a few chunks of records.
constexpr uint32_t TAIL_ROOTS = 1024, TAIL_RECS_PER_ROOT = 8;   // take a round of <= 1024 roots and <= 8192 records
struct TailArgs {
  uint32_t *roots[2];   // round r reads roots[(r - 1) & 1]
  uint32_t *el[2];      // round r >= 2 reads el[r & 1]: three arrays of pcap records
  size_t pcap;
  const uint32_t *segcount;   // round 2: the raster pass's segmented list
  uint32_t segcap;
  uint32_t *cur;
  unsigned long long *best, *link;
  uint32_t B;
  uint32_t *rc, *flag;
  uint32_t troots, trecs;
  int rlo, rhi, rmax, maxhops;
};
__global__ __launch_bounds__(TAILT) void k_rounds_tail(TailArgs a) {
  auto count = [&](int i) { return __hip_atomic_load(&a.rc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  int r = a.rlo;
  for (; r <= a.rhi; r++)
    if (count(4 * r) <= a.troots && count(4 * r + 1) <= a.trecs) break;
  if (r > a.rhi) return;
  for (; r <= a.rmax; r++) {
    const uint32_t nr = count(4 * r), ne = count(4 * r + 1);
    if (nr == 0) break;
    const uint32_t *rin = a.roots[(r - 1) & 1];
    uint32_t *rout = a.roots[r & 1];
    const uint32_t *ei = a.el[r & 1];
    uint32_t *eo = a.el[(r + 1) & 1];
    best_reset_body<TAILT>(rin, nr, a.best, 0, 1);
    __syncthreads();
    if (r == 2)
      edge_round_body<true, TAILT>(ei, ei + a.pcap, ei + 2 * a.pcap, (uint32_t)a.pcap, a.segcount, a.segcap, a.cur, a.best, a.B, eo,
                                   eo + a.pcap, eo + 2 * a.pcap, &a.rc[4 * (r + 1) + 1], 0, 1);
    else
      edge_round_body<false, TAILT>(ei, ei + a.pcap, ei + 2 * a.pcap, ne, nullptr, 0u, a.cur, a.best, a.B, eo, eo + a.pcap,
                                    eo + 2 * a.pcap, &a.rc[4 * (r + 1) + 1], 0, 1);
    __syncthreads();
    hook_body<TAILT>(rin, nr, a.best, a.link, 0, 1);
    __syncthreads();
    chase_links_body<TAILT>(rin, nr, a.link, a.maxhops, a.flag, 0, 1);
    __syncthreads();
    compact_roots_body<TAILT>(rin, nr, a.link, rout, &a.rc[4 * (r + 1)], a.cur, 0, 1);
    __syncthreads();
  }
  if (threadIdx.x == 0) a.rc[2] = (uint32_t)(r - 1);
}

// ------------------------------------------------------------------------------------------
// 5. finalize
// ------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(NTHR) void k_finalize(T *z, const uint32_t *__restrict__ lab,
                                                   const uint32_t *__restrict__ acc, uint32_t n, uint32_t B) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c64 = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c64 < n; c64 += stride) {
    const uint32_t c = (uint32_t)c64;
    const uint32_t b = lab[c];
    if (b == B) continue;
    const uint32_t L = acc[b];
    if (L > Key32<T>::to(z[c])) z[c] = Key32<T>::from(L);
  }
}

// ------------------------------------------------------------------------------------------
// 6. row-block shards (Barnes 2016 tile protocol; reference programs/parallel_priority_flood/main.cpp,
//    Zhou2016pf.hpp): after the local phase every cell knows its watershed label (a cut-row terminal or
//    the outside) and its locally filled level.  What the global solve needs from a shard is, for every
//    pair of adjacent watersheds, the lowest pass between them (WatershedsMeet, Zhou2016pf.hpp:37-62).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t shard_label(uint32_t c, const uint32_t *__restrict__ lab,
                                                const uint32_t *__restrict__ cur, const uint32_t *__restrict__ tid,
                                                uint32_t B) {
  const uint32_t l = cur[lab[c]] & ~CLOSED;
  return l == B ? NO_TID : tid[l];   // NO_TID doubles as "the outside" in exported edges
}

// open-addressing table of (min(la,lb) << 32 | max(la,lb)) + 1 -> lowest pass key.
// One 64x32 tile per block: the watershed label (three dependent gathers: basin -> component -> terminal id) and
// the locally filled level of every cell of the tile and of its forward halo are fetched ONCE, in three batches,
// into LDS; the pair tests then run on LDS and only cells on a watershed boundary touch the global table.
constexpr int EW = 64, EH = 32, ELW = EW + 2, ELH = EH + 1;
constexpr uint32_t E_INVALID = 0xFFFFFFFEu;   // outside the raster: pairs with it are skipped
template <class T, int TOPO>
__global__ __launch_bounds__(NTHR) void k_shard_edges(const T *__restrict__ z, const uint32_t *__restrict__ lab,
                                                      const uint32_t *__restrict__ cur, const uint32_t *__restrict__ acc,
                                                      const uint32_t *__restrict__ tid, uint32_t B, int w, int h,
                                                      unsigned long long *hkeys, uint32_t *hvals, uint32_t hmask,
                                                      uint32_t *overflow, uint32_t tilesX, uint32_t ntiles) {
  __shared__ uint32_t sl[ELH * ELW];
  __shared__ uint32_t sw[ELH * ELW];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * EW, y0 = (int)(t / tilesX) * EH;
  constexpr int IPT = (ELH * ELW + NTHR - 1) / NTHR;
  uint32_t lv[IPT], kv[IPT];
  bool ok[IPT];
#pragma unroll
  for (int r = 0; r < IPT; r++) {   // batch 1: basin label and elevation key
    const int i = threadIdx.x + r * NTHR;
    const int ly = i / ELW, lx = i - ly * ELW;
    const int gx = x0 - 1 + lx, gy = y0 + ly;
    ok[r] = i < ELH * ELW && gx >= 0 && gx < w && gy < h;
    lv[r] = B;
    kv[r] = 0;
    if (ok[r]) { lv[r] = lab[(size_t)gy * w + gx]; kv[r] = Key32<T>::to(z[(size_t)gy * w + gx]); }
  }
  uint32_t cv[IPT], av[IPT];
#pragma unroll
  for (int r = 0; r < IPT; r++) {   // batch 2: component and filled level (label B = the outside: cur[B], acc[B] exist)
    cv[r] = cur[lv[r]] & ~CLOSED;
    av[r] = acc[lv[r]];
  }
  uint32_t tv[IPT];
#pragma unroll
  for (int r = 0; r < IPT; r++) tv[r] = cv[r] == B ? NO_TID : tid[cv[r]];   // batch 3: NO_TID doubles as "the outside"
#pragma unroll
  for (int r = 0; r < IPT; r++) {
    const int i = threadIdx.x + r * NTHR;
    if (i < ELH * ELW) {
      sl[i] = ok[r] ? tv[r] : E_INVALID;
      sw[i] = (lv[r] != B && av[r] > kv[r]) ? av[r] : kv[r];
    }
  }
  __syncthreads();
  const int lx = threadIdx.x & (EW - 1), ly0 = threadIdx.x >> 6;
#pragma unroll 2
  for (int j = 0; j < EH / 4; j++) {
    const int ly = ly0 + 4 * j;
    const int o = ly * ELW + lx + 1;
    const uint32_t la = sl[o];
    if (la == E_INVALID) continue;
    const uint32_t wa = sw[o];
    // forward neighbours only (E, SW, S, SE): every adjacent pair is seen once
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (TOPO == 4 && (k == 1 || k == 3)) continue;
      const int q = o + (k == 0 ? 1 : k == 1 ? ELW - 1 : k == 2 ? ELW : ELW + 1);
      const uint32_t lb = sl[q];
      if (lb == la || lb == E_INVALID) continue;
      const uint32_t wb = sw[q];
      const uint32_t pass = wa > wb ? wa : wb;
      const uint32_t lo = la < lb ? la : lb, hi = la < lb ? lb : la;
      const unsigned long long key = (((unsigned long long)lo << 32) | hi) + 1ull;   // never 0 (lo != hi)
      uint32_t slot = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & hmask;
      for (uint32_t probe = 0;; probe++) {
        if (probe > hmask) { *overflow = 1; break; }
        unsigned long long cur_k = __hip_atomic_load(&hkeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur_k == 0) cur_k = atomicCAS(&hkeys[slot], 0ull, key);
        if (cur_k == 0 || cur_k == key) {
          if (__hip_atomic_load(&hvals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pass) atomicMin(&hvals[slot], pass);
          break;
        }
        slot = (slot + 1) & hmask;
      }
    }
  }
}


__global__ __launch_bounds__(NTHR) void k_shard_edges_compact(const unsigned long long *__restrict__ hkeys,
                                                              const uint32_t *__restrict__ hvals, uint32_t hsize,
                                                              uint32_t *edges, uint32_t *nedges) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;   // grid covers whole waves
  const bool used = i < hsize && hkeys[i] != 0;
  const unsigned long long bal = __ballot(used);
  if (bal == 0) return;
  const int lane = threadIdx.x & 63, leader = (int)__ffsll((long long)bal) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(nedges, (uint32_t)__popcll(bal));
  base = __shfl(base, leader, 64);
  if (used) {
    const unsigned long long k = hkeys[i] - 1ull;
    const uint32_t e = base + __popcll(bal & ((1ull << lane) - 1ull));
    edges[3 * e] = (uint32_t)(k >> 32);
    edges[3 * e + 1] = (uint32_t)k;
    edges[3 * e + 2] = hvals[i];
  }
}

// raise every basin by the globally solved level of its watershed's terminal (SecondRound,
// parallel_priority_flood/main.cpp:315-321): levels[tid] for tid in [0, 2w)
__global__ __launch_bounds__(NTHR) void k_shard_apply(const uint32_t *__restrict__ cur, uint32_t *acc,
                                                      const uint32_t *__restrict__ tid,
                                                      const uint32_t *__restrict__ levels, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  const uint32_t l = cur[b] & ~CLOSED;
  if (l == B) return;   // drains to the true border inside this shard: already final
  const uint32_t g = levels[tid[l]];
  if (g > acc[b]) acc[b] = g;
}

// ------------------------------------------------------------------------------------------
// host driver
// ------------------------------------------------------------------------------------------
// Phases 1-4: descent forest, basins, Boruvka rounds.  With open_top/open_bottom the first/last row is
// a cut row of a row-block shard whose cells are frozen terminals.
template <class T, int TOPO>
static void fill_local_phase(const T *d_z, int w, int h, int open_top, int open_bottom, BufAlloc alloc, FillBuffers &fb,
                             hipStream_t s, const uint8_t *outlet = nullptr) {
  const uint64_t n64 = (uint64_t)w * (uint64_t)h;
  if (n64 > 0x7FFF0000ull) throw Error(RDGPU_ERR_ARG, "rdgpu_fill: raster (or shard) has more than 2^31-65536 cells");
  const uint32_t n = (uint32_t)n64;
  g_stats = rdgpu_fill_stats{n64, 0, 0, 0, 0, (uint32_t)(TW * TH), 0};
  fb = FillBuffers();
  const bool sharded = open_top || open_bottom;
  if (w <= 2 || (!sharded && h <= 2)) { fb.trivial = true; return; }  // every cell is a border cell

  Workspace &ws = Workspace::get();
  uint32_t *lab = alloc.get<uint32_t>("fill.lab", n);
  fb.lab = lab;
  uint32_t *dflags = ws.buf<uint32_t>("fill.flags", 16);  // [0] chase flag, [1] pit total, [2] root counter
  uint32_t *hw = ws.host_words();

  const uint32_t tilesX = cdiv(w, TW), tilesY = cdiv(h, TH), ntiles = tilesX * tilesY;
  const uint32_t sgrid = std::min(cdiv(n, NTHR), 256u * 32u);  // grid-stride 1-D kernels

  // descent forest: one word per cell (basin id / pending pointer / off the raster); pits are numbered by the same kernel
  const uint32_t dtx = cdiv(w, DW), dnt = dtx * cdiv(h, DH);
  RD_HIP(hipMemsetAsync(dflags, 0, 2 * sizeof(uint32_t), s));
  // naturally aligned quads when every row starts on a quad boundary; the any-width quad loads otherwise
  const bool vec = (w % 4) == 0 && (reinterpret_cast<uintptr_t>(d_z) % (4 * sizeof(T))) == 0;
  if (vec)
    RD_LAUNCH("fill.descent", (k_descent<T, TOPO, true>), dim3(xcd_grid(dnt)), dim3(NTHR), 0, s, d_z, lab, dflags + 1, w,
              h, dtx, dnt, open_top, open_bottom, outlet);
  else
    RD_LAUNCH("fill.descent", (k_descent<T, TOPO, false>), dim3(xcd_grid(dnt)), dim3(NTHR), 0, s, d_z, lab, dflags + 1, w,
              h, dtx, dnt, open_top, open_bottom, outlet);
  RD_HIP(hipMemcpyAsync(hw, dflags + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  const uint32_t B = hw[0];
  g_stats.basins = B;
  fb.B = B;
  if (B == 0) { fb.trivial = true; return; }  // no pits and no terminals: nothing to raise
  RD_LAUNCH("fill.tile_label", k_tile_label, dim3(xcd_grid(dnt)), dim3(NTHR), 0, s, lab, w, h, dtx, dnt, B, 256, dflags);
  RD_HIP(hipMemcpyAsync(hw, dflags, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  g_stats.jump_passes = 1;
  if (hw[0] != 0) {
    // pathologically long tile-to-tile chains: compress them (each pass shortens every path >= 32x), relabel
    for (;;) {
      RD_HIP(hipMemsetAsync(dflags, 0, sizeof(uint32_t), s));
      RD_LAUNCH("fill.chase", k_chase, dim3(sgrid), dim3(NTHR), 0, s, lab, n, 32, dflags);
      RD_HIP(hipMemcpyAsync(hw, dflags, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      RD_HIP(hipStreamSynchronize(s));
      g_stats.jump_passes++;
      if (hw[0] == 0) break;
    }
    RD_LAUNCH("fill.label_cells", k_label_cells, dim3(sgrid), dim3(NTHR), 0, s, lab, n, B);
  }

  uint32_t *cur = alloc.get<uint32_t>("fill.cur", (size_t)B + 1);
  uint32_t *acc = alloc.get<uint32_t>("fill.acc", (size_t)B + 1);
  fb.cur = cur;
  fb.acc = acc;
  uint32_t *tid = nullptr;
  if (sharded) {
    tid = alloc.get<uint32_t>("fill.tid", (size_t)B + 1);
    fb.tid = tid;
    RD_HIP(hipMemsetAsync(tid, 0xFF, ((size_t)B + 1) * sizeof(uint32_t), s));
    RD_LAUNCH("fill.mark_terminals", k_mark_terminals, dim3(cdiv(w, NTHR)), dim3(NTHR), 0, s, lab, tid, w, h, open_top,
              open_bottom);
  }
  unsigned long long *best = ws.buf<unsigned long long>("fill.best", (size_t)B + 1);
  unsigned long long *link = ws.buf<unsigned long long>("fill.link", (size_t)B + 1);
  uint32_t *rootsA = ws.buf<uint32_t>("fill.rootsA", B);
  uint32_t *rootsB = ws.buf<uint32_t>("fill.rootsB", B);
  RD_HIP(hipMemsetAsync(dflags + 2, 0, sizeof(uint32_t), s));
  RD_LAUNCH("fill.init_tables", k_init_tables, dim3(cdiv((uint64_t)B + 1, NTHR)), dim3(NTHR), 0, s, cur, acc, link,
            rootsA, dflags + 2, (const uint32_t *)tid, B);
  RD_HIP(hipMemcpyAsync(hw, dflags + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));

  uint32_t nroots = hw[0];
  // per-tile flag "still holds a component boundary" (ping-pong); round 1 visits every tile
  uint8_t *alive = ws.buf<uint8_t>("fill.alive", ntiles);
  uint32_t *tlist = ws.buf<uint32_t>("fill.tlist", ntiles);
  uint32_t nlive = ntiles;
  bool first = true;
  // The pair list (see k_scan EMIT): round 1 is the only raster pass unless something overflows.  Capacity: 12
  // records per basin (measured at S3: 4.6), at most one per two cells; per segment a multiple of a k_edge_round block.
  // RDGPU_FILL_EDGES=0 keeps every round on the raster; RDGPU_FILL_EDGE_CAP=<records> overrides the list capacity
  // (both exist for the tests of the overflow fallback and for A/B timing).
  const char *env_edges = getenv("RDGPU_FILL_EDGES"), *env_cap = getenv("RDGPU_FILL_EDGE_CAP");
  const bool edges_enabled = !(env_edges && env_edges[0] == '0');
  bool edge_mode = false;           // rounds 2.. run on the pair list
  EdgeOut eo{};
  uint32_t nseg = 1, nedges = 0;
  uint32_t *elist[2] = {nullptr, nullptr};   // ping-pong record buffers: a | b | k planes of ecap[] records
  size_t ecap[2] = {0, 0};
  int ein = 0;
  bool eseg = true;                 // the input list is still the segmented one of the raster pass
  if (edges_enabled && nroots > 0) {
    while (nseg < ESEG && (uint64_t)nseg * 128 <= ntiles) nseg *= 2;
    const uint64_t cap = env_cap ? strtoull(env_cap, nullptr, 10) : std::min<uint64_t>(12ull * B, n / 2) + 2048;
    const uint32_t segcap = cdiv(cdiv(cap, nseg), NTHR * EPT) * (NTHR * EPT);
    ecap[0] = (size_t)nseg * segcap;
    elist[0] = ws.buf<uint32_t>("fill.edges0", 3 * ecap[0]);
    uint32_t *segcount = ws.buf<uint32_t>("fill.segcount", nseg);
    RD_HIP(hipMemsetAsync(segcount, 0, nseg * sizeof(uint32_t), s));
    RD_HIP(hipMemsetAsync(dflags + 4, 0, 2 * sizeof(uint32_t), s));
    eo = EdgeOut{elist[0], elist[0] + ecap[0], elist[0] + 2 * ecap[0], segcount, segcap, nseg - 1, dflags + 5};
  }
  const bool emit = eo.a != nullptr;
  while (nroots > 0) {
    const uint32_t rgrid = cdiv(nroots, NTHR);
    RD_LAUNCH("fill.best_reset", k_best_reset, dim3(rgrid), dim3(NTHR), 0, s, rootsA, nroots, best);
    RD_HIP(hipMemsetAsync(dflags + 3, 0, sizeof(uint32_t), s));
    if (edge_mode) {
      // contract the pair list: in -> out (dense), proposals to best[]
      const int eout = ein ^ 1;
      RD_HIP(hipMemsetAsync(dflags + 4, 0, sizeof(uint32_t), s));
      const uint32_t *ia = elist[ein], *ib = elist[ein] + ecap[ein], *ik = elist[ein] + 2 * ecap[ein];
      uint32_t *oa = elist[eout], *ob = elist[eout] + ecap[eout], *ok = elist[eout] + 2 * ecap[eout];
      if (eseg)
        RD_LAUNCH("fill.edge_round", (k_edge_round<true>), dim3(cdiv(ecap[ein], NTHR * EPT)), dim3(NTHR), 0, s, ia, ib, ik,
                  (uint32_t)ecap[ein], (const uint32_t *)eo.segcount, eo.segcap, (const uint32_t *)cur, best, B, oa, ob, ok,
                  dflags + 4);
      else if (nedges > 0)
        RD_LAUNCH("fill.edge_round", (k_edge_round<false>), dim3(cdiv(nedges, NTHR * EPT)), dim3(NTHR), 0, s, ia, ib, ik,
                  nedges, (const uint32_t *)nullptr, 0u, (const uint32_t *)cur, best, B, oa, ob, ok, dflags + 4);
      eseg = false;
      ein = eout;
    } else if (nlive > 0) {
#define RD_SCAN(FIRST_, VEC_, EMIT_, LIST, NWORK)                                                                \
  RD_LAUNCH("fill.scan", (k_scan<T, TOPO, FIRST_, VEC_, EMIT_>), dim3(xcd_grid(NWORK)), dim3(NTHR), 0, s, d_z, lab, cur, best, w, \
            h, B, tilesX, ntiles, (const uint32_t *)(LIST), (uint32_t)(NWORK), alive, eo)
#define RD_SCAN_V(FIRST_, EMIT_, LIST, NWORK)                                                                    \
  { if (vec) RD_SCAN(FIRST_, true, EMIT_, LIST, NWORK); else RD_SCAN(FIRST_, false, EMIT_, LIST, NWORK); }
      if (first && !sharded) { if (emit) RD_SCAN_V(true, true, nullptr, ntiles) else RD_SCAN_V(true, false, nullptr, ntiles) }
      else if (first) { if (emit) RD_SCAN_V(false, true, nullptr, ntiles) else RD_SCAN_V(false, false, nullptr, ntiles) }
      else RD_SCAN_V(false, false, tlist, nlive)
#undef RD_SCAN_V
#undef RD_SCAN
      RD_LAUNCH("fill.compact_alive", k_compact_alive, dim3(cdiv(ntiles, NTHR)), dim3(NTHR), 0, s, (const uint8_t *)alive, ntiles,
                tlist, dflags + 3);
      if (first && emit)
        RD_LAUNCH("fill.sum_segments", k_sum_segments, dim3(1), dim3(NTHR), 0, s, (const uint32_t *)eo.segcount, nseg, dflags + 4);
      g_stats.scan_tiles += first ? ntiles : nlive;
    }
    RD_LAUNCH("fill.hook", k_hook, dim3(rgrid), dim3(NTHR), 0, s, rootsA, nroots, best, link);
    for (;;) {
      RD_HIP(hipMemsetAsync(dflags, 0, sizeof(uint32_t), s));
      RD_LAUNCH("fill.chase_links", k_chase_links, dim3(rgrid), dim3(NTHR), 0, s, rootsA, nroots, link, 32, dflags);
      RD_HIP(hipMemcpyAsync(hw, dflags, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      RD_HIP(hipStreamSynchronize(s));
      if (hw[0] == 0) break;
    }
    RD_LAUNCH("fill.update_basins", k_update_basins, dim3(cdiv(B, NTHR)), dim3(NTHR), 0, s, cur, acc, link, B);
    RD_HIP(hipMemsetAsync(dflags + 2, 0, sizeof(uint32_t), s));
    RD_LAUNCH("fill.compact_roots", k_compact_roots, dim3(cdiv(nroots, NTHR * RPT)), dim3(NTHR), 0, s, rootsA, nroots, link,
              rootsB, dflags + 2);
    RD_HIP(hipMemcpyAsync(hw, dflags + 2, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    const uint32_t next = hw[0];
    if (next >= nroots) throw Error(RDGPU_ERR_HIP, "rdgpu_fill: contraction made no progress (internal error)");
    nroots = next;
    nlive = hw[1];
    if (first && emit && hw[3] == 0 && nroots > 0) {
      // the raster pass recorded every adjacent component pair: the remaining rounds run on that list
      edge_mode = true;
      nedges = hw[2];
      g_stats.edge_records = nedges;
      ecap[1] = std::max<size_t>(nedges, 1);
      elist[1] = ws.buf<uint32_t>("fill.edges1", 3 * ecap[1]);
    } else if (edge_mode) {
      nedges = hw[2];
    }
    first = false;
    std::swap(rootsA, rootsB);
    g_stats.rounds++;
  }
}

// The local phase of a whole raster on workspace buffers, for the other files of the library (fill_shared.hpp).
template <class T>
void fill_local_phase_plain(const T *d_z, int w, int h, int topology, FillBuffers &fb, hipStream_t s) {
  BufAlloc ws_alloc{false, nullptr};
  if (topology == 8) fill_local_phase<T, 8>(d_z, w, h, 0, 0, ws_alloc, fb, s);
  else fill_local_phase<T, 4>(d_z, w, h, 0, 0, ws_alloc, fb, s);
}
template void fill_local_phase_plain<uint8_t>(const uint8_t *, int, int, int, FillBuffers &, hipStream_t);
template void fill_local_phase_plain<int8_t>(const int8_t *, int, int, int, FillBuffers &, hipStream_t);
template void fill_local_phase_plain<int16_t>(const int16_t *, int, int, int, FillBuffers &, hipStream_t);
template void fill_local_phase_plain<uint16_t>(const uint16_t *, int, int, int, FillBuffers &, hipStream_t);
template void fill_local_phase_plain<int32_t>(const int32_t *, int, int, int, FillBuffers &, hipStream_t);
template void fill_local_phase_plain<uint32_t>(const uint32_t *, int, int, int, FillBuffers &, hipStream_t);
template void fill_local_phase_plain<float>(const float *, int, int, int, FillBuffers &, hipStream_t);

// The same in tile order (64 x 32 tiles, XCD-banded, aligned quads): the cells of a tile share a few dozen basins, so
// the acc[] lines stay in the XCD's L2 while the tile is worked on -- in row order every row segment of a basin
// fetched its line again (5.5 GB of gathers on top of 12.8 GB of rows at S3).  A quad is written back only when one of
// its cells is raised (unchanged cells get their own bits back).
template <class T>
__global__ __launch_bounds__(NTHR) void k_finalize_tiled(T *z, const uint32_t *__restrict__ lab,
                                                         const uint32_t *__restrict__ acc, int w, int h, uint32_t B,
                                                         uint32_t tilesX, uint32_t ntiles) {
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * TW, y0 = (int)(t / tilesX) * TH;
  const int gx = x0 + 4 * (threadIdx.x & 15), ry = threadIdx.x >> 4;   // 16 quads per row, rows ry and ry + 16
  struct alignas(4 * sizeof(T)) ZQ { T v[4]; };
  ZQ zq[2];
  uint4 lq[2];
  bool ok[2];
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int gy = y0 + ry + 16 * r;
    ok[r] = gx < w && gy < h;
    const size_t g = ok[r] ? (size_t)gy * w + gx : 0;
    zq[r] = *reinterpret_cast<const ZQ *>(z + g);
    lq[r] = *reinterpret_cast<const uint4 *>(lab + g);
  }
  uint32_t L[2][4];
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const uint32_t l[4] = {lq[r].x, lq[r].y, lq[r].z, lq[r].w};
#pragma unroll
    for (int e = 0; e < 4; e++) L[r][e] = acc[l[e]];   // acc[B] (the outside) is 0: never above a key that matters
  }
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const uint32_t l[4] = {lq[r].x, lq[r].y, lq[r].z, lq[r].w};
    bool any = false;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (l[e] != B && L[r][e] > Key32<T>::to(zq[r].v[e])) { zq[r].v[e] = Key32<T>::from(L[r][e]); any = true; }
    }
    if (any && ok[r]) *reinterpret_cast<ZQ *>(z + (size_t)(y0 + ry + 16 * r) * w + gx) = zq[r];
  }
}

template <class T>
static void fill_finalize(T *d_z, int w, int h, const FillBuffers &fb, hipStream_t s) {
  if (fb.trivial) return;
  const uint32_t n = (uint32_t)((uint64_t)w * h);
  if ((w % 4) == 0 && (reinterpret_cast<uintptr_t>(d_z) % (4 * sizeof(T))) == 0) {
    const uint32_t tilesX = cdiv(w, TW), ntiles = tilesX * cdiv(h, TH);
    RD_LAUNCH("fill.finalize", (k_finalize_tiled<T>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_z, fb.lab, fb.acc, w, h, fb.B,
              tilesX, ntiles);
    return;
  }
  const uint32_t sgrid = std::min(cdiv(n, NTHR), 256u * 32u);
  RD_LAUNCH("fill.finalize", (k_finalize<T>), dim3(sgrid), dim3(NTHR), 0, s, d_z, fb.lab, fb.acc, n, fb.B);
}

// a shard's finish on compact labels: the nodes' levels from the (raised) basin levels, then the raster pass
template <class T>
static void fill_finalize16(T *d_z, int w, int h, const FillBuffers &fb, hipStream_t s);

// pit_mask<topo>(elevations, pit_mask) (reference depressions/Barnes2014.hpp:593-676; apps/rd_depressions_mask.cpp):
// the same flood, recording which cells it would raise instead of raising them.  1 = the cell lies strictly below the
// level it is reached at (W > z), 0 = not in a pit, 3 = NoData (every NoData cell, :668-669).
template <class T>
__global__ __launch_bounds__(NTHR) void k_pit_mask(const T *__restrict__ z, T nodata, const uint32_t *__restrict__ lab,
                                                   const uint32_t *__restrict__ acc, uint8_t *__restrict__ mask, uint32_t n,
                                                   uint32_t B, int trivial) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c64 = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c64 < n; c64 += stride) {
    const uint32_t c = (uint32_t)c64;
    const T e = z[c];
    uint8_t m = 0;
    if (e == nodata) m = 3;
    else if (!trivial) {
      const uint32_t b = lab[c];
      if (b != B && acc[b] > Key32<T>::to(e)) m = 1;
    }
    mask[c] = m;
  }
}

static void check_pit_mask_args(const void *z, int w, int h, int topology, const void *mask) {
  check_fill_args(z, w, h, topology);
  if (!mask) throw Error(RDGPU_ERR_ARG, "rdgpu_pit_mask: null mask pointer");
}

template <class T>
static void pit_mask_device(const T *d_z, T nodata, int w, int h, int topology, uint8_t *d_mask, hipStream_t s) {
  check_pit_mask_args(d_z, w, h, topology, d_mask);
  FillBuffers fb;
  BufAlloc ws_alloc{false, nullptr};
  if (topology == 8) fill_local_phase<T, 8>(d_z, w, h, 0, 0, ws_alloc, fb, s);
  else fill_local_phase<T, 4>(d_z, w, h, 0, 0, ws_alloc, fb, s);
  const uint32_t n = (uint32_t)((uint64_t)w * h);
  RD_LAUNCH("fill.pit_mask", (k_pit_mask<T>), dim3(std::min(cdiv(n, NTHR), 256u * 32u)), dim3(NTHR), 0, s, d_z, nodata,
            (const uint32_t *)fb.lab, (const uint32_t *)fb.acc, d_mask, n, fb.B, fb.trivial ? 1 : 0);
}

template <class T>
static void pit_mask_host(const T *dem, T nodata, int w, int h, int topology, uint8_t *mask) {
  check_pit_mask_args(dem, w, h, topology, mask);
  const size_t n = (size_t)w * h;
  HostStage st;
  const T *d = st.in("host.dem", dem, n);
  uint8_t *dm = st.out("host.dirs", mask, n);
  pit_mask_device<T>(d, nodata, w, h, topology, dm, nullptr);
  st.finish();
}

// ------------------------------------------------------------------------------------------
// PriorityFlood_Barnes2014_max_dep<topo>(elevations, max_dep_size) (reference depressions/Barnes2014.hpp:844-931;
// apps/rd_depressions_flood.cpp:16-19 with a non-zero third argument; goldens tests/depressions/testdem1.{1,2}.out,
// tests/tests.cpp:273-287): the same flood, but a depression is only raised when it has at most max_dep_size cells.
//
// What the reference counts as ONE depression is one run of its pit queue (:893-906): the cell c popped from the heap
// (level L = z(c)) floods every not yet visited cell BELOW L that it can reach through such cells (:918-921), and the
// run's cells are raised to L together, or not at all, when the next cell is popped from the heap.  In terms of the
// plain fill W: the run consists of raised cells (z < W = L); adjacent raised cells always have the same W, so the
// connected components of the raised cells ("pockets") are what can be flooded, each by the FIRST popped cell of
// elevation exactly L next to it, and a run = the pockets that share that cell.
//   * pockets: the raised cells of one basin of the descent forest are connected (every raised cell descends to the pit
//     through lower, hence raised, cells of its basin), so pockets are unions of basins -- a union-find over basins,
//     united wherever two raised cells of different basins touch (k_md_pockets; it also counts the raised cells per
//     basin, one atomic per run of equal labels in a wavefront row).
//   * spawner: the lowest cell index among the un-raised cells of elevation L next to the pocket (k_md_spawn).  When a
//     DEM has no two cells of equal elevation there is exactly one candidate; with ties the reference takes whichever
//     std::priority_queue pops first, which this rule cannot promise to reproduce.
//   * runs: every spawner unites the pockets it spawns (k_md_runs), sizes are summed per run, cells of runs with at
//     most max_dep_size cells are raised (k_md_apply).
// (The reference never applies the run started by the LAST cell popped from its heap, :891/:900 -- the loop ends first.
// On a DEM without equal elevations that cell, the highest un-raised one, cannot have started a run: a pocket has more
// than one rim cell and all of them would have to be the highest cell.)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_md_init(uint32_t *par, uint32_t *cnt, uint32_t *spawn, uint32_t *size, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  par[b] = b; cnt[b] = 0; spawn[b] = 0xFFFFFFFFu; size[b] = 0;
}

template <class T, int TOPO>
__global__ __launch_bounds__(NTHR) void k_md_pockets(const T *__restrict__ z, const uint32_t *__restrict__ lab,
                                                     const uint32_t *__restrict__ acc, uint32_t *par, uint32_t *cnt, int w,
                                                     int h, uint32_t B) {
  // one wavefront per 64-cell row segment (grid-stride over segments)
  const uint32_t segsX = ((uint32_t)w + 63u) / 64u;
  const uint64_t nseg = (uint64_t)segsX * (uint64_t)h;
  const int lane = threadIdx.x & 63;
  for (uint64_t sgi = (uint64_t)blockIdx.x * (NTHR / 64) + (threadIdx.x >> 6); sgi < nseg; sgi += (uint64_t)gridDim.x * (NTHR / 64)) {
    const int y = (int)(sgi / segsX), x = (int)(sgi % segsX) * 64 + lane;
    const bool in = x < w;
    const size_t c = (size_t)y * w + (in ? x : 0);
    const uint32_t b = in ? lab[c] : B;
    const bool raised = in && b != B && acc[b] > Key32<T>::to(z[c]);
    if (raised) {
      // forward neighbours: every adjacent pair of raised cells is looked at once
      const int nx[4] = {1, 1, 0, -1}, ny[4] = {0, 1, 1, 1};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (TOPO == 4 && (k == 1 || k == 3)) continue;
        const int xx = x + nx[k], yy = y + ny[k];
        if (xx < 0 || xx >= w || yy >= h) continue;
        const size_t q = (size_t)yy * w + xx;
        const uint32_t bq = lab[q];
        if (bq == b || bq == B) continue;
        if (acc[bq] > Key32<T>::to(z[q])) md_unite(par, b, bq);
      }
    }
    // raised cells per basin: one atomic per run of equal labels along the row segment
    const uint32_t key = raised ? b : 0xFFFFFFFFu;
    const uint32_t left = __shfl_up(key, 1, 64);
    const bool head = raised && (lane == 0 || left != key);
    const unsigned long long heads = __ballot(head), rs = __ballot(raised);
    if (head) {
      const unsigned long long above = lane < 63 ? (heads >> (lane + 1)) : 0ull;
      const int next = above ? lane + __ffsll((long long)above) : 64;   // next run head (of any label)
      // the run ends at the next head or at the first un-raised lane
      const unsigned long long notr = lane < 63 ? ((~rs) >> (lane + 1)) : 0ull;
      const int stop = notr ? lane + __ffsll((long long)notr) : 64;
      const int end = next < stop ? next : stop;
      atomicAdd(&cnt[b], (uint32_t)(end - lane));
    }
  }
}

__global__ __launch_bounds__(NTHR) void k_md_sizes(uint32_t *par, const uint32_t *__restrict__ cnt, uint32_t *size, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  const uint32_t c = cnt[b];
  if (c) atomicAdd(&size[md_find(par, b)], c);
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_md_apply(T *z, const uint32_t *__restrict__ lab, const uint32_t *__restrict__ acc,
                                                   uint32_t *par, const uint32_t *__restrict__ size, uint64_t n, uint32_t B,
                                                   uint64_t max_dep) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t b = lab[c];
    if (b == B) continue;
    const uint32_t L = acc[b];
    if (!(L > Key32<T>::to(z[c]))) continue;
    if ((uint64_t)size[md_find(par, b)] <= max_dep) z[c] = Key32<T>::from(L);
  }
}

// ---- tie detector (r05) -------------------------------------------------------------------------------------------------
// With equal elevations a pocket can have SEVERAL cells able to flood it (un-raised cells of elevation exactly L next to it);
// which of them the reference's std::priority_queue pops first decides which pockets end up in one run, hence whether the
// run passes the size limit.  Everything else about the result is order free.  So: ncand[pocket] = the number of distinct
// candidate cells; pockets that share ANY candidate cell are joined into a CLUSTER (par2, a coarser union-find than the
// runs, which only join through the chosen spawner); a cluster holding a pocket with two or more candidates is tie-flagged.
// Inside an unflagged cluster every pocket has exactly one possible flooding cell, so its runs -- and with them the output
// on all of the cluster's cells -- do not depend on the pop order.  Inside a flagged one the order matters only where the
// size limit can fall either way (k_md_tie_mask): S3, limit 100: 3420 of 4.18 million pockets have two candidates, most of
// them lakes far above the limit.  A difference from the reference on an unmasked cell would be a bug, not a tie
// (tests/test_s3_f2_gpu.py and tests/test_maxdep_gpu.py assert that there is none).
template <class T, int TOPO>
__global__ __launch_bounds__(NTHR) void k_md_ties(const T *__restrict__ z, const uint32_t *__restrict__ lab,
                                                  const uint32_t *__restrict__ acc, uint32_t *par, uint32_t *par2, uint32_t *ncand,
                                                  int w, int h, uint32_t B) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t b = lab[c];
    const uint32_t kz = Key32<T>::to(z[c]);
    if (b != B && acc[b] > kz) continue;   // raised cells are flooded, they do not flood
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    uint32_t seen[8];
    int ns = 0;
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
      const uint32_t r = md_find(par, bq);                  // its pocket
      bool dup = false;
      for (int i = 0; i < ns; i++) dup |= seen[i] == r;
      if (!dup) seen[ns++] = r;
    }
    for (int i = 0; i < ns; i++) {
      atomicAdd(&ncand[seen[i]], 1u);
      if (i) md_unite(par2, seen[0], seen[i]);
    }
  }
}
// pockets (roots of par with a candidate), tie pockets (two or more candidates); flags the clusters of the latter
__global__ __launch_bounds__(NTHR) void k_md_flag(uint32_t *par, uint32_t *par2, const uint32_t *__restrict__ ncand, uint32_t *flag,
                                                  unsigned long long *counts, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  const uint32_t nc = b < B ? ncand[b] : 0u;   // (only pocket roots were counted into)
  if (nc >= 2) flag[md_find(par2, b)] = 1u;
  const unsigned long long p1 = __ballot(nc >= 1), p2 = __ballot(nc >= 2);
  if ((threadIdx.x & 63) == 0) {
    if (p1) atomicAdd(&counts[0], (unsigned long long)__popcll(p1));
    if (p2) atomicAdd(&counts[1], (unsigned long long)__popcll(p2));
  }
}
// cells per pocket (sizeP, at the pocket's root in par) and per cluster (size2, at the cluster's root in par2)
__global__ __launch_bounds__(NTHR) void k_md_tie_sizes(uint32_t *par, uint32_t *par2, const uint32_t *__restrict__ cnt, uint32_t *sizeP,
                                                       uint32_t *size2, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  const uint32_t c = cnt[b];
  if (!c) return;
  atomicAdd(&sizeP[md_find(par, b)], c);
  atomicAdd(&size2[md_find(par2, b)], c);
}
// per cell: can the heap's order decide whether this cell is raised?  It lies in a pocket of a tie-flagged cluster, AND the
// size limit can fall either way: a pocket larger than the limit is never raised (any run holding it is larger still), a
// cluster that fits the limit as a whole is always raised (every run is part of it) -- whatever the order.  (mask optional;
// counts those cells and the pocket cells)
template <class T>
__global__ __launch_bounds__(NTHR) void k_md_tie_mask(const T *__restrict__ z, const uint32_t *__restrict__ lab,
                                                      const uint32_t *__restrict__ acc, uint32_t *par, uint32_t *par2,
                                                      const uint32_t *__restrict__ flag, const uint32_t *__restrict__ sizeP,
                                                      const uint32_t *__restrict__ size2, uint64_t max_dep,
                                                      uint8_t *mask, unsigned long long *counts, uint64_t n, uint32_t B) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  unsigned long long nt = 0, np = 0;
  for (uint64_t c0 = (uint64_t)blockIdx.x * NTHR; c0 < n; c0 += stride) {
    const uint64_t c = c0 + threadIdx.x;
    bool pocket = false, tie = false;
    if (c < n) {
      const uint32_t b = lab[c];
      pocket = b != B && acc[b] > Key32<T>::to(z[c]);
      if (pocket) {
        const uint32_t c2 = md_find(par2, b);
        tie = flag[c2] != 0 && (uint64_t)size2[c2] > max_dep && (uint64_t)sizeP[md_find(par, b)] <= max_dep;
      }
      if (mask) mask[c] = tie ? 1 : 0;
    }
    nt += (unsigned long long)__popcll(__ballot(tie));
    np += (unsigned long long)__popcll(__ballot(pocket));
  }
  if ((threadIdx.x & 63) == 0) {
    if (nt) atomicAdd(&counts[2], nt);
    if (np) atomicAdd(&counts[3], np);
  }
}
static thread_local rdgpu_max_dep_stats g_md_stats;
static thread_local unsigned long long *g_md_pinned = nullptr;   // the tie detector's counts of the last call, once its stream got there
static thread_local bool g_md_pending = false;
static thread_local hipStream_t g_md_stream = nullptr;

template <class T, int TOPO>
static void fill_max_dep_device_t(T *d_z, int w, int h, uint64_t max_dep, hipStream_t s, uint8_t *d_tie_mask = nullptr) {
  g_md_stats = rdgpu_max_dep_stats{0, 0, 0, 0};
  g_md_pending = false;
  if (d_tie_mask) RD_HIP(hipMemsetAsync(d_tie_mask, 0, (size_t)w * h, s));
  FillBuffers fb;
  BufAlloc ws_alloc{false, nullptr};
  fill_local_phase<T, TOPO>(d_z, w, h, 0, 0, ws_alloc, fb, s);
  if (fb.trivial) return;
  const uint64_t n = (uint64_t)w * h;
  const uint32_t B = fb.B;
  Workspace &ws = Workspace::get();
  uint32_t *par = ws.buf<uint32_t>("maxdep.par", B), *cnt = ws.buf<uint32_t>("maxdep.cnt", B);
  uint32_t *spawn = ws.buf<uint32_t>("maxdep.spawn", B), *size = ws.buf<uint32_t>("maxdep.size", B);
  const uint32_t bgrid = cdiv(B, NTHR), sgrid = (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u);
  RD_LAUNCH("maxdep.init", k_md_init, dim3(bgrid), dim3(NTHR), 0, s, par, cnt, spawn, size, B);
  RD_LAUNCH("maxdep.pockets", (k_md_pockets<T, TOPO>), dim3(256u * 16u), dim3(NTHR), 0, s, (const T *)d_z, (const uint32_t *)fb.lab,
            (const uint32_t *)fb.acc, par, cnt, w, h, B);
  {   // the tie detector: before the runs join pockets in `par`
    uint32_t *par2 = ws.buf<uint32_t>("maxdep.par2", B), *ncand = ws.buf<uint32_t>("maxdep.ncand", B), *flag = ws.buf<uint32_t>("maxdep.flag", B);
    unsigned long long *counts = ws.buf<unsigned long long>("maxdep.counts", 4);
    RD_HIP(hipMemcpyAsync(par2, par, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    RD_HIP(hipMemsetAsync(ncand, 0, (size_t)B * sizeof(uint32_t), s));
    RD_HIP(hipMemsetAsync(flag, 0, (size_t)B * sizeof(uint32_t), s));
    RD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), s));
    RD_LAUNCH("maxdep.ties", (k_md_ties<T, TOPO>), dim3(sgrid), dim3(NTHR), 0, s, (const T *)d_z, (const uint32_t *)fb.lab,
              (const uint32_t *)fb.acc, par, par2, ncand, w, h, B);
    RD_LAUNCH("maxdep.flag", k_md_flag, dim3(bgrid), dim3(NTHR), 0, s, par, par2, (const uint32_t *)ncand, flag, counts, B);
    uint32_t *sizeP = ws.buf<uint32_t>("maxdep.sizeP", B), *size2 = ws.buf<uint32_t>("maxdep.size2", B);
    RD_HIP(hipMemsetAsync(sizeP, 0, (size_t)B * sizeof(uint32_t), s));
    RD_HIP(hipMemsetAsync(size2, 0, (size_t)B * sizeof(uint32_t), s));
    RD_LAUNCH("maxdep.tie_sizes", k_md_tie_sizes, dim3(bgrid), dim3(NTHR), 0, s, par, par2, (const uint32_t *)cnt, sizeP, size2, B);
    RD_LAUNCH("maxdep.tie_mask", (k_md_tie_mask<T>), dim3(sgrid), dim3(NTHR), 0, s, (const T *)d_z, (const uint32_t *)fb.lab,
              (const uint32_t *)fb.acc, par, par2, (const uint32_t *)flag, (const uint32_t *)sizeP, (const uint32_t *)size2, max_dep,
              d_tie_mask, counts, n, B);
    // the counts come back LAZILY (the stream-ordered `_dev_` entry must not block the host): copied into a pinned
    // word block behind the kernels, read by rdgpu_fill_max_dep_get_stats after it has waited for this stream
    if (!g_md_pinned) RD_HIP(hipHostMalloc((void **)&g_md_pinned, 4 * sizeof(unsigned long long)));
    RD_HIP(hipMemcpyAsync(g_md_pinned, counts, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    g_md_pending = true;
    g_md_stream = s;
  }
  RD_LAUNCH("maxdep.spawn", (k_md_spawn<T, TOPO, 0>), dim3(sgrid), dim3(NTHR), 0, s, (const T *)d_z, (const uint32_t *)fb.lab,
            (const uint32_t *)fb.acc, par, spawn, w, h, B);
  RD_LAUNCH("maxdep.runs", (k_md_spawn<T, TOPO, 1>), dim3(sgrid), dim3(NTHR), 0, s, (const T *)d_z, (const uint32_t *)fb.lab,
            (const uint32_t *)fb.acc, par, spawn, w, h, B);
  RD_LAUNCH("maxdep.sizes", k_md_sizes, dim3(bgrid), dim3(NTHR), 0, s, par, (const uint32_t *)cnt, size, B);
  RD_LAUNCH("maxdep.apply", (k_md_apply<T>), dim3(sgrid), dim3(NTHR), 0, s, d_z, (const uint32_t *)fb.lab, (const uint32_t *)fb.acc,
            par, (const uint32_t *)size, n, B, max_dep);
}

template <class T>
static void fill_max_dep_device(T *d_z, int w, int h, int topology, uint64_t max_dep, hipStream_t s, uint8_t *d_tie_mask = nullptr) {
  check_fill_args(d_z, w, h, topology);
  if (topology == 8) fill_max_dep_device_t<T, 8>(d_z, w, h, max_dep, s, d_tie_mask);
  else fill_max_dep_device_t<T, 4>(d_z, w, h, max_dep, s, d_tie_mask);
}

template <class T>
static void fill_max_dep_host(T *dem, int w, int h, int topology, uint64_t max_dep) {
  check_fill_args(dem, w, h, topology);
  HostStage st;
  T *d = st.inout("host.dem", dem, (size_t)w * h);
  fill_max_dep_device<T>(d, w, h, topology, max_dep, nullptr);
  st.finish();
}

// ==========================================================================================================
// The compact-label fill (r03): 16-bit labels, no label pass over the raster.
//
// The classic path above reads the raster four times (descent, labels, pair pass, finalize: 4.8 x the algorithmic bytes
// at S3) and moves a 32-bit label per cell through three of them.  Here
//   k_descent16      descent pointers and in-tile path compression as k_descent; then every ROOT of the tile -- a pit, a
//                    cell draining off the raster, a cell whose descent neighbour lies outside the tile -- becomes a
//                    NODE: local slot 0.., global id tile_base + slot, G[node] = basin id | PEND | first cell outside
//                    the tile | OUTP.  A cell's label is the SLOT of its root: 2 bytes per cell (lab16).
//   k_resolve_nodes  node -> basin (curN): a pending node follows the tiles' edge records / G from tile to tile.  A table
//                    pass over ~2 % of the cell count replaces k_tile_label's raster pass (10.7 GB at S3).
//   k_pairs16        the one pair pass, reading z + lab16 (6 B / cell) and taking the components from curN.
//   rounds           unchanged (pair list).
//   k_finalize16     z <- max(z, level of the cell's node): z + lab16 and the tile's node levels from LDS, formed from curN
//                    and the basins' levels as they are staged (the shards keep a table of them: k_node_levels).
// (Tried first and dropped: the pairs in the descent kernel itself, on slots, with the pairs across tile edges from edge
// strips -- correct, but slot boundaries are several times as many as basin boundaries, since every exit of a tile is a
// slot of its own until it is resolved: 22 ms for the kernel, 80 M records; profiles/r03h_fill_fused_ab.json.)
// Anything the scheme cannot hold (more nodes or records than the buffers) raises a flag and the classic path runs.
// Row-block shards, pit_mask, max_dep and the watershed code keep the classic path (they consume 32-bit labels).
// ==========================================================================================================
// Node and pit ids are handed out per tile with ONE returning atomic -- and same-address device atomics serialise at
// ~12 ns each: 390 625 tiles on one counter are 4.5 ms of the kernel whatever else it does (r04).  So there are up to 32
// STRIPES (tile t uses stripe t & smask), each with its own counter word on its own 128-byte line, its own region of the
// node table (rcap nodes) and its own run of pit numbers; k_stripe_offsets turns the pit numbers into dense basin ids
// afterwards (pitoff[]), which k_resolve_nodes adds when it writes a node's component.
constexpr int FSTRIPES = 32, FSTRIDE = 16;   // counter words are FSTRIDE * 8 bytes apart
struct FusedBuf {
  uint16_t *lab16;                 // [cells] slot of the cell's root within its descent tile
  uint32_t *G;                     // [gcap] node table: stripe s owns [s * rcap, (s + 1) * rcap)
  uint32_t *tile_base, *tile_count;   // [descent tiles]
  unsigned long long *counters;    // [stripe * FSTRIDE] (nodes << 32) | pits of the stripe; [stripe * FSTRIDE + 1] its dissolved pits
  uint32_t gcap, rcap, smask;
  uint32_t *overflow;
  // the first and last column of every descent tile as compact records (key, slot), [tile][side][row]: the pair pass takes
  // its tiles' ring columns from these -- read from the raster a ring column costs a 64-byte sector per row and array
  // for one cell (12.5 GB per pass at S3 once the neighbouring tile's rows are no longer in L2; r04a counters)
  uint32_t *edgeK = nullptr;
  uint16_t *edgeS = nullptr;
  // the first and last ROW of every descent tile, slots only, [tile][top / bottom][column].  With the columns' slots these
  // are every label the node chase can ask for (k_resolve_nodes: a pending node names a cell on the outer ring of a
  // neighbouring tile): two 128-byte lines per tile side instead of one sector of the 2-byte raster per hop
  uint16_t *edgeR = nullptr;
};

// after the descent: dense basin ids.  out[0] = basins, out[1] = nodes in use, out[2] = the fullest stripe's node count,
// out[3] = dissolved pits (no basins: not in out[0])
__global__ __launch_bounds__(64) void k_stripe_offsets(const unsigned long long *__restrict__ counters, uint32_t nstripes,
                                                       uint32_t *pitoff, uint32_t *out, uint32_t *forest_max) {
  const uint32_t s = threadIdx.x;
  const unsigned long long c = s < nstripes ? counters[s * FSTRIDE] : 0ull;
  const uint32_t pits = (uint32_t)c, nodes = (uint32_t)(c >> 32);
  uint32_t incl = pits, tot = nodes, mx = nodes;
  uint32_t dis = s < nstripes ? (uint32_t)counters[s * FSTRIDE + 1] : 0u;   // the stripe's dissolved pits (k_descent16)
  uint32_t mxd = nodes + dis;   // the stripe's nodes had no pit dissolved: what the node table is asked to hold (fill_fused)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if ((int)s >= o) incl += v;
    tot += __shfl_xor(tot, o, 64);
    mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
    dis += __shfl_xor(dis, o, 64);
    mxd = max(mxd, (uint32_t)__shfl_xor(mxd, o, 64));
  }
  if (s < nstripes) pitoff[s] = incl - pits;
  if (s == 63) { out[0] = incl; out[1] = tot; out[2] = mx; out[3] = dis; *forest_max = mxd; }
}

// maximum / minimum over the 64 lanes, in every lane: a DPP prefix scan (row shifts, then row broadcasts) whose last lane
// holds the result -- six VALU instructions and a v_readlane
// Edge of the blocks of the coarse flood: k_descent16 leaves the blocks' minima, their fill is a lower bound
// of the filled surface (rdgpu_fill_coarse_block).
constexpr int COARSE_CB = 16;
// the minimum over each row of 16 lanes, in the row's last lane (the other lanes hold the minimum of the lanes up to them)
__device__ __forceinline__ uint32_t row_min_u32(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1 (all ones: the identity)
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1 (0: the identity)
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return ~wave_max_u32(~v); }

// OUTLETS: cells flagged in `outlet` drain like the raster's border cells (interior outlets: the restricted fills of
// pfdirs.hip); the instantiation of the plain fill does not look at the pointer.
// There, all outlets of a tile share ONE node (slot 0: a tile of walls has thousands of them), node 0 of the table is a
// global "outside" node, and `skip` (optional, per descent tile) names the tiles that hold nothing but outlets, ring
// included: they get no work -- label 0 everywhere (written once: skip == 1; 2: written before), node 0.
// CUT: the raster is a row-block shard -- the cells of an open first / last row are frozen terminals (own roots, numbered
// like pits, never draining), not border cells.
template <class T, int TOPO, bool VEC, bool OUTLETS = false, bool CUT = false, bool COARSE = false>
__global__ __launch_bounds__(NTHR) void k_descent16(const T *__restrict__ z, FusedBuf fo, int w, int h,
                                                    uint32_t tilesX, uint32_t ntiles, const uint8_t *__restrict__ outlet = nullptr,
                                                    const uint8_t *__restrict__ skip = nullptr,
                                                    const uint32_t *__restrict__ tlist = nullptr, int open_top = 0,
                                                    int open_bottom = 0, int dissolve = 0,
                                                    uint32_t *__restrict__ tile_max = nullptr,
                                                    uint32_t *__restrict__ coarse = nullptr, uint32_t cbx = 0, uint32_t cby = 0) {
  // tlist (optional, with OUTLETS): the tiles to work on, one block each (ntiles = the raster's tiles all the same)
  // dissolve (block-uniform; the plain fill only): a pit whose lowest neighbour q lies in the tile and does not drain
  // into it is no basin of its own -- it points at q, and its label carries q's direction for the finalize
  // tile_max (optional; the plain fill only): tile_max[t] = the largest key among the tile's cells, for the finalize's
  // flooded-tile test (k_finalize16).  0xFFFFFFFF for a tile that is not interior: it holds a border cell, which is never
  // raised, or cells outside the raster -- such a tile never passes the test.
  // coarse (with COARSE; the plain fill only -- without it the kernel is the one it was): the cby x cbx raster of the minima of the CB x CB blocks anchored at (0, 0), as
  // keys, over the blocks' cells inside the raster.  Every tile writes its blocks, the tiles on the raster's rim included: a
  // wavefront owns CB rows and a DPP row is CB lanes, so a block is one row of lanes of one wavefront.
  constexpr bool DIS_OK = !OUTLETS && !CUT;
  const bool dis = DIS_OK && dissolve != 0;
  __shared__ uint32_t dcnt;
  __shared__ uint32_t wkmax[NTHR / 64];
  __shared__ uint32_t sk[DLH * DLW];
  // rows of LPD = 66 entries: with 64 two-byte entries every row starts on the same LDS bank and the jumps' gathers --
  // neighbouring columns of different rows -- collide (29 % of the kernel's LDS cycles, r03e)
  constexpr int LPD = DW + 2;
  __shared__ uint16_t lp[DH * LPD];
  __shared__ uint32_t wtot[NTHR / 64];
  __shared__ uint32_t pbase, rbase, fits_s;
  const uint32_t t = (OUTLETS && tlist) ? tlist[blockIdx.x] : xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * DW, y0 = (int)(t / tilesX) * DH;
  if (OUTLETS && skip && skip[t]) {
    if (threadIdx.x == 0) { fo.tile_base[t] = 0; fo.tile_count[t] = 1; }
    if (skip[t] == 1) {
      const int lx_ = threadIdx.x & (DW - 1), gx_ = x0 + lx_;
      for (int ly_ = threadIdx.x >> 6; ly_ < DH; ly_ += NTHR / 64)
        if (gx_ < w && y0 + ly_ < h) fo.lab16[(size_t)(y0 + ly_) * w + gx_] = 0;
    }
    return;
  }
  // (block-uniform) an INTERIOR tile: the tile and its halo lie in the raster and the tile holds no cell of the raster's
  // first or last row or column.  Its cells need no bounds, border or cut-row tests anywhere below (at 40000^2 that is
  // 99.7 % of the tiles).  The fills with outlets read outlet[] per cell and keep the general body.
  const bool inner = !OUTLETS && x0 >= 1 && y0 >= 1 && x0 + DW <= w - 1 && y0 + DH <= h - 1;
  {
    constexpr int NQ = DLH * (DW / 4), QPT = (NQ + NTHR - 1) / NTHR;
    Quad<T> zq[QPT];
    if (y0 >= 1 && y0 + DH < h && x0 + DW <= w) {   // (block-uniform) every row and quad of the window lies in the raster: no tests
#pragma unroll
      for (int r = 0; r < QPT; r++) {
        const int i = threadIdx.x + r * NTHR;
        const int ly = i / (DW / 4), q = i - ly * (DW / 4);
        if (i < NQ) zq[r] = load_quad<T, VEC>(z + (size_t)(y0 - 1 + ly) * w, x0 + 4 * q, w, T());
      }
      // (every load is out before the first key is formed: the float key's add moves up to its load otherwise, and with
      // it a wait for that load alone -- the five loads then go one after the other, +0.14 ms per launch at 40000^2)
#pragma unroll
      for (int r = 0; r < QPT; r++) keys_after_loads(zq[r]);
#pragma unroll
      for (int r = 0; r < QPT; r++) {
        const int i = threadIdx.x + r * NTHR;
        if (i >= NQ) continue;
        const int ly = i / (DW / 4), q = i - ly * (DW / 4);
        const int o = ly * DLW + 1 + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; e++) sk[o + e] = key32_fast<T>(zq[r].v[e]);
      }
    } else {
      bool okq[QPT];
#pragma unroll
      for (int r = 0; r < QPT; r++) {
        const int i = threadIdx.x + r * NTHR;
        const int ly = i / (DW / 4), q = i - ly * (DW / 4);
        const int gx = x0 + 4 * q, gy = y0 - 1 + ly;
        okq[r] = i < NQ && gy >= 0 && gy < h && gx < w;
        if (okq[r]) zq[r] = load_quad<T, VEC>(z + (size_t)gy * w, gx, w, T());
      }
#pragma unroll
      for (int r = 0; r < QPT; r++) keys_after_loads(zq[r]);
#pragma unroll
      for (int r = 0; r < QPT; r++) {
        const int i = threadIdx.x + r * NTHR;
        if (i >= NQ) continue;
        const int ly = i / (DW / 4), q = i - ly * (DW / 4);
        const int o = ly * DLW + 1 + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; e++) sk[o + e] = (okq[r] && x0 + 4 * q + e < w) ? key32_fast<T>(zq[r].v[e]) : 0xFFFFFFFFu;
      }
    }
    for (int i = threadIdx.x; i < 2 * DLH; i += NTHR) {   // halo columns
      const int ly = i >> 1, lxh = (i & 1) ? DLW - 1 : 0;
      const int gx = x0 - 1 + lxh, gy = y0 - 1 + ly;
      uint32_t kk = 0xFFFFFFFFu;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) kk = key32_fast<T>(z[(size_t)gy * w + gx]);
      sk[ly * DLW + lxh] = kk;
    }
    if (DIS_OK && threadIdx.x == 0) dcnt = 0;
  }
  __syncthreads();
  // (the wavefront's index as a SCALAR: everything derived from the row -- bounds tests, LDS row offsets -- then runs on the
  // scalar unit; this kernel is bound by VALU issue, 4 cycles per wave instruction)
  //
  // r04d: the kernel's VALU work per row of 64 cells went 143 -> ~70 instructions by three changes.
  //  * The 8-neighbour minimum WITH its position from row triples: min3 + "first of (a, b, c) equal to it" once per row,
  //    used by the cell above and the cell below; the winner carries one packed word (pointer delta | exit code | which
  //    column / row it lies in), so nothing is decoded afterwards.
  //  * Roots point to THEMSELVES in lp and pointers are byte offsets: a jump is lp[lp[p]] with no compare or select, a
  //    cell is finished when the two reads agree, and the wavefronts iterate on their own rows without barriers (every
  //    value a racing read can see is an ancestor on the cell's path).  The exit codes stay in registers.
  //  * Slots go to a 16-bit array laid over the keys (dead by then) at the SAME offsets as lp: label = slot16[p].
  const int wave_s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lx = threadIdx.x & (DW - 1), ly0 = wave_s * (DH / 4);
  const int gx = x0 + lx;
  constexpr int RPT = DH / 4;                      // rows per thread
  static_assert(RPT == 16, "four code words of four bytes, 16-bit row masks");
  uint16_t *const slot16 = reinterpret_cast<uint16_t *>(sk);   // valid once the keys are dead (after the edge keys are out)
  const uint32_t selfb0 = (uint32_t)((ly0 * LPD + lx) * 2);
  uint32_t p[RPT];                                 // the cell's pointer: byte offset into lp
  // four bits per row, rows 0..7 and 8..15: 1..8 the lowest neighbour (an exit's target, a pit's q), 9 drains off the raster.
  // (Two words and one select to read a row's: with four words of a byte per row the select chain became an indexed load
  // from a copy of the words in scratch memory.)
  uint32_t codesLo = 0, codesHi = 0;
  uint32_t rootmask = 0, pitmask = 0, outmask = 0;
  uint32_t kmax = 0;   // the largest key of the thread's cells (interior tiles with tile_max: the keys are live only here)
  uint32_t kmin = 0xFFFFFFFFu;   // the smallest (a cell outside the raster holds 0xFFFFFFFF in sk)
  {
    // packed word of a candidate: [15:0] byte delta + 134, [19:16] exit code, [26:24] column 0 / 1 / 2, [27] row above, [29] row below
    constexpr uint32_t WT0 = 0u | (1u << 16) | (1u << 24) | (1u << 27), WT1 = 2u | (2u << 16) | (1u << 25) | (1u << 27),
                       WT2 = 4u | (3u << 16) | (1u << 26) | (1u << 27);
    constexpr uint32_t WM0 = (uint32_t)(2 * LPD) | (4u << 16) | (1u << 24), WM2 = (uint32_t)(2 * LPD + 4) | (5u << 16) | (1u << 26);
    constexpr uint32_t BADD = (uint32_t)(4 * LPD) + (5u << 16) + ((1u << 29) - (1u << 27));
    const bool colin = gx < w, colborder = (gx == 0) | (gx == w - 1);
    const uint32_t cmcol = lx == 0 ? (1u << 24) : lx == DW - 1 ? (1u << 26) : 0u;
    uint32_t ta, tb, tc, tm, tW, ma, mb, mc, mm3, mW;   // the triples of the row above and of the cell's row
    auto triple = [&](int r, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &m, uint32_t &W) {
      a = sk[r * DLW + lx];
      b = sk[r * DLW + lx + 1];
      c = sk[r * DLW + lx + 2];
      if (TOPO == 8) {
        m = min(min(a, b), c);
        W = a == m ? WT0 : b == m ? WT1 : WT2;
      } else {
        m = b;
        W = WT1;
      }
    };
    triple(ly0, ta, tb, tc, tm, tW);
    triple(ly0 + 1, ma, mb, mc, mm3, mW);
    // INNER: an interior tile (above) -- every cell lies in the raster and none on its border or on a cut row, so the
    // sixteen rows' lane masks for those tests (scalar-unit work, a quarter of the kernel's scalar instructions) are not
    // formed at all
    auto classify = [&](auto INNER) {
#pragma unroll
    for (int j = 0; j < RPT; j++) {
      const int ly = ly0 + j, gy = y0 + ly;   // (scalar)
      uint32_t ba, bb, bc, bm, bW;
      triple(ly + 2, ba, bb, bc, bm, bW);
      const uint32_t kc = mb;
      if (DIS_OK && INNER) kmax = max(kmax, kc);
      if (DIS_OK && COARSE) kmin = min(kmin, kc);
      const bool midfirst = ma <= mc;
      const uint32_t mm = midfirst ? ma : mc;
      const uint32_t bk = min(min(tm, mm), bm);
      const bool isT = tm == bk, isM = mm == bk;
      const uint32_t wM = midfirst ? WM0 : WM2, wB = bW + BADD, wMB = isM ? wM : wB;
      const uint32_t W = isT ? tW : wMB;
      const bool drains = (bk < kc) | ((bk == kc) & (isT | (isM & midfirst)));
      uint32_t cm = cmcol;
      if (j == 0 && ly0 == 0) cm |= 1u << 27;                   // (only a wavefront's first / last row can be the tile's)
      if (j == RPT - 1 && ly0 == DH - RPT) cm |= 1u << 29;
      const bool outside = (W & cm) != 0u;
      const uint32_t self = selfb0 + (uint32_t)(j * LPD * 2);
      const bool incell = INNER || (colin & (gy < h));
      bool border = !INNER && (colborder | (gy == 0) | (gy == h - 1));
      bool stays = !drains;
      if (CUT && !INNER) {
        const bool cutrow = ((gy == 0) & (open_top != 0)) | ((gy == h - 1) & (open_bottom != 0));
        border = colborder | ((gy == 0) & !open_top) | ((gy == h - 1) & !open_bottom);
        stays |= cutrow;
      }
      if (OUTLETS) border |= incell && outlet[(size_t)gy * w + gx] != 0;
      const bool selfp = !incell | border | stays | outside;
      const uint32_t rel = selfp ? (uint32_t)(2 * LPD + 2) : (W & 0xFFFFu);   // (the delta's bias: the cell itself)
      p[j] = rel + (self - (uint32_t)(2 * LPD + 2));
      *reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(lp) + self) = (uint16_t)p[j];
      const uint32_t cexit = (W >> 16) & 15u;   // (a pit keeps the code of its lowest neighbour: pitmask tells it from an exit)
      const uint32_t code = border ? 9u : cexit;
      if (j < 8) codesLo |= code << (4 * (j & 7));
      else codesHi |= code << (4 * (j & 7));
      bool root = incell & selfp;
      if (OUTLETS) {   // the tile's outlets share slot 0
        const bool outroot = root & border;
        outmask |= (outroot ? 1u : 0u) << j;
        root &= !outroot;
      }
      rootmask |= (root ? 1u : 0u) << j;
      pitmask |= ((root & !border & stays) ? 1u : 0u) << j;
      ta = ma; tb = mb; tc = mc; tm = mm3; tW = mW;
      ma = ba; mb = bb; mc = bc; mm3 = bm; mW = bW;
    }
    };
    if (inner) classify(std::true_type());
    else classify(std::false_type());
    (void)ta; (void)tb; (void)tc;
  }
  // (the masks and codes are formed HERE, in vector registers: left to the compiler they sink below the jump loop, which
  // keeps sixteen rows of lane masks alive in scalar registers and spills them lane by lane)
  asm volatile("" : "+v"(rootmask), "+v"(pitmask), "+v"(outmask), "+v"(codesLo), "+v"(codesHi));
  // the tile's first and last column: the KEYS of the compact records for the pair pass (before the keys' array is reused)
  if (fo.edgeK && threadIdx.x < 2 * DH) {
    const int side = threadIdx.x >> 6, lye = threadIdx.x & (DH - 1), lxe = side ? DW - 1 : 0;
    fo.edgeK[((size_t)t * 2 + side) * DH + lye] = sk[(lye + 1) * DLW + lxe + 1];
  }
  if (DIS_OK && tile_max) {   // (block-uniform) one reduction per wavefront; thread 0 stores the tile's word with its bases
    const uint32_t wm = wave_max_u32(kmax);
    if ((threadIdx.x & 63) == 0) wkmax[wave_s] = wm;
  }
  if (DIS_OK && COARSE) {   // the wavefront's four block minima: lane 15 of each row of lanes holds its row's
    static_assert(COARSE_CB == RPT && COARSE_CB == 16 && DW % COARSE_CB == 0, "a block is a wavefront's rows by a DPP row's lanes");
    const uint32_t bm = row_min_u32(kmin);
    const uint32_t bx = (uint32_t)gx / COARSE_CB, by = (uint32_t)(y0 + ly0) / COARSE_CB;
    if ((lx & (COARSE_CB - 1)) == COARSE_CB - 1 && bx < cbx && by < cby) coarse[(size_t)by * cbx + bx] = bm;
  }
  __syncthreads();
  auto code_of = [codesLo, codesHi](int j) -> int {   // row j's code (j varies per lane)
    return (int)((j < 8 ? codesLo : codesHi) >> (4 * (j & 7)) & 15u);
  };
  // ---- pits that are no depressions.  q, the lowest neighbour of pit p, does not drain into p: then q is not
  // in p's basin, the lowest pass out of that basin is key(q) and only p lies below it.  p points at q -- its catchment
  // joins q's tree, p is no root and no basin -- and the finalize raises p alone to max(key(q), level).  lp[q] is q's
  // pointer as classify stored it (q is never such a pit itself: p is a lower neighbour of q), the jumps start after the
  // second barrier: a cell of another wavefront that read the old lp[p] == p twice would take p for its root.
  uint32_t dissmask = 0;
  if (dis) {
    for (uint32_t m = pitmask; m; m &= m - 1) {
      const int j = __ffs((int)m) - 1;
      const int code = code_of(j);   // 1..8: a pit is no border cell
      const int n = code <= 4 ? code - 1 : code, nr = n >= 6 ? 2 : n >= 3 ? 1 : 0, nc = n - 3 * nr;
      const int qx = lx + nc - 1, qy = ly0 + j + nr - 1;
      if ((unsigned)qx >= (unsigned)DW || (unsigned)qy >= (unsigned)DH) continue;   // q lies in the next tile: p stays a pit
      const uint32_t self = selfb0 + (uint32_t)(j * LPD * 2), qb = (uint32_t)((qy * LPD + qx) * 2);
      if ((uint32_t)*reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(lp) + qb) == self) continue;   // q drains into p
      *reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(lp) + self) = (uint16_t)qb;   // (p[j] stays: the first jump reads lp[self])
      dissmask |= 1u << j;
    }
    rootmask &= ~dissmask;
    pitmask &= ~dissmask;
    if (dissmask) atomicAdd(&dcnt, (uint32_t)__popc(dissmask));
    __syncthreads();
  }
  {   // pointer jumping inside the tile: every wavefront on its own rows until they all point to roots; no barriers
    const char *const lpb = reinterpret_cast<const char *>(lp);
    uint32_t gact = (1u << (RPT / 4)) - 1u;   // (scalar) groups of four rows with a pointer that may still move
    // the first passes move pointers in nearly every group of every tile: they run without the ballots, compares and
    // branches of the convergence test (a root points to itself, so a pass too many changes nothing)
    constexpr int BLIND = 2;
    for (int it = 0; it < BLIND; it++) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int g = 0; g < RPT / 4; g++) {
        uint32_t qv[4], rv[4];
#pragma unroll
        for (int e = 0; e < 4; e++) { qv[e] = *reinterpret_cast<const uint16_t *>(lpb + p[4 * g + e]); asm("" : "+v"(qv[e])); }
#pragma unroll
        for (int e = 0; e < 4; e++) { rv[e] = *reinterpret_cast<const uint16_t *>(lpb + qv[e]); asm("" : "+v"(rv[e])); }
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int j = 4 * g + e;
          p[j] = rv[e];
          *reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(lp) + selfb0 + (uint32_t)(j * LPD * 2)) = (uint16_t)rv[e];
        }
      }
    }
    for (int it = 0; gact != 0u && it < DW * DH; it++) {
      asm volatile("" ::: "memory");   // (other wavefronts write lp meanwhile: nothing read from it is kept across passes)
#pragma unroll
      for (int g = 0; g < RPT / 4; g++) {
        if (!(gact >> g & 1u)) continue;
        uint32_t qv[4], rv[4];
#pragma unroll
        for (int e = 0; e < 4; e++) { qv[e] = *reinterpret_cast<const uint16_t *>(lpb + p[4 * g + e]); asm("" : "+v"(qv[e])); }
#pragma unroll
        for (int e = 0; e < 4; e++) { rv[e] = *reinterpret_cast<const uint16_t *>(lpb + qv[e]); asm("" : "+v"(rv[e])); }   // (opaque 32-bit values: else the compare is narrowed to 16 bits and every value is masked again for its use as an address)
        unsigned long long moving = 0;   // (ballots of the plain compares: lane masks straight from v_cmp, OR-ed on the scalar unit)
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int j = 4 * g + e;
          moving |= __builtin_amdgcn_ballot_w64(rv[e] != qv[e]);   // (equal: qv is a root, the cell is finished)
          p[j] = rv[e];
          *reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(lp) + selfb0 + (uint32_t)(j * LPD * 2)) = (uint16_t)rv[e];
        }
        if (moving == 0ull) gact &= ~(1u << g);
      }
    }
  }
  // ---- nodes: every root of the tile gets a local slot; pits a dense basin id --------------------------------------
  const uint32_t mine = ((uint32_t)__popc(rootmask) << 16) | (uint32_t)__popc(pitmask);   // (<= 1024 each per wavefront)
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if ((threadIdx.x & 63) >= o) incl += v;
  }
  if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
  __syncthreads();   // (also: every wavefront's pointers are final, the keys are dead)
  if (threadIdx.x == 0) {
    const uint32_t nr = (wtot[0] >> 16) + (wtot[1] >> 16) + (wtot[2] >> 16) + (wtot[3] >> 16) + (OUTLETS ? 1u : 0u);
    const uint32_t np = (wtot[0] & 0xFFFFu) + (wtot[1] & 0xFFFFu) + (wtot[2] & 0xFFFFu) + (wtot[3] & 0xFFFFu);
    const uint32_t st = t & fo.smask;   // the tile's stripe: its own counter, node region and run of pit numbers
    const unsigned long long old = atomicAdd(&fo.counters[st * FSTRIDE], ((unsigned long long)nr << 32) | np);
    const uint32_t rl = (uint32_t)(old >> 32);
    pbase = (uint32_t)old;
    rbase = st * fo.rcap + rl;
    fo.tile_base[t] = rbase;
    fo.tile_count[t] = nr;
    if (DIS_OK && tile_max) tile_max[t] = inner ? max(max(wkmax[0], wkmax[1]), max(wkmax[2], wkmax[3])) : 0xFFFFFFFFu;
    fits_s = (unsigned long long)rl + nr <= fo.rcap ? 1u : 0u;
    if (!fits_s) *fo.overflow = 1;
    // the dissolved pits of the stripe: the second word of the stripe's line (a statistic: nothing waits for it)
    if (DIS_OK && dis && dcnt != 0u) atomicAdd(&fo.counters[st * FSTRIDE + 1], (unsigned long long)dcnt);
  }
  {   // (the roots' slots do not depend on the counter: written beside thread 0's atomic)
    uint32_t pre = incl - mine;
    for (int k = 0; k < wave_s; k++) pre += wtot[k];
    uint32_t slot = (pre >> 16) + (OUTLETS ? 1u : 0u);
    if (OUTLETS)
      for (uint32_t m = outmask; m; m &= m - 1)
        *reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(slot16) + selfb0 + (uint32_t)((__ffs((int)m) - 1) * LPD * 2)) = 0;   // slot 0
    for (uint32_t m = rootmask; m; m &= m - 1) {
      const int j = __ffs((int)m) - 1;
      *reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(slot16) + selfb0 + (uint32_t)(j * LPD * 2)) = (uint16_t)slot;
      slot++;
    }
  }
  __syncthreads();
  const uint32_t nodes0 = rbase;
  if (fits_s != 0) {
    uint32_t pre = incl - mine;
    for (int k = 0; k < wave_s; k++) pre += wtot[k];
    uint32_t slot = (pre >> 16) + (OUTLETS ? 1u : 0u), pit = pbase + (pre & 0xFFFFu);
    if (OUTLETS && threadIdx.x == 0) fo.G[nodes0] = OUTP;
    for (uint32_t m = rootmask; m; m &= m - 1) {
      const int j = __ffs((int)m) - 1;
      const int ly = ly0 + j;
      const int code = code_of(j);
      const int n = code <= 4 ? code - 1 : code;   // 3x3 position of the root's descent neighbour (codes 1..8)
      const int nr = n >= 6 ? 2 : n >= 3 ? 1 : 0, nc = n - 3 * nr;
      const uint32_t pend = LAB_PEND | ((uint32_t)(y0 + ly + nr - 1) * (uint32_t)w + (uint32_t)(x0 + lx + nc - 1));
      const uint32_t word = (pitmask >> j & 1u) ? pit++ : code == 9 ? OUTP : pend;
      fo.G[nodes0 + slot] = word;
      slot++;
    }
  }
  // a cell's label: the slot of its root (its own when it is one)
  {
    const char *const sl = reinterpret_cast<const char *>(slot16);
    if (inner) {
#pragma unroll
      for (int j = 0; j < RPT; j++) {
        const int gy = y0 + ly0 + j;
        fo.lab16[(size_t)gy * w + gx] = *reinterpret_cast<const uint16_t *>(sl + p[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < RPT; j++) {
        const int gy = y0 + ly0 + j;
        const uint16_t rv = *reinterpret_cast<const uint16_t *>(sl + p[j]);
        if ((gx < w) & (gy < h)) fo.lab16[(size_t)gy * w + gx] = rv;   // (< 4096: not every cell of a tile can be a root)
      }
    }
    // a dissolved pit's label once more, with its flag and the position of q in the four bits a slot leaves free:
    // slot | (8 | code - 1) << 12.  (The thread that stored the plain label above: the two stores keep their order.  A
    // dissolved pit lies in the raster; lp[self] is p[j], the cell's root, since the jumps' first pass.)
    if (DIS_OK)
      for (uint32_t m = dissmask; m; m &= m - 1) {
        const int j = __ffs((int)m) - 1;
        const uint32_t root = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(lp) + selfb0 + (uint32_t)(j * LPD * 2));
        const uint32_t slot = *reinterpret_cast<const uint16_t *>(sl + root);
        fo.lab16[(size_t)(y0 + ly0 + j) * w + gx] = (uint16_t)(slot | ((8u | (uint32_t)(code_of(j) - 1)) << 12));
      }
    // the tile's first and last column, the SLOTS of the compact records: two wavefronts, one row per lane, coalesced.
    // A cell past the raster's end gets slot 0: the pair pass does read such a record (a ring cell outside the raster is
    // loaded from a clamped position and discarded afterwards), and follows its slot into the node table.
    if (fo.edgeS && threadIdx.x < 2 * DH) {
      const int side = threadIdx.x >> 6, lye = threadIdx.x & (DH - 1), lxe = side ? DW - 1 : 0;
      const uint16_t v = lp[lye * LPD + lxe];
      const bool in = inner || (x0 + lxe < w && y0 + lye < h);
      fo.edgeS[((size_t)t * 2 + side) * DH + lye] = in ? *reinterpret_cast<const uint16_t *>(sl + v) : (uint16_t)0;
    }
    // the tile's first and last ROW likewise, for the node chase (k_resolve_nodes): the other two wavefronts, one column
    // per lane.  No keys go with them: the pair pass reads its ring rows from the raster, coalesced.
    if (fo.edgeR && threadIdx.x >= 2 * DH) {
      static_assert(NTHR == 2 * DH + 2 * DW, "two wavefronts for the columns, two for the rows");
      const int side = (threadIdx.x >> 6) & 1, lxe = threadIdx.x & (DW - 1), lye = side ? DH - 1 : 0;
      const uint16_t v = lp[lye * LPD + lxe];
      const bool in = inner || (x0 + lxe < w && y0 + lye < h);
      fo.edgeR[((size_t)t * 2 + side) * DW + lxe] = in ? *reinterpret_cast<const uint16_t *>(sl + v) : (uint16_t)0;
    }
  }
}

// node -> its basin as a component id: curN[n] = basin, or B | CLOSED for the outside.  A pending node names the first
// cell outside its tile on the path: that cell's node is looked up through lab16 and the tile bases, and so on from
// tile to tile.  A pit's word is its number WITHIN ITS STRIPE: the basin id is that plus the stripe's offset, the stripe
// being that of the node the word was found in.  A chain of several hops is shortened for the others: the node's word
// becomes the last cell of the chain (any value ever stored in G is a valid continuation: concurrent chasers and stale
// reads are harmless).  grid: (nodes of the fullest stripe, stripes).
// edgeS / edgeR (optional, both or none): the label of the cell comes from the edge records of its tile instead of the
// raster.  That is complete because every value ever stored in G with LAB_PEND is the first cell outside some tile on a
// descent path -- the words of the descent kernel by construction, the shortened words `LAB_PEND | last` because `last`
// was itself the target of a hop -- and such a cell lies on the outer ring of its own tile: its first or last column
// (edgeS), its first or last row (edgeR), a corner in both.  A tile's nodes point into the edges of its 8 neighbours, so
// the records are read with locality where the raster gave a sector per 2-byte label.  (A cell on no edge cannot occur;
// it takes the raster's label all the same.)  Without records -- the fills with outlets, whose skipped tiles write
// none -- every label comes from lab16.
__global__ __launch_bounds__(NTHR) void k_resolve_nodes(uint32_t *G, const unsigned long long *__restrict__ counters,
                                                        const uint32_t *__restrict__ pitoff, uint32_t rcap,
                                                        const uint16_t *__restrict__ lab16,
                                                        const uint32_t *__restrict__ tile_base, int w, uint32_t tilesX,
                                                        uint32_t B, uint32_t *curN, uint32_t *flag,
                                                        const uint32_t *__restrict__ tid = nullptr,
                                                        const uint16_t *__restrict__ edgeS = nullptr,
                                                        const uint16_t *__restrict__ edgeR = nullptr) {
  const uint32_t st = blockIdx.y, i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= (uint32_t)(counters[st * FSTRIDE] >> 32)) return;
  const uint32_t n = st * rcap + i;
  uint32_t v = G[n], fn = n, last = 0;
  int hops = 0;
  while ((v & LAB_PEND) && v != OUTP) {
    const uint32_t cell = v & ~LAB_PEND;
    const uint32_t cx = cell % (uint32_t)w, cy = cell / (uint32_t)w;
    const uint32_t tile = (cy / DH) * tilesX + cx / DW;
    const uint32_t lx = cx % DW, ly = cy % DH;
    const uint16_t *src = lab16 + cell;
    if (edgeS) {
      if (lx == 0u || lx == (uint32_t)(DW - 1)) src = edgeS + ((size_t)tile * 2 + (lx != 0u)) * DH + ly;
      else if (ly == 0u || ly == (uint32_t)(DH - 1)) src = edgeR + ((size_t)tile * 2 + (ly != 0u)) * DW + lx;
    }
    fn = tile_base[tile] + (*src & (uint16_t)(DW * DH - 1));   // (the raster's label of a dissolved pit carries a flag)
    last = cell;
    v = __hip_atomic_load(&G[fn], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (++hops > (1 << 22)) { *flag = 1; break; }   // (cannot happen: descent paths are loop free)
  }
  if (hops > 1) __hip_atomic_store(&G[n], LAB_PEND | last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (v == OUTP || (v & LAB_PEND)) { curN[n] = B | CLOSED; return; }
  const uint32_t b = v + pitoff[fn / rcap];
  curN[n] = (tid && tid[b] != NO_TID) ? (b | CLOSED) : b;   // a shard's cut-row terminals are closed components
}

// A shard's cut-row cells are roots of their tiles with a pit number of their own: tid[basin] = terminal id (top row: x,
// bottom row: w + x), straight from the node table (a pit's word needs no chase), before the nodes are resolved.
__global__ __launch_bounds__(NTHR) void k_mark_terminals16(const uint16_t *__restrict__ lab16, const uint32_t *__restrict__ tile_base,
                                                           const uint32_t *__restrict__ G, const uint32_t *__restrict__ pitoff,
                                                           uint32_t rcap, uint32_t *tid, int w, int h, uint32_t dtx, int open_top,
                                                           int open_bottom) {
  const int x = blockIdx.x * NTHR + threadIdx.x;
  if (x <= 0 || x >= w - 1) return;
  if (open_top) {
    const uint32_t node = tile_base[(uint32_t)(x / DW)] + lab16[x];
    tid[G[node] + pitoff[node / rcap]] = (uint32_t)x;
  }
  if (open_bottom) {
    const uint32_t node = tile_base[(uint32_t)((h - 1) / DH) * dtx + (uint32_t)(x / DW)] + lab16[(size_t)(h - 1) * w + x];
    tid[G[node] + pitoff[node / rcap]] = (uint32_t)(w + x);
  }
}

// per node: the terminal id of its watershed after the local rounds (NO_TID: it drains to the true border inside the shard)
__global__ __launch_bounds__(NTHR) void k_node_watersheds(const uint32_t *__restrict__ curN, const uint32_t *__restrict__ cur,
                                                          const uint32_t *__restrict__ tid,
                                                          const unsigned long long *__restrict__ counters, uint32_t rcap, uint32_t B,
                                                          uint32_t *nodeW) {
  const uint32_t st = blockIdx.y, i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= (uint32_t)(counters[st * FSTRIDE] >> 32)) return;
  const uint32_t n = st * rcap + i;
  const uint32_t c = cur[curN[n] & ~CLOSED] & ~CLOSED;
  nodeW[n] = c == B ? NO_TID : tid[c];
}

// k_shard_edges on the compact labels: a cell's watershed terminal and locally filled level come from its NODE
// (tile base + 16-bit slot -> nodeW / lvl) instead of label -> component -> terminal.
template <class T, int TOPO>
__global__ __launch_bounds__(NTHR) void k_shard_edges16(const T *__restrict__ z, const uint16_t *__restrict__ lab16,
                                                        const uint32_t *__restrict__ tile_base, uint32_t dtx,
                                                        const uint32_t *__restrict__ nodeW, const uint32_t *__restrict__ lvl,
                                                        int w, int h, unsigned long long *hkeys, uint32_t *hvals, uint32_t hmask,
                                                        uint32_t *overflow, uint32_t tilesX, uint32_t ntiles) {
  __shared__ uint32_t sl[ELH * ELW];
  __shared__ uint32_t sw[ELH * ELW];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * EW, y0 = (int)(t / tilesX) * EH;
  constexpr int IPT = (ELH * ELW + NTHR - 1) / NTHR;
  uint32_t nv[IPT], kv[IPT];
  bool ok[IPT];
#pragma unroll
  for (int r = 0; r < IPT; r++) {   // batch 1: slot, node base of the cell's descent tile, elevation key
    const int i = threadIdx.x + r * NTHR;
    const int ly = i / ELW, lx = i - ly * ELW;
    const int gx = x0 - 1 + lx, gy = y0 + ly;
    ok[r] = i < ELH * ELW && gx >= 0 && gx < w && gy < h;
    const int cx = ok[r] ? gx : 0, cy = ok[r] ? gy : 0;
    const size_t g = (size_t)cy * w + cx;
    nv[r] = tile_base[(uint32_t)(cy / DH) * dtx + (uint32_t)(cx / DW)] + lab16[g];
    kv[r] = Key32<T>::to(z[g]);
  }
  uint32_t wv[IPT], av[IPT];
#pragma unroll
  for (int r = 0; r < IPT; r++) {   // batch 2: the node's watershed terminal and level
    wv[r] = nodeW[nv[r]];
    av[r] = lvl[nv[r]];
  }
#pragma unroll
  for (int r = 0; r < IPT; r++) {
    const int i = threadIdx.x + r * NTHR;
    if (i < ELH * ELW) {
      sl[i] = ok[r] ? wv[r] : E_INVALID;
      sw[i] = av[r] > kv[r] ? av[r] : kv[r];   // (the outside's level is 0)
    }
  }
  __syncthreads();
  const int lx = threadIdx.x & (EW - 1), ly0 = threadIdx.x >> 6;
#pragma unroll 2
  for (int j = 0; j < EH / 4; j++) {
    const int ly = ly0 + 4 * j;
    const int o = ly * ELW + lx + 1;
    const uint32_t la = sl[o];
    if (la == E_INVALID) continue;
    const uint32_t wa = sw[o];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (TOPO == 4 && (k == 1 || k == 3)) continue;
      const int q = o + (k == 0 ? 1 : k == 1 ? ELW - 1 : k == 2 ? ELW : ELW + 1);
      const uint32_t lb = sl[q];
      if (lb == la || lb == E_INVALID) continue;
      const uint32_t wb = sw[q];
      const uint32_t pass = wa > wb ? wa : wb;
      const uint32_t lo = la < lb ? la : lb, hi = la < lb ? lb : la;
      const unsigned long long key = (((unsigned long long)lo << 32) | hi) + 1ull;
      uint32_t slot = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & hmask;
      for (uint32_t probe = 0;; probe++) {
        if (probe > hmask) { *overflow = 1; break; }
        unsigned long long cur_k = __hip_atomic_load(&hkeys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur_k == 0) cur_k = atomicCAS(&hkeys[slot], 0ull, key);
        if (cur_k == 0 || cur_k == key) {
          if (__hip_atomic_load(&hvals[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > pass) atomicMin(&hvals[slot], pass);
          break;
        }
        slot = (slot + 1) & hmask;
      }
    }
  }
}

// level of every node: the final level of its basin (0 for the outside: never above a key that matters)
__global__ __launch_bounds__(NTHR) void k_node_levels(const uint32_t *__restrict__ curN, const uint32_t *__restrict__ acc,
                                                      const unsigned long long *__restrict__ counters, uint32_t rcap,
                                                      uint32_t *lvl) {
  const uint32_t st = blockIdx.y, i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= (uint32_t)(counters[st * FSTRIDE] >> 32)) return;
  const uint32_t n = st * rcap + i;
  lvl[n] = acc[curN[n] & ~CLOSED];
}

// z <- max(z, level of the cell's node).  One block per descent tile: its node levels (<= 4096) in LDS, then z and the
// 16-bit labels in quads; a quad is written back only when one of its cells is raised.
// curN / acc (optional, both or none; lvl is not read then): the kernel forms the levels itself, level of a node = acc[its
// basin], while it stages them -- the table pass that wrote lvl[] for this one reader (k_node_levels) is not needed.
// FLOOD (the plain fill, with curN / acc and tile_max): a tile wholly under one lake is written without being
// read.  The block stages its levels FIRST and reduces their minimum and maximum; when all are one level L and L lies
// strictly above tile_max[t], the tile's largest key (k_descent16), every cell of the tile comes out at L whatever it
// holds -- max(key, L) = L, a dissolved pit's max(key(q), L) = L as well, q being a cell of the tile -- so neither z nor
// lab16 is loaded.  Strictly: a cell AT the level keeps its bits today (-0.0 under a lake at +0.0).  Such a tile lies
// inside the raster (tile_max is 0xFFFFFFFF elsewhere).  Every other tile loads its quads after the decision and goes on
// as ever.  flooded (optional): counts the tiles written that way, for rdgpu_fill_flooded_tiles.
template <class T, bool VEC, bool FLOOD = false>
__global__ __launch_bounds__(NTHR) void k_finalize16(T *z, const uint16_t *__restrict__ lab16, const uint32_t *__restrict__ lvl,
                                                     const uint32_t *__restrict__ tile_base, const uint32_t *__restrict__ tile_count,
                                                     int w, int h, uint32_t tilesX, uint32_t ntiles,
                                                     const uint8_t *__restrict__ skip = nullptr,
                                                     const uint32_t *__restrict__ tlist = nullptr,
                                                     const uint32_t *__restrict__ curN = nullptr,
                                                     const uint32_t *__restrict__ acc = nullptr,
                                                     const uint32_t *__restrict__ tile_max = nullptr,
                                                     unsigned long long *flooded = nullptr) {
  __shared__ uint32_t sl[DH * DW];
  __shared__ uint32_t wlo[NTHR / 64], whi[NTHR / 64];
  const uint32_t t = tlist ? tlist[blockIdx.x] : xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  if (skip && skip[t]) return;
  const int x0 = (int)(t % tilesX) * DW, y0 = (int)(t / tilesX) * DH;
  const int qx = threadIdx.x & 15, ry = threadIdx.x >> 4;   // 16 quads per row, rows ry, ry + 16, ry + 32, ry + 48
  const int gx = x0 + 4 * qx;
  Quad<T> zqs[DH / 16];
  Quad<uint16_t> lqs[DH / 16];
  auto load_quads = [&]() {
#pragma unroll
    for (int r = 0; r < DH / 16; r++) {
      const int gy = y0 + ry + 16 * r;
      const bool in = gx < w && gy < h;
      const size_t g = in ? (size_t)gy * w + gx : 0;
      zqs[r] = load_quad<T, VEC>(z + (g - (in ? gx : 0)), in ? gx : 0, w, T());
      lqs[r] = load_quad<uint16_t, VEC>(lab16 + (g - (in ? gx : 0)), in ? gx : 0, w, (uint16_t)0);
    }
  };
  if (FLOOD) {
    // the tile's three words, then the two gathers, with nothing in between: every other tile's quads wait for this chain
    const uint32_t base = tile_base[t], cnt = tile_count[t], kmax = tile_max[t];
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint32_t i = threadIdx.x; i < cnt; i += NTHR) {
      const uint32_t L = acc[curN[base + i] & ~CLOSED];
      sl[i] = L;
      lo = min(lo, L);
      hi = max(hi, L);
    }
    lo = wave_min_u32(lo);
    hi = wave_max_u32(hi);
    if ((threadIdx.x & 63) == 0) { wlo[threadIdx.x >> 6] = lo; whi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = min(min(wlo[0], wlo[1]), min(wlo[2], wlo[3]));
    hi = max(max(whi[0], whi[1]), max(whi[2], whi[3]));
    // (block-uniform.  lo == hi is a guard: above the tile's largest key the levels can only be one lake's)
    if (lo == hi && lo > kmax) {
      const T v = Key32<T>::from(lo);
#pragma unroll
      for (int r = 0; r < DH / 16; r++) {
        const size_t g = (size_t)(y0 + ry + 16 * r) * w + gx;   // (an interior tile: every quad lies in the raster)
        if (VEC) {
          struct alignas(4 * sizeof(T)) AQ { T v[4]; };
          AQ a;
#pragma unroll
          for (int e = 0; e < 4; e++) a.v[e] = v;
          *reinterpret_cast<AQ *>(z + g) = a;
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++) z[g + e] = v;
        }
      }
      if (flooded && threadIdx.x == 0) atomicAdd(flooded, 1ull);
      return;
    }
    load_quads();
  } else {
    // the thread's quads first (in flight while the node levels arrive), then the tile's levels into LDS
    load_quads();
    const uint32_t base = tile_base[t], cnt = tile_count[t];
    if (curN) {
      for (uint32_t i = threadIdx.x; i < cnt; i += NTHR) sl[i] = acc[curN[base + i] & ~CLOSED];
    } else {
      for (uint32_t i = threadIdx.x; i < cnt; i += NTHR) sl[i] = lvl[base + i];
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < DH / 16; r++) {
    const int gy = y0 + ry + 16 * r;
    if (gx >= w || gy >= h) continue;
    const size_t g = (size_t)gy * w + gx;
    Quad<T> zq = zqs[r];
    const Quad<uint16_t> lq = lqs[r];
    bool any = false;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (gx + e >= w) continue;
      const uint32_t lab = lq.v[e];
      uint32_t L = sl[lab & (uint32_t)(DW * DH - 1)];
      if (lab & 0x8000u) {
        // a dissolved pit (k_descent16): its floor is the key of q, the neighbour it points at, in the same descent
        // tile and basin.  z[q] is read now, maybe while another thread raises it: to max(key(q), L), so the same result.
        const int d = (int)(lab >> 12) & 7, n = d < 4 ? d : d + 1, nr = n >= 6 ? 2 : n >= 3 ? 1 : 0, nc = n - 3 * nr;
        const T zn = z[(size_t)(gy + nr - 1) * w + (size_t)(gx + e + nc - 1)];   // (no border cell: q lies in the raster)
        const uint32_t kq = Key32<T>::to(zn);
        L = kq > L ? kq : L;
      }
      if (L > Key32<T>::to(zq.v[e])) { zq.v[e] = Key32<T>::from(L); any = true; }
    }
    if (any) {
      if (VEC) {
        struct alignas(4 * sizeof(T)) AQ { T v[4]; };
        AQ a;
#pragma unroll
        for (int e = 0; e < 4; e++) a.v[e] = zq.v[e];
        *reinterpret_cast<AQ *>(z + g) = a;
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (gx + e < w) z[g + e] = zq.v[e];
      }
    }
  }
}

// ==========================================================================================================
// The pair pass of the compact-label fill, a PERSISTENT kernel (r04).
//
// It is persistent because one block per 64 x 32 tile spent two thirds of its wave cycles parked on a chain of dependent
// global round trips (tile bases -> 16-bit labels -> component gathers from the node table) before its LDS phases could
// start.  Here a block stays resident and walks its share of the tiles (its XCD's band, strided by the number of blocks
// per XCD); the NEXT tile's rows, labels, ring cells and the node table of its descent tile are loaded into registers
// while the current tile goes through its LDS phases, so the phases of successive tiles follow each other without the
// round trips in between.  The components of the tile's own cells come from the descent
// tile's node table staged in LDS (one coalesced read of its ~80 entries instead of 2 048 gathers); only the 129 cells
// of the ring, which belong to the neighbouring descent tiles, are gathered one by one.  Phases, tables, records and
// proposals are k_scan<EMIT>'s.
// ==========================================================================================================
constexpr int NT_CAP = 512;   // node-table entries of one descent tile held in LDS (more: gathered from HBM)
static_assert(NT_CAP * 4 <= PT_SLOTS * 8, "the node table lives in the pair table's storage");
static_assert(NT_CAP % NTHR == 0, "a thread stages NT_CAP / NTHR entries");
// Boundary cells the list holds.  A tile with more (block-uniform: the wavefronts' counts summed in LDS) is worked one
// band of TH / 4 rows at a time, list -> barrier -> pair loop per band, the pair table accumulating across the bands.
// 1 008 and not 1 024: with the four words below the kernel's LDS is 22 528 bytes, seven blocks to a CU.
constexpr int LIST_CAP = 1008;
static_assert(LIST_CAP >= TW * (TH / 4), "a band's boundary cells fit the list");
static_assert(LIST_CAP >= PT_SLOTS, "the list holds the occupied slots of the pair table afterwards");
static_assert(2 * (TH + 1) * LW * 4 + LIST_CAP * 2 + PT_SLOTS * 12 + 16 <= 22528, "k_pairs16: LDS of seven blocks per CU");
static_assert(TW == DW && DH % TH == 0, "a scan tile lies inside one descent tile");
constexpr uint32_t NO_TILE = 0xFFFFFFFFu;
// a 16-bit label's slot: the plain fill's descent flags a dissolved pit in the four bits above it, for the finalize alone
constexpr uint32_t LAB16_SLOT = (uint32_t)(DW * DH - 1);
// The pair pass looks E, SE, S and SW only: of the halo around a tile it reads the row below, the column to the right and
// the left column from the tile's second row down -- never the row above (the tile above finds those pairs) or the cell to
// the left of the first row.  Those cells are neither loaded nor staged, and the LDS images start at the tile's first row.
constexpr int PLH = TH + 1;                    // LDS rows of the pair pass: the tile's and the ring row below
constexpr int RING = LW + TH + (TH - 1);       // ring cells: the row below, the right column, the left column from row 2

// A pair that found no slot in the tile's table goes straight to the BLOCK's segment (k_pairs16: one segment per
// resident block, filled through a counter in LDS) and proposes on its own.
__device__ __forceinline__ void pair_spill_local(const EdgeOut &eo, unsigned long long *best, uint32_t seg, uint32_t *seg_fill,
                                                 uint32_t lo, uint32_t hi, uint32_t key) {
  const unsigned long long cl = ((unsigned long long)key << 32) | hi, ch = ((unsigned long long)key << 32) | lo;
  if (!(lo & CLOSED) && cl < best[lo]) atomicMin(&best[lo], cl);
  if (!(hi & CLOSED) && ch < best[hi]) atomicMin(&best[hi], ch);
  const uint32_t g = atomicAdd(seg_fill, 1u);
  if (g < eo.seglimit) {
    const size_t i = (size_t)seg * eo.segcap + g;
    eo.a[i] = lo; eo.b[i] = hi; eo.k[i] = key;
  } else {
    *eo.overflow = 1;
  }
}

#ifdef RDGPU_PROBES
// tools/probes/pairs_residency.py: wall_clock64() of every block of the k_pairs16 launches at entry [2 b] and at exit
// [2 b + 1] -- all blocks of a grid of resident blocks have entered before the first one leaves
__device__ unsigned long long *g_probe_pairs_clock = nullptr;
extern "C" int rdgpu_probe_pairs_clock(unsigned long long *d_clock) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_probe_pairs_clock), &d_clock, sizeof d_clock) == hipSuccess ? 0 : 1;
}
// tools/probes/coarse_flood.py: a device array of one byte per descent tile that the plain fill hands to the PAIR PASS ONLY
// as its `skip` (nullptr: none).  The surface of such a fill is wrong; what the run is for is k_pairs16's traced time
// without those tiles.
static const uint8_t *g_probe_pairs_skip = nullptr;
extern "C" int rdgpu_probe_pairs_skip(const uint8_t *d_skip) {
  g_probe_pairs_skip = d_skip;
  return 0;
}
#endif

// The kernel is held to 96 SGPRs (it takes all 102 when let, and spills to VGPR lanes either way; no scratch): a CU admits
// seven 256-thread blocks only up to an .sgpr_count of 96, and the LDS (22 528 B) and the VGPRs (<= 72) are cut for seven.
template <class T, int TOPO, bool VEC>
__global__ __launch_bounds__(NTHR) __attribute__((amdgpu_num_sgpr(96))) void k_pairs16(const T *__restrict__ z, const uint16_t *__restrict__ lab16,
                                                  const uint32_t *__restrict__ curN, unsigned long long *best,
                                                  int w, int h, uint32_t B, uint32_t tilesX,
                                                  const uint32_t *__restrict__ tiles_in, uint32_t nwork,
                                                  EdgeOut eo,
                                                  const uint32_t *__restrict__ tile_base,
                                                  const uint32_t *__restrict__ tile_count, uint32_t dtx,
                                                  const uint8_t *__restrict__ skip,
                                                  const uint32_t *__restrict__ edgeK, const uint16_t *__restrict__ edgeS) {
  __shared__ __attribute__((aligned(8))) uint32_t sk[PLH * LW];   // (row r = the tile's row r; column 0 = the left ring column)
  __shared__ uint32_t sc[PLH * LW];
  __shared__ __attribute__((aligned(4))) uint16_t list[LIST_CAP];   // boundary cells
  __shared__ unsigned long long pt_pair[PT_SLOTS];                  // the pair table; before it is reset: the node table
  uint32_t *const ntab = reinterpret_cast<uint32_t *>(pt_pair);
  __shared__ uint32_t pt_key[PT_SLOTS];
  __shared__ uint32_t nlist, pt_n, pt_base, seg_fill;
  uint32_t *const tab_id = sk;   // the component table lives in the keys' storage once the pairs are reduced
  unsigned long long *const tab_val = reinterpret_cast<unsigned long long *>(sk + SC_SLOTS);

  // ---- this block's tiles: its XCD's band, strided over the XCD's blocks (tile j, j + blocks, ...), so that the blocks of
  // an XCD work on neighbouring tiles at any time (a run of consecutive tiles per block was measured 0.15 ms slower;
  // neither keeps the neighbours' rows in the 4 MB L2 for the ring columns -- hence the edge records: 22.9 GB fetched per
  // launch without them, 12.5 with).
  const uint32_t xcd = blockIdx.x & 7u, kstep = gridDim.x >> 3, per = (nwork + 7u) / 8u;
  const uint32_t seg = blockIdx.x;   // the block's own segment of the pair list: no counter in HBM to wait for
  uint32_t it = blockIdx.x >> 3;
  auto next_tile = [&](uint32_t &i) -> uint32_t {
    while (i < per) {
      const uint32_t wi = xcd * per + i;
      if (wi >= nwork) break;
      const uint32_t t = tiles_in ? tiles_in[wi] : wi;
      if (!skip) return t;
      const int x0 = (int)(t % tilesX) * TW, y0 = (int)(t / tilesX) * TH;
      if (!skip[(uint32_t)(y0 / DH) * dtx + (uint32_t)(x0 / DW)]) return t;
      i += kstep;
    }
    i = per;
    return NO_TILE;
  };
  if (threadIdx.x == 0) seg_fill = 0;

  // ---- the prefetched tile (registers) -----------------------------------------------------------------------------
  Quad<T> zq[2];
  Quad<uint16_t> lq[2];
  T rz = T();
  uint32_t rl = 0, rtb = 0, rc = 0, tbC = 0, cnt = 0, rkey = 0;
  uint32_t nt[NT_CAP / NTHR];
  // ring cell of a thread (threads >= RING repeat the last one's loads and store nothing).  Everything that depends on
  // the thread index is recomputed from an opaque copy of it in every trip of the tile loop: hoisted out of the loop
  // these few dozen offsets and addresses cost 30 VGPRs, i.e. a third of the resident blocks.
  // (ring coordinates as before: the cell is raster cell (x0 - 1 + ring_x, y0 - 1 + ring_y); ring_y is 1 ... TH + 1)
  auto ring_y = [](int tid) { const int rk = min(tid, RING - 1); return rk < LW ? TH + 1 : rk < LW + TH ? rk - LW + 1 : rk - LW - TH + 2; };
  auto ring_x = [](int tid) { const int rk = min(tid, RING - 1); return rk < LW ? rk : rk < LW + TH ? LW - 1 : 0; };

  auto load_a = [&](uint32_t t, int tid) {   // everything that only needs the tile's coordinates; branch free (clamped addresses)
    const int x0 = (int)(t % tilesX) * TW, y0 = (int)(t / tilesX) * TH;
    const uint32_t dC = (uint32_t)(y0 / DH) * dtx + (uint32_t)(x0 / DW);
    tbC = tile_base[dC];
    cnt = tile_count[dC];
    {   // the ring first: its component gather (load_b) then only waits for these
      const int rx = ring_x(tid), ry = ring_y(tid);
      const int gx = min(max(x0 - 1 + rx, 0), w - 1), gy = min(max(y0 - 1 + ry, 0), h - 1);
      // a ring COLUMN cell comes from the neighbouring descent tile's edge records (edgeK / edgeS, when the descent
      // wrote them): the left ring column is that tile's last column, the right one its first
      const bool col = edgeK && ry <= TH && tid < RING;
      const uint32_t dtn = (uint32_t)(gy / DH) * dtx + (uint32_t)(gx / DW);
      const size_t e = ((size_t)dtn * 2 + (rx == 0 ? 1 : 0)) * DH + (uint32_t)(gy % DH);
      const size_t g = col ? (size_t)y0 * w + x0 : (size_t)gy * w + gx;   // (a column cell reads nothing new from the raster)
      rtb = tile_base[dtn];
      rl = col ? (uint32_t)edgeS[e] : (uint32_t)lab16[g] & LAB16_SLOT;
      rkey = col ? edgeK[e] : 0u;
      rz = z[g];
    }
    // the tile's quads: the tile's first cell is a block-uniform (scalar) address, a thread adds a 32-bit byte offset
    const size_t tile0 = (size_t)y0 * w + x0;
    const char *zt = reinterpret_cast<const char *>(z + tile0), *lt = reinterpret_cast<const char *>(lab16 + tile0);
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int i = tid + r * NTHR;
      const int ly = i / (TW / 4), q = i - ly * (TW / 4);
      const int gx = x0 + 4 * q, gy = y0 + ly;
      const bool ok = gy < h && gx < w;
      if (VEC) {
        const uint32_t cell = ok ? (uint32_t)ly * (uint32_t)w + 4u * (uint32_t)q : 0u;
        struct alignas(4 * sizeof(T)) AZ { T v[4]; };
        struct alignas(8) AL { uint16_t v[4]; };
        const AL a = *reinterpret_cast<const AL *>(lt + cell * (uint32_t)sizeof(uint16_t));
        const AZ b = *reinterpret_cast<const AZ *>(zt + cell * (uint32_t)sizeof(T));
#pragma unroll
        for (int e = 0; e < 4; e++) { lq[r].v[e] = a.v[e]; zq[r].v[e] = b.v[e]; }
      } else {
        const size_t row = ok ? (size_t)gy * w : 0;
        lq[r] = load_quad<uint16_t, false>(lab16 + row, ok ? gx : 0, w, (uint16_t)0);
        zq[r] = load_quad<T, false>(z + row, ok ? gx : 0, w, T());
        if (!ok)   // (the raster's first cells stand in: THEIR labels belong to another descent tile; slot 0 exists in every tile)
#pragma unroll
          for (int e = 0; e < 4; e++) lq[r].v[e] = 0;
      }
    }
  };
  auto load_b = [&](int tid) {   // what needs load_a's words: the node table, the ring cells' components
    const uint32_t nn = (cnt <= (uint32_t)NT_CAP && cnt) ? cnt : 1u;
    nt[0] = curN[tbC + min((uint32_t)tid, nn - 1u)];   // (cnt >= 1: the tile holds a cell)
    if (nn > (uint32_t)NTHR) {   // (block-uniform) a tile has about 80 nodes: one load per thread holds them
#pragma unroll
      for (int k = 1; k < NT_CAP / NTHR; k++) {
        const uint32_t idx = (uint32_t)tid + k * NTHR;
        nt[k] = curN[tbC + min(idx, nn - 1u)];
      }
    }
    rc = curN[rtb + rl];
  };

#ifdef RDGPU_PROBES
  if (g_probe_pairs_clock && threadIdx.x == 0) g_probe_pairs_clock[2 * blockIdx.x] = g_probe_pairs_clock[2 * blockIdx.x + 1] = wall_clock64();
#endif
  uint32_t t = next_tile(it);
  if (t == NO_TILE) return;
  load_a(t, (int)threadIdx.x);
  load_b((int)threadIdx.x);
  constexpr int ROWS = TH / 4;
  for (;;) {
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));   // opaque: see above
    const int lane = tid & 63;
    const int rly = ring_y(tid), rlx = ring_x(tid);
    const bool isring = tid < RING;
    const int x0 = (int)(t % tilesX) * TW, y0 = (int)(t / tilesX) * TH;
    // ---- stage 1: the node table of the tile's descent tile; reset the tile's tables --------------------------------
    const bool tabled = cnt <= (uint32_t)NT_CAP;
    ntab[tid] = nt[0];
    if (tabled && cnt > (uint32_t)NTHR) {   // (as load_b loaded them; a label is < cnt: nothing past cnt is looked up)
#pragma unroll
      for (int k = 1; k < NT_CAP / NTHR; k++) ntab[tid + k * NTHR] = nt[k];
    }
    if (tid == 0) { nlist = 0; pt_n = 0; }
    __syncthreads();
    // ---- stage 2: keys and components of the tile and its ring into LDS ---------------------------------------------
    {
      uint32_t cq[2][4];
      // (a quad outside the raster holds labels of this descent tile -- its first quad's, or zeros: the lookups need no
      // guard -- and a label is < cnt <= NT_CAP when the table is used)
      if (tabled) {
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
          for (int e = 0; e < 4; e++) cq[r][e] = ntab[lq[r].v[e] & LAB16_SLOT];
      } else {   // more nodes than the table holds (white noise): gathered
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
          for (int e = 0; e < 4; e++) cq[r][e] = curN[tbC + ((uint32_t)lq[r].v[e] & LAB16_SLOT)];
      }
      if (x0 + TW <= w && y0 + TH <= h) {   // (block-uniform) the whole tile lies in the raster: no tests
#pragma unroll
        for (int r = 0; r < 2; r++) {
          const int i = tid + r * NTHR;
          const int ly = i / (TW / 4), q = i - ly * (TW / 4);
          const int o = ly * LW + 1 + 4 * q;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            sk[o + e] = key32_fast<T>(zq[r].v[e]);
            sc[o + e] = cq[r][e];
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < 2; r++) {
          const int i = tid + r * NTHR;
          const int ly = i / (TW / 4), q = i - ly * (TW / 4);
          const int gx = x0 + 4 * q, gy = y0 + ly;
          const int o = ly * LW + 1 + 4 * q;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const bool in = gy < h && gx + e < w;
            sk[o + e] = in ? key32_fast<T>(zq[r].v[e]) : 0u;
            sc[o + e] = in ? cq[r][e] : (B | CLOSED);
          }
        }
      }
      if (isring) {
        const int gx = x0 - 1 + rlx, gy = y0 - 1 + rly;
        const bool ok = gx >= 0 && gx < w && gy >= 0 && gy < h;
        const bool col = edgeK && rly <= TH;
        sk[(rly - 1) * LW + rlx] = ok ? (col ? rkey : key32_fast<T>(rz)) : 0u;
        sc[(rly - 1) * LW + rlx] = ok ? rc : (B | CLOSED);
      }
    }
    // ---- the next tile's loads go out now and land while this tile is worked on ---------------------------------------
    it += kstep;
    const uint32_t tn = next_tile(it);
    const uint32_t tl = tn != NO_TILE ? tn : t;   // (no next tile: this one's rows once more -- cheaper than a branch)
    load_a(tl, tid);
    __syncthreads();
    // (the node table's storage becomes the pair table: every lookup in it was made before the barrier above)
    pt_pair[tid] = ~0ull;
    pt_key[tid] = 0xFFFFFFFFu;
    static_assert(PT_SLOTS == NTHR, "one slot per thread");
    // ---- phase 1: detect (k_scan's) -----------------------------------------------------------------------------------
    constexpr int NF = TOPO == 8 ? 4 : 2;
    const int foff[4] = {1, TOPO == 8 ? LW + 1 : LW, LW, LW - 1};
    // pass 0 lists the whole tile.  Only when that is more than the list holds do passes 1 ... 4 follow, one band each
    // (white noise; a tile of the bench DEM has ~450 boundary cells): the wavefront of the band detects once more.
#pragma nounroll
    for (int pass = 0;; pass++) {
    // (the thread's offsets once more from an opaque copy of its index, so that none of them is kept across the pair loop
    // for the passes that hardly ever come)
    asm volatile("" : "+v"(tid));
    const int band = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (pass == 0 || band == pass - 1) {
      const int lx = tid & (TW - 1), lane = tid & 63;
      const int gxl = x0 + lx;
      const int yb = band * ROWS;
      uint32_t c1[3], c2[3];
      {
        const int o = yb * LW + lx;   // (c1[0] of the tile's first row is the one cell nobody staged: it is not used)
#pragma unroll
        for (int e = 0; e < 3; e++) c1[e] = sc[o + e];
      }
      unsigned long long bal[ROWS];
      bool bnd[ROWS];
      // (k_scan's "the tile still holds an open boundary" flag feeds the raster rounds, which this path does not have)
      const int rows_in = min(h - y0 - yb, ROWS);   // rows of this band inside the raster
      const bool colin = gxl < w;
#pragma unroll
      for (int j = 0; j < ROWS; j++) {
        const int ly = yb + j;
        {
          const int o = (ly + 1) * LW + lx;
#pragma unroll
          for (int e = 0; e < 3; e++) c2[e] = sc[o + e];
        }
        const uint32_t C = c1[1];
        uint32_t df = (c1[2] ^ C) | (c2[1] ^ C);
        if (TOPO == 8) df |= (c2[0] ^ C) | (c2[2] ^ C);
        // (opaque: else the or-chain becomes one compare per neighbour and the or is done on lane masks, by the scalar unit)
        asm volatile("" : "+v"(df));
        bnd[j] = df != 0 && colin && j < rows_in;
        bal[j] = __builtin_amdgcn_ballot_w64(bnd[j]);   // (the builtin: __ballot() costs two VALU instructions)
#pragma unroll
        for (int e = 0; e < 3; e++) c1[e] = c2[e];
      }
      uint32_t total = 0;
#pragma unroll
      for (int j = 0; j < ROWS; j++) total += (uint32_t)__popcll(bal[j]);
      if (total) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&nlist, total);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base + total <= (uint32_t)LIST_CAP)   // (else nlist ends above LIST_CAP, and the bands' passes follow)
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
          if (bnd[j])
            list[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[j] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[j], 0u))] =
                (uint16_t)((yb + j) * LW + lx + 1);
          base += (uint32_t)__popcll(bal[j]);
        }
      }
    }
    __syncthreads();
    if (pass == 0) load_b(tid);
    // ---- phase 2: the pairs (k_scan<EMIT>'s) -----------------------------------------------------------------------
    const uint32_t nl = nlist;
    if (nl <= (uint32_t)LIST_CAP)
    for (uint32_t i = tid; i < nl; i += NTHR) {
      const int o = list[i];
      const uint32_t C = sc[o], kc = sk[o];
      uint32_t nD[NF], nH[NF];
#pragma unroll
      for (int e = 0; e < NF; e++) { nD[e] = sc[o + foff[e]]; nH[e] = sk[o + foff[e]]; }
      uint32_t pd[2] = {C, C}, pk[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
      for (int e = 0; e < NF; e++) {
        const uint32_t D = nD[e], hn = nH[e] > kc ? nH[e] : kc;
        if (D != C && !(C & D & CLOSED)) {
          if (pd[0] == C) pd[0] = D;
          if (D == pd[0]) pk[0] = hn < pk[0] ? hn : pk[0];
          else {
            if (pd[1] == C) pd[1] = D;
            if (D == pd[1]) pk[1] = hn < pk[1] ? hn : pk[1];
            else if (!pair_insert(pt_pair, pt_key, C < D ? C : D, C < D ? D : C, hn))
              pair_spill_local(eo, best, seg, &seg_fill, C < D ? C : D, C < D ? D : C, hn);
          }
        }
      }
      uint32_t ps[2], pq[2], lo[2], hi[2];
      unsigned long long pv[2];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        lo[j] = C < pd[j] ? C : pd[j];
        hi[j] = C < pd[j] ? pd[j] : C;
        ps[j] = pair_home(lo[j], hi[j]);
        pv[j] = pt_pair[ps[j]];
        pq[j] = pt_key[ps[j]];
      }
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (pd[j] != C) {
          const unsigned long long pr = ((unsigned long long)lo[j] << 32) | hi[j];
          if (pv[j] == pr) { if (pk[j] < pq[j]) atomicMin(&pt_key[ps[j]], pk[j]); }
          else if (!pair_insert(pt_pair, pt_key, lo[j], hi[j], pk[j])) pair_spill_local(eo, best, seg, &seg_fill, lo[j], hi[j], pk[j]);
        }
      }
    }
    if (pass == 0 ? nl <= (uint32_t)LIST_CAP : pass == TH / ROWS) break;
    __syncthreads();   // every thread has read nlist and is through with the list
    if (tid == 0) nlist = 0;
    __syncthreads();
    }
    __syncthreads();
    tab_id[tid] = 0xFFFFFFFFu;
    tab_val[tid] = ~0ull;
    static_assert(SC_SLOTS == NTHR, "one slot per thread");
    {
      const bool occ = pt_pair[tid] != ~0ull;
      const unsigned long long bal = __ballot(occ);
      uint32_t base = 0;
      if (lane == 0 && bal) base = atomicAdd(&pt_n, (uint32_t)__popcll(bal));
      base = __shfl(base, 0, 64);
      if (occ) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)tid;
    }
    __syncthreads();
    const uint32_t tot = pt_n;
    if (tid == 0) {
      uint32_t ob = seg_fill;   // (spills are over: nothing else touches the counter until the next tile's pairs)
      if (ob + tot > eo.seglimit) { *eo.overflow = 1; ob = 0xFFFFFFFFu; }
      else seg_fill = ob + tot;
      pt_base = ob;
    }
    for (uint32_t i = tid; i < tot; i += NTHR) {
      const int sl = list[i];
      const unsigned long long pr = pt_pair[sl];
      const uint32_t lo = (uint32_t)(pr >> 32), hi = (uint32_t)pr, key = pt_key[sl];
      if (!(lo & CLOSED)) {
        const unsigned long long cand = ((unsigned long long)key << 32) | hi;
        const int slot = tab_slot(tab_id, lo);
        if (slot >= 0) atomicMin(&tab_val[slot], cand);
        else if (cand < best[lo]) atomicMin(&best[lo], cand);
      }
      if (!(hi & CLOSED)) {
        const unsigned long long cand = ((unsigned long long)key << 32) | lo;
        const int slot = tab_slot(tab_id, hi);
        if (slot >= 0) atomicMin(&tab_val[slot], cand);
        else if (cand < best[hi]) atomicMin(&best[hi], cand);
      }
    }
    __syncthreads();
    {
      const uint32_t C = tab_id[tid];
      if (C != 0xFFFFFFFFu) {
        const unsigned long long cand = tab_val[tid];
        if (cand < best[C]) atomicMin(&best[C], cand);   // cheap (possibly stale) pre-check first
      }
    }
    const uint32_t ob = pt_base;
    if (ob != 0xFFFFFFFFu) {
      const size_t g0 = (size_t)seg * eo.segcap + ob;
      for (uint32_t i = tid; i < tot; i += NTHR) {
        const int sl = list[i];
        const unsigned long long pr = pt_pair[sl];
        eo.a[g0 + i] = (uint32_t)(pr >> 32);
        eo.b[g0 + i] = (uint32_t)pr;
        eo.k[g0 + i] = pt_key[sl];
      }
    }
    __syncthreads();   // the tables, the list and the keys' storage are free for the next tile
    if (tn == NO_TILE) break;
    t = tn;
  }
  // (after an overflow seg_fill can lie past seglimit: the rounds enqueued before the host sees the flag read only the
  // records that were written)
  if (threadIdx.x == 0) eo.segcount[seg] = min(seg_fill, eo.seglimit);
#ifdef RDGPU_PROBES
  if (g_probe_pairs_clock && threadIdx.x == 0) g_probe_pairs_clock[2 * blockIdx.x + 1] = wall_clock64();
#endif
}

// ==========================================================================================================
// The coarse flood (r13): tiles the pair pass need not visit.
//
// lb = the fill of the raster of block minima that k_descent16 left (COARSE_CB x COARSE_CB blocks): a lower bound of the
// filled surface, since a path of cells to the border maps to a path of blocks whose maximum is not larger.  An interior
// descent tile whose blocks all have lb above the tile's largest key is strictly raised everywhere, hence (r11) wholly under
// one lake at some level L above that key: FLAGGED.  k_pairs16 takes flag[] as its `skip`.
// ==========================================================================================================
__global__ __launch_bounds__(NTHR) void k_flag_tiles(const uint32_t *__restrict__ tile_max, const uint32_t *__restrict__ lb,
                                                     uint32_t dtx, uint32_t dnt, uint32_t cbx, uint8_t *__restrict__ flag,
                                                     unsigned long long *count) {
  const uint32_t t = blockIdx.x * NTHR + threadIdx.x;
  if (t >= dnt) return;
  const uint32_t km = tile_max[t];
  bool f = false;
  if (km != 0xFFFFFFFFu) {   // interior: its DW / COARSE_CB blocks a side all lie in the coarse raster
    constexpr uint32_t BPT = DW / COARSE_CB;
    const uint32_t bx0 = (t % dtx) * BPT, by0 = (t / dtx) * BPT;
    uint32_t m = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t j = 0; j < BPT; j++)
#pragma unroll
      for (uint32_t i = 0; i < BPT; i++) m = min(m, lb[(size_t)(by0 + j) * cbx + bx0 + i]);
    f = m > km;
  }
  flag[t] = f ? 1 : 0;
  // (RDGPU_FILL_COUNT_COARSE=1 only.  A list of the flagged tiles for k_pairs_flooded, appended to with one atomic add per
  // wavefront, cost this kernel 70 us on its one counter and saved the other nothing: its time is not in the idle wavefronts.)
  if (count && f) atomicAdd(count, 1ull);
}

// What stands in for a flagged tile's pair pass.  Every pair the tile's own scan would find joins two basins that end at
// the tile's level L, below L; such an edge never decides a level (after the last of them a path to the outside goes on from
// a basin of level L, with a maximum >= L), so they may be replaced by anything below L that keeps those basins connected.
// With R the first basin of the tile's node table and K = tile_max[t] < L:
//   star  (R, p, K) for every other basin p of the node table;
//   ring  (R, basin(b), max(K, key(b))) for every cell b outside the tile that its forward scan meets (D8: the column to
//         the right, the row below with both corners, the left column from the second row; D4: right column and row below):
//         the true weight where key(b) >= L, and an edge below L between two basins of level L where not.
// One record per distinct basin (a table per wavefront in LDS; what finds no slot goes out on its own).  Nothing of the
// tile's own cells is read.  One wavefront per tile and one trip: every load that needs only the tile's index goes out
// first, the gathers from the node table second -- the kernel is three round trips to HBM long and lives on the number
// of wavefronts in flight (a persistent version, 512 blocks walking the tiles, took 1.1 ms at S3: 190 trips of dependent
// round trips each).  The records go to the segments [seg0, seg0 + nfseg) of the pair list, behind the pair pass's; a
// segment is shared by the blocks with blockIdx.x % nfseg in common, through its fill count in HBM (one atomic add per
// tile; zeroed with the pair pass's counts before the launch).
constexpr int FT_SLOTS = 256, FT_PROBES = 16;
template <class T, int TOPO>
__global__ __launch_bounds__(NTHR) void k_pairs_flooded(const T *__restrict__ z, const uint16_t *__restrict__ lab16,
                                                        const uint32_t *__restrict__ curN, unsigned long long *best, int w,
                                                        uint32_t dtx, uint32_t dnt, const uint8_t *__restrict__ flag,
                                                        const uint32_t *__restrict__ tile_max,
                                                        const uint32_t *__restrict__ tile_base,
                                                        const uint32_t *__restrict__ tile_count,
                                                        const uint32_t *__restrict__ edgeK, const uint16_t *__restrict__ edgeS,
                                                        EdgeOut eo, uint32_t seg0, uint32_t nfseg) {
  constexpr int NW = NTHR / 64;
  __shared__ uint32_t tb_id[NW][FT_SLOTS], tb_key[NW][FT_SLOTS];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  uint32_t *const ids = tb_id[wave], *const keys = tb_key[wave];
  const uint32_t seg = seg0 + blockIdx.x % nfseg;
  const uint32_t t = blockIdx.x * NW + (uint32_t)wave;
  const bool on = t < dnt && flag[t] != 0;   // (wavefront-uniform)
  if (on)
    for (int i = lane; i < FT_SLOTS; i += 64) { ids[i] = 0xFFFFFFFFu; keys[i] = 0xFFFFFFFFu; }
  // n records of the calling lanes (n: the wavefront's total, has: this lane has one) into the segment
  auto emit = [&](bool has, uint32_t p, uint32_t key, uint32_t R) {
    const unsigned long long bal = __ballot(has);
    if (bal == 0ull) return;
    const uint32_t n = (uint32_t)__popcll(bal);
    uint32_t g0 = 0;
    if (lane == __ffsll((long long)bal) - 1) {
      g0 = atomicAdd(&eo.segcount[seg], n);
      if (g0 + n > eo.seglimit) {   // (the count goes back: what reads the list afterwards never sees more than was written)
        atomicSub(&eo.segcount[seg], n);
        *eo.overflow = 1;
        g0 = 0xFFFFFFFFu;
      }
    }
    g0 = __shfl(g0, __ffsll((long long)bal) - 1, 64);
    if (!has) return;
    const uint32_t lo = min(R, p), hi = max(R, p);
    const unsigned long long cl = ((unsigned long long)key << 32) | hi, ch = ((unsigned long long)key << 32) | lo;
    if (!(lo & CLOSED) && cl < best[lo]) atomicMin(&best[lo], cl);
    if (!(hi & CLOSED) && ch < best[hi]) atomicMin(&best[hi], ch);
    if (g0 != 0xFFFFFFFFu) {
      const size_t i = (size_t)seg * eo.segcap + g0 + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      eo.a[i] = lo; eo.b[i] = hi; eo.k[i] = key;
    }
  };
  uint32_t R = 0, K = 0;
  // what a lane brings to the table: up to two nodes of the star (more: the loop below) and three ring cells
  uint32_t sp[2] = {0, 0}, rp[3] = {0, 0, 0}, rk[3] = {0, 0, 0};
  bool sh[2] = {false, false}, rh[3] = {false, false, false};
  uint32_t base = 0, cnt = 0, pB = 0, kB = 0;
  if (on) {
    base = tile_base[t]; cnt = tile_count[t]; K = tile_max[t];
    const int x0 = (int)(t % dtx) * DW, y0 = (int)(t / dtx) * DH;   // (an interior tile: its ring lies in the raster)
    // first trip: indices, slots and keys
    const size_t eR = ((size_t)(t + 1) * 2 + 0) * DH + lane;        // the right neighbour's first column
    const size_t eL = ((size_t)(t - 1) * 2 + 1) * DH + lane;        // the left neighbour's last column
    const uint32_t tbR = tile_base[t + 1], sR = edgeS[eR];
    rk[0] = edgeK[eR];
    uint32_t tbL = 0, sL = 0;
    rh[0] = true;
    rh[1] = TOPO == 8 && lane >= 1;
    if (rh[1]) { tbL = tile_base[t - 1]; sL = edgeS[eL]; rk[1] = edgeK[eL]; }
    // the row below: columns x0 ... x0 + 63, and with D8 the two corners from lanes 0 (x0 - 1) and 1 (x0 + 64)
    const int gy = y0 + DH;
    const size_t gB = (size_t)gy * w + x0 + lane;
    const uint32_t tB = (uint32_t)(gy / DH) * dtx + (uint32_t)(x0 / DW);
    const uint32_t tbB = tile_base[tB], sB = (uint32_t)lab16[gB] & LAB16_SLOT;
    const T zB = z[gB];
    rh[2] = TOPO == 8 && lane < 2;
    uint32_t tbC = 0, sC = 0;
    T zC = T();
    if (rh[2]) {
      const size_t gC = (size_t)gy * w + (lane ? x0 + DW : x0 - 1);
      tbC = tile_base[lane ? tB + 1 : tB - 1];
      sC = (uint32_t)lab16[gC] & LAB16_SLOT;
      zC = z[gC];
    }
    // second trip: the basins
    sh[0] = (uint32_t)lane < cnt;
    sh[1] = (uint32_t)lane + 64u < cnt;
    if (sh[0]) sp[0] = curN[base + lane];
    if (sh[1]) sp[1] = curN[base + 64 + lane];
    rp[0] = curN[tbR + sR];
    if (rh[1]) rp[1] = curN[tbL + sL];
    pB = curN[tbB + sB];
    if (rh[2]) { rp[2] = curN[tbC + sC]; rk[2] = key32_fast<T>(zC); }
    R = __shfl(sp[0], 0, 64);   // (cnt >= 1: the tile holds a cell)
    // the row below goes in with the ring cells: lane's own cell first
    rk[0] = max(K, rk[0]); rk[1] = max(K, rk[1]); rk[2] = max(K, rk[2]);
    kB = max(K, key32_fast<T>(zB));
  }
  __syncthreads();   // (the tables are clear)
  if (on) {
    auto put = [&](bool has, uint32_t p, uint32_t key) {   // (R, p, key) into the wavefront's table: the lowest key per basin p
      bool placed = !has || p == R;
      if (!placed) {
        uint32_t sl = (p * 0x9E3779B1u) >> 24;
        static_assert(FT_SLOTS == 256, "the hash's eight bits");
        for (int k = 0; k < FT_PROBES && !placed; k++, sl = (sl + 1) & (FT_SLOTS - 1)) {
          const uint32_t old = atomicCAS(&ids[sl], 0xFFFFFFFFu, p);
          if (old == 0xFFFFFFFFu || old == p) { atomicMin(&keys[sl], key); placed = true; }
        }
      }
      emit(!placed, p, key, R);   // (no slot within reach: the record goes out on its own; the wavefront calls together)
    };
    put(sh[0], sp[0], K);
    put(sh[1], sp[1], K);
    for (uint32_t i0 = 128; i0 < cnt; i0 += 64) {   // (wavefront-uniform; a tile of the bench DEM has ~80 nodes)
      const bool has = i0 + (uint32_t)lane < cnt;
      put(has, has ? curN[base + i0 + lane] : 0u, K);
    }
    put(true, pB, kB);
#pragma unroll
    for (int e = 0; e < 3; e++) put(rh[e], rp[e], rk[e]);
  }
  __syncthreads();   // (the wavefront's table is complete)
  if (on) {   // the table's records: one allocation in the segment, one proposal for R, one per other end
    constexpr int SPL = FT_SLOTS / 64;
    uint32_t p[SPL], k[SPL], n = 0, before[SPL];
    unsigned long long mine = ~0ull;   // R's best candidate among this lane's records
#pragma unroll
    for (int e = 0; e < SPL; e++) {
      p[e] = ids[lane + 64 * e];
      k[e] = keys[lane + 64 * e];
      const unsigned long long bal = __ballot(p[e] != 0xFFFFFFFFu);
      before[e] = n + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      n += (uint32_t)__popcll(bal);
      if (p[e] != 0xFFFFFFFFu) mine = min(mine, ((unsigned long long)k[e] << 32) | p[e]);
    }
    if (n) {   // (wavefront-uniform)
      uint32_t g0 = 0;
      if (lane == 0) {
        g0 = atomicAdd(&eo.segcount[seg], n);
        if (g0 + n > eo.seglimit) {
          atomicSub(&eo.segcount[seg], n);
          *eo.overflow = 1;
          g0 = 0xFFFFFFFFu;
        }
      }
      g0 = __shfl(g0, 0, 64);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor((long long)mine, o, 64));
      if (lane == 0 && mine < best[R]) atomicMin(&best[R], mine);   // (R is open: a basin of raised cells)
#pragma unroll
      for (int e = 0; e < SPL; e++) {
        if (p[e] == 0xFFFFFFFFu) continue;
        const uint32_t lo = min(R, p[e]), hi = max(R, p[e]);
        const unsigned long long c = ((unsigned long long)k[e] << 32) | R;
        if (!(p[e] & CLOSED) && c < best[p[e]]) atomicMin(&best[p[e]], c);
        if (g0 != 0xFFFFFFFFu) {
          const size_t i = (size_t)seg * eo.segcap + g0 + before[e];
          eo.a[i] = lo; eo.b[i] = hi; eo.k[i] = k[e];
        }
      }
    }
  }
}

// tiles the last plain fill of this thread wrote without reading them (RDGPU_FILL_COUNT_FLOODED=1; else 0): the finalize's
// counter, copied to pinned memory behind the kernel and read once its stream got there
static thread_local unsigned long long *g_fl_pinned = nullptr;
static thread_local unsigned long long g_fl_count = 0;
static thread_local bool g_fl_pending = false;
static thread_local hipStream_t g_fl_stream = nullptr;
// tiles the coarse flood flagged in the last plain fill of this thread (RDGPU_FILL_COUNT_COARSE=1; else 0): k_flag_tiles'
// counter, brought home the same way
static thread_local unsigned long long *g_co_pinned = nullptr;
static thread_local unsigned long long g_co_count = 0;
static thread_local bool g_co_pending = false;
static thread_local hipStream_t g_co_stream = nullptr;
static thread_local int g_coarse_depth = 0;   // inside the coarse fill of a fill: that one runs no coarse fill of its own
// Descent tiles from which the coarse flood runs when RDGPU_FILL_COARSE is not set (=1: at any size, =0: never).  Below,
// the coarse fill's two host round trips and 28 small launches cost more than the pair pass saves, on the side lane too
// (r14; there the node resolve is too short to hide them): G(3) switched off against forced on, two alternating runs each,
//    4096^2   (4 096 tiles) 0.37 / 0.37 against 0.61 / 0.59 ms      8192^2  (16 384) 0.81 / 0.82 against 1.02 / 1.02
//   16384^2  (65 536)       2.52 / 2.52 against 2.61 / 2.61        32768^2 (262 144) 9.00 / 8.96 against 8.88 / 8.85
// (r13, on the caller's stream: 2.53 against 2.68 and 8.97 against 8.98.)  DESIGN 3a; profiles/fill_coarse_lane_ab.json.
constexpr uint32_t COARSE_MIN_TILES = 262144;
// Work on a side lane must not outlive the call that forked it: the workspace is the next call's.  While `stream` is set
// (from the fork until the caller's stream waits for the join) leaving the scope waits for the lane.
struct LaneGuard {
  hipStream_t stream = nullptr;
  LaneGuard() = default;
  LaneGuard(const LaneGuard &) = delete;
  LaneGuard &operator=(const LaneGuard &) = delete;
  ~LaneGuard() {
    if (stream) (void)hipStreamSynchronize(stream);
  }
};

// f(std::true_type()) or f(std::false_type()): a runtime flag becomes a template argument of the launches in f
template <class F>
static void with_flag(bool b, F &&f) {
  if (b) f(std::true_type());
  else f(std::false_type());
}

template <class T>
static void fill_finalize16(T *d_z, int w, int h, const FillBuffers &fb, hipStream_t s) {
  if (fb.trivial) return;
  const uint32_t dtx = cdiv(w, DW), dnt = dtx * cdiv(h, DH);
  const dim3 ngrid(cdiv(std::max(fb.nnmax, 1u), NTHR), fb.nstripes);
  RD_LAUNCH("fill.node_levels", k_node_levels, ngrid, dim3(NTHR), 0, s, (const uint32_t *)fb.curN, (const uint32_t *)fb.acc,
            (const unsigned long long *)fb.counters, fb.rcap, fb.lvl);
  const bool vec = (w % 4) == 0 && (reinterpret_cast<uintptr_t>(d_z) % (4 * sizeof(T))) == 0;
  with_flag(vec, [&](auto V) {
    RD_LAUNCH("fill.finalize", (k_finalize16<T, V>), dim3(xcd_grid(dnt)), dim3(NTHR), 0, s, d_z, (const uint16_t *)fb.lab16,
              (const uint32_t *)fb.lvl, (const uint32_t *)fb.tile_base, (const uint32_t *)fb.tile_count, w, h, dtx, dnt,
              (const uint8_t *)nullptr, (const uint32_t *)nullptr);
  });
}

// The compact-label fill's host side.  false: the DEM does not fit the scheme's buffers (more nodes or pair records than
// provided for: e.g. white noise), a hook chain was left unfinished, or RDGPU_FILL_EDGES=0 asks for the raster rounds --
// the DEM has not been changed, the classic path runs.
// lists (optional, with skip): device arrays [descent tiles to visit | scan tiles to visit | tiles to finalize], each of
// `stride` entries, and their lengths on the host
// resident blocks of the persistent pair pass: what the kernel's registers and LDS let a CU hold (asked of the runtime),
// times the CUs, rounded to a multiple of 8 so that every XCD gets the same number.
// At most PAIRS_BPC per CU: the runtime answers 8 for a 256-thread block of 81 - 96 SGPRs, a CU admits
// floor(800 / (ceil(sgpr / 16) * 16 + 16)) = 7 of them.  The tiles are dealt out over the grid beforehand, so an eighth block
// would wait for a resident one to finish and then walk its share alone.
constexpr int PAIRS_BPC = 7;
template <class K>
static int pairs_blocks(K kernel) {
  int dev = 0, cus = 0, bpc = 0;
  RD_HIP(hipGetDevice(&dev));
  RD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  RD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, NTHR, 0));
  bpc = std::min(bpc, PAIRS_BPC);
  return std::max(8, (cus * std::max(bpc, 1)) / 8 * 8);
}

// Grid of the first list round (k_edge_round<true>): a block takes the chunks blk, blk + grid, ... of NTHR * EPT records, and
// a segment is `cps` chunks of which only the first few hold records.  How evenly the blocks share those is decided by
// grid mod cps: at 8192 blocks and 34 chunks per segment (1792 segments at S3) the remainder 32 gives four filled chunks to
// 40 % of the blocks and none to 35 %.  The remainder nearest to the golden section of cps (and coprime to it) spreads every
// block's chunks over the segment: 522 -> 511 us there (the rest of what the kernel lost against 1536 segments of 40
// chunks, 475 us, is the larger number of partly filled chunks: 14 336 against 13 824).
static uint32_t seg_round_grid(uint32_t maxg, uint32_t nchunks, uint32_t cps) {
  if (nchunks <= maxg || cps < 3 || cps >= maxg) return std::min(maxg, nchunks);
  uint32_t step = (uint32_t)(cps * 0.6180339887 + 0.5);
  while (std::gcd(step, cps) != 1) step++;
  step %= cps;
  const uint32_t g = maxg - maxg % cps + step;
  return g > maxg ? g - cps : g;
}

struct SparseLists {
  const uint32_t *d = nullptr;
  uint32_t stride = 0, n[3] = {0, 0, 0};
};
// keep (with alloc): the call is a row-block shard's local phase -- open_top / open_bottom name its cut rows, the tables the
// shard needs later (labels, node tables, basins' components and levels, terminal ids) come from `alloc` and are handed
// over in *keep, and the DEM is NOT raised (rdgpu_fill_shard_finish does that, after the levels of the cut-row
// terminals are known).
template <class T, int TOPO>
static bool fill_fused(T *d_z, int w, int h, hipStream_t s, const uint8_t *outlet = nullptr, const uint8_t *skip = nullptr,
                       const SparseLists *lists = nullptr, FillBuffers *keep = nullptr, BufAlloc *alloc = nullptr,
                       int open_top = 0, int open_bottom = 0) {
  if (g_coarse_depth == 0) {
    g_fl_pending = false;
    g_fl_count = 0;
    g_co_pending = false;
    g_co_count = 0;
  }
  const char *env_edges = getenv("RDGPU_FILL_EDGES");
  if (env_edges && env_edges[0] == '0') return false;   // (the raster-round fallback lives in the classic path)
  const uint64_t n64 = (uint64_t)w * (uint64_t)h;
  if (n64 > 0x7FFF0000ull) throw Error(RDGPU_ERR_ARG, "rdgpu_fill: raster (or shard) has more than 2^31-65536 cells");
  const uint32_t n = (uint32_t)n64;
  if (w <= 2 || h <= 2) return false;   // every cell is a border cell: the classic path's trivial case
  g_stats = rdgpu_fill_stats{n64, 0, 0, 0, 0, (uint32_t)(TW * TH), 0};
  Workspace &ws = Workspace::get();
  uint32_t *hw = ws.host_words();
  const uint32_t dtx = cdiv(w, DW), dty = cdiv(h, DH), dnt = dtx * dty;
  const uint32_t tilesX = cdiv(w, TW), tilesY = cdiv(h, TH), ntiles = tilesX * tilesY;
  const bool vec = (w % 4) == 0 && (reinterpret_cast<uintptr_t>(d_z) % (4 * sizeof(T))) == 0;
  FusedBuf fo;
  fo.gcap = n / 4 + 4096;
  uint32_t nstripes = 1;   // every stripe's region holds at least two tiles of nothing but roots
  while (nstripes < (uint32_t)FSTRIPES && fo.gcap / (2 * nstripes) >= 8192u && dnt >= 8 * nstripes) nstripes *= 2;
  fo.rcap = fo.gcap / nstripes;
  fo.smask = nstripes - 1;
  const bool sharded = keep != nullptr;
  if (sharded && !(open_top || open_bottom)) return false;   // (a block without a cut is the whole raster: the caller's other path)
  // what outlives the call in a shard comes from the shard's allocator
  auto persistent = [&](const char *name, size_t bytes) -> void * {
    return sharded ? (void *)alloc->get<uint8_t>(name, bytes) : ws.buf(name, bytes);
  };
  fo.lab16 = (uint16_t *)persistent("fused.lab16", (size_t)n * 2);
  fo.G = (uint32_t *)persistent("fused.G", (size_t)fo.gcap * 4);
  fo.tile_base = (uint32_t *)persistent("fused.tile_base", (size_t)dnt * 4);
  fo.tile_count = (uint32_t *)persistent("fused.tile_count", (size_t)dnt * 4);
  // [0] chase flag, [2] roots, [3] alive tiles, [4] records, [5] overflow, [8] basins, [9] nodes, [10] nodes of the fullest stripe
  uint32_t *dflags = ws.buf<uint32_t>("fused.flags", 16);
  fo.counters = (unsigned long long *)persistent("fused.counters", (size_t)FSTRIPES * FSTRIDE * 8);
  uint32_t *pitoff = ws.buf<uint32_t>("fused.pitoff", FSTRIPES);
  fo.overflow = dflags + 5;
  uint32_t *curN = (uint32_t *)persistent("fused.curN", (size_t)fo.gcap * 4);
  if (!outlet) {   // (with outlets, tiles are skipped: their records would be stale)
    fo.edgeK = ws.buf<uint32_t>("fused.edgeK", (size_t)dnt * 2 * DH);
    fo.edgeS = ws.buf<uint16_t>("fused.edgeS", (size_t)dnt * 2 * DH);
    fo.edgeR = ws.buf<uint16_t>("fused.edgeR", (size_t)dnt * 2 * DW);
  }
  RD_HIP(hipMemsetAsync(dflags, 0, 16 * sizeof(uint32_t), s));
  RD_HIP(hipMemsetAsync(fo.counters, 0, (size_t)FSTRIPES * FSTRIDE * sizeof(unsigned long long), s));
  if (outlet) {   // node 0 (the first of stripe 0): the "outside" node of the skipped tiles
    static const uint32_t one = 1u, outp = OUTP;
    RD_HIP(hipMemcpyAsync(reinterpret_cast<uint32_t *>(fo.counters) + 1, &one, sizeof(uint32_t), hipMemcpyHostToDevice, s));
    RD_HIP(hipMemcpyAsync(fo.G, &outp, sizeof(uint32_t), hipMemcpyHostToDevice, s));
  }
  const bool listed = outlet && skip && lists && lists->d;
  const uint32_t *dl = listed ? lists->d : nullptr, *sl_ = listed ? lists->d + lists->stride : nullptr,
                 *fl = listed ? lists->d + 2 * (size_t)lists->stride : nullptr;
  if (listed && lists->n[0] == 0) return true;   // nothing but walls anywhere: nothing to raise
  // RDGPU_FILL_DISSOLVE=0: every pit of the descent forest stays a basin (the plain fill; shards and outlets never dissolve)
  const char *env_dis = getenv("RDGPU_FILL_DISSOLVE");
  const int dissolve = (!outlet && !sharded && !(env_dis && env_dis[0] == '0')) ? 1 : 0;
  // RDGPU_FILL_FLOODED=0: the finalize reads every tile (the plain fill; shards and outlets always do).  Else the descent
  // leaves every tile's largest key and the finalize writes the tiles wholly under one lake without reading them.
  const char *env_fl = getenv("RDGPU_FILL_FLOODED"), *env_flc = getenv("RDGPU_FILL_COUNT_FLOODED");
  uint32_t *tile_max = nullptr;
  if (!outlet && !sharded && !(env_fl && env_fl[0] == '0')) tile_max = ws.buf<uint32_t>("fused.tile_max", dnt);
  // RDGPU_FILL_COUNT_FLOODED=1: the finalize counts those tiles (rdgpu_fill_flooded_tiles; else no atomics on the path)
  unsigned long long *flooded = nullptr;
  if (!outlet && !sharded && env_flc && env_flc[0] == '1' && g_coarse_depth == 0) {
    flooded = ws.buf<unsigned long long>("fused.flooded", 1);
    RD_HIP(hipMemsetAsync(flooded, 0, sizeof(unsigned long long), s));
  }
  // RDGPU_FILL_COARSE (the plain fill with tile_max only; =0 off, =1 on at any size, unset: from COARSE_MIN_TILES descent
  // tiles): the descent leaves the minima of the COARSE_CB x COARSE_CB blocks, their fill flags the tiles the pair pass skips
  const uint32_t cbx = cdiv(w, COARSE_CB), cby = cdiv(h, COARSE_CB);
  const char *env_co = getenv("RDGPU_FILL_COARSE");
  uint32_t *coarse = nullptr;
  if (tile_max && g_coarse_depth == 0 && cbx > 2 && cby > 2 && !(env_co && env_co[0] == '0') &&
      ((env_co && env_co[0] == '1') || dnt >= COARSE_MIN_TILES))
    coarse = ws.buf<uint32_t>("fused.coarse", (size_t)cbx * cby);
  // (outlets never come with a cut; the kernel reads outlet, skip and dl only with OUTLETS, the cut rows only with CUT)
  with_flag(vec, [&](auto V) {
    auto descent = [&](auto OUTLETS, auto CUT, auto COARSE) {
      RD_LAUNCH("fill.descent", (k_descent16<T, TOPO, V, OUTLETS, CUT, COARSE>), dim3(listed ? lists->n[0] : xcd_grid(dnt)), dim3(NTHR), 0, s,
                (const T *)d_z, fo, w, h, dtx, dnt, outlet, skip, dl, open_top, open_bottom, dissolve, tile_max, coarse, cbx, cby);
    };
    if (outlet) descent(std::true_type(), std::false_type(), std::false_type());
    else if (sharded) descent(std::false_type(), std::true_type(), std::false_type());
    else if (coarse) descent(std::false_type(), std::false_type(), std::true_type());
    else descent(std::false_type(), std::false_type(), std::false_type());
  });
  RD_LAUNCH("fill.stripe_offsets", k_stripe_offsets, dim3(1), dim3(64), 0, s, (const unsigned long long *)fo.counters, nstripes, pitoff,
            dflags + 8, dflags + 6);
  RD_HIP(hipMemcpyAsync(hw, dflags + 4, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  g_stats.host_syncs++;
  // more nodes than a stripe's table holds: nothing was written to the DEM.  The dissolved pits of a stripe count as the
  // nodes they would have been (hw[2]), so which rasters take the compact path does not depend on the rule: a raster of
  // nothing but such pits (a D4 checkerboard: every second cell) would fit with it and overflow without.
  if (hw[1] != 0 || hw[2] > fo.rcap) { if (getenv("RDGPU_FILL_DEBUG")) fprintf(stderr, "fill_fused: node table overflow (nstripes %u rcap %u)\n", nstripes, fo.rcap); return false; }
  const uint32_t B = hw[4], NNmax = hw[6];   // basins (rows of the tables); nodes of the fullest stripe
  const uint32_t ndis = hw[7];               // pits the descent dissolved: no basins, each raised to its neighbour's key at least
  g_stats.basins = (uint64_t)B + ndis;       // (the pits of the descent forest, as ever)
  g_stats.dissolved_pits = ndis;
  if (sharded) {
    *keep = FillBuffers();
    keep->B = B;
    if (B == 0) { keep->trivial = true; return true; }   // no pits and no terminals: nothing to raise
  }
  if (B == 0 && ndis == 0) return true;        // no pits: nothing to raise
  const dim3 ngrid(cdiv(std::max(NNmax, 1u), NTHR), nstripes);
  auto finalize = [&](const uint32_t *curN_, const uint32_t *acc_) {
    // (no table of node levels on this path: the finalize takes a tile's levels from curN and acc as it stages them)
    with_flag(vec, [&](auto V) {
      if (tile_max)
        RD_LAUNCH("fill.finalize", (k_finalize16<T, V, true>), dim3(xcd_grid(dnt)), dim3(NTHR), 0, s, d_z, (const uint16_t *)fo.lab16,
                  (const uint32_t *)nullptr, (const uint32_t *)fo.tile_base, (const uint32_t *)fo.tile_count, w, h, dtx, dnt,
                  (const uint8_t *)nullptr, (const uint32_t *)nullptr, curN_, acc_, (const uint32_t *)tile_max, flooded);
      else
        RD_LAUNCH("fill.finalize", (k_finalize16<T, V>), dim3(listed ? lists->n[2] : xcd_grid(dnt)), dim3(NTHR), 0, s, d_z,
                  (const uint16_t *)fo.lab16, (const uint32_t *)nullptr, (const uint32_t *)fo.tile_base, (const uint32_t *)fo.tile_count, w,
                  h, dtx, dnt, skip, fl, curN_, acc_);
    });
    if (flooded) {   // the count goes home behind the finalize; rdgpu_fill_flooded_tiles waits for it, the fill does not
      if (!g_fl_pinned) RD_HIP(hipHostMalloc((void **)&g_fl_pinned, sizeof(unsigned long long)));
      RD_HIP(hipMemcpyAsync(g_fl_pinned, flooded, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      g_fl_pending = true;
      g_fl_stream = s;
    }
  };
  if (B == 0) {   // nothing but dissolved pits: every node is the outside's (level 0), the pits rise to their neighbours' keys
    uint32_t *acc0 = ws.buf<uint32_t>("fill.acc", 1);
    RD_HIP(hipMemsetAsync(acc0, 0, sizeof(uint32_t), s));
    RD_LAUNCH("fill.resolve_nodes", k_resolve_nodes, ngrid, dim3(NTHR), 0, s, fo.G, (const unsigned long long *)fo.counters,
              (const uint32_t *)pitoff, fo.rcap, (const uint16_t *)fo.lab16, (const uint32_t *)fo.tile_base, w, dtx, B, curN, dflags,
              (const uint32_t *)nullptr, (const uint16_t *)fo.edgeS, (const uint16_t *)fo.edgeR);
    g_stats.jump_passes = 1;
    finalize(curN, acc0);
    return true;
  }
  uint32_t *tid = nullptr;
  if (sharded) {
    tid = alloc->get<uint32_t>("fill.tid", (size_t)B + 1);
    RD_HIP(hipMemsetAsync(tid, 0xFF, ((size_t)B + 1) * sizeof(uint32_t), s));
    RD_LAUNCH("fill.mark_terminals", k_mark_terminals16, dim3(cdiv(w, NTHR)), dim3(NTHR), 0, s, (const uint16_t *)fo.lab16,
              (const uint32_t *)fo.tile_base, (const uint32_t *)fo.G, (const uint32_t *)pitoff, fo.rcap, tid, w, h, dtx, open_top,
              open_bottom);
  }
  // r14: the coarse flood runs on a side lane of the workspace, beside k_resolve_nodes and k_init_tables.  It
  // needs nothing but the descent's block minima and tile_max, complete since the synchronisation above; the fork is
  // recorded on the idle stream BEFORE the two kernels are enqueued, so the lane does not wait for them.
  // RDGPU_FILL_COARSE_LANE=0: on the caller's stream behind them, as r13 had it.
  const char *env_lane = getenv("RDGPU_FILL_COARSE_LANE");
  Workspace::SideLane *lane = coarse && !(env_lane && env_lane[0] == '0') ? &ws.side_lane(0) : nullptr;
  LaneGuard lane_open;
  if (lane) {
    RD_HIP(hipEventRecord(lane->fork, s));
    RD_HIP(hipStreamWaitEvent(lane->stream, lane->fork, 0));
    lane_open.stream = lane->stream;
  }
  const hipStream_t cs = lane ? lane->stream : s;   // the coarse flood's stream
  RD_LAUNCH("fill.resolve_nodes", k_resolve_nodes, ngrid, dim3(NTHR), 0, s, fo.G, (const unsigned long long *)fo.counters,
            (const uint32_t *)pitoff, fo.rcap, (const uint16_t *)fo.lab16, (const uint32_t *)fo.tile_base, w, dtx, B, curN, dflags,
            (const uint32_t *)tid, (const uint16_t *)fo.edgeS, (const uint16_t *)fo.edgeR);
  g_stats.jump_passes = 1;
  uint32_t *cur = sharded ? alloc->get<uint32_t>("fill.cur", (size_t)B + 1) : ws.buf<uint32_t>("fill.cur", (size_t)B + 1);
  uint32_t *acc = sharded ? alloc->get<uint32_t>("fill.acc", (size_t)B + 1) : ws.buf<uint32_t>("fill.acc", (size_t)B + 1);
  unsigned long long *best = ws.buf<unsigned long long>("fill.best", (size_t)B + 1);
  unsigned long long *link = ws.buf<unsigned long long>("fill.link", (size_t)B + 1);
  uint32_t *rootsA = ws.buf<uint32_t>("fill.rootsA", B);
  uint32_t *rootsB = ws.buf<uint32_t>("fill.rootsB", B);
  RD_HIP(hipMemsetAsync(dflags + 2, 0, sizeof(uint32_t), s));
  RD_LAUNCH("fill.init_tables", k_init_tables, dim3(cdiv((uint64_t)B + 1, NTHR)), dim3(NTHR), 0, s, cur, acc, link, rootsA,
            dflags + 2, (const uint32_t *)tid, B);
  // ---- the coarse flood: the fill of the block minima, in place, by this very function (its buffers and profile entries
  // under "coarse."; it reads the pinned words, whose values this call holds in locals by now).  k_resolve_nodes and
  // k_init_tables are in the caller's stream already; on the lane (cs != s) its kernels run beside them, its two
  // synchronisations wait for the lane alone, and the caller's stream waits for the lane's join before anything else is
  // enqueued on it: whatever follows, every early return included, is ordered behind the lane.  (An exception between the
  // fork and that wait -- the nested fill's as well -- waits for the lane as it unwinds: lane_open.)  Its synchronisations
  // are this fill's.
  uint8_t *tflag = nullptr;
  if (coarse) {
    const rdgpu_fill_stats outer = g_stats;
    bool ok = false;
    g_coarse_depth++;
    try {
      NameScope scope("coarse.");
      ok = fill_fused<uint32_t, TOPO>(coarse, (int)cbx, (int)cby, cs);
    } catch (...) {
      g_coarse_depth--;
      g_stats = outer;
      throw;
    }
    g_coarse_depth--;
    const uint32_t syncs = g_stats.host_syncs;
    g_stats = outer;
    g_stats.host_syncs += syncs;
    unsigned long long *ccount = nullptr;
    if (ok) {   // (else: the coarse raster does not fit the compact path -- nothing is flagged, the fill goes on as ever)
      tflag = ws.buf<uint8_t>("fused.tile_flag", dnt);
      const char *env_coc = getenv("RDGPU_FILL_COUNT_COARSE");
      if (env_coc && env_coc[0] == '1') {
        ccount = ws.buf<unsigned long long>("fused.coarse_count", 1);
        RD_HIP(hipMemsetAsync(ccount, 0, sizeof(unsigned long long), cs));
      }
      RD_LAUNCH("fill.flag_tiles", k_flag_tiles, dim3(cdiv(dnt, NTHR)), dim3(NTHR), 0, cs, (const uint32_t *)tile_max,
                (const uint32_t *)coarse, dtx, dnt, cbx, tflag, ccount);
    }
    if (lane) {
      RD_HIP(hipEventRecord(lane->join, cs));
      RD_HIP(hipStreamWaitEvent(s, lane->join, 0));
      lane_open.stream = nullptr;
    }
    if (ccount) {
      if (!g_co_pinned) RD_HIP(hipHostMalloc((void **)&g_co_pinned, sizeof(unsigned long long)));
      RD_HIP(hipMemcpyAsync(g_co_pinned, ccount, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      g_co_pending = true;
      g_co_stream = s;
    }
  }
  uint32_t nroots0 = B;
  if (sharded) {   // the frozen terminals are no roots: the list was compacted, its length comes back
    RD_HIP(hipMemcpyAsync(hw, dflags + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    g_stats.host_syncs++;
    nroots0 = hw[0];
  }
  const uint32_t nwork1 = listed ? lists->n[1] : ntiles;   // scan tiles the pair pass visits
  static thread_local int pb_cache[2] = {0, 0};   // (per element type and topology: this function is a template)
  int &pb = pb_cache[vec ? 1 : 0];
  if (!pb) pb = vec ? pairs_blocks(k_pairs16<T, TOPO, true>) : pairs_blocks(k_pairs16<T, TOPO, false>);
  const uint32_t pgrid = std::max(8u, std::min<uint32_t>(xcd_grid(std::max(nwork1, 1u)), (uint32_t)pb));
  // the pair list of the one raster pass: capacity as in the classic path, one segment per block of the pair pass, and
  // behind them those of k_pairs_flooded (a flagged tile leaves ~40 records, three tiles in ten are flagged at S3: 512
  // segments fill about as far as the pair pass's 1 792)
  const uint32_t fseg = tflag ? std::max(1u, std::min(512u, cdiv(dnt, 64u))) : 0u;
  const uint32_t nseg = pgrid + fseg;
  const char *env_cap = getenv("RDGPU_FILL_EDGE_CAP");
  const uint64_t cap = env_cap ? strtoull(env_cap, nullptr, 10) : std::min<uint64_t>(12ull * B, n / 2) + 2048;
  const uint32_t segcap = cdiv(cdiv(cap, nseg), NTHR * EPT) * (NTHR * EPT);
  const size_t ecap = (size_t)nseg * segcap;
  uint32_t *elist[2] = {ws.buf<uint32_t>("fill.edges0", 3 * ecap), nullptr};
  size_t pcap[2] = {ecap, 0};
  uint32_t *segcount = ws.buf<uint32_t>("fill.segcount", nseg);
  RD_HIP(hipMemsetAsync(segcount, 0, nseg * sizeof(uint32_t), s));
  EdgeOut eo{elist[0], elist[0] + ecap, elist[0] + 2 * ecap, segcount, segcap, nseg - 1, dflags + 5};
  eo.seglimit = env_cap ? (uint32_t)std::min<uint64_t>(segcap, std::max<uint64_t>(1, cdiv(cap, nseg))) : segcap;   // (the cap given on purpose is enforced to the record: the overflow tests)
  int ein = 0;
  bool eseg = true;
  // What the parts of the pair pass cost, r05 at S3 (profiles/r05e_*, measured by switching its phases off): staging +
  // detection 2.5 ms, list 0.4, gathers 0.45, sorting the neighbours 1.0, table 1.8, proposals + records 0.5 = 6.1.
  // Built on that and measured SLOWER or equal, not kept: the pair pass on local component ids with a direct triangular pair
  // table (9.5 ms: its LDS atomics and the id lookups cost more than the hash they replace), one table trip per cell with
  // the cells of a second component on a wavefront's own list (6.1-6.2), a two-slot fast path (6.2).
  // r06: the rounds are enqueued WITHOUT a host read-back between them.  Every round kernel takes its counts from the device
  // (rc[4 r] = live roots entering round r, rc[4 r + 1] = records of the list it contracts) and runs a grid-stride loop over
  // a grid the host sizes from upper bounds: live roots at least halve per round (every one hooks into another component or
  // the outside), the record list never grows.  After a batch of rounds -- as many as the halving bound and the measured
  // shrink (a factor 4 - 9 per round) make plausible -- ONE synchronisation reads every round's counts and the error flags;
  // only a fill that is not finished by then (never seen) enqueues more.  A fill has two synchronisations: after the
  // descent (the basin count sizes the tables) and here.  (r05: one per round, 10 per fill at S3 -- on a busy host each is a
  // scheduling quantum, profiles/README.md r05u.)
  constexpr int MAXR = 48;
  uint32_t *rc = ws.buf<uint32_t>("fused.round_counts", 4 * (MAXR + 2));
  RD_HIP(hipMemsetAsync(rc, 0, 4 * (MAXR + 2) * sizeof(uint32_t), s));
  hw[220] = nroots0;   // (pinned; beyond the words the read-backs use)
  RD_HIP(hipMemcpyAsync(rc + 4, hw + 220, sizeof(uint32_t), hipMemcpyHostToDevice, s));
  pcap[1] = ecap;   // (the second list is sized for whatever the first pass may leave: its count stays on the device)
  elist[1] = ws.buf<uint32_t>("fill.edges1", 3 * pcap[1]);
  const uint32_t gcap = 2048;   // blocks of a grid-stride launch: 8 per CU
  int rdone = 0;                // rounds enqueued so far
  uint32_t rounds_run = 0;
  // r07: cur[] is kept for the round's roots only (k_compact_roots) and the basins are settled once after the rounds
  // (k_settle_basins) -- k_update_basins rewrote all B entries of cur[] and acc[] in every enqueued round, 11 gather passes
  // over 1e7 basins at S3 where one does.  And the small rounds are ONE launch: a round whose live roots and records are
  // under the thresholds is k_rounds_tail's, with every round after it; the full-width kernels enqueued for it return at once.
  uint32_t troots = TAIL_ROOTS;
  if (const char *env_tail = getenv("RDGPU_FILL_TAIL_ROOTS")) troots = (uint32_t)std::min<unsigned long long>(strtoull(env_tail, nullptr, 10), 0xFFFFFFFFull);
  const uint32_t trecs = (uint32_t)std::min<unsigned long long>((unsigned long long)troots * TAIL_RECS_PER_ROOT, 0xFFFFFFFFull);
  uint32_t *const rootsP[2] = {rootsA, rootsB};   // round r reads rootsP[(r - 1) & 1] and leaves its survivors in the other
  auto enqueue_tail = [&](int rlo, int rhi, int rmax) {
    TailArgs ta;
    ta.roots[0] = rootsP[0]; ta.roots[1] = rootsP[1];
    ta.el[0] = elist[0]; ta.el[1] = elist[1];
    ta.pcap = ecap; ta.segcount = segcount; ta.segcap = segcap;
    ta.cur = cur; ta.best = best; ta.link = link; ta.B = B; ta.rc = rc; ta.flag = dflags;
    ta.troots = troots; ta.trecs = trecs;
    ta.rlo = std::max(2, rlo); ta.rhi = rhi; ta.rmax = rmax; ta.maxhops = 1 << 14;
    RD_LAUNCH("fill.rounds_tail", k_rounds_tail, dim3(1), dim3(TAILT), 0, s, ta);
  };
  auto enqueue_round = [&](int r) {   // r = 1, 2, ...
    uint32_t *rootsA = rootsP[(r - 1) & 1], *rootsB = rootsP[r & 1];
    TailGate gate;
    if (troots && r >= 2) { gate.cnt = rc + 4 * r; gate.roots = troots; gate.recs = trecs; }
    const uint32_t bound = std::max(1u, r - 1 < 31 ? nroots0 >> (r - 1) : 1u);   // live roots at most halve... at least
    const uint32_t rgrid = std::min(gcap, cdiv(bound, NTHR));
    const uint32_t *nr = rc + 4 * r, *ne = rc + 4 * r + 1;
    uint32_t *nr_next = rc + 4 * (r + 1), *ne_next = rc + 4 * (r + 1) + 1;
    RD_LAUNCH("fill.best_reset", k_best_reset, dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)rootsA, 0u, best, nr, gate);
    if (r == 1) {   // round 1: the one raster pass (components gathered from the node table)
      const uint32_t nwork = listed ? lists->n[1] : ntiles;
      const uint8_t *pskip = tflag ? tflag : skip;   // (tflag: the plain fill, which has no skip of its own)
#ifdef RDGPU_PROBES
      if (!outlet && !sharded && g_probe_pairs_skip) pskip = g_probe_pairs_skip;
#endif
      if (nwork > 0)   // (none although basins exist cannot happen -- a pit is a wet cell; kept safe)
        with_flag(vec, [&](auto V) {
          RD_LAUNCH("fill.scan", (k_pairs16<T, TOPO, V>), dim3(pgrid), dim3(NTHR), 0, s, (const T *)d_z, (const uint16_t *)fo.lab16,
                    (const uint32_t *)curN, best, w, h, B, tilesX, sl_, nwork, eo, (const uint32_t *)fo.tile_base,
                    (const uint32_t *)fo.tile_count, dtx, pskip, (const uint32_t *)fo.edgeK, (const uint16_t *)fo.edgeS);
        });
      if (tflag)
        RD_LAUNCH("fill.pairs_flooded", (k_pairs_flooded<T, TOPO>), dim3(cdiv(dnt, NTHR / 64)), dim3(NTHR), 0, s, (const T *)d_z,
                  (const uint16_t *)fo.lab16, (const uint32_t *)curN, best, w, dtx, dnt, (const uint8_t *)tflag,
                  (const uint32_t *)tile_max, (const uint32_t *)fo.tile_base, (const uint32_t *)fo.tile_count,
                  (const uint32_t *)fo.edgeK, (const uint16_t *)fo.edgeS, eo, pgrid, fseg);
      RD_LAUNCH("fill.sum_segments", k_sum_segments, dim3(1), dim3(NTHR), 0, s, (const uint32_t *)eo.segcount, nseg, rc + 4 * 1 + 1,
                rc + 4 * 2 + 1);   // (and where round 2's gate reads it)
      g_stats.scan_tiles += ntiles;
    } else {
      const int eout = ein ^ 1;
      const uint32_t *ia = elist[ein], *ib = elist[ein] + pcap[ein], *ik = elist[ein] + 2 * pcap[ein];
      uint32_t *oa = elist[eout], *ob = elist[eout] + pcap[eout], *ok = elist[eout] + 2 * pcap[eout];
      if (eseg)   // round 2 reads the segmented list of the raster pass: the segments' fill counts are on the device
        RD_LAUNCH("fill.edge_round", (k_edge_round<true>),
                  dim3(seg_round_grid(4 * gcap, (uint32_t)cdiv(ecap, NTHR * EPT), segcap / (NTHR * EPT))), dim3(NTHR), 0,
                  s, ia, ib, ik, (uint32_t)ecap, (const uint32_t *)segcount, segcap, (const uint32_t *)cur, best, B, oa, ob, ok, ne_next,
                  (const uint32_t *)nullptr, gate);
      else
        RD_LAUNCH("fill.edge_round", (k_edge_round<false>), dim3(gcap), dim3(NTHR), 0, s, ia, ib, ik, 0u,
                  (const uint32_t *)nullptr, 0u, (const uint32_t *)cur, best, B, oa, ob, ok, ne_next, ne, gate);
      eseg = false;
      ein = eout;
    }
    RD_LAUNCH("fill.hook", k_hook, dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)rootsA, 0u, (const unsigned long long *)best, link, nr,
              gate);
    // One pass: a thread follows its chain of hooks for up to 16384 steps (the chains of a round are a handful of hooks
    // long).  "A chain was left unfinished" stays in dflags[0] for the read-back after the batch and sends the raster to
    // the classic path, whose loop repeats the pass: nothing has been written to the DEM yet.
    RD_LAUNCH("fill.chase_links", k_chase_links, dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)rootsA, 0u, link, 1 << 14, dflags,
              nr, gate);
    RD_LAUNCH("fill.compact_roots", k_compact_roots, dim3(std::min(gcap, cdiv(bound, NTHR * RPT))), dim3(NTHR), 0, s,
              (const uint32_t *)rootsA, 0u, (const unsigned long long *)link, rootsB, nr_next, nr, cur, gate);
  };
  // round 1 writes the records' total where round 2 expects it
  // (k_sum_segments above: rc[4 * 1 + 1] is unused by round 1 itself; round 2 reads the segmented list and needs no count)
  uint32_t *hrc = ws.host_words() + 16;   // (pinned: the counts of every round, read once per batch)
  {
    uint32_t lg = 0;
    while ((1ull << lg) < (unsigned long long)nroots0 + 1ull) lg++;
    int batch = std::min(MAXR, std::max(4, (int)(2 * lg + 4) / 5 + 1));   // ~log5.7(roots) + 1: S3 enqueues 11, runs 9
    if (troots) {
      // full-width rounds up to the first whose roots are under the threshold if they shrink by 4 a round (measured: 4 - 9),
      // that one included as a margin; the tail kernel takes over wherever the counts on the device say, or not at all --
      // then the fill is not finished after the batch and enqueues more, as before
      int r4 = 2;
      while (r4 < batch && (2 * (r4 - 1) < 32 ? nroots0 >> (2 * (r4 - 1)) : 0u) > troots) r4++;
      batch = std::min(batch, r4);
    }
    const char *env_batch = getenv("RDGPU_FILL_ROUND_BATCH");
    if (env_batch) batch = std::min(MAXR, std::max(1, atoi(env_batch)));   // (tests: several batches)
    uint32_t last_live = 0xFFFFFFFFu;
    for (;;) {
      const int rfirst = rdone + 1;
      for (int k = 0; k < batch && rdone < MAXR; k++) enqueue_round(++rdone);
      // (with RDGPU_FILL_ROUND_BATCH a batch stays a batch: the tail kernel runs the rounds enqueued for it and no more)
      if (troots) enqueue_tail(rfirst, env_batch ? rdone : std::min(rdone + 1, MAXR), env_batch ? rdone : MAXR);
      RD_HIP(hipMemcpyAsync(hrc, rc, 4 * (MAXR + 2) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      RD_HIP(hipMemcpyAsync(hw, dflags, 14 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      RD_HIP(hipStreamSynchronize(s));
      g_stats.host_syncs++;
      if (getenv("RDGPU_FILL_DEBUG")) fprintf(stderr, "fill_fused: pair pass: %u records, overflow %u, %u tiles on the slow road; %d rounds enqueued\n", hrc[4 + 1], hw[5], hw[12], rdone);
      // Not reachable on purpose by a DEM a test can hold.  A thread of k_chase_links gives up after 16384 hops over links
      // that nobody has shortened yet, so a round needs a chain of more than 16384 basins each spilling into the next (a
      // staircase of pits: tests/test_fallback_engines_gpu.py builds one of 20 000) AND the threads behind a link must not
      // have finished first: every thread of the round runs at once and stores its own shortened link as soon as it ends,
      // so a walk from distance d meets a finished link after about sqrt(2 d) hops.  16384 hops taken alone would need a
      // chain of ~10^8 basins, or a grid whose blocks run one after the other from the chain's far end -- timing, not input.
      if (hw[0] != 0) { if (getenv("RDGPU_FILL_DEBUG")) fprintf(stderr, "fill_fused: hook chain unfinished\n"); return false; }
      if (hw[5] != 0) { if (getenv("RDGPU_FILL_DEBUG")) fprintf(stderr, "fill_fused: pair list overflow (B %u cap %llu nseg %u segcap %u nwork %u)\n", B, (unsigned long long)cap, nseg, segcap, nwork1); return false; }   // the pair list overflowed: the DEM is untouched, the classic path takes over
      if ((int)hrc[2] > rdone) rdone = std::min<int>(hrc[2], MAXR);   // (rounds the tail kernel ran past the enqueued ones)
      rounds_run = 0;
      for (int r = 1; r <= rdone; r++) rounds_run += hrc[4 * r] != 0;
      g_stats.edge_records = hrc[4 + 1];
      const uint32_t live = hrc[4 * (rdone + 1)];
      if (live == 0) break;
      if (live >= last_live || rdone >= MAXR) throw Error(RDGPU_ERR_HIP, "rdgpu_fill: contraction made no progress (internal error)");
      last_live = live;
      if (!env_batch) batch = 4;
    }
  }
  g_stats.rounds += rounds_run;
  RD_LAUNCH("fill.settle_basins", k_settle_basins, dim3(cdiv(B, NTHR)), dim3(NTHR), 0, s, cur, acc, link, B, 1 << 14, dflags);
  if (sharded) {   // the level and the watershed of every node, and everything rdgpu_fill_shard_export / _finish need
    uint32_t *lvl = fo.G;   // (the node table is dead: its storage holds the nodes' levels)
    RD_LAUNCH("fill.node_levels", k_node_levels, ngrid, dim3(NTHR), 0, s, (const uint32_t *)curN, (const uint32_t *)acc,
              (const unsigned long long *)fo.counters, fo.rcap, lvl);
    uint32_t *nodeW = alloc->get<uint32_t>("fused.nodeW", fo.gcap);
    RD_LAUNCH("fill.node_watersheds", k_node_watersheds, ngrid, dim3(NTHR), 0, s, (const uint32_t *)curN, (const uint32_t *)cur,
              (const uint32_t *)tid, (const unsigned long long *)fo.counters, fo.rcap, B, nodeW);
    keep->compact = true;
    keep->cur = cur; keep->acc = acc; keep->tid = tid;
    keep->lab16 = fo.lab16; keep->tile_base = fo.tile_base; keep->tile_count = fo.tile_count;
    keep->curN = curN; keep->lvl = lvl; keep->nodeW = nodeW; keep->counters = fo.counters;
    keep->rcap = fo.rcap; keep->nstripes = nstripes; keep->nnmax = NNmax;
    return true;
  }
  if (listed && lists->n[2] == 0) return true;
  finalize((const uint32_t *)curN, (const uint32_t *)acc);
  return true;
}

template <class T>
static void fill_device(T *d_z, int w, int h, int topology, hipStream_t s) {
  check_fill_args(d_z, w, h, topology);
  if (topology == 8 ? fill_fused<T, 8>(d_z, w, h, s) : fill_fused<T, 4>(d_z, w, h, s)) return;
  FillBuffers fb;
  BufAlloc ws_alloc{false, nullptr};
  if (topology == 8) fill_local_phase<T, 8>(d_z, w, h, 0, 0, ws_alloc, fb, s);
  else fill_local_phase<T, 4>(d_z, w, h, 0, 0, ws_alloc, fb, s);
  fill_finalize<T>(d_z, w, h, fb, s);
}

// The D8 fill with interior outlets (cells flagged in d_outlet drain like border cells).
template <class T>
static void fill_outlets_device(T *d_z, const uint8_t *d_outlet, const uint8_t *d_skip, int w, int h, hipStream_t s,
                                const SparseLists *lists = nullptr) {
  check_fill_args(d_z, w, h, 8);
  if (!d_outlet) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_outlets: null outlet mask");
  if (w <= 2 || h <= 2) return;   // every cell is a border cell
  if (fill_fused<T, 8>(d_z, w, h, s, d_outlet, d_skip, lists)) return;
  FillBuffers fb;   // (the compact labels ran out of table space: the classic path)
  BufAlloc ws_alloc{false, nullptr};
  fill_local_phase<T, 8>(d_z, w, h, 0, 0, ws_alloc, fb, s, d_outlet);
  fill_finalize<T>(d_z, w, h, fb, s);
}

template <class T>
static void fill_host(T *dem, int w, int h, int topology) {
  check_fill_args(dem, w, h, topology);
  HostStage st;
  T *d = st.inout("host.dem", dem, (size_t)w * h);
  fill_device<T>(d, w, h, topology, nullptr);
  st.finish();
}

}  // namespace rdgpu

// ------------------------------------------------------------------------------------------
// shard handle (C-ABI object)
// ------------------------------------------------------------------------------------------
struct rdgpu_fill_shard {
  int dtype = 0;   // 0 u8, 1 i16, 2 u16, 3 i32, 4 u32, 5 f32, 6 i8
  void *d_dem = nullptr;
  int w = 0, h = 0, topology = 8, open_top = 0, open_bottom = 0;
  hipStream_t stream = nullptr;
  rdgpu::FillBuffers fb;
  std::vector<void *> owned;
  bool cached = false;   // its buffers are the process-wide cached shard workspace (see shard_begin)
  int device = 0;
  uint32_t *d_edges = nullptr;
  uint32_t nedges = 0;
  rdgpu_fill_stats stats{};
};

namespace rdgpu {

template <class T>
struct DtypeCode;
template <> struct DtypeCode<uint8_t> { static constexpr int v = 0; };
template <> struct DtypeCode<int16_t> { static constexpr int v = 1; };
template <> struct DtypeCode<uint16_t> { static constexpr int v = 2; };
template <> struct DtypeCode<int32_t> { static constexpr int v = 3; };
template <> struct DtypeCode<uint32_t> { static constexpr int v = 4; };
template <> struct DtypeCode<float> { static constexpr int v = 5; };
template <> struct DtypeCode<int8_t> { static constexpr int v = 6; };

// One shard per process is the multi-GPU case (one rank, one GPU, one row block), and there a fill must not pay
// hipMalloc / hipFree of its ~5 B/cell of tables on every call: the first live shard keeps its buffers in the
// grow-only workspace (under names of their own); shards begun while it is alive own theirs (tests and tools
// drive many shards from one process).
static bool g_cached_shard_live[64] = {};   // per device: the workspace slots are per device too

static void shard_free(rdgpu_fill_shard *sh) {
  if (!sh) return;
  std::lock_guard<std::recursive_mutex> lock(api_mutex());
  for (void *p : sh->owned) (void)hipFree(p);
  if (sh->cached) {
    g_cached_shard_live[sh->device & 63] = false;
    Workspace::get().unpin();
  }
  delete sh;
}

template <class T, int TOPO>
static void shard_edges(rdgpu_fill_shard *sh) {
  const int w = sh->w, h = sh->h;
  hipStream_t s = sh->stream;
  Workspace &ws = Workspace::get();
  uint32_t *hw = ws.host_words();
  // adjacent watershed pairs form a planar graph over <= 2w terminals + the outside
  uint32_t hsize = 1024;
  while (hsize < 16u * (uint32_t)w) hsize <<= 1;
  for (;;) {
    unsigned long long *hkeys = ws.buf<unsigned long long>("shard.hkeys", hsize);
    uint32_t *hvals = ws.buf<uint32_t>("shard.hvals", hsize);
    uint32_t *ctr = ws.buf<uint32_t>("shard.ctr", 4);
    RD_HIP(hipMemsetAsync(hkeys, 0, (size_t)hsize * 8, s));
    RD_HIP(hipMemsetAsync(hvals, 0xFF, (size_t)hsize * 4, s));
    RD_HIP(hipMemsetAsync(ctr, 0, 16, s));
    const uint32_t etx = cdiv(w, EW), ent = etx * cdiv(h, EH);
    if (sh->fb.compact)
      RD_LAUNCH("shard.edges", (k_shard_edges16<T, TOPO>), dim3(xcd_grid(ent)), dim3(NTHR), 0, s, (const T *)sh->d_dem,
                (const uint16_t *)sh->fb.lab16, (const uint32_t *)sh->fb.tile_base, cdiv(w, DW), (const uint32_t *)sh->fb.nodeW,
                (const uint32_t *)sh->fb.lvl, w, h, hkeys, hvals, hsize - 1, ctr, etx, ent);
    else
      RD_LAUNCH("shard.edges", (k_shard_edges<T, TOPO>), dim3(xcd_grid(ent)), dim3(NTHR), 0, s,
                (const T *)sh->d_dem, (const uint32_t *)sh->fb.lab, (const uint32_t *)sh->fb.cur,
                (const uint32_t *)sh->fb.acc, (const uint32_t *)sh->fb.tid, sh->fb.B, w, h, hkeys, hvals, hsize - 1, ctr, etx,
                ent);
    uint32_t *edges = (uint32_t *)nullptr;
    if (sh->cached) {
      edges = ws.buf<uint32_t>("shard.edges", (size_t)hsize * 3);
    } else {
      void *p = nullptr;
      RD_HIP(hipMalloc(&p, (size_t)hsize * 12));
      sh->owned.push_back(p);
      edges = (uint32_t *)p;
    }
    RD_LAUNCH("shard.edges_compact", k_shard_edges_compact, dim3(cdiv(hsize, NTHR)), dim3(NTHR), 0, s,
              (const unsigned long long *)hkeys, (const uint32_t *)hvals, hsize, edges, ctr + 1);
    RD_HIP(hipMemcpyAsync(hw, ctr, 8, hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    if (hw[0] == 0 && hw[1] * 2 <= hsize) {
      sh->d_edges = edges;
      sh->nedges = hw[1];
      return;
    }
    if (hsize >= (1u << 28)) throw Error(RDGPU_ERR_HIP, "rdgpu_fill_shard: watershed edge table overflow");
    hsize <<= 2;   // too full (or overflowed): retry with a larger table
  }
}

template <class T>
static rdgpu_fill_shard *shard_begin(T *d_dem, int w, int h, int topology, int open_top, int open_bottom,
                                     hipStream_t s) {
  check_fill_args(d_dem, w, h, topology);
  if ((open_top || open_bottom) && h < 2) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard: a shard needs at least 2 rows");
  rdgpu_fill_shard *sh = new rdgpu_fill_shard();
  try {
    sh->dtype = DtypeCode<T>::v;
    sh->d_dem = d_dem;
    sh->w = w; sh->h = h; sh->topology = topology;
    sh->open_top = open_top ? 1 : 0; sh->open_bottom = open_bottom ? 1 : 0;
    sh->stream = s;
    RD_HIP(hipGetDevice(&sh->device));
    sh->cached = !g_cached_shard_live[sh->device & 63];
    if (sh->cached) {
      g_cached_shard_live[sh->device & 63] = true;
      Workspace::get().pin();   // (its tables live in the workspace: release_workspace() is refused while it is alive)
    }
    BufAlloc alloc{!sh->cached, &sh->owned, sh->cached};
    // the local phase on compact labels (r04: the whole-raster engine with the cut rows as frozen terminals); the classic
    // 32-bit-label phase where that does not apply (RDGPU_SHARD_FUSED=0, tiny blocks, tables that do not fit)
    const char *sf = getenv("RDGPU_SHARD_FUSED");
    bool done = false;
    if (!(sf && sf[0] == '0') && !sh->open_top && !sh->open_bottom) {
      // a block without a cut is the whole raster (one rank): the plain compact-label fill, raised at once -- nothing is
      // left for the exchange or for finish
      done = topology == 8 ? fill_fused<T, 8>(d_dem, w, h, s) : fill_fused<T, 4>(d_dem, w, h, s);
      if (done) { sh->fb = FillBuffers(); sh->fb.trivial = true; }
    } else if (!(sf && sf[0] == '0')) {
      const size_t owned_before = sh->owned.size();
      done = topology == 8 ? fill_fused<T, 8>(d_dem, w, h, s, nullptr, nullptr, nullptr, &sh->fb, &alloc, sh->open_top, sh->open_bottom)
                           : fill_fused<T, 4>(d_dem, w, h, s, nullptr, nullptr, nullptr, &sh->fb, &alloc, sh->open_top, sh->open_bottom);
      if (!done) {
        // the attempt gave up (node table or pair list too small: white noise): what it allocated for itself goes back before
        // the classic phase allocates its own tables, or the shard would hold both until shard_free; the
        // half-filled FillBuffers is reset as well
        RD_HIP(hipStreamSynchronize(s));
        for (size_t i = owned_before; i < sh->owned.size(); i++) (void)hipFree(sh->owned[i]);
        sh->owned.resize(owned_before);
        sh->fb = FillBuffers();
      }
    }
    if (!done) {
      if (topology == 8) fill_local_phase<T, 8>(d_dem, w, h, sh->open_top, sh->open_bottom, alloc, sh->fb, s);
      else fill_local_phase<T, 4>(d_dem, w, h, sh->open_top, sh->open_bottom, alloc, sh->fb, s);
    }
    sh->stats = g_stats;
    if (!sh->fb.trivial && sh->fb.tid) {
      if (topology == 8) shard_edges<T, 8>(sh);
      else shard_edges<T, 4>(sh);
    }
  } catch (...) {
    shard_free(sh);
    throw;
  }
  return sh;
}

template <class T>
static void shard_export_rows(rdgpu_fill_shard *sh, uint32_t *top_keys, uint32_t *bottom_keys) {
  const int w = sh->w, h = sh->h;
  std::vector<T> row(w);
  for (int which = 0; which < 2; which++) {
    uint32_t *out = which == 0 ? top_keys : bottom_keys;
    if (!out) continue;
    const T *src = (const T *)sh->d_dem + (which == 0 ? 0 : (size_t)(h - 1) * w);
    RD_HIP(hipMemcpyAsync(row.data(), src, (size_t)w * sizeof(T), hipMemcpyDeviceToHost, sh->stream));
    RD_HIP(hipStreamSynchronize(sh->stream));
    for (int x = 0; x < w; x++) out[x] = Key32<T>::to(row[x]);
  }
}

template <class T>
static void shard_finish(rdgpu_fill_shard *sh, const uint32_t *levels2w) {
  hipStream_t s = sh->stream;
  if (!sh->fb.trivial) {
    if (sh->fb.tid) {
      if (!levels2w) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard_finish: levels required for a shard with cut rows");
      uint32_t *dl = Workspace::get().buf<uint32_t>("shard.levels", (size_t)2 * sh->w);
      RD_HIP(hipMemcpyAsync(dl, levels2w, (size_t)2 * sh->w * 4, hipMemcpyHostToDevice, s));
      RD_LAUNCH("shard.apply", k_shard_apply, dim3(cdiv(sh->fb.B, NTHR)), dim3(NTHR), 0, s,
                (const uint32_t *)sh->fb.cur, sh->fb.acc, (const uint32_t *)sh->fb.tid, (const uint32_t *)dl, sh->fb.B);
    }
    if (sh->fb.compact) fill_finalize16<T>((T *)sh->d_dem, sh->w, sh->h, sh->fb, s);
    else fill_finalize<T>((T *)sh->d_dem, sh->w, sh->h, sh->fb, s);
  }
  RD_HIP(hipStreamSynchronize(s));   // levels2w is caller memory; buffers are freed next
}

// ------------------------------------------------------------------------------------------
// 7. GPU solve of the joined shard graph (device-resident variant of shardgraph.hip's host solve)
// The label graph (cut-row terminals + the outside, watershed edges of every shard, edges across every
// cut) is contracted with the SAME Boruvka machinery as the raster: only the scan differs -- it
// enumerates edges instead of cells.  A 105 ms host Priority-Flood at 8 shards becomes ~1 ms.
//   keys_all  [S][2][w]   cut-row keys of every shard
//   edges_all [S][cap][3] watershed edges of every shard (a, b, pass), counts[S] valid triples each
// Nodes: s*2w + tid; NOUT = S*2w is the outside.
// ------------------------------------------------------------------------------------------
struct GraphDesc {
  const uint32_t *keys_all, *edges_all, *counts;
  uint32_t S, w, cap, topo;
};

__device__ __forceinline__ bool graph_edge(const GraphDesc &g, uint64_t idx, uint32_t &a, uint32_t &b, uint32_t &pass) {
  const uint32_t per = 2u * g.w, NOUT = g.S * per;
  const uint64_t nintra = (uint64_t)g.S * g.cap;
  if (idx < nintra) {
    const uint32_t s = (uint32_t)(idx / g.cap), e = (uint32_t)(idx % g.cap);
    if (e >= g.counts[s]) return false;
    const uint32_t *t = g.edges_all + ((size_t)s * g.cap + e) * 3;
    a = t[0] == NO_TID ? NOUT : s * per + t[0];
    b = t[1] == NO_TID ? NOUT : s * per + t[1];
    pass = t[2];
    return true;
  }
  // edges across the cut between shard s (bottom row) and s+1 (top row), HandleEdge main.cpp:344-378
  idx -= nintra;
  const uint32_t s = (uint32_t)(idx / (3ull * g.w));
  if (s + 1 >= g.S) return false;
  const uint32_t r = (uint32_t)(idx % (3ull * g.w));
  const int x = (int)(r / 3), dx = (int)(r % 3) - 1;
  if (g.topo == 4 && dx != 0) return false;
  const int x2 = x + dx;
  if (x2 < 0 || x2 >= (int)g.w) return false;
  const bool sa = x == 0 || x == (int)g.w - 1, sb = x2 == 0 || x2 == (int)g.w - 1;   // side columns: true border
  if (sa && sb) return false;
  a = sa ? NOUT : s * per + g.w + (uint32_t)x;
  b = sb ? NOUT : (s + 1) * per + (uint32_t)x2;
  const uint32_t ka = g.keys_all[((size_t)s * 2 + 1) * g.w + x], kb = g.keys_all[((size_t)(s + 1) * 2) * g.w + x2];
  pass = ka > kb ? ka : kb;
  return true;
}

// a shard's edge count beyond the capacity of the gathered payload: its edges were not sent (sharded.py, one exchange)
__global__ void k_graph_check_counts(const uint32_t *__restrict__ counts, uint32_t S, uint32_t cap, uint32_t *flag) {
  for (uint32_t s = threadIdx.x; s < S; s += blockDim.x)
    if (counts[s] > cap) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(NTHR) void k_graph_touch(GraphDesc g, uint64_t nslots, uint32_t *closed) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x; i < nslots; i += stride) {
    uint32_t a, b, p;
    if (!graph_edge(g, i, a, b, p)) continue;
    closed[a] = NO_TID;   // NO_TID = "open" in k_init_tables' convention
    closed[b] = NO_TID;
  }
}

__global__ __launch_bounds__(NTHR) void k_graph_scan(GraphDesc g, uint64_t nslots, const uint32_t *__restrict__ cur,
                                                     unsigned long long *best) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x; i < nslots; i += stride) {
    uint32_t a, b, p;
    if (!graph_edge(g, i, a, b, p)) continue;
    const uint32_t ca = cur[a], cb = cur[b];
    if (ca == cb) continue;
    if (!(ca & CLOSED)) {
      const unsigned long long e = ((unsigned long long)p << 32) | cb;
      if (e < best[ca]) atomicMin(&best[ca], e);
    }
    if (!(cb & CLOSED)) {
      const unsigned long long e = ((unsigned long long)p << 32) | ca;
      if (e < best[cb]) atomicMin(&best[cb], e);
    }
  }
}

__global__ __launch_bounds__(NTHR) void k_graph_levels(const uint32_t *__restrict__ cur, const uint32_t *__restrict__ acc,
                                                       const uint32_t *__restrict__ closed, uint32_t *levels, uint32_t NOUT) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= NOUT) return;
  levels[i] = closed[i] == NO_TID ? acc[i] : 0u;   // untouched ids (non-cut rows, side columns) -> 0
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_rows_to_keys(const T *__restrict__ top, const T *__restrict__ bottom,
                                                       uint32_t *keys, int w) {
  const int x = blockIdx.x * NTHR + threadIdx.x;
  if (x >= w) return;
  keys[x] = Key32<T>::to(top[x]);
  keys[w + x] = Key32<T>::to(bottom[x]);
}

static void graph_solve_device(int S, int w, int topo, const uint32_t *d_keys_all, const uint32_t *d_edges_all,
                               const uint32_t *d_counts, uint32_t cap, uint32_t *d_levels_all, hipStream_t s) {
  if (S < 1 || w < 1 || !d_keys_all || !d_levels_all) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_graph_solve_dev: bad arguments");
  const uint32_t per = 2u * (uint32_t)w, NOUT = (uint32_t)S * per;
  RD_HIP(hipMemsetAsync(d_levels_all, 0, (size_t)NOUT * 4, s));
  if (S == 1) return;
  Workspace &ws = Workspace::get();
  uint32_t *hw = ws.host_words();
  GraphDesc g{d_keys_all, d_edges_all, d_counts, (uint32_t)S, (uint32_t)w, cap, (uint32_t)topo};
  const uint64_t nslots = (uint64_t)S * cap + (uint64_t)(S - 1) * 3ull * (uint64_t)w;
  const uint32_t B = NOUT;   // "basins" = graph nodes, index B = the outside
  uint32_t *cur = ws.buf<uint32_t>("graph.cur", (size_t)B + 1);
  uint32_t *acc = ws.buf<uint32_t>("graph.acc", (size_t)B + 1);
  uint32_t *closed = ws.buf<uint32_t>("graph.closed", (size_t)B + 1);
  unsigned long long *best = ws.buf<unsigned long long>("graph.best", (size_t)B + 1);
  unsigned long long *link = ws.buf<unsigned long long>("graph.link", (size_t)B + 1);
  uint32_t *rootsA = ws.buf<uint32_t>("graph.rootsA", B), *rootsB = ws.buf<uint32_t>("graph.rootsB", B);
  uint32_t *dflags = ws.buf<uint32_t>("graph.flags", 16);
  const uint32_t egrid = (uint32_t)std::min<uint64_t>((nslots + NTHR - 1) / NTHR, 256u * 16u);
  RD_HIP(hipMemsetAsync(closed, 0, ((size_t)B + 1) * 4, s));   // 0 = closed (isolated) until an edge touches it
  RD_LAUNCH("graph.touch", k_graph_touch, dim3(egrid), dim3(NTHR), 0, s, g, nslots, closed);
  RD_HIP(hipMemsetAsync(dflags, 0, 16 * 4, s));
  if (d_counts) hipLaunchKernelGGL(k_graph_check_counts, dim3(1), dim3(64), 0, s, d_counts, (uint32_t)S, cap, dflags + 3);
  RD_LAUNCH("graph.init_tables", k_init_tables, dim3(cdiv((uint64_t)B + 1, NTHR)), dim3(NTHR), 0, s, cur, acc, link, rootsA,
            dflags + 2, (const uint32_t *)closed, B);
  RD_HIP(hipMemcpyAsync(hw, dflags + 2, 8, hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  if (hw[1] != 0) throw Error(RDGPU_ERR_CAPACITY, "rdgpu_fill_graph_solve_dev: a shard holds more edges than the gathered payload has room for");
  const uint32_t nroots0 = hw[0];
  // r06: the rounds as in fill_fused -- counts on the device (rc[4 r] = live roots entering round r), grid-stride round kernels,
  // a batch of rounds per synchronisation (r05: two to three synchronisations PER ROUND; every rank of a sharded fill runs this
  // solve, so its host round trips are on every rank's critical path)
  constexpr int MAXR = 40;
  uint32_t *rc = ws.buf<uint32_t>("graph.round_counts", 4 * (MAXR + 2));
  RD_HIP(hipMemsetAsync(rc, 0, 4 * (MAXR + 2) * sizeof(uint32_t), s));
  hw[220] = nroots0;
  RD_HIP(hipMemcpyAsync(rc + 4, hw + 220, sizeof(uint32_t), hipMemcpyHostToDevice, s));
  uint32_t *hrc = hw + 16;
  int rdone = 0;
  uint32_t lg = 0;
  while ((1ull << lg) < (unsigned long long)nroots0 + 1ull) lg++;
  int batch = std::min(MAXR, std::max(4, (int)(2 * lg + 4) / 5 + 2));
  uint32_t last_live = 0xFFFFFFFFu;
  while (nroots0 > 0) {
    for (int k = 0; k < batch && rdone < MAXR; k++) {
      const int r = ++rdone;
      const uint32_t bound = std::max(1u, r - 1 < 31 ? nroots0 >> (r - 1) : 1u);
      const uint32_t rgrid = std::min(2048u, cdiv(bound, NTHR));
      const uint32_t *nr = rc + 4 * r;
      RD_LAUNCH("graph.best_reset", k_best_reset, dim3(rgrid), dim3(NTHR), 0, s, rootsA, 0u, best, nr);
      RD_LAUNCH("graph.scan", k_graph_scan, dim3(egrid), dim3(NTHR), 0, s, g, nslots, (const uint32_t *)cur, best);
      RD_LAUNCH("graph.hook", k_hook, dim3(rgrid), dim3(NTHR), 0, s, rootsA, 0u, best, link, nr);
      RD_LAUNCH("graph.chase_links", k_chase_links, dim3(rgrid), dim3(NTHR), 0, s, rootsA, 0u, link, 1 << 14, dflags, nr);
      RD_LAUNCH("graph.update", k_update_basins, dim3(cdiv(B, NTHR)), dim3(NTHR), 0, s, cur, acc, link, B, nr);
      RD_LAUNCH("graph.compact_roots", k_compact_roots, dim3(std::min(2048u, cdiv(bound, NTHR * RPT))), dim3(NTHR), 0, s, rootsA, 0u, link,
                rootsB, rc + 4 * (r + 1), nr);
      std::swap(rootsA, rootsB);
    }
    RD_HIP(hipMemcpyAsync(hrc, rc, 4 * (MAXR + 2) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RD_HIP(hipMemcpyAsync(hw, dflags, 4, hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    if (hw[0] != 0) throw Error(RDGPU_ERR_HIP, "rdgpu_fill_graph_solve_dev: a chain of hooks longer than 16384 (internal error)");
    const uint32_t live = hrc[4 * (rdone + 1)];
    if (live == 0) break;
    if (live >= last_live || rdone >= MAXR)
      throw Error(RDGPU_ERR_HIP, "rdgpu_fill_graph_solve_dev: a cut-row terminal is not connected to the outside");
    last_live = live;
    batch = 4;
  }
  RD_LAUNCH("graph.levels", k_graph_levels, dim3(cdiv(NOUT, NTHR)), dim3(NTHR), 0, s, (const uint32_t *)cur,
            (const uint32_t *)acc, (const uint32_t *)closed, d_levels_all, NOUT);
}

template <class T>
static void shard_export_dev(rdgpu_fill_shard *sh, uint32_t *d_keys, uint32_t *d_edges, uint32_t cap) {
  const int w = sh->w, h = sh->h;
  const T *base = (const T *)sh->d_dem;
  RD_LAUNCH("shard.rows_to_keys", (k_rows_to_keys<T>), dim3(cdiv(w, NTHR)), dim3(NTHR), 0, sh->stream, base,
            base + (size_t)(h - 1) * w, d_keys, w);
  if (sh->nedges) {
    if (!d_edges || cap < sh->nedges) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard_export_dev: edge buffer too small");
    RD_HIP(hipMemcpyAsync(d_edges, sh->d_edges, (size_t)sh->nedges * 12, hipMemcpyDeviceToDevice, sh->stream));
  }
}

template <class T>
static void shard_finish_dev(rdgpu_fill_shard *sh, const uint32_t *d_levels2w) {
  hipStream_t s = sh->stream;
  if (!sh->fb.trivial) {
    if (sh->fb.tid) {
      if (!d_levels2w) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard_finish_dev: levels required for a shard with cut rows");
      RD_LAUNCH("shard.apply", k_shard_apply, dim3(cdiv(sh->fb.B, NTHR)), dim3(NTHR), 0, s, (const uint32_t *)sh->fb.cur,
                sh->fb.acc, (const uint32_t *)sh->fb.tid, d_levels2w, sh->fb.B);
    }
    if (sh->fb.compact) fill_finalize16<T>((T *)sh->d_dem, sh->w, sh->h, sh->fb, s);
    else fill_finalize<T>((T *)sh->d_dem, sh->w, sh->h, sh->fb, s);
  }
  RD_HIP(hipStreamSynchronize(s));   // the handle's buffers are freed next
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_FILL_API(SUF, T)                                                                       \
  extern "C" int rdgpu_fill_multi_##SUF(T *, int, int, int, const int *, int);                    \
  extern "C" int rdgpu_fill_##SUF(T *dem, int w, int h, int topology) {                           \
    const std::vector<int> devs = env_devices();                                                  \
    if (devs.size() > 1 && h >= 2 * (int)devs.size())                                             \
      return rdgpu_fill_multi_##SUF(dem, w, h, topology, devs.data(), (int)devs.size());          \
    return guarded([&] { fill_host<T>(dem, w, h, topology); });                                   \
  }                                                                                               \
  extern "C" int rdgpu_fill_outlets_dev_##SUF(T *d_dem, const uint8_t *d_outlet, int w, int h, void *stream) { \
    return rdgpu::guarded([&] { rdgpu::fill_outlets_device<T>(d_dem, d_outlet, nullptr, w, h, (hipStream_t)stream); }); \
  }                                                                                                \
  extern "C" int rdgpu_fill_outlets_skip_dev_##SUF(T *d_dem, const uint8_t *d_outlet, const uint8_t *d_skip, int w, int h, \
                                                   void *stream) {                                 \
    return rdgpu::guarded([&] { rdgpu::fill_outlets_device<T>(d_dem, d_outlet, d_skip, w, h, (hipStream_t)stream); }); \
  }                                                                                                \
  extern "C" int rdgpu_fill_outlets_lists_dev_##SUF(T *d_dem, const uint8_t *d_outlet, const uint8_t *d_skip,             \
                                                    const uint32_t *d_lists, uint32_t stride, const uint32_t *counts3, int w, \
                                                    int h, void *stream) {                         \
    return rdgpu::guarded([&] {                                                                    \
      rdgpu::SparseLists l;                                                                        \
      l.d = d_lists; l.stride = stride;                                                            \
      for (int k = 0; k < 3; k++) l.n[k] = counts3[k];                                             \
      rdgpu::fill_outlets_device<T>(d_dem, d_outlet, d_skip, w, h, (hipStream_t)stream, &l);       \
    });                                                                                            \
  }                                                                                                \
  extern "C" int rdgpu_fill_dev_##SUF(T *d_dem, int w, int h, int topology, void *stream) {       \
    return guarded([&] { fill_device<T>(d_dem, w, h, topology, (hipStream_t)stream); });          \
  }                                                                                               \
  extern "C" int rdgpu_fill_max_dep_##SUF(T *dem, int w, int h, int topology, uint64_t max_dep_size) { \
    return guarded([&] { fill_max_dep_host<T>(dem, w, h, topology, max_dep_size); });             \
  }                                                                                               \
  extern "C" int rdgpu_fill_max_dep_dev_##SUF(T *d_dem, int w, int h, int topology, uint64_t max_dep_size, void *stream) { \
    return guarded([&] { fill_max_dep_device<T>(d_dem, w, h, topology, max_dep_size, (hipStream_t)stream); }); \
  }                                                                                               \
  extern "C" int rdgpu_fill_max_dep_ties_dev_##SUF(T *d_dem, int w, int h, int topology, uint64_t max_dep_size,            \
                                                   uint8_t *d_tie_mask, void *stream) {                                  \
    return guarded([&] { fill_max_dep_device<T>(d_dem, w, h, topology, max_dep_size, (hipStream_t)stream, d_tie_mask); }); \
  }                                                                                               \
  extern "C" int rdgpu_pit_mask_##SUF(const T *dem, T nodata, int w, int h, int topology, uint8_t *mask) { \
    return guarded([&] { pit_mask_host<T>(dem, nodata, w, h, topology, mask); });                 \
  }                                                                                               \
  extern "C" int rdgpu_pit_mask_dev_##SUF(const T *d_dem, T nodata, int w, int h, int topology, uint8_t *d_mask, \
                                          void *stream) {                                         \
    return guarded([&] { pit_mask_device<T>(d_dem, nodata, w, h, topology, d_mask, (hipStream_t)stream); }); \
  }                                                                                               \
  extern "C" int rdgpu_fill_shard_begin_##SUF(T *d_dem, int w, int h, int topology, int open_top, \
                                              int open_bottom, void *stream, rdgpu_fill_shard **out) { \
    return guarded([&] {                                                                          \
      if (!out) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard_begin: null output handle");         \
      *out = shard_begin<T>(d_dem, w, h, topology, open_top, open_bottom, (hipStream_t)stream);   \
    });                                                                                           \
  }
RD_FILL_API(u8, uint8_t)
RD_FILL_API(i16, int16_t)
RD_FILL_API(u16, uint16_t)
RD_FILL_API(i32, int32_t)
RD_FILL_API(u32, uint32_t)
RD_FILL_API(f32, float)
RD_FILL_API(i8, int8_t)

#define RD_DISPATCH(sh, CALL)                                                  \
  switch ((sh)->dtype) {                                                       \
    case 0: { using T = uint8_t; CALL; } break;                                \
    case 1: { using T = int16_t; CALL; } break;                                \
    case 2: { using T = uint16_t; CALL; } break;                               \
    case 3: { using T = int32_t; CALL; } break;                                \
    case 4: { using T = uint32_t; CALL; } break;                               \
    case 6: { using T = int8_t; CALL; } break;                                 \
    default: { using T = float; CALL; } break;                                 \
  }

extern "C" int rdgpu_fill_shard_edge_count(rdgpu_fill_shard *sh, uint32_t *n_edges) {
  return guarded([&] {
    if (!sh || !n_edges) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard_edge_count: null pointer");
    *n_edges = sh->nedges;
  });
}

extern "C" int rdgpu_fill_shard_export(rdgpu_fill_shard *sh, uint32_t *top_keys, uint32_t *bottom_keys,
                                       uint32_t *edges) {
  return guarded([&] {
    if (!sh) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard_export: null handle");
    RD_DISPATCH(sh, shard_export_rows<T>(sh, top_keys, bottom_keys));
    if (edges && sh->nedges) {
      RD_HIP(hipMemcpyAsync(edges, sh->d_edges, (size_t)sh->nedges * 12, hipMemcpyDeviceToHost, sh->stream));
      RD_HIP(hipStreamSynchronize(sh->stream));
    }
  });
}

extern "C" int rdgpu_fill_shard_finish(rdgpu_fill_shard *sh, const uint32_t *levels) {
  if (!sh) { set_last_error("rdgpu_fill_shard_finish: null handle"); return RDGPU_ERR_ARG; }
  std::lock_guard<std::recursive_mutex> lock(api_mutex());
  const int rc = guarded([&] { RD_DISPATCH(sh, shard_finish<T>(sh, levels)); });
  g_stats = sh->stats;
  shard_free(sh);
  return rc;
}

extern "C" int rdgpu_fill_shard_export_dev(rdgpu_fill_shard *sh, uint32_t *d_keys, uint32_t *d_edges, uint32_t cap) {
  return guarded([&] {
    if (!sh || !d_keys) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_shard_export_dev: null pointer");
    RD_DISPATCH(sh, shard_export_dev<T>(sh, d_keys, d_edges, cap));
  });
}

extern "C" int rdgpu_fill_shard_finish_dev(rdgpu_fill_shard *sh, const uint32_t *d_levels) {
  if (!sh) { set_last_error("rdgpu_fill_shard_finish_dev: null handle"); return RDGPU_ERR_ARG; }
  std::lock_guard<std::recursive_mutex> lock(api_mutex());
  const int rc = guarded([&] { RD_DISPATCH(sh, shard_finish_dev<T>(sh, d_levels)); });
  g_stats = sh->stats;
  shard_free(sh);
  return rc;
}

extern "C" int rdgpu_fill_graph_solve_dev(int nshards, int width, int topology, const uint32_t *d_keys_all,
                                          const uint32_t *d_edges_all, const uint32_t *d_counts, uint32_t cap,
                                          uint32_t *d_levels_all, void *stream) {
  return guarded([&] {
    if (topology != 8 && topology != 4) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_graph_solve_dev: topology must be 8 or 4");
    graph_solve_device(nshards, width, topology, d_keys_all, d_edges_all, d_counts, cap, d_levels_all, (hipStream_t)stream);
  });
}

extern "C" int rdgpu_fill_shard_free(rdgpu_fill_shard *sh) {
  shard_free(sh);
  return RDGPU_OK;
}

extern "C" int rdgpu_fill_max_dep_get_stats(rdgpu_max_dep_stats *out) {
  if (!out) return RDGPU_ERR_ARG;
  if (g_md_pending) {
    if (hipStreamSynchronize(g_md_stream) != hipSuccess) { set_last_error("rdgpu_fill_max_dep_get_stats: hipStreamSynchronize failed"); return RDGPU_ERR_HIP; }
    g_md_stats = rdgpu_max_dep_stats{g_md_pinned[0], g_md_pinned[1], g_md_pinned[2], g_md_pinned[3]};
    g_md_pending = false;
  }
  *out = g_md_stats;
  return RDGPU_OK;
}

extern "C" int rdgpu_fill_coarse_block(void) { return rdgpu::COARSE_CB; }
extern "C" int rdgpu_fill_coarse_tiles(uint64_t *out) {
  using namespace rdgpu;
  if (!out) return RDGPU_ERR_ARG;
  if (g_co_pending) {
    if (hipStreamSynchronize(g_co_stream) != hipSuccess) { set_last_error("rdgpu_fill_coarse_tiles: hipStreamSynchronize failed"); return RDGPU_ERR_HIP; }
    g_co_count = *g_co_pinned;
    g_co_pending = false;
  }
  *out = g_co_count;
  return RDGPU_OK;
}
extern "C" int rdgpu_fill_flooded_tiles(uint64_t *out) {
  if (!out) return RDGPU_ERR_ARG;
  if (g_fl_pending) {
    if (hipStreamSynchronize(g_fl_stream) != hipSuccess) { set_last_error("rdgpu_fill_flooded_tiles: hipStreamSynchronize failed"); return RDGPU_ERR_HIP; }
    g_fl_count = *g_fl_pinned;
    g_fl_pending = false;
  }
  *out = g_fl_count;
  return RDGPU_OK;
}

extern "C" int rdgpu_fill_get_stats(rdgpu_fill_stats *out) {
  if (!out) return RDGPU_ERR_ARG;
  *out = g_stats;
  return RDGPU_OK;
}
