// flat_planes.inc -- included by flats.hip (namespace rdgpu, after the bitmap search's helpers).
//
// r06: the two level fields of the directions-only flat resolution as BIT PLANES, end to end.
//
// The bitmap search (relax_visit) walks a 64 x 64 tile with lane = row and 64-bit row masks, but keeps its levels as one
// int per cell in the raster's layout (lane = column): every visit transposes twice -- 64 row loads with two ballots each
// on the way in, sixteen v_readlane and eight selects per changed row on the way out -- and those two transpositions, not
// the breadth-first steps, are most of a visit's ~3000 - 5000 wavefront instructions (r06a: 18 levels of ~45 instructions
// per working visit).  What consumes the levels afterwards, k_flat_dirs_q, needs three bits of them per cell.
//
// So the levels stay in the layout the search works in:
//   P[tile][plane][row]   16 planes of 64-bit row words: bit c of plane j of row r = bit j of the level of cell (r, c);
//                         levels 1 .. 65533 (PL_MAX + 254), all ones = not reached / does not take part.  8 KB per tile and
//                         field (the int raster: 16 KB), read and written by the tile's own visits only.
//   E[tile][4][64]        the levels of the tile's top and bottom row (lane = column) and left and right column (lane =
//                         row) as ints (DINF = not reached): what the NEIGHBOURS' visits read as their ring -- four
//                         coalesced loads instead of two row loads and two column gathers.
//   R[tile][row]          the cells reached so far (for the last pass).
// A visit loads its sixteen plane words and the ring in one go, finds "reached" / "front" for its start level by a
// bit-sliced compare, runs the same level loop, adds the segment's base to the eight relative planes bit-sliced and merges
// them into the sixteen absolute ones -- no transposition, no LDS (open water runs through the same loop).  The last pass
// (k_flat_dirs_qp) does d8_masked_FlowDir's comparison bit-sliced as well, 64 cells per operation, and only its output --
// one byte per cell that gets a direction -- is turned into the raster's layout.
// A level that does not fit 16 bits raises `overflow`; the caller then runs the int engine (nothing was written to dirs).
// The limit is looked at where a visit starts and where a 256-level segment starts, not per level (the level loop is the
// hottest code of the search): a segment that starts at base < PL_MAX assigns levels up to base + 255, also after a jump to
// the next ring level (a jump of 256 or more ends the segment first).  So PL_MAX leaves one whole segment below 0xFFFF:
// no level the planes are given reaches the all-ones pattern or wraps, and the edge ints the neighbours read are true.
constexpr int NPL = 16;
// segments starting here or later: overflow (PlaneField::max_level; RDGPU_FLAT_PLANES_MAX lowers it: tests)
constexpr int32_t PL_MAX = 0xFFFF - (1 << BPLANES);
static_assert(PL_MAX - 1 + (1 << BPLANES) - 1 < 0xFFFF, "a segment's last level must stay below the not-reached pattern");
// (struct PlaneField: flats.hip, beside BitsScratch)

template <bool CO>
__device__ __forceinline__ unsigned long long ld64(const unsigned long long *p) {
  if (CO) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}
template <bool CO>
__device__ __forceinline__ void st64(unsigned long long *p, unsigned long long v) {
  if (CO) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// Start of a field: the planes (seeds at their level, everything else all ones), the edge ints, the reached rows; with
// WRITE_M the bitmap of the cells that take part; the tiles to visit first; the edge counts (as k_bits_prepare).
template <bool TOWARDS, bool WRITE_M>
__global__ __launch_bounds__(NTHR) void k_planes_prepare(const uint8_t *__restrict__ flags, PlaneField pf, unsigned long long *mbits,
                                                         unsigned long long *seeds_out, uint8_t *tile_active, uint32_t *counts, int w,
                                                         int h, uint32_t tilesX, uint32_t tilesY) {
  constexpr int SEED = TOWARDS ? 2 : 1;
  __shared__ unsigned long long srows[BT];
  const uint32_t t = blockIdx.x;
  const int tx = (int)(t % tilesX), ty = (int)(t / tilesX);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gx = tx * BT + lane;
  unsigned long long mrow = 0, srow = 0;   // lane j < 16: the masks of row wv * 16 + j
  uint32_t nlow = 0, nhigh = 0, nnoflow = 0;
  uint8_t f[16];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int gy = ty * BT + wv * 16 + j;
    f[j] = (gx < w && gy < h) ? flags[(size_t)gy * w + gx] : (uint8_t)0;
  }
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const bool seed = TOWARDS ? (f[j] & F_NEAR) != 0 : (f[j] & F_HIGH) != 0;
    const unsigned long long mb = __ballot((f[j] & F_NOFLOW) != 0), sb = __ballot(seed);
    if (lane == j) { mrow = mb; srow = sb; }
    if (counts) {
      const unsigned long long lb = __ballot((f[j] & F_LOW) != 0), hb = __ballot((f[j] & F_HIGH) != 0);
      nnoflow += (uint32_t)__popcll(mb);
      nlow += (uint32_t)__popcll(lb);
      nhigh += (uint32_t)__popcll(hb);
    }
  }
  if (lane < 16) {
    const int row = wv * 16 + lane;
    if (WRITE_M) mbits[(size_t)t * BT + row] = mrow;
    if (seeds_out) seeds_out[(size_t)t * BT + row] = srow;
    pf.R[(size_t)t * BT + row] = srow;
    srows[row] = srow;
    // (the planes themselves are NOT written here: a tile's first visit builds them from R, the seeds' rows -- 8 KB per tile
    // and field that the start would write and the first visit read back; a tile that is never visited keeps R = 0 wherever
    // the last pass looks)
    // left / right column: lane = row
    pf.E[(size_t)t * 256 + 128 + row] = (srow & 1ull) ? SEED : DINF;
    pf.E[(size_t)t * 256 + 192 + row] = (srow >> 63 & 1ull) ? SEED : DINF;
  }
  const int any = __syncthreads_or(srow != 0);
  if (wv < 2) {   // top row, and the tile's last own row: lane = column
    const int brow = min(BT - 1, h - 1 - ty * BT);
    const unsigned long long sr = srows[wv == 0 ? 0 : brow];
    pf.E[(size_t)t * 256 + wv * 64 + lane] = (sr >> lane & 1ull) ? SEED : DINF;
  }
  if (any && threadIdx.x < 9) {
    const int ntx = tx + (int)threadIdx.x % 3 - 1, nty = ty + (int)threadIdx.x / 3 - 1;
    if (ntx >= 0 && nty >= 0 && ntx < (int)tilesX && nty < (int)tilesY) tile_active[nty * tilesX + ntx] = 1;
  }
  if (counts && lane == 0 && (nlow | nhigh | nnoflow)) {
    uint32_t *c = counts + 3 * ((t * 4 + wv) & 255u);
    if (nlow) atomicAdd(c, nlow);
    if (nhigh) atomicAdd(c + 1, nhigh);
    if (nnoflow) atomicAdd(c + 2, nnoflow);
  }
}

// One visit of tile t by one wavefront, on the planes; returns the 9-bit mask of the neighbouring tiles to wake.
template <int SEED_LEVEL, bool CO>
__device__ __forceinline__ uint32_t relax_visit_p(const unsigned long long *__restrict__ mbits, uint8_t *expanded, const PlaneField pf,
                                                  const uint32_t t, int w, int h, uint32_t tilesX, uint32_t tilesY) {
  const int lane = threadIdx.x & 63;
  const int tx = (int)(t % tilesX), ty = (int)(t / tilesX);
  const int y0 = ty * BT;
  const int brow = min(BT - 1, h - 1 - y0);   // the tile's last own row (63 except in the last tile row)
  const bool hasL = tx > 0, hasR = tx + 1 < (int)tilesX, hasT = ty > 0, hasB = ty + 1 < (int)tilesY;
  const size_t tb = (size_t)t * BT;
  // own planes and the ring: every load of the visit in flight together
  // A tile's FIRST visit finds no planes: it starts from the seeds' rows (R as the start left it).  In the rounds the flag is
  // read first (a branch); in the asynchronous tail, where a visit's latency is what counts and first visits are rare, the
  // planes are loaded regardless and dropped.
  bool first;
  if (CO) first = __hip_atomic_load(&expanded[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
  else first = expanded[t] == 0;
  unsigned long long own[NPL];
  const unsigned long long seeds = ld64<CO>(&pf.R[tb + lane]);
  if (CO || !__builtin_amdgcn_readfirstlane((int)first)) {
#pragma unroll
    for (int j = 0; j < NPL; j++) own[j] = ld64<CO>(&pf.P[((size_t)t * NPL + j) * BT + lane]);
  }
  const unsigned long long M = mbits[tb + lane];
  const unsigned long long mT = hasT ? mbits[tb - (size_t)tilesX * BT + (BT - 1)] : 0ull;   // (wave uniform)
  const unsigned long long mB = hasB ? mbits[tb + (size_t)tilesX * BT] : 0ull;
  const unsigned long long mL = hasL ? mbits[tb - BT + lane] : 0ull;
  const unsigned long long mR = hasR ? mbits[tb + BT + lane] : 0ull;
  const bool eTL = hasL && hasT && (mbits[tb - (size_t)tilesX * BT - BT + (BT - 1)] >> 63 & 1ull);
  const bool eTR = hasR && hasT && (mbits[tb - (size_t)tilesX * BT + BT + (BT - 1)] & 1ull);
  const bool eBL = hasL && hasB && (mbits[tb + (size_t)tilesX * BT - BT] >> 63 & 1ull);
  const bool eBR = hasR && hasB && (mbits[tb + (size_t)tilesX * BT + BT] & 1ull);
  const int32_t *const E = pf.E;
  const size_t eb = (size_t)t * 256, eup = (size_t)tilesX * 256;
  int32_t tv = hasT ? ldD<CO>(&E[eb - eup + 64 + lane]) : DINF;     // the bottom row of the tile above
  int32_t bv = hasB ? ldD<CO>(&E[eb + eup + lane]) : DINF;          // the top row of the tile below
  int32_t lv = hasL ? ldD<CO>(&E[eb - 256 + 192 + lane]) : DINF;    // the right column of the tile to the left
  int32_t rv = hasR ? ldD<CO>(&E[eb + 256 + 128 + lane]) : DINF;
  int32_t tl = eTL ? ldD<CO>(&E[eb - eup - 256 + 64 + 63]) : DINF, tr = eTR ? ldD<CO>(&E[eb - eup + 256 + 64]) : DINF;
  int32_t bl = eBL ? ldD<CO>(&E[eb + eup - 256 + 63]) : DINF, br = eBR ? ldD<CO>(&E[eb + eup + 256]) : DINF;
  const int32_t oldT = ldD<CO>(&E[eb + lane]), oldB = ldD<CO>(&E[eb + 64 + lane]), oldL = ldD<CO>(&E[eb + 128 + lane]),
                oldR = ldD<CO>(&E[eb + 192 + lane]);
  if (!(mT >> lane & 1ull)) tv = DINF;
  if (!(mB >> lane & 1ull)) bv = DINF;
  if (!(mL >> 63 & 1ull)) lv = DINF;
  if (!(mR & 1ull)) rv = DINF;
  tl = __builtin_amdgcn_readfirstlane(tl); tr = __builtin_amdgcn_readfirstlane(tr);
  bl = __builtin_amdgcn_readfirstlane(bl); br = __builtin_amdgcn_readfirstlane(br);
  int32_t newT = oldT, newB = oldB, newL = oldL, newR = oldR;
  // the level at which each edge cell is reached from the ring (as relax_visit)
  const int32_t tL = from_left(tv, tl), tR = from_right(tv, tr), bL = from_left(bv, bl), bR = from_right(bv, br);
  const int32_t lU = from_left(lv, tl), lD = from_right(lv, bl), rU = from_left(rv, tr), rD = from_right(rv, br);
  auto reach = [](int32_t a, int32_t b, int32_t c) { const int32_t m = imin(a, imin(b, c)); return m < DINF ? m + 1 : DINF; };
  const int32_t iT = reach(tL, tv, tR), iL = reach(lU, lv, lD), iR = reach(rU, rv, rD);
  // (the bottom ring row meets the tile's LAST OWN row: lane = column all the same)
  const int32_t iB = reach(bL, bv, bR);
  int32_t imax_;
  {
    auto fin = [](int32_t v) { return v < DINF ? v : -1; };
    imax_ = __builtin_amdgcn_readfirstlane(wave_max_i32(max(max(fin(iT), fin(iB)), max(fin(iL), fin(iR)))));
  }
  const unsigned long long m0 = readlane64(M, 0), m63 = readlane64(M, brow);
  int32_t chg = DINF;
  if ((m0 >> lane & 1ull) && iT < oldT) chg = iT;
  if ((m63 >> lane & 1ull) && iB < oldB) chg = imin(chg, iB);
  if ((M & 1ull) && iL < oldL) chg = imin(chg, iL);
  if ((M >> 63 & 1ull) && iR < oldR) chg = imin(chg, iR);
  int32_t level = __builtin_amdgcn_readfirstlane(wave_min_i32(chg));   // the level being assigned
  first = __builtin_amdgcn_readfirstlane((int)first) != 0;
  if (first) {
    level = imin(level, SEED_LEVEL + 1);
    if (lane == 0) {
      if (CO) __hip_atomic_store(&expanded[t], (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else expanded[t] = 1;
    }
#pragma unroll
    for (int j = 0; j < NPL; j++) own[j] = (SEED_LEVEL >> j & 1) ? ~0ull : ~seeds;
  }
#ifdef RDGPU_PROBES
  uint32_t *const ph = g_probe_hist ? g_probe_hist + ((SEED_LEVEL == 2 ? 0u : 5u) * tilesX * tilesY + t) : nullptr;
  const uint32_t pstride = tilesX * tilesY;
  uint32_t psteps = 0;
  if (ph && lane == 0) {
    atomicAdd(&ph[0], 1u);
    if (level < DINF) {
      atomicAdd(&ph[pstride], 1u);
      const uint32_t last = ph[4 * pstride];
      if (last != 0 && (uint32_t)level < last) atomicAdd(&ph[3 * pstride], 1u);
      ph[4 * pstride] = (uint32_t)level;
    }
  }
#endif
  if (level >= DINF) return 0u;   // nothing new reaches this tile
  if (level >= pf.max_level) {
    if (lane == 0) atomicExch(pf.overflow, 1u);
    return 0u;
  }
  // the cells below the start level are "reached", those one below it the front: one bit-sliced compare with K = level - 1
  unsigned long long A, F, Rec = 0, RecAll = 0;
  {
    const uint32_t K = (uint32_t)(level - 1);
    unsigned long long lt = 0, eq = ~0ull;
#pragma unroll
    for (int j = NPL - 1; j >= 0; j--) {
      if (K >> j & 1u) { lt |= eq & ~own[j]; eq &= own[j]; }
      else eq &= ~own[j];
    }
    A = M & ~(lt | eq);
    F = M & eq;
  }
  uint32_t Plo[BPLANES], Phi[BPLANES];
#pragma unroll
  for (int j = 0; j < BPLANES; j++) Plo[j] = Phi[j] = 0;
  int32_t base = level;
  bool over = false;

  // the cells recorded since the last flush get base + their relative level, bit-sliced, in the sixteen absolute planes
  auto flush = [&]() {
    const uint32_t ub = (uint32_t)base;
    unsigned long long c = 0;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
      const unsigned long long a = j < BPLANES ? (((unsigned long long)Phi[j < BPLANES ? j : 0] << 32) | Plo[j < BPLANES ? j : 0]) : 0ull;
      const unsigned long long bm = (ub >> j & 1u) ? ~0ull : 0ull;
      const unsigned long long x = a ^ bm;
      const unsigned long long sres = x ^ c;
      c = (a & bm) | (c & x);
      own[j] = (own[j] & ~Rec) | (sres & Rec);
    }
    RecAll |= Rec;
    Rec = 0;
#pragma unroll
    for (int j = 0; j < BPLANES; j++) Plo[j] = Phi[j] = 0;
  };

  for (bool searching = true; searching;) {
    if (level >= pf.max_level) { over = true; break; }
    for (;;) {
      if (level - base >= (1 << BPLANES)) break;   // planes full: flush, then on with this level
      uint32_t nlo, nhi;
      {
        const unsigned long long v = F | row_above(F) | row_below(F);
        const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
        nlo = lo | (lo << 1) | __builtin_amdgcn_alignbit(hi, lo, 1);
        nhi = hi | (hi >> 1) | __builtin_amdgcn_alignbit(hi, lo, 31);
      }
      if (level <= imax_) {
        const unsigned long long T = __ballot(iT == level), B = __ballot(iB == level);
        const unsigned long long tb_ = (lane == 0 ? T : 0ull) | (lane == brow ? B : 0ull);
        nlo |= (uint32_t)tb_ | (iL == level ? 1u : 0u);
        nhi |= (uint32_t)(tb_ >> 32) | (iR == level ? 0x80000000u : 0u);
      }
      nlo &= (uint32_t)A; nhi &= (uint32_t)(A >> 32);
      const unsigned long long N = ((unsigned long long)nhi << 32) | nlo;
#ifdef RDGPU_PROBES
      psteps++;
#endif
      if (__any(N != 0)) {
        const int32_t rel = level - base;
        A &= ~N;
        Rec |= N;
#pragma unroll
        for (int j = 0; j < BPLANES; j++) {
          const uint32_t m = (uint32_t)(-(int32_t)((uint32_t)rel >> j & 1u));
          Plo[j] |= nlo & m;
          Phi[j] |= nhi & m;
        }
        F = N;
        level++;
        continue;
      }
      if (!__any(A != 0) || level >= imax_) { searching = false; break; }
      auto pend = [&](int32_t v) { return v > level ? v : DINF; };
      const int32_t nx = __builtin_amdgcn_readfirstlane(wave_min_i32(imin(imin(pend(iT), pend(iB)), imin(pend(iL), pend(iR)))));
      if (nx >= DINF) { searching = false; break; }
      level = nx;
      F = 0;
    }
    if (__any(Rec != 0)) flush();
    base = level;
  }
#ifdef RDGPU_PROBES
  if (ph && lane == 0) atomicAdd(&ph[2 * pstride], psteps);
#endif
  if (over && lane == 0) atomicExch(pf.overflow, 1u);
  if (!first && !__any(RecAll != 0)) return 0u;
  // store: the planes (a first visit's in any case), the reached rows, and the edge levels that changed
#pragma unroll
  for (int j = 0; j < NPL; j++) st64<CO>(&pf.P[((size_t)t * NPL + j) * BT + lane], own[j]);
  st64<CO>(&pf.R[tb + lane], M & ~A);
  {
    auto col = [&](int bit) {   // lane = row: the level of column `bit` (0 or 63) of this lane's row
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < NPL; j++) v |= (uint32_t)(own[j] >> bit & 1ull) << j;
      return v == 0xFFFFu ? DINF : (int32_t)v;
    };
    auto rowv = [&](int r) {    // lane = column: the level of this lane's cell in row r (wave uniform)
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < NPL; j++) v |= lanes_of(readlane64(own[j], r), 1u << j);
      return v == 0xFFFFu ? DINF : (int32_t)v;
    };
    if (__any((RecAll & 1ull) != 0)) { newL = col(0); stD<CO>(&pf.E[eb + 128 + lane], newL); }
    if (__any((RecAll >> 63 & 1ull) != 0)) { newR = col(63); stD<CO>(&pf.E[eb + 192 + lane], newR); }
    if (readlane64(RecAll, 0) != 0) { newT = rowv(0); stD<CO>(&pf.E[eb + lane], newT); }
    if (readlane64(RecAll, brow) != 0) { newB = rowv(brow); stD<CO>(&pf.E[eb + 64 + lane], newB); }
  }
  // wake a neighbouring tile only if an edge cell that moved here can still lower one of ITS cells (as relax_visit)
  uint32_t wake = 0;
  {
    auto gain = [](int32_t ring, int32_t v) { return ring > v + 1; };
    const bool movedT = newT < oldT, movedB = newB < oldB, movedL = newL < oldL, movedR = newR < oldR;
    const bool eT = mT >> lane & 1ull, eB = mB >> lane & 1ull;
    const bool eTl = lane > 0 ? (mT >> (lane - 1) & 1ull) : eTL, eTr = lane < 63 ? (mT >> (lane + 1) & 1ull) : eTR;
    const bool eBl = lane > 0 ? (mB >> (lane - 1) & 1ull) : eBL, eBr = lane < 63 ? (mB >> (lane + 1) & 1ull) : eBR;
    if (movedT) {
      if (eT && gain(tv, newT)) wake |= 1u << 1;
      if (eTl && gain(tL, newT)) wake |= lane > 0 ? 1u << 1 : 1u << 0;
      if (eTr && gain(tR, newT)) wake |= lane < 63 ? 1u << 1 : 1u << 2;
    }
    if (movedB) {
      if (eB && gain(bv, newB)) wake |= 1u << 7;
      if (eBl && gain(bL, newB)) wake |= lane > 0 ? 1u << 7 : 1u << 6;
      if (eBr && gain(bR, newB)) wake |= lane < 63 ? 1u << 7 : 1u << 8;
    }
    const unsigned long long eLm = __ballot(mL >> 63 & 1ull), eRm = __ballot(mR & 1ull);
    const bool eL = eLm >> lane & 1ull, eR = eRm >> lane & 1ull;
    const bool eLu = lane > 0 ? (eLm >> (lane - 1) & 1ull) : eTL, eLd = lane < 63 ? (eLm >> (lane + 1) & 1ull) : eBL;
    const bool eRu = lane > 0 ? (eRm >> (lane - 1) & 1ull) : eTR, eRd = lane < 63 ? (eRm >> (lane + 1) & 1ull) : eBR;
    if (movedL) {
      if (eL && gain(lv, newL)) wake |= 1u << 3;
      if (eLu && gain(lU, newL)) wake |= lane > 0 ? 1u << 3 : 1u << 0;
      if (eLd && gain(lD, newL)) wake |= lane < 63 ? 1u << 3 : 1u << 6;
    }
    if (movedR) {
      if (eR && gain(rv, newR)) wake |= 1u << 5;
      if (eRu && gain(rU, newR)) wake |= lane > 0 ? 1u << 5 : 1u << 2;
      if (eRd && gain(rD, newR)) wake |= lane < 63 ? 1u << 5 : 1u << 8;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) wake |= __shfl_xor(wake, o, 64);
  return wake;
}

template <int SEED_LEVEL>
__global__ __launch_bounds__(NTHR, 4) void k_relax_planes(const unsigned long long *__restrict__ mbits, uint8_t *expanded, PlaneField pf,
                                                       const uint32_t *__restrict__ tiles, const uint32_t *__restrict__ count,
                                                       uint8_t *next_active, int w, int h, uint32_t tilesX, uint32_t tilesY) {
  const uint32_t n = *count;
  for (uint32_t i = gridDim.x * 4 + blockIdx.x * NTHR + threadIdx.x; i < n; i += gridDim.x * NTHR) next_active[tiles[i]] = 1;
  const uint32_t wi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wi >= n) return;
  const int lane = threadIdx.x & 63;
  const uint32_t t = tiles[wi];
  const uint32_t wake = relax_visit_p<SEED_LEVEL, false>(mbits, expanded, pf, t, w, h, tilesX, tilesY);
  if (lane < 9 && lane != 4 && (wake >> lane & 1u)) {
    const int tx = (int)(t % tilesX), ty = (int)(t / tilesX);
    const int ntx = tx + lane % 3 - 1, nty = ty + lane / 3 - 1;
    if (ntx >= 0 && nty >= 0 && ntx < (int)tilesX && nty < (int)tilesY) next_active[nty * tilesX + ntx] = 1;
  }
}

// ------------------------------------------------------------------------------------------
// The last pass from the planes: d8_masked_FlowDir (flat_resolution.hpp:42-65) for every cell the towards search reached,
// on the masks MODULO 8 (see k_flat_dirs_q for why that is exact), bit-sliced: lane = row, a 64-bit word = 64 cells.
//   q = (2 * towards - away) & 7 in three planes (away: 0 where the away search did not get), NP = the cell does not take
//   part (not reached by the towards search).  A neighbour's planes are the own ones shifted by a column (the carry from the
//   ring column) and / or a row (DPP, the ring row entering at lanes 0 / brow).  Per neighbour k = 1 .. 8, in the
//   reference's order: rb = ((q_n - q_c + 4) & 7) | NP_n << 3, taken if rb < m, or rb == m and the choice so far is a
//   diagonal and k a cardinal (:53-61); m starts at 4 (only strictly lower masks count), dir at 0.
// One wavefront per tile.
// ------------------------------------------------------------------------------------------
struct QRow { unsigned long long q0, q1, q2, np, near; };
__device__ __forceinline__ QRow q_row(const PlaneField &T, const PlaneField &A, const unsigned long long *__restrict__ near, bool have_away,
                                      size_t tile, int row, bool exists) {
  QRow r{0, 0, 0, ~0ull, 0};
  if (!exists) return r;
  const size_t pb = tile * NPL * BT + row, rb = tile * BT + row;
  const unsigned long long t0 = T.P[pb], t1 = T.P[pb + BT], rt = T.R[rb];
  unsigned long long a0 = 0, a1 = 0, a2 = 0;
  if (have_away) {
    const unsigned long long ra = A.R[rb];
    a0 = A.P[pb] & ra; a1 = A.P[pb + BT] & ra; a2 = A.P[pb + 2 * BT] & ra;
  }
  // (t1 t0 0) - (a2 a1 a0) modulo 8
  r.q0 = a0;
  const unsigned long long b1 = a0;
  r.q1 = t0 ^ a1 ^ b1;
  const unsigned long long b2 = (~t0 & (a1 | b1)) | (a1 & b1);
  r.q2 = t1 ^ a2 ^ b2;
  r.np = ~rt;
  r.near = near[rb];
  return r;
}

// guards (optional): the two fields' overflow words and the two tails' abort words -- with one of them set the levels are
// not final and the pass leaves `dirs` alone (the host, which reads the same words after the call's one synchronisation, then
// finishes the search another way and runs the pass again).
__global__ __launch_bounds__(NTHR) void k_flat_dirs_qp(PlaneField T, PlaneField A, const unsigned long long *__restrict__ near, int have_away,
                                                       uint8_t *dirs, int w, int h, uint32_t tilesX, uint32_t tilesY,
                                                       const uint32_t *__restrict__ g_over, const uint32_t *__restrict__ g_abort_t,
                                                       const uint32_t *__restrict__ g_abort_a) {
  if ((g_over && (g_over[0] | g_over[1])) || (g_abort_t && *g_abort_t) || (g_abort_a && *g_abort_a)) return;
  const uint32_t ntiles = tilesX * tilesY;
  const uint32_t t = xcd_tile(blockIdx.x, (ntiles + 3) / 4) * 4 + (threadIdx.x >> 6);
  if (t >= ntiles) return;
  const int lane = threadIdx.x & 63;
  const int tx = (int)(t % tilesX), ty = (int)(t / tilesX);
  const int x0 = tx * BT, y0 = ty * BT;
  const int brow = min(BT - 1, h - 1 - y0);
  const bool hasL = tx > 0, hasR = tx + 1 < (int)tilesX, hasT = ty > 0, hasB = ty + 1 < (int)tilesY;
  const bool ha = have_away != 0;
  const QRow c = q_row(T, A, near, ha, t, lane, true);
  // the centre cells that get a direction here: reached, not next to a low edge (those have theirs), interior of the raster
  unsigned long long want = ~c.np & ~c.near;
  {
    const int gy = y0 + lane;
    if (gy <= 0 || gy >= h - 1) want = 0;
    if (x0 == 0) want &= ~1ull;
    const int lastc = w - 1 - x0;   // column of the raster's last cell in this tile's frame (>= 64: not in this tile)
    if (lastc < 64) want &= (lastc <= 0) ? 0ull : ((1ull << lastc) - 1ull);
  }
  if (!__any(want != 0)) return;
  // the ring: rows above / below (lane = their column word, wave uniform), columns left / right (one bit per lane)
  const QRow up = q_row(T, A, near, ha, (size_t)t - tilesX, BT - 1, hasT), dn = q_row(T, A, near, ha, (size_t)t + tilesX, 0, hasB);
  const QRow lf = q_row(T, A, near, ha, (size_t)t - 1, lane, hasL), rt = q_row(T, A, near, ha, (size_t)t + 1, lane, hasR);
  const QRow ul = q_row(T, A, near, ha, (size_t)t - tilesX - 1, BT - 1, hasT && hasL), ur = q_row(T, A, near, ha, (size_t)t - tilesX + 1, BT - 1, hasT && hasR);
  const QRow dl = q_row(T, A, near, ha, (size_t)t + tilesX - 1, 0, hasB && hasL), dr = q_row(T, A, near, ha, (size_t)t + tilesX + 1, 0, hasB && hasR);
  // one plane of the 3 x 3 neighbourhood: X = the tile's rows, U / D = the ring rows' words, and the ring columns' bits
  // (lbit / rbit per lane = row; the four corners)
  struct Plane { unsigned long long x, up, dn; uint32_t lb, rb, ulb, urb, dlb, drb; };
  auto plane = [&](unsigned long long x, unsigned long long u, unsigned long long d, unsigned long long l, unsigned long long r,
                   unsigned long long cul, unsigned long long cur, unsigned long long cdl, unsigned long long cdr) {
    Plane p;
    p.x = x; p.up = u; p.dn = d;
    p.lb = (uint32_t)(l >> 63 & 1ull); p.rb = (uint32_t)(r & 1ull);
    p.ulb = (uint32_t)(cul >> 63 & 1ull); p.urb = (uint32_t)(cur & 1ull); p.dlb = (uint32_t)(cdl >> 63 & 1ull); p.drb = (uint32_t)(cdr & 1ull);
    return p;
  };
  const Plane P0 = plane(c.q0, up.q0, dn.q0, lf.q0, rt.q0, ul.q0, ur.q0, dl.q0, dr.q0);
  const Plane P1 = plane(c.q1, up.q1, dn.q1, lf.q1, rt.q1, ul.q1, ur.q1, dl.q1, dr.q1);
  const Plane P2 = plane(c.q2, up.q2, dn.q2, lf.q2, rt.q2, ul.q2, ur.q2, dl.q2, dr.q2);
  const Plane P3 = plane(c.np, up.np, dn.np, lf.np, rt.np, ul.np, ur.np, dl.np, dr.np);
  // the row above / below every lane's row, as (word, left bit, right bit)
  struct Row3 { unsigned long long x; uint32_t lb, rb; };
  auto above = [&](const Plane &p) {
    Row3 r;
    r.x = row_above(p.x); r.lb = dpp_up(p.lb); r.rb = dpp_up(p.rb);
    if (lane == 0) { r.x = p.up; r.lb = p.ulb; r.rb = p.urb; }
    return r;
  };
  auto below = [&](const Plane &p) {
    Row3 r;
    r.x = row_below(p.x); r.lb = dpp_dn(p.lb); r.rb = dpp_dn(p.rb);
    if (lane == brow) { r.x = p.dn; r.lb = p.dlb; r.rb = p.drb; }
    return r;
  };
  auto same = [&](const Plane &p) { return Row3{p.x, p.lb, p.rb}; };
  // the value of the cell to the left (dx = -1) / right (dx = +1) / same column of every cell of a row
  auto shift = [](const Row3 &r, int dx) -> unsigned long long {
    if (dx < 0) return (r.x << 1) | (unsigned long long)r.lb;
    if (dx > 0) return (r.x >> 1) | ((unsigned long long)r.rb << 63);
    return r.x;
  };
  const Row3 a0 = above(P0), a1 = above(P1), a2 = above(P2), a3 = above(P3);
  const Row3 s0 = same(P0), s1 = same(P1), s2 = same(P2), s3 = same(P3);
  const Row3 b0 = below(P0), b1 = below(P1), b2 = below(P2), b3 = below(P3);
  const unsigned long long C0 = c.q0, C1 = c.q1, C2 = ~c.q2;   // q_c - 4 modulo 8
  unsigned long long m0 = 0, m1 = 0, m2 = ~0ull, m3 = 0;      // m = 4
  unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
  auto step = [&](const Row3 &r0, const Row3 &r1, const Row3 &r2, const Row3 &r3, int dx, int k) {
    const unsigned long long V0 = shift(r0, dx), V1 = shift(r1, dx), V2 = shift(r2, dx), V3 = shift(r3, dx);
    // rb = ((v - qc) & 7) | np << 3
    const unsigned long long R0 = V0 ^ C0, br1 = ~V0 & C0;
    const unsigned long long R1 = V1 ^ C1 ^ br1, br2 = (~V1 & (C1 | br1)) | (C1 & br1);
    const unsigned long long R2 = V2 ^ C2 ^ br2, R3 = V3;
    // rb < m, rb == m (4-bit, from the top)
    unsigned long long lt = ~R3 & m3, eq = ~(R3 ^ m3);
    lt |= eq & ~R2 & m2; eq &= ~(R2 ^ m2);
    lt |= eq & ~R1 & m1; eq &= ~(R1 ^ m1);
    lt |= eq & ~R0 & m0; eq &= ~(R0 ^ m0);
    unsigned long long take = lt;
    if (k & 1) take |= eq & (d1 | d2 | d3) & ~d0;   // the choice so far is a diagonal (even, > 0), k a cardinal
    m0 = (m0 & ~take) | (R0 & take); m1 = (m1 & ~take) | (R1 & take);
    m2 = (m2 & ~take) | (R2 & take); m3 = (m3 & ~take) | (R3 & take);
    d0 = (k & 1) ? (d0 | take) : (d0 & ~take);
    d1 = (k & 2) ? (d1 | take) : (d1 & ~take);
    d2 = (k & 4) ? (d2 | take) : (d2 & ~take);
    d3 = (k & 8) ? (d3 | take) : (d3 & ~take);
  };
  // neighbours 1 .. 8 in the 234 / 105 / 876 numbering
  step(s0, s1, s2, s3, -1, 1);
  step(a0, a1, a2, a3, -1, 2);
  step(a0, a1, a2, a3, 0, 3);
  step(a0, a1, a2, a3, 1, 4);
  step(s0, s1, s2, s3, 1, 5);
  step(b0, b1, b2, b3, 1, 6);
  step(b0, b1, b2, b3, 0, 7);
  step(b0, b1, b2, b3, -1, 8);
  // out: one byte per wanted cell, row by row (lane = column)
  unsigned long long rows = __ballot(want != 0);
  while (rows) {
    const int r = __ffsll((long long)rows) - 1;
    rows &= rows - 1;
    const unsigned long long wr = readlane64(want, r);
    const uint32_t v = lanes_of(readlane64(d0, r), 1u) | lanes_of(readlane64(d1, r), 2u) | lanes_of(readlane64(d2, r), 4u) |
                       lanes_of(readlane64(d3, r), 8u);
    if (lanes_of(wr, 1u)) dirs[(size_t)(y0 + r) * w + x0 + lane] = (uint8_t)v;
  }
}
