// breach.hip -- depression breaching on the D8 link forest: the carve along GIVEN directions (rdgpu_d8_breach_along) and
// CompleteBreaching_Lindsay2016<D8> (rdgpu_breach_d8: pit stencil, the flood's tree from pfdirs.hip under Lindsay's
// conventions, the carve along that tree).  The contracts are in include/rdgpu.h, the formulation in DESIGN.md section 6n.
//
// The carve is a FILTERED closure.  Every pit p sends its level dem(p) down the chain of links; the level enters a cell x
// iff dem(x) >= dem(p), and a cell ends at the least level that entered it.  As a word that only grows:
//   word(level) = ~ord(level) (+ 1 for the 32-bit integer types, see BrWord), 0 = "no level",
//   thr(x)      = ~ord(dem(x)): a word t enters x iff t's level word >= thr(x).
// A lower level is a larger word, and a larger word passes wherever a smaller one does, so the words are closed downstream
// exactly as extreme.hip closes its keys -- pushed over doubled pointers, first in LDS, then over the border nodes -- if
// every pointer, WHEREVER it is doubled, carries the largest thr over the cells it spans, its target included: a word is
// pushed across a pointer iff it is >= that span threshold.  Two spans compose by the maximum.
//   k_br_links         per border node: the node its in-tile path leaves to, and the span threshold of that path up to and
//                      including the entry cell of the next tile -- ONE 64-bit word per node (threshold << 32 | node).
//   k_br_close<SEED>   the pits' words closed in the tile (pointer and threshold doubled together in LDS); every exit cell
//                      whose word enters its target raises the target's node.
//   k_br_round         the node words pushed over doubled (pointer, threshold) words, ping-pong; ceil(log2(nodes)) + 1 rounds
//                      enqueued, a round returns at once on a device-side flag when its predecessor raised nothing.
//   k_br_close<WRITE>  the pits' words and the node words of the tile's own border slots closed in the tile; every cell
//                      decoded and both planes written once.
// No host synchronisation in the carve's device driver; 2 memsets + 3 + rounds launches, fixed by the raster's size.
// LDS per block: 4752 B staged directions + 8448 B pointers + 16896 B thresholds + 16896 B words = 46992 B (three blocks
// per CU); 63888 B with the 64-bit words of i32 / u32 (two blocks).  Scratch: two 8-byte link buffers and one word per node,
// 20 or 24 B; 256 nodes per 4096 cells: 1.5 B per cell.
#include "d8_forest.hpp"
#include "pfdirs.hpp"

#include <algorithm>
#include <limits>
#include <string>
#include <type_traits>

namespace rdgpu {

constexpr unsigned long long BR_NONE = 0x00000000FFFFFFFFull;   // a node's (threshold, link) word: no link
constexpr uint32_t BR_BLOCK = 0xFFFFFFFFu;                      // the threshold of an f32 NaN cell: no f32 word reaches it
enum { BR_SEED = 0, BR_WRITE = 1 };

// The word of a level.  ~ord is never 0 for the 8- and 16-bit types and for f32 (ord == 0xFFFFFFFF would be a NaN), so 0 is
// free for "no level" there.  For i32 and u32 the type's maximum has ~ord == 0: their words are 64 bits wide, ~ord + 1.
template <class T>
struct BrWord {
  typedef uint32_t type;
  static constexpr uint32_t BIAS = 0;
};
template <>
struct BrWord<int32_t> {
  typedef unsigned long long type;
  static constexpr uint32_t BIAS = 1;
};
template <>
struct BrWord<uint32_t> {
  typedef unsigned long long type;
  static constexpr uint32_t BIAS = 1;
};

// ord: T onto uint32, monotone.  f32: the IEEE total order on the non-NaN values.
template <class T>
__device__ __forceinline__ uint32_t br_ord(T v) {
  if constexpr (std::is_same<T, float>::value) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  } else if constexpr (std::is_signed<T>::value) {
    return (uint32_t)(int32_t)v ^ 0x80000000u;
  } else {
    return (uint32_t)v;
  }
}
// the bits of the T that ord maps to o, zero-extended
template <class T>
__device__ __forceinline__ uint32_t br_unord(uint32_t o) {
  if constexpr (std::is_same<T, float>::value) return (o >> 31) ? o ^ 0x80000000u : ~o;
  else if constexpr (std::is_signed<T>::value) return o ^ 0x80000000u;
  else return o;
}
// the threshold of a cell that holds v
template <class T>
__device__ __forceinline__ uint32_t br_thr(T v) {
  if constexpr (std::is_same<T, float>::value) {
    if (!(v == v)) return BR_BLOCK;
  }
  return ~br_ord<T>(v);
}
template <class T>
__device__ __forceinline__ void br_store_bits(T *p, uint32_t bits) {
  if constexpr (sizeof(T) == 4) *reinterpret_cast<uint32_t *>(p) = bits;
  else if constexpr (sizeof(T) == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)bits;
  else *reinterpret_cast<uint8_t *>(p) = (uint8_t)bits;
}

// ---- the node links with their span thresholds ---------------------------------------------------------------------------
struct BrLinkTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(4)));
  uint16_t lp[LT * LPS];   // tile pointers with FOREST_END, as k_forest_links'
  uint32_t th[LT * LPS];   // the largest thr over the cells the pointer spans, its target included (an end: 0)
};

template <class T>
__global__ __launch_bounds__(NTHR, 3) void k_br_links(const uint8_t *__restrict__ dirs, uint8_t nodata, const T *__restrict__ dem, int w,
                                                      int h, uint32_t tilesX, uint32_t ntiles, unsigned long long *__restrict__ nxt0) {
  __shared__ BrLinkTile S;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, S.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {   // every cell's own threshold, for the cells that point at it
    const int ly = ly0 + 4 * j, gx = x0 + lx, gy = y0 + ly;
    S.th[ly * LPS + lx] = (gx < w && gy < h) ? br_thr<T>(dem[(size_t)gy * w + gx]) : 0u;
  }
  __syncthreads();
  uint32_t p[FOREST_RPT], th[FOREST_RPT];
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int kind = forest_link(S.sd, nodata, lx, ly, tx, ty);
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : (self | FOREST_END);
    th[j] = kind == 1 ? S.th[ty * LPS + tx] : 0u;
    S.lp[self] = (uint16_t)p[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) S.th[(ly0 + 4 * j) * LPS + lx] = th[j];
  __syncthreads();
  // forest_jump_sync with the thresholds: pointer and threshold are read together before the barrier and stored together
  // behind it, so that every pair in the table is one consistent span
  {
    uint32_t q[FOREST_RPT], tq[FOREST_RPT];
#pragma unroll 1
    for (int it = 0; it < FOREST_JUMPS; it++) {
      bool moving = false;
#pragma unroll
      for (int j = 0; j < FOREST_RPT; j++) {
        const bool end = p[j] & FOREST_END;
        q[j] = end ? p[j] : S.lp[p[j]];
        tq[j] = end ? th[j] : max(th[j], S.th[p[j] & FOREST_CELL]);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < FOREST_RPT; j++) {
        p[j] = q[j];
        th[j] = tq[j];
        moving |= !(q[j] & FOREST_END);
        S.lp[(ly0 + 4 * j) * LPS + lx] = (uint16_t)q[j];
        S.th[(ly0 + 4 * j) * LPS + lx] = tq[j];
      }
      if (!__syncthreads_or(moving)) break;
    }
  }
  const int slot = (int)threadIdx.x;
  unsigned long long word = BR_NONE;
  if (slot < BORDER_SLOTS) {
    int bx, by, tx, ty;
    border_cell(slot, bx, by);
    const uint32_t rp = S.lp[by * LPS + bx], root = rp & FOREST_CELL;
    if (rp & FOREST_END) {
      const int ry = (int)root / LPS, rx = (int)root - ry * LPS;
      if (forest_link(S.sd, nodata, rx, ry, tx, ty) == 2) {   // (the target participates: it lies inside the raster)
        const uint32_t a = max(S.th[by * LPS + bx], br_thr<T>(dem[(size_t)(y0 + ty) * w + (x0 + tx)]));
        word = ((unsigned long long)a << 32) | tile_node(x0 + tx, y0 + ty, tilesX);
      }
    }
  }
  nxt0[(size_t)t * TILE_SLOTS + slot] = word;
}

// One doubling round over the nodes, from src into dst (never in place); a node pushes its word across its link iff the
// word passes the link's span threshold.  Returns at once when *gate == 0.  flag_out: a word was raised.
template <class W, uint32_t BIAS>
__global__ __launch_bounds__(NTHR) void k_br_round(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst,
                                                   W *nval, uint32_t nnodes, const uint32_t *__restrict__ gate, uint32_t *flag_out) {
  if (*gate == 0) return;
  bool flag = false;
  for (uint32_t i = blockIdx.x * NTHR + threadIdx.x; i < nnodes; i += gridDim.x * NTHR) {   // (nnodes: a multiple of NTHR)
    const unsigned long long u = src[i];
    const uint32_t n = (uint32_t)u, a = (uint32_t)(u >> 32);
    unsigned long long out = BR_NONE;
    if (n < nnodes) {
      const unsigned long long v = src[n];
      if ((uint32_t)v < nnodes) out = ((unsigned long long)max(a, (uint32_t)(v >> 32)) << 32) | (uint32_t)v;
      const W k = __hip_atomic_load(&nval[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k != 0 && (uint32_t)(k - BIAS) >= a) flag |= atomicMax(&nval[n], k) < k;
    }
    dst[i] = out;
  }
  if (__any(flag) && (threadIdx.x & 63) == 0) *flag_out = 1;
}

// ---- the closure inside a tile --------------------------------------------------------------------------------------------
template <class W>
struct BrTile {
  uint8_t sd[SDH * SDW] __attribute__((aligned(8)));
  uint16_t lp[LT * LPS];   // no end flag here: an end cell points at itself
  uint32_t th[LT * LPS];   // the span threshold of that pointer (an end: 0)
  W word[LT * LPS] __attribute__((aligned(8)));
};

// BR_SEED:  words = the pits' own; closed in the tile; an exit cell whose word enters its target raises the target's node.
// BR_WRITE: words = the pits' own and the node words of the tile's border slots; closed in the tile; decoded and written.
template <class T, int MODE>
__global__ __launch_bounds__(NTHR, (sizeof(typename BrWord<T>::type) == 8 ? 2 : 3)) void k_br_close(
    const uint8_t *__restrict__ dirs, uint8_t nodata, const T *__restrict__ dem, const uint8_t *__restrict__ pits, int w, int h,
    uint32_t tilesX, uint32_t ntiles, typename BrWord<T>::type *nval, uint32_t *exit_out, T *__restrict__ out,
    uint8_t *__restrict__ path) {
  typedef typename BrWord<T>::type W;
  constexpr uint32_t BIAS = BrWord<T>::BIAS;
  __shared__ BrTile<W> S;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, S.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t a[FOREST_RPT];
  uint32_t pitmask = 0;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int gx = x0 + lx, gy = y0 + ly0 + 4 * j;
    a[j] = 0;
    if (gx < w && gy < h) {
      const size_t g = (size_t)gy * w + gx;
      a[j] = br_thr<T>(dem[g]);
      bool pit = pits[g] != 0;
      if constexpr (std::is_same<T, float>::value) pit = pit && a[j] != BR_BLOCK;   // a NaN cell is never a pit
      pitmask |= (pit ? 1u : 0u) << j;
    }
  }
  __syncthreads();
  uint32_t p[FOREST_RPT], th[FOREST_RPT];
  uint32_t exitmask = 0;
  bool any = false;
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int kind = forest_link(S.sd, nodata, lx, ly, tx, ty);
    W k = (kind >= 0 && (pitmask >> j & 1u)) ? (W)a[j] + BIAS : (W)0;   // (a cell that does not participate is never a pit)
    if (MODE == BR_WRITE && kind >= 0) {
      const int slot = border_slot(lx, ly);
      if (slot >= 0) {   // what the rounds brought to this entry cell has passed its threshold already
        const W nk = nval[(size_t)t * TILE_SLOTS + slot];
        k = nk > k ? nk : k;
      }
    }
    p[j] = kind == 1 ? (uint32_t)(ty * LPS + tx) : self;
    exitmask |= (kind == 2 ? 1u : 0u) << j;
    S.lp[self] = (uint16_t)p[j];
    S.th[self] = a[j];
    S.word[self] = k;
    any |= k != 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) th[j] = p[j] != (uint32_t)((ly0 + 4 * j) * LPS + lx) ? S.th[p[j]] : 0u;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) S.th[(ly0 + 4 * j) * LPS + lx] = th[j];
  // forest_close with the thresholds: round r pushes by 2^r, across a pointer only what passes its span; pointer and
  // threshold are read together before the barrier and stored together behind it.  A round that raises nothing has closed
  // the words.
  if (__syncthreads_or(any)) {
    uint32_t q[FOREST_RPT], tq[FOREST_RPT];
#pragma unroll 1
    for (int it = 0; it < FOREST_JUMPS; it++) {
      bool fresh = false;
#pragma unroll
      for (int j = 0; j < FOREST_RPT; j++) {
        q[j] = S.lp[p[j]];
        tq[j] = max(th[j], S.th[p[j]]);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < FOREST_RPT; j++) {
        const uint32_t self = (uint32_t)((ly0 + 4 * j) * LPS + lx);
        if (p[j] != self) {
          const W k = __hip_atomic_load(&S.word[self], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (k != 0 && (uint32_t)(k - BIAS) >= th[j]) fresh |= atomicMax(&S.word[p[j]], k) < k;
        }
        S.lp[self] = (uint16_t)q[j];
        S.th[self] = tq[j];
      }
      if (!__syncthreads_or(fresh)) break;
#pragma unroll
      for (int j = 0; j < FOREST_RPT; j++) {
        p[j] = q[j];
        th[j] = tq[j];
      }
    }
  }
  if (MODE == BR_SEED) {
    bool pushed = false;
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      if (!(exitmask >> j & 1u)) continue;
      const int ly = ly0 + 4 * j;
      const W k = S.word[ly * LPS + lx];
      if (k == 0) continue;
      int tx, ty;
      forest_link(S.sd, nodata, lx, ly, tx, ty);   // (the target participates: it lies inside the raster)
      if ((uint32_t)(k - BIAS) < br_thr<T>(dem[(size_t)(y0 + ty) * w + (x0 + tx)])) continue;
      atomicMax(&nval[tile_node(x0 + tx, y0 + ty, tilesX)], k);
      pushed = true;
    }
    if (__any(pushed) && (threadIdx.x & 63) == 0) *exit_out = 1;
  } else {
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      const int ly = ly0 + 4 * j, gx = x0 + lx, gy = y0 + ly;
      if (gx >= w || gy >= h) continue;
      const W k = S.word[ly * LPS + lx];
      const size_t g = (size_t)gy * w + gx;
      if (out) {
        if (k != 0) br_store_bits<T>(out + g, br_unord<T>(~(uint32_t)(k - BIAS)));
        else out[g] = dem[g];
      }
      if (path) path[g] = k != 0 ? 1 : 0;
    }
  }
}

// ---- the carve's drivers ---------------------------------------------------------------------------------------------------
static void br_check_args(const void *dirs, const void *dem, const void *pits, int w, int h, const void *out, const void *path,
                          const char *who) {
  if (!dirs || !dem || !pits) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  if (!out && !path) throw Error(RDGPU_ERR_ARG, std::string(who) + ": no output requested");
  check_forest_dims(w, h, who);
}

// arguments checked by the caller; d_out may be d_dem's twin but not d_dem itself (the exits read their targets' levels)
template <class T>
static void breach_along_device(const uint8_t *d_dirs, uint8_t nodata, const T *d_dem, const uint8_t *d_pits, int w, int h, T *d_out,
                                uint8_t *d_path, hipStream_t s) {
  typedef typename BrWord<T>::type W;
  constexpr uint32_t BIAS = BrWord<T>::BIAS;
  const ForestDims fd(w, h);
  const uint32_t tilesX = fd.tilesX, ntiles = fd.ntiles, nnodes = (uint32_t)fd.nnodes;
  const int rounds = forest_rounds(nnodes);
  Workspace &ws = Workspace::get();
  unsigned long long *pp[2] = {ws.buf<unsigned long long>("breach.nxt_a", nnodes), ws.buf<unsigned long long>("breach.nxt_b", nnodes)};
  W *nval = ws.buf<W>("breach.nval", nnodes);
  // flags: [0] the seed pass raised a node word | [1 + r] round r raised one
  uint32_t *flags = ws.buf<uint32_t>("breach.flags", (size_t)rounds + 1);
  RD_HIP(hipMemsetAsync(flags, 0, ((size_t)rounds + 1) * sizeof(uint32_t), s));
  RD_HIP(hipMemsetAsync(nval, 0, (size_t)nnodes * sizeof(W), s));
  const uint32_t rgrid = std::min<uint32_t>(ntiles, 2048u);
  RD_LAUNCH("breach.links", (k_br_links<T>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_dem, w, h, tilesX, ntiles, pp[0]);
  RD_LAUNCH("breach.seed", (k_br_close<T, BR_SEED>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_dem, d_pits, w, h, tilesX,
            ntiles, nval, flags, (T *)nullptr, (uint8_t *)nullptr);
  for (int r = 0; r < rounds; r++)
    RD_LAUNCH("breach.round", (k_br_round<W, BIAS>), dim3(rgrid), dim3(NTHR), 0, s, (const unsigned long long *)pp[r & 1], pp[(r + 1) & 1],
              nval, nnodes, (const uint32_t *)(flags + r), flags + r + 1);
  RD_LAUNCH("breach.write", (k_br_close<T, BR_WRITE>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, d_dem, d_pits, w, h,
            tilesX, ntiles, nval, (uint32_t *)nullptr, d_out, d_path);
}

template <class T>
static void breach_along_host(const uint8_t *dirs, uint8_t nodata, const T *dem, const uint8_t *pits, int w, int h, T *out, uint8_t *path,
                              const char *who) {
  br_check_args(dirs, dem, pits, w, h, out, path, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  const T *dz = st.in("host.dem", dem, n);
  const uint8_t *dp = st.in("host.breach.pits", pits, n);
  T *dout = st.out("host.breach.out", out, n);
  uint8_t *dpath = st.out("host.breach.path", path, n);
  breach_along_device<T>(dd, nodata, dz, dp, w, h, dout, dpath, nullptr);
  st.finish();
}

// ---- CompleteBreaching_Lindsay2016<D8> ---------------------------------------------------------------------------------------
static thread_local rdgpu_breach_stats g_breach_stats = {0, 0, 0, 0, 0, 0};

template <class T>
__device__ __forceinline__ bool br_eq_nodata(T v, T nodata) { return v == nodata; }

// cells equal to NoData (striped counter)
template <class T>
__global__ __launch_bounds__(NTHR) void k_br_count_nodata(const T *__restrict__ z, T nodata, uint64_t n, unsigned long long *count) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  uint32_t c0 = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) c0 += br_eq_nodata<T>(z[c], nodata) ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) c0 += __shfl_down(c0, o, 64);
  if ((threadIdx.x & 63) == 0 && c0) atomicAdd(count, (unsigned long long)c0);
}

// The reference's pit pass (:78-123) as a stencil.  It runs in raster order and in place, but no two adjacent cells can each
// be strictly below all their neighbours, and a raised cell never ends above a neighbour:
//   d1(c) = min_n z(n) where c is interior and z(c) < min_n z(n) (the minimum starts at the type's largest finite value, as the
//           reference's does), else z(c);
//   pit(c) <=> c is interior and z(c) <= min(d1 of the neighbours that precede c in raster order, z of those that follow).
template <class T>
__device__ __forceinline__ T br_d1(const T *__restrict__ z, int x, int y, int w, int h) {
  const T e = z[(size_t)y * w + x];
  if (x == 0 || y == 0 || x == w - 1 || y == h - 1) return e;
  T lo = std::numeric_limits<T>::max();
#pragma unroll
  for (int k = 1; k <= 8; k++) {
    const T v = z[(size_t)(y + d8dy(k)) * w + (x + d8dx(k))];
    lo = v < lo ? v : lo;
  }
  return e < lo ? lo : e;
}
template <class T>
__global__ __launch_bounds__(NTHR) void k_br_pits(const T *__restrict__ z, T *__restrict__ d1, uint8_t *__restrict__ pits, int w, int h,
                                                  unsigned long long *counts /* [0] pits, [1] cells raised */) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  uint32_t np = 0, nr = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    const T e = z[c];
    const T own = br_d1<T>(z, x, y, w, h);
    bool pit = false;
    if (x > 0 && y > 0 && x < w - 1 && y < h - 1) {
      T lo = std::numeric_limits<T>::max();
#pragma unroll
      for (int k = 1; k <= 8; k++) {
        const int nx = x + d8dx(k), ny = y + d8dy(k);
        const bool before = ny < y || (ny == y && nx < x);
        const T v = before ? br_d1<T>(z, nx, ny, w, h) : z[(size_t)ny * w + nx];
        lo = v < lo ? v : lo;
      }
      pit = e <= lo;
    }
    T store = own;
    if constexpr (std::is_same<T, float>::value) {
      if (own == 0.0f) store = 0.0f;   // the reference compares -0 == +0; the carve orders by bits: one zero from here on
    }
    d1[c] = store;
    pits[c] = pit ? 1 : 0;
    np += pit;
    nr += !(own == e);
  }
  for (int o = 32; o > 0; o >>= 1) { np += __shfl_down(np, o, 64); nr += __shfl_down(nr, o, 64); }
  if ((threadIdx.x & 63) == 0 && np) atomicAdd(&counts[0], (unsigned long long)np);
  if ((threadIdx.x & 63) == 0 && nr) atomicAdd(&counts[1], (unsigned long long)nr);
}

// the edge cells are the flood's seeds: no back link.  And the cells the carve lowered.
template <class T>
__global__ __launch_bounds__(NTHR) void k_br_finish(uint8_t *dirs, const T *__restrict__ d1, const T *__restrict__ out, int w, int h,
                                                    unsigned long long *counts /* [2] cells lowered */) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  uint32_t nl = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    if (dirs && (x == 0 || y == 0 || x == w - 1 || y == h - 1)) dirs[c] = 0;
    nl += out[c] < d1[c];
  }
  for (int o = 32; o > 0; o >>= 1) nl += __shfl_down(nl, o, 64);
  if ((threadIdx.x & 63) == 0 && nl) atomicAdd(&counts[2], (unsigned long long)nl);
}

static inline uint32_t br_sgrid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 64u); }

static void breach_check_args(const void *dem, int w, int h, const char *who) {
  if (!dem) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, std::string(who) + ": width and height must be positive");
  if ((uint64_t)w * (uint64_t)h > 0x7FFF0000ull) throw Error(RDGPU_ERR_ARG, std::string(who) + ": raster too large");
}

// arguments checked by the caller.  Synchronises the stream (the flood's tree is iterated from the host).
template <class T>
static void breach_device(T *d_dem, T nodata, int has_nodata, int w, int h, uint8_t *d_dirs_out, uint8_t *d_path_out, hipStream_t s,
                          const char *who) {
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  g_breach_stats = rdgpu_breach_stats{0, 0, 0, 0, 0, 0};
  unsigned long long *counts = ws.buf<unsigned long long>("breach.counts", 4);
  RD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), s));
  unsigned long long hc[4] = {0, 0, 0, 0};
  if (has_nodata) {
    RD_LAUNCH("breach.count_nodata", (k_br_count_nodata<T>), dim3(br_sgrid(n)), dim3(NTHR), 0, s, (const T *)d_dem, nodata, n, counts + 3);
    RD_HIP(hipMemcpyAsync(hc + 3, counts + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    if (hc[3] != 0)
      throw Error(RDGPU_ERR_UNSUPPORTED, std::string(who) + ": the raster holds NoData cells; breaching with NoData cells as outlets is not built");
  }
  if (w < 3 || h < 3) {   // no interior cell: nothing is a pit
    if (d_dirs_out) RD_HIP(hipMemsetAsync(d_dirs_out, 0, n, s));
    if (d_path_out) RD_HIP(hipMemsetAsync(d_path_out, 0, n, s));
    return;
  }
  T *d1 = ws.buf<T>("breach.d1", n);
  uint8_t *pits = ws.buf<uint8_t>("breach.pits", n);
  uint8_t *dirs = d_dirs_out ? d_dirs_out : ws.buf<uint8_t>("breach.dirs", n);
  RD_LAUNCH("breach.pits", (k_br_pits<T>), dim3(br_sgrid(n)), dim3(NTHR), 0, s, (const T *)d_dem, d1, pits, w, h, counts);
  rdgpu_pf_flowdirs_stats ts;
  pfd::pf_tree_device<T>(d1, w, h, dirs, pfd::PFD_CONV_LINDSAY, s, &ts);
  breach_along_device<T>(dirs, 255, d1, pits, w, h, d_dem, d_path_out, s);
  RD_LAUNCH("breach.finish", (k_br_finish<T>), dim3(br_sgrid(n)), dim3(NTHR), 0, s, d_dirs_out, (const T *)d1, (const T *)d_dem, w, h, counts);
  RD_HIP(hipMemcpyAsync(hc, counts, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  g_breach_stats.pits = hc[0];
  g_breach_stats.raised = hc[1];
  g_breach_stats.lowered = hc[2];
  g_breach_stats.unresolved = ts.unresolved;
  g_breach_stats.twins = ts.twins;
  g_breach_stats.tie_passes = ts.tie_passes;
}

template <class T>
static void breach_host(T *dem, T nodata, int has_nodata, int w, int h, uint8_t *dirs_out, uint8_t *path_out, const char *who) {
  breach_check_args(dem, w, h, who);
  const size_t n = (size_t)w * h;
  HostStage st;
  T *dz = st.inout("host.dem", dem, n);
  uint8_t *dd = st.out("host.dirs", dirs_out, n);
  uint8_t *dp = st.out("host.breach.path", path_out, n);
  breach_device<T>(dz, nodata, has_nodata, w, h, dd, dp, nullptr, who);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_DEFINE_BREACH(SUF, T)                                                                                                       \
  extern "C" int rdgpu_d8_breach_along_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const T *dem, const uint8_t *pits, int width,   \
                                             int height, T *out, uint8_t *path) {                                                     \
    return guarded([&] { breach_along_host<T>(dirs, dir_nodata, dem, pits, width, height, out, path, "rdgpu_d8_breach_along_" #SUF); }); \
  }                                                                                                                                    \
  extern "C" int rdgpu_d8_breach_along_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const T *d_dem, const uint8_t *d_pits,    \
                                                 int width, int height, T *d_out, uint8_t *d_path, void *hip_stream) {                \
    return guarded([&] {                                                                                                               \
      br_check_args(d_dirs, d_dem, d_pits, width, height, d_out, d_path, "rdgpu_d8_breach_along_dev_" #SUF);                          \
      if (d_out == d_dem) throw Error(RDGPU_ERR_ARG, "rdgpu_d8_breach_along_dev_" #SUF ": out must not be the dem itself");           \
      breach_along_device<T>(d_dirs, dir_nodata, d_dem, d_pits, width, height, d_out, d_path, (hipStream_t)hip_stream);               \
    });                                                                                                                                \
  }                                                                                                                                    \
  extern "C" int rdgpu_breach_d8_##SUF(T *dem, T nodata, int has_nodata, int width, int height, uint8_t *dirs_out, uint8_t *path_out) { \
    return guarded([&] { breach_host<T>(dem, nodata, has_nodata, width, height, dirs_out, path_out, "rdgpu_breach_d8_" #SUF); });     \
  }                                                                                                                                    \
  extern "C" int rdgpu_breach_d8_dev_##SUF(T *d_dem, T nodata, int has_nodata, int width, int height, uint8_t *d_dirs_out,            \
                                           uint8_t *d_path_out, void *hip_stream) {                                                   \
    return guarded([&] {                                                                                                               \
      breach_check_args(d_dem, width, height, "rdgpu_breach_d8_dev_" #SUF);                                                           \
      breach_device<T>(d_dem, nodata, has_nodata, width, height, d_dirs_out, d_path_out, (hipStream_t)hip_stream,                     \
                       "rdgpu_breach_d8_dev_" #SUF);                                                                                  \
    });                                                                                                                                \
  }
RD_DEFINE_BREACH(i8, int8_t)
RD_DEFINE_BREACH(u8, uint8_t)
RD_DEFINE_BREACH(i16, int16_t)
RD_DEFINE_BREACH(u16, uint16_t)
RD_DEFINE_BREACH(i32, int32_t)
RD_DEFINE_BREACH(u32, uint32_t)
RD_DEFINE_BREACH(f32, float)
#undef RD_DEFINE_BREACH

extern "C" int rdgpu_breach_get_stats(rdgpu_breach_stats *out) {
  if (!out) return RDGPU_ERR_ARG;
  *out = rdgpu::g_breach_stats;
  return 0;
}
