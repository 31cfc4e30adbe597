// dephier.hip -- the depression hierarchy: the binary merge tree of the leaf depressions, a leaf label per cell, and per
// node its spill pair, level, cells and volume (include/rdgpu.h, "depression hierarchy").
// Reference counterpart: depressions/depression_hierarchy.hpp (GetDepressionHierarchy, CalculateMarginalVolumes,
// CalculateTotalVolumes); the contract in rdgpu.h fixes every tie the reference leaves to its pop order.
//
// The descent is this file's own.  The fill's local phase (fill_local_phase_plain) numbers its basins in the order its
// tiles finish them, keeps one id for the whole outside and, on its fused path, dissolves pits; the contract wants every
// pit of the plain (value, index) descent and leaves numbered by raster index, so nothing of fb.lab could be kept.
//   k_dh_descent   one raster pass: every interior cell -> its lowest (key, index) neighbour, itself (a pit), or OUTSIDE
//                  on the border ring.  k_dh_descent_ocean is its twin for a caller-given ocean mask: the cells of the mask
//                  drain OUTSIDE, every other cell -- the ring's, with their partial neighbourhoods, included -- descends.
//   k_dh_jump      pointer jumping, eight hops a round, until a round changes nothing.
//   k_dh_flag + an exclusive scan + k_dh_leaf   the leaves, numbered by ascending pit index; ptr[] becomes leaf[] in place.
//   k_dh_edges<0/1>  count, scan, emit: every cell, as the HIGHER cell of an edge, one record per neighbouring leaf (the
//                  lowest-index lower neighbour of that leaf), laid out by cell and by ascending lower cell.
//   a stable radix sort of the records by (key of the higher cell, higher cell): with the layout above that is the
//                  contract's total order (dem[hi], hi, lo).
//   k_dh_ends      the two leaves of every sorted record.
//   k_dh_pairs + a stable sort by pair of leaves + k_dh_heads + a select + a sort of the positions + k_dh_gather
//                  the minimum edge of every pair, in key order: the REDUCED records.  Their two leaves, two words per
//                  record, are what the builder reads.
//   the builder    serial Kruskal on the host over the reduced records (stats.builder = RDGPU_DEPHIER_BUILDER_HOST_KRUSKAL).
//                  It writes parent / children / lowest pit / spill record per node, and the tree's height.
//   k_dh_lift      the binary-lifting table over the parents (ceil(log2(height + 1)) planes).
//   k_dh_charge    one raster pass: a cell is charged to its first ancestor-or-self whose level is not below it, found
//                  by the lifting table (levels do not fall towards the root).
//   k_dh_accum     child-before-parent totals in ONE launch: a thread per leaf climbs, the second arrival at a node
//                  (an agent-scope counter) combines its two children and goes on, the first one leaves.
//   k_dh_table, k_dh_labels   the records and the label raster.
// Volumes: integer element types in 64-bit integers (differences of keys are differences of values).  f32: the marginal
// sums are double atomics in no fixed order; the climb carries double-double totals, so it adds no rounding of its own.
#include "common.hpp"
#include "fill_shared.hpp"

#include <hipcub/hipcub.hpp>

#include <type_traits>

namespace rdgpu {

static_assert(sizeof(rdgpu_dephier_node) == 56, "eight 32-bit words and three doubles, no padding");
static_assert(sizeof(rdgpu_dephier_stats) == 56, "three 64-bit and eight 32-bit words");

constexpr uint32_t DH_NONE = 0xFFFFFFFFu;

// words other workgroups write while this kernel runs: agent scope (the per-XCD L2s are not coherent)
__device__ __forceinline__ uint32_t dh_ld(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void dh_st(uint32_t *p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long dh_ld64(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void dh_st64(unsigned long long *p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the neighbours of a cell in ascending raster index
template <int TOPO>
__device__ __forceinline__ constexpr int dh_dx(int k) {
  constexpr int d8[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, d4[4] = {0, -1, 1, 0};
  return TOPO == 8 ? d8[k & 7] : d4[k & 3];
}
template <int TOPO>
__device__ __forceinline__ constexpr int dh_dy(int k) {
  constexpr int d8[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, d4[4] = {-1, 0, 0, 1};
  return TOPO == 8 ? d8[k & 7] : d4[k & 3];
}

template <class T, int TOPO>
__global__ __launch_bounds__(NTHR) void k_dh_descent(const T *__restrict__ z, uint32_t *__restrict__ ptr, int w, int h) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    if (x == 0 || y == 0 || x == w - 1 || y == h - 1) {
      ptr[c] = DH_NONE;
      continue;
    }
    const unsigned long long self = ((unsigned long long)Key32<T>::to(z[c]) << 32) | c;
    unsigned long long best = self;
#pragma unroll
    for (int k = 0; k < TOPO; k++) {   // (an interior cell: every neighbour is in the raster)
      const uint64_t q = (uint64_t)((int64_t)c + (int64_t)dh_dy<TOPO>(k) * w + dh_dx<TOPO>(k));
      const unsigned long long kq = ((unsigned long long)Key32<T>::to(z[q]) << 32) | q;
      best = kq < best ? kq : best;
    }
    ptr[c] = (uint32_t)best;
  }
}

// The descent for a caller-given ocean: a cell of the mask drains OUTSIDE whatever its value; any other cell looks at the
// neighbours it has inside the raster (a masked neighbour counts by its value like any other).  *oceans: the number of
// masked cells, one add per wavefront that saw any.
template <class T, int TOPO>
__global__ __launch_bounds__(NTHR) void k_dh_descent_ocean(const T *__restrict__ z, const uint8_t *__restrict__ ocean,
                                                         uint32_t *__restrict__ ptr, int w, int h, uint32_t *oceans) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  uint32_t mine = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    if (ocean[c]) {
      ptr[c] = DH_NONE;
      mine++;
      continue;
    }
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    unsigned long long best = ((unsigned long long)Key32<T>::to(z[c]) << 32) | c;
#pragma unroll
    for (int k = 0; k < TOPO; k++) {
      const int xx = x + dh_dx<TOPO>(k), yy = y + dh_dy<TOPO>(k);
      if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
      const uint64_t q = (uint64_t)yy * w + xx;
      const unsigned long long kq = ((unsigned long long)Key32<T>::to(z[q]) << 32) | q;
      best = kq < best ? kq : best;
    }
    ptr[c] = (uint32_t)best;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(oceans, mine);
}

// ptr[c] is always an ancestor of c in the descent forest (or OUTSIDE once the path is known to end there), whatever other
// workgroups have written meanwhile; a round that finds every pointer at a pit or OUTSIDE leaves *changed at 0
__global__ __launch_bounds__(NTHR) void k_dh_jump(uint32_t *ptr, uint64_t n, uint32_t *changed) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  bool any = false;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    uint32_t p = dh_ld(&ptr[c]);
    if (p == DH_NONE || p == (uint32_t)c) continue;
    const uint32_t p0 = p;
    bool done = false;
    for (int k = 0; k < 8; k++) {
      const uint32_t q = dh_ld(&ptr[p]);
      if (q == p) { done = true; break; }
      p = q;
      if (q == DH_NONE) { done = true; break; }
    }
    if (p != p0) dh_st(&ptr[c], p);
    any |= !done;
  }
  if (__ballot(any) && (threadIdx.x & 63) == 0) dh_st(changed, 1u);
}

__global__ __launch_bounds__(NTHR) void k_dh_flag(const uint32_t *__restrict__ ptr, uint32_t *__restrict__ rank, uint64_t n,
                                                  uint32_t *pits) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  uint32_t mine = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t f = ptr[c] == (uint32_t)c ? 1u : 0u;
    rank[c] = f;
    mine += f;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(pits, mine);
}

// ptr[c] (the pit of c, or OUTSIDE) -> the pit's leaf id, in place: a thread reads no word of ptr but its own
template <class T>
__global__ __launch_bounds__(NTHR) void k_dh_leaf(const T *__restrict__ z, uint32_t *ptr, const uint32_t *__restrict__ rank,
                                                  uint32_t *__restrict__ pitcell, uint32_t *__restrict__ pitkey, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t p = ptr[c];
    if (p == DH_NONE) continue;
    const uint32_t l = rank[p];
    if (p == (uint32_t)c) {
      pitcell[l] = p;
      pitkey[l] = Key32<T>::to(z[c]);
    }
    ptr[c] = l;
  }
}

// Cell c as the higher cell of an edge: a neighbour q that is lower under (key, index) and lies in another leaf.  Of the
// neighbours in one leaf the first in the list -- the lowest index -- dominates the others.  EMIT == 0: off[c] = the
// number of records and the two totals; EMIT == 1: the records, at off[c] (scanned), by ascending q.
template <class T, int TOPO, int EMIT>
__global__ __launch_bounds__(NTHR) void k_dh_edges(const T *__restrict__ z, const uint32_t *__restrict__ leaf, uint32_t *off,
                                                   unsigned long long *__restrict__ keys, uint32_t *__restrict__ lo, int w,
                                                   int h, unsigned long long *totals) {
  const uint64_t n = (uint64_t)w * h, stride = (uint64_t)gridDim.x * NTHR;
  uint32_t kept = 0, raw = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int x = (int)(c % (uint64_t)w), y = (int)(c / (uint64_t)w);
    const uint32_t lc = leaf[c];
    const unsigned long long self = ((unsigned long long)Key32<T>::to(z[c]) << 32) | c;
    uint32_t seen[TOPO];
    uint32_t m = 0;
    const uint32_t base = EMIT ? off[c] : 0u;
#pragma unroll
    for (int k = 0; k < TOPO; k++) {
      const int xx = x + dh_dx<TOPO>(k), yy = y + dh_dy<TOPO>(k);
      if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
      const uint64_t q = (uint64_t)yy * w + xx;
      const uint32_t lq = leaf[q];
      if (lq == lc) continue;
      const unsigned long long kq = ((unsigned long long)Key32<T>::to(z[q]) << 32) | q;
      if (!(kq < self)) continue;
      raw++;
      bool dup = false;
#pragma unroll
      for (int j = 0; j < TOPO; j++) dup |= j < (int)m && seen[j] == lq;
      if (dup) continue;
#pragma unroll
      for (int j = 0; j < TOPO; j++)
        if (j == (int)m) seen[j] = lq;
      if (EMIT) {
        keys[(uint64_t)base + m] = self;
        lo[(uint64_t)base + m] = (uint32_t)q;
      }
      m++;
    }
    if (!EMIT) {
      off[c] = m;
      kept += m;
    }
  }
  if (!EMIT) {
    unsigned long long a = kept, b = raw;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      a += __shfl_down(a, d, 64);
      b += __shfl_down(b, d, 64);
    }
    if ((threadIdx.x & 63) == 0 && b) {
      atomicAdd(&totals[0], a);
      atomicAdd(&totals[1], b);
    }
  }
}

__global__ __launch_bounds__(NTHR) void k_dh_ends(const unsigned long long *__restrict__ skeys, const uint32_t *__restrict__ slo,
                                                  const uint32_t *__restrict__ leaf, uint32_t *__restrict__ ea,
                                                  uint32_t *__restrict__ eb, uint32_t E) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= E) return;
  ea[i] = leaf[(uint32_t)skeys[i]];
  eb[i] = leaf[slo[i]];
}

// the pair of leaves of a sorted record (the outside is leaf P), lower id first, and the record's sorted position
__global__ __launch_bounds__(NTHR) void k_dh_pairs(const uint32_t *__restrict__ ea, const uint32_t *__restrict__ eb,
                                                   unsigned long long *__restrict__ pk, uint32_t *__restrict__ idx, uint32_t E,
                                                   uint32_t P) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= E) return;
  const uint32_t a = ea[i] == DH_NONE ? P : ea[i], b = eb[i] == DH_NONE ? P : eb[i];
  pk[i] = ((unsigned long long)(a < b ? a : b) << 32) | (a < b ? b : a);
  idx[i] = i;
}

// after the stable sort by pair: the first record of a run is the pair's minimum edge
__global__ __launch_bounds__(NTHR) void k_dh_heads(const unsigned long long *__restrict__ spk, uint8_t *__restrict__ head, uint32_t E) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= E) return;
  head[i] = (i == 0 || spk[i] != spk[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(NTHR) void k_dh_gather(const uint32_t *__restrict__ pos, const unsigned long long *__restrict__ skeys,
                                                    const uint32_t *__restrict__ slo, const uint32_t *__restrict__ ea,
                                                    const uint32_t *__restrict__ eb, unsigned long long *__restrict__ rkeys,
                                                    uint32_t *__restrict__ rlo, uint32_t *__restrict__ rea,
                                                    uint32_t *__restrict__ reb, uint32_t R) {
  const uint32_t j = blockIdx.x * NTHR + threadIdx.x;
  if (j >= R) return;
  const uint32_t i = pos[j];
  rkeys[j] = skeys[i];
  rlo[j] = slo[i];
  rea[j] = ea[i];
  reb[j] = eb[i];
}

// what the builder hands back per node: spill = (index of the sorted record << 1) | (1: the node's side is the higher cell)
__global__ __launch_bounds__(NTHR) void k_dh_nodes(const uint32_t *__restrict__ spill, const unsigned long long *__restrict__ skeys,
                                                   uint32_t *__restrict__ lvl, uint32_t *__restrict__ arrive,
                                                   uint32_t *__restrict__ mc, unsigned long long *__restrict__ mv, uint32_t count) {
  const uint32_t v = blockIdx.x * NTHR + threadIdx.x;
  if (v >= count) return;
  lvl[v] = (uint32_t)(skeys[spill[v] >> 1] >> 32);
  arrive[v] = 0;
  mc[v] = 0;
  mv[v] = 0ull;
}

// plane j of the lifting table: the ancestor 2^j steps up, DH_NONE past the root (plane 0 is the parents)
__global__ __launch_bounds__(NTHR) void k_dh_lift(const uint32_t *__restrict__ prev, uint32_t *__restrict__ next, uint32_t count) {
  const uint32_t v = blockIdx.x * NTHR + threadIdx.x;
  if (v >= count) return;
  const uint32_t u = prev[v];
  next[v] = u == DH_NONE ? DH_NONE : prev[u];
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_dh_charge(const T *__restrict__ z, const uint32_t *__restrict__ leaf,
                                                    const uint32_t *__restrict__ up, const uint32_t *__restrict__ lvl,
                                                    uint32_t *mc, unsigned long long *mv, uint64_t n, uint32_t count, int planes) {
  constexpr bool INTEGER = std::is_integral<T>::value;
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    uint32_t v = leaf[c];
    if (v == DH_NONE) continue;
    const T zc = z[c];
    const uint32_t k = Key32<T>::to(zc);
    if (lvl[v] < k) {
      // the highest ancestor-or-self still below the cell, then one step more
      for (int j = planes - 1; j >= 0; j--) {
        const uint32_t u = up[(size_t)j * count + v];
        if (u != DH_NONE && lvl[u] < k) v = u;
      }
      v = up[v];
      if (v == DH_NONE) continue;   // above the spill of its top-level depression: in no depression
    }
    const uint32_t L = lvl[v];
    atomicAdd(&mc[v], 1u);
    if (INTEGER) atomicAdd(&mv[v], (unsigned long long)(L - k));
    else atomicAdd(reinterpret_cast<double *>(&mv[v]), (double)Key32<T>::from(L) - (double)zc);
  }
}

// double-double sums for the climb (-ffp-contract=off: the error terms below stay as written)
struct DD { double h, l; };
__device__ __forceinline__ DD dd_add(DD a, DD b) {
  const double s = a.h + b.h, bb = s - a.h;
  double e = (a.h - (s - bb)) + (b.h - bb);
  e += a.l + b.l;
  const double hi = s + e;
  return DD{hi, e - (hi - s)};
}
__device__ __forceinline__ DD dd_mul(double a, double b) {
  const double p = a * b;
  return DD{p, __builtin_fma(a, b, -p)};
}

// totals[v] = the node's own charge + its children's, the children's volumes lifted to the node's level.  A thread per
// leaf; at a node the first arrival leaves and the second -- which sees both children's totals: release by the fence
// before the counter, acquire by the fence after it -- combines them and climbs on.  No thread waits for another.
template <class T>
__global__ __launch_bounds__(NTHR) void k_dh_accum(const uint32_t *__restrict__ par, const uint32_t *__restrict__ lch,
                                                   const uint32_t *__restrict__ rch, const uint32_t *__restrict__ lvl,
                                                   const uint32_t *__restrict__ mc, const unsigned long long *__restrict__ mv,
                                                   uint32_t *tc, unsigned long long *tvh, unsigned long long *tvl,
                                                   uint32_t *arrive, uint32_t P) {
  constexpr bool INTEGER = std::is_integral<T>::value;
  uint32_t v = blockIdx.x * NTHR + threadIdx.x;
  if (v >= P) return;
  dh_st(&tc[v], mc[v]);
  dh_st64(&tvh[v], mv[v]);
  dh_st64(&tvl[v], 0ull);
  for (;;) {
    const uint32_t p = par[v];
    if (p == DH_NONE) return;
    __threadfence();
    if (__hip_atomic_fetch_add(&arrive[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
    __threadfence();
    const uint32_t a = lch[p], b = rch[p];
    const uint32_t ca = dh_ld(&tc[a]), cb = dh_ld(&tc[b]);
    const uint32_t Lp = lvl[p], La = lvl[a], Lb = lvl[b];
    dh_st(&tc[p], mc[p] + ca + cb);
    if (INTEGER) {
      const unsigned long long t = mv[p] + dh_ld64(&tvh[a]) + (unsigned long long)ca * (unsigned long long)(Lp - La) +
                                   dh_ld64(&tvh[b]) + (unsigned long long)cb * (unsigned long long)(Lp - Lb);
      dh_st64(&tvh[p], t);
      dh_st64(&tvl[p], 0ull);
    } else {
      const double dp = (double)Key32<T>::from(Lp);
      DD t{__builtin_bit_cast(double, mv[p]), 0.0};
      t = dd_add(t, DD{__builtin_bit_cast(double, dh_ld64(&tvh[a])), __builtin_bit_cast(double, dh_ld64(&tvl[a]))});
      t = dd_add(t, dd_mul((double)ca, dp - (double)Key32<T>::from(La)));
      t = dd_add(t, DD{__builtin_bit_cast(double, dh_ld64(&tvh[b])), __builtin_bit_cast(double, dh_ld64(&tvl[b]))});
      t = dd_add(t, dd_mul((double)cb, dp - (double)Key32<T>::from(Lb)));
      dh_st64(&tvh[p], __builtin_bit_cast(unsigned long long, t.h));
      dh_st64(&tvl[p], __builtin_bit_cast(unsigned long long, t.l));
    }
    v = p;
  }
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_dh_table(const T *__restrict__ z, const uint32_t *__restrict__ leaf,
                                                   const uint32_t *__restrict__ par, const uint32_t *__restrict__ lch,
                                                   const uint32_t *__restrict__ rch, const uint32_t *__restrict__ pitleaf,
                                                   const uint32_t *__restrict__ spill, const uint32_t *__restrict__ pitcell,
                                                   const unsigned long long *__restrict__ skeys, const uint32_t *__restrict__ slo,
                                                   const uint32_t *__restrict__ tc, const unsigned long long *__restrict__ tvh,
                                                   const unsigned long long *__restrict__ tvl, rdgpu_dephier_node *table,
                                                   uint32_t written) {
  constexpr bool INTEGER = std::is_integral<T>::value;
  const uint32_t v = blockIdx.x * NTHR + threadIdx.x;
  if (v >= written) return;
  const uint32_t sp = spill[v], e = sp >> 1;
  const uint32_t hi = (uint32_t)skeys[e], lo = slo[e];
  rdgpu_dephier_node d;
  d.parent = par[v];
  d.lchild = lch[v];
  d.rchild = rch[v];
  d.pit_cell = pitcell[pitleaf[v]];
  d.inside_cell = (sp & 1u) ? hi : lo;
  d.outside_cell = (sp & 1u) ? lo : hi;
  d.geolink = leaf[d.outside_cell];
  d.cells = tc[v];
  d.level = (double)z[hi];
  d.pit_elevation = (double)z[d.pit_cell];
  d.volume = INTEGER ? (double)tvh[v] : __builtin_bit_cast(double, tvh[v]) + __builtin_bit_cast(double, tvl[v]);
  table[v] = d;
}

__global__ __launch_bounds__(NTHR) void k_dh_labels(const uint32_t *__restrict__ leaf, int32_t *__restrict__ labels, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) labels[c] = (int32_t)leaf[c];   // OUTSIDE is -1
}

__global__ void k_dh_counts(uint32_t *count, uint32_t *leaves, uint32_t nodes, uint32_t pits) {
  if (count) *count = nodes;
  if (leaves) *leaves = pits;
}

static thread_local rdgpu_dephier_stats dh_last = {};

// ---- the builder: serial Kruskal over the sorted records -------------------------------------------------------------
struct DhTree {
  std::vector<uint32_t> par, lch, rch, pitleaf, spill;
  uint32_t roots = 0, height = 0;
};

static uint32_t dh_find(std::vector<uint32_t> &uf, uint32_t x) {
  uint32_t r = x;
  while (uf[r] != r) r = uf[r];
  while (uf[x] != r) { const uint32_t nx = uf[x]; uf[x] = r; x = nx; }
  return r;
}

static void dh_kruskal(const std::vector<uint32_t> &ea, const std::vector<uint32_t> &eb, const std::vector<uint32_t> &pitcell,
                       const std::vector<uint32_t> &pitkey, uint32_t P, DhTree &t) {
  const size_t cap = 2 * (size_t)P;
  t.par.assign(cap, DH_NONE); t.lch.assign(cap, DH_NONE); t.rch.assign(cap, DH_NONE); t.pitleaf.resize(cap); t.spill.assign(cap, 0u);
  std::vector<uint32_t> uf(P + 1), top(P + 1);
  for (uint32_t i = 0; i <= P; i++) { uf[i] = i; top[i] = i; }
  for (uint32_t i = 0; i < P; i++) t.pitleaf[i] = i;
  uint32_t count = P, live = P;   // live: sets that have not joined the outside
  const size_t E = ea.size();
  for (size_t i = 0; i < E && live; i++) {
    const uint32_t ra = dh_find(uf, ea[i] == DH_NONE ? P : ea[i]), rb = dh_find(uf, eb[i] == DH_NONE ? P : eb[i]);
    if (ra == rb) continue;
    const uint32_t out = dh_find(uf, P);
    if (ra == out || rb == out) {
      const bool hi_in = rb == out;   // the side that is not the outside becomes a root
      const uint32_t r = hi_in ? ra : rb, A = top[r];
      t.spill[A] = ((uint32_t)i << 1) | (hi_in ? 1u : 0u);
      uf[r] = out;
      t.roots++;
      live--;
      continue;
    }
    const uint32_t A = top[ra], B = top[rb], N = count++;
    t.spill[A] = ((uint32_t)i << 1) | 1u;
    t.spill[B] = (uint32_t)i << 1;
    t.par[A] = t.par[B] = N;
    const uint32_t pa = t.pitleaf[A], pb = t.pitleaf[B];
    const bool a_first = pitkey[pa] != pitkey[pb] ? pitkey[pa] < pitkey[pb] : pitcell[pa] < pitcell[pb];
    t.lch[N] = a_first ? A : B;
    t.rch[N] = a_first ? B : A;
    t.pitleaf[N] = a_first ? pa : pb;
    uf[rb] = ra;
    top[ra] = N;
    live--;
  }
  if (live) throw Error(RDGPU_ERR_HIP, "rdgpu_depression_hierarchy: the edge records do not connect every leaf to the outside");
  t.par.resize(count); t.lch.resize(count); t.rch.resize(count); t.pitleaf.resize(count); t.spill.resize(count);
  // height: a parent's id is above its children's
  std::vector<uint32_t> depth(count, 0u);
  for (uint32_t v = count; v-- > 0;) {
    if (t.par[v] != DH_NONE) depth[v] = depth[t.par[v]] + 1u;
    t.height = std::max(t.height, depth[v]);
  }
}

template <class T>
static void dh_upload(uint32_t *d, const std::vector<T> &v, hipStream_t s) {
  RD_HIP(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
}

template <class T, int TOPO>
static void dephier_device_t(const T *d_z, int w, int h, const uint8_t *d_ocean, int32_t *d_labels, rdgpu_dephier_node *d_table, uint32_t capacity,
                             uint32_t *d_count, uint32_t *d_leaves, hipStream_t s) {
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  rdgpu_dephier_stats st = {};
  st.builder = RDGPU_DEPHIER_BUILDER_HOST_KRUSKAL;
  const uint32_t rgrid = (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u);
  uint32_t *leaf = ws.buf<uint32_t>("dephier.leaf", n), *off = ws.buf<uint32_t>("dephier.off", n);
  // [0] records kept, [1] raw, [2] lo: changed, hi: ocean cells (a masked call), [3] lo: pits
  unsigned long long *words = ws.buf<unsigned long long>("dephier.words", 4);
  uint32_t *changed = reinterpret_cast<uint32_t *>(words + 2), *pits = reinterpret_cast<uint32_t *>(words + 3);
  uint32_t *hw = ws.host_words();

  if (d_ocean) {
    RD_HIP(hipMemsetAsync(changed + 1, 0, sizeof(uint32_t), s));
    RD_LAUNCH("dephier.descent_ocean", (k_dh_descent_ocean<T, TOPO>), dim3(rgrid), dim3(NTHR), 0, s, d_z, d_ocean, leaf, w, h,
              changed + 1);
  } else {
    RD_LAUNCH("dephier.descent", (k_dh_descent<T, TOPO>), dim3(rgrid), dim3(NTHR), 0, s, d_z, leaf, w, h);
  }
  for (;;) {
    RD_HIP(hipMemsetAsync(changed, 0, sizeof(uint32_t), s));
    RD_LAUNCH("dephier.jump", k_dh_jump, dim3(rgrid), dim3(NTHR), 0, s, leaf, n, changed);
    st.jump_rounds++;
    RD_HIP(hipMemcpyAsync(hw, changed, (d_ocean ? 2 : 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));   // (+ the ocean count)
    RD_HIP(hipStreamSynchronize(s));
    if (d_ocean && !hw[1]) throw Error(RDGPU_ERR_ARG, "rdgpu_depression_hierarchy_ocean: no ocean cells");
    if (!hw[0]) break;
    if (st.jump_rounds >= 64) throw Error(RDGPU_ERR_HIP, "rdgpu_depression_hierarchy: the descent paths did not resolve");
  }
  RD_HIP(hipMemsetAsync(words, 0, 4 * sizeof(unsigned long long), s));
  RD_LAUNCH("dephier.flag", k_dh_flag, dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)leaf, off, n, pits);
  RD_HIP(hipMemcpyAsync(hw, pits, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  const uint32_t P = hw[0];
  st.pits = P;
  if (!P) {   // no pit: every cell drains outside
    if (d_labels) RD_HIP(hipMemsetAsync(d_labels, 0xFF, n * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_dh_counts, dim3(1), dim3(1), 0, s, d_count, d_leaves, 0u, 0u);
    RD_HIP(hipGetLastError());
    dh_last = st;
    return;
  }
  size_t tb = 0, tb2 = 0;
  RD_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, off, off, (int)n, s));
  void *tmp = ws.buf("dephier.scan_tmp", tb);
  {
    Profiler &pf = Profiler::get();
    if (pf.enabled) pf.begin("dephier.scan", s);
    RD_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, off, off, (int)n, s));
    if (pf.enabled) pf.end(s);
  }
  uint32_t *pitcell = ws.buf<uint32_t>("dephier.pitcell", P), *pitkey = ws.buf<uint32_t>("dephier.pitkey", P);
  RD_LAUNCH("dephier.leaf", (k_dh_leaf<T>), dim3(rgrid), dim3(NTHR), 0, s, d_z, leaf, (const uint32_t *)off, pitcell, pitkey, n);

  // edges: count, scan, emit, sort
  RD_LAUNCH("dephier.edges_count", (k_dh_edges<T, TOPO, 0>), dim3(rgrid), dim3(NTHR), 0, s, d_z, (const uint32_t *)leaf, off,
            (unsigned long long *)nullptr, (uint32_t *)nullptr, w, h, words);
  unsigned long long *hq = reinterpret_cast<unsigned long long *>(hw);
  RD_HIP(hipMemcpyAsync(hq, words, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  st.cell_pairs = hq[1];
  st.edges_raw = hq[0];
  if (hq[0] > 0x7FFF0000ull) throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_depression_hierarchy: more than 2^31-65536 edge records");
  const uint32_t E = (uint32_t)hq[0];
  {
    Profiler &pf = Profiler::get();
    if (pf.enabled) pf.begin("dephier.scan", s);
    RD_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, off, off, (int)n, s));
    if (pf.enabled) pf.end(s);
  }
  unsigned long long *keys = ws.buf<unsigned long long>("dephier.keys", E), *skeys = ws.buf<unsigned long long>("dephier.skeys", E);
  uint32_t *lo = ws.buf<uint32_t>("dephier.lo", E), *slo = ws.buf<uint32_t>("dephier.slo", E);
  RD_LAUNCH("dephier.edges_emit", (k_dh_edges<T, TOPO, 1>), dim3(rgrid), dim3(NTHR), 0, s, d_z, (const uint32_t *)leaf, off, keys,
            lo, w, h, words);
  RD_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb2, keys, skeys, lo, slo, (int)E, 0, 64, s));
  void *tmp2 = ws.buf("dephier.sort_tmp", tb2);
  {
    Profiler &pf = Profiler::get();
    if (pf.enabled) pf.begin("dephier.sort", s);
    RD_HIP(hipcub::DeviceRadixSort::SortPairs(tmp2, tb2, keys, skeys, lo, slo, (int)E, 0, 64, s));
    if (pf.enabled) pf.end(s);
  }
  uint32_t *ea = reinterpret_cast<uint32_t *>(keys), *eb = lo;   // (the unsorted records are dead after the sort)
  RD_LAUNCH("dephier.ends", k_dh_ends, dim3(cdiv(E, NTHR)), dim3(NTHR), 0, s, (const unsigned long long *)skeys,
            (const uint32_t *)slo, (const uint32_t *)leaf, ea, eb, E);

  // the minimum edge of every pair of leaves: a stable sort by pair keeps the key order inside a pair, the heads of the
  // runs are the minima, and sorting their positions puts them back into key order
  unsigned long long *pk = ws.buf<unsigned long long>("dephier.pairs", E), *spk = ws.buf<unsigned long long>("dephier.spairs", E);
  uint32_t *idx = ws.buf<uint32_t>("dephier.pos", E), *sidx = ws.buf<uint32_t>("dephier.spos", E);
  uint8_t *head = ws.buf<uint8_t>("dephier.head", E);
  RD_LAUNCH("dephier.pairs", k_dh_pairs, dim3(cdiv(E, NTHR)), dim3(NTHR), 0, s, (const uint32_t *)ea, (const uint32_t *)eb, pk, idx, E, P);
  int pbits = 1;
  while ((1ull << pbits) <= (unsigned long long)P) pbits++;
  size_t tb3 = 0, tb4 = 0, tb5 = 0;
  RD_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb3, pk, spk, idx, sidx, (int)E, 0, 32 + pbits, s));
  RD_HIP(hipcub::DeviceSelect::Flagged(nullptr, tb4, sidx, head, idx, pits, (int)E, s));
  RD_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tb5, idx, sidx, (int)E, 0, 32, s));
  void *tmp3 = ws.buf("dephier.reduce_tmp", std::max(tb3, std::max(tb4, tb5)));
  {
    Profiler &pf = Profiler::get();
    if (pf.enabled) pf.begin("dephier.pair_sort", s);
    RD_HIP(hipcub::DeviceRadixSort::SortPairs(tmp3, tb3, pk, spk, idx, sidx, (int)E, 0, 32 + pbits, s));
    if (pf.enabled) pf.end(s);
  }
  RD_LAUNCH("dephier.heads", k_dh_heads, dim3(cdiv(E, NTHR)), dim3(NTHR), 0, s, (const unsigned long long *)spk, head, E);
  RD_HIP(hipcub::DeviceSelect::Flagged(tmp3, tb4, sidx, head, idx, pits, (int)E, s));   // (pits: a free device word by now)
  RD_HIP(hipMemcpyAsync(hw, pits, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  const uint32_t R = hw[0];
  st.edges_reduced = R;
  RD_HIP(hipcub::DeviceRadixSort::SortKeys(tmp3, tb5, idx, sidx, (int)R, 0, 32, s));
  unsigned long long *rkeys = pk;                                   // (the pair keys are dead)
  uint32_t *rlo = ws.buf<uint32_t>("dephier.rlo", R), *rea = ws.buf<uint32_t>("dephier.rea", R), *reb = ws.buf<uint32_t>("dephier.reb", R);
  RD_LAUNCH("dephier.gather", k_dh_gather, dim3(cdiv(R, NTHR)), dim3(NTHR), 0, s, (const uint32_t *)sidx,
            (const unsigned long long *)skeys, (const uint32_t *)slo, (const uint32_t *)ea, (const uint32_t *)eb, rkeys, rlo, rea, reb, R);
  skeys = rkeys;                                                    // from here on the records are the reduced ones
  slo = rlo;

  // the builder, on the host
  std::vector<uint32_t> hea(R), heb(R), hpc(P), hpk(P);
  DhTree t;
  {
    Profiler &pf = Profiler::get();
    if (pf.enabled) pf.begin("dephier.builder", s);
    RD_HIP(hipMemcpyAsync(hea.data(), rea, (size_t)R * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RD_HIP(hipMemcpyAsync(heb.data(), reb, (size_t)R * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RD_HIP(hipMemcpyAsync(hpc.data(), pitcell, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RD_HIP(hipMemcpyAsync(hpk.data(), pitkey, (size_t)P * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    dh_kruskal(hea, heb, hpc, hpk, P, t);
    if (pf.enabled) pf.end(s);
  }
  const uint32_t count = (uint32_t)t.par.size();
  st.nodes = count;
  st.roots = t.roots;
  st.builder_rounds = 1;
  st.height = t.height;
  int planes = 1;
  while ((1ull << planes) < (uint64_t)t.height + 1ull) planes++;
  st.lift_planes = (uint32_t)planes;
  uint32_t *up = ws.buf<uint32_t>("dephier.up", (size_t)planes * count);   // plane 0: the parents
  uint32_t *lch = ws.buf<uint32_t>("dephier.lchild", count), *rch = ws.buf<uint32_t>("dephier.rchild", count);
  uint32_t *pitleaf = ws.buf<uint32_t>("dephier.pitleaf", count), *spill = ws.buf<uint32_t>("dephier.spill", count);
  uint32_t *lvl = ws.buf<uint32_t>("dephier.level", count), *arrive = ws.buf<uint32_t>("dephier.arrive", count);
  uint32_t *mc = ws.buf<uint32_t>("dephier.mcells", count), *tc = ws.buf<uint32_t>("dephier.cells", count);
  unsigned long long *mv = ws.buf<unsigned long long>("dephier.mvolume", count);
  unsigned long long *tvh = ws.buf<unsigned long long>("dephier.volume", count), *tvl = ws.buf<unsigned long long>("dephier.volume_lo", count);
  dh_upload(up, t.par, s);
  dh_upload(lch, t.lch, s);
  dh_upload(rch, t.rch, s);
  dh_upload(pitleaf, t.pitleaf, s);
  dh_upload(spill, t.spill, s);
  RD_HIP(hipStreamSynchronize(s));   // (the vectors above are pageable and go out of scope with this call)
  const uint32_t ngrid = cdiv(count, NTHR);
  RD_LAUNCH("dephier.nodes", k_dh_nodes, dim3(ngrid), dim3(NTHR), 0, s, (const uint32_t *)spill, (const unsigned long long *)skeys,
            lvl, arrive, mc, mv, count);
  for (int j = 1; j < planes; j++)
    RD_LAUNCH("dephier.lift", k_dh_lift, dim3(ngrid), dim3(NTHR), 0, s, (const uint32_t *)(up + (size_t)(j - 1) * count),
              up + (size_t)j * count, count);
  RD_LAUNCH("dephier.charge", (k_dh_charge<T>), dim3(rgrid), dim3(NTHR), 0, s, d_z, (const uint32_t *)leaf, (const uint32_t *)up,
            (const uint32_t *)lvl, mc, mv, n, count, planes);
  RD_LAUNCH("dephier.accum", (k_dh_accum<T>), dim3(cdiv(P, NTHR)), dim3(NTHR), 0, s, (const uint32_t *)up, (const uint32_t *)lch,
            (const uint32_t *)rch, (const uint32_t *)lvl, (const uint32_t *)mc, (const unsigned long long *)mv, tc, tvh, tvl, arrive, P);
  const uint32_t written = d_table ? std::min(count, capacity) : 0u;
  if (written)
    RD_LAUNCH("dephier.table", (k_dh_table<T>), dim3(cdiv(written, NTHR)), dim3(NTHR), 0, s, d_z, (const uint32_t *)leaf,
              (const uint32_t *)up, (const uint32_t *)lch, (const uint32_t *)rch, (const uint32_t *)pitleaf, (const uint32_t *)spill,
              (const uint32_t *)pitcell, (const unsigned long long *)skeys, (const uint32_t *)slo, (const uint32_t *)tc,
              (const unsigned long long *)tvh, (const unsigned long long *)tvl, d_table, written);
  if (d_labels) RD_LAUNCH("dephier.labels", k_dh_labels, dim3(rgrid), dim3(NTHR), 0, s, (const uint32_t *)leaf, d_labels, n);
  hipLaunchKernelGGL(k_dh_counts, dim3(1), dim3(1), 0, s, d_count, d_leaves, count, P);
  RD_HIP(hipGetLastError());
  dh_last = st;
}

static void check_dephier_args(const void *dem, int w, int h, int topology, const rdgpu_dephier_node *table, uint32_t capacity,
                               const uint32_t *count) {
  check_fill_args(dem, w, h, topology);
  if ((uint64_t)w * (uint64_t)h > 0x7FFF0000ull) throw Error(RDGPU_ERR_ARG, "rdgpu_depression_hierarchy: raster has more than 2^31-65536 cells");
  if (!count) throw Error(RDGPU_ERR_ARG, "rdgpu_depression_hierarchy: null count pointer");
  if (!table && capacity) throw Error(RDGPU_ERR_ARG, "rdgpu_depression_hierarchy: null table with a non-zero capacity");
}

template <class T>
static void dephier_device(const T *d_z, int w, int h, int topology, const uint8_t *d_ocean, int32_t *d_labels,
                           rdgpu_dephier_node *d_table, uint32_t capacity, uint32_t *d_count, uint32_t *d_leaves, hipStream_t s) {
  check_dephier_args(d_z, w, h, topology, d_table, capacity, d_count);
  if (topology == 8) dephier_device_t<T, 8>(d_z, w, h, d_ocean, d_labels, d_table, capacity, d_count, d_leaves, s);
  else dephier_device_t<T, 4>(d_z, w, h, d_ocean, d_labels, d_table, capacity, d_count, d_leaves, s);
}

// host-pointer form: H2D, the device form, D2H of the labels, the two counts and the records that were written
template <class T>
static void dephier_host(const T *dem, int w, int h, int topology, const uint8_t *ocean, int32_t *labels,
                         rdgpu_dephier_node *table, uint32_t capacity, uint32_t *count, uint32_t *leaves) {
  check_dephier_args(dem, w, h, topology, table, capacity, count);
  const size_t n = (size_t)w * h;
  HostStage st;
  const T *d = st.in("host.dem", dem, n);
  const uint8_t *doc = st.in("dephier.host.ocean", ocean, n);   // (null: the border ring)
  uint32_t *dc = st.out("dephier.host.count", count, 1);
  uint32_t *dl = st.out("dephier.host.leaves", leaves, 1);
  int32_t *dlab = st.out("dephier.host.labels", labels, n);
  const uint32_t cap = (uint32_t)std::min<uint64_t>(capacity, 2 * n);   // (fewer than two nodes per cell)
  rdgpu_dephier_node *dt = cap ? Workspace::get().buf<rdgpu_dephier_node>("dephier.host.table", cap) : nullptr;   // (fetched: cut to the count)
  dephier_device<T>(d, w, h, topology, doc, dlab, dt, cap, dc, dl, nullptr);
  st.finish();
  st.fetch(table, dt, std::min(*count, cap));
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_DEPHIER_API(SUF, T)                                                                                        \
  extern "C" int rdgpu_depression_hierarchy_##SUF(const T *dem, int w, int h, int topology, int32_t *labels,          \
                                                  rdgpu_dephier_node *table, uint32_t capacity, uint32_t *count,      \
                                                  uint32_t *leaves) {                                                 \
    return guarded([&] { dephier_host<T>(dem, w, h, topology, nullptr, labels, table, capacity, count, leaves); });   \
  }                                                                                                                   \
  extern "C" int rdgpu_depression_hierarchy_ocean_##SUF(const T *dem, int w, int h, int topology, const uint8_t *ocean, \
                                                        int32_t *labels, rdgpu_dephier_node *table, uint32_t capacity, \
                                                        uint32_t *count, uint32_t *leaves) {                          \
    return guarded([&] { dephier_host<T>(dem, w, h, topology, ocean, labels, table, capacity, count, leaves); });     \
  }                                                                                                                   \
  extern "C" int rdgpu_depression_hierarchy_dev_##SUF(const T *d_dem, int w, int h, int topology, int32_t *d_labels,  \
                                                      rdgpu_dephier_node *d_table, uint32_t capacity,                 \
                                                      uint32_t *d_count, uint32_t *d_leaves, void *stream) {          \
    return guarded([&] {                                                                                              \
      dephier_device<T>(d_dem, w, h, topology, nullptr, d_labels, d_table, capacity, d_count, d_leaves,               \
                        (hipStream_t)stream);                                                                         \
    });                                                                                                               \
  }                                                                                                                   \
  extern "C" int rdgpu_depression_hierarchy_ocean_dev_##SUF(const T *d_dem, int w, int h, int topology,               \
                                                            const uint8_t *d_ocean, int32_t *d_labels,                \
                                                            rdgpu_dephier_node *d_table, uint32_t capacity,           \
                                                            uint32_t *d_count, uint32_t *d_leaves, void *stream) {    \
    return guarded([&] {                                                                                              \
      dephier_device<T>(d_dem, w, h, topology, d_ocean, d_labels, d_table, capacity, d_count, d_leaves,               \
                        (hipStream_t)stream);                                                                         \
    });                                                                                                               \
  }
RD_DEPHIER_API(u8, uint8_t)
RD_DEPHIER_API(i8, int8_t)
RD_DEPHIER_API(i16, int16_t)
RD_DEPHIER_API(u16, uint16_t)
RD_DEPHIER_API(i32, int32_t)
RD_DEPHIER_API(u32, uint32_t)
RD_DEPHIER_API(f32, float)

// f64 needs the dense value ranks of fill64.hip (a follow-up); a double carries neither the elevations nor the volumes
// of 64-bit integers exactly
#define RD_DEPHIER_UNSUPPORTED(SUF, T)                                                                                \
  extern "C" int rdgpu_depression_hierarchy_##SUF(const T *, int, int, int, int32_t *, rdgpu_dephier_node *, uint32_t, \
                                                  uint32_t *, uint32_t *) {                                           \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_depression_hierarchy: 64-bit elevations are not supported"); }); \
  }                                                                                                                   \
  extern "C" int rdgpu_depression_hierarchy_dev_##SUF(const T *, int, int, int, int32_t *, rdgpu_dephier_node *,      \
                                                      uint32_t, uint32_t *, uint32_t *, void *) {                     \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_depression_hierarchy: 64-bit elevations are not supported"); }); \
  }                                                                                                                   \
  extern "C" int rdgpu_depression_hierarchy_ocean_##SUF(const T *, int, int, int, const uint8_t *, int32_t *,         \
                                                        rdgpu_dephier_node *, uint32_t, uint32_t *, uint32_t *) {     \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_depression_hierarchy: 64-bit elevations are not supported"); }); \
  }                                                                                                                   \
  extern "C" int rdgpu_depression_hierarchy_ocean_dev_##SUF(const T *, int, int, int, const uint8_t *, int32_t *,     \
                                                            rdgpu_dephier_node *, uint32_t, uint32_t *, uint32_t *,   \
                                                            void *) {                                                 \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_depression_hierarchy: 64-bit elevations are not supported"); }); \
  }
RD_DEPHIER_UNSUPPORTED(f64, double)
RD_DEPHIER_UNSUPPORTED(i64, int64_t)
RD_DEPHIER_UNSUPPORTED(u64, uint64_t)

extern "C" int rdgpu_dephier_get_stats(rdgpu_dephier_stats *out) {
  if (!out) return RDGPU_ERR_ARG;
  *out = dh_last;
  return RDGPU_OK;
}
