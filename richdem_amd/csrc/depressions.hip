// depressions.hip -- the depression inventory: a label per cell and one record per depression of the fill
// (include/rdgpu.h, "depression inventory").  No reference counterpart.
//
// Everything rests on what the comment above k_md_pockets in fill.hip states: adjacent raised cells share one filled
// level, the connected components of the raised cells ("pockets") are the filled lakes, and every pocket is a union of
// basins of the descent forest.  So the lakes come out of a union-find over the basins (about 10^7 at 40000 x 40000), not
// out of a connected-component labelling of the cells:
//   k_dp_pockets   the one reducing raster pass (z + lab): unites the basins of touching raised cells, and reduces per
//                  BASIN the raised cells, the lowest cell index, the lowest (key, index) and the volume -- the level of a
//                  basin is known (acc[basin]), so nothing has to wait for the pockets.  Each row segment of 64 cells is
//                  one wavefront; a run of equal labels is reduced across its lanes first (segmented shuffle reduction)
//                  and costs four atomics, whatever its length.
//   k_dp_fold      per basin: its root, and its reductions folded into the root's (a table pass, no raster).
//   k_md_spawn<0>  (fill_shared.hpp, unchanged) the raster pass that finds the cell each pocket is flooded from: the outlet.
//   k_dp_keys + a radix sort of the B (first cell | none, basin) pairs: the dense numbering by first cell without
//                  reading the raster; it also counts the pockets.
//   k_dp_table     per sorted pocket: its dense id, and its record with the three gathers from the DEM.
//   k_dp_ids + k_dp_labels   basin -> dense id, then the one raster pass that writes the labels (skipped without labels).
// The element type T is what the structure is computed on (the Key32 types); V is what the values are gathered from:
// V = T, or V = double with T = uint32_t for the dense value ranks of an f64 raster (fill64.hip), where uniq[rank] gives
// the level back.
#include "common.hpp"
#include "fill_shared.hpp"

#include <hipcub/hipcub.hpp>

#include <type_traits>

namespace rdgpu {

static_assert(sizeof(rdgpu_depression) == 40, "four 32-bit words and three doubles, no padding");

constexpr uint32_t DP_NONE = 0xFFFFFFFFu;

__host__ __device__ static inline double dp_key64_to_double(uint64_t k) {   // (fill64.hip Key64<double>::from)
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __builtin_bit_cast(double, b);
}

__global__ __launch_bounds__(NTHR) void k_dp_init(uint32_t *par, uint32_t *cnt, uint32_t *first, unsigned long long *pit,
                                                  unsigned long long *vol, uint32_t *outlet, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  par[b] = b; cnt[b] = 0; first[b] = DP_NONE; pit[b] = ~0ull; vol[b] = 0ull; outlet[b] = DP_NONE;
}

// Integer element types: the keys are the values plus a constant, so a difference of keys is the difference of the
// values, exact in 32 bits, and the sum is exact in 64.  Floating point: one rounding per difference, summed in double.
template <class T, class V, int TOPO>
__global__ __launch_bounds__(NTHR) void k_dp_pockets(const T *__restrict__ z, const V *__restrict__ vals,
                                                     const uint64_t *__restrict__ uniq, const uint32_t *__restrict__ lab,
                                                     const uint32_t *__restrict__ acc, uint32_t *par, uint32_t *cnt,
                                                     uint32_t *first, unsigned long long *pit, unsigned long long *vol, int w,
                                                     int h, uint32_t B) {
  constexpr bool INTEGER = std::is_integral<V>::value;
  using Acc = typename std::conditional<INTEGER, unsigned long long, double>::type;
  // one wavefront per 64-cell row segment (grid-stride over segments), as k_md_pockets
  const uint32_t segsX = ((uint32_t)w + 63u) / 64u;
  const uint64_t nseg = (uint64_t)segsX * (uint64_t)h;
  const int lane = threadIdx.x & 63;
  for (uint64_t sgi = (uint64_t)blockIdx.x * (NTHR / 64) + (threadIdx.x >> 6); sgi < nseg; sgi += (uint64_t)gridDim.x * (NTHR / 64)) {
    const int y = (int)(sgi / segsX), x = (int)(sgi % segsX) * 64 + lane;
    const bool in = x < w;
    const size_t c = (size_t)y * w + (in ? x : 0);
    const uint32_t b = in ? lab[c] : B;
    const uint32_t kz = Key32<T>::to(z[c]);
    const uint32_t L = b != B ? acc[b] : 0u;
    const bool raised = in && b != B && L > kz;
    Acc term = 0;
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
      if (INTEGER) term = (Acc)(L - kz);
      else if (uniq) term = (Acc)(dp_key64_to_double(uniq[L]) - (double)vals[c]);
      else term = (Acc)((double)Key32<T>::from(L) - (double)vals[c]);
    }
    // runs of equal labels along the row segment: reduced across their lanes, then one set of atomics per run
    const uint32_t key = raised ? b : DP_NONE;
    const uint32_t left = __shfl_up(key, 1, 64);
    const bool head = raised && (lane == 0 || left != key);
    const unsigned long long bnd = __ballot(head) | ~__ballot(raised);   // lanes no run continues into
    const unsigned long long above = lane < 63 ? (bnd >> (lane + 1)) : 0ull;
    const int end = above ? lane + __ffsll((long long)above) : 64;        // one past the last lane of this lane's run
    unsigned long long pk = raised ? (((unsigned long long)kz << 32) | (unsigned long long)c) : ~0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      // before the step lane l holds the reduction over lanes [l, min(l + d, end))
      const unsigned long long opk = __shfl_down(pk, d, 64);
      const Acc ot = __shfl_down(term, d, 64);
      if (lane + d < end) {
        pk = opk < pk ? opk : pk;
        term += ot;
      }
    }
    if (head) {
      atomicAdd(&cnt[b], (uint32_t)(end - lane));
      // the head is the run's lowest index; rows of one basin arrive roughly in order, so most of these tests fail
      if ((uint32_t)c < __hip_atomic_load(&first[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&first[b], (uint32_t)c);
      if (pk < __hip_atomic_load(&pit[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&pit[b], pk);
      if (INTEGER) atomicAdd(&vol[b], (unsigned long long)term);
      else atomicAdd(reinterpret_cast<double *>(&vol[b]), (double)term);
    }
  }
}

// root[b]; the reductions of a basin that is not its pocket's root are added to the root's.  Only roots are written and
// only by atomics, every thread reads its own basin's words alone, and par is not changed: safe in place.
template <bool INTEGER>
__global__ __launch_bounds__(NTHR) void k_dp_fold(uint32_t *par, uint32_t *root, uint32_t *cnt, uint32_t *first,
                                                  unsigned long long *pit, unsigned long long *vol, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b >= B) return;
  const uint32_t r = md_find(par, b);
  root[b] = r;
  if (r == b) return;
  const uint32_t c = cnt[b];
  if (!c) return;   // (cannot happen: only basins with raised cells are united)
  atomicAdd(&cnt[r], c);
  atomicMin(&first[r], first[b]);
  atomicMin(&pit[r], pit[b]);
  if (INTEGER) atomicAdd(&vol[r], vol[b]);
  else atomicAdd(reinterpret_cast<double *>(&vol[r]), __builtin_bit_cast(double, vol[b]));
}

// sort keys: the first cell of every pocket (a root with raised cells), DP_NONE for every other basin; counts the pockets
__global__ __launch_bounds__(NTHR) void k_dp_keys(const uint32_t *__restrict__ root, const uint32_t *__restrict__ cnt,
                                                  const uint32_t *__restrict__ first, uint32_t *keys, uint32_t *ids,
                                                  uint32_t *count, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  const bool pocket = b < B && root[b] == b && cnt[b] != 0;
  if (b < B) {
    keys[b] = pocket ? first[b] : DP_NONE;
    ids[b] = b;
  }
  const unsigned long long m = __ballot(pocket);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(count, (uint32_t)__popcll(m));
}

// sorted position i -> dense id i + 1 of that pocket, and its record
template <class V, bool INTEGER>
__global__ __launch_bounds__(NTHR) void k_dp_table(const uint32_t *__restrict__ skeys, const uint32_t *__restrict__ sids,
                                                   const uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ pit,
                                                   const uint32_t *__restrict__ outlet, const unsigned long long *__restrict__ vol,
                                                   const V *__restrict__ vals, uint32_t *dense, rdgpu_depression *table,
                                                   uint32_t capacity, uint32_t B) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= B) return;
  const uint32_t fc = skeys[i];
  if (fc == DP_NONE) return;
  const uint32_t r = sids[i];
  dense[r] = i + 1u;
  if (!table || i >= capacity) return;
  rdgpu_depression d;
  d.first_cell = fc;
  d.pit_cell = (uint32_t)pit[r];
  d.outlet_cell = outlet[r];
  d.cells = cnt[r];
  // (every pocket has both cells; an index that was never set is not followed)
  d.level = d.outlet_cell != DP_NONE ? (double)vals[d.outlet_cell] : __builtin_nan("");
  d.pit_elevation = d.pit_cell != DP_NONE ? (double)vals[d.pit_cell] : __builtin_nan("");
  d.volume = INTEGER ? (double)vol[r] : __builtin_bit_cast(double, vol[r]);
  table[i] = d;
}

__global__ __launch_bounds__(NTHR) void k_dp_ids(const uint32_t *__restrict__ root, const uint32_t *__restrict__ dense,
                                                 uint32_t *bid, uint32_t B) {
  const uint32_t b = blockIdx.x * NTHR + threadIdx.x;
  if (b < B) bid[b] = dense[root[b]];   // (read only for basins with raised cells: their roots are pockets)
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_dp_labels(const T *__restrict__ z, const uint32_t *__restrict__ lab,
                                                    const uint32_t *__restrict__ acc, const uint32_t *__restrict__ bid,
                                                    int32_t *__restrict__ labels, uint64_t n, uint32_t B) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const uint32_t b = lab[c];
    int32_t l = 0;
    if (b != B && acc[b] > Key32<T>::to(z[c])) l = (int32_t)bid[b];
    labels[c] = l;
  }
}

template <class T, class V, int TOPO>
static void depressions_device_t(const T *d_z, const V *d_vals, const uint64_t *d_uniq, int w, int h, int32_t *d_labels,
                                 rdgpu_depression *d_table, uint32_t capacity, uint32_t *d_count, hipStream_t s) {
  constexpr bool INTEGER = std::is_integral<V>::value;
  const uint64_t n = (uint64_t)w * h;
  RD_HIP(hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
  FillBuffers fb;
  fill_local_phase_plain<T>(d_z, w, h, TOPO, fb, s);
  if (fb.trivial) {
    if (d_labels) RD_HIP(hipMemsetAsync(d_labels, 0, n * sizeof(int32_t), s));
    return;
  }
  const uint32_t B = fb.B;
  Workspace &ws = Workspace::get();
  uint32_t *par = ws.buf<uint32_t>("depr.par", B), *root = ws.buf<uint32_t>("depr.root", B);
  uint32_t *cnt = ws.buf<uint32_t>("depr.cells", B), *first = ws.buf<uint32_t>("depr.first", B);
  uint32_t *outlet = ws.buf<uint32_t>("depr.outlet", B);
  unsigned long long *pit = ws.buf<unsigned long long>("depr.pit", B), *vol = ws.buf<unsigned long long>("depr.volume", B);
  uint32_t *keys = ws.buf<uint32_t>("depr.keys", B), *ids = ws.buf<uint32_t>("depr.ids", B);
  uint32_t *skeys = ws.buf<uint32_t>("depr.skeys", B), *sids = ws.buf<uint32_t>("depr.sids", B);
  uint32_t *dense = keys;   // (the unsorted keys are dead after the sort)
  const uint32_t bgrid = cdiv(B, NTHR), sgrid = (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u);
  RD_LAUNCH("depr.init", k_dp_init, dim3(bgrid), dim3(NTHR), 0, s, par, cnt, first, pit, vol, outlet, B);
  RD_LAUNCH("depr.pockets", (k_dp_pockets<T, V, TOPO>), dim3(256u * 16u), dim3(NTHR), 0, s, d_z, d_vals, d_uniq,
            (const uint32_t *)fb.lab, (const uint32_t *)fb.acc, par, cnt, first, pit, vol, w, h, B);
  RD_LAUNCH("depr.outlets", (k_md_spawn<T, TOPO, 0>), dim3(sgrid), dim3(NTHR), 0, s, d_z, (const uint32_t *)fb.lab,
            (const uint32_t *)fb.acc, par, outlet, w, h, B);
  RD_LAUNCH("depr.fold", (k_dp_fold<INTEGER>), dim3(bgrid), dim3(NTHR), 0, s, par, root, cnt, first, pit, vol, B);
  RD_LAUNCH("depr.keys", k_dp_keys, dim3(bgrid), dim3(NTHR), 0, s, (const uint32_t *)root, (const uint32_t *)cnt,
            (const uint32_t *)first, keys, ids, d_count, B);
  size_t tb = 0;
  RD_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, skeys, ids, sids, (int)B, 0, 32, s));
  void *tmp = ws.buf("depr.sort_tmp", tb);
  {
    Profiler &pf = Profiler::get();
    if (pf.enabled) pf.begin("depr.sort", s);
    RD_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, skeys, ids, sids, (int)B, 0, 32, s));
    if (pf.enabled) pf.end(s);
  }
  RD_LAUNCH("depr.table", (k_dp_table<V, INTEGER>), dim3(bgrid), dim3(NTHR), 0, s, (const uint32_t *)skeys,
            (const uint32_t *)sids, (const uint32_t *)cnt, (const unsigned long long *)pit, (const uint32_t *)outlet,
            (const unsigned long long *)vol, d_vals, dense, d_table, capacity, B);
  if (!d_labels) return;
  uint32_t *bid = ids;      // (so are the unsorted ids)
  RD_LAUNCH("depr.ids", k_dp_ids, dim3(bgrid), dim3(NTHR), 0, s, (const uint32_t *)root, (const uint32_t *)dense, bid, B);
  RD_LAUNCH("depr.labels", (k_dp_labels<T>), dim3(sgrid), dim3(NTHR), 0, s, d_z, (const uint32_t *)fb.lab,
            (const uint32_t *)fb.acc, (const uint32_t *)bid, d_labels, n, B);
}

static void check_depr_args(const void *dem, int w, int h, int topology, const rdgpu_depression *table, uint32_t capacity,
                            const uint32_t *count) {
  check_fill_args(dem, w, h, topology);
  if ((uint64_t)w * (uint64_t)h > 0x7FFF0000ull) throw Error(RDGPU_ERR_ARG, "rdgpu_depressions: raster has more than 2^31-65536 cells");
  if (!count) throw Error(RDGPU_ERR_ARG, "rdgpu_depressions: null count pointer");
  if (!table && capacity) throw Error(RDGPU_ERR_ARG, "rdgpu_depressions: null table with a non-zero capacity");
}

template <class T>
static void depressions_device(const T *d_z, int w, int h, int topology, int32_t *d_labels, rdgpu_depression *d_table,
                               uint32_t capacity, uint32_t *d_count, hipStream_t s) {
  check_depr_args(d_z, w, h, topology, d_table, capacity, d_count);
  if (topology == 8) depressions_device_t<T, T, 8>(d_z, d_z, nullptr, w, h, d_labels, d_table, capacity, d_count, s);
  else depressions_device_t<T, T, 4>(d_z, d_z, nullptr, w, h, d_labels, d_table, capacity, d_count, s);
}

void depressions_on_ranks(const uint32_t *d_rk, const uint64_t *d_uniq, const double *d_vals, int w, int h, int topology,
                          int32_t *d_labels, rdgpu_depression *d_table, uint32_t capacity, uint32_t *d_count, hipStream_t s) {
  check_depr_args(d_vals, w, h, topology, d_table, capacity, d_count);
  if (topology == 8) depressions_device_t<uint32_t, double, 8>(d_rk, d_vals, d_uniq, w, h, d_labels, d_table, capacity, d_count, s);
  else depressions_device_t<uint32_t, double, 4>(d_rk, d_vals, d_uniq, w, h, d_labels, d_table, capacity, d_count, s);
}

template <>
void depressions_device<double>(const double *d_z, int w, int h, int topology, int32_t *d_labels, rdgpu_depression *d_table,
                                uint32_t capacity, uint32_t *d_count, hipStream_t s) {
  check_depr_args(d_z, w, h, topology, d_table, capacity, d_count);
  depressions_f64_device(d_z, w, h, topology, d_labels, d_table, capacity, d_count, s);
}

// host-pointer form: H2D, the device form, D2H of the labels, the count and the records that were written
template <class T>
static void depressions_host(const T *dem, int w, int h, int topology, int32_t *labels, rdgpu_depression *table,
                             uint32_t capacity, uint32_t *count) {
  check_depr_args(dem, w, h, topology, table, capacity, count);
  const size_t n = (size_t)w * h;
  HostStage st;
  const T *d = st.in("depr.host.dem", dem, n);
  uint32_t *dc = st.out("depr.host.count", count, 1);
  int32_t *dl = st.out("depr.host.labels", labels, n);
  const uint32_t cap = (uint32_t)std::min<uint64_t>(capacity, n);   // (there are fewer depressions than cells)
  rdgpu_depression *dt = cap ? Workspace::get().buf<rdgpu_depression>("depr.host.table", cap) : nullptr;   // (fetched: cut to the count)
  depressions_device<T>(d, w, h, topology, dl, dt, cap, dc, nullptr);
  st.finish();
  st.fetch(table, dt, std::min(*count, cap));
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_DEPR_API(SUF, T)                                                                                          \
  extern "C" int rdgpu_depressions_##SUF(const T *dem, int w, int h, int topology, int32_t *labels,                  \
                                         rdgpu_depression *table, uint32_t capacity, uint32_t *count) {              \
    return guarded([&] { depressions_host<T>(dem, w, h, topology, labels, table, capacity, count); });               \
  }                                                                                                                  \
  extern "C" int rdgpu_depressions_dev_##SUF(const T *d_dem, int w, int h, int topology, int32_t *d_labels,          \
                                             rdgpu_depression *d_table, uint32_t capacity, uint32_t *d_count,        \
                                             void *stream) {                                                         \
    return guarded([&] { depressions_device<T>(d_dem, w, h, topology, d_labels, d_table, capacity, d_count, (hipStream_t)stream); }); \
  }
RD_DEPR_API(u8, uint8_t)
RD_DEPR_API(i8, int8_t)
RD_DEPR_API(i16, int16_t)
RD_DEPR_API(u16, uint16_t)
RD_DEPR_API(i32, int32_t)
RD_DEPR_API(u32, uint32_t)
RD_DEPR_API(f32, float)
RD_DEPR_API(f64, double)

// 64-bit integers: a double carries neither their elevations nor their volumes exactly
#define RD_DEPR_UNSUPPORTED(SUF, T)                                                                                  \
  extern "C" int rdgpu_depressions_##SUF(const T *, int, int, int, int32_t *, rdgpu_depression *, uint32_t, uint32_t *) { \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_depressions: 64-bit integer elevations are not supported"); }); \
  }                                                                                                                  \
  extern "C" int rdgpu_depressions_dev_##SUF(const T *, int, int, int, int32_t *, rdgpu_depression *, uint32_t,      \
                                             uint32_t *, void *) {                                                   \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_depressions: 64-bit integer elevations are not supported"); }); \
  }
RD_DEPR_UNSUPPORTED(i64, int64_t)
RD_DEPR_UNSUPPORTED(u64, uint64_t)
