// fsm.hip -- Fill-Spill-Merge: a water raster routed through the depression hierarchy into lakes with a level each
// (include/rdgpu.h, "fill-spill-merge").  Reference counterpart: depressions/fill_spill_merge.hpp
// with surface water only; where the reference floods every lake from its pit with a priority queue, a lake's level here
// is a closed form over the sorted cells of its subtree.
//   k_fsm_extract  the 56-byte table -> parent / lchild / rchild / geolink / volume, 24 bytes a node, and the leaf count.
//   k_fsm_gather   one raster pass: water[c] into leaf_water[labels[c]] by double atomics, a wavefront's run of equal
//                  labels combined first; the ocean's share and the two refusal flags block-reduced.
//   the pour       serial, on the host, over the extracted columns (fsm_pour): w per node with path compression over
//                  full nodes, then top(leaf) in one descending pass and the list of lake tops.
//   k_fsm_lakes    level(f) of every lake top; a full lake's water level is that.
//   partial lakes  k_fsm_count, a select of the record cells in raster order, k_fsm_keys, a stable radix sort by
//                  (lake rank, key of dem) over the bits in use, k_fsm_vals (segment heads, elevations in double), a
//                  segmented inclusive scan (hipcub's by-key scan: it carries across blocks), k_fsm_level (the minimum
//                  qualifying position per segment) and k_fsm_height.
//   k_fsm_depth    one raster pass: depth, and its sum.
#include "common.hpp"
#include "fill_shared.hpp"

#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <type_traits>

namespace rdgpu {

static_assert(sizeof(rdgpu_fsm_result) == 32, "three doubles and two 32-bit words");
static_assert(sizeof(rdgpu_fsm_stats) == 48, "a 64-bit word, a double and eight 32-bit words");

constexpr uint32_t FSM_NONE = 0xFFFFFFFFu;
constexpr uint32_t FSM_OCEAN = 0xFFFFFFFEu;   // a shortcut's target: the rest of the water is lost
constexpr uint32_t FSM_BAD_WATER = 1u, FSM_BAD_LABEL = 2u;

// device words of one call: two doubles, then four 32-bit words
struct FsmWords {
  double ocean, standing;
  uint32_t flags, leaves, records, pad;
};

// the key bits of an element type: Key32<T>::to stays below 2^(8 sizeof(T))
template <class T>
constexpr int fsm_key_bits() { return sizeof(T) >= 4 ? 32 : (int)sizeof(T) * 8; }

__device__ __forceinline__ double fsm_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

__global__ __launch_bounds__(NTHR) void k_fsm_extract(const rdgpu_dephier_node *__restrict__ table, uint32_t *__restrict__ par,
                                                      uint32_t *__restrict__ lch, uint32_t *__restrict__ rch,
                                                      uint32_t *__restrict__ geo, double *__restrict__ vol,
                                                      double *__restrict__ leaf_water, uint32_t count, FsmWords *words) {
  const uint32_t v = blockIdx.x * NTHR + threadIdx.x;
  bool leaf = false;
  if (v < count) {
    const rdgpu_dephier_node d = table[v];
    par[v] = d.parent;
    lch[v] = d.lchild;
    rch[v] = d.rchild;
    geo[v] = d.geolink;
    vol[v] = d.volume;
    leaf_water[v] = 0.0;
    leaf = d.lchild == FSM_NONE;
  }
  const unsigned long long m = __ballot(leaf);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&words->leaves, (uint32_t)__popcll(m));
}

// Every wavefront walks 64 consecutive cells at a time with all its lanes (a lane past the end carries label -2 and no
// water), so the runs of equal labels can be summed by shuffles: rid numbers the runs, and after the doubling steps the
// first lane of a run holds the run's water.
__global__ __launch_bounds__(NTHR) void k_fsm_gather(const int32_t *__restrict__ labels, const double *__restrict__ water,
                                                     double *leaf_water, uint64_t n, FsmWords *words) {
  __shared__ double s_ocean[NTHR / 64];
  __shared__ uint32_t s_flags[NTHR / 64];
  const uint32_t P = words->leaves;   // (written by k_fsm_extract, the launch before this one; 0 without a table)
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  double ocean = 0.0;
  uint32_t flags = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * NTHR + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint64_t c = base + lane;
    int32_t l = -2;
    double v = 0.0;
    if (c < n) {
      l = labels[c];
      v = water[c];
      if (!(v >= 0.0) || !(v <= 1.7976931348623157e308)) { flags |= FSM_BAD_WATER; v = 0.0; }
      if (l < -1 || (l >= 0 && (uint32_t)l >= P)) { flags |= FSM_BAD_LABEL; l = -2; }
    }
    const int32_t lprev = __shfl_up(l, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || l != lprev);
    const int rid = __popcll(heads & (~0ull >> (63 - lane)));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double vo = __shfl_down(v, d, 64);
      const int ro = __shfl_down(rid, d, 64);
      if (lane + d < 64 && ro == rid) v += vo;
    }
    if ((heads >> lane) & 1ull) {
      if (l >= 0) { if (v > 0.0) atomicAdd(&leaf_water[l], v); }
      else if (l == -1) ocean += v;
    }
  }
  ocean = fsm_wave_sum(ocean);
  flags = (__ballot(flags & FSM_BAD_WATER) ? FSM_BAD_WATER : 0u) | (__ballot(flags & FSM_BAD_LABEL) ? FSM_BAD_LABEL : 0u);
  if (lane == 0) {
    s_ocean[threadIdx.x >> 6] = ocean;
    s_flags[threadIdx.x >> 6] = flags;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    uint32_t f = 0;
    for (int i = 0; i < NTHR / 64; i++) {
      t += s_ocean[i];
      f |= s_flags[i];
    }
    if (t > 0.0) atomicAdd(&words->ocean, t);
    if (f) atomicOr(&words->flags, f);
  }
}

// per lake top (rank r, node top[r]): its spill level; a full lake (prank NONE) stands at it
__global__ __launch_bounds__(NTHR) void k_fsm_lakes(const rdgpu_dephier_node *__restrict__ table, const uint32_t *__restrict__ top,
                                                    const uint32_t *__restrict__ prank, double *__restrict__ lvl,
                                                    double *__restrict__ hl, uint32_t L) {
  const uint32_t r = blockIdx.x * NTHR + threadIdx.x;
  if (r >= L) return;
  const double v = table[top[r]].level;
  lvl[r] = v;
  hl[r] = prank[r] == FSM_NONE ? v : -INFINITY;
}

// a cell gives a record when it belongs to a partial lake and lies below the lake's spill level
template <class T>
struct FsmRecord {
  const T *z;
  const int32_t *labels;
  const uint32_t *lake_of_leaf, *prank;
  const double *lvl;
  uint32_t P;
  __device__ __forceinline__ uint32_t lake(uint64_t c) const {   // the rank of the cell's PARTIAL lake where it gives a record
    const int32_t l = labels[c];
    if (l < 0 || (uint32_t)l >= P) return FSM_NONE;
    const uint32_t r = lake_of_leaf[l];
    if (r == FSM_NONE || prank[r] == FSM_NONE) return FSM_NONE;
    return (double)z[c] < lvl[r] ? prank[r] : FSM_NONE;
  }
  __device__ __forceinline__ bool operator()(const uint32_t &c) const { return lake(c) != FSM_NONE; }
};

template <class T>
__global__ __launch_bounds__(NTHR) void k_fsm_count(FsmRecord<T> rec, uint64_t n, unsigned long long *total) {
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  uint32_t mine = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) mine += rec.lake(c) != FSM_NONE ? 1u : 0u;
#pragma unroll
  for (int d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, (unsigned long long)mine);
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_fsm_keys(FsmRecord<T> rec, const uint32_t *__restrict__ cells,
                                                   unsigned long long *__restrict__ keys, uint32_t R) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= R) return;
  const uint32_t c = cells[i];
  keys[i] = ((unsigned long long)rec.lake(c) << fsm_key_bits<T>()) | Key32<T>::to(rec.z[c]);
}

// after the sort: the segment (partial lake) of every record, its elevation in double, and the first record of a segment
template <class T>
__global__ __launch_bounds__(NTHR) void k_fsm_vals(const T *__restrict__ z, const unsigned long long *__restrict__ skeys,
                                                   const uint32_t *__restrict__ scells, uint32_t *__restrict__ seg,
                                                   double *__restrict__ val, uint32_t *__restrict__ segstart, uint32_t R,
                                                   uint32_t Lp) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= R) return;
  const uint32_t r = min((uint32_t)(skeys[i] >> fsm_key_bits<T>()), Lp - 1u);   // (below Lp as the records were selected)
  seg[i] = r;
  val[i] = (double)z[scells[i]];
  if (i == 0 || min((uint32_t)(skeys[i - 1] >> fsm_key_bits<T>()), Lp - 1u) != r) segstart[r] = i;
}

// position k (1-based in its segment) qualifies when (w + S_k) / k does not reach above the next cell; the last one always
__global__ __launch_bounds__(NTHR) void k_fsm_level(const uint32_t *__restrict__ seg, const double *__restrict__ val,
                                                    const double *__restrict__ S, const uint32_t *__restrict__ segstart,
                                                    const double *__restrict__ pw, uint32_t *kmin, uint32_t R) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= R) return;
  const uint32_t r = seg[i];
  const double k = (double)(i - segstart[r] + 1u);
  const bool last = i + 1 == R || seg[i + 1] != r;
  if (last || (pw[r] + S[i]) / k <= val[i + 1]) atomicMin(&kmin[r], i);
}

__global__ __launch_bounds__(NTHR) void k_fsm_height(const uint32_t *__restrict__ prank, const double *__restrict__ S,
                                                     const uint32_t *__restrict__ segstart, const uint32_t *__restrict__ kmin,
                                                     const double *__restrict__ pw, double *__restrict__ hl, uint32_t L) {
  const uint32_t r = blockIdx.x * NTHR + threadIdx.x;
  if (r >= L) return;
  const uint32_t p = prank[r];
  if (p == FSM_NONE) return;
  const uint32_t i = kmin[p];
  hl[r] = i == FSM_NONE ? -INFINITY : (pw[p] + S[i]) / (double)(i - segstart[p] + 1u);   // (no record: no cell below the level)
}

template <class T>
__global__ __launch_bounds__(NTHR) void k_fsm_depth(const T *__restrict__ z, const int32_t *__restrict__ labels,
                                                    const uint32_t *__restrict__ lake_of_leaf, const double *__restrict__ hl,
                                                    double *__restrict__ depth, uint64_t n, uint32_t P, FsmWords *words) {
  __shared__ double s_sum[NTHR / 64];
  const uint64_t stride = (uint64_t)gridDim.x * NTHR;
  double sum = 0.0;
  for (uint64_t c = (uint64_t)blockIdx.x * NTHR + threadIdx.x; c < n; c += stride) {
    const int32_t l = labels[c];
    double d = 0.0;
    if (l >= 0 && (uint32_t)l < P) {
      const uint32_t r = lake_of_leaf[l];
      if (r != FSM_NONE) {
        const double h = hl[r], zc = (double)z[c];
        if (zc < h) d = h - zc;
      }
    }
    depth[c] = d;
    sum += d;
  }
  sum = fsm_wave_sum(sum);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < NTHR / 64; i++) t += s_sum[i];
    if (t > 0.0) atomicAdd(&words->standing, t);
  }
}

__global__ void k_fsm_result(rdgpu_fsm_result *out, double water_in, double ocean, uint32_t lakes, uint32_t full_lakes,
                             const FsmWords *words) {
  rdgpu_fsm_result r;
  r.water_in = water_in;
  r.ocean = ocean;
  r.standing = words->standing;
  r.lakes = lakes;
  r.full_lakes = full_lakes;
  *out = r;
}

static thread_local rdgpu_fsm_stats fsm_last = {};

// ---- the host pass ----------------------------------------------------------------------------------------------------
struct FsmTree {
  std::vector<uint32_t> par, lch, rch, geo;
  std::vector<double> vol;
};

// the records are what the hierarchy writes: leaves first, children below their parents, every link in range
static void fsm_check_table(const FsmTree &t, uint32_t P) {
  const uint32_t count = (uint32_t)t.par.size();
  for (uint32_t v = 0; v < count; v++) {
    const uint32_t a = t.lch[v], b = t.rch[v], p = t.par[v], g = t.geo[v];
    const bool leaf = a == FSM_NONE && b == FSM_NONE;
    if (leaf != (v < P)) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: the leaves are not the first records of the table");
    if (!leaf && !(a < v && b < v && a != b))
      throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: a child id is not below its parent's");
    if (p != FSM_NONE && !(p < count && p > v && (t.lch[p] == v || t.rch[p] == v)))
      throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: a parent does not list the node as its child");
    if (g != FSM_NONE && g >= P) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: a geolink is not a leaf");
  }
}

// The contract's pour, leaf by leaf in ascending id.  jump[m], set for full nodes only, is a node further along the path
// the loop takes from m: every node in between is full, and whatever a first visit sets on the way (w of a parent whose
// children have both filled) was set by the visit that recorded the path, so following it leaves the same values.
static double fsm_pour(const FsmTree &t, const std::vector<double> &leaf_water, std::vector<double> &w, rdgpu_fsm_stats &st) {
  const uint32_t count = (uint32_t)t.par.size(), P = (uint32_t)leaf_water.size();
  const uint64_t hop_cap = 4ull * count + 64ull;   // (a table that belongs to no DEM may loop: it gives unspecified values)
  w.assign(count, 0.0);
  std::vector<uint32_t> jump(count, FSM_NONE), path;
  double ocean = 0.0;
  for (uint32_t leaf = 0; leaf < P; leaf++) {
    double x = leaf_water[leaf];
    if (!(x > 0.0)) continue;
    st.pours++;
    uint32_t n = leaf;
    uint64_t hops = 0;
    path.clear();
    for (;;) {
      if (w[n] < t.vol[n]) {
        const double cap = t.vol[n] - w[n];
        if (x < cap) { w[n] += x; break; }
        w[n] = t.vol[n];
        x -= cap;
      }
      if (x <= 0.0) break;
      uint32_t nxt;
      if (jump[n] != FSM_NONE) {
        nxt = jump[n];
        st.shortcut_hits++;
      } else {
        const uint32_t p = t.par[n];
        if (p == FSM_NONE) {
          nxt = t.geo[n] == FSM_NONE ? FSM_OCEAN : t.geo[n];
        } else {
          const uint32_t s = t.lch[p] == n ? t.rch[p] : t.lch[p];
          if (w[s] >= t.vol[s]) {
            if (w[p] == 0.0) w[p] = std::min(t.vol[p], t.vol[t.lch[p]] + t.vol[t.rch[p]]);
            nxt = p;
          } else {
            nxt = t.geo[n] == FSM_NONE ? FSM_OCEAN : t.geo[n];   // (NONE under a parent: not a hierarchy's table)
          }
        }
      }
      path.push_back(n);
      n = nxt;
      if (n == FSM_OCEAN || hops >= hop_cap) {
        ocean += x;
        n = FSM_OCEAN;
        break;
      }
      hops++;
    }
    if (hops < hop_cap)
      for (uint32_t m : path) jump[m] = n;
    st.longest_pour = (uint32_t)std::max<uint64_t>(st.longest_pour, std::min<uint64_t>(hops, 0xFFFFFFFFull));
  }
  return ocean;
}

template <class T>
static void fsm_up(T *d, const std::vector<T> &v, hipStream_t s) {
  if (!v.empty()) RD_HIP(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
}
template <class T>
static void fsm_down(std::vector<T> &v, const T *d, size_t count, hipStream_t s) {
  v.resize(count);
  if (count) RD_HIP(hipMemcpyAsync(v.data(), d, count * sizeof(T), hipMemcpyDeviceToHost, s));
}

static void check_fsm_args(const void *dem, int w, int h, const void *labels, const void *table, uint32_t count,
                           const void *water, const void *depth) {
  check_fill_args(dem, w, h, 8);
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  if (n > 0x7FFF0000ull) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: raster has more than 2^31-65536 cells");
  if (!labels || !water || !depth) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: null labels, water or depth");
  if (!table && count) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: null table with a non-zero count");
  if (count > 2 * n) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: more nodes than two per cell");
  const uintptr_t a = (uintptr_t)water, b = (uintptr_t)depth, bytes = (uintptr_t)(n * sizeof(double));
  if (a < b + bytes && b < a + bytes) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: depth overlaps water");
}

template <class T>
static void fsm_device(const T *d_z, int w, int h, const int32_t *d_labels, const rdgpu_dephier_node *d_table, uint32_t count,
                       const double *d_water, double *d_depth, double *d_nw, rdgpu_fsm_result *d_result, hipStream_t s) {
  check_fsm_args(d_z, w, h, d_labels, d_table, count, d_water, d_depth);
  const uint64_t n = (uint64_t)w * h;
  Workspace &ws = Workspace::get();
  Profiler &pf = Profiler::get();
  rdgpu_fsm_stats st = {};
  st.nodes = count;
  const uint32_t rgrid = (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u);
  FsmWords *words = ws.buf<FsmWords>("fsm.words", 1);
  unsigned long long *total = ws.buf<unsigned long long>("fsm.total", 1);
  FsmWords *hw = reinterpret_cast<FsmWords *>(ws.host_words());
  const size_t cn = std::max<uint32_t>(count, 1u);
  uint32_t *par = ws.buf<uint32_t>("fsm.parent", cn), *lch = ws.buf<uint32_t>("fsm.lchild", cn);
  uint32_t *rch = ws.buf<uint32_t>("fsm.rchild", cn), *geo = ws.buf<uint32_t>("fsm.geolink", cn);
  double *vol = ws.buf<double>("fsm.volume", cn), *leaf_water = ws.buf<double>("fsm.leaf_water", cn);

  RD_HIP(hipMemsetAsync(words, 0, sizeof(FsmWords), s));
  if (count)
    RD_LAUNCH("fsm.extract", k_fsm_extract, dim3(cdiv(count, NTHR)), dim3(NTHR), 0, s, d_table, par, lch, rch, geo, vol, leaf_water,
              count, words);
  RD_LAUNCH("fsm.gather", k_fsm_gather, dim3(rgrid), dim3(NTHR), 0, s, d_labels, d_water, leaf_water, n, words);
  RD_HIP(hipMemcpyAsync(hw, words, sizeof(FsmWords), hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  if (hw->flags & FSM_BAD_LABEL) throw Error(RDGPU_ERR_ARG, "rdgpu_fill_spill_merge: a label outside [-1, leaves)");
  if (hw->flags & FSM_BAD_WATER)
    throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_fill_spill_merge: negative or non-finite water (groundwater is not supported)");
  const uint32_t P = hw->leaves;
  const double ocean0 = hw->ocean;
  st.leaves = P;

  // the host pass: 24 bytes a node and 8 a leaf down, the pour, the lake tops, the lake tables up
  const auto t0 = std::chrono::steady_clock::now();
  if (pf.enabled) pf.begin("fsm.host_pass", s);
  FsmTree t;
  std::vector<double> lw, wn;
  fsm_down(t.par, par, count, s);
  fsm_down(t.lch, lch, count, s);
  fsm_down(t.rch, rch, count, s);
  fsm_down(t.geo, geo, count, s);
  fsm_down(t.vol, vol, count, s);
  fsm_down(lw, leaf_water, P, s);
  RD_HIP(hipStreamSynchronize(s));
  fsm_check_table(t, P);
  double water_in = ocean0;
  for (uint32_t l = 0; l < P; l++) water_in += lw[l];
  const double ocean = ocean0 + fsm_pour(t, lw, wn, st);
  // top(n) in one descending pass (a parent's id is above its children's); the lake tops by ascending id
  std::vector<uint32_t> topn(count, FSM_NONE), rank_of(count, FSM_NONE), tops, prank, lake_of_leaf(P, FSM_NONE);
  std::vector<double> pw;   // the water of the partial lakes, by partial rank
  for (uint32_t v = count; v-- > 0;) {
    const uint32_t p = t.par[v];
    if (p != FSM_NONE && topn[p] != FSM_NONE) topn[v] = topn[p];
    else if (wn[v] > 0.0) topn[v] = v;
  }
  for (uint32_t v = 0; v < count; v++)
    if (topn[v] == v) {
      const bool full = wn[v] >= t.vol[v];
      if (!full) pw.push_back(wn[v]);
      prank.push_back(full ? FSM_NONE : (uint32_t)pw.size() - 1u);
      rank_of[v] = (uint32_t)tops.size();
      tops.push_back(v);
    }
  for (uint32_t l = 0; l < P; l++)
    if (topn[l] != FSM_NONE) lake_of_leaf[l] = rank_of[topn[l]];
  const uint32_t L = (uint32_t)tops.size(), Lp = (uint32_t)pw.size();
  st.lakes = L;
  st.partial_lakes = Lp;
  uint32_t *d_lol = ws.buf<uint32_t>("fsm.lake_of_leaf", std::max<uint32_t>(P, 1u));
  uint32_t *d_top = ws.buf<uint32_t>("fsm.lake_top", std::max<uint32_t>(L, 1u)), *d_prank = ws.buf<uint32_t>("fsm.lake_partial", std::max<uint32_t>(L, 1u));
  double *d_pw = ws.buf<double>("fsm.partial_water", std::max<uint32_t>(Lp, 1u));
  double *lvl = ws.buf<double>("fsm.lake_spill", std::max<uint32_t>(L, 1u)), *hl = ws.buf<double>("fsm.lake_level", std::max<uint32_t>(L, 1u));
  if (L) {
    fsm_up(d_top, tops, s);
    fsm_up(d_prank, prank, s);
    fsm_up(d_pw, pw, s);
  }
  fsm_up(d_lol, lake_of_leaf, s);
  if (d_nw) fsm_up(d_nw, wn, s);
  RD_HIP(hipStreamSynchronize(s));   // (the vectors above are pageable and go out of scope with this call)
  if (pf.enabled) pf.end(s);
  st.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  if (L) RD_LAUNCH("fsm.lakes", k_fsm_lakes, dim3(cdiv(L, NTHR)), dim3(NTHR), 0, s, d_table, (const uint32_t *)d_top,
                   (const uint32_t *)d_prank, lvl, hl, L);
  if (Lp) {
    const FsmRecord<T> rec{d_z, d_labels, d_lol, d_prank, lvl, P};
    RD_HIP(hipMemsetAsync(total, 0, sizeof(unsigned long long), s));
    RD_LAUNCH("fsm.count", (k_fsm_count<T>), dim3(rgrid), dim3(NTHR), 0, s, rec, n, total);
    unsigned long long *hq = reinterpret_cast<unsigned long long *>(ws.host_words());
    RD_HIP(hipMemcpyAsync(hq, total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    const uint32_t R = (uint32_t)hq[0];   // (at most n, which is below 2^31)
    st.records = R;
    uint32_t *segstart = ws.buf<uint32_t>("fsm.seg_start", Lp), *kmin = ws.buf<uint32_t>("fsm.seg_min", Lp);
    RD_HIP(hipMemsetAsync(segstart, 0xFF, (size_t)Lp * sizeof(uint32_t), s));
    RD_HIP(hipMemsetAsync(kmin, 0xFF, (size_t)Lp * sizeof(uint32_t), s));
    double *S = nullptr;
    if (R) {
      uint32_t *cells = ws.buf<uint32_t>("fsm.cells", R), *scells = ws.buf<uint32_t>("fsm.scells", R), *seg = ws.buf<uint32_t>("fsm.seg", R);
      unsigned long long *keys = ws.buf<unsigned long long>("fsm.keys", R), *skeys = ws.buf<unsigned long long>("fsm.skeys", R);
      double *val = ws.buf<double>("fsm.val", R);
      S = ws.buf<double>("fsm.prefix", R);
      int rbits = 1;
      while ((1ull << rbits) < (unsigned long long)Lp) rbits++;
      const int end_bit = fsm_key_bits<T>() + rbits;
      st.sort_bits = (uint32_t)end_bit;
      hipcub::CountingInputIterator<uint32_t> all(0u);
      uint32_t *nsel = &words->records;
      size_t b1 = 0, b2 = 0, b3 = 0;
      RD_HIP(hipcub::DeviceSelect::If(nullptr, b1, all, cells, nsel, (int)n, rec, s));
      RD_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b2, keys, skeys, cells, scells, (int)R, 0, end_bit, s));
      RD_HIP(hipcub::DeviceScan::InclusiveSumByKey(nullptr, b3, seg, val, S, (int)R, hipcub::Equality(), s));
      void *tmp = ws.buf("fsm.cub_tmp", std::max(b1, std::max(b2, b3)));
      if (pf.enabled) pf.begin("fsm.select", s);
      RD_HIP(hipcub::DeviceSelect::If(tmp, b1, all, cells, nsel, (int)n, rec, s));   // (the same predicate: exactly R cells)
      if (pf.enabled) pf.end(s);
      RD_LAUNCH("fsm.keys", (k_fsm_keys<T>), dim3(cdiv(R, NTHR)), dim3(NTHR), 0, s, rec, (const uint32_t *)cells, keys, R);
      if (pf.enabled) pf.begin("fsm.sort", s);
      RD_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, b2, keys, skeys, cells, scells, (int)R, 0, end_bit, s));
      if (pf.enabled) pf.end(s);
      RD_LAUNCH("fsm.vals", (k_fsm_vals<T>), dim3(cdiv(R, NTHR)), dim3(NTHR), 0, s, d_z, (const unsigned long long *)skeys,
                (const uint32_t *)scells, seg, val, segstart, R, Lp);
      if (pf.enabled) pf.begin("fsm.scan", s);
      RD_HIP(hipcub::DeviceScan::InclusiveSumByKey(tmp, b3, seg, val, S, (int)R, hipcub::Equality(), s));
      if (pf.enabled) pf.end(s);
      RD_LAUNCH("fsm.level", k_fsm_level, dim3(cdiv(R, NTHR)), dim3(NTHR), 0, s, (const uint32_t *)seg, (const double *)val,
                (const double *)S, (const uint32_t *)segstart, (const double *)d_pw, kmin, R);
    }
    RD_LAUNCH("fsm.height", k_fsm_height, dim3(cdiv(L, NTHR)), dim3(NTHR), 0, s, (const uint32_t *)d_prank, (const double *)S,
              (const uint32_t *)segstart, (const uint32_t *)kmin, (const double *)d_pw, hl, L);
  }
  RD_LAUNCH("fsm.depth", (k_fsm_depth<T>), dim3(rgrid), dim3(NTHR), 0, s, d_z, d_labels, (const uint32_t *)d_lol, (const double *)hl,
            d_depth, n, L ? P : 0u, words);
  if (d_result) {
    hipLaunchKernelGGL(k_fsm_result, dim3(1), dim3(1), 0, s, d_result, water_in, ocean, L, L - Lp, (const FsmWords *)words);
    RD_HIP(hipGetLastError());
  }
  fsm_last = st;
}

// host-pointer form: H2D, the device form, D2H of the depth, the node water and the result
template <class T>
static void fsm_host(const T *dem, int w, int h, const int32_t *labels, const rdgpu_dephier_node *table, uint32_t count,
                     const double *water, double *depth, double *node_water, rdgpu_fsm_result *result) {
  check_fsm_args(dem, w, h, labels, table, count, water, depth);
  const size_t n = (size_t)w * h;
  HostStage st;
  const T *d = st.in("host.dem", dem, n);
  const int32_t *dl = st.in("fsm.host.labels", labels, n);
  const rdgpu_dephier_node *dt = count ? st.in("fsm.host.table", table, count) : nullptr;
  const double *dw = st.in("fsm.host.water", water, n);
  double *dd = st.out("fsm.host.depth", depth, n);
  double *dn = count ? st.out("fsm.host.node_water", node_water, count) : nullptr;
  rdgpu_fsm_result *dr = st.out("fsm.host.result", result, 1);
  fsm_device<T>(d, w, h, dl, dt, count, dw, dd, dn, dr, nullptr);
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

#define RD_FSM_API(SUF, T)                                                                                            \
  extern "C" int rdgpu_fill_spill_merge_##SUF(const T *dem, int w, int h, const int32_t *labels,                      \
                                              const rdgpu_dephier_node *table, uint32_t count, const double *water,   \
                                              double *depth, double *node_water, rdgpu_fsm_result *result) {          \
    return guarded([&] { fsm_host<T>(dem, w, h, labels, table, count, water, depth, node_water, result); });          \
  }                                                                                                                   \
  extern "C" int rdgpu_fill_spill_merge_dev_##SUF(const T *d_dem, int w, int h, const int32_t *d_labels,              \
                                                  const rdgpu_dephier_node *d_table, uint32_t count,                  \
                                                  const double *d_water, double *d_depth, double *d_node_water,       \
                                                  rdgpu_fsm_result *d_result, void *stream) {                         \
    return guarded([&] {                                                                                              \
      fsm_device<T>(d_dem, w, h, d_labels, d_table, count, d_water, d_depth, d_node_water, d_result, (hipStream_t)stream); \
    });                                                                                                               \
  }
RD_FSM_API(u8, uint8_t)
RD_FSM_API(i8, int8_t)
RD_FSM_API(i16, int16_t)
RD_FSM_API(u16, uint16_t)
RD_FSM_API(i32, int32_t)
RD_FSM_API(u32, uint32_t)
RD_FSM_API(f32, float)

// the hierarchy has no 64-bit entries either: there is no table to hand in
#define RD_FSM_UNSUPPORTED(SUF, T)                                                                                    \
  extern "C" int rdgpu_fill_spill_merge_##SUF(const T *, int, int, const int32_t *, const rdgpu_dephier_node *, uint32_t, \
                                              const double *, double *, double *, rdgpu_fsm_result *) {               \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_fill_spill_merge: 64-bit elevations are not supported"); }); \
  }                                                                                                                   \
  extern "C" int rdgpu_fill_spill_merge_dev_##SUF(const T *, int, int, const int32_t *, const rdgpu_dephier_node *,   \
                                                  uint32_t, const double *, double *, double *, rdgpu_fsm_result *,   \
                                                  void *) {                                                           \
    return guarded([&] { throw Error(RDGPU_ERR_UNSUPPORTED, "rdgpu_fill_spill_merge: 64-bit elevations are not supported"); }); \
  }
RD_FSM_UNSUPPORTED(f64, double)
RD_FSM_UNSUPPORTED(i64, int64_t)
RD_FSM_UNSUPPORTED(u64, uint64_t)

extern "C" int rdgpu_fsm_get_stats(rdgpu_fsm_stats *out) {
  if (!out) return RDGPU_ERR_ARG;
  *out = fsm_last;
  return RDGPU_OK;
}
