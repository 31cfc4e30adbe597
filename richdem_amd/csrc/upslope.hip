// upslope.hip -- membership on the D8 direction forest: catchments of seed cells, outlets (the drainage-basin map) and
// the reference's d8_upslope_cells (include/richdem/methods/d8_methods.hpp:144-236).
//
// "The path of cell c" is c, the cell c's direction points to, and so on; it ends at a cell without a direction 1..8 or
// whose target is off the raster.  The reference expands upstream from a rasterised line with a serial FIFO.  Here the
// answer found DOWNSTREAM is brought back up, with the machinery of accum.hip's tile links run the other way round:
//   1. k_up_tile    every 64 x 64 tile on its own: the directions staged in LDS, every cell pointer-jumped to the in-tile
//                   end of its path -- a seed, a cell without a target, or an EXIT (a cell whose target lies in another
//                   tile).  Only the tile's 252 border cells publish: one 64-bit node each, either RESOLVED with the
//                   answer of its in-tile end, or the node of the neighbouring tile's border cell its exit flows to.
//   2. k_up_round   pointer doubling over the nodes, in place: an unresolved node takes the word of the node it points
//                   to.  ceil(log2(nodes)) + 1 rounds at most; a round whose predecessor left nothing unresolved returns
//                   at once (a device-side flag, no host synchronisation).  What is unresolved after the last round runs
//                   round a direction loop and has no answer.
//   3. k_up_final   every tile again: the in-tile ends recomputed in LDS (cheaper than a per-cell root in memory), an
//                   exit's answer read from the node it flows to, every cell written once.
// Seeds cost no raster of their own: the OUTPUT raster holds them between the passes.  Only tiles that contain a seed
// are initialised and read back (a flag per tile), so a handful of pour points costs nothing per cell.  The position of a
// seed in the caller's list is scattered with atomicMin: of two entries for one cell the first wins, deterministically.
#include "d8_forest.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace rdgpu {

constexpr uint32_t UP_NONE = 0xFFFFFFFFu;
constexpr unsigned long long UP_RESOLVED = 1ull << 63;
enum { UP_CATCH = 0, UP_OUTLET = 1, UP_CELLS = 2 };   // int32 labels | uint32 outlet indices | the reference's 2 / 1 / 255

template <int MODE> struct UpOut { using type = int32_t; };
template <> struct UpOut<UP_OUTLET> { using type = uint32_t; };
template <> struct UpOut<UP_CELLS> { using type = uint8_t; };

struct UpTile {   // a tile's LDS state
  uint8_t sd[SDH * SDW] __attribute__((aligned(4)));   // staged directions (tile_front.hpp)
  uint16_t lp[LT * LPS];                               // per cell: a tile pointer (d8_forest.hpp), FOREST_END once that cell is known to be its end
  uint32_t sv[LT * LPS];                               // per cell: position of the seed on it in the seed list (UP_NONE: none); k_up_final: the ends' answers
};

// the link of the cell at (lx, ly): 0 none (the path ends here), 1 to (tx, ty) inside the tile, 2 to (tx, ty) in another tile.
// Catchments follow a direction onto any cell of the raster (a NoData cell may be a seed); outlets stop BEFORE a NoData
// cell (the outlet is the path's last cell that is not NoData).
template <int MODE>
__device__ __forceinline__ int up_link(const uint8_t *sd, int lx, int ly, int x0, int y0, int w, int h, uint8_t nodata, int &tx,
                                       int &ty) {
  const uint32_t d = sd[(ly + 1) * SDW + SDO + lx];
  tx = lx; ty = ly;
  if (d == nodata || d - 1u >= 8u) return 0;
  tx = lx + d8dx((int)d); ty = ly + d8dy((int)d);
  const int gx = x0 + tx, gy = y0 + ty;
  if (gx < 0 || gy < 0 || gx >= w || gy >= h) return 0;
  if (MODE == UP_OUTLET && sd[(ty + 1) * SDW + SDO + tx] == nodata) return 0;
  return (tx >= 0 && tx < LT && ty >= 0 && ty < LT) ? 1 : 2;
}

// Stages the tile, loads its seeds and pointer-jumps every cell to the in-tile end of its path: p[j] is the end of the
// thread's cell (lx, ly0 + 4 j) where it carries FOREST_END (an end itself has self | FOREST_END); a cell whose pointer
// does not runs into a direction loop inside the tile.  Returns the mask of the thread's cells that are seeds.
template <int MODE>
__device__ __forceinline__ uint32_t up_tile_ends(UpTile &T, const uint8_t *__restrict__ dirs, uint8_t nodata, int w, int h, int x0,
                                                 int y0, const typename UpOut<MODE>::type *seeds, bool has_seeds,
                                                 uint32_t (&p)[FOREST_RPT]) {
  stage_dirs_rows(dirs, w, h, x0, y0, nodata, T.sd);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t seedmask = 0;
  uint32_t sidx[FOREST_RPT];
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j, gx = x0 + lx, gy = y0 + ly;
    uint32_t s = UP_NONE;
    if (MODE != UP_OUTLET && has_seeds && gx < w && gy < h) {
      const size_t g = (size_t)gy * w + gx;
      if (MODE == UP_CELLS) s = seeds[g] == 2 ? 0u : UP_NONE;
      else s = (uint32_t)seeds[g];
    }
    sidx[j] = s;
    seedmask |= (s != UP_NONE ? 1u : 0u) << j;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    int tx, ty;
    const int k = up_link<MODE>(T.sd, lx, ly, x0, y0, w, h, nodata, tx, ty);
    p[j] = (k == 1 && sidx[j] == UP_NONE) ? (uint32_t)(ty * LPS + tx) : (self | FOREST_END);   // a seed absorbs, like an exit or a sink
    T.lp[self] = (uint16_t)p[j];
    T.sv[self] = sidx[j];
  }
  __syncthreads();
  // two hops per trip: a trip at least triples the distance covered, twelve trips cover any loop-free path of 4096 cells;
  // what still moves then runs round a direction loop
#pragma unroll 1
  for (int it = 0; it < 12; it++) {
    bool moving = false;
#pragma unroll
    for (int j = 0; j < FOREST_RPT; j++) {
      const uint32_t q = (p[j] & FOREST_END) ? p[j] : T.lp[p[j]];
      const uint32_t r = (q & FOREST_END) ? q : T.lp[q];
      moving |= !(r & FOREST_END);
      p[j] = r;
      T.lp[(ly0 + 4 * j) * LPS + lx] = (uint16_t)r;
    }
    if (!__syncthreads_or(moving)) break;
  }
  __syncthreads();
  return seedmask;
}

// the answer carried by a seed
template <int MODE>
__device__ __forceinline__ uint32_t up_seed_value(uint32_t pos, const int32_t *__restrict__ seed_labels) {
  return MODE == UP_CELLS ? 1u : (uint32_t)seed_labels[pos];
}

template <int MODE>
__global__ __launch_bounds__(NTHR, 5) void k_up_tile(const uint8_t *__restrict__ dirs, uint8_t nodata, int w, int h, uint32_t tilesX,
                                                     uint32_t ntiles, const typename UpOut<MODE>::type *seeds,
                                                     const uint8_t *__restrict__ tileflag, const int32_t *__restrict__ seed_labels,
                                                     uint32_t none, unsigned long long *__restrict__ node) {
  __shared__ UpTile T;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  const bool has_seeds = MODE != UP_OUTLET && tileflag[t] != 0;
  uint32_t p[FOREST_RPT];
  up_tile_ends<MODE>(T, dirs, nodata, w, h, x0, y0, seeds, has_seeds, p);
  // what a path that ENTERS the tile at a border cell comes to, one border cell per thread
  const int slot = (int)threadIdx.x;
  unsigned long long word = UP_RESOLVED | none;   // (the four spare slots; a path into an in-tile loop)
  if (slot < BORDER_SLOTS) {
    int bx, by;
    border_cell(slot, bx, by);
    const uint32_t rp = T.lp[by * LPS + bx], root = rp & FOREST_CELL;
    if (rp & FOREST_END) {
      const int ry = (int)root / LPS, rx = (int)root - ry * LPS;
      const uint32_t s = T.sv[root];
      int tx, ty;
      if (s != UP_NONE) word = UP_RESOLVED | up_seed_value<MODE>(s, seed_labels);
      else if (up_link<MODE>(T.sd, rx, ry, x0, y0, w, h, nodata, tx, ty) == 2) word = tile_node(x0 + tx, y0 + ty, tilesX);
      else if (MODE == UP_OUTLET && T.sd[(ry + 1) * SDW + SDO + rx] != nodata) word = UP_RESOLVED | ((uint32_t)(y0 + ry) * (uint32_t)w + (uint32_t)(x0 + rx));
    }
  }
  node[(size_t)t * TILE_SLOTS + slot] = word;
}

// flags[r]: round r left a node unresolved
__global__ __launch_bounds__(NTHR) void k_up_round(unsigned long long *node, uint64_t nnodes, uint32_t *flags, int r) {
  if (r > 0 && flags[r - 1] == 0) return;
  const uint64_t i = (uint64_t)blockIdx.x * NTHR + threadIdx.x;
  bool open = false;
  if (i < nnodes) {
    const unsigned long long v = node[i];
    if (!(v & UP_RESOLVED)) {
      const unsigned long long nx = node[(uint32_t)v];   // (in place: whichever word is read, old or new, lies further down the path)
      node[i] = nx;
      open = !(nx & UP_RESOLVED);
    }
  }
  if (__any(open) && (threadIdx.x & 63) == 0) flags[r] = 1;
}

template <int MODE>
__global__ __launch_bounds__(NTHR, 5) void k_up_final(const uint8_t *__restrict__ dirs, uint8_t nodata, int w, int h, uint32_t tilesX,
                                                      uint32_t ntiles, const uint8_t *__restrict__ tileflag,
                                                      const int32_t *__restrict__ seed_labels, uint32_t none,
                                                      const unsigned long long *__restrict__ node,
                                                      typename UpOut<MODE>::type *out) {
  using O = typename UpOut<MODE>::type;
  __shared__ UpTile T;
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  const bool has_seeds = MODE != UP_OUTLET && tileflag[t] != 0;
  uint32_t p[FOREST_RPT];
  const uint32_t seedmask = up_tile_ends<MODE>(T, dirs, nodata, w, h, x0, y0, out, has_seeds, p);
  const int lx = threadIdx.x & (LT - 1), ly0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // the ends' answers: every end is some thread's own cell (all node reads of the block in flight together)
  uint32_t endmask = 0;
  unsigned long long nv[FOREST_RPT];
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    nv[j] = 0;
    if (p[j] != ((uint32_t)(ly * LPS + lx) | FOREST_END) || (seedmask >> j & 1u)) continue;
    int tx, ty;
    if (up_link<MODE>(T.sd, lx, ly, x0, y0, w, h, nodata, tx, ty) == 2) {
      nv[j] = node[tile_node(x0 + tx, y0 + ty, tilesX)];
      endmask |= 1u << j;
    }
  }
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j;
    const uint32_t self = (uint32_t)(ly * LPS + lx);
    if (p[j] != (self | FOREST_END)) continue;
    uint32_t a = none;
    if (seedmask >> j & 1u) a = up_seed_value<MODE>(T.sv[self], seed_labels);
    else if (endmask >> j & 1u) a = (nv[j] & UP_RESOLVED) ? (uint32_t)nv[j] : none;
    else if (MODE == UP_OUTLET && T.sd[(ly + 1) * SDW + SDO + lx] != nodata) a = (uint32_t)(y0 + ly) * (uint32_t)w + (uint32_t)(x0 + lx);
    T.sv[self] = a;   // (its seed position is read by nobody else)
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < FOREST_RPT; j++) {
    const int ly = ly0 + 4 * j, gx = x0 + lx, gy = y0 + ly;
    if (gx >= w || gy >= h) continue;
    uint32_t a = (p[j] & FOREST_END) ? T.sv[p[j] & FOREST_CELL] : none;   // else: into a direction loop inside the tile
    if (MODE == UP_CELLS && (seedmask >> j & 1u)) a = 2u;
    out[(size_t)gy * w + gx] = (O)a;
  }
}

// ---- seeds ------------------------------------------------------------------------------------------------------------
// bad[0]: a seed cell lies outside the raster; tileflag: the tiles that hold a seed
__global__ __launch_bounds__(NTHR) void k_up_seed_tiles(const uint32_t *__restrict__ cells, uint32_t n, int w, uint64_t ncells,
                                                        uint32_t tilesX, uint8_t *tileflag, uint32_t *bad) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cells[i];
  if (c >= ncells) { *bad = 1; return; }
  tileflag[(c / (uint32_t)w / LT) * tilesX + (c % (uint32_t)w) / LT] = 1;
}
template <class O>
__global__ __launch_bounds__(NTHR) void k_up_seed_init(O *out, const uint8_t *__restrict__ tileflag, int w, int h, uint32_t tilesX) {
  const uint32_t t = blockIdx.x;
  if (!tileflag[t]) return;
  const int x0 = (int)(t % tilesX) * LT, y0 = (int)(t / tilesX) * LT;
  for (int i = (int)threadIdx.x; i < LT * LT; i += NTHR) {
    const int gx = x0 + (i & (LT - 1)), gy = y0 + i / LT;
    if (gx < w && gy < h) out[(size_t)gy * w + gx] = (O)UP_NONE;
  }
}
template <class O>
__global__ __launch_bounds__(NTHR) void k_up_seed_scatter(const uint32_t *__restrict__ cells, uint32_t n, O *out) {
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  if (i >= n) return;
  if (sizeof(O) == 1) out[cells[i]] = (O)2;
  else atomicMin(reinterpret_cast<uint32_t *>(out) + cells[i], i);   // the first entry of the list wins
}

// ---- drivers ----------------------------------------------------------------------------------------------------------
// seeds_checked: the caller has verified every seed cell (host entries); else they are verified here, which costs the
// one host synchronisation of the call
template <int MODE>
static void upslope_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, const uint32_t *d_cells, const int32_t *d_labels,
                           uint32_t n_seeds, uint32_t none, typename UpOut<MODE>::type *d_out, hipStream_t s, bool seeds_checked,
                           const char *who) {
  using O = typename UpOut<MODE>::type;
  if (!d_dirs || !d_out) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_forest_dims(w, h, who);
  if (MODE != UP_OUTLET && n_seeds && (!d_cells || (MODE == UP_CATCH && !d_labels)))
    throw Error(RDGPU_ERR_ARG, std::string(who) + ": null seed array");
  if (n_seeds == UP_NONE) throw Error(RDGPU_ERR_ARG, std::string(who) + ": too many seeds");
  const ForestDims fd(w, h);
  const uint32_t tilesX = fd.tilesX, ntiles = fd.ntiles;
  const uint64_t nnodes = fd.nnodes;
  Workspace &ws = Workspace::get();
  unsigned long long *node = ws.buf<unsigned long long>("upslope.node", nnodes);
  uint8_t *tileflag = ws.buf<uint8_t>("upslope.tileflag", ntiles);
  const int rounds = forest_rounds(nnodes);
  uint32_t *flags = ws.buf<uint32_t>("upslope.flags", (size_t)rounds + 1);   // [rounds]: a seed outside the raster
  RD_HIP(hipMemsetAsync(flags, 0, ((size_t)rounds + 1) * sizeof(uint32_t), s));
  if (MODE != UP_OUTLET) {
    RD_HIP(hipMemsetAsync(tileflag, 0, ntiles, s));
    if (n_seeds) {
      const uint32_t sg = (n_seeds + NTHR - 1) / NTHR;
      RD_LAUNCH("upslope.seed_tiles", k_up_seed_tiles, dim3(sg), dim3(NTHR), 0, s, d_cells, n_seeds, w, (uint64_t)w * h, tilesX,
                tileflag, flags + rounds);
      if (!seeds_checked) {   // nothing of the output has been written yet
        uint32_t *hw = ws.host_words();
        RD_HIP(hipMemcpyAsync(hw, flags + rounds, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        RD_HIP(hipStreamSynchronize(s));
        if (hw[0]) throw Error(RDGPU_ERR_ARG, std::string(who) + ": a seed cell lies outside the raster");
      }
      RD_LAUNCH("upslope.seed_init", (k_up_seed_init<O>), dim3(ntiles), dim3(NTHR), 0, s, d_out, (const uint8_t *)tileflag, w, h,
                tilesX);
      RD_LAUNCH("upslope.seed_scatter", (k_up_seed_scatter<O>), dim3(sg), dim3(NTHR), 0, s, d_cells, n_seeds, d_out);
    }
  }
  RD_LAUNCH("upslope.tile", (k_up_tile<MODE>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, w, h, tilesX, ntiles,
            (const O *)d_out, (const uint8_t *)tileflag, d_labels, none, node);
  const uint32_t ngrid = (uint32_t)((nnodes + NTHR - 1) / NTHR);
  for (int r = 0; r < rounds; r++) RD_LAUNCH("upslope.round", k_up_round, dim3(ngrid), dim3(NTHR), 0, s, node, nnodes, flags, r);
  RD_LAUNCH("upslope.final", (k_up_final<MODE>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_dirs, nodata, w, h, tilesX, ntiles,
            (const uint8_t *)tileflag, d_labels, none, (const unsigned long long *)node, d_out);
}

// The reference's "modified Bresenham" (d8_methods.hpp:186-212), oddities included: the line is the function's input
// contract.  float error term and slope; per column the cell (x, y), and when the error reaches 0.5 also (x + 1, y)
// before y moves by one.  Where the reference would mark a cell outside the raster (undefined behaviour there) this
// throws.
static std::vector<uint32_t> upslope_line(int w, int h, int x0, int y0, int x1, int y1, const char *who) {
  check_forest_dims(w, h, who);
  if (x0 > x1) { std::swap(x0, x1); std::swap(y0, y1); }
  const Error outside(RDGPU_ERR_ARG, std::string(who) + ": the line leaves the raster");
  if (x0 < 0 || x1 >= w || y0 < 0 || y0 >= h) throw outside;   // (x0, y0) and a cell of column x1 are always marked
  const long long deltax = (long long)x1 - x0, deltay = (long long)y1 - y0;
  float error = 0;
  float deltaerr = (float)deltay / (float)deltax;
  if (deltaerr < 0) deltaerr = -deltaerr;
  const int step = deltay > 0 ? 1 : deltay < 0 ? -1 : 0;
  std::vector<uint32_t> cells;
  int y = y0;
  for (int x = x0; x <= x1; x++) {
    if (y < 0 || y >= h) throw outside;
    cells.push_back((uint32_t)y * (uint32_t)w + (uint32_t)x);
    error += deltaerr;
    if (error >= 0.5f) {
      if (x + 1 >= w) throw outside;
      cells.push_back((uint32_t)y * (uint32_t)w + (uint32_t)(x + 1));
      y += step;
      error -= 1;
    }
  }
  return cells;
}

static void upslope_cells_device(const uint8_t *d_dirs, uint8_t nodata, int w, int h, int x0, int y0, int x1, int y1, uint8_t *d_out,
                                 hipStream_t s, const char *who) {
  if (!d_dirs || !d_out) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  const std::vector<uint32_t> line = upslope_line(w, h, x0, y0, x1, y1, who);
  uint32_t *d_cells = Workspace::get().buf<uint32_t>("upslope.line", line.size());
  RD_HIP(hipMemcpyAsync(d_cells, line.data(), line.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));   // (pageable: staged before it returns)
  upslope_device<UP_CELLS>(d_dirs, nodata, w, h, d_cells, nullptr, (uint32_t)line.size(), 255u, d_out, s, true, who);
}

// host rasters: staged in the workspace, as d8_flow_accum's
template <int MODE>
static void upslope_host(const uint8_t *dirs, uint8_t nodata, int w, int h, const uint32_t *cells, const int32_t *labels,
                         uint32_t n_seeds, uint32_t none, int x0, int y0, int x1, int y1, typename UpOut<MODE>::type *out,
                         const char *who) {
  using O = typename UpOut<MODE>::type;
  if (!dirs || !out) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null pointer");
  check_forest_dims(w, h, who);
  const size_t n = (size_t)w * h;
  std::vector<uint32_t> line;
  if (MODE == UP_CELLS) line = upslope_line(w, h, x0, y0, x1, y1, who);
  if (MODE == UP_CATCH && n_seeds) {
    if (!cells || !labels) throw Error(RDGPU_ERR_ARG, std::string(who) + ": null seed array");
    for (uint32_t i = 0; i < n_seeds; i++)
      if (cells[i] >= n) throw Error(RDGPU_ERR_ARG, std::string(who) + ": a seed cell lies outside the raster");
  }
  HostStage st;
  const uint8_t *dd = st.in("host.dirs", dirs, n);
  O *dout = st.out("host.upslope", out, n);
  if (MODE == UP_CELLS) {
    upslope_cells_device(dd, nodata, w, h, x0, y0, x1, y1, reinterpret_cast<uint8_t *>(dout), nullptr, who);
  } else {
    const bool seeds = MODE == UP_CATCH && n_seeds;
    const uint32_t *dc = st.in("host.seed_cells", seeds ? cells : nullptr, n_seeds);
    const int32_t *dl = st.in("host.seed_labels", seeds ? labels : nullptr, n_seeds);
    upslope_device<MODE>(dd, nodata, w, h, dc, dl, n_seeds, none, dout, nullptr, true, who);
  }
  st.finish();
}

}  // namespace rdgpu

using namespace rdgpu;

extern "C" int rdgpu_d8_catchments(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint32_t *seed_cells,
                                   const int32_t *seed_labels, uint32_t n_seeds, int32_t unreached, int32_t *labels) {
  return guarded([&] {
    upslope_host<UP_CATCH>(dirs, dir_nodata, width, height, seed_cells, seed_labels, n_seeds, (uint32_t)unreached, 0, 0, 0, 0, labels,
                           "rdgpu_d8_catchments");
  });
}
extern "C" int rdgpu_d8_catchments_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, const uint32_t *d_seed_cells,
                                       const int32_t *d_seed_labels, uint32_t n_seeds, int32_t unreached, int32_t *d_labels,
                                       void *hip_stream) {
  return guarded([&] {
    upslope_device<UP_CATCH>(d_dirs, dir_nodata, width, height, d_seed_cells, d_seed_labels, n_seeds, (uint32_t)unreached, d_labels,
                             (hipStream_t)hip_stream, false, "rdgpu_d8_catchments_dev");
  });
}
extern "C" int rdgpu_d8_outlets(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, uint32_t *outlet) {
  return guarded([&] {
    upslope_host<UP_OUTLET>(dirs, dir_nodata, width, height, nullptr, nullptr, 0, UP_NONE, 0, 0, 0, 0, outlet, "rdgpu_d8_outlets");
  });
}
extern "C" int rdgpu_d8_outlets_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, uint32_t *d_outlet,
                                    void *hip_stream) {
  return guarded([&] {
    upslope_device<UP_OUTLET>(d_dirs, dir_nodata, width, height, nullptr, nullptr, 0, UP_NONE, d_outlet, (hipStream_t)hip_stream, true,
                              "rdgpu_d8_outlets_dev");
  });
}
extern "C" int rdgpu_d8_upslope_cells(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, int x0, int y0, int x1, int y1,
                                      uint8_t *out) {
  return guarded([&] {
    upslope_host<UP_CELLS>(dirs, dir_nodata, width, height, nullptr, nullptr, 0, 255u, x0, y0, x1, y1, out, "rdgpu_d8_upslope_cells");
  });
}
extern "C" int rdgpu_d8_upslope_cells_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, int x0, int y0, int x1,
                                          int y1, uint8_t *d_out, void *hip_stream) {
  return guarded([&] {
    upslope_cells_device(d_dirs, dir_nodata, width, height, x0, y0, x1, y1, d_out, (hipStream_t)hip_stream, "rdgpu_d8_upslope_cells_dev");
  });
}

// host code only: no device is touched (and none is needed), hence no `guarded`
extern "C" int rdgpu_d8_upslope_line(int width, int height, int x0, int y0, int x1, int y1, uint32_t *cells, uint32_t capacity,
                                     uint32_t *n) {
  try {
    if (!n) throw Error(RDGPU_ERR_ARG, "rdgpu_d8_upslope_line: null pointer");
    const std::vector<uint32_t> line = upslope_line(width, height, x0, y0, x1, y1, "rdgpu_d8_upslope_line");
    *n = (uint32_t)line.size();
    if (!cells && capacity == 0) return RDGPU_OK;   // the count alone
    if (!cells || capacity < line.size()) throw Error(RDGPU_ERR_ARG, "rdgpu_d8_upslope_line: capacity too small");
    std::copy(line.begin(), line.end(), cells);
    return RDGPU_OK;
  } catch (const Error &e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return RDGPU_ERR_HIP;
  }
}
