/* rdgpu.h -- C-ABI of librdgpu.so, the MI355X (gfx950) engine behind RichDEM's
 * FillDepressions / pit_mask / d8_flow_directions / barnes_flat_resolution_d8 / ResolveFlatsEpsilon /
 * d8_flow_accum / FA_D8 / FA_Tarboton / FA_Quinn / FA_Holmgren / FA_Freeman / FlowAccumulation(props).
 *
 * NaN elevations are unsupported input throughout (the reference's heaps and compares give them no defined place either;
 * a float NoData value must be a number -- NaN never equals itself, so NaN "NoData" cells would count as data).
 *
 * Plain pointers and sizes only.  Rasters are dense row-major, i = y*width + x,
 * no padding (reference: include/richdem/common/Array2D.hpp:592-595).  All
 * functions return 0 on success and a non-zero code on failure; the message is
 * available from rdgpu_last_error().  The C++ shim include/rdgpu/richdem_gpu.hpp
 * turns non-zero into std::runtime_error, the reference's error convention.
 *
 * Two families:
 *   rdgpu_<op>_<dtype>(host pointers...)       drop-in boundary: H2D, compute, D2H
 *                                              into the SAME host buffer
 *   rdgpu_<op>_dev_<dtype>(device pointers...) HBM-resident variant (bench.py,
 *                                              multi-GPU shards, chaining stages)
 *
 * dtype suffixes: i8 u8 i16 u16 i32 u32 f32 everywhere; f64 i64 u64 additionally for the fill (exact: f64 through the f32
 * engine when the values fit, 64-bit values through dense value ranks otherwise), for d8_flow_directions, flat
 * resolution, ResolveFlatsEpsilon and FA_D8 / FM_D8 (these compare elevations in their own type); the D-infinity / MFD
 * families take i8 ... f64.  The row-block shard entry points of the fill take the 8 / 16 / 32-bit types.
 *
 * Threading: every entry point runs under the lock OF THE DEVICE that is current when it is entered (not a process-wide
 * lock): calls from several host threads on ONE device (e.g. Python threads with the GIL released by the wrapper) are
 * safe and run one after the other -- when the calling thread changes, that device is synchronised first, because its
 * calls share one grow-only workspace -- while threads on DIFFERENT devices run side by side.  The single-process
 * multi-device entry points (rdgpu_*_multi_*, and the plain host entries when RDGPU_DEVICES routes them there) run one
 * orchestrator at a time per process and must not be called from inside one another.
 * Streams: the `_dev_` entry points enqueue on the stream they are given and use that shared per-device workspace for
 * their scratch.  Issue all `_dev_` calls of a process on ONE stream per device, or synchronise between calls issued on
 * different streams -- two calls in flight on two streams would overwrite each other's scratch.  (The handle-based shard
 * entry points keep their state in buffers of their own.)
 */
#ifndef RDGPU_H_
#define RDGPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDGPU_OK 0
#define RDGPU_ERR_HIP 1         /* a HIP runtime call failed (no GPU, OOM, ...) */
#define RDGPU_ERR_ARG 2         /* bad dimensions / null pointer / bad topology  */
#define RDGPU_ERR_UNSUPPORTED 3 /* dtype not supported by this build             */
#define RDGPU_ERR_CAPACITY 4    /* rdgpu_fill_graph_solve_dev: a count in d_counts exceeds `cap` -- that shard's edges are
                                   not in d_edges_all; nothing was solved (the caller repeats its exchange with more room) */

/* ---- runtime ---------------------------------------------------------------------------- */
const char *rdgpu_last_error(void);
const char *rdgpu_version(void);
int rdgpu_device_count(int *count);
int rdgpu_set_device(int device_id);
/* Free the grow-only device workspace cached between calls. */
int rdgpu_release_workspace(void);

/* ---- FillDepressions<topology>(Array2D<T>&) -----------------------------------------------
 * Replaces richdem::FillDepressions (include/richdem/depressions/depressions.hpp:13-21), i.e.
 * PriorityFlood_Zhou2016 (depressions/Zhou2016.hpp:126-191) for topology 8 and
 * PriorityFlood_Barnes2014<D4> (depressions/Barnes2014.hpp:230-304) for topology 4.
 * In place; NoData is an ordinary elevation, exactly as in the reference. */
int rdgpu_fill_u8(uint8_t *dem, int width, int height, int topology);
int rdgpu_fill_i16(int16_t *dem, int width, int height, int topology);
int rdgpu_fill_u16(uint16_t *dem, int width, int height, int topology);
int rdgpu_fill_i32(int32_t *dem, int width, int height, int topology);
int rdgpu_fill_u32(uint32_t *dem, int width, int height, int topology);
int rdgpu_fill_f32(float *dem, int width, int height, int topology);
int rdgpu_fill_i8(int8_t *dem, int width, int height, int topology);
/* 64-bit element types: exact as well -- f64 DEMs whose values fit f32 run the f32 engine, everything
 * else is filled on dense ranks of the values (csrc/fill64.hip). */
int rdgpu_fill_f64(double *dem, int width, int height, int topology);
int rdgpu_fill_i64(int64_t *dem, int width, int height, int topology);
int rdgpu_fill_u64(uint64_t *dem, int width, int height, int topology);

int rdgpu_fill_dev_u8(uint8_t *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_i16(int16_t *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_u16(uint16_t *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_i32(int32_t *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_u32(uint32_t *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_f32(float *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_i8(int8_t *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_f64(double *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_i64(int64_t *d_dem, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_dev_u64(uint64_t *d_dem, int width, int height, int topology, void *hip_stream);

/* HasDepressions<topology>(const Array2D<T>&) (depressions/Barnes2014.hpp:44-103; apps/rd_depressions_has.cpp:14):
 * *out = 1 when the DEM holds a depression, i.e. when FillDepressions<topology> would raise at least one cell (the
 * reference runs the flood of PriorityFlood_Original without raising and stops at the first cell discovered from a higher
 * one, :91-95 -- the same predicate whatever its heap does among equal keys), 0 otherwise.  The DEM is not modified.
 * PriorityFlood_Original<topology> (:136-198) returns the surface of FillDepressions<topology>: rdgpu_fill_<T>.
 *
 * PriorityFlood_Wei2018(Array2D<T>&) (depressions/Wei2018.hpp:154-202): the D8 fill whose seeds are the raster's edge
 * cells AND every data cell next to a NoData cell (InitPriorityQue, :14-50): NoData cells are never altered and NoData
 * regions inside the raster are outlets.  Equal to rdgpu_fill_<T> on rasters without NoData (tests/tests.cpp:259-262). */
#define RDGPU_DECL_VARIANTS(SUF, T)                                                                                  \
  int rdgpu_has_depressions_##SUF(const T *dem, int width, int height, int topology, int *out);                      \
  int rdgpu_has_depressions_dev_##SUF(const T *d_dem, int width, int height, int topology, int *out, void *hip_stream); \
  int rdgpu_fill_wei2018_##SUF(T *dem, T nodata, int width, int height);                                             \
  int rdgpu_fill_wei2018_dev_##SUF(T *d_dem, T nodata, int width, int height, void *hip_stream);
RDGPU_DECL_VARIANTS(u8, uint8_t)
RDGPU_DECL_VARIANTS(i8, int8_t)
RDGPU_DECL_VARIANTS(i16, int16_t)
RDGPU_DECL_VARIANTS(u16, uint16_t)
RDGPU_DECL_VARIANTS(i32, int32_t)
RDGPU_DECL_VARIANTS(u32, uint32_t)
RDGPU_DECL_VARIANTS(f32, float)
RDGPU_DECL_VARIANTS(f64, double)
RDGPU_DECL_VARIANTS(i64, int64_t)
RDGPU_DECL_VARIANTS(u64, uint64_t)
#undef RDGPU_DECL_VARIANTS

/* PriorityFlood_Barnes2014_max_dep<topology>(Array2D<T>&, uint64_t max_dep_size) (depressions/Barnes2014.hpp:844-931;
 * apps/rd_depressions_flood.cpp:16-19 with a non-zero third argument): only depressions of at most max_dep_size
 * cells are filled, the others are left as they are.  "Depression" as the reference counts it: the cells below the
 * level L that one cell of elevation L floods in one run of its pit queue.  Identical to the reference on DEMs without
 * equal elevations and on the reference's goldens (tests/depressions/testdem1.{1,2}.out); when several cells of
 * elevation L touch the same pocket the reference's grouping follows std::priority_queue's pop order, this one the
 * lowest cell index.  Where that can happen is DETECTED on the device: pockets sharing any possible flooding cell form a
 * cluster, a cluster holding a pocket with two or more possible flooding cells is tie-flagged, and inside it the order
 * matters only for pockets within the size limit of clusters beyond it; on all other cells
 * the output does not depend on the pop order (rdgpu_fill_max_dep_get_stats; rdgpu_fill_max_dep_ties_dev_<T> also writes
 * the flagged cells as a uint8 mask -- the parity tests assert that every cell differing from the reference lies in it). */
typedef struct rdgpu_max_dep_stats {
  uint64_t pockets;           /* connected components of the cells the plain fill would raise */
  uint64_t tie_pockets;       /* ... that two or more cells of their spill elevation can flood: the heap's order decides */
  uint64_t tie_cluster_cells; /* cells whose fate the heap's order can decide: pockets no larger than the limit, in tie-flagged
                                 clusters larger than the limit (0: the result is the reference's whatever its heap does) */
  uint64_t pocket_cells;      /* cells the plain fill would raise */
} rdgpu_max_dep_stats;
int rdgpu_fill_max_dep_get_stats(rdgpu_max_dep_stats *out);   /* of the calling thread's last max_dep fill; waits for that
                                                                  call's stream (the `_dev_` entries themselves do not block) */
#define RDGPU_DECL_MAXDEP(SUF, T)                                                                       \
  int rdgpu_fill_max_dep_##SUF(T *dem, int width, int height, int topology, uint64_t max_dep_size);     \
  int rdgpu_fill_max_dep_dev_##SUF(T *d_dem, int width, int height, int topology, uint64_t max_dep_size, void *hip_stream); \
  int rdgpu_fill_max_dep_ties_dev_##SUF(T *d_dem, int width, int height, int topology, uint64_t max_dep_size,              \
                                        uint8_t *d_tie_mask, void *hip_stream);
RDGPU_DECL_MAXDEP(u8, uint8_t)
RDGPU_DECL_MAXDEP(i16, int16_t)
RDGPU_DECL_MAXDEP(u16, uint16_t)
RDGPU_DECL_MAXDEP(i32, int32_t)
RDGPU_DECL_MAXDEP(u32, uint32_t)
RDGPU_DECL_MAXDEP(f32, float)
RDGPU_DECL_MAXDEP(i8, int8_t)
RDGPU_DECL_MAXDEP(f64, double)    /* the 64-bit element types run on dense value ranks (csrc/fill64.hip), as the fill does */
RDGPU_DECL_MAXDEP(i64, int64_t)
RDGPU_DECL_MAXDEP(u64, uint64_t)
#undef RDGPU_DECL_MAXDEP

/* pit_mask<topology>(const Array2D<T>&, Array2D<uint8_t>&) (depressions/Barnes2014.hpp:593-676,
 * apps/rd_depressions_mask.cpp:16): 1 = the cell lies in a depression (the fill would raise it), 0 = not,
 * 3 = NoData.  The DEM is not modified. */
#define RDGPU_DECL_PITMASK(SUF, T)                                                                        \
  int rdgpu_pit_mask_##SUF(const T *dem, T nodata, int width, int height, int topology, uint8_t *mask);   \
  int rdgpu_pit_mask_dev_##SUF(const T *d_dem, T nodata, int width, int height, int topology, uint8_t *d_mask, void *hip_stream);
RDGPU_DECL_PITMASK(u8, uint8_t)
RDGPU_DECL_PITMASK(i16, int16_t)
RDGPU_DECL_PITMASK(u16, uint16_t)
RDGPU_DECL_PITMASK(i32, int32_t)
RDGPU_DECL_PITMASK(u32, uint32_t)
RDGPU_DECL_PITMASK(f32, float)
RDGPU_DECL_PITMASK(i8, int8_t)
RDGPU_DECL_PITMASK(f64, double)
RDGPU_DECL_PITMASK(i64, int64_t)
RDGPU_DECL_PITMASK(u64, uint64_t)
#undef RDGPU_DECL_PITMASK

/* ---- PriorityFloodEpsilon_Barnes2014<topology>(Array2D<T>&) ------------------------------------------------------
 * Replaces richdem::PriorityFloodEpsilon_Barnes2014 (include/richdem/depressions/Barnes2014.hpp:335-420) =
 * FillDepressionsEpsilon (depressions/depressions.hpp:23); Python rd.FillDepressions(epsilon=True) ->
 * rdPFepsilonD8 / rdPFepsilonD4 (wrappers/pyrichdem/src/pywrapper.hpp:34-35).  In place; every depression and flat
 * gets a gradient of one representable step (std::nextafter) per cell towards its outlet.  Floating-point DEMs only:
 * the reference throws "Priority-Flood+Epsilon is only available for floating-point data types!" for the integer
 * types (:424-451) and so does the C++ shim.  NoData cells are never altered and act as outlets of value NoData
 * (what the reference does with NoData regions that touch the raster border, given its precondition that NoData is
 * lower than every data value).
 * The result is the unique surface E = z on the border / NoData, E(c) = max(z(c), nextafter(min over neighbours
 * E(n))) elsewhere; it equals the reference's output on every DEM in which no two cells of the reference's heap tie
 * (with ties the reference's output depends on std::priority_queue's pop order; this surface is then <= it). */
int rdgpu_fill_epsilon_f32(float *dem, float nodata, int width, int height, int topology);
int rdgpu_fill_epsilon_f64(double *dem, double nodata, int width, int height, int topology);
int rdgpu_fill_epsilon_dev_f32(float *d_dem, float nodata, int width, int height, int topology, void *hip_stream);
int rdgpu_fill_epsilon_dev_f64(double *d_dem, double nodata, int width, int height, int topology, void *hip_stream);
typedef struct rdgpu_epsilon_stats {
  uint32_t rounds;           /* tile-relaxation rounds, all attempts                                            */
  uint32_t attempts;         /* 1 unless the assumed slack was too small for the DEM (RDGPU_EPS_SLACK=<steps>)  */
  uint64_t tile_relaxations; /* tiles relaxed, summed over the rounds                                           */
  uint64_t slack;            /* the slack the successful attempt ran with, in representable steps               */
  uint64_t max_lift;         /* largest lift of a cell above the plain fill, in representable steps             */
  uint64_t tie_sources;      /* gradient sources (cells at their own elevation next to a raised cell) whose elevation
                                another source shares: 0 = identical to the reference; otherwise the reference's result
                                follows std::priority_queue's pop order there and this surface is a cell-wise lower
                                bound of it (RDGPU_EPS_TIES=0 skips the count)                                      */
} rdgpu_epsilon_stats;
int rdgpu_fill_epsilon_get_stats(rdgpu_epsilon_stats *out);

/* ---- PriorityFloodWatersheds_Barnes2014<topology>(Array2D<T>&, Array2D<int32_t>& labels, bool alter_elevations) ----
 * Replaces richdem::PriorityFloodWatersheds_Barnes2014 (include/richdem/depressions/Barnes2014.hpp:713-807): labels[i] =
 * the watershed the cell drains to (every data cell of the raster border, and every data cell next to a NoData region
 * connected to it, starts a watershed; labels are numbered from 1 in the order the reference pops their first cell,
 * i.e. by elevation; cells that are never labelled -- NoData connected to the border -- hold -1 = labels.noData()).
 * alter != 0: the DEM is filled as by PriorityFlood_Barnes2014 (:793-794).  Identical to the reference, numbering
 * included, on DEMs without equal elevations among the cells of its heap; with ties the reference's partition follows
 * std::priority_queue's pop order. */
/* PriorityFloodFlowdirs_Barnes2014(elevations, flowdirs) -- depressions/Barnes2014.hpp:483-555: D8 directions of the flood
 * that does not raise the DEM; every cell points at the neighbour that was flooded first (border cells off the raster, NoData
 * cells 0).  Identical to the reference, equal elevations included: the reference's queue breaks ties by insertion order
 * (GridCellZk_low_pq, common/grid_cell.hpp:101-122) and that order is reproduced as a fixed point -- an exact
 * flood of the raster's unique ranks, then passes over (tree of directions, ranks) until both reproduce themselves, a second
 * flood once the ranks rest (3 - 4 passes on float terrain, the breadth-first depth of the largest plateau on integer DEMs;
 * RDGPU_PFD_TREE_ITER=0: a flood in every pass).  The passes are BOUNDED by a count, RDGPU_PFD_TIE_PASSES (default 1000:
 * deterministic -- the same DEM gives the same raster on every machine); a wall-time bound is opt-in
 * (RDGPU_PFD_TIE_SECONDS=<seconds>, checked between passes: a result stopped by the clock is NOT reproducible across
 * machines or host loads).  When a bound stops the passes the call still returns RDGPU_OK, the result is an exact flood of a
 * stable order and stats.unresolved != 0 says how many ranks were still moving (the C++ shim logs one line to stderr, the
 * Python layer raises a RuntimeWarning): callers that need the reference's tie order must read the stats.  RDGPU_PFD_RANKS=0 is the FAST path for callers who do not need the
 * reference's tie order: one flood, ties decided by neighbour number (seconds instead of tens of seconds at 40000^2);
 * stats.unresolved then counts the cells where a tie decided.  One fill per nesting level of the depressions per flood. */
typedef struct rdgpu_pf_flowdirs_stats {
  uint32_t levels;      /* fills run */
  uint32_t twins;       /* cells whose elevation occurs more than once in the raster: 0 => the result is the reference's */
  uint64_t unresolved;  /* twins != 0: cells whose place in the tie order was still moving when the passes ran out (0: the
                           result is the reference's; = twins when no re-rank pass ran at all, RDGPU_PFD_TIE_PASSES=0);
                           RDGPU_PFD_RANKS=0: directions decided by neighbour number */
  uint32_t tie_passes;  /* passes of the tie order's fixed point (rank computations; not every pass floods) */
  uint32_t reserved;
} rdgpu_pf_flowdirs_stats;
int rdgpu_pf_flowdirs_get_stats(rdgpu_pf_flowdirs_stats *out);
#define RDGPU_DECL_PFD(SUF, T)                                                                              \
  int rdgpu_pf_flowdirs_##SUF(const T *dem, T nodata, int width, int height, uint8_t *dirs);                \
  int rdgpu_pf_flowdirs_dev_##SUF(const T *d_dem, T nodata, int width, int height, uint8_t *d_dirs, void *hip_stream); \
  /* building block: the D8 fill with interior outlets (cells flagged in d_outlet drain like border cells) */ \
  int rdgpu_fill_outlets_dev_##SUF(T *d_dem, const uint8_t *d_outlet, int width, int height, void *hip_stream); \
  /* ... d_skip (per 64 x 64 tile, optional): 1 / 2 = nothing but outlets in the tile and around it (1: first time) */ \
  int rdgpu_fill_outlets_skip_dev_##SUF(T *d_dem, const uint8_t *d_outlet, const uint8_t *d_skip, int width, int height, \
                                        void *hip_stream);                                                    \
  /* ... d_lists: [tiles in state 0 or 1 | their 64 x 32 pair-pass tiles (state 0) | tiles in state 0], `stride` entries each, \
     counts3 (host): their lengths -- the raster kernels are launched over the lists only */                  \
  int rdgpu_fill_outlets_lists_dev_##SUF(T *d_dem, const uint8_t *d_outlet, const uint8_t *d_skip, const uint32_t *d_lists, \
                                         uint32_t stride, const uint32_t *counts3, int width, int height, void *hip_stream);
RDGPU_DECL_PFD(u8, uint8_t)
RDGPU_DECL_PFD(i8, int8_t)
RDGPU_DECL_PFD(i16, int16_t)
RDGPU_DECL_PFD(u16, uint16_t)
RDGPU_DECL_PFD(i32, int32_t)
RDGPU_DECL_PFD(u32, uint32_t)
RDGPU_DECL_PFD(f32, float)
#undef RDGPU_DECL_PFD
/* f64 / i64 / u64: on the dense value ranks of the DEM (fill64.hip), no restriction on the values */
#define RDGPU_DECL_PFD64(SUF, T)                                                                            \
  int rdgpu_pf_flowdirs_##SUF(const T *dem, T nodata, int width, int height, uint8_t *dirs);                \
  int rdgpu_pf_flowdirs_dev_##SUF(const T *d_dem, T nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
RDGPU_DECL_PFD64(f64, double)
RDGPU_DECL_PFD64(i64, int64_t)
RDGPU_DECL_PFD64(u64, uint64_t)
#undef RDGPU_DECL_PFD64

#define RDGPU_DECL_WS(SUF, T)                                                                                          \
  int rdgpu_watersheds_##SUF(T *dem, T nodata, int width, int height, int topology, int alter, int32_t *labels);      \
  int rdgpu_watersheds_dev_##SUF(T *d_dem, T nodata, int width, int height, int topology, int alter, int32_t *d_labels, void *hip_stream);
RDGPU_DECL_WS(u8, uint8_t)
RDGPU_DECL_WS(i16, int16_t)
RDGPU_DECL_WS(u16, uint16_t)
RDGPU_DECL_WS(i32, int32_t)
RDGPU_DECL_WS(u32, uint32_t)
RDGPU_DECL_WS(f32, float)
RDGPU_DECL_WS(i8, int8_t)
RDGPU_DECL_WS(f64, double)
RDGPU_DECL_WS(i64, int64_t)
RDGPU_DECL_WS(u64, uint64_t)
#undef RDGPU_DECL_WS

/* Environment switches of the fill (read at every call; for tests and A/B timing, results never change):
 *   RDGPU_FILL_EDGES=0         every contraction round is a raster pass (the r01d engine; default: one raster pass,
 *                              then rounds on the component-pair list it records)
 *   RDGPU_FILL_EDGE_CAP=<n>    capacity of that list in records (default min(12 per basin, cells/2)); a list
 *                              that does not fit falls back to raster passes
 *   RDGPU_FILL_ROUND_BATCH=<n> contraction rounds enqueued per stream synchronisation (default: all of them at once --
 *                              a fill synchronises twice, rdgpu_fill_stats::host_syncs)
 *   RDGPU_FILL_TAIL_ROOTS=<n>  a round entered by at most n live roots and 8 n pair records, and every round after it,
 *                              runs in the single-workgroup tail kernel (default 1024); 0: never, every round is
 *                              full-width launches; a huge value: from round 2 on
 *   RDGPU_FILL_DISSOLVE=0      every pit of the descent forest is a basin (default: a pit whose lowest neighbour lies in its
 *                              64 x 64 tile and drains elsewhere joins that neighbour's tree and is raised on its own;
 *                              rdgpu_fill_stats::dissolved_pits)
 *   RDGPU_FILL_FLOODED=0       the finalize reads every tile (default: a 64 x 64 tile whose node levels are one level
 *                              strictly above the tile's largest key -- a tile wholly under one lake -- is written at
 *                              that level without its elevations or labels being read)
 *   RDGPU_FILL_COUNT_FLOODED=1 the finalize counts the tiles it writes that way, one atomic add each, for
 *                              rdgpu_fill_flooded_tiles (default: no counter, no atomics)
 *   RDGPU_FILL_COARSE=0        no coarse flood; =1: at any raster size (default: from 262 144 descent tiles, 32 768^2 cells).
 *                              The descent leaves the minima of the 16 x 16 blocks, their fill (a nested fill: two more
 *                              stream synchronisations, host_syncs 4) is a lower bound of the filled surface, and a 64 x 64
 *                              tile whose blocks all lie above the tile's largest cell is left out of the pair pass: a
 *                              star and a ring of pair records stand in for it.  Needs RDGPU_FILL_FLOODED != 0.
 *   RDGPU_FILL_COARSE_LANE=0   the nested fill runs on the caller's stream, behind the node resolve (default: on a second
 *                              stream of the library's, beside it; the caller's stream waits for that stream before the
 *                              pair pass, so the call is ordered on the caller's stream as ever.  Same output either way)
 *   RDGPU_FILL_COUNT_COARSE=1  counts the tiles left out, for rdgpu_fill_coarse_tiles (default: no counter) */
/* Statistics of the last fill on this process (for DESIGN.md / bench.py reporting). */
typedef struct rdgpu_fill_stats {
  uint64_t cells;       /* width*height                                   */
  uint64_t basins;      /* descent-forest roots (pits) not draining out   */
  uint32_t rounds;      /* Boruvka contraction rounds                     */
  uint32_t jump_passes; /* pointer-jumping passes over the descent forest */
  uint64_t scan_tiles;  /* tiles visited by fill.scan, summed over the rounds */
  uint32_t tile_cells;  /* cells per scan tile                               */
  uint32_t edge_records; /* component-pair records the first raster pass handed to rounds 2.. (0: raster rounds) */
  uint32_t host_syncs;   /* stream synchronisations inside the fill (r06: 2 -- after the descent, after the rounds) */
  uint32_t dissolved_pits; /* of `basins`: pits the descent dissolved -- single cells whose lowest neighbour drains elsewhere;
                              they get no row in the basin tables and no pair records (0 with RDGPU_FILL_DISSOLVE=0, in the
                              shards, the fills with outlets and the classic path); this word was `reserved` */
} rdgpu_fill_stats;
int rdgpu_fill_get_stats(rdgpu_fill_stats *out);
/* Tiles the last plain fill of the calling thread wrote without reading them.  Counted only under
 * RDGPU_FILL_COUNT_FLOODED=1 (else 0, as after a fill with outlets, a shard or RDGPU_FILL_FLOODED=0).  The fill itself
 * does not wait for the count: this call synchronises with the fill's stream. */
int rdgpu_fill_flooded_tiles(uint64_t *out);
/* Tiles the coarse flood of the last plain fill of the calling thread left out of the pair pass.  Counted only under
 * RDGPU_FILL_COUNT_COARSE=1 (else 0, as when no coarse flood ran).  Synchronises with the fill's stream. */
int rdgpu_fill_coarse_tiles(uint64_t *out);
/* Edge of the coarse flood's blocks, in cells (16). */
int rdgpu_fill_coarse_block(void);

/* ---- row-block shards: the tile protocol of programs/parallel_priority_flood over GPUs ---------
 * Mirrors the reference's tiled Priority-Flood (Barnes 2016; programs/parallel_priority_flood/main.cpp:
 * Consumer FirstRound :276-313 / SecondRound :315-330, Producer Calculations :401-547; Zhou2016pf.hpp).
 * The DEM is cut into row blocks; one block per GPU (or one after the other on one GPU).
 *   1. rdgpu_fill_shard_begin_<T>   local phase on the block resident in HBM: fills it against its own
 *                                   perimeter, labels every cell with the cut-row cell ("terminal") or
 *                                   the outside its watershed drains to, and reduces the lowest pass
 *                                   between every pair of adjacent watersheds (the spillover graph).
 *                                   open_top / open_bottom: the first / last row is a cut, not DEM border.
 *   2. rdgpu_fill_shard_export      what the reference's Job1 carries (main.cpp:147-173): the cut rows'
 *                                   elevations (as order-preserving uint32 keys) and the graph edges
 *                                   (a, b, pass) with a/b = terminal ids (top row: x, bottom row:
 *                                   width + x) or 0xFFFFFFFF for the outside.  Host buffers.
 *   3. exchange                     every rank all-gathers (2*width keys + edges) -- RCCL over xGMI in
 *                                   richdem_amd/sharded.py; nothing else crosses GPUs.
 *   4. rdgpu_fill_graph_solve       host: joins the shard graphs along the cuts and floods the label
 *                                   graph from the outside (= the producer's aggregated Priority-Flood).
 *                                   keys/levels: [nshards][2][width]; edges: concatenated triples,
 *                                   edge_offsets[nshards+1] in triples.  Deterministic, so every rank
 *                                   solves redundantly instead of broadcasting (Job2, main.cpp:549-554).
 *   5. rdgpu_fill_shard_finish      raises the block (levels = this shard's [2][width] slice), writes
 *                                   the filled elevations in place and releases the handle.
 * rdgpu_fill_sharded_<T> runs 1-5 shard after shard on one GPU (tiling-invariance tests; DEMs cut
 * this way give bit-identical results to rdgpu_fill_<T>). */
typedef struct rdgpu_fill_shard rdgpu_fill_shard;
int rdgpu_fill_shard_begin_u8(uint8_t *d_rows, int width, int rows, int topology, int open_top, int open_bottom, void *hip_stream, rdgpu_fill_shard **out);
int rdgpu_fill_shard_begin_i16(int16_t *d_rows, int width, int rows, int topology, int open_top, int open_bottom, void *hip_stream, rdgpu_fill_shard **out);
int rdgpu_fill_shard_begin_u16(uint16_t *d_rows, int width, int rows, int topology, int open_top, int open_bottom, void *hip_stream, rdgpu_fill_shard **out);
int rdgpu_fill_shard_begin_i32(int32_t *d_rows, int width, int rows, int topology, int open_top, int open_bottom, void *hip_stream, rdgpu_fill_shard **out);
int rdgpu_fill_shard_begin_u32(uint32_t *d_rows, int width, int rows, int topology, int open_top, int open_bottom, void *hip_stream, rdgpu_fill_shard **out);
int rdgpu_fill_shard_begin_f32(float *d_rows, int width, int rows, int topology, int open_top, int open_bottom, void *hip_stream, rdgpu_fill_shard **out);
int rdgpu_fill_shard_begin_i8(int8_t *d_rows, int width, int rows, int topology, int open_top, int open_bottom, void *hip_stream, rdgpu_fill_shard **out);
int rdgpu_fill_shard_edge_count(rdgpu_fill_shard *shard, uint32_t *n_edges);
int rdgpu_fill_shard_export(rdgpu_fill_shard *shard, uint32_t *top_keys, uint32_t *bottom_keys, uint32_t *edges);
int rdgpu_fill_shard_finish(rdgpu_fill_shard *shard, const uint32_t *levels);
int rdgpu_fill_shard_free(rdgpu_fill_shard *shard);
int rdgpu_fill_graph_solve(int nshards, int width, int topology, const uint32_t *keys, const uint32_t *edges,
                           const uint64_t *edge_offsets, uint32_t *levels);
/* Device-resident variants of steps 2, 4 and 5 (nothing but the all-gather leaves HBM):
 *   export_dev : d_keys[2*width] <- cut-row keys, d_edges[3*cap] <- edge triples (count from edge_count)
 *   graph_solve_dev : d_keys_all [nshards][2][width], d_edges_all [nshards][cap][3] with d_counts[nshards]
 *                     valid triples per shard -> d_levels_all [nshards][2][width]; the label graph is
 *                     contracted on the GPU with the fill's own Boruvka kernels
 *   finish_dev : levels = this shard's [2][width] slice, on the device */
int rdgpu_fill_shard_export_dev(rdgpu_fill_shard *shard, uint32_t *d_keys, uint32_t *d_edges, uint32_t cap);
int rdgpu_fill_graph_solve_dev(int nshards, int width, int topology, const uint32_t *d_keys_all,
                               const uint32_t *d_edges_all, const uint32_t *d_counts, uint32_t cap,
                               uint32_t *d_levels_all, void *hip_stream);
int rdgpu_fill_shard_finish_dev(rdgpu_fill_shard *shard, const uint32_t *d_levels);
/* One process, several devices (the reference's tiled driver, programs/parallel_priority_flood/main.cpp:276-330,
 * :401-547, as a library call): row block s of the host raster goes to devices[s] over that device's own PCIe link,
 * is filled locally there (one host thread per device: the devices work side by side), the cut rows and spillover
 * graphs are joined and solved on devices[0] (RDGPU_MULTI_HOST_SOLVE=1: on the host), every device raises its block and
 * returns it.  Same result as rdgpu_fill_<T>, bit for bit.  A device id may be listed more than once (its blocks are
 * then handled in order).  EXPERIMENTAL in one respect: this build's test boxes have one GPU, so the entry is verified
 * with one physical device listed several times -- threads, staging, the joined solve -- not on several devices.
 * rdgpu_fill_<T> itself takes this path when the environment holds RDGPU_DEVICES=<id>,<id>,... with two or more ids,
 * so rdgpu::FillDepressions(Array2D&) and apps/rd_depressions_flood use several GPUs without a change of signature. */
int rdgpu_fill_multi_u8(uint8_t *dem, int width, int height, int topology, const int *devices, int ndevices);
int rdgpu_fill_multi_i16(int16_t *dem, int width, int height, int topology, const int *devices, int ndevices);
int rdgpu_fill_multi_u16(uint16_t *dem, int width, int height, int topology, const int *devices, int ndevices);
int rdgpu_fill_multi_i32(int32_t *dem, int width, int height, int topology, const int *devices, int ndevices);
int rdgpu_fill_multi_u32(uint32_t *dem, int width, int height, int topology, const int *devices, int ndevices);
int rdgpu_fill_multi_f32(float *dem, int width, int height, int topology, const int *devices, int ndevices);
int rdgpu_fill_multi_i8(int8_t *dem, int width, int height, int topology, const int *devices, int ndevices);
int rdgpu_fill_sharded_u8(uint8_t *dem, int width, int height, int topology, int nshards);
int rdgpu_fill_sharded_i16(int16_t *dem, int width, int height, int topology, int nshards);
int rdgpu_fill_sharded_u16(uint16_t *dem, int width, int height, int topology, int nshards);
int rdgpu_fill_sharded_i32(int32_t *dem, int width, int height, int topology, int nshards);
int rdgpu_fill_sharded_u32(uint32_t *dem, int width, int height, int topology, int nshards);
int rdgpu_fill_sharded_f32(float *dem, int width, int height, int topology, int nshards);
int rdgpu_fill_sharded_i8(int8_t *dem, int width, int height, int topology, int nshards);

/* ---- d8_flow_directions(const Array2D<T>&, Array2D<uint8_t>&) ------------------------------
 * Replaces richdem::d8_flow_directions / d8_FlowDir (include/richdem/flowmet/d8_flowdirs.hpp:96-123,
 * :32-74).  dirs[i] in {0 = NO_FLOW, 1..8 = neighbour in the 234/105/876 numbering, 255 =
 * FLOWDIR_NO_DATA} (common/constants.hpp:76-80).  The shim sets flowdirs.setNoData(255). */
int rdgpu_d8_flowdirs_u8(const uint8_t *dem, uint8_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_i16(const int16_t *dem, int16_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_u16(const uint16_t *dem, uint16_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_i32(const int32_t *dem, int32_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_u32(const uint32_t *dem, uint32_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_f32(const float *dem, float nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_f64(const double *dem, double nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_i8(const int8_t *dem, int8_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_i64(const int64_t *dem, int64_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_u64(const uint64_t *dem, uint64_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_d8_flowdirs_dev_u8(const uint8_t *d_dem, uint8_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_i16(const int16_t *d_dem, int16_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_u16(const uint16_t *d_dem, uint16_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_i32(const int32_t *d_dem, int32_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_u32(const uint32_t *d_dem, uint32_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_f32(const float *d_dem, float nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_f64(const double *d_dem, double nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_i8(const int8_t *d_dem, int8_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_i64(const int64_t *d_dem, int64_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_d8_flowdirs_dev_u64(const uint64_t *d_dem, uint64_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);

/* ---- barnes_flat_resolution_d8(Array2D<T>& elevations, Array2D<uint8_t>& flowdirs, alter=false) --
 * Replaces richdem::barnes_flat_resolution_d8 (include/richdem/flats/flat_resolution.hpp:587-605) with
 * alter == false: d8_flow_directions, then resolve_flats_barnes (:447-517), then d8_flow_flats
 * (:96-116).  dirs is written in full; NO_FLOW cells of flats without an outlet stay 0.
 * rdgpu_resolve_flats_* additionally returns the flat_mask of resolve_flats_barnes (identical to the
 * reference's values) and the flat partition (labels[i] = 1 + lowest cell index of the cell's flat,
 * 0 for cells outside drainable flats; the reference numbers flats in scan order instead -- only
 * the partition is defined by the algorithm).  mask / labels may be NULL. */
int rdgpu_flat_resolution_d8_u8(const uint8_t *dem, uint8_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_i16(const int16_t *dem, int16_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_u16(const uint16_t *dem, uint16_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_i32(const int32_t *dem, int32_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_u32(const uint32_t *dem, uint32_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_f32(const float *dem, float nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_f64(const double *dem, double nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_i8(const int8_t *dem, int8_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_i64(const int64_t *dem, int64_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_u64(const uint64_t *dem, uint64_t nodata, int width, int height, uint8_t *dirs);
int rdgpu_flat_resolution_d8_dev_u8(const uint8_t *d_dem, uint8_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_i16(const int16_t *d_dem, int16_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_u16(const uint16_t *d_dem, uint16_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_i32(const int32_t *d_dem, int32_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_u32(const uint32_t *d_dem, uint32_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_f32(const float *d_dem, float nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_f64(const double *d_dem, double nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_i8(const int8_t *d_dem, int8_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_i64(const int64_t *d_dem, int64_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_flat_resolution_d8_dev_u64(const uint64_t *d_dem, uint64_t nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
int rdgpu_resolve_flats_u8(const uint8_t *dem, uint8_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_i16(const int16_t *dem, int16_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_u16(const uint16_t *dem, uint16_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_i32(const int32_t *dem, int32_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_u32(const uint32_t *dem, uint32_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_f32(const float *dem, float nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_f64(const double *dem, double nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_i8(const int8_t *dem, int8_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_i64(const int64_t *dem, int64_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);
int rdgpu_resolve_flats_u64(const uint64_t *dem, uint64_t nodata, int width, int height, uint8_t *dirs, int32_t *mask, int32_t *labels);

/* alter == true (flat_resolution.hpp:597-600 + d8_flats_alter_dem :545-582): the DEM is raised in place by
 * flat_mask increments of nextafterf inside drainable flats, then plain D8 directions are taken on it (the reference
 * applies nextafterf, i.e. float steps, to every element type). */
#define RDGPU_DECL_ALTER(SUF, T)                                                                                       \
  int rdgpu_flat_resolution_d8_alter_##SUF(T *dem, T nodata, int width, int height, uint8_t *dirs);                     \
  int rdgpu_flat_resolution_d8_alter_dev_##SUF(T *d_dem, T nodata, int width, int height, uint8_t *d_dirs, void *hip_stream);
RDGPU_DECL_ALTER(f32, float)
RDGPU_DECL_ALTER(f64, double)
/* integer element types: the reference's step is (T)nextafterf((float)e, numeric_limits<T>::infinity() == 0) -- one
 * towards zero per increment (one float spacing for magnitudes of 2^24 and more) -- reproduced as is */
RDGPU_DECL_ALTER(u8, uint8_t)
RDGPU_DECL_ALTER(i8, int8_t)
RDGPU_DECL_ALTER(i16, int16_t)
RDGPU_DECL_ALTER(u16, uint16_t)
RDGPU_DECL_ALTER(i32, int32_t)
RDGPU_DECL_ALTER(u32, uint32_t)
RDGPU_DECL_ALTER(i64, int64_t)
RDGPU_DECL_ALTER(u64, uint64_t)
#undef RDGPU_DECL_ALTER

/* Environment switches of the directions-only flat resolution (read at every call; A/B timing and tests, results never change;
 * the stencil relaxation engine, the last pass over the DEM, the classification's own bitmaps and their switches are gone: their
 * record is in docs/HISTORY.md and profiles/):
 *   RDGPU_FLAT_PLANES=0         the two level fields as one int per cell instead of 16 bit planes per 64 x 64 tile (the plane
 *                               engine also steps aside by itself when a level may not fit 16 bits: a flat more than
 *                               65 279 levels deep, e.g. open water that far across; flat_mask / labels, alter = true,
 *                               ResolveFlatsEpsilon and the row-block shards always use ints)
 *   RDGPU_FLAT_STATIC=0         the towards search in batches of rounds decided on the host instead of one enqueue
 *   RDGPU_FLAT_ASYNC=<n>        a search's rounds hand over to resident wavefronts once a round visits fewer than n tiles
 *                               (default 20000; 0: rounds to the end), RDGPU_FLAT_ASYNC_BLOCKS / _STATS tune and report them,
 *                               RDGPU_FLAT_ASYNC_FAIL=1 declares a tail failed (tests: the recovery in rounds)
 *   RDGPU_FLAT_PLANES_MAX=<n>   lowers the level from which the plane engine steps aside (tests)
 *   RDGPU_FLAT_TRACE=1          per-round counts and visit statistics on stderr (ints, no side stream)
 *   RDGPU_FLAT_AWAY_BESIDE=0    the away search after the towards search instead of beside its tail
 * ResolveFlatsEpsilon: RDGPU_RFE_OVERLAP=0 (the labels on the caller's stream instead of beside the towards search's tail) */
typedef struct rdgpu_flat_stats {
  uint64_t low_edges;      /* find_flat_edges: cells with flow next to an equal NO_FLOW cell */
  uint64_t high_edges;     /* NO_FLOW cells next to higher terrain                           */
  uint64_t noflow_cells;   /* cells without a local gradient                                 */
  uint32_t away_levels;    /* tile-relaxation rounds, away-from-higher gradient              */
  uint32_t towards_levels; /* tile-relaxation rounds, towards-lower gradient                 */
} rdgpu_flat_stats;
int rdgpu_flat_get_stats(rdgpu_flat_stats *out);
/* The asynchronous tails of the two level searches of the last flat resolution on this thread (csrc/flats.hip,
 * k_relax_bits_async; no reference counterpart -- the reference's searches are serial queues, flats/flat_resolution.hpp:152-298):
 * tile visits by the resident wavefronts, tiles that were live when the rounds handed over (summed over the launches),
 * launches, launches that gave up and were finished in rounds.  plane_repeats: 1 when this thread's last directions-only call
 * found a level beyond the planes' range and was repeated on the int engine, else 0. */
typedef struct rdgpu_flat_async_stats {
  uint64_t visits;
  uint32_t launches;
  uint32_t failures;
  uint32_t live_tiles;
  uint32_t plane_repeats;
} rdgpu_flat_async_stats;
int rdgpu_flat_get_async_stats(rdgpu_flat_async_stats *out);

/* ResolveFlatsEpsilon(Array2D<T>&) (flats/flats.hpp:21-28; rd.ResolveFlats): the DEM is altered in place so
 * that every flat with an outlet drains -- each interior cell of such a flat is raised by flat_mask increments
 * of std::nextafter(e, numeric_limits<T>::infinity()) in its own type (float / double: towards +inf; integer
 * types: numeric_limits<int>::infinity() is 0, so the reference moves the value towards zero -- kept). */
#define RDGPU_DECL_RFE(SUF, T)                                                    \
  int rdgpu_resolve_flats_epsilon_##SUF(T *dem, T nodata, int width, int height); \
  int rdgpu_resolve_flats_epsilon_dev_##SUF(T *d_dem, T nodata, int width, int height, void *hip_stream);
RDGPU_DECL_RFE(u8, uint8_t)
RDGPU_DECL_RFE(i16, int16_t)
RDGPU_DECL_RFE(u16, uint16_t)
RDGPU_DECL_RFE(i32, int32_t)
RDGPU_DECL_RFE(u32, uint32_t)
RDGPU_DECL_RFE(f32, float)
RDGPU_DECL_RFE(f64, double)
RDGPU_DECL_RFE(i8, int8_t)
RDGPU_DECL_RFE(i64, int64_t)
RDGPU_DECL_RFE(u64, uint64_t)
#undef RDGPU_DECL_RFE

/* ---- flat resolution over row-block shards ---------------------------
 * barnes_flat_resolution_d8 (flats/flat_resolution.hpp:587-605) when the raster is split into row blocks,
 * one per GPU.  d_rows = the shard's own rows plus TWO ghost rows per cut (ghost_top / ghost_bottom are 0
 * at the raster's first / last block, 2 otherwise), device resident and kept alive until _free.
 * Protocol, for phase 0 (towards low edges) and then phase 1 (away from high edges):
 *     repeat { _relax(phase); _boundary(phase, out[2w]);  all-gather;  stop when no gathered row changed;
 *              _inject(phase, last own row of the block above, first own row of the block below) }
 * then  _heights(out[8w]);  all-gather;  rdgpu_flat_graph_solve_dev(gathered, world, w, solved[world*4w]);
 *       _finish(solved + rank*4w, dirs of the own rows).
 * The result equals rdgpu_flat_resolution_d8 of the whole raster restricted to the own rows.           */
typedef struct rdgpu_flat_shard rdgpu_flat_shard;
int rdgpu_flat_shard_begin_u8(const uint8_t *d_rows, uint8_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_i16(const int16_t *d_rows, int16_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_u16(const uint16_t *d_rows, uint16_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_i32(const int32_t *d_rows, int32_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_u32(const uint32_t *d_rows, uint32_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_f32(const float *d_rows, float nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_f64(const double *d_rows, double nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_i8(const int8_t *d_rows, int8_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_i64(const int64_t *d_rows, int64_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_begin_u64(const uint64_t *d_rows, uint64_t nodata, int width, int rows, int ghost_top, int ghost_bottom, void *hip_stream, rdgpu_flat_shard **out);
int rdgpu_flat_shard_relax(rdgpu_flat_shard *shard, int phase);
int rdgpu_flat_shard_boundary(rdgpu_flat_shard *shard, int phase, int32_t *d_out_2w);
int rdgpu_flat_shard_inject(rdgpu_flat_shard *shard, int phase, const int32_t *d_row_above, const int32_t *d_row_below);
int rdgpu_flat_shard_heights(rdgpu_flat_shard *shard, int32_t *d_out_8w);
int rdgpu_flat_graph_solve_dev(const int32_t *d_gathered, int world, int width, int32_t *d_out, void *hip_stream);
int rdgpu_flat_shard_finish(rdgpu_flat_shard *shard, const int32_t *d_heights_4w, uint8_t *d_dirs_out);
int rdgpu_flat_shard_rounds(const rdgpu_flat_shard *shard, int phase);
void rdgpu_flat_shard_free(rdgpu_flat_shard *shard);

/* barnes_flat_resolution_d8(alter = false) of ONE raster over SEVERAL devices of this process: row block s (+ two ghost
 * rows per cut) on devices[s], a host thread per device, the cut rows of the two level fields exchanged from device to
 * device (peer copies; RDGPU_MULTI_HOST_STAGED=1: through the host) until none changes, the flat heights agreed on devices[0]; the result equals rdgpu_flat_resolution_d8_<T> on the whole
 * raster.  A device may be listed more than once.  rdgpu_flat_resolution_d8_<T> takes this path when RDGPU_DEVICES
 * lists two or more ids.  (Verified on one physical device listed several times.) */
#define RDGPU_DECL_FLATS_MULTI(SUF, T) \
  int rdgpu_flat_resolution_d8_multi_##SUF(const T *dem, T nodata, int width, int height, uint8_t *dirs, const int *devices, int ndevices);
RDGPU_DECL_FLATS_MULTI(u8, uint8_t)
RDGPU_DECL_FLATS_MULTI(i8, int8_t)
RDGPU_DECL_FLATS_MULTI(i16, int16_t)
RDGPU_DECL_FLATS_MULTI(u16, uint16_t)
RDGPU_DECL_FLATS_MULTI(i32, int32_t)
RDGPU_DECL_FLATS_MULTI(u32, uint32_t)
RDGPU_DECL_FLATS_MULTI(f32, float)
RDGPU_DECL_FLATS_MULTI(f64, double)
RDGPU_DECL_FLATS_MULTI(i64, int64_t)
RDGPU_DECL_FLATS_MULTI(u64, uint64_t)
#undef RDGPU_DECL_FLATS_MULTI

/* ---- d8_flow_accum(const Array2D<uint8_t>& flowdirs, Array2D<A>& area) ----------------------
 * Replaces richdem::d8_flow_accum (include/richdem/methods/d8_methods.hpp:47-139): area = number of
 * cells draining through each cell (itself included); cells whose direction equals dir_nodata get
 * -1 (area.noData(), :64).  Exact (integer arithmetic) for every output type. */
int rdgpu_d8_flow_accum_i32(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, int32_t *area);
int rdgpu_d8_flow_accum_f32(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, float *area);
int rdgpu_d8_flow_accum_f64(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, double *area);
int rdgpu_d8_flow_accum_dev_i32(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, int32_t *d_area, void *hip_stream);
int rdgpu_d8_flow_accum_dev_f32(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, float *d_area, void *hip_stream);
int rdgpu_d8_flow_accum_dev_f64(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, double *d_area, void *hip_stream);

/* ---- row-block shards of d8_flow_accum: the protocol of programs/parallel_d8_accum over GPUs -------
 * (reference programs/parallel_d8_accum/main.cpp: per-tile accumulation :373-464, paths leaving through the
 * perimeter :270-334, inflow added along the in-tile path :344-370.)  Each rank holds a row block of the
 * uint8 directions plus the adjacent direction row of each neighbouring block (NULL at the DEM edge).
 *   begin    pending-inflow counts (including inflow across the cuts) + all walks that start in the block;
 *            a walk that crosses a cut drops (arrivals << 56 | total) into the outbox slot of the
 *            receiving column
 *   outbox   d_out[2][width] <- {sent up, sent down}; clears the outboxes
 *   inject   the neighbours' outboxes arrive; completed cut-row cells resume walking
 *   (repeat outbox / exchange / inject until every outbox of every rank is empty)
 *   finish   area block in the requested type; releases the handle.
 * Integer arithmetic, exact; the result equals rdgpu_d8_flow_accum_* on the whole raster. */
typedef struct rdgpu_accum_shard rdgpu_accum_shard;
int rdgpu_accum_shard_begin(const uint8_t *d_dirs_rows, uint8_t dir_nodata, int width, int rows,
                            const uint8_t *d_row_above, const uint8_t *d_row_below, void *hip_stream,
                            rdgpu_accum_shard **out);
/* One exchange instead of one per cut crossing (the protocol of programs/parallel_d8_accum/main.cpp:270-464), for
 * directions without loops (every direction raster derived from a DEM):
 *   begin_local  pending counts from the block's own cells only: every cell completes, the outboxes hold what the
 *                block's own cells send across each cut
 *   links        d_links[2][width]: where the flow ENTERING at each cell of the first / last row leaves the block
 *                again -- (1 << 31 if across the lower cut) | receiving column, or -1; *d_pending: cells the local
 *                phase could not complete (a direction loop: fall back to begin / outbox / inject)
 *   (one all-gather of outbox + links; every rank solves the forest over the cut-row cells:
 *    richdem_amd/sharded.py accum_link_solve)
 *   add_paths    the inflow of each entry cell is added along its path inside the block
 *   finish       as above. */
int rdgpu_accum_shard_begin_local(const uint8_t *d_dirs_rows, uint8_t dir_nodata, int width, int rows,
                                  const uint8_t *d_row_above, const uint8_t *d_row_below, void *hip_stream,
                                  rdgpu_accum_shard **out);
int rdgpu_accum_shard_links(rdgpu_accum_shard *shard, int32_t *d_links, unsigned long long *d_pending);
int rdgpu_accum_shard_add_paths(rdgpu_accum_shard *shard, const unsigned long long *d_in_top,
                                const unsigned long long *d_in_bottom);
int rdgpu_accum_shard_outbox(rdgpu_accum_shard *shard, unsigned long long *d_out);
int rdgpu_accum_shard_inject(rdgpu_accum_shard *shard, const unsigned long long *d_from_above,
                             const unsigned long long *d_from_below);
int rdgpu_accum_shard_finish_i32(rdgpu_accum_shard *shard, int32_t *d_area);
int rdgpu_accum_shard_finish_f32(rdgpu_accum_shard *shard, float *d_area);
int rdgpu_accum_shard_finish_f64(rdgpu_accum_shard *shard, double *d_area);
int rdgpu_accum_shard_free(rdgpu_accum_shard *shard);

/* d8_flow_accum of ONE raster over SEVERAL devices of this process (the reference's tiled driver
 * programs/parallel_d8_accum/main.cpp:373-464 as a library call): row block s on devices[s] (a host thread per device,
 * its own PCIe link), one exchange of the cut rows' outboxes and links -- device to device by peer copies, the forest over
 * the cut rows solved on devices[0]; RDGPU_MULTI_HOST_STAGED=1: through the host --, the same result as
 * rdgpu_d8_flow_accum_<A> on the whole raster.  Direction loops fall back to devices[0] alone.  A device may be listed
 * more than once.  rdgpu_d8_flow_accum_<A> takes this path when RDGPU_DEVICES lists two or more ids.
 * (Verified on one physical device listed several times: this build's test boxes have one GPU.) */
int rdgpu_d8_flow_accum_multi_i32(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, int32_t *area, const int *devices, int ndevices);
int rdgpu_d8_flow_accum_multi_f32(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, float *area, const int *devices, int ndevices);
int rdgpu_d8_flow_accum_multi_f64(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, double *area, const int *devices, int ndevices);

/* ---- FA_D8(const Array2D<T>& elevations, Array2D<double>& accum) ----------------------------
 * Replaces richdem::FA_D8 (include/richdem/methods/flow_accumulation.hpp:27) = FM_D8
 * (flowmet/OCallaghan1984.hpp:13-77) + FlowAccumulation (methods/flow_accumulation_generic.hpp:33-100)
 * without materialising the 36 B/cell Array3D.  accum is in/out: on entry the flow each cell
 * generates (1 by default in the reference's callers), on return the accumulation; NoData cells get
 * -1 (ACCUM_NO_DATA).  Exact for integer-valued weights; for general weights the f64 summation order
 * differs from the reference's FIFO order (results agree to f64 rounding, <= 1 ULP after an f32 cast). */
int rdgpu_fa_d8_u8(const uint8_t *dem, uint8_t nodata, int width, int height, double *accum);
int rdgpu_fa_d8_i16(const int16_t *dem, int16_t nodata, int width, int height, double *accum);
int rdgpu_fa_d8_u16(const uint16_t *dem, uint16_t nodata, int width, int height, double *accum);
int rdgpu_fa_d8_i32(const int32_t *dem, int32_t nodata, int width, int height, double *accum);
int rdgpu_fa_d8_u32(const uint32_t *dem, uint32_t nodata, int width, int height, double *accum);
int rdgpu_fa_d8_f32(const float *dem, float nodata, int width, int height, double *accum);
int rdgpu_fa_d8_f64(const double *dem, double nodata, int width, int height, double *accum);
int rdgpu_fa_d8_i8(const int8_t *dem, int8_t nodata, int width, int height, double *accum);
int rdgpu_fa_d8_i64(const int64_t *dem, int64_t nodata, int width, int height, double *accum);
int rdgpu_fa_d8_u64(const uint64_t *dem, uint64_t nodata, int width, int height, double *accum);
/* FM_D8 alone (richdem::FM_D8, flowmet/OCallaghan1984.hpp:81-84) as the 9-float proportions array */
int rdgpu_fm_d8_u8(const uint8_t *dem, uint8_t nodata, int width, int height, float *props9);
int rdgpu_fm_d8_i16(const int16_t *dem, int16_t nodata, int width, int height, float *props9);
int rdgpu_fm_d8_u16(const uint16_t *dem, uint16_t nodata, int width, int height, float *props9);
int rdgpu_fm_d8_i32(const int32_t *dem, int32_t nodata, int width, int height, float *props9);
int rdgpu_fm_d8_u32(const uint32_t *dem, uint32_t nodata, int width, int height, float *props9);
int rdgpu_fm_d8_f32(const float *dem, float nodata, int width, int height, float *props9);
int rdgpu_fm_d8_f64(const double *dem, double nodata, int width, int height, float *props9);
int rdgpu_fm_d8_i8(const int8_t *dem, int8_t nodata, int width, int height, float *props9);
int rdgpu_fm_d8_i64(const int64_t *dem, int64_t nodata, int width, int height, float *props9);
int rdgpu_fm_d8_u64(const uint64_t *dem, uint64_t nodata, int width, int height, float *props9);
int rdgpu_fa_d8_dev_u8(const uint8_t *d_dem, uint8_t nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_i16(const int16_t *d_dem, int16_t nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_u16(const uint16_t *d_dem, uint16_t nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_i32(const int32_t *d_dem, int32_t nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_u32(const uint32_t *d_dem, uint32_t nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_f32(const float *d_dem, float nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_f64(const double *d_dem, double nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_i8(const int8_t *d_dem, int8_t nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_i64(const int64_t *d_dem, int64_t nodata, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_fa_d8_dev_u64(const uint64_t *d_dem, uint64_t nodata, int width, int height, double *d_accum, void *hip_stream);
/* FA_D8 when the CALLER KNOWS that every cell generates a flow of 1 -- it built the accumulation array itself, as
 * apps/rd_flow_accumulation.cpp:13 (Array2D<double> accum(dem, 1)) and rd.FlowAccumulation(weights=None) do: accum is
 * OUTPUT ONLY.  The plain entries above have to read the weights once to find that out (12.8 GB at 40000^2) and, on the
 * host path, upload them (12.8 GB over PCIe); these do neither.  Same result as the plain entry on an array of ones. */
#define RDGPU_DECL_FA_UNIT(SUF, T)                                                                              \
  int rdgpu_fa_d8_unit_##SUF(const T *dem, T nodata, int width, int height, double *accum_out);                 \
  int rdgpu_fa_d8_unit_dev_##SUF(const T *d_dem, T nodata, int width, int height, double *d_accum_out, void *hip_stream);
RDGPU_DECL_FA_UNIT(u8, uint8_t) RDGPU_DECL_FA_UNIT(i8, int8_t) RDGPU_DECL_FA_UNIT(i16, int16_t) RDGPU_DECL_FA_UNIT(u16, uint16_t)
RDGPU_DECL_FA_UNIT(i32, int32_t) RDGPU_DECL_FA_UNIT(u32, uint32_t) RDGPU_DECL_FA_UNIT(f32, float) RDGPU_DECL_FA_UNIT(f64, double)
RDGPU_DECL_FA_UNIT(i64, int64_t) RDGPU_DECL_FA_UNIT(u64, uint64_t)
#undef RDGPU_DECL_FA_UNIT

/* ---- D-infinity (Tarboton 1997) and the generic FlowAccumulation ---------------------------------
 * rdgpu_dinf_flowdirs_<T>   replaces richdem::dinf_flow_directions (include/richdem/flowmet/dinf_flowdirs.hpp
 *                           :128-152): float32 angle in [0, 2*pi), 0 = NO_FLOW, -1 = NoData.
 * rdgpu_fm_tarboton_<T>     replaces richdem::FM_Tarboton / FM_Dinfinity (flowmet/Tarboton1997.hpp:14-144):
 *                           9 floats per cell, index 9*i+n (common/Array3D.hpp:203-206).
 * rdgpu_fa_tarboton_<T>     replaces richdem::FA_Tarboton / FA_Dinfinity (methods/flow_accumulation.hpp:16-17);
 *                           accum in/out like rdgpu_fa_d8_*.
 * rdgpu_flow_accumulation_f64  replaces richdem::FlowAccumulation(const Array3D<float>&, Array2D<double>&)
 *                           (methods/flow_accumulation_generic.hpp:33-100) for ANY proportions array.
 * Angles/proportions use double atan2/sqrt as the reference does; device libm may differ from glibc in the
 * last ulp, so these are specified to <= 1 ULP (f32), not bit-exact; accumulation sums in a different
 * order than the reference's FIFO (exact for integer-valued flows). */
#define RDGPU_DECL_MFD(SUF, T)                                                                          \
  int rdgpu_dinf_flowdirs_##SUF(const T *dem, T nodata, int width, int height, float *angles);           \
  int rdgpu_dinf_flowdirs_dev_##SUF(const T *d_dem, T nodata, int width, int height, float *d_angles, void *hip_stream); \
  int rdgpu_fm_tarboton_##SUF(const T *dem, T nodata, int width, int height, float *props9);             \
  int rdgpu_fa_tarboton_##SUF(const T *dem, T nodata, int width, int height, double *accum);             \
  int rdgpu_fa_tarboton_dev_##SUF(const T *d_dem, T nodata, int width, int height, double *d_accum, void *hip_stream);
RDGPU_DECL_MFD(u8, uint8_t)
RDGPU_DECL_MFD(i16, int16_t)
RDGPU_DECL_MFD(u16, uint16_t)
RDGPU_DECL_MFD(i32, int32_t)
RDGPU_DECL_MFD(u32, uint32_t)
RDGPU_DECL_MFD(f32, float)
RDGPU_DECL_MFD(f64, double)
RDGPU_DECL_MFD(i8, int8_t)
#undef RDGPU_DECL_MFD
/* ---- D-infinity across flats ----------------------------------------------------------------------
 * FM_Tarboton gives a cell without a descending facet NO_FLOW, so on a filled DEM the D-infinity products stop at
 * every lake surface.  The _flats entries route such cells over Barnes' flat mask WITHOUT altering the DEM.  No
 * reference function returns this (its resolve_flats_barnes_dinf works on the angle raster, where flow due east and
 * NO_FLOW are both 0.0); the rule is defined here:
 *   1. the proportions start as rdgpu_fm_tarboton_<T>'s;
 *   2. d8 = rdgpu_d8_flowdirs(z), (flat_mask, labels) = rdgpu_flat_resolution_d8's mask path on (z, d8); NoData
 *      neighbours count by their value, as there;
 *   3. a cell c is PATCHED iff d8(c) == NO_FLOW and labels(c) != 0 (such a cell is interior);
 *   4. its 3 x 3 window of flat_mask, every neighbour with another label replaced by a NoData sentinel, goes through
 *      FM_Tarboton's cell rule (flowmet/Tarboton1997.hpp:75-141: 1e-7 thresholds, facets n = 1..8); the result
 *      replaces the cell's shares;
 *   5. where no facet descends, share 1 goes to the first n in 1..8 whose neighbour has the same label and a
 *      strictly smaller mask value;
 *   6. where there is none either, the cell stays NO_FLOW (counted in unresolved_cells).
 * Nothing else changes: cells with a gradient, flats without an outlet, edge cells and cells whose descending
 * facets all touch NoData are FM_Tarboton's.  Every patched share points at a smaller mask value: no cycles.
 * rdgpu_fm_tarboton_flats_<T>   the 9-float layout of rdgpu_fm_tarboton_<T>.
 * rdgpu_fa_tarboton_flats_<T>   rdgpu_fa_tarboton_<T> over these proportions; accum in/out, the 36 B/cell array is
 *                               never materialised.
 * (rdgpu_dinf_distance_down_flats_<T>: with the distance entries below.)
 * At most 0x7FFF0000 cells (the flat resolution's limit).  The _dev forms are ordered on hip_stream but wait for it
 * where the flat resolution reads its counts back.  Scratch: rdgpu_fa_tarboton's plus the flat resolution's plus one
 * byte per cell.
 * rdgpu_dinf_flats_get_stats: the counts of the calling thread's last _flats call (any of the entries); waits for that
 * call's stream.  All zero before the first call. */
typedef struct rdgpu_dinf_flats_stats {
  uint64_t noflow_cells;     /* interior data cells FM_Tarboton leaves without flow */
  uint64_t patched_cells;    /* cells patched under rule 3 */
  uint64_t fallback_cells;   /* of those, served by rule 5 */
  uint64_t unresolved_cells; /* patched but still without flow, rule 6 */
} rdgpu_dinf_flats_stats;
int rdgpu_dinf_flats_get_stats(rdgpu_dinf_flats_stats *out);
#define RDGPU_DECL_MFD_FLATS(SUF, T)                                                                            \
  int rdgpu_fm_tarboton_flats_##SUF(const T *dem, T nodata, int width, int height, float *props9);              \
  int rdgpu_fm_tarboton_flats_dev_##SUF(const T *d_dem, T nodata, int width, int height, float *d_props9, void *hip_stream); \
  int rdgpu_fa_tarboton_flats_##SUF(const T *dem, T nodata, int width, int height, double *accum);              \
  int rdgpu_fa_tarboton_flats_dev_##SUF(const T *d_dem, T nodata, int width, int height, double *d_accum, void *hip_stream);
RDGPU_DECL_MFD_FLATS(u8, uint8_t)
RDGPU_DECL_MFD_FLATS(i8, int8_t)
RDGPU_DECL_MFD_FLATS(u16, uint16_t)
RDGPU_DECL_MFD_FLATS(i16, int16_t)
RDGPU_DECL_MFD_FLATS(u32, uint32_t)
RDGPU_DECL_MFD_FLATS(i32, int32_t)
RDGPU_DECL_MFD_FLATS(f32, float)
RDGPU_DECL_MFD_FLATS(f64, double)
#undef RDGPU_DECL_MFD_FLATS
/* FM_Holmgren(x) / FM_Freeman(x) / FM_Quinn / FM_D4 proportions and the matching FA_* accumulations
 * (flowmet/Holmgren1994.hpp:14, Freeman1991.hpp:14, Quinn1991.hpp:13, OCallaghan1984.hpp:86;
 * methods/flow_accumulation.hpp:18-20,28).  method: 0 Holmgren, 1 Freeman, 2 Quinn, 3 D4; xparam is the
 * exponent of methods 0 and 1.  accum is in/out as for rdgpu_fa_d8 (in: flow generated per cell).      */
#define RDGPU_DECL_MFD2(SUF, T)                                                                          \
  int rdgpu_fm_mfd_##SUF(const T *dem, T nodata, int width, int height, int method, double xparam, float *props9); \
  int rdgpu_fm_mfd_dev_##SUF(const T *d_dem, T nodata, int width, int height, int method, double xparam, float *d_props9, void *hip_stream); \
  int rdgpu_fa_mfd_##SUF(const T *dem, T nodata, int width, int height, int method, double xparam, double *accum); \
  int rdgpu_fa_mfd_dev_##SUF(const T *d_dem, T nodata, int width, int height, int method, double xparam, double *d_accum, void *hip_stream);
RDGPU_DECL_MFD2(u8, uint8_t)
RDGPU_DECL_MFD2(i16, int16_t)
RDGPU_DECL_MFD2(u16, uint16_t)
RDGPU_DECL_MFD2(i32, int32_t)
RDGPU_DECL_MFD2(u32, uint32_t)
RDGPU_DECL_MFD2(f32, float)
RDGPU_DECL_MFD2(f64, double)
RDGPU_DECL_MFD2(i8, int8_t)
#undef RDGPU_DECL_MFD2
int rdgpu_flow_accumulation_f64(const float *props9, int width, int height, double *accum);
int rdgpu_flow_accumulation_dev_f64(const float *d_props9, int width, int height, double *d_accum, void *hip_stream);
int rdgpu_flow_accumulation_rounds(uint32_t *rounds); /* work-list rounds of the last generic accumulation */

/* ---- TerrainAttribute: slope, aspect, curvature, SPI, CTI ------------------------------------
 * Replaces richdem::TA_slope_riserun / _percentage / _degrees / _radians, TA_aspect, TA_curvature,
 * TA_planform_curvature, TA_profile_curvature and TA_SPI / TA_CTI (include/richdem/methods/terrain_attributes.hpp).
 * One pass of a 3 x 3 stencil in double, the reference's operations in the reference's order: rise/run, percentage and
 * the three curvatures are bit-equal to the reference's, the atan / atan2 / log attributes within 1 float32 ULP.
 * A neighbour that is off the grid or == nodata (compared in T) takes the centre's value; every value is multiplied by
 * zscale; cell_x / cell_y are the cell lengths |geotransform[1]| / |geotransform[5]| (their sign is ignored; zero or
 * non-finite is an error); a NoData cell gives out_nodata.  A flat window has aspect 270, as in the reference.
 *   rdgpu_terrain_attribute[_dev]_<T>    one attribute (an RDGPU_TA_* id) into one float plane
 *   rdgpu_terrain_attributes[_dev]_<T>   every attribute of `mask` (bit k = id k) in ONE launch / one read of the DEM:
 *                                        outs[k] is the plane of attribute k, for every bit k of mask (other entries of
 *                                        the RDGPU_TA_COUNT-entry array are not read)
 *   rdgpu_ta_spi[_dev] / rdgpu_ta_cti[_dev]   log((fa / (cell_x * cell_y)) * (slope + 0.001)), CTI with / for *; where
 *                                        fa == fa_nodata or slope == slope_nodata the result is -1, the NoData the
 *                                        reference sets on its output.
 * An unknown id / mask, a non-positive size, a null pointer or a bad cell length returns RDGPU_ERR_ARG before any
 * device work. */
enum {
  RDGPU_TA_SLOPE_RISERUN = 0,
  RDGPU_TA_SLOPE_PERCENTAGE = 1,
  RDGPU_TA_SLOPE_DEGREES = 2,
  RDGPU_TA_SLOPE_RADIANS = 3,
  RDGPU_TA_ASPECT = 4,
  RDGPU_TA_CURVATURE = 5,
  RDGPU_TA_PLANFORM_CURVATURE = 6,
  RDGPU_TA_PROFILE_CURVATURE = 7,
  RDGPU_TA_COUNT = 8
};
#define RDGPU_DECL_TERRAIN(SUF, T)                                                                                   \
  int rdgpu_terrain_attribute_##SUF(const T *dem, T nodata, int width, int height, double cell_x, double cell_y,     \
                                    float zscale, int attribute, float *out, float out_nodata);                      \
  int rdgpu_terrain_attribute_dev_##SUF(const T *d_dem, T nodata, int width, int height, double cell_x,              \
                                        double cell_y, float zscale, int attribute, float *d_out, float out_nodata,  \
                                        void *hip_stream);                                                           \
  int rdgpu_terrain_attributes_##SUF(const T *dem, T nodata, int width, int height, double cell_x, double cell_y,    \
                                     float zscale, unsigned mask, float *const *outs, float out_nodata);             \
  int rdgpu_terrain_attributes_dev_##SUF(const T *d_dem, T nodata, int width, int height, double cell_x,             \
                                         double cell_y, float zscale, unsigned mask, float *const *d_outs,           \
                                         float out_nodata, void *hip_stream);
RDGPU_DECL_TERRAIN(u8, uint8_t)
RDGPU_DECL_TERRAIN(i16, int16_t)
RDGPU_DECL_TERRAIN(u16, uint16_t)
RDGPU_DECL_TERRAIN(i32, int32_t)
RDGPU_DECL_TERRAIN(u32, uint32_t)
RDGPU_DECL_TERRAIN(f32, float)
RDGPU_DECL_TERRAIN(f64, double)
RDGPU_DECL_TERRAIN(i8, int8_t)
RDGPU_DECL_TERRAIN(i64, int64_t)
RDGPU_DECL_TERRAIN(u64, uint64_t)
#undef RDGPU_DECL_TERRAIN
int rdgpu_ta_spi(const double *fa, double fa_nodata, const float *slope, float slope_nodata, int width, int height,
                 double cell_x, double cell_y, float *out);
int rdgpu_ta_spi_dev(const double *d_fa, double fa_nodata, const float *d_slope, float slope_nodata, int width,
                     int height, double cell_x, double cell_y, float *d_out, void *hip_stream);
int rdgpu_ta_cti(const double *fa, double fa_nodata, const float *slope, float slope_nodata, int width, int height,
                 double cell_x, double cell_y, float *out);
int rdgpu_ta_cti_dev(const double *d_fa, double fa_nodata, const float *d_slope, float slope_nodata, int width,
                     int height, double cell_x, double cell_y, float *d_out, void *hip_stream);

/* ---- upslope cells, catchments and outlets on the D8 direction forest -------------------------
 * Replaces richdem::d8_upslope_cells (include/richdem/methods/d8_methods.hpp:144-236) and answers the two questions
 * next to it.  Directions are uint8 D8 codes (0 NO_FLOW, 1..8, dir_nodata).  "The path of cell c" is c, the cell c's
 * direction points to, and so on; it ends at a cell without a direction 1..8 (NO_FLOW, NoData, any other code) or
 * whose target is off the raster.  A path that runs into a direction loop never ends.  Exact; one read of the
 * directions per tile pass, two tile passes, 8 bytes of scratch per 16 cells.
 *   rdgpu_d8_catchments     every cell gets the label of the FIRST seed on its path, itself included; a cell whose path
 *                           meets no seed (or never ends without meeting one) gets `unreached`.  seed_cells are flat
 *                           indices y * width + x.  A seed labels itself whatever its own direction is (NoData, NO_FLOW,
 *                           a cell of a loop).  Of two entries for one cell the first of the list wins.  A seed
 *                           outside the raster returns RDGPU_ERR_ARG before anything is written.  n_seeds may be 0.
 *   rdgpu_d8_outlets        every cell whose direction is not NoData gets the flat index of the last cell of its path
 *                           that is not NoData: one id per drainage basin, and the id says where the basin drains.
 *                           NoData cells and cells whose path never ends get 0xFFFFFFFF.
 *   rdgpu_d8_upslope_cells  the reference's function: 2 on the cells of the line (x0,y0)-(x1,y1) as
 *                           rdgpu_d8_upslope_line rasterises it, 1 on every cell whose path meets one, 255
 *                           (FLOWDIR_NO_DATA) elsewhere.  x0 == x1 and y0 == y1: a pour point.
 *   rdgpu_d8_upslope_line   host code only (no GPU needed): the cells the reference's "modified Bresenham" marks, in its
 *                           order.  End points are swapped when x0 > x1; the error term and slope are float; per column
 *                           the cell (x, y) is marked, and when the error reaches 0.5 also (x + 1, y) before y moves by
 *                           one row -- a steep line stops short of (x1, y1); x0 == x1 with y0 != y1 marks (x0, y0) and
 *                           (x0 + 1, y0) only.  Where that procedure would mark a cell outside the raster (undefined
 *                           behaviour in the reference) RDGPU_ERR_ARG is returned and nothing is written.  *n receives
 *                           the number of cells (at most 2 * width); with cells == NULL and capacity == 0 only the
 *                           count is returned; a capacity below the count is RDGPU_ERR_ARG.
 * The _dev forms take device pointers (the seed arrays too) and are ordered on hip_stream; rdgpu_d8_catchments_dev
 * synchronises that stream once, to verify the seeds before it writes. */
int rdgpu_d8_catchments(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint32_t *seed_cells,
                        const int32_t *seed_labels, uint32_t n_seeds, int32_t unreached, int32_t *labels);
int rdgpu_d8_catchments_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, const uint32_t *d_seed_cells,
                            const int32_t *d_seed_labels, uint32_t n_seeds, int32_t unreached, int32_t *d_labels,
                            void *hip_stream);
int rdgpu_d8_outlets(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, uint32_t *outlet);
int rdgpu_d8_outlets_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, uint32_t *d_outlet, void *hip_stream);
int rdgpu_d8_upslope_cells(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, int x0, int y0, int x1, int y1,
                           uint8_t *out);
int rdgpu_d8_upslope_cells_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, int x0, int y0, int x1, int y1,
                               uint8_t *d_out, void *hip_stream);
int rdgpu_d8_upslope_line(int width, int height, int x0, int y0, int x1, int y1, uint32_t *cells, uint32_t capacity, uint32_t *n);

/* ---- upslope extremes: the largest or smallest value over each cell's drainage area ------------
 * No reference counterpart (TauDEM ships it as "D8 Extreme Upslope Value").  Directions are uint8 D8 codes (0 NO_FLOW,
 * 1..8 index the neighbour in the reference's dx / dy tables, dir_nodata); values is a raster of T of the same size.
 *   A cell PARTICIPATES iff dirs != dir_nodata.  A participating cell CONTRIBUTES iff its value is not value_nodata
 *   (compared with == in T: -0.0f equals a NoData of 0.0f) and, for f32, is not a NaN (a NaN never contributes, whatever
 *   value_nodata is).
 *   The LINK of a participating cell c exists iff its code is 1..8, its target lies in the raster and the target
 *   participates; otherwise c's tree ends at c.
 *   U(v), the upslope set of a participating cell v, is the set of participating cells whose chain of links reaches v,
 *   v included.  On a direction loop every loop cell has the same U: the loop and everything that drains into it.
 *   Nothing is special-cased for loops and no loop sentinel is written.
 *   ORDER: integers in their numeric order; f32 in the IEEE total order restricted to the non-NaN values,
 *   -inf < ... < -0 < +0 < ... < +inf: -0 and +0 are DISTINCT here and ordered, although == does not tell them apart.
 * Per-cell outputs, each a nullable pointer (a call must request at least one):
 *   at_cell  uint32  the lowest flat index y * width + x among the contributing cells of U(v) whose value is the maximum
 *                    (which == RDGPU_EXTREME_MAX) or the minimum (RDGPU_EXTREME_MIN) under that order; 0xFFFFFFFF where
 *                    v does not participate or U(v) has no contributing cell.
 *   extreme  T       values[at_cell[v]], bit for bit; value_nodata with its bits unchanged where at_cell is 0xFFFFFFFF.
 * Every cell of every requested plane is written exactly once, the inputs are not modified, and the result is exact and
 * identical from run to run.  T: i8 u8 i16 u16 i32 u32 f32.  f64, i64 and u64 are NOT declared: the engine carries value
 * and cell index in one 64-bit word, which 64-bit values do not fit.
 * A null dirs or values, both outputs null, a which other than 0 or 1, a non-positive size or more than 0xFFFF0000
 * cells returns RDGPU_ERR_ARG before any device work; nothing is written then.  The _dev forms take device pointers and
 * are ordered on hip_stream without synchronising it.  Scratch (1 byte per cell) comes from the workspace pool. */
enum { RDGPU_EXTREME_MAX = 0, RDGPU_EXTREME_MIN = 1 };
#define RDGPU_DECL_EXTREME(SUF, T)                                                                                          \
  int rdgpu_d8_upslope_extreme_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const T *values, T value_nodata, int width,  \
                                     int height, int which, T *extreme /* nullable */, uint32_t *at_cell /* nullable */);  \
  int rdgpu_d8_upslope_extreme_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const T *d_values, T value_nodata,     \
                                         int width, int height, int which, T *d_extreme /* nullable */,                    \
                                         uint32_t *d_at_cell /* nullable */, void *hip_stream);
RDGPU_DECL_EXTREME(i8, int8_t)
RDGPU_DECL_EXTREME(u8, uint8_t)
RDGPU_DECL_EXTREME(i16, int16_t)
RDGPU_DECL_EXTREME(u16, uint16_t)
RDGPU_DECL_EXTREME(i32, int32_t)
RDGPU_DECL_EXTREME(u32, uint32_t)
RDGPU_DECL_EXTREME(f32, float)
#undef RDGPU_DECL_EXTREME

/* ---- breaching along given D8 directions: pit levels carved down the direction forest ---------
 * The carve of CompleteBreaching_Lindsay2016 (depressions/Lindsay2016.hpp:138-153) on directions the caller gives -- the
 * flood's tree (rdgpu_breach_d8 below), flat-resolved directions, a channel tree -- stated as a reachability closure, so
 * that direction loops need no special case.  dirs are uint8 D8 codes as in rdgpu_d8_flow_path (0 NO_FLOW, 1..8,
 * dir_nodata), dem a raster of T of the same size, pits a uint8 mask (non-zero: the cell is a pit; required).
 *   A cell PARTICIPATES iff dirs != dir_nodata.  The LINK of a participating cell exists iff its code is 1..8, its target
 *   lies in the raster and the target participates (the links of the upslope extremes above).
 *   A PIT is a participating cell with pits != 0 whose value, for f32, is not a NaN.
 *   final(c) = the least dem(p) over the pits p with a chain of links p -> ... -> c on which every cell, c included, has
 *              dem >= dem(p) (p == c counts: a pit ends at its own level or below);
 *            = dem(c) where there is no such pit.
 *   A cell that does not participate is never a pit, is never changed and ends every chain; so does, for f32, a NaN cell.
 *   ORDER: integers in their numeric order; f32 in the IEEE total order on the non-NaN values (-0 below +0), as above.
 * Per-cell outputs, each a nullable pointer (a call must request at least one):
 *   out   T      final(c): a copy of some cell's value, bit for bit.
 *   path  uint8  1 where such a pit exists (a walk of the reference carves or passes the cell), else 0.
 * Every cell of every requested plane is written exactly once, the inputs are not modified, and the result is exact and
 * identical from run to run.  T: i8 u8 i16 u16 i32 u32 f32.  A null dirs, dem or pits, both outputs null, a non-positive
 * size or more than 0xFFFF0000 cells returns RDGPU_ERR_ARG before any device work; nothing is written then.  The _dev
 * forms take device pointers (d_out must not be d_dem) and are ordered on hip_stream without synchronising it.  Scratch
 * (1.5 bytes per cell) comes from the workspace pool. */
#define RDGPU_DECL_BREACH_ALONG(SUF, T)                                                                                    \
  int rdgpu_d8_breach_along_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const T *dem, const uint8_t *pits, int width,  \
                                  int height, T *out /* nullable */, uint8_t *path /* nullable */);                       \
  int rdgpu_d8_breach_along_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const T *d_dem, const uint8_t *d_pits,   \
                                      int width, int height, T *d_out /* nullable */, uint8_t *d_path /* nullable */,     \
                                      void *hip_stream);
RDGPU_DECL_BREACH_ALONG(i8, int8_t)
RDGPU_DECL_BREACH_ALONG(u8, uint8_t)
RDGPU_DECL_BREACH_ALONG(i16, int16_t)
RDGPU_DECL_BREACH_ALONG(u16, uint16_t)
RDGPU_DECL_BREACH_ALONG(i32, int32_t)
RDGPU_DECL_BREACH_ALONG(u32, uint32_t)
RDGPU_DECL_BREACH_ALONG(f32, float)
#undef RDGPU_DECL_BREACH_ALONG

/* ---- CompleteBreaching_Lindsay2016<Topology::D8>(Array2D<T>&) -- depressions/Lindsay2016.hpp:48-178 ----
 * In place.  Three stages: (1) the reference's pit pass as a stencil -- an interior cell not above any neighbour is a pit
 * and is raised to its lowest neighbour; (2) the Priority-Flood tree of the raised DEM under the reference's queue
 * conventions (edge cells seeded in raster order, neighbours pushed in the order 1..8, ties popped in insertion order:
 * rdgpu_pf_flowdirs' machinery with another convention, its bounds and environment switches included); (3)
 * rdgpu_d8_breach_along on that tree.  Equal to the reference on every cell, equal elevations included, while
 * stats.unresolved == 0.  f32 compares as the reference does (-0 equals +0; a zero of either sign is written as +0); NaN
 * elevations are unsupported input.
 *   dirs_out  uint8, nullable  the flood's tree: every interior cell points at the cell that pushed it (its back link), the
 *                              edge cells hold 0.
 *   path_out  uint8, nullable  1 on every cell a walk of the reference carves or passes, the pits included.
 * width < 3 or height < 3: the DEM is returned unchanged (dirs_out and path_out all 0).
 * has_nodata != 0 and some cell equal to nodata: RDGPU_ERR_UNSUPPORTED, found by one reduction before anything is written
 * (the reference seeds the cells next to NoData as well; not built).  has_nodata == 0: nodata is ignored.
 * A null dem, a non-positive size or more than 0x7FFF0000 cells is RDGPU_ERR_ARG before any device work.  The _dev forms
 * take device pointers and synchronise hip_stream (the tree is iterated from the host).  D4, the 64-bit element types and
 * the selective and constrained modes of Lindsay2016() are not declared. */
typedef struct rdgpu_breach_stats {
  uint64_t pits;        /* cells the pit pass marked */
  uint64_t lowered;     /* cells the carve left below the raised DEM */
  uint64_t raised;      /* cells the pit pass raised */
  uint64_t unresolved;  /* the tree's rdgpu_pf_flowdirs_stats.unresolved: 0 => the result is the reference's */
  uint32_t twins;       /* the tree's rdgpu_pf_flowdirs_stats.twins */
  uint32_t tie_passes;  /* the tree's rdgpu_pf_flowdirs_stats.tie_passes */
} rdgpu_breach_stats;
int rdgpu_breach_get_stats(rdgpu_breach_stats *out);
#define RDGPU_DECL_BREACH(SUF, T)                                                                                          \
  int rdgpu_breach_d8_##SUF(T *dem /* in place */, T nodata, int has_nodata, int width, int height,                       \
                            uint8_t *dirs_out /* nullable */, uint8_t *path_out /* nullable */);                          \
  int rdgpu_breach_d8_dev_##SUF(T *d_dem /* in place */, T nodata, int has_nodata, int width, int height,                 \
                                uint8_t *d_dirs_out /* nullable */, uint8_t *d_path_out /* nullable */, void *hip_stream);
RDGPU_DECL_BREACH(i8, int8_t)
RDGPU_DECL_BREACH(u8, uint8_t)
RDGPU_DECL_BREACH(i16, int16_t)
RDGPU_DECL_BREACH(u16, uint16_t)
RDGPU_DECL_BREACH(i32, int32_t)
RDGPU_DECL_BREACH(u32, uint32_t)
RDGPU_DECL_BREACH(f32, float)
#undef RDGPU_DECL_BREACH

/* ---- channel network and Strahler stream order on the D8 direction forest ---------------------
 * No reference counterpart (include/richdem/methods/strahler.hpp is a commented-out draft).  Directions are uint8 D8
 * codes (0 NO_FLOW, 1..8, dir_nodata); chan is an optional channel mask (uint8, non-zero = channel), and chan == NULL
 * means every cell whose direction is not dir_nodata is a channel.
 *   A CHANNEL CELL is a cell with chan != 0 and dirs != dir_nodata.  The CHANNEL CHILDREN of v are the channel cells
 *   among its eight neighbours whose direction 1..8 points at v.
 *   order(v) = 1                 for a channel cell without channel children,
 *            = m + 1 or m        for any other channel cell, m being the largest order among its children: m + 1 if at
 *                                least two children have order m (three equal children give m + 1, not m + 2), else m,
 *            = 0                 for a cell that is no channel cell, NoData cells included,
 *            = 255               for a channel cell on a direction loop, or downstream of one: its order has no finite
 *                                derivation.  (A cell has one target, so what lies downstream of a loop lies on it; the
 *                                channel cells that drain INTO a loop are ordinary trees and get finite orders.)
 *   The mask need not be closed downstream: a channel cell whose target is no channel cell, lies off the raster, or
 *   whose code is not 1..8 simply ends its tree.  An order k needs 2^(k-1) heads, so no order above 32 (let alone 254)
 *   can occur on a raster the engine accepts.  Exact.
 *   rdgpu_d8_channels_f64   chan = (accum != accum_nodata && accum >= threshold) ? 1 : 0; a threshold that is not
 *                           finite is RDGPU_ERR_ARG.
 *   rdgpu_d8_stream_links   classifies every channel cell from one 3 x 3 pass over dirs, chan and order; the kinds are
 *                           exclusive, the first that applies in the order of enum rdgpu_stream_kind; 0 on cells that
 *                           are no channel cells.
 *   rdgpu_d8_stream_order_get_stats   of the calling thread's last stream-order call: the levels and the node rounds
 *                           per level it ENQUEUED (bounds fixed by the raster's size; what has nothing to do returns
 *                           at once on the device), and its number of kernel launches.
 * A null pointer other than chan, a non-positive size or more cells than the engine accepts (0xFFFF0000) returns
 * RDGPU_ERR_ARG before any device work; nothing is written then.  The _dev forms take device pointers and are ordered
 * on hip_stream without synchronising it.  Scratch (13 bytes per 16 cells) comes from the workspace pool. */
enum rdgpu_stream_kind {
  RDGPU_STREAM_NONE = 0,       /* no channel cell */
  RDGPU_STREAM_HEAD = 1,       /* no channel child */
  RDGPU_STREAM_JUNCTION = 2,   /* at least two channel children */
  RDGPU_STREAM_ORDER_STEP = 3, /* one channel child of another order: cannot occur by the definition, an assertion value */
  RDGPU_STREAM_MOUTH = 4,      /* its target is no channel cell */
  RDGPU_STREAM_PLAIN = 5
};
int rdgpu_d8_stream_order(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan /* nullable */,
                          uint8_t *order);
int rdgpu_d8_stream_order_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height,
                              const uint8_t *d_chan /* nullable */, uint8_t *d_order, void *hip_stream);
int rdgpu_d8_stream_order_get_stats(int *levels, int *rounds_per_level, int *launches);
int rdgpu_d8_channels_f64(const double *accum, double accum_nodata, double threshold, int width, int height, uint8_t *chan);
int rdgpu_d8_channels_dev_f64(const double *d_accum, double accum_nodata, double threshold, int width, int height,
                              uint8_t *d_chan, void *hip_stream);
int rdgpu_d8_stream_links(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan /* nullable */,
                          const uint8_t *order, uint8_t *kind);
int rdgpu_d8_stream_links_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height,
                              const uint8_t *d_chan /* nullable */, const uint8_t *d_order, uint8_t *d_kind, void *hip_stream);

/* ---- flow distance, drainage cell and HAND on the D8 direction forest --------------------------
 * No reference counterpart.  Directions are uint8 D8 codes (0 NO_FLOW, 1..8 index the neighbour in the reference's
 * dx / dy tables, dir_nodata); "the path of cell c" is the one of the upslope entries above; chan is an optional uint8
 * mask as in the stream-order entries.
 *   A STOP CELL is a cell with chan != 0 and dirs != dir_nodata.
 *   With chan given, the DRAINAGE CELL of c is the first stop cell on c's path, c included.  With chan == NULL it is the
 *   last cell of c's path that is not NoData: rdgpu_d8_outlets' answer, bit for bit.
 *   A cell has NO drainage cell when its direction is NoData, when its path ends without meeting a stop cell, or when
 *   its path runs into a direction loop before meeting one.  A stop cell on a loop is its own drainage cell and breaks
 *   the loop for everything upstream of it.
 * Per-cell outputs, each a nullable pointer (a call must request at least one):
 *   to_cell  uint32                    flat index y * width + x of the drainage cell, 0xFFFFFFFF where there is none.
 *   steps    uint32 [3][height][width] the steps from c to its drainage cell: plane 0 along x (codes 1, 5: dy == 0),
 *                                      plane 1 along y (codes 3, 7: dx == 0), plane 2 diagonal.  All 0 on a drainage
 *                                      cell, all 0xFFFFFFFF where there is none.  A path has fewer steps than the
 *                                      raster has cells, so no count overflows.
 *   dist     float64                   (double)nx * cell_x + (double)ny * cell_y + (double)nd * diag, evaluated in that
 *                                      order with a rounding after every product and every sum (no fused multiply-add),
 *                                      diag = sqrt(cell_x * cell_x + cell_y * cell_y) computed once on the host;
 *                                      dist_nodata where there is no drainage cell.  A function of three integers:
 *                                      exact, independent of any summation order.
 *   hand     float64 (rdgpu_d8_hand_<T>, which also takes the DEM): (double)dem[c] - (double)dem[to_cell[c]];
 *                                      out_nodata where there is no drainage cell or where either elevation equals
 *                                      dem_nodata (compared in T).  Not clamped: an unfilled DEM may give negative
 *                                      values.  T: i8 u8 i16 u16 i32 u32 f32 f64 -- one rounding of exact operands.
 * cell_x and cell_y: their sign is ignored; zero or not finite is RDGPU_ERR_ARG.  A null dirs (dem, hand), no output
 * requested, a non-positive size or more than 0xFFFF0000 cells returns RDGPU_ERR_ARG before any device work; nothing
 * is written then.  The _dev forms take device pointers and are ordered on hip_stream without synchronising it.
 * Scratch (2.5 bytes per cell; HAND 4 more) comes from the workspace pool. */
int rdgpu_d8_flow_path(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan /* nullable */,
                       double cell_x, double cell_y, uint32_t *to_cell /* nullable */, uint32_t *steps /* nullable */,
                       double *dist /* nullable */, double dist_nodata);
int rdgpu_d8_flow_path_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, const uint8_t *d_chan /* nullable */,
                           double cell_x, double cell_y, uint32_t *d_to_cell /* nullable */, uint32_t *d_steps /* nullable */,
                           double *d_dist /* nullable */, double dist_nodata, void *hip_stream);
#define RDGPU_DECL_HAND(SUF, T)                                                                                       \
  int rdgpu_d8_hand_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const T *dem, T dem_nodata, int width, int height, \
                          const uint8_t *chan /* nullable */, double *hand, double out_nodata);                       \
  int rdgpu_d8_hand_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const T *d_dem, T dem_nodata, int width,     \
                              int height, const uint8_t *d_chan /* nullable */, double *d_hand, double out_nodata,    \
                              void *hip_stream);
RDGPU_DECL_HAND(i8, int8_t)
RDGPU_DECL_HAND(u8, uint8_t)
RDGPU_DECL_HAND(i16, int16_t)
RDGPU_DECL_HAND(u16, uint16_t)
RDGPU_DECL_HAND(i32, int32_t)
RDGPU_DECL_HAND(u32, uint32_t)
RDGPU_DECL_HAND(f32, float)
RDGPU_DECL_HAND(f64, double)
#undef RDGPU_DECL_HAND

/* ---- stream reaches on the D8 direction forest: reach labels, one record per reach, reach catchments ----
 * No reference counterpart (TauDEM's StreamNet calls these links; rdgpu_d8_stream_links above keeps that name for its
 * per-cell kinds).  Directions are uint8 D8 codes (0 NO_FLOW, 1..8, dir_nodata); chan is the optional uint8 mask of the
 * stream-order block (NULL: every cell with dirs != dir_nodata is a channel cell).  CHANNEL CELL and CHANNEL CHILDREN are
 * those of that block; the CHANNEL TARGET of a channel cell is the cell its code 1..8 points at, if that is a channel
 * cell (else it has none).
 *   A channel cell is a TOP iff it has 0 channel children (a head) or at least 2 (a junction).  A junction belongs to
 *   the reach below it.  A channel cell with exactly one channel child belongs to the reach of that child.
 *   A REACH is a top together with every cell that reaches it by walking up through only-children.
 *   The BOTTOM of a reach is its cell whose channel target does not exist (a mouth) or is a junction.  Every bottom has
 *   exactly one top.  A channel cell on a direction loop that no channel tributary joins has no top and belongs to NO
 *   reach.  A loop that a tributary joins is an ordinary reach from that junction round to the cell before it; its
 *   `down` is then its own label or that of another loop reach.  Nothing is special-cased for loops.
 *   NUMBERING: reaches are labelled 1..N by ascending raster index y * width + x of their bottom cell, independent of
 *   any execution order.  0 means "none".
 *   The CATCHMENT of a cell c with dirs != dir_nodata: follow the path of c (the path of the upslope block, over the
 *   full directions, c included) to its first channel cell; the catchment is that cell's reach label.  It is 0 when the
 *   path ends or enters a loop before meeting a channel cell, when that channel cell has no reach, and on NoData cells.
 *   On a channel cell, catchment equals reach.  Equivalently -- the engine's route -- it is the label of the first
 *   reach-bottom on c's path: to_cell of rdgpu_d8_flow_path with the bottoms as chan.
 * Outputs, each nullable except count:
 *   reach      uint32  the label of the reach a channel cell belongs to, 0 elsewhere.
 *   catchment  uint32  as defined above.
 *   table      the first min(N, capacity) records by label (table[i] describes label i + 1); records past N are not
 *              touched.  table == NULL with capacity == 0 is the sizing call.
 *   count      always the true N.  A call with only count is valid.
 * Every requested plane is written on every cell; inputs are never written.  Every field is an integer count or a
 * function of integer counts: exact, and identical from run to run.
 * A null dirs or count, a null table with a non-zero capacity, a non-positive size or more than 0xFFFF0000 cells, cell
 * lengths that are zero or not finite (their sign is ignored) return RDGPU_ERR_ARG before any device work; nothing is
 * written then.  The _dev form takes device pointers (d_count included) and is ordered on hip_stream without
 * synchronising it.  Scratch comes from the workspace pool: 3 bytes per cell (bottom mask, cell class, rank of a bottom
 * in its block of 256 cells), the flow-path engine's 2.5, and 4 more when neither label plane is requested while the
 * table is (the drainage cells live in a requested plane otherwise). */
typedef struct rdgpu_reach {
  uint32_t top_cell;        /* its head or junction */
  uint32_t bottom_cell;
  uint32_t down;            /* label of the reach its bottom's channel target belongs to; 0 at a mouth */
  uint32_t up;              /* channel children of top_cell: 0 head, 2..8 junction; == number of reaches whose down is
                               this label */
  uint32_t cells;           /* channel cells in the reach */
  uint32_t catchment_cells; /* cells whose catchment is this label, channel cells included */
  uint32_t steps[3];        /* cells of the reach that have a channel target, by the kind of that step: x (codes 1, 5),
                               y (3, 7), diagonal; the bottom's step into the junction it joins counts, a mouth's does
                               not exist */
  uint32_t order;           /* order[top_cell] if an order raster is given (it is constant along a reach), else 0; not
                               checked */
  double length;            /* steps as a length, evaluated as rdgpu_d8_flow_path's dist is (a rounding after every
                               product and every sum, diag once on the host) */
} rdgpu_reach;              /* 48 bytes, no implicit padding */
int rdgpu_d8_stream_reaches(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, const uint8_t *chan /* nullable */,
                            const uint8_t *order /* nullable */, double cell_x, double cell_y, uint32_t *reach /* nullable */,
                            uint32_t *catchment /* nullable */, rdgpu_reach *table /* nullable */, uint32_t capacity,
                            uint32_t *count);
int rdgpu_d8_stream_reaches_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height,
                                const uint8_t *d_chan /* nullable */, const uint8_t *d_order /* nullable */, double cell_x,
                                double cell_y, uint32_t *d_reach /* nullable */, uint32_t *d_catchment /* nullable */,
                                rdgpu_reach *d_table /* nullable */, uint32_t capacity, uint32_t *d_count, void *hip_stream);

/* ---- longest upstream flow path on the D8 direction forest -------------------------------------
 * No reference counterpart (TauDEM's plen, WhiteboxTools' MaxUpslopeFlowpathLength and LongestFlowpath).  Directions are
 * uint8 D8 codes (0 NO_FLOW, 1..8, dir_nodata).
 *   D(c), steps(c), outlet(c) are dist, steps and to_cell of rdgpu_d8_flow_path with chan == NULL, bit for bit.  A cell
 *   HAS A PATH iff that to_cell is not 0xFFFFFFFF: NoData cells have none, nor do cells whose path runs into a direction
 *   loop.
 *   U(v), for a cell v with a path, is v and every cell whose path passes through v; all of them have a path.
 *   head(v) is the cell of U(v) with the greatest D, compared as doubles (all finite and >= 0); among equal D the lowest
 *   flat index y * width + x.  For u in U(v) the steps from u to v are steps(u) - steps(v) plane by plane, so head(v) is
 *   the cell upstream of v that is farthest from v.  D is a ROUNDED function of three integers: two different step
 *   triples whose real lengths lie within a rounding of each other are ordered by their rounded D, and by index where
 *   the rounded values are equal.
 * Per-cell outputs, each a nullable pointer (a call must request at least one):
 *   from_cell      uint32                    head(v); 0xFFFFFFFF where v has no path.
 *   steps          uint32 [3][height][width] steps(head(v)) - steps(v) per plane (along x, along y, diagonal).  All 0
 *                                            where v is its own head, all 0xFFFFFFFF where v has no path.
 *   length         float64                   (double)nx * cell_x + (double)ny * cell_y + (double)nd * diag of those three
 *                                            counts, evaluated as rdgpu_d8_flow_path's dist is (a rounding after every
 *                                            product and every sum, no fused multiply-add, diag computed once on the
 *                                            host); length_nodata where v has no path.
 *   on_basin_path  uint8                     1 iff head(v) == head(outlet(v)), else 0; 0 where v has no path.  These are
 *                                            exactly the cells of the longest flow path of v's basin, from its head down
 *                                            to the outlet: head(v) lies in U(v), so the head's path passes through v,
 *                                            and a cell on head(outlet)'s path has that cell as the maximum of its own,
 *                                            smaller upslope set.
 * Every cell of every requested plane is written exactly once, the inputs are not modified, and the result is exact and
 * identical from run to run.  cell_x and cell_y: their sign is ignored; zero or not finite is RDGPU_ERR_ARG.  A null
 * dirs, no output requested, a non-positive size or more than 0xFFFF0000 cells returns RDGPU_ERR_ARG before any device
 * work; nothing is written then.  The _dev form takes device pointers and is ordered on hip_stream without
 * synchronising it.  Scratch (16 bytes per cell, the flow-path engine's 2.5 among them; on_basin_path 4 more, 8 without
 * from_cell) comes from the workspace pool. */
int rdgpu_d8_longest_flow_path(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, double cell_x, double cell_y,
                               uint32_t *from_cell /* nullable */, uint32_t *steps /* nullable */, double *length /* nullable */,
                               double length_nodata, uint8_t *on_basin_path /* nullable */);
int rdgpu_d8_longest_flow_path_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, double cell_x, double cell_y,
                                   uint32_t *d_from_cell /* nullable */, uint32_t *d_steps /* nullable */,
                                   double *d_length /* nullable */, double length_nodata, uint8_t *d_on_basin_path /* nullable */,
                                   void *hip_stream);

/* ---- weighted accumulation on the D8 direction forest, and the total upstream length -----------
 * The reference's FlowAccumulation (methods/flow_accumulation_generic.hpp:33-100) on the proportions of GIVEN D8
 * directions, without the [h, w, 9] proportions array.  Directions are uint8 D8 codes (0 NO_FLOW, 1..8 index the
 * neighbour in the reference's dx / dy tables, dir_nodata); weights is a raster of W of the same size.
 *   A cell PARTICIPATES iff dirs != dir_nodata.  A participating cell CONTRIBUTES iff its weight is not weight_nodata
 *   (compared with == in W: -0.0 equals a NoData of 0.0) and, for f32 and f64, is not a NaN (a NaN never contributes,
 *   whatever weight_nodata is).  A cell that does not contribute still passes on what it receives; infinities are added
 *   as they are.
 *   The LINK of a participating cell c exists iff its code is 1..8, its target lies in the raster and the target
 *   participates; otherwise c's tree ends at c.
 *   A cell is ON A LOOP iff following links from it comes back to it.
 *   T(v), for a participating cell v, holds v and every cell u whose chain of links reaches v with no cell of that chain
 *   before v on a loop.  For a cell off every loop this is its whole drainage area; for a loop cell it is the trees that
 *   enter the loop at that cell: the links of a loop carry nothing.  Nothing is special-cased for loops and no loop
 *   sentinel is written.
 *   sum[v] is the sum of the weights of the contributing cells of T(v); sum_nodata where v does not participate.
 * This is what the reference leaves in its accumulation array (loop cells keep their own weight plus what arrived), with
 * two deliberate differences: edge cells take part like any other cell, and the NoData value is the caller's.
 * W: i8 u8 i16 u16 i32 u32 with S = int64_t: exact and identical from run to run; the sum fits int64_t on every raster
 * below 2^31 cells.  W: f32 f64 with S = double: every weight is converted to double exactly, then added in double in an
 * unspecified order -- exact, and therefore reproducible, whenever every partial sum is representable (integer-valued
 * weights, as for rdgpu_fa_d8); otherwise within the recursive-summation bound of the true sum,
 * |sum[v] - true| <= g * (sum of |w| over T(v)), g = (k - 1) u / (1 - (k - 1) u), u = 2^-53, k the contributing cells
 * of T(v).  64-bit integer weights are NOT declared.
 * Every cell of sum is stored exactly once (sum is also the accumulator: a cell that receives inflow is afterwards
 * changed by atomic adds alone, so nothing but the final value may be read from it); the inputs are not modified.  A null pointer, a non-positive size or more than 0xFFFF0000 cells returns RDGPU_ERR_ARG before any device
 * work; nothing is written then.  The _dev forms take device pointers and are ordered on hip_stream without
 * synchronising it.  Scratch (4 bytes per cell) comes from the workspace pool. */
#define RDGPU_DECL_WEIGHTED(SUF, W, S)                                                                                    \
  int rdgpu_d8_flow_accum_weighted_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const W *weights, W weight_nodata,     \
                                         int width, int height, S *sum, S sum_nodata);                                   \
  int rdgpu_d8_flow_accum_weighted_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const W *d_weights,              \
                                             W weight_nodata, int width, int height, S *d_sum, S sum_nodata,             \
                                             void *hip_stream);
RDGPU_DECL_WEIGHTED(i8, int8_t, int64_t)
RDGPU_DECL_WEIGHTED(u8, uint8_t, int64_t)
RDGPU_DECL_WEIGHTED(i16, int16_t, int64_t)
RDGPU_DECL_WEIGHTED(u16, uint16_t, int64_t)
RDGPU_DECL_WEIGHTED(i32, int32_t, int64_t)
RDGPU_DECL_WEIGHTED(u32, uint32_t, int64_t)
RDGPU_DECL_WEIGHTED(f32, float, double)
RDGPU_DECL_WEIGHTED(f64, double, double)
#undef RDGPU_DECL_WEIGHTED
/* The total upstream length (TauDEM's tlen): the summed length of every link of the tree above a cell.  Participation,
 * links, loops and T(v) are those of the block above.  Per-cell outputs, each a nullable pointer (a call must request at
 * least one):
 *   steps    uint32 [3][height][width] plane k: the number of cells u of T(v), v excluded, whose link is of kind k --
 *                                      plane 0 along x (codes 1, 5), plane 1 along y (codes 3, 7), plane 2 diagonal:
 *                                      rdgpu_d8_flow_path's three kinds.  All 0xFFFFFFFF where v does not participate.
 *   length   float64                   (double)nx * cell_x + (double)ny * cell_y + (double)nd * diag of those three
 *                                      counts, evaluated as rdgpu_d8_flow_path's dist is (a rounding after every
 *                                      product and every sum, no fused multiply-add, diag computed once on the
 *                                      host); length_nodata where v does not participate.
 * Exact and identical from run to run.  cell_x and cell_y: their sign is ignored; zero or not finite is RDGPU_ERR_ARG.
 * A null dirs, no output requested, a non-positive size or more than 0xFFFF0000 cells returns RDGPU_ERR_ARG before any
 * device work; nothing is written then.  The _dev form takes device pointers and is ordered on hip_stream without
 * synchronising it.  Scratch (20 bytes per cell) comes from the workspace pool. */
int rdgpu_d8_total_upstream_length(const uint8_t *dirs, uint8_t dir_nodata, int width, int height, double cell_x, double cell_y,
                                   uint32_t *steps /* nullable */, double *length /* nullable */, double length_nodata);
int rdgpu_d8_total_upstream_length_dev(const uint8_t *d_dirs, uint8_t dir_nodata, int width, int height, double cell_x,
                                       double cell_y, uint32_t *d_steps /* nullable */, double *d_length /* nullable */,
                                       double length_nodata, void *hip_stream);

/* ---- limited accumulation on the D8 direction forest: losses, decay and capacity --------------
 * The accumulation above with a per-cell limit on what a cell passes on.  It covers the descent of the reference's
 * MoveWaterIntoPits (depressions/fill_spill_merge.hpp:226-318: a negative wtd is a storage deficit that inflow fills
 * before anything moves on) and TauDEM's DecayAccum and TransLimAccum.  Participation, contribution (of `supply`,
 * against supply_nodata), links, loops and the raster limits are those of rdgpu_d8_flow_accum_weighted_<W>, word for
 * word.  W is f32 or f64; supply, capacity and factor are rasters of W, converted to double exactly, and everything is
 * computed in double.  s(v) is v's supply where it contributes, else 0.  For a participating cell v off the loops:
 *   total(v) = s(v) + the sum of out(u) over the cells u whose link ends at v;
 *   a        = factor ? factor(v) * total(v) : total(v)      a NaN factor counts as 1; any other factor is used as given
 *                                                            (IEEE arithmetic: a NaN product counts as 0);
 *   out(v)   = min(max(a, 0), max(capacity(v), 0))           capacity == NULL or a NaN cell: no limit; +inf is allowed;
 *   kept(v)  = total(v) - out(v)                             positive: deposited, stored or decayed there; negative: a
 *                                                            deficit that inflow did not fill.
 * The out of a cell without a link is what leaves the system there (a pit, a flat cell, the raster's edge, a NoData
 * neighbour).  A LOOP cell never completes: its out is 0, its kept is its own supply plus what its tributaries brought;
 * the links of a loop carry nothing.  Cells that do not participate get nodata_out in both planes.
 * OUTPUTS, each nullable; at least one must be requested, and a plane that is not requested is not written:
 *   out, kept   float64 [height][width]; they must not overlap each other or an input.
 *   result      supplied: the sum of the contributing supplies of participating cells; left: the sum of out over the
 *               participating cells without a link; kept_pos / kept_neg: the sums of the positive / negative kept.
 *               supplied = left + kept_pos + kept_neg up to summation order: the mass balance.
 * ARITHMETIC.  The sums arrive in an unspecified order; the result is exact, and therefore reproducible, whenever every
 * partial sum and product is representable (dyadic supplies and factors of moderate range).  With factor NULL or every
 * factor in [0, 1] each node map is monotone and non-expansive, so a rounding made upstream never grows on its way down:
 * out(v) and kept(v) lie within g * (sum of |s| over T(v)), g = k u / (1 - k u), u = 2^-53, k the cells of T(v), of their
 * exact values, plus one rounding for kept (the k - 1 additions of T(v) give this as in the block above; the up to k
 * products of a factor raster are roundings too, so with a factor what is PROVEN is 2 k in place of k, and the tests hold
 * the engine to k).  NO bound is given for factors outside [0, 1].  The four sums of result are plain double sums in no
 * fixed order.
 * A null dirs or supply, no output requested, a non-positive size or more than 0xFFFF0000 cells returns RDGPU_ERR_ARG
 * before any device work; nothing is written then.  Inputs are never written.  The _dev forms take device pointers
 * (d_result: one device struct) and are ordered on hip_stream without synchronising it: three launches and, with
 * d_result, one memset.  Scratch (4 bytes per cell; 8 more when neither plane is requested) comes from the workspace pool
 * under names starting with "accum_limited.". */
typedef struct rdgpu_limited_result {       /* 32 bytes */
  double supplied, left, kept_pos, kept_neg;
} rdgpu_limited_result;
#define RDGPU_DECL_LIMITED(SUF, W)                                                                                        \
  int rdgpu_d8_flow_accum_limited_##SUF(const uint8_t *dirs, uint8_t dir_nodata, const W *supply, W supply_nodata,       \
                                        const W *capacity /* nullable */, const W *factor /* nullable */, int width,     \
                                        int height, double *out /* nullable */, double *kept /* nullable */,             \
                                        double nodata_out, rdgpu_limited_result *result /* nullable */);                 \
  int rdgpu_d8_flow_accum_limited_dev_##SUF(const uint8_t *d_dirs, uint8_t dir_nodata, const W *d_supply,                \
                                            W supply_nodata, const W *d_capacity /* nullable */,                         \
                                            const W *d_factor /* nullable */, int width, int height,                     \
                                            double *d_out /* nullable */, double *d_kept /* nullable */,                 \
                                            double nodata_out, rdgpu_limited_result *d_result /* nullable */,            \
                                            void *hip_stream);
RDGPU_DECL_LIMITED(f32, float)
RDGPU_DECL_LIMITED(f64, double)
#undef RDGPU_DECL_LIMITED

/* ---- depression inventory: labels and one record per depression of the fill --------------------
 * No reference counterpart (the flat inventory of the lakes FillDepressions produces; the tree of the depressions
 * inside them is rdgpu_depression_hierarchy_<T> below).  Let W = FillDepressions<topology>(dem) exactly as rdgpu_fill_<T> computes it; NoData is an elevation like any
 * other, as in that entry.  A cell is RAISED iff W > dem.  A DEPRESSION is a connected component of the raised cells
 * under `topology` (8 or 4, the one used for the fill).  Adjacent raised cells share one W: the depression's level.
 *   labels  int32 per cell (nullable): 0 on un-raised cells, 1..N on depressions, numbered by ascending lowest raster
 *           index (y * width + x) of their cells -- independent of any execution order.  Always complete.
 *   table   (nullable) record i describes label i + 1; at most `capacity` records are written, the first ones by label.
 *   count   N, always the true number whatever the capacity.  table == NULL with capacity == 0 is the sizing call.
 * Integer element types sum `volume` in 64-bit integers and convert once (exact below 2^53).  f32 / f64 sum it in
 * double in no fixed order: its last bits are NOT reproducible from run to run; every term is non-negative, so
 * |volume - exact sum| <= cells * 2^-52 * (exact sum).  Every other field is exact and reproducible.
 * f64 runs on the dense value ranks of the raster (structure) and gathers level, pit_elevation and volume from the
 * original values.  The i64 / u64 entries exist and return RDGPU_ERR_UNSUPPORTED: a double cannot carry their
 * elevations or volumes exactly.  Argument checks and size limits are those of rdgpu_fill_<T>; a null count, or a null
 * table with a non-zero capacity, is RDGPU_ERR_ARG.  A DEM with nothing to raise gives all-zero labels and count 0.
 * The _dev forms take device pointers (d_count one device word) and are ordered on hip_stream; like
 * rdgpu_fill_max_dep_dev_<T> they add no wait of their own to those of the fill's local phase.  Scratch comes from the
 * workspace pool under names starting with "depr.". */
typedef struct rdgpu_depression {
  uint32_t first_cell;    /* lowest raster index in the depression */
  uint32_t pit_cell;      /* index of its lowest dem value; the lowest index among equal values */
  uint32_t outlet_cell;   /* lowest raster index among the UN-raised cells adjacent (by topology) to the depression
                             with dem == level: where the flood enters it */
  uint32_t cells;         /* number of cells */
  double level;           /* (double)dem[outlet_cell] = W on every cell of the depression */
  double pit_elevation;   /* (double)dem[pit_cell] */
  double volume;          /* sum over the cells of (level - dem), in elevation units x cells */
} rdgpu_depression;
#define RDGPU_DECL_DEPR(SUF, T)                                                                                        \
  int rdgpu_depressions_##SUF(const T *dem, int width, int height, int topology, int32_t *labels /* nullable */,      \
                              rdgpu_depression *table /* nullable */, uint32_t capacity, uint32_t *count);            \
  int rdgpu_depressions_dev_##SUF(const T *d_dem, int width, int height, int topology, int32_t *d_labels /* nullable */, \
                                  rdgpu_depression *d_table /* nullable */, uint32_t capacity, uint32_t *d_count,     \
                                  void *hip_stream);
RDGPU_DECL_DEPR(u8, uint8_t)
RDGPU_DECL_DEPR(i8, int8_t)
RDGPU_DECL_DEPR(i16, int16_t)
RDGPU_DECL_DEPR(u16, uint16_t)
RDGPU_DECL_DEPR(i32, int32_t)
RDGPU_DECL_DEPR(u32, uint32_t)
RDGPU_DECL_DEPR(f32, float)
RDGPU_DECL_DEPR(f64, double)
RDGPU_DECL_DEPR(i64, int64_t)   /* RDGPU_ERR_UNSUPPORTED */
RDGPU_DECL_DEPR(u64, uint64_t)  /* RDGPU_ERR_UNSUPPORTED */
#undef RDGPU_DECL_DEPR

/* ---- depression hierarchy: the merge tree of the depressions, leaf labels, levels and volumes ----
 * Reference: depressions/depression_hierarchy.hpp (GetDepressionHierarchy with its marginal and total volumes), for a
 * DEM whose border ring is the ocean.  The reference's tree depends on its pop order wherever two elevations are equal
 * or two outlets share a saddle cell; this contract does not.
 *
 * DEFINITIONS.  Let < on cells be the strict total order by (dem value, raster index y * width + x).  NoData is an
 * elevation like any other, as in rdgpu_fill_<T>.  topology is 8 or 4.
 *   Descent.  Every interior cell points at its lowest neighbour if that neighbour is lower than itself, otherwise it
 *     is a PIT.  Cells of the border ring drain OUTSIDE.  leaf(c) is the pit the descent path of c ends in, or outside
 *     if the path reaches the border ring.
 *   Edges.  For adjacent cells a, b with leaf(a) != leaf(b) (outside counts as a leaf here): hi is the greater of the
 *     two cells and lo the lesser under <; the edge key is (dem[hi], hi index, lo index), compared lexicographically;
 *     the edge between two leaves is the minimum key over all their adjacent cell pairs.  The order is total, so
 *     nothing below depends on an execution order.
 *   Tree.  Kruskal over the edges in ascending key, with outside as a node.  An edge whose two ends are in the same set
 *     is skipped.  If one end's set contains outside, the other set's top node becomes a ROOT: parent = NONE, and the
 *     set joins outside.  Otherwise the two top nodes A, B get a new parent node N.  The node that is merged or made a
 *     root takes the edge's spill fields: level = dem[hi], inside_cell (the edge cell that lies in the node) and
 *     outside_cell (the other one).  lchild is the child with the lower pit_cell under <, and N.pit_cell =
 *     lchild.pit_cell.
 *   Numbering.  Leaves are 0..P-1 by ascending pit raster index; internal nodes are P..count-1 in creation order, that
 *     is ascending edge key, so child id < parent id.  NONE is 0xFFFFFFFF.
 *   Reductions.  cells(n) = #{c : leaf(c) below n, dem[c] <= level(n)}, and volume(n) is the sum of (level(n) - dem[c])
 *     over those cells.  Equivalently a cell is charged to its first ancestor-or-self with level >= dem[c] and the
 *     totals add up the tree: the reference's CalculateMarginalVolumes / CalculateTotalVolumes, including its <=.
 *     Integer element types sum in 64-bit integers and convert once.  f32 sums in double in no fixed order:
 *     |volume - exact| <= cells * 2^-52 * exact; every other field is exact and reproducible.
 *
 * ENTRIES.  labels (int32 per cell, nullable): the leaf id of leaf(c), -1 where that is outside.  table (nullable):
 * record i is node i; at most `capacity` records are written, the first ones.  count: the number of nodes, always the
 * true value; table == NULL with capacity == 0 is the sizing call.  leaves (nullable): P.  A raster without pits gives
 * count 0, leaves 0 and all labels -1.  Element types u8, i8, i16, u16, i32, u32, f32; the f64, i64 and u64 entries
 * exist and return RDGPU_ERR_UNSUPPORTED.  Argument checks are those of rdgpu_depressions_<T>: a null dem or count, a
 * non-positive size, a topology other than 8 or 4, a null table with a non-zero capacity or more than 2^31-65536 cells
 * is RDGPU_ERR_ARG before any device work, and nothing is written then.  The input is never written.  The _dev forms
 * take device pointers (d_count, d_leaves one device word each) and are ordered on hip_stream, which they wait for
 * several times: the tree is built on the host (rdgpu_dephier_stats.builder).  Scratch comes from the workspace pool
 * under names starting with "dephier.".
 *
 * A CALLER-GIVEN OCEAN.  rdgpu_depression_hierarchy_ocean_<T> takes the same arguments plus `ocean` after `topology`: one
 * byte per cell, non-zero means ocean (the reference's label raster with OCEAN marked; rdgpu_bucket_fill_from_edges_<T>
 * below builds such a mask).  ocean == NULL is the border ring: the entry above, bit for bit.  Otherwise the
 * DEFINITIONS hold with these differences:
 *   Ocean set.  O is the set of cells with a non-zero byte.  The border ring is NOT added to it: a caller who wants the
 *     ring sets it in the mask.
 *   Descent.  A cell of O drains OUTSIDE.  Every other cell, border cells included, points at its lowest neighbour inside
 *     the raster under < if that neighbour is lower than itself, otherwise it is a PIT; a neighbour in O counts by its
 *     value like any other.  leaf(c) is outside when the path reaches a cell of O.
 *   Edges, keys, Kruskal with the outside as a node, numbering and reductions are unchanged: cells of O are labelled -1
 *     and are charged to no node; an outside_cell may be an ocean cell, and then geolink is NONE.
 * O empty is RDGPU_ERR_ARG ("no ocean cells"; the reference throws), found by the first pass, and nothing is written.
 * All cells in O gives count 0, leaves 0 and all labels -1.  The mask is never written. */
typedef struct rdgpu_dephier_node {         /* 56 bytes: eight 32-bit words, three doubles */
  uint32_t parent, lchild, rchild;      /* NONE: root / leaf */
  uint32_t pit_cell;
  uint32_t inside_cell, outside_cell;   /* the spill pair; level = max of their dem values */
  uint32_t geolink;                     /* leaf id of leaf(outside_cell), NONE when that is outside */
  uint32_t cells;
  double level, pit_elevation, volume;
} rdgpu_dephier_node;
#define RDGPU_DEPHIER_NONE 0xFFFFFFFFu
#define RDGPU_DECL_DEPHIER(SUF, T)                                                                                     \
  int rdgpu_depression_hierarchy_##SUF(const T *dem, int width, int height, int topology, int32_t *labels /* nullable */, \
                                       rdgpu_dephier_node *table /* nullable */, uint32_t capacity, uint32_t *count,  \
                                       uint32_t *leaves /* nullable */);                                              \
  int rdgpu_depression_hierarchy_dev_##SUF(const T *d_dem, int width, int height, int topology,                       \
                                           int32_t *d_labels /* nullable */, rdgpu_dephier_node *d_table /* nullable */, \
                                           uint32_t capacity, uint32_t *d_count, uint32_t *d_leaves /* nullable */,   \
                                           void *hip_stream);                                                         \
  int rdgpu_depression_hierarchy_ocean_##SUF(const T *dem, int width, int height, int topology,                       \
                                             const uint8_t *ocean /* nullable: the border ring */,                    \
                                             int32_t *labels /* nullable */, rdgpu_dephier_node *table /* nullable */, \
                                             uint32_t capacity, uint32_t *count, uint32_t *leaves /* nullable */);    \
  int rdgpu_depression_hierarchy_ocean_dev_##SUF(const T *d_dem, int width, int height, int topology,                 \
                                                 const uint8_t *d_ocean /* nullable: the border ring */,              \
                                                 int32_t *d_labels /* nullable */,                                    \
                                                 rdgpu_dephier_node *d_table /* nullable */, uint32_t capacity,       \
                                                 uint32_t *d_count, uint32_t *d_leaves /* nullable */, void *hip_stream);
RDGPU_DECL_DEPHIER(u8, uint8_t)
RDGPU_DECL_DEPHIER(i8, int8_t)
RDGPU_DECL_DEPHIER(i16, int16_t)
RDGPU_DECL_DEPHIER(u16, uint16_t)
RDGPU_DECL_DEPHIER(i32, int32_t)
RDGPU_DECL_DEPHIER(u32, uint32_t)
RDGPU_DECL_DEPHIER(f32, float)
RDGPU_DECL_DEPHIER(f64, double)    /* RDGPU_ERR_UNSUPPORTED */
RDGPU_DECL_DEPHIER(i64, int64_t)   /* RDGPU_ERR_UNSUPPORTED */
RDGPU_DECL_DEPHIER(u64, uint64_t)  /* RDGPU_ERR_UNSUPPORTED */
#undef RDGPU_DECL_DEPHIER
/* of the calling thread's last hierarchy call (zero pits: only pits and jump_rounds are set) */
#define RDGPU_DEPHIER_BUILDER_HOST_KRUSKAL 1u   /* serial Kruskal on the host over the sorted edge records */
typedef struct rdgpu_dephier_stats {
  uint64_t cell_pairs;       /* (higher cell, lower neighbour) pairs across two leaves */
  uint64_t edges_raw;        /* edge records emitted and sorted: one per higher cell and neighbouring leaf */
  uint64_t edges_reduced;    /* after the reduction to the minimum edge per pair of leaves: what the builder reads */
  uint32_t pits, nodes, roots;
  uint32_t builder;          /* RDGPU_DEPHIER_BUILDER_* */
  uint32_t builder_rounds;   /* passes of the builder over the records (1 for the serial one) */
  uint32_t jump_rounds;      /* pointer-jumping launches of the descent */
  uint32_t height;           /* edges on the longest leaf-to-root path */
  uint32_t lift_planes;      /* planes of the lifting table the charging pass walks */
} rdgpu_dephier_stats;
int rdgpu_dephier_get_stats(rdgpu_dephier_stats *out);

/* ---- bucket fill from the edges: paint a mask over the cells of one value that the border reaches ----
 * Reference: misc/misc_methods.hpp (BucketFillFromEdges<topo>(check, set, check_value, set_value)), with
 * `set == set_value` read as `mask != 0`.  ELIGIBLE = {c : check[c] == check_value under C++ ==, and mask[c] == 0 on
 * entry}: NaN equals nothing, -0.0 equals 0.0.  mask[c] becomes 1 for every eligible cell connected under `topology`
 * (8 or 4), through eligible cells, to an eligible cell of the border ring; every other byte is left as it was.  filled
 * (nullable): the number of bytes set.  The result depends on no order of visits.  The cells are labelled by a union-find
 * in four launches whatever the shape of the region; scratch (4 bytes per cell) comes from the workspace pool under names
 * starting with "bucketfill.".  Every element type is supported (the operation is equality alone).  A null check or
 * mask, a non-positive size, a topology other than 8 or 4 or more than 2^31-65536 cells is RDGPU_ERR_ARG before any
 * device work, and nothing is written then.  check is never written.  The _dev form takes device pointers (d_filled one
 * 64-bit device word) and is ordered on hip_stream without synchronising it. */
#define RDGPU_DECL_BUCKET(SUF, T)                                                                                      \
  int rdgpu_bucket_fill_from_edges_##SUF(const T *check, int width, int height, int topology, T check_value,          \
                                         uint8_t *mask /* in/out */, uint64_t *filled /* nullable */);                \
  int rdgpu_bucket_fill_from_edges_dev_##SUF(const T *d_check, int width, int height, int topology, T check_value,    \
                                             uint8_t *d_mask /* in/out */, uint64_t *d_filled /* nullable */,         \
                                             void *hip_stream);
RDGPU_DECL_BUCKET(u8, uint8_t)
RDGPU_DECL_BUCKET(i8, int8_t)
RDGPU_DECL_BUCKET(i16, int16_t)
RDGPU_DECL_BUCKET(u16, uint16_t)
RDGPU_DECL_BUCKET(i32, int32_t)
RDGPU_DECL_BUCKET(u32, uint32_t)
RDGPU_DECL_BUCKET(f32, float)
RDGPU_DECL_BUCKET(f64, double)
RDGPU_DECL_BUCKET(i64, int64_t)
RDGPU_DECL_BUCKET(u64, uint64_t)
#undef RDGPU_DECL_BUCKET

/* ---- fill-spill-merge: route surface water through the depression hierarchy ----
 * Reference: depressions/fill_spill_merge.hpp (FillSpillMerge) with surface water only; the ocean is the ocean cells of
 * the hierarchy call (the border ring, or the mask given to rdgpu_depression_hierarchy_ocean_<T>).  The reference floods
 * every lake from its pit with a priority queue; this contract states the same result without an order of visits, and
 * the two agree on every cell of tie-free inputs (tests/golden/make_golden_fsm.py).
 *
 * INPUTS.  dem, width, height; labels and table[count]: what rdgpu_depression_hierarchy_<T> gave for this DEM (either
 * topology: nothing below looks at a neighbour); water: one double per cell, finite and >= 0.  Groundwater (a negative
 * value) is out of scope: a negative or non-finite value is RDGPU_ERR_UNSUPPORTED, found by the first pass, before any
 * output is written.  P, the number of leaves, is the number of records without children; they are records 0..P-1.
 *   1. GATHER.  leaf_water(l) = the sum of water[c] over the cells with labels[c] == l; the water of the cells labelled
 *      -1 goes to `ocean`.  Sums in double in no fixed order: |sum - exact| <= cells * 2^-52 * sum.
 *   2. POUR (serial, on the host, over the node table alone).  w(n), one double per node, starts at 0; n is FULL when
 *      w(n) >= volume(n).  For the leaves l = 0..P-1 in ascending id with leaf_water(l) > 0, pour(leaf_water(l), l):
 *        pour(x, n): loop
 *          if w(n) < volume(n): cap = volume(n) - w(n)
 *              if x < cap: w(n) += x; return
 *              w(n) = volume(n); x -= cap
 *          if x <= 0: return
 *          p = parent(n)
 *          if p == NONE: if geolink(n) == NONE: ocean += x; return
 *                        n = geolink(n); continue             (a root: over its spill into the tree beyond, or lost)
 *          s = the other child of p
 *          if s is FULL: if w(p) == 0: w(p) = min(volume(p), volume(lchild(p)) + volume(rchild(p)))
 *                        n = p                                (the two lakes have merged)
 *          else: n = geolink(n)                               (a leaf below s: the spill pair's far side)
 *      w of an internal node is the water of the merged lake, its children's included; it stays 0 until a pour climbs
 *      into the node.  The engine skips runs of full nodes by path compression; the values are those of the loop above.
 *   3. LAKES.  f is a LAKE TOP when w(f) > 0 and parent(f) is NONE or w(parent(f)) == 0.  top(n) is the highest
 *      ancestor-or-self of n that is a lake top, or none; the cells of lake f are those with top(labels[c]) == f.
 *      h(f) = level(f) if f is FULL.  Otherwise sort the lake's cells with dem < level(f) by (dem, raster index), with
 *      1-based positions and prefix sums S_k of their elevations in double: h(f) = (w(f) + S_k) / k for the smallest k
 *      with (w(f) + S_k) / k <= dem of cell k + 1, or k = the last position.
 *   4. DEPTH.  depth[c] = h(f) - dem[c] where c belongs to lake f and dem[c] < h(f); 0 elsewhere, the ocean cells of the
 *      hierarchy call included.
 * OUTPUTS.  depth: one double per cell; it must not overlap water.  node_water (nullable): w, one double per node.
 * result (nullable): water_in (all the water handed in), ocean (what left the raster), standing (the sum of depth), the
 * number of lake tops and how many of them are full.  water_in = standing + ocean within cells * 2^-52 * water_in.
 * With count == 0 depth is all zero and all the water goes to the ocean.
 * ARGUMENTS.  Those of rdgpu_depression_hierarchy_<T>, and: a null labels, water or depth, a null table with count > 0,
 * depth overlapping water, a label outside [-1, P) (found by the gather), a record whose children are not both below it
 * or both NONE, whose parent does not list it as a child, or whose geolink is not a leaf (found by the host pass): all
 * RDGPU_ERR_ARG, and nothing is written.  A table that passes these checks but does not belong to the DEM gives
 * unspecified values, never an out-of-range access.  Element types u8, i8, i16, u16, i32, u32, f32; the f64, i64 and u64
 * entries exist and return RDGPU_ERR_UNSUPPORTED.  Inputs are never written.  The _dev forms take device pointers
 * (d_result: one device struct) and are ordered on hip_stream, which they wait for several times: the pour runs on the
 * host over 24 bytes per node.  Scratch comes from the workspace pool under names starting with "fsm.". */
typedef struct rdgpu_fsm_result {           /* 32 bytes */
  double water_in, ocean, standing;
  uint32_t lakes, full_lakes;
} rdgpu_fsm_result;
#define RDGPU_DECL_FSM(SUF, T)                                                                                         \
  int rdgpu_fill_spill_merge_##SUF(const T *dem, int width, int height, const int32_t *labels,                        \
                                   const rdgpu_dephier_node *table, uint32_t count, const double *water, double *depth, \
                                   double *node_water /* nullable */, rdgpu_fsm_result *result /* nullable */);       \
  int rdgpu_fill_spill_merge_dev_##SUF(const T *d_dem, int width, int height, const int32_t *d_labels,                \
                                       const rdgpu_dephier_node *d_table, uint32_t count, const double *d_water,      \
                                       double *d_depth, double *d_node_water /* nullable */,                          \
                                       rdgpu_fsm_result *d_result /* nullable */, void *hip_stream);
RDGPU_DECL_FSM(u8, uint8_t)
RDGPU_DECL_FSM(i8, int8_t)
RDGPU_DECL_FSM(i16, int16_t)
RDGPU_DECL_FSM(u16, uint16_t)
RDGPU_DECL_FSM(i32, int32_t)
RDGPU_DECL_FSM(u32, uint32_t)
RDGPU_DECL_FSM(f32, float)
RDGPU_DECL_FSM(f64, double)    /* RDGPU_ERR_UNSUPPORTED */
RDGPU_DECL_FSM(i64, int64_t)   /* RDGPU_ERR_UNSUPPORTED */
RDGPU_DECL_FSM(u64, uint64_t)  /* RDGPU_ERR_UNSUPPORTED */
#undef RDGPU_DECL_FSM
/* of the calling thread's last fill-spill-merge call */
typedef struct rdgpu_fsm_stats {            /* 48 bytes */
  uint64_t records;          /* (lake, elevation) records sorted: the cells of the partial lakes below their spill level */
  double host_ms;            /* the host pass: the two transfers, the checks, the pour, the lake tops */
  uint32_t nodes, leaves;
  uint32_t lakes, partial_lakes;
  uint32_t pours;            /* leaves with water */
  uint32_t longest_pour;     /* node-to-node hops of the longest pour, a shortcut counting as one */
  uint32_t shortcut_hits;    /* hops taken over the path-compression table */
  uint32_t sort_bits;        /* key bits the radix sort ran over */
} rdgpu_fsm_stats;
int rdgpu_fsm_get_stats(rdgpu_fsm_stats *out);

/* ---- flow distance and drop (HAND) DOWN to the stop cells over D-infinity / MFD proportions ----
 * No reference counterpart (TauDEM's DinfDistDown is the product meant).  Proportions are the reference's nine floats
 * per cell, [height][width][9]: slot 0 is -2 for NoData, slots 1..8 the shares to the neighbours 1 left, 2 up-left,
 * 3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left.
 *   THE GRAPH is the generic accumulation's: the RECEIVERS R(c) of a data cell c are the neighbours n with
 *   props(c, n) > 0 that lie inside the raster and are not NoData.  A cell on the raster's edge has R(c) empty.  A share
 *   into NoData is dropped; it is not an error.
 *   A STOP CELL is, with chan given (uint8 mask), a data cell with chan != 0; with chan == NULL a data cell with R(c)
 *   empty.
 *   Every data cell ends in one of three states.  RESOLVED: a stop cell, with value 0; and a non-stop cell with R(c) not
 *   empty, once every cell of R(c) is decided, if under strict != 0 every receiver is RESOLVED, under strict == 0 at
 *   least one is.  DEAD: a non-stop cell with R(c) empty (only with chan given), and a non-stop cell whose receivers are
 *   all decided and that does not meet the condition above.  UNDECIDED: a cell on a cycle of positive shares, or one that
 *   depends on such a cell.  A stop cell on a cycle is RESOLVED and breaks the cycle for its donors.
 *   The CONTRIBUTING receivers of c are the RESOLVED members of R(c) (under strict != 0: all of R(c)).
 * Outputs, both float64 [height][width], each a nullable pointer (a call must request at least one):
 *   dist   the increment towards receiver n is len(n) = |cell_x| for n in {1, 5}, |cell_y| for n in {3, 7}, diag
 *          otherwise; diag = sqrt(cell_x * cell_x + cell_y * cell_y) computed once on the host.
 *   drop   the increment is (double)z(c) - (double)z(n); it needs the elevations.  Not clamped: an unfilled DEM gives
 *          negative values.
 * Per contributing receiver n, v_n = Q(n) + inc(c, n): one double addition (for drop, the one subtraction first).  stat
 * combines them:
 *   stat == 1   Q(c) = min v_n;   stat == 2   Q(c) = max v_n   (taken over n = 1..8 in that order with < and >);
 *   stat == 0   with exactly one contributing receiver Q(c) = v_n, no multiply and no divide; otherwise
 *               num = sum (double)p_n * v_n, den = sum (double)p_n, both over n = 1..8 in that order starting from 0.0,
 *               every product and every sum rounded on its own (no fused multiply-add), Q(c) = num / den.
 * DEAD, undecided and NoData cells get out_nodata.  Both outputs are functions of the inputs alone: every value is
 * computed once, from final operands in a fixed order, so they are reproducible bit for bit.  With chan == NULL no cell
 * is DEAD and strict makes no difference.
 * cell_x and cell_y: their sign is ignored; zero or not finite is RDGPU_ERR_ARG.  A null props9 (dem), no output
 * requested, drop without elev, stat outside 0..2, a non-positive size or more than 0xFFFF0000 cells returns
 * RDGPU_ERR_ARG before any device work; nothing is written then.  Inputs are never written.  The _dev forms take device
 * pointers and are ordered on hip_stream without synchronising it.
 * rdgpu_dinf_distance_down_<T> takes a DEM: the proportions are FM_Tarboton's in compact form (5 bytes per cell, the
 * array is never materialised) and the elevations are the DEM's.  T: u8 i8 i16 u16 i32 u32 f32 f64.
 * rdgpu_dinf_distance_down_flats_<T> is the same over the proportions of rdgpu_fm_tarboton_flats_<T> ("D-infinity across
 * flats" above): same arguments, same statistics, same strict rule; at most 0x7FFF0000 cells.
 * rdgpu_mfd_distance_rounds: the work-list launches of the last call.  RDGPU_MFD_DISTANCE_STACK_BELOW: lists shorter
 * than this many cells run in the kernel that keeps its by-products on a per-wavefront stack (default 4194304; 0: never).
 * Scratch (13 bytes per cell, shared with the accumulation; 8 more for drop from a DEM that is not float64) comes from
 * the workspace pool. */
int rdgpu_mfd_distance_down(const float *props9, int width, int height, const uint8_t *chan /* nullable */,
                            const double *elev /* nullable; required iff drop */, int stat, int strict, double cell_x,
                            double cell_y, double *dist /* nullable */, double *drop /* nullable */, double out_nodata);
int rdgpu_mfd_distance_down_dev(const float *d_props9, int width, int height, const uint8_t *d_chan /* nullable */,
                                const double *d_elev /* nullable; required iff drop */, int stat, int strict, double cell_x,
                                double cell_y, double *d_dist /* nullable */, double *d_drop /* nullable */,
                                double out_nodata, void *hip_stream);
int rdgpu_mfd_distance_rounds(uint32_t *rounds);
#define RDGPU_DECL_DINF_DIST(FL, SUF, T)                                                                                  \
  int rdgpu_dinf_distance_down##FL##_##SUF(const T *dem, T nodata, int width, int height, const uint8_t *chan /* nullable */, \
                                     int stat, int strict, double cell_x, double cell_y, double *dist /* nullable */,     \
                                     double *drop /* nullable */, double out_nodata);                                     \
  int rdgpu_dinf_distance_down##FL##_dev_##SUF(const T *d_dem, T nodata, int width, int height,                           \
                                         const uint8_t *d_chan /* nullable */, int stat, int strict, double cell_x,       \
                                         double cell_y, double *d_dist /* nullable */, double *d_drop /* nullable */,     \
                                         double out_nodata, void *hip_stream);
RDGPU_DECL_DINF_DIST(, u8, uint8_t) RDGPU_DECL_DINF_DIST(_flats, u8, uint8_t)
RDGPU_DECL_DINF_DIST(, i16, int16_t) RDGPU_DECL_DINF_DIST(_flats, i16, int16_t)
RDGPU_DECL_DINF_DIST(, u16, uint16_t) RDGPU_DECL_DINF_DIST(_flats, u16, uint16_t)
RDGPU_DECL_DINF_DIST(, i32, int32_t) RDGPU_DECL_DINF_DIST(_flats, i32, int32_t)
RDGPU_DECL_DINF_DIST(, u32, uint32_t) RDGPU_DECL_DINF_DIST(_flats, u32, uint32_t)
RDGPU_DECL_DINF_DIST(, f32, float) RDGPU_DECL_DINF_DIST(_flats, f32, float)
RDGPU_DECL_DINF_DIST(, f64, double) RDGPU_DECL_DINF_DIST(_flats, f64, double)
RDGPU_DECL_DINF_DIST(, i8, int8_t) RDGPU_DECL_DINF_DIST(_flats, i8, int8_t)
#undef RDGPU_DECL_DINF_DIST

/* ---- flow distance and rise UP to the sources (the ridge) over D-infinity / MFD proportions ----
 * No reference counterpart (TauDEM's DinfDistUp is the product meant).  Proportions and neighbour numbering as in the
 * block above.
 *   THE GRAPH is the generic accumulation's with a share threshold.  min_share is a float, min_share >= 0, compared in
 *   float32.  A LINK d -> c exists when d is a data cell that is not on the raster's edge, c is the neighbour n of d, c
 *   lies inside the raster and is a data cell, and props(d, n) > min_share.  min_share = 0 is the accumulation's graph;
 *   this is TauDEM's "proportion threshold", whose default there is 0.5.  A share into NoData or out of the raster is
 *   dropped; it is not an error.
 *   The DONORS D(c) of a data cell c are the cells with a link into c.  Cells on the raster's edge have donors but are
 *   never donors.  A SOURCE is a data cell with D(c) empty; its values are 0.  A cell with donors is decided once all its
 *   donors are decided.  A cell on a cycle of links, or downstream of one, stays UNDECIDED; nothing waits for it.
 * Outputs, both float64 [height][width], each a nullable pointer (a call must request at least one):
 *   dist   the increment over the link d -> c is the length of that step: |cell_x| for a link along x (n in {1, 5}),
 *          |cell_y| for a link along y (n in {3, 7}), diag otherwise; diag = sqrt(cell_x * cell_x + cell_y * cell_y)
 *          computed once on the host.
 *   rise   the increment is (double)z(d) - (double)z(c); it needs the elevations.  Not clamped.
 * Per donor d, v_d = Q(d) + inc: one double addition (for rise, the one subtraction first).  The donors are taken in the
 * order of their position m = 1..8 around c (d is the neighbour m of c).  stat combines them:
 *   stat == 1   Q(c) = min v_d, with <;   stat == 2   Q(c) = max v_d, with >;
 *   stat == 0   with exactly one donor Q(c) = v_d, no multiply and no divide; otherwise num = sum (double)p * v_d and
 *               den = sum (double)p, p the share of the link d -> c, both over m = 1..8 in that order starting from 0.0,
 *               every product and every sum rounded on its own (no fused multiply-add), Q(c) = num / den.
 * Undecided and NoData cells get out_nodata.  Both outputs are functions of the inputs alone: every value is computed
 * once, from final operands in a fixed order, so they are reproducible bit for bit.
 * cell_x and cell_y: their sign is ignored; zero or not finite is RDGPU_ERR_ARG.  A negative or non-finite min_share, a
 * null props9 (dem), no output requested, rise without elev, stat outside 0..2, a non-positive size or more than
 * 0xFFFF0000 cells returns RDGPU_ERR_ARG before any device work; nothing is written then.  Inputs are never written.
 * The _dev forms take device pointers and are ordered on hip_stream without synchronising it.
 * rdgpu_dinf_distance_up_<T> takes a DEM: the proportions are FM_Tarboton's in compact form and the elevations are the
 * DEM's.  T: u8 i8 i16 u16 i32 u32 f32 f64.  rdgpu_dinf_distance_up_flats_<T> is the same over the proportions of
 * rdgpu_fm_tarboton_flats_<T>; at most 0x7FFF0000 cells.
 * rdgpu_mfd_distance_rounds reports the work-list launches of the last call of either direction, and
 * RDGPU_MFD_DISTANCE_STACK_BELOW is read by both.  Scratch as for the down entries. */
int rdgpu_mfd_distance_up(const float *props9, int width, int height, const double *elev /* nullable; required iff rise */,
                          int stat, float min_share, double cell_x, double cell_y, double *dist /* nullable */,
                          double *rise /* nullable */, double out_nodata);
int rdgpu_mfd_distance_up_dev(const float *d_props9, int width, int height,
                              const double *d_elev /* nullable; required iff rise */, int stat, float min_share,
                              double cell_x, double cell_y, double *d_dist /* nullable */, double *d_rise /* nullable */,
                              double out_nodata, void *hip_stream);
#define RDGPU_DECL_DINF_DISTUP(FL, SUF, T)                                                                                \
  int rdgpu_dinf_distance_up##FL##_##SUF(const T *dem, T nodata, int width, int height, int stat, float min_share,        \
                                         double cell_x, double cell_y, double *dist /* nullable */,                       \
                                         double *rise /* nullable */, double out_nodata);                                 \
  int rdgpu_dinf_distance_up##FL##_dev_##SUF(const T *d_dem, T nodata, int width, int height, int stat, float min_share,  \
                                             double cell_x, double cell_y, double *d_dist /* nullable */,                 \
                                             double *d_rise /* nullable */, double out_nodata, void *hip_stream);
RDGPU_DECL_DINF_DISTUP(, u8, uint8_t) RDGPU_DECL_DINF_DISTUP(_flats, u8, uint8_t)
RDGPU_DECL_DINF_DISTUP(, i16, int16_t) RDGPU_DECL_DINF_DISTUP(_flats, i16, int16_t)
RDGPU_DECL_DINF_DISTUP(, u16, uint16_t) RDGPU_DECL_DINF_DISTUP(_flats, u16, uint16_t)
RDGPU_DECL_DINF_DISTUP(, i32, int32_t) RDGPU_DECL_DINF_DISTUP(_flats, i32, int32_t)
RDGPU_DECL_DINF_DISTUP(, u32, uint32_t) RDGPU_DECL_DINF_DISTUP(_flats, u32, uint32_t)
RDGPU_DECL_DINF_DISTUP(, f32, float) RDGPU_DECL_DINF_DISTUP(_flats, f32, float)
RDGPU_DECL_DINF_DISTUP(, f64, double) RDGPU_DECL_DINF_DISTUP(_flats, f64, double)
RDGPU_DECL_DINF_DISTUP(, i8, int8_t) RDGPU_DECL_DINF_DISTUP(_flats, i8, int8_t)
#undef RDGPU_DECL_DINF_DISTUP

/* ---- reverse accumulation, largest weight downslope and upslope dependence over D-infinity / MFD proportions ----
 * No reference counterpart (TauDEM's DinfRevAccum with its dmax, and DinfUpDependence, are the products meant): a
 * quantity summed or maximised over everything that lies DOWNSLOPE of a cell, weighted by the shares -- the transpose of
 * the accumulation.  Proportions, neighbour numbering 1..8 and the graph are those of "flow distance and drop DOWN"
 * above: the RECEIVERS R(c) of a data cell c are the neighbours n with props(c, n) > 0 that lie inside the raster and
 * are data cells.  A cell on the raster's edge has R(c) empty.  A share into NoData is dropped.
 * Inputs:
 *   dest      uint8 mask, nullable.  A data cell with dest != 0 is ABSORBING: its R(c) is taken as empty, what lies
 *             below it does not count, and it is never a donor for the counters.
 *   weights   float64 raster, nullable.  With a raster given, a data cell CONTRIBUTES iff its weight is not
 *             weight_nodata and is not a NaN (the compare is == on doubles, so -0.0 equals a NoData of 0.0; pass a NaN
 *             for "no NoData value": rdgpu_d8_flow_accum_weighted's convention).  With weights == NULL, dest is
 *             required, the weight is 1.0 on absorbing cells and 0.0 elsewhere, and every data cell contributes: the
 *             upslope dependence, the fraction of a cell's flow that reaches the destination set.  A cell that does not
 *             contribute still passes on what lies below it.
 * A cell is DECIDED once every member of R(c) is decided; the thread that decides it computes both planes once, from
 * final operands, in the fixed order n = 1..8.  A cell on a cycle of positive shares, or one that depends on such a cell,
 * stays UNDECIDED; nothing waits for it.  An absorbing cell on a cycle is decided and breaks the cycle.
 * Outputs, both float64 [height][width], each a nullable pointer (a call must request at least one):
 *   racc   S = w(c) if c contributes, else +0.0; then, for n = 1..8 in that order and each receiver,
 *          S = S + (double)p_n * racc(n), every product and every sum rounded on its own (no fused multiply-add).
 *          Infinities are added as IEEE adds them.  With shares that sum to 1 and a per-cell travel time as the weight
 *          this is the expected travel time to the outlet (with dest given: to the absorbing cells).
 *   wmax   (needs weights) the largest contributing weight at c or at any cell reachable from c over receivers, stopping
 *          at absorbing cells: start with w(c) if c contributes; then, for n = 1..8 in that order, take wmax(n) of every
 *          receiver that HAS a maximum when c has none yet or when it is > the current one.  A decided cell with no
 *          contributing weight at or below it has no maximum: it gets out_nodata in wmax, while its racc is a plain sum
 *          (0.0 if nothing contributes).
 * Undecided and NoData cells get out_nodata in both planes.  Both planes are functions of the inputs alone and are
 * reproducible bit for bit.
 * A null props9 (dem), no output requested, wmax without weights, neither weights nor dest, a non-positive size or more
 * than 0xFFFF0000 cells (0x7FFF0000 for the _flats forms) returns RDGPU_ERR_ARG before any device work; nothing is
 * written then.  Inputs are never written.  The _dev forms take device pointers and are ordered on hip_stream without
 * synchronising it.
 * rdgpu_dinf_reverse_accum_<T> takes a DEM: the proportions are FM_Tarboton's in compact form (5 bytes per cell, the
 * array is never materialised).  T: u8 i8 i16 u16 i32 u32 f32 f64.  rdgpu_dinf_reverse_accum_flats_<T> is the same over
 * the proportions of rdgpu_fm_tarboton_flats_<T>.
 * rdgpu_mfd_distance_rounds reports the work-list launches of the last call of these or of either distance engine, and
 * RDGPU_MFD_DISTANCE_STACK_BELOW is read here too.  Scratch: the accumulation's 13 bytes per cell, from the workspace
 * pool. */
int rdgpu_mfd_reverse_accum(const float *props9, int width, int height, const double *weights /* nullable */,
                            double weight_nodata, const uint8_t *dest /* nullable */, double *racc /* nullable */,
                            double *wmax /* nullable */, double out_nodata);
int rdgpu_mfd_reverse_accum_dev(const float *d_props9, int width, int height, const double *d_weights /* nullable */,
                                double weight_nodata, const uint8_t *d_dest /* nullable */, double *d_racc /* nullable */,
                                double *d_wmax /* nullable */, double out_nodata, void *hip_stream);
#define RDGPU_DECL_DINF_REV(FL, SUF, T)                                                                                   \
  int rdgpu_dinf_reverse_accum##FL##_##SUF(const T *dem, T nodata, int width, int height,                                 \
                                           const double *weights /* nullable */, double weight_nodata,                   \
                                           const uint8_t *dest /* nullable */, double *racc /* nullable */,               \
                                           double *wmax /* nullable */, double out_nodata);                               \
  int rdgpu_dinf_reverse_accum##FL##_dev_##SUF(const T *d_dem, T nodata, int width, int height,                           \
                                               const double *d_weights /* nullable */, double weight_nodata,             \
                                               const uint8_t *d_dest /* nullable */, double *d_racc /* nullable */,       \
                                               double *d_wmax /* nullable */, double out_nodata, void *hip_stream);
RDGPU_DECL_DINF_REV(, u8, uint8_t) RDGPU_DECL_DINF_REV(_flats, u8, uint8_t)
RDGPU_DECL_DINF_REV(, i16, int16_t) RDGPU_DECL_DINF_REV(_flats, i16, int16_t)
RDGPU_DECL_DINF_REV(, u16, uint16_t) RDGPU_DECL_DINF_REV(_flats, u16, uint16_t)
RDGPU_DECL_DINF_REV(, i32, int32_t) RDGPU_DECL_DINF_REV(_flats, i32, int32_t)
RDGPU_DECL_DINF_REV(, u32, uint32_t) RDGPU_DECL_DINF_REV(_flats, u32, uint32_t)
RDGPU_DECL_DINF_REV(, f32, float) RDGPU_DECL_DINF_REV(_flats, f32, float)
RDGPU_DECL_DINF_REV(, f64, double) RDGPU_DECL_DINF_REV(_flats, f64, double)
RDGPU_DECL_DINF_REV(, i8, int8_t) RDGPU_DECL_DINF_REV(_flats, i8, int8_t)
#undef RDGPU_DECL_DINF_REV

/* ---- synthetic input (test/bench input generator) ----------- */
int rdgpu_synth_dem_dev_f32(float *d_dem, int width, int height, int seed, int x0, int y0,
                            float tilt, void *hip_stream);

/* ---- per-kernel timing (HIP events on the launch stream) -----------------------------------
 * rdgpu_profile_enable(1) makes every kernel launch be bracketed by hipEvents on the stream it
 * is launched on.  rdgpu_profile_collect() synchronises and folds the pending event pairs into
 * per-kernel totals.  rdgpu_profile_get() reads one kernel's totals; rdgpu_profile_name(i)
 * enumerates kernel names (NULL past the end).  rdgpu_profile_reset() clears totals. */
int rdgpu_profile_enable(int on);
int rdgpu_profile_collect(void);
int rdgpu_profile_reset(void);
const char *rdgpu_profile_name(int index);
int rdgpu_profile_get(const char *kernel, double *total_ms, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* RDGPU_H_ */
