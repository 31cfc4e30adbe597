// rdgpu/richdem_gpu.hpp -- C++ shim: the reference's function names and Array2D<T> signatures over
// the C-ABI of librdgpu.so (include/rdgpu.h).  Host code stays C++; HIP lives only behind the C-ABI.
//
// Every function is templated on the ARRAY type, so the same shim binds to
//   * richdem::Array2D<T>  -- inside the reference tree (apps/rd_depressions_flood.cpp,
//                             apps/rd_flow_accumulation.cpp, apps/rd_d8_flowdirs.cpp compile unchanged
//                             apart from the namespace of the call), and
//   * rdgpu::Array2D<T>    -- the stand-alone container in rdgpu/Array2D.hpp.
// Required of the array type: data(), width(), height(), noData(), setNoData(), resize(other, val),
// templateCopy(other) -- all present in the reference's Array2D (common/Array2D.hpp).
//
// Contracts kept from the reference:
//   * all functions are void, modify / size their outputs exactly as the reference does, and report
//     failure by throwing std::runtime_error (the C-ABI's non-zero codes are converted here);
//   * the DEM buffer is never freed or reallocated: results are copied back into data();
//   * works for owning and for wrapping (externally owned) arrays.
#pragma once

#include <cstdint>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../rdgpu.h"

namespace rdgpu {
namespace detail {

inline void check(int rc, const char *what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + rdgpu_last_error());
}

template <class A>
using elem_t = typename std::remove_cv<typename std::remove_pointer<decltype(std::declval<A &>().data())>::type>::type;

[[noreturn]] inline void unsupported(const char *fn) {
  throw std::runtime_error(std::string(fn) + ": element type not supported by the MI355X engine");
}

// ---- overload sets: element type -> C-ABI entry point ---------------------------------------
#define RDGPU_SHIM_ELEV(SUF, T)                                                                            \
  inline int c_fill(T *p, int w, int h, int t) { return rdgpu_fill_##SUF(p, w, h, t); }
RDGPU_SHIM_ELEV(u8, uint8_t)
RDGPU_SHIM_ELEV(i16, int16_t)
RDGPU_SHIM_ELEV(u16, uint16_t)
RDGPU_SHIM_ELEV(i32, int32_t)
RDGPU_SHIM_ELEV(u32, uint32_t)
RDGPU_SHIM_ELEV(f32, float)
RDGPU_SHIM_ELEV(f64, double)
RDGPU_SHIM_ELEV(i64, int64_t)
RDGPU_SHIM_ELEV(u64, uint64_t)
RDGPU_SHIM_ELEV(i8, int8_t)
#undef RDGPU_SHIM_ELEV
template <class T>
int c_fill(T *, int, int, int) { unsupported("FillDepressions"); }

#define RDGPU_SHIM_STENCIL(SUF, T)                                                                         \
  inline int c_flowdirs(const T *p, T nd, int w, int h, uint8_t *o) { return rdgpu_d8_flowdirs_##SUF(p, nd, w, h, o); } \
  inline int c_flatres(const T *p, T nd, int w, int h, uint8_t *o) { return rdgpu_flat_resolution_d8_##SUF(p, nd, w, h, o); } \
  inline int c_fa_d8(const T *p, T nd, int w, int h, double *a) { return rdgpu_fa_d8_##SUF(p, nd, w, h, a); } \
  inline int c_fa_d8_unit(const T *p, T nd, int w, int h, double *a) { return rdgpu_fa_d8_unit_##SUF(p, nd, w, h, a); } \
  inline int c_fa_dinf(const T *p, T nd, int w, int h, double *a) { return rdgpu_fa_tarboton_##SUF(p, nd, w, h, a); } \
  inline int c_fa_mfd(const T *p, T nd, int w, int h, int m, double x, double *a) { return rdgpu_fa_mfd_##SUF(p, nd, w, h, m, x, a); } \
  inline int c_rfe(T *p, T nd, int w, int h) { return rdgpu_resolve_flats_epsilon_##SUF(p, nd, w, h); } \
  inline int c_dinf(const T *p, T nd, int w, int h, float *o) { return rdgpu_dinf_flowdirs_##SUF(p, nd, w, h, o); } \
  inline int c_fm_d8(const T *p, T nd, int w, int h, float *o) { return rdgpu_fm_d8_##SUF(p, nd, w, h, o); } \
  inline int c_fm_dinf(const T *p, T nd, int w, int h, float *o) { return rdgpu_fm_tarboton_##SUF(p, nd, w, h, o); } \
  inline int c_fm_mfd(const T *p, T nd, int w, int h, int m, double x, float *o) { return rdgpu_fm_mfd_##SUF(p, nd, w, h, m, x, o); }
RDGPU_SHIM_STENCIL(u8, uint8_t)
RDGPU_SHIM_STENCIL(i16, int16_t)
RDGPU_SHIM_STENCIL(u16, uint16_t)
RDGPU_SHIM_STENCIL(i32, int32_t)
RDGPU_SHIM_STENCIL(u32, uint32_t)
RDGPU_SHIM_STENCIL(f32, float)
RDGPU_SHIM_STENCIL(f64, double)
RDGPU_SHIM_STENCIL(i8, int8_t)
#undef RDGPU_SHIM_STENCIL
#define RDGPU_SHIM_STENCIL64(SUF, T)                                                                       \
  inline int c_flowdirs(const T *p, T nd, int w, int h, uint8_t *o) { return rdgpu_d8_flowdirs_##SUF(p, nd, w, h, o); } \
  inline int c_flatres(const T *p, T nd, int w, int h, uint8_t *o) { return rdgpu_flat_resolution_d8_##SUF(p, nd, w, h, o); } \
  inline int c_fa_d8(const T *p, T nd, int w, int h, double *a) { return rdgpu_fa_d8_##SUF(p, nd, w, h, a); } \
  inline int c_fa_d8_unit(const T *p, T nd, int w, int h, double *a) { return rdgpu_fa_d8_unit_##SUF(p, nd, w, h, a); } \
  inline int c_rfe(T *p, T nd, int w, int h) { return rdgpu_resolve_flats_epsilon_##SUF(p, nd, w, h); } \
  inline int c_fm_d8(const T *p, T nd, int w, int h, float *o) { return rdgpu_fm_d8_##SUF(p, nd, w, h, o); }
RDGPU_SHIM_STENCIL64(i64, int64_t)
RDGPU_SHIM_STENCIL64(u64, uint64_t)
#undef RDGPU_SHIM_STENCIL64
// D-infinity across flats (rdgpu.h "D-infinity across flats"): the D-infinity family's eight element types
#define RDGPU_SHIM_DINF_FLATS(SUF, T)                                                                      \
  inline int c_fm_dinf_flats(const T *p, T nd, int w, int h, float *o) { return rdgpu_fm_tarboton_flats_##SUF(p, nd, w, h, o); } \
  inline int c_fa_dinf_flats(const T *p, T nd, int w, int h, double *a) { return rdgpu_fa_tarboton_flats_##SUF(p, nd, w, h, a); }
RDGPU_SHIM_DINF_FLATS(u8, uint8_t) RDGPU_SHIM_DINF_FLATS(i8, int8_t) RDGPU_SHIM_DINF_FLATS(u16, uint16_t)
RDGPU_SHIM_DINF_FLATS(i16, int16_t) RDGPU_SHIM_DINF_FLATS(u32, uint32_t) RDGPU_SHIM_DINF_FLATS(i32, int32_t)
RDGPU_SHIM_DINF_FLATS(f32, float) RDGPU_SHIM_DINF_FLATS(f64, double)
#undef RDGPU_SHIM_DINF_FLATS
template <class T>
int c_fm_dinf_flats(const T *, T, int, int, float *) { unsupported("FM_Tarboton_flats"); }
template <class T>
int c_fa_dinf_flats(const T *, T, int, int, double *) { unsupported("FA_Tarboton_flats"); }
template <class T>
int c_flowdirs(const T *, T, int, int, uint8_t *) { unsupported("d8_flow_directions"); }
template <class T>
int c_flatres(const T *, T, int, int, uint8_t *) { unsupported("barnes_flat_resolution_d8"); }
template <class T>
int c_fa_d8(const T *, T, int, int, double *) { unsupported("FA_D8"); }
template <class T>
int c_fa_d8_unit(const T *, T, int, int, double *) { unsupported("FA_D8"); }
template <class T>
int c_fa_dinf(const T *, T, int, int, double *) { unsupported("FA_Tarboton"); }
template <class T>
int c_dinf(const T *, T, int, int, float *) { unsupported("dinf_flow_directions"); }
template <class T>
int c_fa_mfd(const T *, T, int, int, int, double, double *) { unsupported("FA_Holmgren / FA_Freeman / FA_Quinn / FA_D4"); }
template <class T>
int c_rfe(T *, T, int, int) { unsupported("ResolveFlatsEpsilon"); }
template <class T>
int c_fm_d8(const T *, T, int, int, float *) { unsupported("FM_D8"); }
template <class T>
int c_fm_dinf(const T *, T, int, int, float *) { unsupported("FM_Tarboton"); }
template <class T>
int c_fm_mfd(const T *, T, int, int, int, double, float *) { unsupported("FM_Holmgren / FM_Freeman / FM_Quinn / FM_D4"); }

#define RDGPU_SHIM_VARIANTS(SUF, T)                                                                          \
  inline int c_hasdep(const T *p, int w, int h, int t, int *o) { return rdgpu_has_depressions_##SUF(p, w, h, t, o); } \
  inline int c_fill_wei(T *p, T nd, int w, int h) { return rdgpu_fill_wei2018_##SUF(p, nd, w, h); }
RDGPU_SHIM_VARIANTS(u8, uint8_t) RDGPU_SHIM_VARIANTS(i8, int8_t) RDGPU_SHIM_VARIANTS(i16, int16_t)
RDGPU_SHIM_VARIANTS(u16, uint16_t) RDGPU_SHIM_VARIANTS(i32, int32_t) RDGPU_SHIM_VARIANTS(u32, uint32_t)
RDGPU_SHIM_VARIANTS(f32, float) RDGPU_SHIM_VARIANTS(f64, double) RDGPU_SHIM_VARIANTS(i64, int64_t)
RDGPU_SHIM_VARIANTS(u64, uint64_t)
#undef RDGPU_SHIM_VARIANTS
template <class T>
int c_hasdep(const T *, int, int, int, int *) { unsupported("HasDepressions"); }
template <class T>
int c_fill_wei(T *, T, int, int) { unsupported("PriorityFlood_Wei2018"); }

#define RDGPU_SHIM_PITMASK(SUF, T) \
  inline int c_pitmask(const T *p, T nd, int w, int h, int topo, uint8_t *m) { return rdgpu_pit_mask_##SUF(p, nd, w, h, topo, m); }
RDGPU_SHIM_PITMASK(u8, uint8_t)
RDGPU_SHIM_PITMASK(i16, int16_t)
RDGPU_SHIM_PITMASK(u16, uint16_t)
RDGPU_SHIM_PITMASK(i32, int32_t)
RDGPU_SHIM_PITMASK(u32, uint32_t)
RDGPU_SHIM_PITMASK(f32, float)
RDGPU_SHIM_PITMASK(i8, int8_t)
RDGPU_SHIM_PITMASK(f64, double)
RDGPU_SHIM_PITMASK(i64, int64_t)
RDGPU_SHIM_PITMASK(u64, uint64_t)
#undef RDGPU_SHIM_PITMASK
template <class T>
int c_pitmask(const T *, T, int, int, int, uint8_t *) { unsupported("pit_mask"); }

#define RDGPU_SHIM_MAXDEP(SUF, T) \
  inline int c_fill_maxdep(T *p, int w, int h, int t, uint64_t m) { return rdgpu_fill_max_dep_##SUF(p, w, h, t, m); }
RDGPU_SHIM_MAXDEP(u8, uint8_t)
RDGPU_SHIM_MAXDEP(i16, int16_t)
RDGPU_SHIM_MAXDEP(u16, uint16_t)
RDGPU_SHIM_MAXDEP(i32, int32_t)
RDGPU_SHIM_MAXDEP(u32, uint32_t)
RDGPU_SHIM_MAXDEP(f32, float)
RDGPU_SHIM_MAXDEP(i8, int8_t)
RDGPU_SHIM_MAXDEP(f64, double)
RDGPU_SHIM_MAXDEP(i64, int64_t)
RDGPU_SHIM_MAXDEP(u64, uint64_t)
#undef RDGPU_SHIM_MAXDEP
template <class T>
int c_fill_maxdep(T *, int, int, int, uint64_t) { unsupported("PriorityFlood_Barnes2014_max_dep"); }

#define RDGPU_SHIM_WS(SUF, T) \
  inline int c_watersheds(T *p, T nd, int w, int h, int t, int alter, int32_t *l) { return rdgpu_watersheds_##SUF(p, nd, w, h, t, alter, l); }
RDGPU_SHIM_WS(u8, uint8_t)
RDGPU_SHIM_WS(i16, int16_t)
RDGPU_SHIM_WS(u16, uint16_t)
RDGPU_SHIM_WS(i32, int32_t)
RDGPU_SHIM_WS(u32, uint32_t)
RDGPU_SHIM_WS(f32, float)
RDGPU_SHIM_WS(i8, int8_t)
RDGPU_SHIM_WS(f64, double)
RDGPU_SHIM_WS(i64, int64_t)
RDGPU_SHIM_WS(u64, uint64_t)
#undef RDGPU_SHIM_WS
template <class T>
int c_watersheds(T *, T, int, int, int, int, int32_t *) { unsupported("PriorityFloodWatersheds_Barnes2014"); }

#define RDGPU_SHIM_PFD(SUF, T) \
  inline int c_pf_flowdirs(const T *p, T nd, int w, int h, uint8_t *o) { return rdgpu_pf_flowdirs_##SUF(p, nd, w, h, o); }
RDGPU_SHIM_PFD(u8, uint8_t) RDGPU_SHIM_PFD(i8, int8_t) RDGPU_SHIM_PFD(i16, int16_t) RDGPU_SHIM_PFD(u16, uint16_t)
RDGPU_SHIM_PFD(i32, int32_t) RDGPU_SHIM_PFD(u32, uint32_t) RDGPU_SHIM_PFD(f32, float)
RDGPU_SHIM_PFD(f64, double) RDGPU_SHIM_PFD(i64, int64_t) RDGPU_SHIM_PFD(u64, uint64_t)
#undef RDGPU_SHIM_PFD
template <class T>
int c_pf_flowdirs(const T *, T, int, int, uint8_t *) { unsupported("PriorityFloodFlowdirs_Barnes2014"); }

inline int c_fill_eps(float *p, float nd, int w, int h, int t) { return rdgpu_fill_epsilon_f32(p, nd, w, h, t); }
inline int c_fill_eps(double *p, double nd, int w, int h, int t) { return rdgpu_fill_epsilon_f64(p, nd, w, h, t); }
template <class T>
int c_fill_eps(T *, T, int, int, int) {   // depressions/Barnes2014.hpp:424-451
  throw std::runtime_error("Priority-Flood+Epsilon is only available for floating-point data types!");
}

#define RDGPU_SHIM_ALTER(SUF, T) \
  inline int c_flatres_alter(T *p, T nd, int w, int h, uint8_t *o) { return rdgpu_flat_resolution_d8_alter_##SUF(p, nd, w, h, o); }
RDGPU_SHIM_ALTER(f32, float) RDGPU_SHIM_ALTER(f64, double) RDGPU_SHIM_ALTER(u8, uint8_t) RDGPU_SHIM_ALTER(i8, int8_t)
RDGPU_SHIM_ALTER(i16, int16_t) RDGPU_SHIM_ALTER(u16, uint16_t) RDGPU_SHIM_ALTER(i32, int32_t) RDGPU_SHIM_ALTER(u32, uint32_t)
RDGPU_SHIM_ALTER(i64, int64_t) RDGPU_SHIM_ALTER(u64, uint64_t)
#undef RDGPU_SHIM_ALTER

inline int c_accum(const uint8_t *d, uint8_t nd, int w, int h, int32_t *a) { return rdgpu_d8_flow_accum_i32(d, nd, w, h, a); }
inline int c_accum(const uint8_t *d, uint8_t nd, int w, int h, float *a) { return rdgpu_d8_flow_accum_f32(d, nd, w, h, a); }
inline int c_accum(const uint8_t *d, uint8_t nd, int w, int h, double *a) { return rdgpu_d8_flow_accum_f64(d, nd, w, h, a); }
template <class A>
int c_accum(const uint8_t *, uint8_t, int, int, A *) { unsupported("d8_flow_accum"); }

// Topology enumerators: richdem::Topology and rdgpu::Topology both declare {D8, D4} in this order
// (reference common/constants.hpp:97-100).
template <auto topo>
constexpr int topology_code() {
  static_assert(std::is_enum<decltype(topo)>::value, "topology must be Topology::D8 or Topology::D4");
  return static_cast<int>(topo) == 0 ? 8 : 4;
}

}  // namespace detail

// ---- depressions -------------------------------------------------------------------------------
// richdem::PriorityFlood_Zhou2016(Array2D<T>&)            depressions/Zhou2016.hpp:126-191
template <class A>
void PriorityFlood_Zhou2016(A &dem) {
  detail::check(detail::c_fill(dem.data(), dem.width(), dem.height(), 8), "PriorityFlood_Zhou2016");
}

// richdem::PriorityFlood_Barnes2014<topo>(Array2D<T>&)    depressions/Barnes2014.hpp:230-304
template <auto topo, class A>
void PriorityFlood_Barnes2014(A &dem) {
  detail::check(detail::c_fill(dem.data(), dem.width(), dem.height(), detail::topology_code<topo>()),
                "PriorityFlood_Barnes2014");
}

// richdem::FillDepressions<topo>(Array2D<T>&)             depressions/depressions.hpp:13-21
template <auto topo, class A>
void FillDepressions(A &dem) {
  detail::check(detail::c_fill(dem.data(), dem.width(), dem.height(), detail::topology_code<topo>()), "FillDepressions");
}

// richdem::PriorityFlood_Original<topo>(Array2D<T>&)      depressions/Barnes2014.hpp:136-198: the surface of
// FillDepressions<topo> (every flood of this family returns it, tests/tests.cpp:233-271)
template <auto topo, class A>
void PriorityFlood_Original(A &dem) {
  detail::check(detail::c_fill(dem.data(), dem.width(), dem.height(), detail::topology_code<topo>()), "PriorityFlood_Original");
}

// richdem::PriorityFlood_Wei2018(Array2D<T>&)             depressions/Wei2018.hpp:154-202: D8; NoData cells are left alone
// and the data cells next to them are seeds beside the raster's edge cells (InitPriorityQue, :14-50)
template <class A>
void PriorityFlood_Wei2018(A &dem) {
  using T = detail::elem_t<A>;
  if (dem.width() == 0 || dem.height() == 0) return;
  detail::check(detail::c_fill_wei((T *)dem.data(), dem.noData(), dem.width(), dem.height()), "PriorityFlood_Wei2018");
}

// richdem::HasDepressions<topo>(const Array2D<T>&)        depressions/Barnes2014.hpp:44-103 (apps/rd_depressions_has.cpp:14)
template <auto topo, class A>
bool HasDepressions(const A &elevations) {
  if (elevations.width() == 0 || elevations.height() == 0) return false;   // (an empty queue: "No depressions found.")
  int found = 0;
  detail::check(detail::c_hasdep(elevations.data(), elevations.width(), elevations.height(), detail::topology_code<topo>(), &found),
                "HasDepressions");
  return found != 0;
}

// richdem::PriorityFlood_Barnes2014_max_dep<topo>(Array2D<T>&, uint64_t max_dep_size)   depressions/Barnes2014.hpp:844-931
// (apps/rd_depressions_flood.cpp:16-19): only depressions of at most max_dep_size cells are filled
template <auto topo, class A>
void PriorityFlood_Barnes2014_max_dep(A &dem, uint64_t max_dep_size) {
  using T = detail::elem_t<A>;
  if (dem.width() == 0 || dem.height() == 0) return;
  detail::check(detail::c_fill_maxdep((T *)dem.data(), dem.width(), dem.height(), detail::topology_code<topo>(), max_dep_size),
                "PriorityFlood_Barnes2014_max_dep");
}

// richdem::PriorityFloodWatersheds_Barnes2014<topo>(Array2D<T>&, Array2D<int32_t>&, bool alter_elevations)
// depressions/Barnes2014.hpp:713-807: labels resized to the DEM, NoData -1 (:737-738)
template <auto topo, class A, class L>
void PriorityFloodWatersheds_Barnes2014(A &elevations, L &labels, bool alter_elevations) {
  using T = detail::elem_t<A>;
  static_assert(std::is_same<detail::elem_t<L>, int32_t>::value, "PriorityFloodWatersheds_Barnes2014: labels must be Array2D<int32_t>");
  labels.resize(elevations.width(), elevations.height(), -1);
  labels.setNoData(-1);
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::check(detail::c_watersheds((T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(),
                                     detail::topology_code<topo>(), alter_elevations ? 1 : 0, labels.data()),
                "PriorityFloodWatersheds_Barnes2014");
}

// richdem::PriorityFloodEpsilon_Barnes2014<topo>(Array2D<T>&)   depressions/Barnes2014.hpp:335-420; integer element
// types throw std::runtime_error as the reference's specialisations do (:424-451)
template <auto topo, class A>
void PriorityFloodEpsilon_Barnes2014(A &dem) {
  using T = detail::elem_t<A>;
  if (dem.width() == 0 || dem.height() == 0) return;
  detail::check(detail::c_fill_eps((T *)dem.data(), dem.noData(), dem.width(), dem.height(), detail::topology_code<topo>()),
                "PriorityFloodEpsilon_Barnes2014");
}

// richdem::FillDepressionsEpsilon<topo>(Array2D<T>&)      depressions/depressions.hpp:23
template <auto topo, class A>
void FillDepressionsEpsilon(A &dem) {
  PriorityFloodEpsilon_Barnes2014<topo>(dem);
}

// ---- flow directions ---------------------------------------------------------------------------
namespace detail {
template <class E, class F, class Fn>
void dirs_into(const E &elevations, F &flowdirs, Fn fn, const char *who) {
  using U = elem_t<F>;
  flowdirs.resize(elevations);          // d8_flowdirs.hpp:107
  flowdirs.setNoData((U)255);           // FLOWDIR_NO_DATA, d8_flowdirs.hpp:109
  const int w = elevations.width(), h = elevations.height();
  if (w == 0 || h == 0) return;
  if constexpr (std::is_same<U, uint8_t>::value) {
    check(fn(elevations.data(), elevations.noData(), w, h, flowdirs.data()), who);
  } else {  // the reference allows any integer U: compute in u8, widen
    std::vector<uint8_t> tmp((size_t)w * h);
    check(fn(elevations.data(), elevations.noData(), w, h, tmp.data()), who);
    for (size_t i = 0; i < tmp.size(); i++) flowdirs.data()[i] = (U)tmp[i];
  }
}
}  // namespace detail

// richdem::PriorityFloodFlowdirs_Barnes2014(const Array2D<T>&, Array2D<d8_flowdir_t>&)   depressions/Barnes2014.hpp:483-555
// flowdirs resized to the DEM, NoData = NO_FLOW (0) (:495-496).  Identical to the reference, equal elevations included
// (rdgpu.h; rdgpu_pf_flowdirs_get_stats says how many passes the tie order took).
template <class E, class F>
void PriorityFloodFlowdirs_Barnes2014(const E &elevations, F &flowdirs) {
  static_assert(std::is_same<detail::elem_t<F>, uint8_t>::value, "PriorityFloodFlowdirs_Barnes2014: flowdirs must be Array2D<d8_flowdir_t>");
  flowdirs.resize(elevations.width(), elevations.height());
  flowdirs.setNoData((uint8_t)0);
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::check(detail::c_pf_flowdirs(elevations.data(), elevations.noData(), elevations.width(), elevations.height(), flowdirs.data()),
                "PriorityFloodFlowdirs_Barnes2014");
  rdgpu_pf_flowdirs_stats st;
  if (rdgpu_pf_flowdirs_get_stats(&st) == 0 && st.unresolved != 0)   // (the reference's RDLOG_WARN channel is stderr too)
    std::fprintf(stderr, "W PriorityFloodFlowdirs_Barnes2014: the order of %llu of %u equal-elevation cells had not settled when the "
                         "tie-order passes were stopped (RDGPU_PFD_TIE_PASSES / RDGPU_PFD_TIE_SECONDS); directions are the "
                         "reference's only where those ties do not decide\n", (unsigned long long)st.unresolved, st.twins);
}

// richdem::d8_flow_directions(const Array2D<T>&, Array2D<U>&)   flowmet/d8_flowdirs.hpp:96-123
template <class E, class F>
void d8_flow_directions(const E &elevations, F &flowdirs) {
  using T = detail::elem_t<E>;
  detail::dirs_into(elevations, flowdirs,
                    [](const T *p, T nd, int w, int h, uint8_t *o) { return detail::c_flowdirs(p, nd, w, h, o); },
                    "d8_flow_directions");
}

// richdem::barnes_flat_resolution_d8(Array2D<T>&, Array2D<U>&, bool alter)   flats/flat_resolution.hpp:587-605
template <class E, class F>
void barnes_flat_resolution_d8(E &elevations, F &flowdirs, bool alter) {
  using T = detail::elem_t<E>;
  if (alter) {   // flat_resolution.hpp:597-600: the DEM itself is raised, then plain D8 directions
    using U = detail::elem_t<F>;
    flowdirs.resize(elevations);
    flowdirs.setNoData((U)255);
    if (elevations.width() > 0 && elevations.height() > 0) {
      std::vector<uint8_t> tmp((size_t)elevations.width() * elevations.height());
      detail::check(detail::c_flatres_alter(elevations.data(), elevations.noData(), elevations.width(),
                                            elevations.height(), tmp.data()),
                    "barnes_flat_resolution_d8");
      for (size_t i = 0; i < tmp.size(); i++) flowdirs.data()[i] = (U)tmp[i];
    }
    flowdirs.templateCopy(elevations);
    return;
  }
  detail::dirs_into(elevations, flowdirs,
                    [](const T *p, T nd, int w, int h, uint8_t *o) { return detail::c_flatres(p, nd, w, h, o); },
                    "barnes_flat_resolution_d8");
  flowdirs.templateCopy(elevations);    // flat_resolution.hpp:604
}

// accum_t other than double (the reference's FA_* / FlowAccumulation are templated on it,
// methods/flow_accumulation.hpp:14-28, flow_accumulation_generic.hpp:33-34): the engine accumulates in double; an
// Array2D<float> / Array2D<int32_t> / ... accumulation array is staged through a double copy (weights in, result out,
// converted as a C++ assignment would).  Equal to the reference whenever every partial sum is exactly representable in
// accum_t -- unit or integer-valued weights with totals below 2^24 for float and (because the reference forms
// `float proportion * accum_t` before it adds) for the integer types as well; beyond that the reference's own value is a
// product of float rounding in its queue's order.
namespace detail {
template <class G, class Fn>
void with_double_accum(G &accum, Fn fn) {
  using A = elem_t<G>;
  static_assert(std::is_arithmetic<A>::value, "the accumulation array must hold an arithmetic type");
  if constexpr (std::is_same<A, double>::value) {
    fn(accum.data());
  } else {
    const size_t n = (size_t)accum.width() * (size_t)accum.height();
    std::vector<double> tmp(n);
    for (size_t i = 0; i < n; i++) tmp[i] = (double)accum.data()[i];
    fn(tmp.data());
    for (size_t i = 0; i < n; i++) accum.data()[i] = (A)tmp[i];
  }
}
}  // namespace detail

// ---- accumulation ------------------------------------------------------------------------------
// richdem::d8_flow_accum(const Array2D<T>& flowdirs, Array2D<U>& area)   methods/d8_methods.hpp:47-139
template <class F, class G>
void d8_flow_accum(const F &flowdirs, G &area) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_flow_accum: flow directions must be uint8_t (d8_flowdir_t)");
  using U = detail::elem_t<G>;
  area.resize(flowdirs, (U)0);          // d8_methods.hpp:63
  area.setNoData((U)-1);                // d8_methods.hpp:64
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(detail::c_accum(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), area.data()),
                "d8_flow_accum");
}

// ---- upslope cells, catchments, outlets --------------------------------------------------------
// richdem::d8_upslope_cells(int x0, int y0, int x1, int y1, const Array2D<T>& flowdirs, Array2D<U>& upslope_cells)
// methods/d8_methods.hpp:144-236: 2 on the cells of the reference's line, 1 on every cell that drains through one,
// FLOWDIR_NO_DATA (255, converted to U) elsewhere; the output is resized to the directions and NoData-tagged with it.
// A line that would leave the raster (undefined behaviour in the reference) throws.
template <class F, class G>
void d8_upslope_cells(int x0, int y0, int x1, int y1, const F &flowdirs, G &upslope_cells) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_upslope_cells: flow directions must be uint8_t (d8_flowdir_t)");
  using U = detail::elem_t<G>;
  upslope_cells.resize(flowdirs);
  upslope_cells.setAll((U)255);          // FLOWDIR_NO_DATA, d8_methods.hpp:179
  upslope_cells.setNoData((U)255);       // d8_methods.hpp:180
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  const size_t n = (size_t)flowdirs.width() * (size_t)flowdirs.height();
  if constexpr (std::is_same<U, uint8_t>::value) {
    detail::check(rdgpu_d8_upslope_cells(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), x0, y0, x1, y1,
                                         upslope_cells.data()), "d8_upslope_cells");
  } else {
    std::vector<uint8_t> tmp(n);
    detail::check(rdgpu_d8_upslope_cells(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), x0, y0, x1, y1,
                                         tmp.data()), "d8_upslope_cells");
    for (size_t i = 0; i < n; i++) upslope_cells.data()[i] = (U)tmp[i];
  }
}

// every cell <- the label of the first seed on its flow path (cells: flat indices y * width + x), `unreached` without one
template <class F, class G>
void d8_catchments(const F &flowdirs, const std::vector<uint32_t> &cells, const std::vector<int32_t> &labels, G &out,
                   int32_t unreached = 0) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_catchments: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<detail::elem_t<G>, int32_t>::value, "d8_catchments: the label raster must be int32_t");
  if (cells.size() != labels.size()) throw std::runtime_error("d8_catchments: one label per seed cell");
  out.resize(flowdirs);
  out.setNoData(unreached);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(rdgpu_d8_catchments(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), cells.data(),
                                    labels.data(), (uint32_t)cells.size(), unreached, out.data()), "d8_catchments");
}

// every cell <- the flat index of the cell it finally drains to; 0xFFFFFFFF (the output's NoData) on NoData cells and loops
template <class F, class G>
void d8_outlets(const F &flowdirs, G &out) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_outlets: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<detail::elem_t<G>, uint32_t>::value, "d8_outlets: the outlet raster must be uint32_t");
  out.resize(flowdirs);
  out.setNoData(0xFFFFFFFFu);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(rdgpu_d8_outlets(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), out.data()), "d8_outlets");
}

// ---- channel network, Strahler stream order (no reference counterpart; the definition is in rdgpu.h) ----------------
// chan <- 1 where accum is not its NoData and accum >= threshold, 0 elsewhere
template <class A, class G>
void d8_channels(const A &accum, double threshold, G &chan) {
  static_assert(std::is_same<detail::elem_t<const A>, double>::value || std::is_same<detail::elem_t<A>, double>::value,
                "d8_channels: the accumulation must be double");
  static_assert(std::is_same<detail::elem_t<G>, uint8_t>::value, "d8_channels: the channel mask must be uint8_t");
  chan.resize(accum);
  chan.setNoData(0);
  if (accum.width() == 0 || accum.height() == 0) return;
  detail::check(rdgpu_d8_channels_f64(accum.data(), accum.noData(), threshold, accum.width(), accum.height(), chan.data()),
                "d8_channels");
}

// order <- the Strahler order of every channel cell, 0 (the output's NoData) off the channels, 255 on direction loops
template <class F, class C, class G>
void d8_stream_order(const F &flowdirs, const C &chan, G &order) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_stream_order: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<detail::elem_t<const C>, uint8_t>::value || std::is_same<detail::elem_t<C>, uint8_t>::value,
                "d8_stream_order: the channel mask must be uint8_t");
  static_assert(std::is_same<detail::elem_t<G>, uint8_t>::value, "d8_stream_order: the order raster must be uint8_t");
  if (chan.width() != flowdirs.width() || chan.height() != flowdirs.height())
    throw std::runtime_error("d8_stream_order: the channel mask must have the directions' size");
  order.resize(flowdirs);
  order.setNoData(0);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(rdgpu_d8_stream_order(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), chan.data(),
                                      order.data()), "d8_stream_order");
}
// every cell with a direction is a channel
template <class F, class G>
void d8_stream_order(const F &flowdirs, G &order) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_stream_order: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<detail::elem_t<G>, uint8_t>::value, "d8_stream_order: the order raster must be uint8_t");
  order.resize(flowdirs);
  order.setNoData(0);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(rdgpu_d8_stream_order(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), nullptr,
                                      order.data()), "d8_stream_order");
}

// richdem::FA_D8(const Array2D<elev_t>&, Array2D<accum_t>&)   methods/flow_accumulation.hpp:27
// accum is in/out: pre-loaded with the flow each cell generates.
template <class E, class G>
void FA_D8(const E &elevations, G &accum) {
  using T = detail::elem_t<E>;
  accum.setNoData((detail::elem_t<G>)-1);   // ACCUM_NO_DATA, flow_accumulation_generic.hpp:40
  if (accum.width() != elevations.width() || accum.height() != elevations.height())   // :42-43
    throw std::runtime_error("Accumulation array must have same dimensions as proportions array!");
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::with_double_accum(accum, [&](double *a) {
    detail::check(detail::c_fa_d8((const T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(), a),
                  "FA_D8");
  });
}

// richdem::FA_Tarboton / FA_Dinfinity(const Array2D<elev_t>&, Array2D<accum_t>&)   methods/flow_accumulation.hpp:16-17
template <class E, class G>
void FA_Tarboton(const E &elevations, G &accum) {
  using T = detail::elem_t<E>;
  accum.setNoData((detail::elem_t<G>)-1);
  if (accum.width() != elevations.width() || accum.height() != elevations.height())
    throw std::runtime_error("Accumulation array must have same dimensions as proportions array!");
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::with_double_accum(accum, [&](double *a) {
    detail::check(detail::c_fa_dinf((const T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(), a),
                  "FA_Tarboton");
  });
}
template <class E, class G>
void FA_Dinfinity(const E &elevations, G &accum) { FA_Tarboton(elevations, accum); }
// FA_Tarboton with the cells of drainable flats routed over Barnes' flat mask (no reference counterpart; the rule is in
// rdgpu.h, "D-infinity across flats").  The DEM is not altered.
template <class E, class G>
void FA_Tarboton_flats(const E &elevations, G &accum) {
  using T = detail::elem_t<E>;
  accum.setNoData((detail::elem_t<G>)-1);
  if (accum.width() != elevations.width() || accum.height() != elevations.height())
    throw std::runtime_error("Accumulation array must have same dimensions as proportions array!");
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::with_double_accum(accum, [&](double *a) {
    detail::check(detail::c_fa_dinf_flats((const T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(), a),
                  "FA_Tarboton_flats");
  });
}

// FA_D8 for a caller that built `accum` as an array of ones itself (apps/rd_flow_accumulation.cpp:13: Array2D<double>
// accum(dem, 1)) and says so: rdgpu::FA_D8(dem, accum, rdgpu::unit_weights).  accum is then output only -- nothing is read
// from it, nothing uploaded (rdgpu_fa_d8_unit_<T>); the result equals FA_D8 on an array of ones.
struct unit_weights_t {};
constexpr unit_weights_t unit_weights{};
template <class E, class G>
void FA_D8(const E &elevations, G &accum, unit_weights_t) {
  using T = detail::elem_t<E>;
  accum.setNoData((detail::elem_t<G>)-1);
  if (accum.width() != elevations.width() || accum.height() != elevations.height())
    throw std::runtime_error("Accumulation array must have same dimensions as proportions array!");
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::with_double_accum(accum, [&](double *a) {
    detail::check(detail::c_fa_d8_unit((const T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(), a),
                  "FA_D8");
  });
}

// richdem::FA_Holmgren / FA_Quinn / FA_Freeman / FA_D4   methods/flow_accumulation.hpp:18-20, :28
namespace detail {
template <class E, class G>
void fa_mfd(const E &elevations, G &accum, int method, double xparam, const char *who) {
  using T = elem_t<E>;
  accum.setNoData((elem_t<G>)-1);
  if (accum.width() != elevations.width() || accum.height() != elevations.height())
    throw std::runtime_error("Accumulation array must have same dimensions as proportions array!");
  if (elevations.width() == 0 || elevations.height() == 0) return;
  with_double_accum(accum, [&](double *a) {
    check(c_fa_mfd((const T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(), method, xparam, a), who);
  });
}
}  // namespace detail
template <class E, class G>
void FA_Holmgren(const E &elevations, G &accum, double xparam) { detail::fa_mfd(elevations, accum, 0, xparam, "FA_Holmgren"); }
template <class E, class G>
void FA_Freeman(const E &elevations, G &accum, double xparam) { detail::fa_mfd(elevations, accum, 1, xparam, "FA_Freeman"); }
template <class E, class G>
void FA_Quinn(const E &elevations, G &accum) { detail::fa_mfd(elevations, accum, 2, 1.0, "FA_Quinn"); }
template <class E, class G>
void FA_D4(const E &elevations, G &accum) { detail::fa_mfd(elevations, accum, 3, 1.0, "FA_D4"); }
template <class E, class G>
void FA_OCallaghanD4(const E &elevations, G &accum) { FA_D4(elevations, accum); }
template <class E, class G>
void FA_OCallaghanD8(const E &elevations, G &accum) { FA_D8(elevations, accum); }

// ---- flow proportions (the Array3D<float> on-the-wire format of rd.FlowProportions) ----------------------------
// richdem::FM_D8 / FM_OCallaghan<D8> (flowmet/OCallaghan1984.hpp:13-84), FM_D4 / FM_OCallaghan<D4> (:86),
// FM_Tarboton / FM_Dinfinity (flowmet/Tarboton1997.hpp:14-144), FM_Holmgren(x) (Holmgren1994.hpp:14),
// FM_Freeman(x) (Freeman1991.hpp:14), FM_Quinn (Quinn1991.hpp:13).  `props` is sized by the caller (nine float
// slots per cell, rdgpu::Array3D<float> or richdem::Array3D<float>); its NoData becomes NO_DATA_GEN = -2.
namespace detail {
// the slot buffer of a proportions array: richdem::Array3D has getData() (common/Array3D.hpp:165), rdgpu::Array3D data()
template <class P>
auto raw3(P &p, int) -> decltype(p.getData()) { return p.getData(); }
template <class P>
auto raw3(P &p, long) -> decltype(p.data()) { return p.data(); }

template <class E, class P, class Fn>
void fm_into(const E &elevations, P &props, Fn fn, const char *who) {
  static_assert(std::is_same<decltype(raw3(props, 0)), float *>::value, "FM_*: the proportions array must be Array3D<float>");
  props.setNoData(-2.0f);               // NO_DATA_GEN, common/constants.hpp:85
  if (props.width() != elevations.width() || props.height() != elevations.height())
    throw std::runtime_error(std::string(who) + ": proportions array must have the dimensions of the elevations");
  if (elevations.width() == 0 || elevations.height() == 0) return;
  check(fn(elevations.data(), elevations.noData(), elevations.width(), elevations.height(), raw3(props, 0)), who);
}
}  // namespace detail
template <class E, class P>
void FM_D8(const E &elevations, P &props) {
  using T = detail::elem_t<E>;
  detail::fm_into(elevations, props, [](const T *p, T nd, int w, int h, float *o) { return detail::c_fm_d8(p, nd, w, h, o); }, "FM_D8");
}
template <class E, class P>
void FM_Tarboton(const E &elevations, P &props) {
  using T = detail::elem_t<E>;
  detail::fm_into(elevations, props, [](const T *p, T nd, int w, int h, float *o) { return detail::c_fm_dinf(p, nd, w, h, o); }, "FM_Tarboton");
}
template <class E, class P>
void FM_Dinfinity(const E &elevations, P &props) { FM_Tarboton(elevations, props); }
// FM_Tarboton across flats (rdgpu.h "D-infinity across flats")
template <class E, class P>
void FM_Tarboton_flats(const E &elevations, P &props) {
  using T = detail::elem_t<E>;
  detail::fm_into(elevations, props, [](const T *p, T nd, int w, int h, float *o) { return detail::c_fm_dinf_flats(p, nd, w, h, o); },
                  "FM_Tarboton_flats");
}
namespace detail {
template <class E, class P>
void fm_mfd(const E &elevations, P &props, int method, double xparam, const char *who) {
  using T = elem_t<E>;
  fm_into(elevations, props,
          [method, xparam](const T *p, T nd, int w, int h, float *o) { return c_fm_mfd(p, nd, w, h, method, xparam, o); }, who);
}
}  // namespace detail
template <class E, class P>
void FM_Holmgren(const E &elevations, P &props, double xparam) { detail::fm_mfd(elevations, props, 0, xparam, "FM_Holmgren"); }
template <class E, class P>
void FM_Freeman(const E &elevations, P &props, double xparam) { detail::fm_mfd(elevations, props, 1, xparam, "FM_Freeman"); }
template <class E, class P>
void FM_Quinn(const E &elevations, P &props) { detail::fm_mfd(elevations, props, 2, 1.0, "FM_Quinn"); }
template <class E, class P>
void FM_D4(const E &elevations, P &props) { detail::fm_mfd(elevations, props, 3, 1.0, "FM_D4"); }
// FM_OCallaghan<topo>: Topology::D8 -> FM_D8, Topology::D4 -> FM_D4 (OCallaghan1984.hpp:81-90)
template <auto topo, class E, class P>
void FM_OCallaghan(const E &elevations, P &props) {
  if (detail::topology_code<topo>() == 8) FM_D8(elevations, props);
  else FM_D4(elevations, props);
}

// richdem::FlowAccumulation(const Array3D<float>&, Array2D<A>&)   methods/flow_accumulation_generic.hpp:33-100
// accum is in/out: pre-loaded with the flow each cell generates.
template <class P, class G>
void FlowAccumulation(const P &props, G &accum) {
  accum.setNoData((detail::elem_t<G>)-1);   // ACCUM_NO_DATA, :40
  if (accum.width() != props.width() || accum.height() != props.height())   // :42-43
    throw std::runtime_error("Accumulation array must have same dimensions as proportions array!");
  if (props.width() == 0 || props.height() == 0) return;
  const float *p9 = detail::raw3(const_cast<P &>(props), 0);   // (the reference's accessor is non-const; read only)
  detail::with_double_accum(accum, [&](double *a) {
    detail::check(rdgpu_flow_accumulation_f64(p9, props.width(), props.height(), a), "FlowAccumulation");
  });
}

// richdem::pit_mask<topo>(const Array2D<T>&, Array2D<uint8_t>&)   depressions/Barnes2014.hpp:593-676
template <auto topo, class E, class M>
void pit_mask(const E &elevations, M &mask) {
  using T = detail::elem_t<E>;
  static_assert(std::is_same<detail::elem_t<M>, uint8_t>::value, "pit_mask: the mask must be Array2D<uint8_t>");
  mask.resize(elevations.width(), elevations.height());   // :619
  mask.setNoData(3);                                       // :620
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::check(detail::c_pitmask((const T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(),
                                  detail::topology_code<topo>(), mask.data()),
                "pit_mask");
}

// richdem::ResolveFlatsEpsilon(Array2D<T>&)   flats/flats.hpp:21-28 (pywrapper.hpp:37 rdResolveFlatsEpsilon)
template <class E>
void ResolveFlatsEpsilon(E &elevations) {
  using T = detail::elem_t<E>;
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::check(detail::c_rfe((T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height()),
                "ResolveFlatsEpsilon");
}

// richdem::dinf_flow_directions(const Array2D<T>&, Array2D<float>&)   flowmet/dinf_flowdirs.hpp:128-152
template <class E, class F>
void dinf_flow_directions(const E &elevations, F &flowdirs) {
  using T = detail::elem_t<E>;
  static_assert(std::is_same<detail::elem_t<F>, float>::value, "dinf_flow_directions: flowdirs must be Array2D<float>");
  flowdirs.resize(elevations);          // :137
  flowdirs.setNoData(-1.0f);            // dinf_NO_DATA, :138
  if (elevations.width() == 0 || elevations.height() == 0) return;
  detail::check(detail::c_dinf((const T *)elevations.data(), elevations.noData(), elevations.width(),
                               elevations.height(), flowdirs.data()),
                "dinf_flow_directions");
}

// ---- TerrainAttribute (methods/terrain_attributes.hpp) ------------------------------------------------------------------
namespace detail {
#define RDGPU_SHIM_TERRAIN(SUF, T)                                                                                   \
  inline int c_terrain(const T *p, T nd, int w, int h, double cx, double cy, float zs, int a, float *o, float ond) { \
    return rdgpu_terrain_attribute_##SUF(p, nd, w, h, cx, cy, zs, a, o, ond);                                        \
  }
RDGPU_SHIM_TERRAIN(u8, uint8_t) RDGPU_SHIM_TERRAIN(i8, int8_t) RDGPU_SHIM_TERRAIN(u16, uint16_t)
RDGPU_SHIM_TERRAIN(i16, int16_t) RDGPU_SHIM_TERRAIN(u32, uint32_t) RDGPU_SHIM_TERRAIN(i32, int32_t)
RDGPU_SHIM_TERRAIN(u64, uint64_t) RDGPU_SHIM_TERRAIN(i64, int64_t) RDGPU_SHIM_TERRAIN(f32, float)
RDGPU_SHIM_TERRAIN(f64, double)
#undef RDGPU_SHIM_TERRAIN
template <class T>
int c_terrain(const T *, T, int, int, double, double, float, int, float *, float) { unsupported("TerrainAttribute"); }

// the cell lengths |geotransform[1]|, |geotransform[5]| (Array2D.hpp:1387-1399).  The reference asserts that there is a
// geotransform and, under NDEBUG, reads past the empty vector: here that is an exception.
template <class A>
void cell_lengths(const A &a, const char *fn, double &cx, double &cy) {
  if (a.geotransform.size() < 6)
    throw std::runtime_error(std::string(fn) + ": the raster has no geotransform, so its cell lengths are unknown");
  cx = a.geotransform[1] < 0 ? -a.geotransform[1] : a.geotransform[1];
  cy = a.geotransform[5] < 0 ? -a.geotransform[5] : a.geotransform[5];
}

// TerrainProcessor (terrain_attributes.hpp:329-348): output.resize(elevations) takes the size, geotransform and projection
// and KEEPS the output's own NoData value, which NoData cells of the input receive.
template <class E, class F>
void terrain(const E &elevations, F &output, float zscale, int attribute, const char *fn) {
  using T = elem_t<E>;
  static_assert(std::is_same<elem_t<F>, float>::value, "TerrainAttribute: the output must be Array2D<float>");
  double cx, cy;
  cell_lengths(elevations, fn, cx, cy);
  output.resize(elevations);
  if (elevations.width() == 0 || elevations.height() == 0) return;
  check(c_terrain((const T *)elevations.data(), elevations.noData(), elevations.width(), elevations.height(), cx, cy,
                  zscale, attribute, output.data(), output.noData()),
        fn);
}

template <class A, class S, class R>
void spi_cti(const A &flow_accumulation, const S &riserun_slope, R &result, bool cti) {
  static_assert(std::is_same<elem_t<A>, double>::value && std::is_same<elem_t<S>, float>::value &&
                    std::is_same<elem_t<R>, float>::value,
                "TA_SPI / TA_CTI: Array2D<double> accumulation, Array2D<float> slope, Array2D<float> result");
  if (flow_accumulation.width() != riserun_slope.width() || flow_accumulation.height() != riserun_slope.height())
    throw std::runtime_error(cti ? "Couldn't calculate CTI! The input matricies were of unequal dimensions!"
                                 : "Couldn't calculate SPI! The input matricies were of unequal dimensions!");
  double cx, cy;
  cell_lengths(flow_accumulation, cti ? "TA_CTI" : "TA_SPI", cx, cy);
  result.resize(flow_accumulation);
  result.setNoData(-1);
  if (flow_accumulation.width() == 0 || flow_accumulation.height() == 0) return;
  const int w = flow_accumulation.width(), h = flow_accumulation.height();
  check(cti ? rdgpu_ta_cti((const double *)flow_accumulation.data(), flow_accumulation.noData(),
                           (const float *)riserun_slope.data(), riserun_slope.noData(), w, h, cx, cy, result.data())
            : rdgpu_ta_spi((const double *)flow_accumulation.data(), flow_accumulation.noData(),
                           (const float *)riserun_slope.data(), riserun_slope.noData(), w, h, cx, cy, result.data()),
        cti ? "TA_CTI" : "TA_SPI");
}
}  // namespace detail

// richdem::TA_slope_riserun / _percentage / _degrees / _radians, TA_aspect, TA_curvature, TA_planform_curvature,
// TA_profile_curvature (const Array2D<T>&, Array2D<float>&, float zscale = 1)   terrain_attributes.hpp:362-562
#define RDGPU_SHIM_TA(NAME, ID)                                            \
  template <class E, class F>                                              \
  void NAME(const E &elevations, F &output, float zscale = 1.0f) {         \
    detail::terrain(elevations, output, zscale, ID, #NAME);                \
  }
RDGPU_SHIM_TA(TA_slope_riserun, RDGPU_TA_SLOPE_RISERUN)
RDGPU_SHIM_TA(TA_slope_percentage, RDGPU_TA_SLOPE_PERCENTAGE)
RDGPU_SHIM_TA(TA_slope_degrees, RDGPU_TA_SLOPE_DEGREES)
RDGPU_SHIM_TA(TA_slope_radians, RDGPU_TA_SLOPE_RADIANS)
RDGPU_SHIM_TA(TA_aspect, RDGPU_TA_ASPECT)
RDGPU_SHIM_TA(TA_curvature, RDGPU_TA_CURVATURE)
RDGPU_SHIM_TA(TA_planform_curvature, RDGPU_TA_PLANFORM_CURVATURE)
RDGPU_SHIM_TA(TA_profile_curvature, RDGPU_TA_PROFILE_CURVATURE)
#undef RDGPU_SHIM_TA

// richdem::TA_SPI / TA_CTI(const Array2D<T>&, const Array2D<U>&, Array2D<V>&)   terrain_attributes.hpp:30-112:
// the result takes the accumulation's size and geotransform, NoData -1
template <class A, class S, class R>
void TA_SPI(const A &flow_accumulation, const S &riserun_slope, R &result) {
  detail::spi_cti(flow_accumulation, riserun_slope, result, false);
}
template <class A, class S, class R>
void TA_CTI(const A &flow_accumulation, const S &riserun_slope, R &result) {
  detail::spi_cti(flow_accumulation, riserun_slope, result, true);
}

// ---- flow distance and HAND on the D8 forest (no reference counterpart; the definition is in rdgpu.h) ---------------
namespace detail {
#define RDGPU_SHIM_HAND(SUF, T)                                                                                            \
  inline int c_hand(const uint8_t *d, uint8_t dnd, const T *z, T znd, int w, int h, const uint8_t *c, double *o, double ond) { \
    return rdgpu_d8_hand_##SUF(d, dnd, z, znd, w, h, c, o, ond);                                                           \
  }
RDGPU_SHIM_HAND(u8, uint8_t) RDGPU_SHIM_HAND(i8, int8_t) RDGPU_SHIM_HAND(u16, uint16_t) RDGPU_SHIM_HAND(i16, int16_t)
RDGPU_SHIM_HAND(u32, uint32_t) RDGPU_SHIM_HAND(i32, int32_t) RDGPU_SHIM_HAND(f32, float) RDGPU_SHIM_HAND(f64, double)
#undef RDGPU_SHIM_HAND
template <class T>
int c_hand(const uint8_t *, uint8_t, const T *, T, int, int, const uint8_t *, double *, double) { unsupported("d8_hand"); }

template <class F, class C>
const uint8_t *path_mask(const F &flowdirs, const C *channels, const char *fn) {
  if (!channels) return nullptr;
  if (channels->width() != flowdirs.width() || channels->height() != flowdirs.height())
    throw std::runtime_error(std::string(fn) + ": the channel mask must have the directions' size");
  return channels->data();
}
}  // namespace detail

// dist <- the length of every cell's flow path to its drainage cell: the outlet, or with a channel mask the first channel
// cell on the path.  The cell lengths are the directions' |geotransform[1]|, |geotransform[5]|; the output takes the
// directions' size, geotransform and projection, NoData -1 (no drainage cell: NoData, a loop, no channel on the path).
template <class F, class G, class C>
void d8_flow_distance(const F &flowdirs, G &dist, const C *channels) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_flow_distance: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<detail::elem_t<G>, double>::value, "d8_flow_distance: the distance raster must be double");
  double cx, cy;
  detail::cell_lengths(flowdirs, "d8_flow_distance", cx, cy);
  const uint8_t *mask = detail::path_mask(flowdirs, channels, "d8_flow_distance");
  dist.resize(flowdirs);
  dist.setNoData(-1.0);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(rdgpu_d8_flow_path(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), mask, cx, cy, nullptr,
                                   nullptr, dist.data(), -1.0), "d8_flow_distance");
}
template <class F, class G>
void d8_flow_distance(const F &flowdirs, G &dist) {
  d8_flow_distance(flowdirs, dist, static_cast<const F *>(nullptr));
}

// hand <- dem[c] - dem[drainage cell of c] (height above the nearest drainage), NoData -9999 where there is no drainage
// cell or one of the two elevations is the DEM's NoData; the output takes the directions' size, geotransform and projection
template <class E, class F, class G, class C>
void d8_hand(const E &dem, const F &flowdirs, G &hand, const C *channels) {
  using T = detail::elem_t<E>;
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_hand: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<detail::elem_t<G>, double>::value, "d8_hand: the HAND raster must be double");
  if (dem.width() != flowdirs.width() || dem.height() != flowdirs.height())
    throw std::runtime_error("d8_hand: the DEM must have the directions' size");
  const uint8_t *mask = detail::path_mask(flowdirs, channels, "d8_hand");
  hand.resize(flowdirs);
  hand.setNoData(-9999.0);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(detail::c_hand(flowdirs.data(), flowdirs.noData(), (const T *)dem.data(), (T)dem.noData(), flowdirs.width(),
                               flowdirs.height(), mask, hand.data(), -9999.0), "d8_hand");
}
template <class E, class F, class G>
void d8_hand(const E &dem, const F &flowdirs, G &hand) {
  d8_hand(dem, flowdirs, hand, static_cast<const F *>(nullptr));
}

// ---- stream reaches on the D8 forest (no reference counterpart; the definitions are in rdgpu.h) ----------------------
// reach <- the label 1..N of every channel cell's reach (0 elsewhere), catchment <- the label of the reach every cell
// drains through (0: none), table[i] <- the record of label i + 1.  channels and order are optional (nullptr: every cell
// with a direction is a channel cell; no order in the records).  The cell lengths are the directions' |geotransform[1]|,
// |geotransform[5]|; the outputs take the directions' size, geotransform and projection, NoData 0.  Two calls of the
// engine: the sizing call, then the one that fills everything.
template <class F, class C, class O, class R>
void d8_stream_reaches(const F &flowdirs, const C *channels, const O *order, R &reach, R &catchment, std::vector<rdgpu_reach> &table) {
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_stream_reaches: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<detail::elem_t<R>, uint32_t>::value, "d8_stream_reaches: the label rasters must be uint32_t");
  const char *fn = "d8_stream_reaches";
  double cx, cy;
  detail::cell_lengths(flowdirs, fn, cx, cy);
  const uint8_t *mask = detail::path_mask(flowdirs, channels, fn);
  if (order && (order->width() != flowdirs.width() || order->height() != flowdirs.height()))
    throw std::runtime_error(std::string(fn) + ": the order raster must have the directions' size");
  const uint8_t *ord = order ? order->data() : nullptr;
  reach.resize(flowdirs);
  reach.setNoData(0);
  catchment.resize(flowdirs);
  catchment.setNoData(0);
  table.clear();
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  uint32_t n = 0;
  detail::check(rdgpu_d8_stream_reaches(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), mask, ord, cx, cy,
                                        nullptr, nullptr, nullptr, 0, &n), fn);
  table.resize(n);
  uint32_t got = 0;
  detail::check(rdgpu_d8_stream_reaches(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), mask, ord, cx, cy,
                                        reach.data(), catchment.data(), n ? table.data() : nullptr, n, &got), fn);
  if (got != n) throw std::runtime_error(std::string(fn) + ": the count changed between the two calls");
}

// ---- distance and drop DOWN to the stop cells over D-infinity / MFD proportions (no reference counterpart; the
// definition is in rdgpu.h) ---------------------------------------------------------------------------------------------
enum class DistanceStat { Average = 0, Minimum = 1, Maximum = 2 };
struct DistanceDownOptions {
  DistanceStat stat = DistanceStat::Average;   // how a cell's receivers are combined
  bool strict = true;                          // every receiver must reach a stop cell (false: at least one)
  double out_nodata = -9999.0;                 // NoData of both outputs: cells without a value
};
namespace detail {
#define RDGPU_SHIM_DINF_DIST(SUF, T)                                                                                        \
  inline int c_dinf_dist(const T *z, T nd, int w, int h, const uint8_t *c, int st, int strict, double cx, double cy, double *d, \
                         double *r, double ond) {                                                                           \
    return rdgpu_dinf_distance_down_##SUF(z, nd, w, h, c, st, strict, cx, cy, d, r, ond);                                   \
  }                                                                                                                         \
  inline int c_dinf_dist_flats(const T *z, T nd, int w, int h, const uint8_t *c, int st, int strict, double cx, double cy,  \
                               double *d, double *r, double ond) {                                                          \
    return rdgpu_dinf_distance_down_flats_##SUF(z, nd, w, h, c, st, strict, cx, cy, d, r, ond);                             \
  }
RDGPU_SHIM_DINF_DIST(u8, uint8_t) RDGPU_SHIM_DINF_DIST(i8, int8_t) RDGPU_SHIM_DINF_DIST(u16, uint16_t)
RDGPU_SHIM_DINF_DIST(i16, int16_t) RDGPU_SHIM_DINF_DIST(u32, uint32_t) RDGPU_SHIM_DINF_DIST(i32, int32_t)
RDGPU_SHIM_DINF_DIST(f32, float) RDGPU_SHIM_DINF_DIST(f64, double)
#undef RDGPU_SHIM_DINF_DIST
template <class T>
int c_dinf_dist(const T *, T, int, int, const uint8_t *, int, int, double, double, double *, double *, double) {
  unsupported("DinfDistanceDown");
}
template <class T>
int c_dinf_dist_flats(const T *, T, int, int, const uint8_t *, int, int, double, double, double *, double *, double) {
  unsupported("DinfDistanceDown_flats");
}
template <class G>
double *dist_plane(G *out, int w, int h, double nodata) {
  if (!out) return nullptr;
  static_assert(std::is_same<elem_t<G>, double>::value, "distance down: the output rasters must be double");
  out->resize(w, h);
  out->setNoData(nodata);
  return out->data();
}
template <class C>
const uint8_t *dist_mask(int w, int h, const C *channels, const char *fn) {
  if (!channels) return nullptr;
  if (channels->width() != w || channels->height() != h)
    throw std::runtime_error(std::string(fn) + ": the channel mask must have the raster's size");
  return channels->data();
}
}  // namespace detail

// *dist, *drop (each optional, at least one) <- the distance and the drop from every cell down to the stop cells over the
// proportions `props` (Array3D<float>): the cells of the channel mask, or without one the cells that have no receiver.
// `elevations` (Array2D<double>, required for drop) are taken as they are.  Cell lengths cell_x, cell_y.  The outputs take
// the proportions' width and height, NoData opt.out_nodata.
template <class P, class E, class G, class C>
void FlowDistanceDown(const P &props, const E *elevations, G *dist, G *drop, const C *channels, double cell_x = 1.0,
                      double cell_y = 1.0, const DistanceDownOptions &opt = DistanceDownOptions()) {
  static_assert(std::is_same<detail::elem_t<E>, double>::value, "FlowDistanceDown: the elevations must be Array2D<double>");
  const int w = props.width(), h = props.height();
  if (!dist && !drop) throw std::runtime_error("FlowDistanceDown: no output requested");
  if (drop && !elevations) throw std::runtime_error("FlowDistanceDown: the drop needs the elevations");
  if (elevations && (elevations->width() != w || elevations->height() != h))
    throw std::runtime_error("FlowDistanceDown: the elevations must have the proportions' size");
  const uint8_t *mask = detail::dist_mask(w, h, channels, "FlowDistanceDown");
  double *pd = detail::dist_plane(dist, w, h, opt.out_nodata), *pr = detail::dist_plane(drop, w, h, opt.out_nodata);
  if (w == 0 || h == 0) return;
  const float *p9 = detail::raw3(const_cast<P &>(props), 0);   // (the reference's accessor is non-const; read only)
  detail::check(rdgpu_mfd_distance_down(p9, w, h, mask, elevations ? (const double *)elevations->data() : nullptr, (int)opt.stat,
                                        opt.strict ? 1 : 0, cell_x, cell_y, pd, pr, opt.out_nodata), "FlowDistanceDown");
}
// the distance alone
template <class P, class G>
void FlowDistanceDown(const P &props, G &dist, double cell_x = 1.0, double cell_y = 1.0,
                      const DistanceDownOptions &opt = DistanceDownOptions()) {
  const int w = props.width(), h = props.height();
  double *pd = detail::dist_plane(&dist, w, h, opt.out_nodata);
  if (w == 0 || h == 0) return;
  detail::check(rdgpu_mfd_distance_down(detail::raw3(const_cast<P &>(props), 0), w, h, nullptr, nullptr, (int)opt.stat,
                                        opt.strict ? 1 : 0, cell_x, cell_y, pd, nullptr, opt.out_nodata), "FlowDistanceDown");
}

// The same over the D-infinity proportions of a DEM (FM_Tarboton, never materialised), elevations and cell lengths
// (|geotransform[1]|, |geotransform[5]|) the DEM's; the outputs take the DEM's size, geotransform and projection.
namespace detail {
template <class E, class G, class C, class Fn>
void dinf_distance_down(const E &dem, G *dist, G *drop, const C *channels, const DistanceDownOptions &opt, Fn entry, const char *who) {
  using T = elem_t<E>;
  const int w = dem.width(), h = dem.height();
  if (!dist && !drop) throw std::runtime_error(std::string(who) + ": no output requested");
  double cx, cy;
  cell_lengths(dem, who, cx, cy);
  const uint8_t *mask = dist_mask(w, h, channels, who);
  for (G *o : {dist, drop})
    if (o) {
      static_assert(std::is_same<elem_t<G>, double>::value, "DinfDistanceDown: the output rasters must be double");
      o->resize(dem);
      o->setNoData(opt.out_nodata);
    }
  if (w == 0 || h == 0) return;
  check(entry((const T *)dem.data(), (T)dem.noData(), w, h, mask, (int)opt.stat, opt.strict ? 1 : 0, cx, cy,
              dist ? dist->data() : nullptr, drop ? drop->data() : nullptr, opt.out_nodata), who);
}
}  // namespace detail
template <class E, class G, class C>
void DinfDistanceDown(const E &dem, G *dist, G *drop, const C *channels, const DistanceDownOptions &opt = DistanceDownOptions()) {
  using T = detail::elem_t<E>;
  detail::dinf_distance_down(dem, dist, drop, channels, opt,
                             [](const T *z, T nd, int w, int h, const uint8_t *c, int st, int strict, double cx, double cy, double *d,
                                double *r, double ond) { return detail::c_dinf_dist(z, nd, w, h, c, st, strict, cx, cy, d, r, ond); },
                             "DinfDistanceDown");
}
// height above the drainage reached over the D-infinity proportions: the drop down to the channel mask
template <class E, class G, class C>
void DinfHand(const E &dem, G &hand, const C &channels, const DistanceDownOptions &opt = DistanceDownOptions()) {
  DinfDistanceDown(dem, static_cast<G *>(nullptr), &hand, &channels, opt);
}
// Both over the proportions of FM_Tarboton_flats: the drainable flats of the DEM pass flow on (rdgpu.h "D-infinity across
// flats"); same arguments, statistics and strict rule.
template <class E, class G, class C>
void DinfDistanceDown_flats(const E &dem, G *dist, G *drop, const C *channels, const DistanceDownOptions &opt = DistanceDownOptions()) {
  using T = detail::elem_t<E>;
  detail::dinf_distance_down(dem, dist, drop, channels, opt,
                             [](const T *z, T nd, int w, int h, const uint8_t *c, int st, int strict, double cx, double cy, double *d,
                                double *r, double ond) { return detail::c_dinf_dist_flats(z, nd, w, h, c, st, strict, cx, cy, d, r, ond); },
                             "DinfDistanceDown_flats");
}
template <class E, class G, class C>
void DinfHand_flats(const E &dem, G &hand, const C &channels, const DistanceDownOptions &opt = DistanceDownOptions()) {
  DinfDistanceDown_flats(dem, static_cast<G *>(nullptr), &hand, &channels, opt);
}

// ---- distance and rise UP to the sources over D-infinity / MFD proportions (no reference counterpart; the definition is
// in rdgpu.h) ------------------------------------------------------------------------------------------------------------
struct DistanceUpOptions {
  DistanceStat stat = DistanceStat::Average;   // how a cell's donors are combined
  float min_share = 0.0f;                      // a share must exceed it to be a link (TauDEM's proportion threshold)
  double out_nodata = -9999.0;                 // NoData of both outputs: cells without a value
};
namespace detail {
#define RDGPU_SHIM_DINF_DISTUP(SUF, T)                                                                                      \
  inline int c_dinf_distup(const T *z, T nd, int w, int h, int st, float ms, double cx, double cy, double *d, double *r,    \
                           double ond) {                                                                                    \
    return rdgpu_dinf_distance_up_##SUF(z, nd, w, h, st, ms, cx, cy, d, r, ond);                                            \
  }                                                                                                                         \
  inline int c_dinf_distup_flats(const T *z, T nd, int w, int h, int st, float ms, double cx, double cy, double *d,         \
                                 double *r, double ond) {                                                                   \
    return rdgpu_dinf_distance_up_flats_##SUF(z, nd, w, h, st, ms, cx, cy, d, r, ond);                                      \
  }
RDGPU_SHIM_DINF_DISTUP(u8, uint8_t) RDGPU_SHIM_DINF_DISTUP(i8, int8_t) RDGPU_SHIM_DINF_DISTUP(u16, uint16_t)
RDGPU_SHIM_DINF_DISTUP(i16, int16_t) RDGPU_SHIM_DINF_DISTUP(u32, uint32_t) RDGPU_SHIM_DINF_DISTUP(i32, int32_t)
RDGPU_SHIM_DINF_DISTUP(f32, float) RDGPU_SHIM_DINF_DISTUP(f64, double)
#undef RDGPU_SHIM_DINF_DISTUP
template <class T>
int c_dinf_distup(const T *, T, int, int, int, float, double, double, double *, double *, double) {
  unsupported("DinfDistanceUp");
}
template <class T>
int c_dinf_distup_flats(const T *, T, int, int, int, float, double, double, double *, double *, double) {
  unsupported("DinfDistanceUp_flats");
}
}  // namespace detail

// *dist, *rise (each optional, at least one) <- the distance and the rise from every cell up to the sources (the cells
// without donors) over the proportions `props` (Array3D<float>).  `elevations` (Array2D<double>, required for rise) are
// taken as they are.  Cell lengths cell_x, cell_y.  The outputs take the proportions' width and height, NoData
// opt.out_nodata.
template <class P, class E, class G>
void FlowDistanceUp(const P &props, const E *elevations, G *dist, G *rise, double cell_x = 1.0, double cell_y = 1.0,
                    const DistanceUpOptions &opt = DistanceUpOptions()) {
  static_assert(std::is_same<detail::elem_t<E>, double>::value, "FlowDistanceUp: the elevations must be Array2D<double>");
  const int w = props.width(), h = props.height();
  if (!dist && !rise) throw std::runtime_error("FlowDistanceUp: no output requested");
  if (rise && !elevations) throw std::runtime_error("FlowDistanceUp: the rise needs the elevations");
  if (elevations && (elevations->width() != w || elevations->height() != h))
    throw std::runtime_error("FlowDistanceUp: the elevations must have the proportions' size");
  double *pd = detail::dist_plane(dist, w, h, opt.out_nodata), *pr = detail::dist_plane(rise, w, h, opt.out_nodata);
  if (w == 0 || h == 0) return;
  const float *p9 = detail::raw3(const_cast<P &>(props), 0);   // (the reference's accessor is non-const; read only)
  detail::check(rdgpu_mfd_distance_up(p9, w, h, elevations ? (const double *)elevations->data() : nullptr, (int)opt.stat,
                                      opt.min_share, cell_x, cell_y, pd, pr, opt.out_nodata), "FlowDistanceUp");
}
// the distance alone
template <class P, class G>
void FlowDistanceUp(const P &props, G &dist, double cell_x = 1.0, double cell_y = 1.0,
                    const DistanceUpOptions &opt = DistanceUpOptions()) {
  const int w = props.width(), h = props.height();
  double *pd = detail::dist_plane(&dist, w, h, opt.out_nodata);
  if (w == 0 || h == 0) return;
  detail::check(rdgpu_mfd_distance_up(detail::raw3(const_cast<P &>(props), 0), w, h, nullptr, (int)opt.stat, opt.min_share,
                                      cell_x, cell_y, pd, nullptr, opt.out_nodata), "FlowDistanceUp");
}

// The same over the D-infinity proportions of a DEM (FM_Tarboton, never materialised), elevations and cell lengths
// (|geotransform[1]|, |geotransform[5]|) the DEM's; the outputs take the DEM's size, geotransform and projection.
namespace detail {
template <class E, class G, class Fn>
void dinf_distance_up(const E &dem, G *dist, G *rise, const DistanceUpOptions &opt, Fn entry, const char *who) {
  using T = elem_t<E>;
  const int w = dem.width(), h = dem.height();
  if (!dist && !rise) throw std::runtime_error(std::string(who) + ": no output requested");
  double cx, cy;
  cell_lengths(dem, who, cx, cy);
  for (G *o : {dist, rise})
    if (o) {
      static_assert(std::is_same<elem_t<G>, double>::value, "DinfDistanceUp: the output rasters must be double");
      o->resize(dem);
      o->setNoData(opt.out_nodata);
    }
  if (w == 0 || h == 0) return;
  check(entry((const T *)dem.data(), (T)dem.noData(), w, h, (int)opt.stat, opt.min_share, cx, cy, dist ? dist->data() : nullptr,
              rise ? rise->data() : nullptr, opt.out_nodata), who);
}
}  // namespace detail
template <class E, class G>
void DinfDistanceUp(const E &dem, G *dist, G *rise, const DistanceUpOptions &opt = DistanceUpOptions()) {
  using T = detail::elem_t<E>;
  detail::dinf_distance_up(dem, dist, rise, opt,
                           [](const T *z, T nd, int w, int h, int st, float ms, double cx, double cy, double *d, double *r,
                              double ond) { return detail::c_dinf_distup(z, nd, w, h, st, ms, cx, cy, d, r, ond); },
                           "DinfDistanceUp");
}
// over the proportions of FM_Tarboton_flats: the drainable flats of the DEM pass flow on
template <class E, class G>
void DinfDistanceUp_flats(const E &dem, G *dist, G *rise, const DistanceUpOptions &opt = DistanceUpOptions()) {
  using T = detail::elem_t<E>;
  detail::dinf_distance_up(dem, dist, rise, opt,
                           [](const T *z, T nd, int w, int h, int st, float ms, double cx, double cy, double *d, double *r,
                              double ond) { return detail::c_dinf_distup_flats(z, nd, w, h, st, ms, cx, cy, d, r, ond); },
                           "DinfDistanceUp_flats");
}

// ---- reverse accumulation, largest weight downslope and upslope dependence over D-infinity / MFD proportions (no
// reference counterpart; the definition is in rdgpu.h) ---------------------------------------------------------------
struct ReverseAccumOptions {
  double weight_nodata = std::numeric_limits<double>::quiet_NaN();   // cells with this weight (and NaNs) do not contribute
  double out_nodata = -9999.0;                                       // NoData of the outputs: cells without a value
};
namespace detail {
#define RDGPU_SHIM_DINF_REV(SUF, T)                                                                                         \
  inline int c_dinf_rev(const T *z, T nd, int w, int h, const double *wt, double wnd, const uint8_t *de, double *ra,        \
                        double *wm, double ond) {                                                                           \
    return rdgpu_dinf_reverse_accum_##SUF(z, nd, w, h, wt, wnd, de, ra, wm, ond);                                           \
  }                                                                                                                         \
  inline int c_dinf_rev_flats(const T *z, T nd, int w, int h, const double *wt, double wnd, const uint8_t *de, double *ra,  \
                              double *wm, double ond) {                                                                     \
    return rdgpu_dinf_reverse_accum_flats_##SUF(z, nd, w, h, wt, wnd, de, ra, wm, ond);                                     \
  }
RDGPU_SHIM_DINF_REV(u8, uint8_t) RDGPU_SHIM_DINF_REV(i8, int8_t) RDGPU_SHIM_DINF_REV(u16, uint16_t)
RDGPU_SHIM_DINF_REV(i16, int16_t) RDGPU_SHIM_DINF_REV(u32, uint32_t) RDGPU_SHIM_DINF_REV(i32, int32_t)
RDGPU_SHIM_DINF_REV(f32, float) RDGPU_SHIM_DINF_REV(f64, double)
#undef RDGPU_SHIM_DINF_REV
template <class T>
int c_dinf_rev(const T *, T, int, int, const double *, double, const uint8_t *, double *, double *, double) {
  unsupported("DinfReverseAccumulation");
}
template <class T>
int c_dinf_rev_flats(const T *, T, int, int, const double *, double, const uint8_t *, double *, double *, double) {
  unsupported("DinfReverseAccumulation_flats");
}
template <class W>
const double *rev_weights(int w, int h, const W *weights, const char *fn) {
  if (!weights) return nullptr;
  static_assert(std::is_same<elem_t<W>, double>::value, "reverse accumulation: the weights must be Array2D<double>");
  if (weights->width() != w || weights->height() != h)
    throw std::runtime_error(std::string(fn) + ": the weights must have the raster's size");
  return weights->data();
}
}  // namespace detail

// *racc, *wmax (each optional, at least one; wmax needs weights) <- the reverse accumulation and the largest weight
// downslope over the proportions `props` (Array3D<float>).  `weights` (Array2D<double>, optional) and `dest`
// (Array2D<uint8_t>, optional: the absorbing cells); without weights this is the upslope dependence on dest.  The outputs
// take the proportions' width and height, NoData opt.out_nodata.
template <class P, class W, class C, class G>
void FlowReverseAccumulation(const P &props, const W *weights, const C *dest, G *racc, G *wmax,
                             const ReverseAccumOptions &opt = ReverseAccumOptions()) {
  const int w = props.width(), h = props.height();
  if (!racc && !wmax) throw std::runtime_error("FlowReverseAccumulation: no output requested");
  if (wmax && !weights) throw std::runtime_error("FlowReverseAccumulation: wmax needs the weights");
  if (!weights && !dest) throw std::runtime_error("FlowReverseAccumulation: neither weights nor dest given");
  const double *pw = detail::rev_weights(w, h, weights, "FlowReverseAccumulation");
  const uint8_t *mask = detail::dist_mask(w, h, dest, "FlowReverseAccumulation");
  double *pa = detail::dist_plane(racc, w, h, opt.out_nodata), *pm = detail::dist_plane(wmax, w, h, opt.out_nodata);
  if (w == 0 || h == 0) return;
  const float *p9 = detail::raw3(const_cast<P &>(props), 0);   // (the reference's accessor is non-const; read only)
  detail::check(rdgpu_mfd_reverse_accum(p9, w, h, pw, opt.weight_nodata, mask, pa, pm, opt.out_nodata), "FlowReverseAccumulation");
}

// The same over the D-infinity proportions of a DEM (FM_Tarboton, never materialised); the outputs take the DEM's size,
// geotransform and projection.
namespace detail {
template <class E, class W, class C, class G, class Fn>
void dinf_reverse(const E &dem, const W *weights, const C *dest, G *racc, G *wmax, const ReverseAccumOptions &opt, Fn entry,
                  const char *who) {
  using T = elem_t<E>;
  const int w = dem.width(), h = dem.height();
  if (!racc && !wmax) throw std::runtime_error(std::string(who) + ": no output requested");
  if (wmax && !weights) throw std::runtime_error(std::string(who) + ": wmax needs the weights");
  if (!weights && !dest) throw std::runtime_error(std::string(who) + ": neither weights nor dest given");
  const double *pw = rev_weights(w, h, weights, who);
  const uint8_t *mask = dist_mask(w, h, dest, who);
  for (G *o : {racc, wmax})
    if (o) {
      static_assert(std::is_same<elem_t<G>, double>::value, "DinfReverseAccumulation: the output rasters must be double");
      o->resize(dem);
      o->setNoData(opt.out_nodata);
    }
  if (w == 0 || h == 0) return;
  check(entry((const T *)dem.data(), (T)dem.noData(), w, h, pw, opt.weight_nodata, mask, racc ? racc->data() : nullptr,
              wmax ? wmax->data() : nullptr, opt.out_nodata), who);
}
}  // namespace detail
template <class E, class W, class C, class G>
void DinfReverseAccumulation(const E &dem, const W *weights, const C *dest, G *racc, G *wmax,
                             const ReverseAccumOptions &opt = ReverseAccumOptions()) {
  using T = detail::elem_t<E>;
  detail::dinf_reverse(dem, weights, dest, racc, wmax, opt,
                       [](const T *z, T nd, int w, int h, const double *wt, double wnd, const uint8_t *de, double *ra, double *wm,
                          double ond) { return detail::c_dinf_rev(z, nd, w, h, wt, wnd, de, ra, wm, ond); },
                       "DinfReverseAccumulation");
}
// over the proportions of FM_Tarboton_flats: the drainable flats of the DEM pass flow on
template <class E, class W, class C, class G>
void DinfReverseAccumulation_flats(const E &dem, const W *weights, const C *dest, G *racc, G *wmax,
                                   const ReverseAccumOptions &opt = ReverseAccumOptions()) {
  using T = detail::elem_t<E>;
  detail::dinf_reverse(dem, weights, dest, racc, wmax, opt,
                       [](const T *z, T nd, int w, int h, const double *wt, double wnd, const uint8_t *de, double *ra, double *wm,
                          double ond) { return detail::c_dinf_rev_flats(z, nd, w, h, wt, wnd, de, ra, wm, ond); },
                       "DinfReverseAccumulation_flats");
}
// dep <- the fraction of every cell's flow that reaches the cells of `dest` (TauDEM's DinfUpDependence)
template <class E, class C, class G>
void DinfUpslopeDependence(const E &dem, const C &dest, G &dep, const ReverseAccumOptions &opt = ReverseAccumOptions()) {
  DinfReverseAccumulation(dem, static_cast<const G *>(nullptr), &dest, &dep, static_cast<G *>(nullptr), opt);
}
template <class E, class C, class G>
void DinfUpslopeDependence_flats(const E &dem, const C &dest, G &dep, const ReverseAccumOptions &opt = ReverseAccumOptions()) {
  DinfReverseAccumulation_flats(dem, static_cast<const G *>(nullptr), &dest, &dep, static_cast<G *>(nullptr), opt);
}

// ---- longest upstream flow path on the D8 forest (no reference counterpart; the definition is in rdgpu.h) -----------
// length <- the length of the longest flow path that ends at each cell; *from_cell (optional, uint32_t) <- the flat index
// of that path's head, the lowest on a tie; *on_basin_path (optional, uint8_t) <- 1 on the longest path of every basin,
// from its head down to the outlet.  The cell lengths are the directions' |geotransform[1]|, |geotransform[5]|; the
// outputs take the directions' size, geotransform and projection, NoData -1, 0xFFFFFFFF and 0 (NoData cells and cells
// that drain into a direction loop have no path).
namespace detail {
template <class F, class G>
void longest_prepare(const F &flowdirs, G &length, double &cx, double &cy) {
  static_assert(std::is_same<elem_t<const F>, uint8_t>::value || std::is_same<elem_t<F>, uint8_t>::value,
                "d8_longest_flow_path: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<elem_t<G>, double>::value, "d8_longest_flow_path: the length raster must be double");
  cell_lengths(flowdirs, "d8_longest_flow_path", cx, cy);
  length.resize(flowdirs);
  length.setNoData(-1.0);
}
template <class F, class G>
void longest_run(const F &flowdirs, G &length, double cx, double cy, uint32_t *from, uint8_t *on_path) {
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  check(rdgpu_d8_longest_flow_path(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), cx, cy, from, nullptr,
                                   length.data(), -1.0, on_path), "d8_longest_flow_path");
}
template <class F, class A, class V>
elem_t<A> *longest_plane(const F &flowdirs, A *plane, V nodata) {
  if (!plane) return nullptr;
  plane->resize(flowdirs);
  plane->setNoData(nodata);
  return plane->data();
}
}  // namespace detail
template <class F, class G, class C, class B>
void d8_longest_flow_path(const F &flowdirs, G &length, C *from_cell, B *on_basin_path) {
  static_assert(std::is_same<detail::elem_t<C>, uint32_t>::value, "d8_longest_flow_path: the cell raster must be uint32_t");
  static_assert(std::is_same<detail::elem_t<B>, uint8_t>::value, "d8_longest_flow_path: the path mask must be uint8_t");
  double cx, cy;
  detail::longest_prepare(flowdirs, length, cx, cy);
  uint32_t *from = detail::longest_plane(flowdirs, from_cell, 0xFFFFFFFFu);
  uint8_t *on_path = detail::longest_plane(flowdirs, on_basin_path, (uint8_t)0);
  detail::longest_run(flowdirs, length, cx, cy, from, on_path);
}
template <class F, class G, class C>
void d8_longest_flow_path(const F &flowdirs, G &length, C *from_cell) {
  static_assert(std::is_same<detail::elem_t<C>, uint32_t>::value, "d8_longest_flow_path: the cell raster must be uint32_t");
  double cx, cy;
  detail::longest_prepare(flowdirs, length, cx, cy);
  detail::longest_run(flowdirs, length, cx, cy, detail::longest_plane(flowdirs, from_cell, 0xFFFFFFFFu), nullptr);
}
template <class F, class G>
void d8_longest_flow_path(const F &flowdirs, G &length) {
  double cx, cy;
  detail::longest_prepare(flowdirs, length, cx, cy);
  detail::longest_run(flowdirs, length, cx, cy, nullptr, nullptr);
}

// ---- weighted accumulation and total upstream length on the D8 forest (the definition is in rdgpu.h) ----------------
namespace detail {
#define RDGPU_SHIM_WEIGHTED(SUF, T, S)                                                                          \
  inline int c_weighted(const uint8_t *d, uint8_t dnd, const T *v, T vnd, int w, int h, S *sum, S snd) {        \
    return rdgpu_d8_flow_accum_weighted_##SUF(d, dnd, v, vnd, w, h, sum, snd);                                  \
  }
RDGPU_SHIM_WEIGHTED(u8, uint8_t, int64_t) RDGPU_SHIM_WEIGHTED(i8, int8_t, int64_t) RDGPU_SHIM_WEIGHTED(u16, uint16_t, int64_t)
RDGPU_SHIM_WEIGHTED(i16, int16_t, int64_t) RDGPU_SHIM_WEIGHTED(u32, uint32_t, int64_t) RDGPU_SHIM_WEIGHTED(i32, int32_t, int64_t)
RDGPU_SHIM_WEIGHTED(f32, float, double) RDGPU_SHIM_WEIGHTED(f64, double, double)
#undef RDGPU_SHIM_WEIGHTED
template <class T, class S>
int c_weighted(const uint8_t *, uint8_t, const T *, T, int, int, S *, S) { unsupported("d8_flow_accum_weighted"); }
}  // namespace detail

// sum <- the sum of `weights` over everything that drains through each cell along the GIVEN directions, the cell included
// (richdem::FlowAccumulation on the proportions of these directions, without the proportions array).  Cells whose weight
// is the weights' NoData (or a NaN) add nothing but pass on what they receive.  sum is int64_t for int8 .. uint32 weights
// and double for float and double weights (64-bit integer weights throw); its NoData, kept if it has been set and written
// where the direction is NoData, defaults to -1.  It takes the directions' size, geotransform and projection.
template <class F, class V, class G>
void d8_flow_accum_weighted(const F &flowdirs, const V &weights, G &sum) {
  using T = detail::elem_t<const V>;
  using S = detail::elem_t<G>;
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_flow_accum_weighted: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<S, typename std::conditional<std::is_floating_point<T>::value, double, int64_t>::type>::value,
                "d8_flow_accum_weighted: the sum raster is int64_t for integer weights, double for float and double weights");
  if (weights.width() != flowdirs.width() || weights.height() != flowdirs.height())
    throw std::runtime_error("d8_flow_accum_weighted: the weights must have the directions' size");
  const S sum_nodata = sum.noData();
  sum.resize(flowdirs);
  sum.setNoData(sum_nodata);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  detail::check(detail::c_weighted(flowdirs.data(), flowdirs.noData(), (const T *)weights.data(), (T)weights.noData(),
                                   flowdirs.width(), flowdirs.height(), (S *)sum.data(), sum_nodata), "d8_flow_accum_weighted");
}

// length <- the total length of the links of the tree above each cell (TauDEM's tlen), NoData -1; *along_x, *along_y,
// *diagonal (uint32_t; the second form leaves them out) <- how many of those links run along x, along y and diagonally, NoData
// 0xFFFFFFFF.  The cell lengths are the directions' |geotransform[1]|, |geotransform[5]|; the outputs take the directions'
// size, geotransform and projection.
namespace detail {
template <class F, class G>
void tlen_run(const F &flowdirs, G &length, uint32_t *steps) {
  static_assert(std::is_same<elem_t<const F>, uint8_t>::value || std::is_same<elem_t<F>, uint8_t>::value,
                "d8_total_upstream_length: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<elem_t<G>, double>::value, "d8_total_upstream_length: the length raster must be double");
  double cx, cy;
  cell_lengths(flowdirs, "d8_total_upstream_length", cx, cy);
  length.resize(flowdirs);
  length.setNoData(-1.0);
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  check(rdgpu_d8_total_upstream_length(flowdirs.data(), flowdirs.noData(), flowdirs.width(), flowdirs.height(), cx, cy, steps,
                                       length.data(), -1.0), "d8_total_upstream_length");
}
}  // namespace detail
template <class F, class G, class C>
void d8_total_upstream_length(const F &flowdirs, G &length, C *along_x, C *along_y, C *diagonal) {
  static_assert(std::is_same<detail::elem_t<C>, uint32_t>::value, "d8_total_upstream_length: the step rasters must be uint32_t");
  if (!along_x || !along_y || !diagonal)
    throw std::runtime_error("d8_total_upstream_length: the three step rasters are given together or not at all");
  const size_t n = (size_t)flowdirs.width() * (size_t)flowdirs.height();
  std::vector<uint32_t> steps(3 * n);
  detail::tlen_run(flowdirs, length, steps.data());
  C *planes[3] = {along_x, along_y, diagonal};
  for (int k = 0; k < 3; k++) {
    planes[k]->resize(flowdirs);
    planes[k]->setNoData(0xFFFFFFFFu);
    for (size_t i = 0; i < n; i++) planes[k]->data()[i] = steps[k * n + i];
  }
}
template <class F, class G>
void d8_total_upstream_length(const F &flowdirs, G &length) {
  detail::tlen_run(flowdirs, length, nullptr);
}

// ---- limited accumulation on the D8 forest: losses, decay and capacity (the definition is in rdgpu.h) ----------------
namespace detail {
inline int c_limited(const uint8_t *d, uint8_t dnd, const float *s, float snd, const float *cap, const float *fac, int w, int h,
                     double *out, double *kept, double ond, rdgpu_limited_result *r) {
  return rdgpu_d8_flow_accum_limited_f32(d, dnd, s, snd, cap, fac, w, h, out, kept, ond, r);
}
inline int c_limited(const uint8_t *d, uint8_t dnd, const double *s, double snd, const double *cap, const double *fac, int w, int h,
                     double *out, double *kept, double ond, rdgpu_limited_result *r) {
  return rdgpu_d8_flow_accum_limited_f64(d, dnd, s, snd, cap, fac, w, h, out, kept, ond, r);
}
}  // namespace detail

// Every cell passes on out = min(max(factor * total, 0), max(capacity, 0)) of the total that reached it along the GIVEN
// directions, its own supply included, and keeps the rest: a negative supply is a storage deficit that inflow fills first
// (the descent of richdem::dephier::MoveWaterIntoPits), `factor` a decay, `capacity` a transport limit.  supply is float or
// double; capacity and factor (each may be null; a NaN cell means "none here") have its type and size.  *out and *kept
// (double; each may be null) take the directions' size, geotransform and projection; their NoData, written where the
// direction is NoData, is *out's if it has been set, else *kept's, and defaults to -1.  Returns the four sums of the mass
// balance: supplied = left + kept_pos + kept_neg.
template <class F, class V, class G>
rdgpu_limited_result d8_flow_accum_limited(const F &flowdirs, const V &supply, const V *capacity, const V *factor, G *out, G *kept) {
  using T = detail::elem_t<const V>;
  static_assert(std::is_same<detail::elem_t<const F>, uint8_t>::value || std::is_same<detail::elem_t<F>, uint8_t>::value,
                "d8_flow_accum_limited: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value,
                "d8_flow_accum_limited: supply, capacity and factor are float or double");
  static_assert(std::is_same<detail::elem_t<G>, double>::value, "d8_flow_accum_limited: the out and kept rasters must be double");
  for (const V *a : {&supply, capacity, factor})
    if (a && (a->width() != flowdirs.width() || a->height() != flowdirs.height()))
      throw std::runtime_error("d8_flow_accum_limited: supply, capacity and factor must have the directions' size");
  const double nodata_out = out ? out->noData() : kept ? kept->noData() : -1.0;
  for (G *g : {out, kept})
    if (g) {
      g->resize(flowdirs);
      g->setNoData(nodata_out);
    }
  rdgpu_limited_result r = {0.0, 0.0, 0.0, 0.0};
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return r;
  detail::check(detail::c_limited(flowdirs.data(), flowdirs.noData(), (const T *)supply.data(), (T)supply.noData(),
                                  capacity ? (const T *)capacity->data() : nullptr, factor ? (const T *)factor->data() : nullptr,
                                  flowdirs.width(), flowdirs.height(), out ? out->data() : nullptr, kept ? kept->data() : nullptr,
                                  nodata_out, &r), "d8_flow_accum_limited");
  return r;
}

// ---- upslope extremes on the D8 forest (no reference counterpart; the definition is in rdgpu.h) ----------------------
namespace detail {
#define RDGPU_SHIM_EXTREME(SUF, T)                                                                                      \
  inline int c_extreme(const uint8_t *d, uint8_t dnd, const T *v, T vnd, int w, int h, int which, T *e, uint32_t *at) { \
    return rdgpu_d8_upslope_extreme_##SUF(d, dnd, v, vnd, w, h, which, e, at);                                          \
  }
RDGPU_SHIM_EXTREME(u8, uint8_t) RDGPU_SHIM_EXTREME(i8, int8_t) RDGPU_SHIM_EXTREME(u16, uint16_t) RDGPU_SHIM_EXTREME(i16, int16_t)
RDGPU_SHIM_EXTREME(u32, uint32_t) RDGPU_SHIM_EXTREME(i32, int32_t) RDGPU_SHIM_EXTREME(f32, float)
#undef RDGPU_SHIM_EXTREME
template <class T>
int c_extreme(const uint8_t *, uint8_t, const T *, T, int, int, int, T *, uint32_t *) { unsupported("d8_upslope_extreme"); }
}  // namespace detail

// extreme <- the largest (which == RDGPU_EXTREME_MAX) or smallest (RDGPU_EXTREME_MIN) value of `values` over everything that
// drains through each cell, the cell included; *at_cell (optional, uint32_t) <- the flat index of the cell it sits at, the
// lowest such index on a tie, NoData 0xFFFFFFFF.  Cells whose value is the values' NoData (or a NaN) contribute nothing;
// where nothing contributes, or the direction is NoData, extreme is the values' NoData.  Both outputs take the directions'
// size, geotransform and projection.  Element types: int8 .. uint32 and float; 64-bit values throw.
namespace detail {
template <class F, class V, class E>
void extreme_prepare(const F &flowdirs, const V &values, E &extreme, int which) {
  using T = elem_t<const V>;
  static_assert(std::is_same<elem_t<const F>, uint8_t>::value || std::is_same<elem_t<F>, uint8_t>::value,
                "d8_upslope_extreme: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<elem_t<E>, T>::value, "d8_upslope_extreme: the extreme raster has the values' element type");
  if (values.width() != flowdirs.width() || values.height() != flowdirs.height())
    throw std::runtime_error("d8_upslope_extreme: the values must have the directions' size");
  if (which != RDGPU_EXTREME_MAX && which != RDGPU_EXTREME_MIN)
    throw std::runtime_error("d8_upslope_extreme: which must be RDGPU_EXTREME_MAX or RDGPU_EXTREME_MIN");
  extreme.resize(flowdirs);
  extreme.setNoData(values.noData());
}
template <class F, class V, class E>
void extreme_run(const F &flowdirs, const V &values, E &extreme, uint32_t *at, int which) {
  using T = elem_t<const V>;
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  check(c_extreme(flowdirs.data(), flowdirs.noData(), (const T *)values.data(), (T)values.noData(), flowdirs.width(),
                  flowdirs.height(), which, (T *)extreme.data(), at), "d8_upslope_extreme");
}
}  // namespace detail
template <class F, class V, class E, class C>
void d8_upslope_extreme(const F &flowdirs, const V &values, E &extreme, C *at_cell, int which = RDGPU_EXTREME_MAX) {
  static_assert(std::is_same<detail::elem_t<C>, uint32_t>::value, "d8_upslope_extreme: the cell raster must be uint32_t");
  detail::extreme_prepare(flowdirs, values, extreme, which);
  if (at_cell) {
    at_cell->resize(flowdirs);
    at_cell->setNoData(0xFFFFFFFFu);
  }
  detail::extreme_run(flowdirs, values, extreme, at_cell ? at_cell->data() : nullptr, which);
}
template <class F, class V, class E>
void d8_upslope_extreme(const F &flowdirs, const V &values, E &extreme, int which = RDGPU_EXTREME_MAX) {
  detail::extreme_prepare(flowdirs, values, extreme, which);
  detail::extreme_run(flowdirs, values, extreme, nullptr, which);
}

// ---- depression breaching (depressions/Lindsay2016.hpp, depressions/depressions.hpp:24) ---------------------------------
namespace detail {
#define RDGPU_SHIM_BREACH(SUF, T)                                                                                          \
  inline int c_breach(T *z, T nd, int w, int h, uint8_t *dirs, uint8_t *path) { return rdgpu_breach_d8_##SUF(z, nd, 1, w, h, dirs, path); } \
  inline int c_breach_along(const uint8_t *d, uint8_t dnd, const T *z, const uint8_t *p, int w, int h, T *out, uint8_t *path) { \
    return rdgpu_d8_breach_along_##SUF(d, dnd, z, p, w, h, out, path);                                                     \
  }
RDGPU_SHIM_BREACH(u8, uint8_t) RDGPU_SHIM_BREACH(i8, int8_t) RDGPU_SHIM_BREACH(u16, uint16_t) RDGPU_SHIM_BREACH(i16, int16_t)
RDGPU_SHIM_BREACH(u32, uint32_t) RDGPU_SHIM_BREACH(i32, int32_t) RDGPU_SHIM_BREACH(f32, float)
#undef RDGPU_SHIM_BREACH
template <class T>
int c_breach(T *, T, int, int, uint8_t *, uint8_t *) { unsupported("CompleteBreaching_Lindsay2016"); }
template <class T>
int c_breach_along(const uint8_t *, uint8_t, const T *, const uint8_t *, int, int, T *, uint8_t *) { unsupported("d8_breach_along"); }
}  // namespace detail

// richdem::CompleteBreaching_Lindsay2016<topo>(Array2D<T>&)   depressions/Lindsay2016.hpp:48-178: in place, equal to the
// reference, equal elevations included (rdgpu.h; rdgpu_breach_get_stats relays the tie order's passes).  D8 and element types
// int8 .. uint32 and float; D4 and the 64-bit types throw, and so does a DEM that holds its NoData value (the reference seeds
// the cells next to NoData: not built).
template <auto topo, class A>
void CompleteBreaching_Lindsay2016(A &dem) {
  using T = detail::elem_t<A>;
  if (detail::topology_code<topo>() != 8)
    throw std::runtime_error("CompleteBreaching_Lindsay2016: topology D4 is not supported by the MI355X engine");
  if (dem.width() == 0 || dem.height() == 0) return;
  detail::check(detail::c_breach((T *)dem.data(), (T)dem.noData(), dem.width(), dem.height(), nullptr, nullptr),
                "CompleteBreaching_Lindsay2016");
  rdgpu_breach_stats st;
  if (rdgpu_breach_get_stats(&st) == 0 && st.unresolved != 0)
    std::fprintf(stderr, "W CompleteBreaching_Lindsay2016: the order of %llu of %u equal-elevation cells had not settled when the "
                         "tie-order passes were stopped (RDGPU_PFD_TIE_PASSES / RDGPU_PFD_TIE_SECONDS); the breach paths are the "
                         "reference's only where those ties do not decide\n", (unsigned long long)st.unresolved, st.twins);
}

// richdem::BreachDepressions<topo>(Array2D<T>&)               depressions/depressions.hpp:24
template <auto topo, class A>
void BreachDepressions(A &dem) {
  CompleteBreaching_Lindsay2016<topo>(dem);
}

// The carve along given directions (no reference counterpart; the definition is in rdgpu.h): out <- for every cell the least
// level of a pit (pits != 0) whose level reaches it down the directions over cells that are not below it, else the cell's own
// value; *path (optional, uint8_t) <- 1 where a pit's level arrived.  Both take the directions' size, geotransform and
// projection; out keeps the DEM's NoData.  Element types: int8 .. uint32 and float; 64-bit values throw.
namespace detail {
template <class F, class V, class P, class E>
void breach_along_run(const F &flowdirs, const V &dem, const P &pits, E &out, uint8_t *path) {
  using T = elem_t<const V>;
  static_assert(std::is_same<elem_t<const F>, uint8_t>::value, "d8_breach_along: flow directions must be uint8_t (d8_flowdir_t)");
  static_assert(std::is_same<elem_t<const P>, uint8_t>::value, "d8_breach_along: the pit mask must be uint8_t");
  static_assert(std::is_same<elem_t<E>, T>::value, "d8_breach_along: the output has the DEM's element type");
  if (dem.width() != flowdirs.width() || dem.height() != flowdirs.height() || pits.width() != flowdirs.width() ||
      pits.height() != flowdirs.height())
    throw std::runtime_error("d8_breach_along: the DEM and the pit mask must have the directions' size");
  out.resize(flowdirs);
  out.setNoData(dem.noData());
  if (flowdirs.width() == 0 || flowdirs.height() == 0) return;
  check(c_breach_along(flowdirs.data(), flowdirs.noData(), (const T *)dem.data(), pits.data(), flowdirs.width(), flowdirs.height(),
                       (T *)out.data(), path), "d8_breach_along");
}
}  // namespace detail
template <class F, class V, class P, class E, class Q>
void d8_breach_along(const F &flowdirs, const V &dem, const P &pits, E &out, Q *path) {
  static_assert(std::is_same<detail::elem_t<Q>, uint8_t>::value, "d8_breach_along: the path raster must be uint8_t");
  if (path) {
    path->resize(flowdirs);
    path->setNoData((uint8_t)255);
  }
  detail::breach_along_run(flowdirs, dem, pits, out, path && flowdirs.width() && flowdirs.height() ? path->data() : nullptr);
}
template <class F, class V, class P, class E>
void d8_breach_along(const F &flowdirs, const V &dem, const P &pits, E &out) {
  detail::breach_along_run(flowdirs, dem, pits, out, nullptr);
}

// ---- depression inventory (no reference counterpart; the definition is in rdgpu.h) ----------------------------------
namespace detail {
#define RDGPU_SHIM_DEPR(SUF, T)                                                                                            \
  inline int c_depressions(const T *z, int w, int h, int t, int32_t *l, rdgpu_depression *tab, uint32_t cap, uint32_t *n) { \
    return rdgpu_depressions_##SUF(z, w, h, t, l, tab, cap, n);                                                            \
  }
RDGPU_SHIM_DEPR(u8, uint8_t) RDGPU_SHIM_DEPR(i8, int8_t) RDGPU_SHIM_DEPR(u16, uint16_t) RDGPU_SHIM_DEPR(i16, int16_t)
RDGPU_SHIM_DEPR(u32, uint32_t) RDGPU_SHIM_DEPR(i32, int32_t) RDGPU_SHIM_DEPR(f32, float) RDGPU_SHIM_DEPR(f64, double)
#undef RDGPU_SHIM_DEPR
template <class T>
int c_depressions(const T *, int, int, int, int32_t *, rdgpu_depression *, uint32_t, uint32_t *) { unsupported("Depressions"); }
}  // namespace detail

// labels <- 0 on the cells FillDepressions<topo> leaves alone, 1..N on the lakes it fills (numbered by their lowest raster
// index); table[i] describes label i + 1.  NoData is an elevation like any other, as in FillDepressions.  labels takes the
// DEM's size, geotransform and projection, NoData 0.  Two calls of the engine: the sizing call, then the full one.
template <auto topo, class A, class L>
void Depressions(const A &dem, L &labels, std::vector<rdgpu_depression> &table) {
  using T = detail::elem_t<const A>;
  static_assert(std::is_same<detail::elem_t<L>, int32_t>::value, "Depressions: the label raster must be int32_t");
  labels.resize(dem, 0);
  labels.setNoData(0);
  table.clear();
  if (dem.width() == 0 || dem.height() == 0) return;
  uint32_t n = 0;
  detail::check(detail::c_depressions((const T *)dem.data(), dem.width(), dem.height(), detail::topology_code<topo>(), nullptr,
                                      nullptr, 0, &n), "Depressions");
  table.resize(n);
  uint32_t got = 0;
  detail::check(detail::c_depressions((const T *)dem.data(), dem.width(), dem.height(), detail::topology_code<topo>(),
                                      labels.data(), n ? table.data() : nullptr, n, &got), "Depressions");
  if (got != n) throw std::runtime_error("Depressions: the count changed between the sizing call and the full call");
}

// ---- depression hierarchy (richdem::dephier::GetDepressionHierarchy with the border ring as the ocean; the contract,
// which fixes every tie, is in rdgpu.h) -----------------------------------------------------------------------------
namespace detail {
#define RDGPU_SHIM_DEPHIER(SUF, T)                                                                                   \
  inline int c_dephier(const T *z, int w, int h, int t, int32_t *l, rdgpu_dephier_node *tab, uint32_t cap, uint32_t *n, \
                       uint32_t *leaves) {                                                                            \
    return rdgpu_depression_hierarchy_##SUF(z, w, h, t, l, tab, cap, n, leaves);                                      \
  }
RDGPU_SHIM_DEPHIER(u8, uint8_t) RDGPU_SHIM_DEPHIER(i8, int8_t) RDGPU_SHIM_DEPHIER(u16, uint16_t) RDGPU_SHIM_DEPHIER(i16, int16_t)
RDGPU_SHIM_DEPHIER(u32, uint32_t) RDGPU_SHIM_DEPHIER(i32, int32_t) RDGPU_SHIM_DEPHIER(f32, float)
RDGPU_SHIM_DEPHIER(f64, double) RDGPU_SHIM_DEPHIER(i64, int64_t) RDGPU_SHIM_DEPHIER(u64, uint64_t)   // (these three are refused by the engine)
#undef RDGPU_SHIM_DEPHIER
}  // namespace detail

// The merge tree of the depressions of dem: node i of the returned vector is record i (leaves first, by ascending pit index;
// RDGPU_DEPHIER_NONE marks a root's parent and a leaf's children).  labels <- the leaf a cell descends to, -1 where it
// drains off the raster; it takes the DEM's size, geotransform and projection, NoData -1.  topology is 8 or 4.  NoData of
// the DEM is an elevation like any other.  Two calls of the engine: the sizing call, then the full one.
template <class A, class L>
std::vector<rdgpu_dephier_node> DepressionHierarchy(const A &dem, int topology, L &labels) {
  using T = detail::elem_t<const A>;
  static_assert(std::is_same<detail::elem_t<L>, int32_t>::value, "DepressionHierarchy: the label raster must be int32_t");
  labels.resize(dem, -1);
  labels.setNoData(-1);
  std::vector<rdgpu_dephier_node> table;
  if (dem.width() == 0 || dem.height() == 0) return table;
  uint32_t n = 0, leaves = 0;
  detail::check(detail::c_dephier((const T *)dem.data(), dem.width(), dem.height(), topology, nullptr, nullptr, 0, &n, &leaves),
                "DepressionHierarchy");
  table.resize(n);
  uint32_t got = 0;
  detail::check(detail::c_dephier((const T *)dem.data(), dem.width(), dem.height(), topology, labels.data(),
                                  n ? table.data() : nullptr, n, &got, &leaves), "DepressionHierarchy");
  if (got != n) throw std::runtime_error("DepressionHierarchy: the count changed between the sizing call and the full call");
  return table;
}

// ---- the same with a caller-given ocean (the reference's label raster with any set of cells OCEAN) ------------------
namespace detail {
#define RDGPU_SHIM_DEPHIER_OCEAN(SUF, T)                                                                             \
  inline int c_dephier_ocean(const T *z, int w, int h, int t, const uint8_t *o, int32_t *l, rdgpu_dephier_node *tab, \
                             uint32_t cap, uint32_t *n, uint32_t *leaves) {                                          \
    return rdgpu_depression_hierarchy_ocean_##SUF(z, w, h, t, o, l, tab, cap, n, leaves);                             \
  }
RDGPU_SHIM_DEPHIER_OCEAN(u8, uint8_t) RDGPU_SHIM_DEPHIER_OCEAN(i8, int8_t) RDGPU_SHIM_DEPHIER_OCEAN(u16, uint16_t)
RDGPU_SHIM_DEPHIER_OCEAN(i16, int16_t) RDGPU_SHIM_DEPHIER_OCEAN(u32, uint32_t) RDGPU_SHIM_DEPHIER_OCEAN(i32, int32_t)
RDGPU_SHIM_DEPHIER_OCEAN(f32, float)
RDGPU_SHIM_DEPHIER_OCEAN(f64, double) RDGPU_SHIM_DEPHIER_OCEAN(i64, int64_t) RDGPU_SHIM_DEPHIER_OCEAN(u64, uint64_t)   // (refused by the engine)
#undef RDGPU_SHIM_DEPHIER_OCEAN
}  // namespace detail

// ocean: one byte per cell of the DEM, non-zero means ocean.  The border ring is ocean only where the mask says so; a mask
// without any ocean cell throws (as the reference does).  Labels are -1 on the ocean cells and on what drains into them.
template <class A, class L, class O>
std::vector<rdgpu_dephier_node> DepressionHierarchy(const A &dem, int topology, L &labels, const O &ocean) {
  using T = detail::elem_t<const A>;
  static_assert(std::is_same<detail::elem_t<L>, int32_t>::value, "DepressionHierarchy: the label raster must be int32_t");
  static_assert(std::is_same<detail::elem_t<const O>, uint8_t>::value, "DepressionHierarchy: the ocean mask must be uint8_t");
  if (ocean.width() != dem.width() || ocean.height() != dem.height())
    throw std::runtime_error("DepressionHierarchy: the ocean mask must have the DEM's size");
  labels.resize(dem, -1);
  labels.setNoData(-1);
  std::vector<rdgpu_dephier_node> table;
  if (dem.width() == 0 || dem.height() == 0) return table;
  uint32_t n = 0, leaves = 0;
  detail::check(detail::c_dephier_ocean((const T *)dem.data(), dem.width(), dem.height(), topology, (const uint8_t *)ocean.data(),
                                        nullptr, nullptr, 0, &n, &leaves), "DepressionHierarchy");
  table.resize(n);
  uint32_t got = 0;
  detail::check(detail::c_dephier_ocean((const T *)dem.data(), dem.width(), dem.height(), topology, (const uint8_t *)ocean.data(),
                                        labels.data(), n ? table.data() : nullptr, n, &got, &leaves), "DepressionHierarchy");
  if (got != n) throw std::runtime_error("DepressionHierarchy: the count changed between the sizing call and the full call");
  return table;
}

// ---- BucketFillFromEdges (misc/misc_methods.hpp:317), the reference's signature ---------------------------------------
namespace detail {
#define RDGPU_SHIM_BUCKET(SUF, T)                                                                                    \
  inline int c_bucket(const T *c, int w, int h, int t, T v, uint8_t *m, uint64_t *filled) {                          \
    return rdgpu_bucket_fill_from_edges_##SUF(c, w, h, t, v, m, filled);                                              \
  }
RDGPU_SHIM_BUCKET(u8, uint8_t) RDGPU_SHIM_BUCKET(i8, int8_t) RDGPU_SHIM_BUCKET(u16, uint16_t) RDGPU_SHIM_BUCKET(i16, int16_t)
RDGPU_SHIM_BUCKET(u32, uint32_t) RDGPU_SHIM_BUCKET(i32, int32_t) RDGPU_SHIM_BUCKET(f32, float)
RDGPU_SHIM_BUCKET(f64, double) RDGPU_SHIM_BUCKET(i64, int64_t) RDGPU_SHIM_BUCKET(u64, uint64_t)
#undef RDGPU_SHIM_BUCKET
}  // namespace detail

// set_raster <- set_value on every cell with check_raster == check_value and set_raster != set_value that such cells
// connect to one of them on the border ring (TOPO: 8 or 4).  A byte mask of `set_raster == set_value` goes to the engine;
// set_value is written where the engine set a byte.  Returns the number of cells set.
template <int TOPO, class A, class S>
uint64_t BucketFillFromEdges(const A &check_raster, S &set_raster, const detail::elem_t<const A> &check_value,
                             const detail::elem_t<S> &set_value) {
  using T = detail::elem_t<const A>;
  static_assert(TOPO == 8 || TOPO == 4, "BucketFillFromEdges: the topology is 8 or 4");
  if (check_raster.width() != set_raster.width() || check_raster.height() != set_raster.height())
    throw std::runtime_error("Rasters must have the same dimension for BucketFill!");   // (the reference's message)
  const size_t n = (size_t)check_raster.width() * check_raster.height();
  if (n == 0) return 0;
  std::vector<uint8_t> mask(n);
  for (size_t i = 0; i < n; i++) mask[i] = set_raster.data()[i] == set_value ? 1 : 0;
  const std::vector<uint8_t> before(mask);
  uint64_t filled = 0;
  detail::check(detail::c_bucket((const T *)check_raster.data(), check_raster.width(), check_raster.height(), TOPO, check_value,
                                 mask.data(), &filled), "BucketFillFromEdges");
  for (size_t i = 0; i < n; i++)
    if (mask[i] && !before[i]) set_raster.data()[i] = set_value;
  return filled;
}

// ---- fill-spill-merge (richdem::FillSpillMerge with surface water only; the contract is in rdgpu.h) ------------------
namespace detail {
#define RDGPU_SHIM_FSM(SUF, T)                                                                                       \
  inline int c_fsm(const T *z, int w, int h, const int32_t *l, const rdgpu_dephier_node *tab, uint32_t n, const double *water, \
                   double *depth, double *node_water, rdgpu_fsm_result *res) {                                        \
    return rdgpu_fill_spill_merge_##SUF(z, w, h, l, tab, n, water, depth, node_water, res);                           \
  }
RDGPU_SHIM_FSM(u8, uint8_t) RDGPU_SHIM_FSM(i8, int8_t) RDGPU_SHIM_FSM(u16, uint16_t) RDGPU_SHIM_FSM(i16, int16_t)
RDGPU_SHIM_FSM(u32, uint32_t) RDGPU_SHIM_FSM(i32, int32_t) RDGPU_SHIM_FSM(f32, float)
RDGPU_SHIM_FSM(f64, double) RDGPU_SHIM_FSM(i64, int64_t) RDGPU_SHIM_FSM(u64, uint64_t)   // (these three are refused by the engine)
#undef RDGPU_SHIM_FSM
}  // namespace detail

// Routes the water of wtd (one double per cell, finite and >= 0: surface water only) through the hierarchy that
// DepressionHierarchy(dem, topology, labels) returned and rewrites wtd in place, as the reference does: the depth of the
// standing water per cell, 0 where none stands.  One hierarchy serves any number of calls.  node_water, where given,
// takes the water of every node of the table.
template <class A, class L, class W>
rdgpu_fsm_result FillSpillMerge(const A &dem, const L &labels, const std::vector<rdgpu_dephier_node> &table, W &wtd,
                                std::vector<double> *node_water = nullptr) {
  using T = detail::elem_t<const A>;
  static_assert(std::is_same<detail::elem_t<const L>, int32_t>::value, "FillSpillMerge: the label raster must be int32_t");
  static_assert(std::is_same<detail::elem_t<W>, double>::value, "FillSpillMerge: the water raster must be double");
  rdgpu_fsm_result res = {};
  if (dem.width() == 0 || dem.height() == 0) return res;
  if (labels.width() != dem.width() || labels.height() != dem.height() || wtd.width() != dem.width() || wtd.height() != dem.height())
    throw std::runtime_error("FillSpillMerge: the label and water rasters must have the DEM's size");
  const std::vector<double> water(wtd.data(), wtd.data() + (size_t)dem.width() * dem.height());   // (depth must not overlap water)
  if (node_water) node_water->assign(table.size(), 0.0);
  detail::check(detail::c_fsm((const T *)dem.data(), dem.width(), dem.height(), (const int32_t *)labels.data(),
                              table.empty() ? nullptr : table.data(), (uint32_t)table.size(), water.data(), wtd.data(),
                              node_water && !table.empty() ? node_water->data() : nullptr, &res), "FillSpillMerge");
  return res;
}

}  // namespace rdgpu
