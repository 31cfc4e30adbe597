// tests/golden/dephier_ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY (make_golden_dephier.py).
//
// An extern "C" entry over the UNMODIFIED reference's depressions/depression_hierarchy.hpp (GetDepressionHierarchy, which
// also runs CalculateMarginalVolumes and CalculateTotalVolumes), compiled by make_golden_dephier.py into a temporary
// directory with the flags of oracle/Makefile.  The caller labels the border ring OCEAN and everything else NO_DEP; the
// label raster is rewritten in place.  One row per depression of the reference's vector, the ocean (row 0) included;
// returns their number, or -1 when the capacity is too small.
#include <richdem/common/Array2D.hpp>
#include <richdem/depressions/depression_hierarchy.hpp>

#include <cstdint>

using namespace richdem;
using namespace richdem::dephier;

template <class T, Topology topo>
static int run(const T *dem, int w, int h, uint32_t *label, int cap, uint32_t *u32x7, double *f64x3) {
  Array2D<T> d(const_cast<T *>(dem), w, h);
  Array2D<dh_label_t> lab(label, w, h);
  Array2D<int8_t> flowdirs(w, h, (int8_t)0);
  const auto deps = GetDepressionHierarchy<T, topo>(d, lab, flowdirs);
  if ((int)deps.size() > cap) return -1;
  for (size_t i = 0; i < deps.size(); i++) {
    const auto &p = deps[i];
    uint32_t *u = u32x7 + 7 * i;
    u[0] = p.parent; u[1] = p.lchild; u[2] = p.rchild; u[3] = p.pit_cell; u[4] = p.out_cell; u[5] = p.geolink;
    u[6] = (p.ocean_parent ? 1u : 0u) | (p.cell_count << 1);
    double *f = f64x3 + 3 * i;
    f[0] = (double)p.out_elev; f[1] = (double)p.pit_elev; f[2] = p.dep_vol;
  }
  return (int)deps.size();
}

#define DHREF(SUF, T)                                                                                                  \
  extern "C" int dhref_##SUF(const T *dem, int w, int h, int topology, uint32_t *label, int cap, uint32_t *u, double *f) { \
    return topology == 8 ? run<T, Topology::D8>(dem, w, h, label, cap, u, f) : run<T, Topology::D4>(dem, w, h, label, cap, u, f); \
  }
DHREF(u16, uint16_t)
DHREF(i32, int32_t)
DHREF(f32, float)
