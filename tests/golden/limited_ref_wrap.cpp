// tests/golden/limited_ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY (make_golden_limited.py).
//
// An extern "C" entry over the UNMODIFIED reference's depressions/depression_hierarchy.hpp and
// depressions/fill_spill_merge.hpp, compiled by make_golden_limited.py into a temporary directory with the flags of
// oracle/Makefile: GetDepressionHierarchy<T, D8> once, then, for each of `count` water-table rasters, ResetDH and
// MoveWaterIntoPits alone (the descent, without the spill and the fill that FillSpillMerge runs after it).  The caller
// labels the border ring OCEAN and everything else NO_DEP.  Written back: the labels and the flow directions of the
// hierarchy, every wtd raster in place, and water_vol[k * stride + d] of depression d (0: the ocean) after raster k.
// Returns the number of depressions, the ocean included; nothing per depression is written when it exceeds `stride`.
#include <richdem/common/Array2D.hpp>
#include <richdem/depressions/depression_hierarchy.hpp>
#include <richdem/depressions/fill_spill_merge.hpp>

#include <cstddef>
#include <cstdint>

using namespace richdem;
using namespace richdem::dephier;

template <class T>
static int run(const T *dem, int w, int h, uint32_t *label, int8_t *dirs, double *wtd, int count, double *water_vol, int stride) {
  Array2D<T> d(const_cast<T *>(dem), w, h);
  Array2D<dh_label_t> lab(label, w, h);
  Array2D<flowdir_t> flowdirs(dirs, w, h);
  flowdirs.setAll((flowdir_t)0);
  auto deps = GetDepressionHierarchy<T, Topology::D8>(d, lab, flowdirs);
  if ((int)deps.size() > stride) return (int)deps.size();
  for (int k = 0; k < count; k++) {
    Array2D<double> water(wtd + (size_t)k * w * h, w, h);
    ResetDH(deps);
    MoveWaterIntoPits(d, lab, flowdirs, deps, water);
    for (size_t i = 0; i < deps.size(); i++) water_vol[(size_t)k * stride + i] = deps[i].water_vol;
  }
  return (int)deps.size();
}

extern "C" int limref_i32(const int32_t *dem, int w, int h, uint32_t *label, int8_t *dirs, double *wtd, int count, double *water_vol,
                          int stride) {
  return run(dem, w, h, label, dirs, wtd, count, water_vol, stride);
}
extern "C" int limref_f32(const float *dem, int w, int h, uint32_t *label, int8_t *dirs, double *wtd, int count, double *water_vol,
                          int stride) {
  return run(dem, w, h, label, dirs, wtd, count, water_vol, stride);
}
