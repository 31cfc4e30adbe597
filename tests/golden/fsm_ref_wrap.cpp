// tests/golden/fsm_ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY (make_golden_fsm.py).
//
// An extern "C" entry over the UNMODIFIED reference's depressions/depression_hierarchy.hpp and
// depressions/fill_spill_merge.hpp, compiled by make_golden_fsm.py into a temporary directory with the flags of
// oracle/Makefile: GetDepressionHierarchy<T, D8>, then FillSpillMerge on the same labels and flow directions.  The caller
// labels the border ring OCEAN and everything else NO_DEP, and hands in the water as `wtd` (zero on the border ring: the
// reference app's precondition); `wtd` is rewritten in place.  Returns the number of depressions, the ocean included.
#include <richdem/common/Array2D.hpp>
#include <richdem/depressions/depression_hierarchy.hpp>
#include <richdem/depressions/fill_spill_merge.hpp>

#include <cstdint>

using namespace richdem;
using namespace richdem::dephier;

template <class T>
static int run(const T *dem, int w, int h, uint32_t *label, double *wtd) {
  Array2D<T> d(const_cast<T *>(dem), w, h);
  Array2D<dh_label_t> lab(label, w, h);
  Array2D<flowdir_t> flowdirs(w, h, (flowdir_t)0);
  Array2D<double> water(wtd, w, h);
  auto deps = GetDepressionHierarchy<T, Topology::D8>(d, lab, flowdirs);
  FillSpillMerge(d, lab, flowdirs, deps, water);
  return (int)deps.size();
}

extern "C" int fsmref_i32(const int32_t *dem, int w, int h, uint32_t *label, double *wtd) { return run(dem, w, h, label, wtd); }
extern "C" int fsmref_f32(const float *dem, int w, int h, uint32_t *label, double *wtd) { return run(dem, w, h, label, wtd); }
