// tests/golden/bucketfill_ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY (make_golden_dephier_ocean.py).
//
// An extern "C" entry over the UNMODIFIED reference's misc/misc_methods.hpp (BucketFillFromEdges), compiled by
// make_golden_dephier_ocean.py into a temporary directory with the flags of oracle/Makefile.  The set raster is a byte
// mask holding 0 and 1 only and set_value is 1, so the reference's `set == set_value` is `mask != 0`; the mask is
// rewritten in place.  Returns the number of bytes that changed.
#include <richdem/common/Array2D.hpp>
#include <richdem/misc/misc_methods.hpp>

#include <cstdint>
#include <vector>

using namespace richdem;

template <class T>
static long run(const T *check, int w, int h, int topology, T value, uint8_t *mask) {
  Array2D<T> c(const_cast<T *>(check), w, h);
  Array2D<uint8_t> m(mask, w, h);
  const std::vector<uint8_t> before(mask, mask + (size_t)w * h);
  if (topology == 8) BucketFillFromEdges<Topology::D8>(c, m, value, (uint8_t)1);
  else BucketFillFromEdges<Topology::D4>(c, m, value, (uint8_t)1);
  long changed = 0;
  for (size_t i = 0; i < before.size(); i++) changed += before[i] != mask[i];
  return changed;
}

#define BFREF(SUF, T)                                                                                 \
  extern "C" long bfref_##SUF(const T *check, int w, int h, int topology, T value, uint8_t *mask) { \
    return run<T>(check, w, h, topology, value, mask);                                                \
  }
BFREF(u8, uint8_t)
BFREF(u16, uint16_t)
BFREF(i32, int32_t)
BFREF(f32, float)
