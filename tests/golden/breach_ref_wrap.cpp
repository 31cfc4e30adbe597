// tests/golden/breach_ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY (make_golden_breach.py).
//
// An extern "C" entry over the UNMODIFIED reference's depressions/Lindsay2016.hpp, compiled by make_golden_breach.py into a
// temporary directory with the flags of oracle/Makefile: CompleteBreaching_Lindsay2016<Topology::D8> in place on the caller's
// raster.  nodata is a value the caller has checked to be absent from the raster (an Array2D always has one).
#include <richdem/common/Array2D.hpp>
#include <richdem/depressions/Lindsay2016.hpp>

#include <cstdint>

using namespace richdem;

template <class T>
static void run(T *dem, int w, int h, T nodata) {
  Array2D<T> d(dem, w, h);
  d.setNoData(nodata);
  CompleteBreaching_Lindsay2016<Topology::D8>(d);
}

#define BREACH_REF(SUF, T) \
  extern "C" void breachref_##SUF(T *dem, int w, int h, T nodata) { run<T>(dem, w, h, nodata); }
BREACH_REF(u8, uint8_t)
BREACH_REF(i8, int8_t)
BREACH_REF(u16, uint16_t)
BREACH_REF(i16, int16_t)
BREACH_REF(u32, uint32_t)
BREACH_REF(i32, int32_t)
BREACH_REF(f32, float)
