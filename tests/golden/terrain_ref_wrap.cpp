// tests/golden/terrain_ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY (make_golden_terrain.py).
//
// extern "C" entries over the UNMODIFIED reference's methods/terrain_attributes.hpp, compiled by make_golden_terrain.py
// into a temporary directory with the flags of oracle/Makefile.  The rasters are wrapped in place with the reference's
// Array2D(T*, w, h); the cell lengths enter through the geotransform, the output's NoData is set BEFORE the call (the
// reference's resize() keeps it, as the Python wrapper's -9999 and rd_terrain_property's result(dem) rely on).
#include <richdem/common/Array2D.hpp>
#include <richdem/methods/terrain_attributes.hpp>

#include <cstdint>
#include <cstring>

using namespace richdem;

namespace {
template <class T>
void ta(const T *dem, T nodata, int w, int h, double cx, double cy, float zscale, int attr, float *out, float out_nodata) {
  Array2D<T> a(const_cast<T *>(dem), w, h);
  a.setNoData(nodata);
  a.geotransform = {0.0, cx, 0.0, 0.0, 0.0, -cy};
  Array2D<float> r;
  r.setNoData(out_nodata);
  switch (attr) {
  case 0: TA_slope_riserun(a, r, zscale); break;
  case 1: TA_slope_percentage(a, r, zscale); break;
  case 2: TA_slope_degrees(a, r, zscale); break;
  case 3: TA_slope_radians(a, r, zscale); break;
  case 4: TA_aspect(a, r, zscale); break;
  case 5: TA_curvature(a, r, zscale); break;
  case 6: TA_planform_curvature(a, r, zscale); break;
  case 7: TA_profile_curvature(a, r, zscale); break;
  }
  std::memcpy(out, r.data(), sizeof(float) * (size_t)w * h);
}
}  // namespace

#define TA_API(SUF, T)                                                                                              \
  extern "C" void tref_attribute_##SUF(const T *dem, T nodata, int w, int h, double cx, double cy, float zscale,    \
                                       int attr, float *out, float out_nodata) {                                    \
    ta<T>(dem, nodata, w, h, cx, cy, zscale, attr, out, out_nodata);                                                \
  }
TA_API(u8, uint8_t) TA_API(i8, int8_t) TA_API(u16, uint16_t) TA_API(i16, int16_t) TA_API(u32, uint32_t)
TA_API(i32, int32_t) TA_API(u64, uint64_t) TA_API(i64, int64_t) TA_API(f32, float) TA_API(f64, double)

// which = 0: TA_SPI, 1: TA_CTI; returns the output's NoData as the reference set it
extern "C" float tref_spi_cti(const double *fa, double fa_nodata, const float *slope, float slope_nodata, int w, int h,
                              double cx, double cy, int which, float *out) {
  Array2D<double> a(const_cast<double *>(fa), w, h);
  a.setNoData(fa_nodata);
  a.geotransform = {0.0, cx, 0.0, 0.0, 0.0, -cy};
  Array2D<float> s(const_cast<float *>(slope), w, h);
  s.setNoData(slope_nodata);
  Array2D<float> r;
  if (which == 0) TA_SPI(a, s, r); else TA_CTI(a, s, r);
  std::memcpy(out, r.data(), sizeof(float) * (size_t)w * h);
  return r.noData();
}
