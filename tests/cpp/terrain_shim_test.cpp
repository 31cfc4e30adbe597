// tests/cpp/terrain_shim_test.cpp -- the TerrainAttribute part of include/rdgpu/richdem_gpu.hpp: the reference's side
// effects (output resized, geotransform / projection copied, the output's NoData KEPT, SPI / CTI NoData -1) and its
// exceptions.  Values are checked against tests/golden/ref_terrain.npz by the Python tests; here: a raster whose answers
// are known in closed form.  Built by tests/cpp/Makefile.terrain.
#include <cmath>
#include <cstdio>
#include <string>

#include "rdgpu/Array2D.hpp"
#include "rdgpu/richdem_gpu.hpp"

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } \
  } while (0)

template <class F>
static std::string thrown(F &&f) {
  try { f(); } catch (const std::exception &e) { return e.what(); }
  return "";
}

int main() {
  using rdgpu::Array2D;
  // a plane z = 3x + 4y on 2 x 5 cells: dzdx = 3/2, dzdy = 4/5 in the interior, rise/run = 1.7
  Array2D<int32_t> dem(7, 5, 0);
  for (int y = 0; y < 5; y++)
    for (int x = 0; x < 7; x++) dem.data()[y * 7 + x] = 3 * x + 4 * y;
  dem.setNoData(-7);
  dem.data()[0] = -7;
  dem.geotransform = {100.0, 2.0, 0.0, 200.0, 0.0, -5.0};
  dem.projection = "a projection";
  Array2D<float> out(2, 2, 1.0f);
  out.setNoData(-1234.0f);
  rdgpu::TA_slope_riserun(dem, out);
  CHECK(out.width() == 7 && out.height() == 5);
  CHECK(out.geotransform == dem.geotransform && out.projection == dem.projection);
  CHECK(out.noData() == -1234.0f);                     // resize() keeps the output's own NoData
  CHECK(out.data()[0] == -1234.0f);                    // and NoData cells receive it
  CHECK(out.data()[2 * 7 + 3] == (float)std::sqrt(1.5 * 1.5 + 0.8 * 0.8));
  rdgpu::TA_slope_percentage(dem, out, 2.0f);          // zscale doubles the slope
  CHECK(out.data()[2 * 7 + 3] == (float)(std::sqrt(3.0 * 3.0 + 1.6 * 1.6) * 100));
  rdgpu::TA_curvature(dem, out);
  CHECK(out.data()[2 * 7 + 3] == 0.0f);
  rdgpu::TA_planform_curvature(dem, out);
  CHECK(out.data()[2 * 7 + 3] == 0.0f);
  rdgpu::TA_profile_curvature(dem, out);
  CHECK(out.data()[2 * 7 + 3] == 0.0f);
  rdgpu::TA_slope_degrees(dem, out);
  CHECK(std::fabs(out.data()[2 * 7 + 3] - std::atan(1.7) * 180 / M_PI) < 1e-5);
  rdgpu::TA_slope_radians(dem, out);
  CHECK(std::fabs(out.data()[2 * 7 + 3] - std::atan(1.7)) < 1e-6);
  Array2D<uint8_t> level(4, 3, 9);
  level.setNoData(0);
  level.geotransform = {0, 1, 0, 0, 0, -1};
  Array2D<float> asp;
  rdgpu::TA_aspect(level, asp);
  CHECK(asp.width() == 4 && asp.height() == 3 && asp.data()[5] == 270.0f);   // the reference's level-window aspect
  // an empty geotransform raises (the reference asserts; under NDEBUG it reads past the vector)
  Array2D<float> nogt(4, 4, 1.0f);
  CHECK(thrown([&] { rdgpu::TA_aspect(nogt, asp); }).find("geotransform") != std::string::npos);
  // SPI / CTI
  Array2D<double> acc(7, 5, 8.0);
  acc.setNoData(-1.0);
  acc.data()[3] = -1.0;
  acc.geotransform = dem.geotransform;
  acc.projection = "acc projection";
  Array2D<float> slope(7, 5, 0.999f);
  slope.setNoData(-9999.0f);
  slope.data()[4] = -9999.0f;
  Array2D<float> spi, cti;
  spi.setNoData(55.0f);
  rdgpu::TA_SPI(acc, slope, spi);
  rdgpu::TA_CTI(acc, slope, cti);
  CHECK(spi.width() == 7 && spi.height() == 5 && spi.noData() == -1.0f && cti.noData() == -1.0f);
  CHECK(spi.geotransform == acc.geotransform && spi.projection == acc.projection);
  CHECK(spi.data()[3] == -1.0f && spi.data()[4] == -1.0f && cti.data()[3] == -1.0f && cti.data()[4] == -1.0f);
  CHECK(std::fabs(spi.data()[10] - std::log((8.0 / 10.0) * ((double)0.999f + 0.001))) < 1e-6);
  CHECK(std::fabs(cti.data()[10] - std::log((8.0 / 10.0) / ((double)0.999f + 0.001))) < 1e-6);
  Array2D<float> small(6, 5, 1.0f);
  CHECK(thrown([&] { rdgpu::TA_SPI(acc, small, spi); }) ==
        "Couldn't calculate SPI! The input matricies were of unequal dimensions!");
  CHECK(thrown([&] { rdgpu::TA_CTI(acc, small, cti); }) ==
        "Couldn't calculate CTI! The input matricies were of unequal dimensions!");
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
