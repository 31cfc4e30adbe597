// tests/cpp/extreme_shim_test.cpp -- the upslope-extreme part of include/rdgpu/richdem_gpu.hpp (rdgpu::d8_upslope_extreme)
// on a raster whose answers are known by hand; with two file names (directions, values: native rasters, float values) it
// also writes <prefix>_extreme / <prefix>_at_cell for the mode given, for tests/test_upslope_extreme_shim_gpu.py to compare
// with the Python layer.  Built by tests/cpp/Makefile.extreme.
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

int main(int argc, char **argv) {
  using rdgpu::Array2D;
  if (argc == 5) {   // <directions> <values (float)> <prefix> <max|min>
    Array2D<uint8_t> dirs(std::string(argv[1]), true);
    Array2D<float> values(std::string(argv[2]), true), extreme;
    Array2D<uint32_t> at;
    rdgpu::d8_upslope_extreme(dirs, values, extreme, &at, std::string(argv[4]) == "min" ? RDGPU_EXTREME_MIN : RDGPU_EXTREME_MAX);
    extreme.saveToCache(std::string(argv[3]) + "_extreme");
    at.saveToCache(std::string(argv[3]) + "_at_cell");
    std::printf("written\n");
    return 0;
  }
  // 5 x 3: the middle row flows east (5) to a NO_FLOW cell in the last column; the top row flows south-east (6) into it,
  // the bottom row north (3); (0, 2) is NoData.
  Array2D<uint8_t> dirs(5, 3, 5);
  for (int x = 0; x < 5; x++) { dirs.data()[x] = 6; dirs.data()[10 + x] = 3; }
  dirs.data()[4] = 7;           // (4, 0): south-east would leave the raster; south instead
  dirs.data()[5 + 4] = 0;
  dirs.setNoData(255);
  dirs.data()[10] = 255;
  dirs.geotransform = {100.0, 3.0, 0.0, 200.0, 0.0, -4.0};
  dirs.projection = "a projection";
  // values: 10 * (row + 1) + column, one of them NoData
  Array2D<int16_t> vals(5, 3, 0);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 5; x++) vals.data()[5 * y + x] = (int16_t)(10 * (y + 1) + x);
  vals.setNoData(-1);
  vals.data()[14] = -1;
  Array2D<int16_t> ext(2, 2, 9);
  Array2D<uint32_t> at(1, 1, 9);
  rdgpu::d8_upslope_extreme(dirs, vals, ext, &at);   // the maximum
  CHECK(ext.width() == 5 && ext.height() == 3 && ext.noData() == -1 && at.width() == 5 && at.height() == 3 && at.noData() == 0xFFFFFFFFu);
  CHECK(ext.geotransform == dirs.geotransform && ext.projection == dirs.projection && at.geotransform == dirs.geotransform);
  // (x, 1) collects (x - 1, 0), (x, 2) and (x - 1, 1)'s upslope set: the largest is in the bottom row, 30 + x, but (4, 2) is
  // NoData-valued and (0, 2) has a NoData direction
  const int expmax[15] = {10, 11, 12, 13, 14, 20, 31, 32, 33, 33, -1, 31, 32, 33, -1};
  const uint32_t atmax[15] = {0, 1, 2, 3, 4, 5, 11, 12, 13, 13, 0xFFFFFFFFu, 11, 12, 13, 0xFFFFFFFFu};
  for (int i = 0; i < 15; i++) { CHECK(ext.data()[i] == expmax[i]); CHECK(at.data()[i] == atmax[i]); }
  rdgpu::d8_upslope_extreme(dirs, vals, ext, &at, RDGPU_EXTREME_MIN);
  const int expmin[15] = {10, 11, 12, 13, 14, 20, 10, 10, 10, 10, -1, 31, 32, 33, -1};
  const uint32_t atmin[15] = {0, 1, 2, 3, 4, 5, 0, 0, 0, 0, 0xFFFFFFFFu, 11, 12, 13, 0xFFFFFFFFu};
  for (int i = 0; i < 15; i++) { CHECK(ext.data()[i] == expmin[i]); CHECK(at.data()[i] == atmin[i]); }
  Array2D<int16_t> only(1, 1, 0);
  rdgpu::d8_upslope_extreme(dirs, vals, only, RDGPU_EXTREME_MIN);   // without the cell raster
  for (int i = 0; i < 15; i++) CHECK(only.data()[i] == expmin[i]);
  Array2D<float> valf(5, 3, 1.5f), extf;
  valf.setNoData(-9999.0f);
  valf.data()[7] = 8.25f;
  rdgpu::d8_upslope_extreme(dirs, valf, extf);
  CHECK(extf.data()[6] == 1.5f && extf.data()[7] == 8.25f && extf.data()[9] == 8.25f && extf.data()[10] == -9999.0f && extf.noData() == -9999.0f);
  CHECK(thrown([&] { rdgpu::d8_upslope_extreme(dirs, Array2D<int16_t>(2, 2, 0), ext); }).find("directions' size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::d8_upslope_extreme(dirs, vals, ext, 2); }).find("which") != std::string::npos);
  Array2D<double> vald(5, 3, 1.0), extd;
  CHECK(thrown([&] { rdgpu::d8_upslope_extreme(dirs, vald, extd); }).find("not supported") != std::string::npos);   // 64-bit values
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
