// tests/cpp/weighted_shim_test.cpp -- the weighted-accumulation part of include/rdgpu/richdem_gpu.hpp
// (rdgpu::d8_flow_accum_weighted, rdgpu::d8_total_upstream_length) on a raster whose answers are known by hand; with file
// names (directions, weights: native rasters, float weights) it also writes <prefix>_sum / <prefix>_length / <prefix>_nx,
// _ny, _nd for tests/test_weighted_accum_shim_gpu.py to compare with the Python layer.  Built by
// tests/cpp/Makefile.weighted.
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
  if (argc == 4) {   // <directions> <weights (float)> <prefix>
    Array2D<uint8_t> dirs(std::string(argv[1]), true);
    Array2D<float> weights(std::string(argv[2]), true);
    Array2D<double> sum, length;
    Array2D<uint32_t> nx, ny, nd;
    sum.setNoData(-5.0);
    rdgpu::d8_flow_accum_weighted(dirs, weights, sum);
    rdgpu::d8_total_upstream_length(dirs, length, &nx, &ny, &nd);
    const std::string prefix(argv[3]);
    sum.saveToCache(prefix + "_sum");
    length.saveToCache(prefix + "_length");
    nx.saveToCache(prefix + "_nx");
    ny.saveToCache(prefix + "_ny");
    nd.saveToCache(prefix + "_nd");
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
  // weights: 10 * (row + 1) + column, one of them NoData
  Array2D<int16_t> wts(5, 3, 0);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 5; x++) wts.data()[5 * y + x] = (int16_t)(10 * (y + 1) + x);
  wts.setNoData(-1);
  wts.data()[14] = -1;
  Array2D<int64_t> sum(2, 2, 9);
  rdgpu::d8_flow_accum_weighted(dirs, wts, sum);
  CHECK(sum.width() == 5 && sum.height() == 3 && sum.noData() == -1);
  CHECK(sum.geotransform == dirs.geotransform && sum.projection == dirs.projection);
  // (x, 1) collects (x - 1, 0), (x, 2) and (x - 1, 1)'s total; (4, 1) also (4, 0); (4, 2) has a NoData weight and adds 0
  const int64_t exp[15] = {10, 11, 12, 13, 14, 20, 82, 147, 215, 266, -1, 31, 32, 33, 0};
  for (int i = 0; i < 15; i++) CHECK(sum.data()[i] == exp[i]);
  sum.setNoData(-77);   // a NoData of the caller's is kept
  rdgpu::d8_flow_accum_weighted(dirs, wts, sum);
  CHECK(sum.noData() == -77 && sum.data()[10] == -77 && sum.data()[9] == 266);
  Array2D<float> wf(5, 3, 0.5f);
  wf.setNoData(-9999.0f);
  wf.data()[7] = -9999.0f;
  Array2D<double> sumd;
  rdgpu::d8_flow_accum_weighted(dirs, wf, sumd);
  CHECK(sumd.data()[5] == 0.5 && sumd.data()[6] == 2.0 && sumd.data()[7] == 3.0 && sumd.data()[10] == -1.0 && sumd.noData() == -1.0);
  Array2D<double> wd(5, 3, 0.25), sumdd;
  wd.setNoData(-1.0);
  rdgpu::d8_flow_accum_weighted(dirs, wd, sumdd);
  CHECK(sumdd.data()[6] == 1.0 && sumdd.data()[9] == 3.5);
  // the links above (x, 1): x along x, x along y (one more at (4, 1): (4, 0) flows south), x diagonal; 3, 4, 5 long
  Array2D<double> length(1, 1, 0.0);
  Array2D<uint32_t> nx, ny, nd;
  rdgpu::d8_total_upstream_length(dirs, length, &nx, &ny, &nd);
  CHECK(length.width() == 5 && length.height() == 3 && length.noData() == -1.0 && nx.noData() == 0xFFFFFFFFu);
  CHECK(length.geotransform == dirs.geotransform && nd.geotransform == dirs.geotransform && ny.projection == dirs.projection);
  const double explen[15] = {0, 0, 0, 0, 0, 0, 12, 24, 36, 52, -1, 0, 0, 0, 0};
  const uint32_t N = 0xFFFFFFFFu;
  const uint32_t expx[15] = {0, 0, 0, 0, 0, 0, 1, 2, 3, 4, N, 0, 0, 0, 0}, expy[15] = {0, 0, 0, 0, 0, 0, 1, 2, 3, 5, N, 0, 0, 0, 0};
  for (int i = 0; i < 15; i++) {
    CHECK(length.data()[i] == explen[i]);
    CHECK(nx.data()[i] == expx[i] && ny.data()[i] == expy[i] && nd.data()[i] == expx[i]);
  }
  Array2D<double> only;
  rdgpu::d8_total_upstream_length(dirs, only);   // without the step rasters
  for (int i = 0; i < 15; i++) CHECK(only.data()[i] == explen[i]);
  CHECK(thrown([&] { rdgpu::d8_flow_accum_weighted(dirs, Array2D<int16_t>(2, 2, 0), sum); }).find("directions' size") != std::string::npos);
  Array2D<int64_t> w64(5, 3, 1), sum64;
  CHECK(thrown([&] { rdgpu::d8_flow_accum_weighted(dirs, w64, sum64); }).find("not supported") != std::string::npos);   // 64-bit weights
  CHECK(thrown([&] { rdgpu::d8_total_upstream_length(dirs, only, &nx, &ny, (Array2D<uint32_t> *)nullptr); }).find("together") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
