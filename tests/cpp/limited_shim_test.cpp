// tests/cpp/limited_shim_test.cpp -- the limited-accumulation part of include/rdgpu/richdem_gpu.hpp
// (rdgpu::d8_flow_accum_limited) on a raster whose answers are known by hand; with file names (directions, supply, capacity,
// factor: native rasters, float) it also writes <prefix>_out / <prefix>_kept and prints the four sums for
// tests/test_limited_accum_shim_gpu.py to compare with the Python layer.  Built by tests/cpp/Makefile.limited.
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
  if (argc == 6) {   // <directions> <supply> <capacity> <factor> <prefix>
    Array2D<uint8_t> dirs(std::string(argv[1]), true);
    Array2D<float> supply(std::string(argv[2]), true), capacity(std::string(argv[3]), true), factor(std::string(argv[4]), true);
    Array2D<double> out, kept;
    out.setNoData(-5.0);
    const rdgpu_limited_result r = rdgpu::d8_flow_accum_limited(dirs, supply, &capacity, &factor, &out, &kept);
    const std::string prefix(argv[5]);
    out.saveToCache(prefix + "_out");
    kept.saveToCache(prefix + "_kept");
    std::printf("written %.17g %.17g %.17g %.17g\n", r.supplied, r.left, r.kept_pos, r.kept_neg);
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
  // every cell supplies 1, (1, 1) has a deficit of 5; (3, 1) passes on 2 at the most
  Array2D<double> supply(5, 3, 1.0), capacity(5, 3, std::numeric_limits<double>::quiet_NaN());
  supply.setNoData(-9999.0);
  supply.data()[6] = -5.0;
  capacity.data()[8] = 2.0;
  Array2D<double> out(2, 2, 9.0), kept;
  rdgpu_limited_result r = rdgpu::d8_flow_accum_limited(dirs, supply, &capacity, (const Array2D<double> *)nullptr, &out, &kept);
  CHECK(out.width() == 5 && out.height() == 3 && out.noData() == -1.0 && kept.width() == 5 && kept.noData() == -1.0);
  CHECK(out.geotransform == dirs.geotransform && kept.projection == dirs.projection);
  // (1, 1): -5 + 3 arrive = -2, nothing moves on; (2, 1): 3; (3, 1): 6 arrive, 2 move on; (4, 1): 1 + 3 + 2 leave the system
  const double expo[15] = {1, 1, 1, 1, 1, 1, 0, 3, 2, 6, -1, 1, 1, 1, 1}, expk[15] = {0, 0, 0, 0, 0, 0, -2, 0, 4, 0, -1, 0, 0, 0, 0};
  for (int i = 0; i < 15; i++) CHECK(out.data()[i] == expo[i] && kept.data()[i] == expk[i]);
  CHECK(r.supplied == 8.0 && r.left == 6.0 && r.kept_pos == 4.0 && r.kept_neg == -2.0);
  // float rasters, a factor of one half on the outlet, kept alone with a NoData of the caller's
  Array2D<float> sf(5, 3, 1.0f), ff(5, 3, 1.0f);
  sf.setNoData(-9999.0f);
  sf.data()[6] = -5.0f;
  sf.data()[14] = -9999.0f;     // adds nothing
  ff.data()[9] = 0.5f;
  Array2D<double> keptf;
  keptf.setNoData(-77.0);
  r = rdgpu::d8_flow_accum_limited(dirs, sf, (const Array2D<float> *)nullptr, &ff, (Array2D<double> *)nullptr, &keptf);
  CHECK(keptf.noData() == -77.0 && keptf.data()[10] == -77.0 && keptf.data()[6] == -2.0 && keptf.data()[8] == 0.0);
  CHECK(keptf.data()[9] == 4.5 && r.supplied == 7.0 && r.left == 4.5 && r.kept_pos == 4.5 && r.kept_neg == -2.0);   // 9 arrive
  r = rdgpu::d8_flow_accum_limited(dirs, sf, (const Array2D<float> *)nullptr, (const Array2D<float> *)nullptr, (Array2D<double> *)nullptr,
                                   (Array2D<double> *)nullptr);   // the sums alone
  CHECK(r.supplied == 7.0 && r.left == 9.0 && r.kept_pos == 0.0 && r.kept_neg == -2.0);
  Array2D<double> small(2, 2, 0.0);
  CHECK(thrown([&] { rdgpu::d8_flow_accum_limited(dirs, small, (const Array2D<double> *)nullptr, (const Array2D<double> *)nullptr, &out, &kept); })
            .find("directions' size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::d8_flow_accum_limited(dirs, supply, &small, (const Array2D<double> *)nullptr, &out, &kept); })
            .find("directions' size") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
