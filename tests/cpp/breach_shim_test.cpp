// tests/cpp/breach_shim_test.cpp -- the breaching part of include/rdgpu/richdem_gpu.hpp (rdgpu::BreachDepressions,
// rdgpu::CompleteBreaching_Lindsay2016, rdgpu::d8_breach_along) on rasters whose answers are known by hand; with two file
// names (an int16 native raster in, one out) it breaches the file, for tests/test_breach_shim_gpu.py to compare with the
// Python layer.  Built by tests/cpp/Makefile.breach.
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
  using rdgpu::Topology;
  if (argc == 3) {   // <DEM (int16)> <output>
    Array2D<int16_t> dem(std::string(argv[1]), true);
    rdgpu::BreachDepressions<Topology::D8>(dem);
    dem.saveToCache(std::string(argv[2]));
    std::printf("written\n");
    return 0;
  }
  // 7 x 5 of 9s with a channel of 5s along the middle row from the west edge to a two-cell flat pit of 2s; the flat cells
  // (1, 2) and (2, 2) of the channel are pits as well (an interior cell not above any neighbour)
  Array2D<int16_t> dem(7, 5, 9);
  dem.setNoData(-1);
  for (int x = 0; x < 4; x++) dem.data()[2 * 7 + x] = 5;
  dem.data()[2 * 7 + 4] = dem.data()[2 * 7 + 5] = 2;
  Array2D<int16_t> work = dem;
  rdgpu::BreachDepressions<Topology::D8>(work);
  for (int x = 0; x < 6; x++) CHECK(work.data()[2 * 7 + x] == 2);          // carved to the edge
  for (int i = 0; i < 35; i++)
    if (i / 7 != 2 || i % 7 == 6) CHECK(work.data()[i] == 9);
  rdgpu_breach_stats st;
  CHECK(rdgpu_breach_get_stats(&st) == 0 && st.pits == 4 && st.lowered == 4 && st.raised == 0 && st.unresolved == 0);
  Array2D<int16_t> again = dem;
  rdgpu::CompleteBreaching_Lindsay2016<Topology::D8>(again);
  for (int i = 0; i < 35; i++) CHECK(again.data()[i] == work.data()[i]);
  CHECK(thrown([&] { Array2D<int16_t> d4 = dem; rdgpu::BreachDepressions<Topology::D4>(d4); }).find("D4") != std::string::npos);
  CHECK(thrown([&] { Array2D<double> d(7, 5, 1.0); rdgpu::BreachDepressions<Topology::D8>(d); }).find("not supported") != std::string::npos);
  Array2D<int16_t> holed = dem;
  holed.data()[8] = -1;                                                     // a NoData cell: refused, nothing written
  CHECK(!thrown([&] { rdgpu::BreachDepressions<Topology::D8>(holed); }).empty());
  CHECK(holed.data()[2 * 7 + 1] == 5 && holed.data()[8] == -1);
  // the carve on given directions: the middle row flows west (1); a pit at (5, 2) of level 2, a cell of 1 at (2, 2) stops it
  Array2D<uint8_t> dirs(7, 5, 0), pits(7, 5, 0), path(1, 1, 9);
  dirs.setNoData(255);
  for (int x = 1; x < 7; x++) dirs.data()[2 * 7 + x] = 1;
  dirs.geotransform = {100.0, 3.0, 0.0, 200.0, 0.0, -4.0};
  dirs.projection = "a projection";
  pits.data()[2 * 7 + 5] = 1;
  Array2D<int16_t> z = dem, out(2, 2, 0);
  z.data()[2 * 7 + 2] = 1;
  rdgpu::d8_breach_along(dirs, z, pits, out, &path);
  CHECK(out.width() == 7 && out.height() == 5 && out.noData() == -1 && path.width() == 7 && path.noData() == 255);
  CHECK(out.geotransform == dirs.geotransform && out.projection == dirs.projection && path.geotransform == dirs.geotransform);
  const int exp_row[7] = {5, 5, 1, 2, 2, 2, 9};
  for (int x = 0; x < 7; x++) { CHECK(out.data()[2 * 7 + x] == exp_row[x]); CHECK(path.data()[2 * 7 + x] == (x >= 3 && x <= 5)); }
  Array2D<int16_t> only(1, 1, 0);
  rdgpu::d8_breach_along(dirs, z, pits, only);
  for (int i = 0; i < 35; i++) CHECK(only.data()[i] == out.data()[i]);
  CHECK(thrown([&] { rdgpu::d8_breach_along(dirs, Array2D<int16_t>(2, 2, 0), pits, out); }).find("directions' size") != std::string::npos);
  Array2D<double> zd(7, 5, 1.0), outd;
  CHECK(thrown([&] { rdgpu::d8_breach_along(dirs, zd, pits, outd); }).find("not supported") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
