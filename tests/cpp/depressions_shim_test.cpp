// tests/cpp/depressions_shim_test.cpp -- rdgpu::Depressions<topo> of include/rdgpu/richdem_gpu.hpp on rasters whose
// answers are known by hand (the same ones as tests/test_depression_model.py).  Built by tests/cpp/Makefile.depressions.
#include <cstdio>
#include <string>
#include <vector>

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

static bool same(const rdgpu_depression &d, uint32_t first, uint32_t pit, uint32_t outlet, uint32_t cells, double level,
                 double pit_elevation, double volume) {
  return d.first_cell == first && d.pit_cell == pit && d.outlet_cell == outlet && d.cells == cells && d.level == level &&
         d.pit_elevation == pit_elevation && d.volume == volume;
}

int main() {
  using rdgpu::Array2D;
  // 4 x 4: two pits (1 at cell 5, 2 at cell 10) that touch only diagonally
  Array2D<float> dem(4, 4, 9.0f);
  dem.data()[5] = 1.0f;
  dem.data()[10] = 2.0f;
  dem.geotransform = {100.0, 2.0, 0.0, 200.0, 0.0, -2.0};
  dem.projection = "a projection";
  Array2D<int32_t> labels(2, 2, 7);
  std::vector<rdgpu_depression> table(3);
  rdgpu::Depressions<rdgpu::Topology::D8>(dem, labels, table);
  CHECK(labels.width() == 4 && labels.height() == 4 && labels.noData() == 0);
  CHECK(labels.geotransform == dem.geotransform && labels.projection == dem.projection);
  CHECK(table.size() == 1 && same(table[0], 5, 5, 0, 2, 9.0, 1.0, 15.0));
  for (int i = 0; i < 16; i++) CHECK(labels.data()[i] == ((i == 5 || i == 10) ? 1 : 0));
  CHECK(dem.data()[5] == 1.0f && dem.data()[10] == 2.0f);   // the DEM is an input
  rdgpu::Depressions<rdgpu::Topology::D4>(dem, labels, table);
  CHECK(table.size() == 2 && same(table[0], 5, 5, 1, 1, 9.0, 1.0, 8.0) && same(table[1], 10, 10, 6, 1, 9.0, 2.0, 7.0));
  for (int i = 0; i < 16; i++) CHECK(labels.data()[i] == (i == 5 ? 1 : i == 10 ? 2 : 0));
  // int16, the cascade: the upper lake (cell 8) stands at the lip's level 6, the lower one (cell 10) at 4
  Array2D<int16_t> cas(7, 3, 9);
  cas.data()[8] = 2; cas.data()[9] = 6; cas.data()[10] = 1; cas.data()[17] = 4;
  rdgpu::Depressions<rdgpu::Topology::D8>(cas, labels, table);
  CHECK(labels.width() == 7 && labels.height() == 3);
  CHECK(table.size() == 2 && same(table[0], 8, 8, 9, 1, 6.0, 2.0, 4.0) && same(table[1], 10, 10, 17, 1, 4.0, 1.0, 3.0));
  // nothing to raise, and an empty raster
  Array2D<double> flat(4, 4, 3.0);
  rdgpu::Depressions<rdgpu::Topology::D8>(flat, labels, table);
  CHECK(table.empty());
  for (int i = 0; i < 16; i++) CHECK(labels.data()[i] == 0);
  Array2D<float> none;
  rdgpu::Depressions<rdgpu::Topology::D8>(none, labels, table);
  CHECK(table.empty() && labels.width() == 0 && labels.height() == 0);
  // 64-bit integers are refused
  Array2D<int64_t> big(4, 4, 3);
  CHECK(!thrown([&] { rdgpu::Depressions<rdgpu::Topology::D8>(big, labels, table); }).empty());
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
