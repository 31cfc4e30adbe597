// tests/cpp/dephier_shim_test.cpp -- rdgpu::DepressionHierarchy of include/rdgpu/richdem_gpu.hpp on rasters whose answers
// are known by hand (the same ones as tests/test_dephier_model.py).  Built by tests/cpp/Makefile.dephier.
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

static const uint32_t NONE = RDGPU_DEPHIER_NONE;

static bool links(const rdgpu_dephier_node &d, uint32_t parent, uint32_t lchild, uint32_t rchild, uint32_t pit, uint32_t inside,
                  uint32_t outside, uint32_t geolink) {
  return d.parent == parent && d.lchild == lchild && d.rchild == rchild && d.pit_cell == pit && d.inside_cell == inside &&
         d.outside_cell == outside && d.geolink == geolink;
}
static bool sums(const rdgpu_dephier_node &d, uint32_t cells, double level, double pit_elevation, double volume) {
  return d.cells == cells && d.level == level && d.pit_elevation == pit_elevation && d.volume == volume;
}

int main() {
  using rdgpu::Array2D;
  static_assert(sizeof(rdgpu_dephier_node) == 56, "the record of rdgpu.h");
  // 7 x 3, D4: pits 1 (cell 8), 4 (cell 10) and 2 (cell 12); saddles 6 (cell 9) and 7 (cell 11); the lowest border cell 8 (cell 3)
  Array2D<int32_t> dem(7, 3, 9);
  const int32_t row[7] = {9, 1, 6, 4, 7, 2, 9};
  for (int x = 0; x < 7; x++) dem.data()[7 + x] = row[x];
  dem.data()[3] = 8;
  dem.geotransform = {100.0, 2.0, 0.0, 200.0, 0.0, -2.0};
  dem.projection = "a projection";
  Array2D<int32_t> labels(2, 2, 7);
  std::vector<rdgpu_dephier_node> t = rdgpu::DepressionHierarchy(dem, 4, labels);
  CHECK(labels.width() == 7 && labels.height() == 3 && labels.noData() == -1);
  CHECK(labels.geotransform == dem.geotransform && labels.projection == dem.projection);
  const int32_t want[7] = {-1, 0, 0, 1, 2, 2, -1};
  for (int i = 0; i < 21; i++) CHECK(labels.data()[i] == (i >= 7 && i < 14 ? want[i - 7] : -1));
  CHECK(t.size() == 5);
  if (t.size() == 5) {
    CHECK(links(t[0], 3, NONE, NONE, 8, 9, 10, 1) && sums(t[0], 2, 6.0, 1.0, 5.0));
    CHECK(links(t[1], 3, NONE, NONE, 10, 10, 9, 0) && sums(t[1], 1, 6.0, 4.0, 2.0));
    CHECK(links(t[2], 4, NONE, NONE, 12, 11, 10, 1) && sums(t[2], 2, 7.0, 2.0, 5.0));
    CHECK(links(t[3], 4, 0, 1, 8, 10, 11, 2) && sums(t[3], 3, 7.0, 1.0, 10.0));
    CHECK(links(t[4], NONE, 3, 2, 8, 10, 3, NONE) && sums(t[4], 5, 8.0, 1.0, 20.0));
  }
  for (int x = 0; x < 7; x++) CHECK(dem.data()[7 + x] == row[x]);   // the DEM is an input
  // 5 x 5, D8: three basins over one saddle cell (12): the edge to the lower cell index (8) comes first
  Array2D<float> three(5, 5, 9.0f);
  three.data()[6] = 1.0f; three.data()[8] = 2.0f; three.data()[12] = 5.0f; three.data()[17] = 3.0f;
  t = rdgpu::DepressionHierarchy(three, 8, labels);
  CHECK(t.size() == 5 && labels.data()[12] == 0 && labels.data()[17] == 2 && labels.data()[0] == -1);
  if (t.size() == 5) {
    CHECK(links(t[0], 3, NONE, NONE, 6, 12, 8, 1) && links(t[1], 3, NONE, NONE, 8, 8, 12, 0));
    CHECK(links(t[2], 4, NONE, NONE, 17, 17, 12, 0) && links(t[3], 4, 0, 1, 6, 12, 17, 2));
    CHECK(links(t[4], NONE, 3, 2, 6, 6, 0, NONE) && t[3].level == 5.0 && t[4].level == 9.0);
  }
  // uint8: a pit next to the border ring
  Array2D<uint8_t> edge(4, 3, 5);
  edge.data()[5] = 1; edge.data()[6] = 3; edge.data()[11] = 4;
  t = rdgpu::DepressionHierarchy(edge, 8, labels);
  CHECK(t.size() == 1 && links(t[0], NONE, NONE, NONE, 5, 6, 11, NONE) && sums(t[0], 2, 4.0, 1.0, 4.0));
  t = rdgpu::DepressionHierarchy(edge, 4, labels);
  CHECK(t.size() == 1 && links(t[0], NONE, NONE, NONE, 5, 5, 1, NONE) && t[0].level == 5.0);
  // no pits, and an empty raster
  Array2D<int16_t> flat(6, 5, 3);
  t = rdgpu::DepressionHierarchy(flat, 8, labels);
  CHECK(t.empty());
  for (int i = 0; i < 30; i++) CHECK(labels.data()[i] == -1);
  Array2D<float> none;
  t = rdgpu::DepressionHierarchy(none, 8, labels);
  CHECK(t.empty() && labels.width() == 0 && labels.height() == 0);
  // f64 and 64-bit integers are refused, and so is a topology that is neither 8 nor 4
  Array2D<double> d64(4, 4, 3.0);
  Array2D<int64_t> big(4, 4, 3);
  CHECK(!thrown([&] { rdgpu::DepressionHierarchy(d64, 8, labels); }).empty());
  CHECK(!thrown([&] { rdgpu::DepressionHierarchy(big, 8, labels); }).empty());
  CHECK(!thrown([&] { rdgpu::DepressionHierarchy(three, 6, labels); }).empty());
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
