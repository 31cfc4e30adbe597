// tests/cpp/ocean_shim_test.cpp -- rdgpu::DepressionHierarchy with an ocean mask and rdgpu::BucketFillFromEdges of
// include/rdgpu/richdem_gpu.hpp on rasters whose answers are known by hand (the same ones as
// tests/test_dephier_ocean_model.py).  Built by tests/cpp/Makefile.ocean.
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
  // 3 x 3, D8: a land pit in the corner (cell 0), a second pit (cell 7), ONE ocean cell (8) higher than all the land
  Array2D<int32_t> dem(3, 3, 0);
  const int32_t z[9] = {1, 4, 6, 3, 5, 7, 8, 2, 9};
  for (int i = 0; i < 9; i++) dem.data()[i] = z[i];
  dem.geotransform = {100.0, 2.0, 0.0, 200.0, 0.0, -2.0};
  dem.projection = "a projection";
  Array2D<uint8_t> ocean(3, 3, 0);
  ocean.data()[8] = 1;
  Array2D<int32_t> labels(2, 2, 7);
  std::vector<rdgpu_dephier_node> t = rdgpu::DepressionHierarchy(dem, 8, labels, ocean);
  CHECK(labels.width() == 3 && labels.height() == 3 && labels.noData() == -1);
  CHECK(labels.geotransform == dem.geotransform && labels.projection == dem.projection);
  const int32_t want[9] = {0, 0, 0, 0, 0, 1, 1, 1, -1};
  for (int i = 0; i < 9; i++) CHECK(labels.data()[i] == want[i]);
  CHECK(t.size() == 3);
  if (t.size() == 3) {
    CHECK(links(t[0], 2, NONE, NONE, 0, 3, 7, 1) && sums(t[0], 2, 3.0, 1.0, 2.0));
    CHECK(links(t[1], 2, NONE, NONE, 7, 7, 3, 0) && sums(t[1], 1, 3.0, 2.0, 1.0));
    CHECK(links(t[2], NONE, 0, 1, 0, 4, 8, NONE) && sums(t[2], 8, 9.0, 1.0, 36.0));   // the outside cell is the ocean cell
  }
  for (int i = 0; i < 9; i++) CHECK(dem.data()[i] == z[i] && ocean.data()[i] == (i == 8 ? 1 : 0));   // inputs
  // 5 x 1, D4: the ocean cell (2, value 5) is the wall both pits spill over
  Array2D<int16_t> row(5, 1, 0);
  const int16_t rz[5] = {7, 1, 5, 2, 8};
  for (int i = 0; i < 5; i++) row.data()[i] = rz[i];
  Array2D<uint8_t> wall(5, 1, 0);
  wall.data()[2] = 200;                                                               // any non-zero byte
  t = rdgpu::DepressionHierarchy(row, 4, labels, wall);
  CHECK(t.size() == 2 && labels.data()[0] == 0 && labels.data()[2] == -1 && labels.data()[4] == 1);
  if (t.size() == 2) {
    CHECK(links(t[0], NONE, NONE, NONE, 1, 1, 2, NONE) && sums(t[0], 1, 5.0, 1.0, 4.0));
    CHECK(links(t[1], NONE, NONE, NONE, 3, 3, 2, NONE) && sums(t[1], 1, 5.0, 2.0, 3.0));
  }
  // every cell ocean: no nodes; no ocean cell, a mask of another size, f64: refused
  Array2D<uint8_t> all(5, 1, 1), nothing(5, 1, 0), small(2, 1, 1);
  t = rdgpu::DepressionHierarchy(row, 8, labels, all);
  CHECK(t.empty());
  for (int i = 0; i < 5; i++) CHECK(labels.data()[i] == -1);
  CHECK(thrown([&] { rdgpu::DepressionHierarchy(row, 8, labels, nothing); }).find("no ocean cells") != std::string::npos);
  CHECK(!thrown([&] { rdgpu::DepressionHierarchy(row, 8, labels, small); }).empty());
  Array2D<double> d64(5, 1, 3.0);
  CHECK(!thrown([&] { rdgpu::DepressionHierarchy(d64, 8, labels, all); }).empty());
  Array2D<float> none;
  Array2D<uint8_t> none_mask;
  t = rdgpu::DepressionHierarchy(none, 8, labels, none_mask);
  CHECK(t.empty() && labels.width() == 0);

  // BucketFillFromEdges, the reference's signature: any set raster type, set_value written where the fill reaches
  //   1 0 0 0 0        the corner cell and its diagonal neighbour (D8 only); the lake at (3, 1), (3, 2) touches no edge
  //   0 1 0 1 0
  //   0 0 0 1 0
  //   0 0 0 0 0
  Array2D<float> check(5, 4, 0.0f);
  check.data()[0] = check.data()[6] = check.data()[8] = check.data()[13] = 1.0f;
  Array2D<int32_t> set(5, 4, -3);
  CHECK(rdgpu::BucketFillFromEdges<8>(check, set, 1.0f, 42) == 2);
  for (int i = 0; i < 20; i++) CHECK(set.data()[i] == (i == 0 || i == 6 ? 42 : -3));
  CHECK(rdgpu::BucketFillFromEdges<8>(check, set, 1.0f, 42) == 0);                     // already set: nothing to do
  Array2D<uint8_t> set4(5, 4, 0);
  CHECK(rdgpu::BucketFillFromEdges<4>(check, set4, 1.0f, (uint8_t)9) == 1 && set4.data()[0] == 9 && set4.data()[6] == 0);
  // a pre-set cell stops the fill: the zeros reach the edges everywhere, but not across a wall of set cells
  Array2D<int64_t> zeros(6, 3, 0);
  Array2D<double> setd(6, 3, 0.5);
  for (int y = 0; y < 3; y++) setd.data()[y * 6 + 2] = 7.0;                            // column 2 is already set_value
  setd.data()[6 + 4] = 0.5;
  CHECK(rdgpu::BucketFillFromEdges<4>(zeros, setd, (int64_t)0, 7.0) == 15);
  for (int i = 0; i < 18; i++) CHECK(setd.data()[i] == 7.0);
  Array2D<int32_t> other(2, 2, 0);
  CHECK(thrown([&] { rdgpu::BucketFillFromEdges<8>(check, other, 1.0f, 1); }) == "Rasters must have the same dimension for BucketFill!");
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
