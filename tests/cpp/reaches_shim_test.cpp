// tests/cpp/reaches_shim_test.cpp -- the stream-reach part of include/rdgpu/richdem_gpu.hpp (rdgpu::d8_stream_reaches, with
// and without a channel mask and an order raster) on a raster whose answers are known by hand.  Built by
// tests/cpp/Makefile.reaches.
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

int main() {
  using rdgpu::Array2D;
  // 5 x 3: the middle row flows east (5) to a NO_FLOW cell in the last column; (2, 0) flows south (7) into it, the rest of
  // the top row has no direction; the bottom row flows north (3).  Channels: the middle row and (2, 0), so (2, 1) is a
  // junction.  Cells are 3 wide and 4 high.
  Array2D<uint8_t> dirs(5, 3, 5);
  for (int x = 0; x < 5; x++) { dirs.data()[x] = 0; dirs.data()[10 + x] = 3; }
  dirs.data()[2] = 7;
  dirs.data()[5 + 4] = 0;
  dirs.setNoData(255);
  dirs.geotransform = {100.0, 3.0, 0.0, 200.0, 0.0, -4.0};
  dirs.projection = "a projection";
  Array2D<uint8_t> chan(5, 3, 0), order(5, 3, 0);
  for (int x = 0; x < 5; x++) { chan.data()[5 + x] = 1; order.data()[5 + x] = x < 2 ? 1 : 2; }
  chan.data()[2] = order.data()[2] = 1;
  Array2D<uint32_t> reach(2, 2, 9u), catchment;
  std::vector<rdgpu_reach> table(7);
  rdgpu::d8_stream_reaches(dirs, &chan, &order, reach, catchment, table);
  CHECK(reach.width() == 5 && reach.height() == 3 && reach.noData() == 0u);
  CHECK(catchment.width() == 5 && catchment.height() == 3 && catchment.noData() == 0u);
  CHECK(reach.geotransform == dirs.geotransform && reach.projection == dirs.projection);
  CHECK(catchment.geotransform == dirs.geotransform && catchment.projection == dirs.projection);
  // labels by the raster index of the bottom: (2, 0) alone | (0, 1)-(1, 1) | (2, 1)-(4, 1)
  const uint32_t expr[15] = {0, 0, 1, 0, 0, 2, 2, 3, 3, 3, 0, 0, 0, 0, 0};
  const uint32_t expc[15] = {0, 0, 1, 0, 0, 2, 2, 3, 3, 3, 2, 2, 3, 3, 3};
  for (int i = 0; i < 15; i++) CHECK(reach.data()[i] == expr[i] && catchment.data()[i] == expc[i]);
  CHECK(table.size() == 3);
  if (table.size() == 3) {
    const rdgpu_reach e[3] = {{2, 2, 3, 0, 1, 1, {0, 1, 0}, 1, 4.0}, {5, 6, 3, 0, 2, 4, {2, 0, 0}, 1, 6.0}, {7, 9, 0, 2, 3, 6, {2, 0, 0}, 2, 6.0}};
    for (int i = 0; i < 3; i++) {
      const rdgpu_reach &r = table[i];
      CHECK(r.top_cell == e[i].top_cell && r.bottom_cell == e[i].bottom_cell && r.down == e[i].down && r.up == e[i].up);
      CHECK(r.cells == e[i].cells && r.catchment_cells == e[i].catchment_cells && r.order == e[i].order && r.length == e[i].length);
      CHECK(r.steps[0] == e[i].steps[0] && r.steps[1] == e[i].steps[1] && r.steps[2] == e[i].steps[2]);
    }
  }
  // without a mask and an order: every cell is a channel cell -- four lone cells in the top row, (2, 0), five heads in the
  // bottom row, and (1, 1) .. (4, 1) are junctions; (2, 1) has three children
  const Array2D<uint8_t> *none = nullptr;
  rdgpu::d8_stream_reaches(dirs, none, none, reach, catchment, table);
  CHECK(table.size() == 14);
  for (int i = 0; i < 15; i++) CHECK(reach.data()[i] != 0 && reach.data()[i] == catchment.data()[i]);
  for (const rdgpu_reach &r : table) {
    CHECK(r.order == 0);
    if (r.top_cell == 7) CHECK(r.up == 3 && r.cells == 1 && r.down == reach.data()[8]);
  }
  Array2D<uint8_t> small(2, 2, 1);
  CHECK(thrown([&] { rdgpu::d8_stream_reaches(dirs, &small, none, reach, catchment, table); }).find("directions' size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::d8_stream_reaches(dirs, none, &small, reach, catchment, table); }).find("directions' size") != std::string::npos);
  Array2D<uint8_t> bare(5, 3, 0);
  bare.setNoData(255);
  CHECK(thrown([&] { rdgpu::d8_stream_reaches(bare, none, none, reach, catchment, table); }).find("geotransform") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
