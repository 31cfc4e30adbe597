// tests/cpp/flowpath_shim_test.cpp -- the flow-path part of include/rdgpu/richdem_gpu.hpp (rdgpu::d8_flow_distance and
// rdgpu::d8_hand, with and without a channel mask) on a raster whose answers are known by hand.  Built by
// tests/cpp/Makefile.flowpath.
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
  // 5 x 3: the middle row flows east (5) to a NO_FLOW cell in the last column; the top row flows south-east (6) into it,
  // the bottom row north (3); (0, 2) is NoData.  Cells are 3 wide and 4 high: a diagonal step is 5.
  Array2D<uint8_t> dirs(5, 3, 5);
  for (int x = 0; x < 5; x++) { dirs.data()[x] = 6; dirs.data()[10 + x] = 3; }
  dirs.data()[4] = 7;           // (4, 0): south-east would leave the raster; south instead
  dirs.data()[5 + 4] = 0;
  dirs.setNoData(255);
  dirs.data()[10] = 255;
  dirs.geotransform = {100.0, 3.0, 0.0, 200.0, 0.0, -4.0};
  dirs.projection = "a projection";
  Array2D<double> dist(2, 2, 9.0);
  rdgpu::d8_flow_distance(dirs, dist);
  CHECK(dist.width() == 5 && dist.height() == 3 && dist.noData() == -1.0);
  CHECK(dist.geotransform == dirs.geotransform && dist.projection == dirs.projection);
  const double exp[15] = {5 + 9, 5 + 6, 5 + 3, 5, 4, 12, 9, 6, 3, 0, -1, 4 + 9, 4 + 6, 4 + 3, 4};
  for (int i = 0; i < 15; i++) CHECK(dist.data()[i] == exp[i]);
  // channels: (2, 1) alone.  What lies downstream of it meets no channel.
  Array2D<uint8_t> chan(5, 3, 0);
  chan.data()[5 + 2] = 1;
  rdgpu::d8_flow_distance(dirs, dist, &chan);
  const double expc[15] = {5 + 3, 5, -1, -1, -1, 6, 3, 0, -1, -1, -1, 4 + 3, 4, -1, -1};
  for (int i = 0; i < 15; i++) CHECK(dist.data()[i] == expc[i]);
  // HAND: elevations 10 * (row + 1) + column, one of them NoData
  Array2D<float> dem(5, 3, 0.0f);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 5; x++) dem.data()[5 * y + x] = 10.0f * (y + 1) + x + 0.5f;
  dem.setNoData(-1.0f);
  dem.data()[1] = -1.0f;
  Array2D<double> hand;
  rdgpu::d8_hand(dem, dirs, hand);
  CHECK(hand.width() == 5 && hand.height() == 3 && hand.noData() == -9999.0);
  CHECK(hand.geotransform == dirs.geotransform && hand.projection == dirs.projection);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 5; x++) {
      const int i = 5 * y + x;
      const double e = (i == 1 || i == 10) ? -9999.0 : (double)dem.data()[i] - 24.5;
      CHECK(hand.data()[i] == e);
    }
  rdgpu::d8_hand(dem, dirs, hand, &chan);
  for (int i = 0; i < 15; i++) {
    const double e = (expc[i] < 0 || i == 1) ? -9999.0 : (double)dem.data()[i] - 22.5;
    CHECK(hand.data()[i] == e);
  }
  Array2D<int16_t> demi(5, 3, 7);
  demi.setNoData(-32768);
  demi.data()[5 + 4] = -3;
  rdgpu::d8_hand(demi, dirs, hand);
  CHECK(hand.data()[0] == 10.0 && hand.data()[9] == 0.0 && hand.data()[10] == -9999.0);
  Array2D<uint8_t> small(2, 2, 1);
  CHECK(thrown([&] { rdgpu::d8_flow_distance(dirs, dist, &small); }).find("directions' size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::d8_hand(Array2D<float>(2, 2, 0.0f), dirs, hand); }).find("directions' size") != std::string::npos);
  Array2D<uint8_t> bare(5, 3, 0);
  bare.setNoData(255);
  CHECK(thrown([&] { rdgpu::d8_flow_distance(bare, dist); }).find("geotransform") != std::string::npos);
  bare.geotransform = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  CHECK(!thrown([&] { rdgpu::d8_flow_distance(bare, dist); }).empty());    // a zero cell length
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
