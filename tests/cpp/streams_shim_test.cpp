// tests/cpp/streams_shim_test.cpp -- the channel-network part of include/rdgpu/richdem_gpu.hpp (rdgpu::d8_channels,
// d8_stream_order with and without a channel mask) on a raster whose answers are known by hand.  Built by
// tests/cpp/Makefile.streams.
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
  // 5 x 3: the middle row flows east (5) to a NO_FLOW cell in the last column; the cells of the top row flow south (7) into
  // it, those of the bottom row north (3); (0, 2) is NoData
  Array2D<uint8_t> dirs(5, 3, 5);
  for (int x = 0; x < 5; x++) { dirs.data()[x] = 7; dirs.data()[10 + x] = 3; }
  dirs.data()[5 + 4] = 0;
  dirs.setNoData(255);
  dirs.data()[10] = 255;
  dirs.geotransform = {100.0, 2.0, 0.0, 200.0, 0.0, -2.0};
  dirs.projection = "a projection";
  Array2D<uint8_t> order(2, 2, 9);
  rdgpu::d8_stream_order(dirs, order);
  CHECK(order.width() == 5 && order.height() == 3 && order.noData() == 0);
  CHECK(order.geotransform == dirs.geotransform && order.projection == dirs.projection);
  // (0,1) has one child: 1; (1,1) has (0,1), (1,0), (1,2): three of order 1 -> 2; further east 2 meets two 1s: 2
  const uint8_t exp[15] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 0, 1, 1, 1, 1};
  for (int i = 0; i < 15; i++) CHECK(order.data()[i] == exp[i]);
  Array2D<double> accum(5, 3, 1.0);
  accum.setNoData(-1);
  for (int x = 0; x < 5; x++) accum.data()[5 + x] = 3.0 * (x + 1) - 1.0;   // 2, 5, 8, 11, 14
  accum.data()[10] = -1;
  Array2D<uint8_t> chan;
  rdgpu::d8_channels(accum, 5.0, chan);
  CHECK(chan.width() == 5 && chan.height() == 3);
  const uint8_t expc[15] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0};
  for (int i = 0; i < 15; i++) CHECK(chan.data()[i] == expc[i]);
  rdgpu::d8_stream_order(dirs, chan, order);
  for (int i = 0; i < 15; i++) CHECK(order.data()[i] == expc[i]);             // one chain: order 1 on it
  Array2D<uint8_t> small(2, 2, 1);
  CHECK(thrown([&] { rdgpu::d8_stream_order(dirs, small, order); }).find("directions' size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::d8_channels(accum, __builtin_nan(""), chan); }).find("finite") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
