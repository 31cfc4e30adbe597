// tests/cpp/longest_shim_test.cpp -- the longest-flow-path part of include/rdgpu/richdem_gpu.hpp
// (rdgpu::d8_longest_flow_path) on a raster whose answers are known by hand; with a file name (directions: a native raster)
// it also writes <prefix>_length / <prefix>_from_cell / <prefix>_on_basin_path, for tests/test_longest_path_shim_gpu.py to
// compare with the Python layer.  Built by tests/cpp/Makefile.longest.
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
  if (argc == 3) {   // <directions> <prefix>
    Array2D<uint8_t> dirs(std::string(argv[1]), true), on_path;
    Array2D<double> length;
    Array2D<uint32_t> from;
    rdgpu::d8_longest_flow_path(dirs, length, &from, &on_path);
    length.saveToCache(std::string(argv[2]) + "_length");
    from.saveToCache(std::string(argv[2]) + "_from_cell");
    on_path.saveToCache(std::string(argv[2]) + "_on_basin_path");
    std::printf("written\n");
    return 0;
  }
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
  Array2D<double> length(2, 2, 9.0);
  Array2D<uint32_t> from(1, 1, 9);
  Array2D<uint8_t> on_path(1, 1, 9);
  rdgpu::d8_longest_flow_path(dirs, length, &from, &on_path);
  CHECK(length.width() == 5 && length.height() == 3 && length.noData() == -1.0);
  CHECK(from.width() == 5 && from.height() == 3 && from.noData() == 0xFFFFFFFFu && on_path.width() == 5 && on_path.noData() == 0);
  CHECK(length.geotransform == dirs.geotransform && length.projection == dirs.projection && from.geotransform == dirs.geotransform &&
        on_path.geotransform == dirs.geotransform);
  // distances to the outlet (9): top row 14 11 8 5 4, middle 12 9 6 3 0, bottom - 13 10 7 4.  (x, 1) collects (x - 1, 0),
  // (x - 1, 1) and (x, 2); the farthest cell upstream is cell 0 from (1, 1) on, its own top-left neighbour being as far away
  // as the cell below only for (0, 1), which has no cell above left: itself.
  const uint32_t N = 0xFFFFFFFFu;
  const uint32_t expf[15] = {0, 1, 2, 3, 4, 5, 0, 0, 0, 0, N, 11, 12, 13, 14};
  const double expl[15] = {0, 0, 0, 0, 0, 0, 5, 8, 11, 14, -1, 0, 0, 0, 0};
  const int expp[15] = {1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0};
  for (int i = 0; i < 15; i++) {
    CHECK(from.data()[i] == expf[i]);
    CHECK(length.data()[i] == expl[i]);
    CHECK(on_path.data()[i] == expp[i]);
  }
  Array2D<double> only(1, 1, 0.0);
  rdgpu::d8_longest_flow_path(dirs, only);              // without the optional rasters
  for (int i = 0; i < 15; i++) CHECK(only.data()[i] == expl[i]);
  Array2D<uint32_t> from2;
  rdgpu::d8_longest_flow_path(dirs, only, &from2);
  for (int i = 0; i < 15; i++) CHECK(from2.data()[i] == expf[i] && only.data()[i] == expl[i]);
  Array2D<uint8_t> empty;
  empty.geotransform = dirs.geotransform;
  rdgpu::d8_longest_flow_path(empty, only, &from2);      // an empty raster returns early
  CHECK(only.width() == 0 && from2.width() == 0);
  Array2D<uint8_t> bare(5, 3, 0);
  bare.setNoData(255);
  CHECK(thrown([&] { rdgpu::d8_longest_flow_path(bare, length); }).find("geotransform") != std::string::npos);
  bare.geotransform = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  CHECK(!thrown([&] { rdgpu::d8_longest_flow_path(bare, length); }).empty());    // a zero cell length
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
