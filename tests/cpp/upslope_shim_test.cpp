// tests/cpp/upslope_shim_test.cpp -- the upslope part of include/rdgpu/richdem_gpu.hpp (rdgpu::d8_upslope_cells,
// d8_catchments, d8_outlets).  Built by tests/cpp/Makefile.upslope.
//   upslope_shim_test                  the reference's side effects on a raster whose answers are known by hand
//   upslope_shim_test --batch <file>   one job per line: <dirs file> <w> <h> <nodata> <x0> <y0> <x1> <y1> <out file>; the
//                                      raw uint8 directions are read, rdgpu::d8_upslope_cells' raster is written
//                                      (tests/test_upslope_shim_gpu.py compares it with the compiled reference's)
#include <cstdio>
#include <fstream>
#include <sstream>
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

static int batch(const char *manifest) {
  std::ifstream in(manifest);
  std::string line;
  int jobs = 0;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string src, dst;
    int w, h, nodata, x0, y0, x1, y1;
    if (!(ss >> src >> w >> h >> nodata >> x0 >> y0 >> x1 >> y1 >> dst)) { std::printf("bad job: %s\n", line.c_str()); return 2; }
    rdgpu::Array2D<uint8_t> dirs(w, h, 0);
    dirs.setNoData((uint8_t)nodata);
    std::ifstream f(src, std::ios::binary);
    if (!f.read(reinterpret_cast<char *>(dirs.data()), (std::streamsize)w * h)) { std::printf("cannot read %s\n", src.c_str()); return 2; }
    rdgpu::Array2D<uint8_t> up;
    rdgpu::d8_upslope_cells(x0, y0, x1, y1, dirs, up);
    if (up.width() != w || up.height() != h || up.noData() != 255) { std::printf("bad output raster: %s\n", line.c_str()); return 2; }
    std::ofstream o(dst, std::ios::binary);
    o.write(reinterpret_cast<const char *>(up.data()), (std::streamsize)w * h);
    jobs++;
  }
  std::printf("%d jobs done\n", jobs);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && std::string(argv[1]) == "--batch") return batch(argv[2]);
  using rdgpu::Array2D;
  // 5 x 3, everything flows east (5) along its row; the last column has NO_FLOW; (0, 2) is NoData
  Array2D<uint8_t> dirs(5, 3, 5);
  for (int y = 0; y < 3; y++) dirs.data()[y * 5 + 4] = 0;
  dirs.setNoData(255);
  dirs.data()[2 * 5 + 0] = 255;
  dirs.geotransform = {100.0, 2.0, 0.0, 200.0, 0.0, -2.0};
  dirs.projection = "a projection";
  Array2D<int16_t> up(2, 2, 7);
  up.setNoData(-3);
  rdgpu::d8_upslope_cells(2, 1, 2, 1, dirs, up);                 // the pour point (2, 1)
  CHECK(up.width() == 5 && up.height() == 3 && up.noData() == 255);
  CHECK(up.geotransform == dirs.geotransform && up.projection == dirs.projection);
  const int16_t exp[15] = {255, 255, 255, 255, 255, 1, 1, 2, 255, 255, 255, 255, 255, 255, 255};
  for (int i = 0; i < 15; i++) CHECK(up.data()[i] == exp[i]);
  Array2D<uint8_t> up8;
  rdgpu::d8_upslope_cells(3, 2, 1, 2, dirs, up8);                // swapped end points, a line on row 2
  const uint8_t exp8[15] = {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 2, 2, 2, 255};
  for (int i = 0; i < 15; i++) CHECK(up8.data()[i] == exp8[i]);
  CHECK(thrown([&] { rdgpu::d8_upslope_cells(0, 0, 4, 2, dirs, up8); }).find("leaves the raster") != std::string::npos);
  Array2D<uint32_t> out;
  rdgpu::d8_outlets(dirs, out);
  CHECK(out.width() == 5 && out.height() == 3 && out.noData() == 0xFFFFFFFFu);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 5; x++) CHECK(out.data()[y * 5 + x] == (y == 2 && x == 0 ? 0xFFFFFFFFu : (uint32_t)(y * 5 + 4)));
  Array2D<int32_t> lab;
  rdgpu::d8_catchments(dirs, {3u, 8u, 8u, 10u}, {11, 22, 33, 44}, lab, -1);   // (3,0); (3,1) twice; the NoData cell (0,2)
  CHECK(lab.width() == 5 && lab.height() == 3 && lab.noData() == -1);
  const int32_t expl[15] = {11, 11, 11, 11, -1, 22, 22, 22, 22, -1, 44, -1, -1, -1, -1};
  for (int i = 0; i < 15; i++) CHECK(lab.data()[i] == expl[i]);
  CHECK(thrown([&] { rdgpu::d8_catchments(dirs, {15u}, {1}, lab, -1); }).find("outside the raster") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
