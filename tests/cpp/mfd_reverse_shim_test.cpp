// tests/cpp/mfd_reverse_shim_test.cpp -- the reverse-accumulation part of include/rdgpu/richdem_gpu.hpp
// (rdgpu::FlowReverseAccumulation over an Array3D<float> of proportions, rdgpu::DinfReverseAccumulation[_flats] and
// rdgpu::DinfUpslopeDependence[_flats] over a DEM) on rasters whose answers are known by hand.  Built by
// tests/cpp/Makefile.mfdrev.
#include <cmath>
#include <cstdio>
#include <string>

#include "rdgpu/Array2D.hpp"
#include "rdgpu/Array3D.hpp"
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
  using rdgpu::Array3D;
  using rdgpu::ReverseAccumOptions;
  // 6 x 4, everything NoData but: A = (1, 1) gives 0.25 to B = (2, 1) on its right (5) and 0.75 to C = (2, 2) down-right (6);
  // B gives 1 to (3, 1) on its right and 0.5 to C below it (7); C -> (3, 2) -> (4, 2).
  Array3D<float> props(6, 4, -1.0f);
  for (int y = 0; y < 4; y++)
    for (int x = 0; x < 6; x++) props(x, y, 0) = -2.0f;
  auto name = [&](int x, int y) { props(x, y, 0) = 0.0f; };
  name(1, 1); props(1, 1, 5) = 0.25f; props(1, 1, 6) = 0.75f;
  name(2, 1); props(2, 1, 5) = 1.0f; props(2, 1, 7) = 0.5f;
  name(3, 1);
  name(2, 2); props(2, 2, 5) = 1.0f;
  name(3, 2); props(3, 2, 5) = 1.0f;
  name(4, 2);
  Array2D<double> wts(6, 4, 0.0);
  wts(1, 1) = 1.0; wts(2, 1) = 2.0; wts(3, 1) = 4.0; wts(2, 2) = 8.0; wts(3, 2) = 16.0; wts(4, 2) = -32.0;
  Array2D<uint8_t> *nomask = nullptr;
  Array2D<double> *none = nullptr;
  Array2D<double> racc(2, 2, 9.0), wmax;
  rdgpu::FlowReverseAccumulation(props, &wts, nomask, &racc, &wmax);
  CHECK(racc.width() == 6 && racc.height() == 4 && racc.noData() == -9999.0 && wmax.width() == 6 && wmax.noData() == -9999.0);
  CHECK(racc(0, 0) == -9999.0 && wmax(5, 3) == -9999.0);
  // (4,2) = -32; (3,2) = 16 - 32 = -16; C = 8 - 16 = -8; (3,1) = 4; B = 2 + 1*4 + 0.5*(-8) = 2; A = 1 + 0.25*2 + 0.75*(-8) = -4.5
  CHECK(racc(4, 2) == -32.0 && racc(3, 2) == -16.0 && racc(2, 2) == -8.0 && racc(3, 1) == 4.0 && racc(2, 1) == 2.0);
  CHECK(racc(1, 1) == -4.5);
  CHECK(wmax(4, 2) == -32.0 && wmax(3, 2) == 16.0 && wmax(2, 2) == 16.0 && wmax(3, 1) == 4.0 && wmax(2, 1) == 16.0 && wmax(1, 1) == 16.0);
  // C absorbs: what lies below it does not count; weight NoData 2 takes B out, which still passes on what lies below it
  Array2D<uint8_t> dest(6, 4, 0);
  dest(2, 2) = 1;
  ReverseAccumOptions o;
  o.weight_nodata = 2.0;
  o.out_nodata = -1.0;
  rdgpu::FlowReverseAccumulation(props, &wts, &dest, &racc, none, o);
  CHECK(racc.noData() == -1.0 && racc(0, 0) == -1.0);
  CHECK(racc(2, 2) == 8.0 && racc(2, 1) == 0.0 + 4.0 + 0.5 * 8.0 && racc(1, 1) == 1.0 + 0.25 * 8.0 + 0.75 * 8.0);
  CHECK(racc(3, 2) == -16.0);
  // the dependence on C: A sends 0.75 directly and 0.25 * 0.5 over B
  Array2D<double> dep;
  rdgpu::FlowReverseAccumulation(props, none, &dest, &dep, none, o);
  CHECK(dep(2, 2) == 1.0 && dep(2, 1) == 0.5 && dep(1, 1) == 0.875 && dep(3, 1) == 0.0 && dep(3, 2) == 0.0 && dep(0, 0) == -1.0);
  Array2D<double> small(2, 2, 1.0);
  CHECK(thrown([&] { rdgpu::FlowReverseAccumulation(props, &small, nomask, &racc, none); }).find("raster's size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::FlowReverseAccumulation(props, &wts, nomask, none, none); }).find("no output") != std::string::npos);
  CHECK(thrown([&] { rdgpu::FlowReverseAccumulation(props, none, &dest, &racc, &wmax); }).find("wmax") != std::string::npos);
  CHECK(thrown([&] { rdgpu::FlowReverseAccumulation(props, none, nomask, &racc, none); }).find("neither") != std::string::npos);

  // D-infinity from a DEM: a plane that falls 7 per cell towards the east, 6 x 3.  The interior cells (1..4, 1) flow east
  // with share 1; the cells on the edge have no receivers.
  Array2D<float> dem(6, 3, 0.0f);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 6; x++) dem(x, y) = 100.0f - 7.0f * x;
  dem.setNoData(-1.0f);
  dem.geotransform = {100.0, 3.0, 0.0, 200.0, 0.0, -4.0};
  dem.projection = "a projection";
  Array2D<double> ones(6, 3, 1.0), r2, m2;
  rdgpu::DinfReverseAccumulation(dem, &ones, nomask, &r2, &m2);
  CHECK(r2.width() == 6 && r2.height() == 3 && r2.noData() == -9999.0 && m2.noData() == -9999.0);
  CHECK(r2.geotransform == dem.geotransform && r2.projection == dem.projection && m2.geotransform == dem.geotransform);
  for (int x = 0; x < 6; x++) {
    CHECK(r2(x, 0) == 1.0 && r2(x, 2) == 1.0 && m2(x, 0) == 1.0);
    CHECK(r2(x, 1) == (x == 0 ? 1.0 : 6.0 - x));   // the cells from x to the edge cell (5, 1)
    CHECK(m2(x, 1) == 1.0);
  }
  Array2D<uint8_t> gate(6, 3, 0);
  gate(3, 1) = 1;
  Array2D<double> d2, d3;
  rdgpu::DinfUpslopeDependence(dem, gate, d2);
  CHECK(d2.geotransform == dem.geotransform && d2.projection == dem.projection && d2.noData() == -9999.0);
  CHECK(d2(0, 1) == 0.0 && d2(1, 1) == 1.0 && d2(2, 1) == 1.0 && d2(3, 1) == 1.0 && d2(4, 1) == 0.0 && d2(5, 1) == 0.0 && d2(2, 0) == 0.0);
  rdgpu::DinfUpslopeDependence_flats(dem, gate, d3);                      // no flats on a plane: the same
  CHECK(d3.geotransform == dem.geotransform && d3.projection == dem.projection);
  for (int x = 0; x < 6; x++) CHECK(d3(x, 1) == d2(x, 1) && d3(x, 2) == d2(x, 2));
  rdgpu::DinfReverseAccumulation_flats(dem, &ones, &gate, &r2, none);
  CHECK(r2(1, 1) == 3.0 && r2(3, 1) == 1.0 && r2(4, 1) == 2.0);
  Array2D<int16_t> demi(6, 3, 0);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 6; x++) demi(x, y) = (int16_t)(50 - 2 * x);
  demi.setNoData(-32768);
  rdgpu::DinfReverseAccumulation(demi, &ones, nomask, &r2, none);
  CHECK(r2(1, 1) == 5.0 && r2(4, 1) == 2.0 && r2(5, 1) == 1.0);
  CHECK(thrown([&] { rdgpu::DinfReverseAccumulation(dem, &ones, nomask, none, none); }).find("no output") != std::string::npos);
  CHECK(thrown([&] { rdgpu::DinfReverseAccumulation(dem, none, nomask, &r2, none); }).find("neither") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
