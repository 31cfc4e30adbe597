// tests/cpp/mfd_distance_up_shim_test.cpp -- the distance-up part of include/rdgpu/richdem_gpu.hpp (rdgpu::FlowDistanceUp
// over an Array3D<float> of proportions, rdgpu::DinfDistanceUp and rdgpu::DinfDistanceUp_flats over a DEM) on rasters
// whose answers are known by hand.  Built by tests/cpp/Makefile.mfddistup.
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
  using rdgpu::DistanceStat;
  using rdgpu::DistanceUpOptions;
  // 6 x 4, everything NoData but: A = (1, 1) gives 0.25 to B = (2, 1) on its right (5) and 0.75 to C = (2, 2) down-right (6);
  // B gives 1 to (3, 1) on its right and 0.5 to C below it (7); C -> (3, 2) -> (4, 2).  A is the only source.  The donors of
  // C in the order of their position around it: A (up-left, 2), then B (up, 3).
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
  const double r2 = std::sqrt(2.0);
  Array2D<double> dist(2, 2, 9.0);
  rdgpu::FlowDistanceUp(props, dist);
  CHECK(dist.width() == 6 && dist.height() == 4 && dist.noData() == -9999.0);
  CHECK(dist(1, 1) == 0.0 && dist(2, 1) == 1.0 && dist(3, 1) == 2.0);
  const double c_ave = (0.75 * r2 + 0.5 * 2.0) / (0.75 + 0.5);
  CHECK(dist(2, 2) == c_ave && dist(3, 2) == c_ave + 1.0 && dist(4, 2) == c_ave + 1.0 + 1.0);
  CHECK(dist(0, 0) == -9999.0 && dist(5, 3) == -9999.0);
  DistanceUpOptions o;
  o.stat = DistanceStat::Minimum;
  o.out_nodata = -1.0;
  rdgpu::FlowDistanceUp(props, dist, 3.0, 4.0, o);                       // cells 3 wide and 4 high: a diagonal step is 5
  CHECK(dist.noData() == -1.0 && dist(0, 0) == -1.0 && dist(2, 1) == 3.0 && dist(2, 2) == 5.0 && dist(4, 2) == 11.0);
  o.stat = DistanceStat::Maximum;
  rdgpu::FlowDistanceUp(props, dist, 3.0, 4.0, o);
  CHECK(dist(2, 2) == 7.0 && dist(4, 2) == 13.0);
  o.min_share = 0.5f;                                                    // A -> B and B -> C are no links: B is a source
  rdgpu::FlowDistanceUp(props, dist, 3.0, 4.0, o);
  CHECK(dist(2, 1) == 0.0 && dist(3, 1) == 3.0 && dist(2, 2) == 5.0 && dist(1, 1) == 0.0);
  // the rise: z(A) = 9, z(B) = 6, z(3, 1) = 4.5, z(C) = 8
  Array2D<double> elev(6, 4, 0.0), rise;
  elev(1, 1) = 9.0; elev(2, 1) = 6.0; elev(3, 1) = 4.5; elev(2, 2) = 8.0; elev(3, 2) = 2.0; elev(4, 2) = 1.25;
  o = DistanceUpOptions();
  rdgpu::FlowDistanceUp(props, &elev, &dist, &rise, 1.0, 1.0, o);
  CHECK(rise.width() == 6 && rise.height() == 4 && rise.noData() == -9999.0 && rise(0, 0) == -9999.0);
  CHECK(rise(1, 1) == 0.0 && rise(2, 1) == 3.0 && rise(3, 1) == 4.5 && rise(2, 2) == 1.0 && rise(3, 2) == 7.0 && rise(4, 2) == 7.75);
  CHECK(dist(2, 2) == c_ave);
  Array2D<double> *none = nullptr;
  o.stat = DistanceStat::Minimum;
  elev(2, 1) = 8.5;                                                      // through B the way to C now climbs: 0.5 - 0.5 = 0
  rdgpu::FlowDistanceUp(props, &elev, none, &rise, 1.0, 1.0, o);
  CHECK(rise(2, 1) == 0.5 && rise(2, 2) == 1.0);                         // both ways up from C end at A: 9 - 8
  Array2D<double> small(2, 2, 1.0);
  CHECK(thrown([&] { rdgpu::FlowDistanceUp(props, &small, &dist, none); }).find("proportions' size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::FlowDistanceUp(props, &elev, none, none); }).find("no output") != std::string::npos);
  CHECK(thrown([&] { rdgpu::FlowDistanceUp(props, none, none, &rise); }).find("elevations") != std::string::npos);
  CHECK(!thrown([&] { rdgpu::FlowDistanceUp(props, dist, 0.0, 1.0); }).empty());          // a zero cell length
  o.min_share = -0.5f;
  CHECK(!thrown([&] { rdgpu::FlowDistanceUp(props, dist, 1.0, 1.0, o); }).empty());       // a negative threshold

  // D-infinity from a DEM: a plane that falls 7 per cell towards the east, 6 x 3, cells 3 wide and 4 high.  The interior
  // cells (1..4, 1) flow east with share 1; the cells on the edge are no donors, so (1, 1) is a source and the edge cell
  // (5, 1) has the donor (4, 1).
  Array2D<float> dem(6, 3, 0.0f);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 6; x++) dem(x, y) = 100.0f - 7.0f * x;
  dem.setNoData(-1.0f);
  dem.geotransform = {100.0, 3.0, 0.0, 200.0, 0.0, -4.0};
  dem.projection = "a projection";
  Array2D<double> d2, h2;
  rdgpu::DinfDistanceUp(dem, &d2, &h2);
  CHECK(d2.width() == 6 && d2.height() == 3 && d2.noData() == -9999.0 && h2.noData() == -9999.0);
  CHECK(d2.geotransform == dem.geotransform && d2.projection == dem.projection && h2.geotransform == dem.geotransform);
  for (int x = 0; x < 6; x++) {
    CHECK(d2(x, 0) == 0.0 && d2(x, 2) == 0.0 && h2(x, 0) == 0.0);
    CHECK(d2(x, 1) == (x == 0 ? 0.0 : 3.0 * (x - 1)));
    CHECK(h2(x, 1) == (x == 0 ? 0.0 : 7.0 * (x - 1)));
  }
  Array2D<double> d3, h3;
  DistanceUpOptions half;
  half.min_share = 0.5f;
  half.stat = DistanceStat::Maximum;
  rdgpu::DinfDistanceUp_flats(dem, &d3, &h3, half);                       // no flats on a plane, shares of 1: the same
  CHECK(d3.geotransform == dem.geotransform && d3.projection == dem.projection);
  for (int x = 0; x < 6; x++) CHECK(d3(x, 1) == d2(x, 1) && h3(x, 1) == h2(x, 1) && d3(x, 2) == 0.0);
  Array2D<int16_t> demi(6, 3, 0);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 6; x++) demi(x, y) = (int16_t)(50 - 2 * x);
  demi.setNoData(-32768);
  demi.geotransform = dem.geotransform;
  rdgpu::DinfDistanceUp(demi, &d2, &h2);
  CHECK(d2(1, 1) == 0.0 && d2(3, 1) == 6.0 && d2(5, 1) == 12.0 && h2(5, 1) == 8.0);
  Array2D<float> bare(6, 3, 1.0f);
  CHECK(thrown([&] { rdgpu::DinfDistanceUp(bare, &d2, none); }).find("geotransform") != std::string::npos);
  CHECK(thrown([&] { rdgpu::DinfDistanceUp(dem, none, none); }).find("no output") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
