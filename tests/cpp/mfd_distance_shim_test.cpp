// tests/cpp/mfd_distance_shim_test.cpp -- the distance-down part of include/rdgpu/richdem_gpu.hpp (rdgpu::FlowDistanceDown
// over an Array3D<float> of proportions, rdgpu::DinfDistanceDown and rdgpu::DinfHand over a DEM) on rasters whose answers
// are known by hand.  Built by tests/cpp/Makefile.mfddist.
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
  using rdgpu::DistanceDownOptions;
  using rdgpu::DistanceStat;
  // 6 x 4, everything NoData but: A = (1, 1) gives 0.25 to B = (2, 1) on its right (5) and 0.75 to C = (2, 2) down-right (6);
  // B -> (3, 1); C -> (3, 2) -> (4, 2).  (3, 1) and (4, 2) have no receivers.
  Array3D<float> props(6, 4, -1.0f);
  for (int y = 0; y < 4; y++)
    for (int x = 0; x < 6; x++) props(x, y, 0) = -2.0f;
  auto name = [&](int x, int y) { props(x, y, 0) = 0.0f; };
  name(1, 1); props(1, 1, 5) = 0.25f; props(1, 1, 6) = 0.75f;
  name(2, 1); props(2, 1, 5) = 1.0f;
  name(3, 1);
  name(2, 2); props(2, 2, 5) = 1.0f;
  name(3, 2); props(3, 2, 5) = 1.0f;
  name(4, 2);
  Array2D<double> dist(2, 2, 9.0);
  rdgpu::FlowDistanceDown(props, dist);
  CHECK(dist.width() == 6 && dist.height() == 4 && dist.noData() == -9999.0);
  const double v6 = 2.0 + std::sqrt(2.0);
  CHECK(dist(1, 1) == (0.25 * 2.0 + 0.75 * v6) / (0.25 + 0.75) && dist(1, 1) == 3.060660171779821);
  CHECK(dist(2, 1) == 1.0 && dist(3, 1) == 0.0 && dist(2, 2) == 2.0 && dist(3, 2) == 1.0 && dist(4, 2) == 0.0);
  CHECK(dist(0, 0) == -9999.0 && dist(5, 3) == -9999.0);
  DistanceDownOptions o;
  o.stat = DistanceStat::Minimum;
  o.out_nodata = -1.0;
  rdgpu::FlowDistanceDown(props, dist, 3.0, 4.0, o);                     // cells 3 wide and 4 high: a diagonal step is 5
  CHECK(dist.noData() == -1.0 && dist(0, 0) == -1.0 && dist(1, 1) == 6.0 && dist(2, 2) == 6.0);
  o.stat = DistanceStat::Maximum;
  rdgpu::FlowDistanceDown(props, dist, 3.0, 4.0, o);
  CHECK(dist(1, 1) == 11.0);
  // a channel mask with (3, 1) alone, and the drop: z(A) = 9, z(B) = 5, z(3, 1) = 4.5
  Array2D<uint8_t> chan(6, 4, 0);
  chan(3, 1) = 1;
  Array2D<double> elev(6, 4, 0.0), drop;
  elev(1, 1) = 9.0; elev(2, 1) = 5.0; elev(3, 1) = 4.5; elev(2, 2) = 8.0; elev(3, 2) = 2.0; elev(4, 2) = 1.25;
  o = DistanceDownOptions();
  rdgpu::FlowDistanceDown(props, &elev, &dist, &drop, &chan, 1.0, 1.0, o);   // strict: A has a DEAD receiver
  CHECK(dist(1, 1) == -9999.0 && drop(1, 1) == -9999.0 && dist(2, 1) == 1.0 && drop(2, 1) == 0.5 && drop(3, 1) == 0.0);
  CHECK(dist(4, 2) == -9999.0 && dist(2, 2) == -9999.0);
  o.strict = false;
  rdgpu::FlowDistanceDown(props, &elev, &dist, &drop, &chan, 1.0, 1.0, o);   // lenient: through B alone
  CHECK(dist(1, 1) == 2.0 && drop(1, 1) == 4.5 && dist(2, 2) == -9999.0);
  rdgpu::FlowDistanceDown(props, &elev, static_cast<Array2D<double> *>(nullptr), &drop, static_cast<Array2D<uint8_t> *>(nullptr));
  CHECK(drop(1, 1) == 6.9375 && drop(2, 2) == 6.75);
  Array2D<uint8_t> small(2, 2, 1);
  Array2D<double> *none = nullptr;
  CHECK(thrown([&] { rdgpu::FlowDistanceDown(props, &elev, &dist, none, &small); }).find("raster's size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::FlowDistanceDown(props, &elev, none, none, &chan); }).find("no output") != std::string::npos);
  CHECK(thrown([&] { rdgpu::FlowDistanceDown(props, none, none, &drop, &chan); }).find("elevations") != std::string::npos);
  CHECK(!thrown([&] { rdgpu::FlowDistanceDown(props, dist, 0.0, 1.0); }).empty());        // a zero cell length

  // D-infinity from a DEM: a plane that falls 7 per cell towards the east, 6 x 3, cells 3 wide and 4 high.  The interior
  // cells (1..4, 1) flow east with share 1; the cells on the edge have no receivers.
  Array2D<float> dem(6, 3, 0.0f);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 6; x++) dem(x, y) = 100.0f - 7.0f * x;
  dem.setNoData(-1.0f);
  dem.geotransform = {100.0, 3.0, 0.0, 200.0, 0.0, -4.0};
  dem.projection = "a projection";
  Array2D<double> d2, h2;
  Array2D<uint8_t> *nomask = nullptr;
  rdgpu::DinfDistanceDown(dem, &d2, &h2, nomask);
  CHECK(d2.width() == 6 && d2.height() == 3 && d2.noData() == -9999.0 && h2.noData() == -9999.0);
  CHECK(d2.geotransform == dem.geotransform && d2.projection == dem.projection && h2.geotransform == dem.geotransform);
  for (int x = 0; x < 6; x++) {
    CHECK(d2(x, 0) == 0.0 && d2(x, 2) == 0.0 && h2(x, 0) == 0.0);
    CHECK(d2(x, 1) == (x == 0 ? 0.0 : 3.0 * (5 - x)));
    CHECK(h2(x, 1) == (x == 0 ? 0.0 : 7.0 * (5 - x)));
  }
  Array2D<uint8_t> c2(6, 3, 0);
  c2(3, 1) = 1;
  rdgpu::DinfHand(dem, h2, c2);
  CHECK(h2(1, 1) == 14.0 && h2(2, 1) == 7.0 && h2(3, 1) == 0.0 && h2(4, 1) == -9999.0 && h2(0, 0) == -9999.0);
  Array2D<int16_t> demi(6, 3, 0);
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 6; x++) demi(x, y) = (int16_t)(50 - 2 * x);
  demi.setNoData(-32768);
  demi.geotransform = dem.geotransform;
  rdgpu::DinfDistanceDown(demi, &d2, none, &c2);
  CHECK(d2(1, 1) == 6.0 && d2(3, 1) == 0.0 && d2(4, 1) == -9999.0);
  Array2D<float> bare(6, 3, 1.0f);
  CHECK(thrown([&] { rdgpu::DinfDistanceDown(bare, &d2, none, nomask); }).find("geotransform") != std::string::npos);
  CHECK(thrown([&] { rdgpu::DinfDistanceDown(dem, none, none, nomask); }).find("no output") != std::string::npos);
  CHECK(thrown([&] { rdgpu::DinfHand(dem, h2, small); }).find("raster's size") != std::string::npos);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
