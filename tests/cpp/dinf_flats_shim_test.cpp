// tests/cpp/dinf_flats_shim_test.cpp -- D-infinity across flats through include/rdgpu/richdem_gpu.hpp (rdgpu::FM_Tarboton_flats,
// FA_Tarboton_flats, DinfDistanceDown_flats, DinfHand_flats) on a level plateau with one outlet, where the answers are
// known by hand.  Built by tests/cpp/Makefile.dinfflats.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
  // 130 x 67 (two and a bit of the kernel's 64 x 32 tiles each way): the plateau (columns 20..110, rows 10..55) at 5, one
  // outlet cell (111, 30) at 4 and a channel that falls from it to the right edge; around them a rim that rises with the
  // Chebyshev distance, so that no other cell is without a lower neighbour.
  const int W = 130, H = 67, PX0 = 20, PX1 = 110, PY0 = 10, PY1 = 55, OY = 30;
  Array2D<float> dem(W, H, 0.0f);
  auto in_plateau = [&](int x, int y) { return x >= PX0 && x <= PX1 && y >= PY0 && y <= PY1; };
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      if (in_plateau(x, y)) { dem(x, y) = 5.0f; continue; }
      if (y == OY && x > PX1) { dem(x, y) = 4.0f - 0.01f * (float)(x - PX1 - 1); continue; }
      const int dxp = std::max({PX0 - x, x - PX1, 0}), dyp = std::max({PY0 - y, y - PY1, 0});
      int d = std::max(dxp, dyp);                                  // to the plateau
      if (x > PX1) d = std::min(d, std::abs(y - OY));              // to the channel
      dem(x, y) = 10.0f + (float)d;
    }
  dem.setNoData(-9999.0f);
  dem.geotransform = {100.0, 2.0, 0.0, 200.0, 0.0, -3.0};
  dem.projection = "a projection";
  const int NFLAT = (PX1 - PX0 + 1) * (PY1 - PY0 + 1);             // 4186, of which three touch the outlet

  // proportions: FM_Tarboton leaves the plateau without flow, FM_Tarboton_flats routes it
  Array3D<float> plain(W, H, 7.0f), props(W, H, 7.0f);
  rdgpu::FM_Tarboton(dem, plain);
  rdgpu::FM_Tarboton_flats(dem, props);
  CHECK(props.noData() == -2.0f);
  int dry_plain = 0, dry = 0, changed_outside = 0;
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      if (in_plateau(x, y)) {
        dry_plain += plain(x, y, 0) == -1.0f;
        dry += props(x, y, 0) == -1.0f;
        float sum = 0;
        for (int n = 1; n <= 8; n++) sum += props(x, y, n) > 0 ? props(x, y, n) : 0.0f;
        CHECK(std::fabs(sum - 1.0f) < 1e-6f);
      } else
        for (int n = 0; n <= 8; n++) changed_outside += props(x, y, n) != plain(x, y, n);
    }
  CHECK(dry_plain == NFLAT - 3 && dry == 0 && changed_outside == 0);
  CHECK(props(100, OY, 5) == 1.0f && props(PX1, OY, 5) == 1.0f);     // the outlet's row near the outlet: due east
  rdgpu_dinf_flats_stats st;
  CHECK(rdgpu_dinf_flats_get_stats(&st) == 0);
  CHECK(st.noflow_cells == (uint64_t)(NFLAT - 3) && st.patched_cells == st.noflow_cells && st.unresolved_cells == 0);

  // accumulation, one unit per plateau cell: all of it passes the outlet and reaches the raster's edge
  Array2D<double> acc(W, H, 0.0), acc_plain(W, H, 0.0);
  for (int y = PY0; y <= PY1; y++)
    for (int x = PX0; x <= PX1; x++) acc(x, y) = acc_plain(x, y) = 1.0;
  rdgpu::FA_Tarboton_flats(dem, acc);
  rdgpu::FA_Tarboton(dem, acc_plain);
  CHECK(acc.noData() == -1.0);
  CHECK(std::fabs(acc(PX1 + 1, OY) - NFLAT) < 1e-4 * NFLAT && std::fabs(acc(W - 1, OY) - NFLAT) < 1e-4 * NFLAT);
  CHECK(acc_plain(PX1 + 1, OY) == 3.0);
  Array2D<double> small(3, 3, 1.0);
  CHECK(thrown([&] { rdgpu::FA_Tarboton_flats(dem, small); }).find("same dimensions") != std::string::npos);
  Array3D<float> small3(3, 3, 0.0f);
  CHECK(thrown([&] { rdgpu::FM_Tarboton_flats(dem, small3); }).find("dimensions") != std::string::npos);

  // distance and HAND: the channel mask is the outlet and what lies below it
  Array2D<uint8_t> chan(W, H, 0);
  for (int x = PX1 + 1; x < W; x++) chan(x, OY) = 1;
  rdgpu::DistanceDownOptions o;
  o.stat = rdgpu::DistanceStat::Minimum;
  Array2D<double> dist, hand, hand_plain;
  Array2D<double> *none = nullptr;
  rdgpu::DinfDistanceDown_flats(dem, &dist, none, &chan, o);
  CHECK(dist.width() == W && dist.height() == H && dist.noData() == -9999.0);
  CHECK(dist.geotransform == dem.geotransform && dist.projection == dem.projection);
  CHECK(dist(PX1, OY) == 2.0 && dist(PX1 - 10, OY) == 22.0);         // cells 2 wide: one step, eleven steps due east
  int unreached = 0;
  for (int y = PY0; y <= PY1; y++)
    for (int x = PX0; x <= PX1; x++) unreached += !(dist(x, y) > 0.0);
  CHECK(unreached == 0);
  rdgpu::DinfHand_flats(dem, hand, chan, o);
  rdgpu::DinfHand(dem, hand_plain, chan, o);
  int not_one = 0, plain_reached = 0;
  for (int y = PY0; y <= PY1; y++)
    for (int x = PX0; x <= PX1; x++) {
      not_one += hand(x, y) != 1.0;                                    // the plateau stands 1 above its outlet
      plain_reached += hand_plain(x, y) != -9999.0;
    }
  CHECK(not_one == 0 && plain_reached == 3);
  Array2D<uint8_t> badmask(2, 2, 1);
  CHECK(thrown([&] { rdgpu::DinfHand_flats(dem, hand, badmask); }).find("raster's size") != std::string::npos);
  CHECK(thrown([&] { rdgpu::DinfDistanceDown_flats(dem, none, none, &chan); }).find("no output") != std::string::npos);
  Array2D<float> bare(6, 3, 1.0f);
  CHECK(thrown([&] { rdgpu::DinfDistanceDown_flats(bare, &dist, none, &chan); }).find("geotransform") != std::string::npos);
  // an element type outside the D-infinity family
  Array2D<int64_t> wide(6, 3, 1);
  Array3D<float> p6(6, 3, 0.0f);
  Array2D<double> a6(6, 3, 1.0);
  CHECK(!thrown([&] { rdgpu::FM_Tarboton_flats(wide, p6); }).empty());
  CHECK(!thrown([&] { rdgpu::FA_Tarboton_flats(wide, a6); }).empty());
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
