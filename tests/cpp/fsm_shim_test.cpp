// tests/cpp/fsm_shim_test.cpp -- rdgpu::DepressionHierarchy, then rdgpu::FillSpillMerge of include/rdgpu/richdem_gpu.hpp on a
// raster whose answer is known by hand (the two-pit raster of tests/fsm_cases.py).  Built by tests/cpp/Makefile.fsm.
#include <cmath>
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
  static_assert(sizeof(rdgpu_fsm_result) == 32, "the record of rdgpu.h");
  // 7 x 5, D8: a ring of 9, the interior 8 but for the middle row 3 6 1 8 8.  Leaf 0 (the 3; level 6, volume 3), leaf 1 (the
  // 1 and the saddle 6; level 6, volume 5), their parent (level 9, the 15 interior cells, volume 29).
  Array2D<int32_t> dem(7, 5, 9);
  for (int y = 1; y < 4; y++)
    for (int x = 1; x < 6; x++) dem.data()[7 * y + x] = 8;
  dem.data()[15] = 3; dem.data()[16] = 6; dem.data()[17] = 1;
  Array2D<int32_t> labels;
  const std::vector<rdgpu_dephier_node> t = rdgpu::DepressionHierarchy(dem, 8, labels);
  CHECK(t.size() == 3);
  // 5 on the first pit: 3 fill it to its saddle, 2 go over the spill pair into the second one; 1 on a ring cell is lost
  Array2D<double> wtd(7, 5, 0.0);
  wtd.data()[15] = 5.0;
  wtd.data()[3] = 1.0;
  std::vector<double> nw;
  rdgpu_fsm_result r = rdgpu::FillSpillMerge(dem, labels, t, wtd, &nw);
  CHECK(r.water_in == 6.0 && r.ocean == 1.0 && r.standing == 5.0 && r.lakes == 2 && r.full_lakes == 1);
  CHECK(nw.size() == 3 && nw[0] == 3.0 && nw[1] == 2.0 && nw[2] == 0.0);
  for (int i = 0; i < 35; i++) CHECK(wtd.data()[i] == (i == 15 ? 3.0 : i == 17 ? 2.0 : 0.0));
  // 20 on the first pit: both leaves fill (3 + 5) and the parent takes the rest; its lake stands at (20 + 106) / 15 = 8.4,
  // above the saddle, over all 15 interior cells
  Array2D<double> more(7, 5, 0.0);
  more.data()[15] = 20.0;
  r = rdgpu::FillSpillMerge(dem, labels, t, more);
  CHECK(r.lakes == 1 && r.full_lakes == 0 && r.ocean == 0.0 && std::fabs(r.standing - 20.0) < 1e-12);
  double sum = 0.0;
  for (int i = 0; i < 35; i++) sum += more.data()[i];
  CHECK(std::fabs(sum + r.ocean - r.water_in) <= 35 * 2.220446049250313e-16 * r.water_in);   // conservation
  const double h = 126.0 / 15.0;
  CHECK(std::fabs(more.data()[17] - (h - 1.0)) < 1e-14 && std::fabs(more.data()[16] - (h - 6.0)) < 1e-14);
  CHECK(std::fabs(more.data()[8] - (h - 8.0)) < 1e-14 && more.data()[0] == 0.0 && more.data()[34] == 0.0);
  // the hierarchy serves a second scenario unchanged; the inputs are inputs
  CHECK(dem.data()[15] == 3 && labels.data()[15] == 0 && labels.data()[17] == 1 && t[2].volume == 29.0);
  // groundwater is refused and the raster stays as it was; a raster of another size is refused
  Array2D<double> neg(7, 5, 0.5);
  neg.data()[9] = -1.0;
  CHECK(!thrown([&] { rdgpu::FillSpillMerge(dem, labels, t, neg); }).empty());
  CHECK(neg.data()[9] == -1.0 && neg.data()[8] == 0.5);
  Array2D<double> small(3, 3, 0.0);
  CHECK(!thrown([&] { rdgpu::FillSpillMerge(dem, labels, t, small); }).empty());
  // no pits: everything goes to the ocean
  Array2D<int16_t> flat(6, 5, 3);
  Array2D<int32_t> flab;
  const std::vector<rdgpu_dephier_node> none = rdgpu::DepressionHierarchy(flat, 8, flab);
  Array2D<double> rain(6, 5, 0.25);
  r = rdgpu::FillSpillMerge(flat, flab, none, rain);
  CHECK(none.empty() && r.lakes == 0 && r.ocean == 7.5 && r.water_in == 7.5 && r.standing == 0.0);
  for (int i = 0; i < 30; i++) CHECK(rain.data()[i] == 0.0);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
