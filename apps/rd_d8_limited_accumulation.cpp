// rd_d8_limited_accumulation: D8 accumulation with losses, decay and capacity on the GPU engine, native raster files.
// Every cell passes on out = min(max(factor * total, 0), max(capacity, 0)) of the total that reached it, its own supply
// included, and keeps the rest; a negative supply is a storage deficit (include/rdgpu.h states the definition).  Writes
// <out> and <kept> (float64, NoData -1 where the direction is NoData) and prints the four sums of the mass balance.
// "-" in place of a file name leaves that raster out; at least one of <out> and <kept> is written.
#include "common.hpp"

#include <cstdio>

template <class T>
static int run(char **argv) {
  const auto given = [&](int i) { return std::string(argv[i]) != "-"; };
  apps::Array2D<uint8_t> dirs(std::string(argv[1]), true);
  apps::Array2D<T> supply(std::string(argv[2]), true), capacity, factor;
  if (given(3)) capacity = apps::Array2D<T>(std::string(argv[3]), true);
  if (given(4)) factor = apps::Array2D<T>(std::string(argv[4]), true);
  for (const apps::Array2D<T> *a : {&supply, given(3) ? &capacity : nullptr, given(4) ? &factor : nullptr})
    if (a && (a->width() != dirs.width() || a->height() != dirs.height())) {
      std::cerr << "The directions, the supply, the capacity and the factor differ in size." << std::endl;
      return -1;
    }
  if (!given(5) && !given(6)) {
    std::cerr << "Neither <Out> nor <Kept> is to be written." << std::endl;
    return -1;
  }
  apps::Array2D<double> out, kept;
  const rdgpu_limited_result r = rdgpu::d8_flow_accum_limited(dirs, supply, given(3) ? &capacity : nullptr, given(4) ? &factor : nullptr,
                                                              given(5) ? &out : nullptr, given(6) ? &kept : nullptr);
  if (given(5)) out.saveToCache(std::string(argv[5]));
  if (given(6)) kept.saveToCache(std::string(argv[6]));
  std::printf("supplied %.17g\nleft %.17g\nkept_pos %.17g\nkept_neg %.17g\n", r.supplied, r.left, r.kept_pos, r.kept_neg);
  return 0;
}

static int body(int argc, char **argv) {
  if (argc < 7 || argc > 8) {
    std::cerr << "D8 accumulation with losses (negative supply), decay (factor) and transport capacity" << std::endl;
    std::cerr << argv[0] << " <D8 directions native raster (uint8)> <Supply native raster> <Capacity | -> <Factor | -> <Out | -> <Kept | ->"
              << " [element type: f32]" << std::endl;
    return -1;
  }
  const std::string type = argc == 8 ? argv[7] : "f32";
  if (type == "f32") return run<float>(argv);
  if (type == "f64") return run<double>(argv);
  std::cerr << "Unknown element type '" << type << "' (f32 f64)" << std::endl;
  return -1;
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
