// rd_depressions_breach on the GPU engine, native raster files instead of GDAL ones.
// After reference apps/rd_depressions_breach.cpp: of Lindsay2016()'s modes the engine has COMPLETE breaching without epsilon
// gradients and without a fill afterwards (CompleteBreaching_Lindsay2016<D8>, include/rdgpu.h); the other modes and options
// of the reference's command line are refused by name.
#include "common.hpp"

template <class T>
struct Breach {
  static int run(const std::string &in, const std::string &out) {
    apps::Array2D<T> elevation(in, true);
    rdgpu::CompleteBreaching_Lindsay2016<apps::Topology::D8>(elevation);
    elevation.saveToCache(out);
    return 0;
  }
};

static int body(int argc, char **argv) {
  if (argc < 3 || argc > 5) {
    std::cerr << "Eliminate all depressions via breaching." << std::endl;
    std::cerr << argv[0] << " <Input native raster> <Output native raster> [<Mode> = COMPLETE] [element type = f32]" << std::endl;
    std::cerr << "\t<Mode> - COMPLETE (SELECTIVE and CONSTRAINED are not built)" << std::endl;
    return -1;
  }
  std::string type = "f32";
  for (int i = 3; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "COMPLETE") continue;
    if (a == "SELECTIVE" || a == "CONSTRAINED") throw std::runtime_error("Only COMPLETE breaching is built on the GPU engine.");
    type = a;
  }
  return apps::route<Breach>(type, std::string(argv[1]), std::string(argv[2]));
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
