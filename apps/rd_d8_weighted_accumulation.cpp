// rd_d8_weighted_accumulation: the sum of a weight raster over the drainage area of every cell of a D8 direction raster
// (the cell included) on the GPU engine, native raster files.  Writes <output>: int64 for integer weights, float64 for
// f32 / f64 weights, NoData -1 where the direction is NoData.  Cells whose weight is the weights' NoData, or a NaN, add
// nothing but pass on what they receive (include/rdgpu.h states the definition).
#include "common.hpp"

#include <type_traits>

template <class T>
struct Weighted {
  static int run(const std::string &dirs_file, const std::string &weights_file, const std::string &out_file) {
    apps::Array2D<uint8_t> dirs(dirs_file, true);
    apps::Array2D<T> weights(weights_file, true);
    if (weights.width() != dirs.width() || weights.height() != dirs.height()) {
      std::cerr << "The directions and the weights differ in size." << std::endl;
      return -1;
    }
    apps::Array2D<typename std::conditional<std::is_floating_point<T>::value, double, int64_t>::type> sum;
    rdgpu::d8_flow_accum_weighted(dirs, weights, sum);
    sum.saveToCache(out_file);
    return 0;
  }
};

static int body(int argc, char **argv) {
  if (argc < 4 || argc > 5) {
    std::cerr << "Sum of a weight raster over the drainage area of every cell of a D8 direction raster" << std::endl;
    std::cerr << argv[0] << " <D8 directions native raster (uint8)> <Weights native raster> <Output> [element type: f32]" << std::endl;
    return -1;
  }
  return apps::route<Weighted>(argc == 5 ? argv[4] : "f32", std::string(argv[1]), std::string(argv[2]), std::string(argv[3]));
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
