// rd_upslope_extreme: the largest or smallest value found upstream of every cell of a D8 direction raster (the cell
// included) on the GPU engine, native raster files.  Writes <prefix>_extreme (the values' element type, their NoData where
// nothing contributes) and <prefix>_at_cell (uint32: the flat index of the cell the extreme sits at, the lowest on a tie,
// NoData 0xFFFFFFFF).  Cells whose value is the values' NoData, or a NaN, contribute nothing (include/rdgpu.h states the
// definition).
#include "common.hpp"

template <class T>
struct Extreme {
  static int run(const std::string &dirs_file, const std::string &values_file, const std::string &prefix, int which) {
    apps::Array2D<uint8_t> dirs(dirs_file, true);
    apps::Array2D<T> values(values_file, true);
    if (values.width() != dirs.width() || values.height() != dirs.height()) {
      std::cerr << "The directions and the values differ in size." << std::endl;
      return -1;
    }
    apps::Array2D<T> extreme;
    apps::Array2D<uint32_t> at_cell;
    rdgpu::d8_upslope_extreme(dirs, values, extreme, &at_cell, which);
    extreme.saveToCache(prefix + "_extreme");
    at_cell.saveToCache(prefix + "_at_cell");
    return 0;
  }
};

static int body(int argc, char **argv) {
  const std::string mode = argc >= 5 ? argv[4] : "";
  if (argc < 5 || argc > 6 || (mode != "max" && mode != "min")) {
    std::cerr << "Extreme upslope value of a raster over the drainage area of every cell of a D8 direction raster" << std::endl;
    std::cerr << argv[0] << " <D8 directions native raster (uint8)> <Values native raster> <Output prefix> <max|min> [element type: f32]" << std::endl;
    return -1;
  }
  return apps::route<Extreme>(argc == 6 ? argv[5] : "f32", std::string(argv[1]), std::string(argv[2]), std::string(argv[3]),
                              mode == "max" ? RDGPU_EXTREME_MAX : RDGPU_EXTREME_MIN);
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
