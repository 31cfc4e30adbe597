// rd_longest_flow_path: the length of the longest flow path that ends at every cell of a D8 direction raster on the GPU
// engine, native raster files.  The length is float64 in the units of the directions' geotransform, -1 where a cell has no
// path (NoData, or it drains into a direction loop).  Optionally the flat index of the path's head (uint32, NoData
// 0xFFFFFFFF) and the mask of the longest path of every basin, head to outlet (uint8).  include/rdgpu.h states the
// definition.
#include "common.hpp"

static int body(int argc, char **argv) {
  if (argc < 3 || argc > 5) {
    std::cerr << "Longest upstream flow path of every cell of a D8 direction raster" << std::endl;
    std::cerr << argv[0] << " <D8 directions native raster (uint8)> <Length output (float64)> [<Head cell output (uint32)> [<Basin main path output (uint8)>]]" << std::endl;
    return -1;
  }
  apps::Array2D<uint8_t> dirs(std::string(argv[1]), true);
  apps::Array2D<double> length;
  apps::Array2D<uint32_t> from_cell;
  apps::Array2D<uint8_t> on_basin_path;
  if (argc == 5) rdgpu::d8_longest_flow_path(dirs, length, &from_cell, &on_basin_path);
  else if (argc == 4) rdgpu::d8_longest_flow_path(dirs, length, &from_cell);
  else rdgpu::d8_longest_flow_path(dirs, length);
  length.saveToCache(argv[2]);
  if (argc >= 4) from_cell.saveToCache(argv[3]);
  if (argc == 5) on_basin_path.saveToCache(argv[4]);
  return 0;
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
