// rd_flow_distance: the length of every cell's flow path on the GPU engine, native raster files.  Without a channel raster
// the distance runs to the cell the path finally drains to; with one (uint8, non-zero = channel, e.g. a thresholded
// accumulation) to the first channel cell on the path.  The output is float64 in the units of the directions'
// geotransform, -1 where a cell has no drainage cell (include/rdgpu.h states the definition).
#include "common.hpp"

static int body(int argc, char **argv) {
  if (argc != 3 && argc != 4) {
    std::cerr << "Flow distance to the outlet or to the nearest channel of a D8 direction raster" << std::endl;
    std::cerr << argv[0] << " <D8 directions native raster (uint8)> <Output native raster (float64)> [Channels native raster (uint8)]" << std::endl;
    return -1;
  }
  apps::Array2D<uint8_t> dirs(std::string(argv[1]), true);
  apps::Array2D<double> dist;
  if (argc == 4) {
    apps::Array2D<uint8_t> chan(std::string(argv[3]), true);
    if (chan.width() != dirs.width() || chan.height() != dirs.height()) {
      std::cerr << "The directions and the channels differ in size." << std::endl;
      return -1;
    }
    rdgpu::d8_flow_distance(dirs, dist, &chan);
  } else {
    rdgpu::d8_flow_distance(dirs, dist);
  }
  dist.saveToCache(argv[2]);
  return 0;
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
