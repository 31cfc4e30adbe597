// rd_stream_order: Strahler stream order of the channel network on the GPU engine, native raster files.
// The channels are the cells whose accumulation (d8_flow_accum's float64 raster, e.g. rd_flow_accumulation's output for
// algorithm 1 on a unit cell area) reaches the threshold; the order raster is uint8: 0 off the channels, 255 on
// direction loops (include/rdgpu.h states the definition).
#include "common.hpp"

static int body(int argc, char **argv) {
  if (argc != 5) {
    std::cerr << "Strahler stream order of the channels of a D8 direction raster" << std::endl;
    std::cerr << argv[0] << " <D8 directions native raster (uint8)> <Accumulation native raster (float64)> <Threshold> <Output native raster (uint8)>" << std::endl;
    return -1;
  }
  const double threshold = std::stod(argv[3]);
  apps::Array2D<uint8_t> dirs(std::string(argv[1]), true);
  apps::Array2D<double> accum(std::string(argv[2]), true);
  if (accum.width() != dirs.width() || accum.height() != dirs.height()) {
    std::cerr << "The directions and the accumulation differ in size." << std::endl;
    return -1;
  }
  apps::Array2D<uint8_t> chan, order;
  rdgpu::d8_channels(accum, threshold, chan);
  rdgpu::d8_stream_order(dirs, chan, order);
  order.saveToCache(argv[4]);
  return 0;
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
