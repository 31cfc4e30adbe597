// rd_stream_reaches: the reaches of a D8 channel network on the GPU engine, native raster files: the label of every
// channel cell's reach, the label of the reach every cell drains through (both uint32, 0 = none), and one CSV line per
// reach (include/rdgpu.h states the definitions and the record).  Without a channel raster (uint8, non-zero = channel,
// e.g. a thresholded accumulation) every cell with a direction is a channel cell; with an order raster (uint8, e.g.
// rd_stream_order's) the records carry the order.  Lengths are in the units of the directions' geotransform.
#include "common.hpp"

#include <cstdio>
#include <vector>

static int body(int argc, char **argv) {
  if (argc < 5 || argc > 7) {
    std::cerr << "Reach labels, reach catchments and the per-reach table of a D8 direction raster" << std::endl;
    std::cerr << argv[0] << " <D8 directions native raster (uint8)> <Reach labels output (uint32)> <Reach catchments output (uint32)>"
              << " <Table output (CSV)> [Channels native raster (uint8)] [Stream order native raster (uint8)]" << std::endl;
    return -1;
  }
  apps::Array2D<uint8_t> dirs(std::string(argv[1]), true);
  apps::Array2D<uint8_t> chan, order;
  if (argc >= 6) chan = apps::Array2D<uint8_t>(std::string(argv[5]), true);
  if (argc >= 7) order = apps::Array2D<uint8_t>(std::string(argv[6]), true);
  if ((argc >= 6 && (chan.width() != dirs.width() || chan.height() != dirs.height())) ||
      (argc >= 7 && (order.width() != dirs.width() || order.height() != dirs.height()))) {
    std::cerr << "The directions and the channels or the order differ in size." << std::endl;
    return -1;
  }
  apps::Array2D<uint32_t> reach, catchment;
  std::vector<rdgpu_reach> table;
  rdgpu::d8_stream_reaches(dirs, argc >= 6 ? &chan : nullptr, argc >= 7 ? &order : nullptr, reach, catchment, table);
  std::FILE *f = std::fopen(argv[4], "w");
  if (!f) {
    std::cerr << "Cannot write " << argv[4] << std::endl;
    return -1;
  }
  std::fprintf(f, "label,top_cell,bottom_cell,down,up,cells,catchment_cells,steps_x,steps_y,steps_diagonal,order,length\n");
  for (size_t i = 0; i < table.size(); i++) {
    const rdgpu_reach &r = table[i];
    std::fprintf(f, "%zu,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%.17g\n", i + 1, r.top_cell, r.bottom_cell, r.down, r.up, r.cells,
                 r.catchment_cells, r.steps[0], r.steps[1], r.steps[2], r.order, r.length);
  }
  if (std::fclose(f) != 0) {
    std::cerr << "Cannot write " << argv[4] << std::endl;
    return -1;
  }
  reach.saveToCache(argv[2]);
  catchment.saveToCache(argv[3]);
  return 0;
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
