// rd_fill_spill_merge: the reference's app of that name on the GPU engine, native raster files.  The ocean is the bucket
// fill from the edges over the cells at the ocean level (D8) and every NoData cell; the water on ocean cells is set to 0.
// Surface water comes as one level for every cell (--swl X) or as a raster of doubles (--swf FILE).  Runs the depression
// hierarchy (D8) and Fill-Spill-Merge; writes <prefix>-wtd (double: the standing water per cell) and
// <prefix>-hydrologic-surface-height (double: topography + water).
#include "common.hpp"

#include <vector>

template <class T>
struct Fsm {
  static int run(const std::string &in, const std::string &prefix, double ocean_level, bool have_level, double water_level,
                 const std::string &water_file) {
    apps::Array2D<T> topo(in, true);
    apps::Array2D<double> wtd;
    if (have_level) {
      wtd.resize(topo, water_level);
    } else {
      wtd = apps::Array2D<double>(water_file, true);
      if (wtd.width() != topo.width() || wtd.height() != topo.height()) {
        std::cerr << "The topography and the surface water differ in size." << std::endl;
        return -1;
      }
      wtd.geotransform = topo.geotransform;
      wtd.projection = topo.projection;
    }
    wtd.setNoData((double)topo.noData());
    apps::Array2D<uint8_t> ocean(topo.width(), topo.height(), 0);
    rdgpu::BucketFillFromEdges<8>(topo, ocean, (T)ocean_level, (uint8_t)1);
    for (int64_t i = 0; i < (int64_t)topo.size(); i++) {
      if (topo.isNoData(i)) ocean.data()[i] = 1;
      if (ocean.data()[i]) wtd.data()[i] = 0.0;
    }
    apps::Array2D<int32_t> label;
    const std::vector<rdgpu_dephier_node> deps = rdgpu::DepressionHierarchy(topo, 8, label, ocean);
    rdgpu::FillSpillMerge(topo, label, deps, wtd);
    wtd.saveToCache(prefix + "-wtd");
    for (int64_t i = 0; i < (int64_t)topo.size(); i++)
      if (!topo.isNoData(i)) wtd.data()[i] += (double)topo.data()[i];
    wtd.saveToCache(prefix + "-hydrologic-surface-height");
    return 0;
  }
};

static int body(int argc, char **argv) {
  const char *usage = " <topography> <output prefix> <ocean_level> (--swl X | --swf FILE) [type = f32]";
  if (argc < 6 || argc > 7) {
    std::cerr << "Fill-Spill-Merge" << std::endl << argv[0] << usage << std::endl;
    return -1;
  }
  const std::string opt = argv[4];
  if (opt != "--swl" && opt != "--swf") {
    std::cerr << argv[0] << usage << std::endl;
    return -1;
  }
  const bool have_level = opt == "--swl";
  return apps::route<Fsm>(argc > 6 ? argv[6] : "f32", std::string(argv[1]), std::string(argv[2]), std::stod(argv[3]), have_level,
                          have_level ? std::stod(argv[5]) : 0.0, std::string(have_level ? "" : argv[5]));
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
