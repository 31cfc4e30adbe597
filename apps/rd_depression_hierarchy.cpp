// rd_depression_hierarchy: the reference's app of that name on the GPU engine, native raster files.  The ocean is every
// NoData cell and every cell equal to the ocean level, anywhere in the raster (the reference app's rule: no bucket fill);
// the border ring is ocean only where that rule says so.  Writes <prefix>-label (uint32: leaf id + 1, 0 = ocean or
// draining straight into it) and <prefix>-graph.csv, one line per node: a merged node's children carry
// "parent+1,child+1,0", a root carries "geolink+1,child+1,1" (0 where the spill leads into the ocean).
#include "common.hpp"

#include <cstdio>
#include <vector>

template <class T>
struct Hierarchy {
  static int run(const std::string &in, const std::string &prefix, double ocean_level) {
    apps::Array2D<T> topo(in, true);
    apps::Array2D<uint8_t> ocean(topo.width(), topo.height(), 0);
    const T level = (T)ocean_level;
    for (int64_t i = 0; i < (int64_t)topo.size(); i++)
      if (topo.isNoData(i) || topo.data()[i] == level) ocean.data()[i] = 1;
    apps::Array2D<int32_t> leaf;
    const std::vector<rdgpu_dephier_node> deps = rdgpu::DepressionHierarchy(topo, 8, leaf, ocean);
    apps::Array2D<uint32_t> label;
    label.resize(topo, 0);
    label.setNoData(0);
    for (int64_t i = 0; i < (int64_t)topo.size(); i++) label.data()[i] = (uint32_t)(leaf.data()[i] + 1);
    const std::string graph = prefix + "-graph.csv";
    std::FILE *f = std::fopen(graph.c_str(), "w");
    if (!f) {
      std::cerr << "Cannot write " << graph << std::endl;
      return -1;
    }
    std::fprintf(f, "parent,child,oceanlink\n");
    for (size_t i = 0; i < deps.size(); i++) {
      const rdgpu_dephier_node &d = deps[i];
      if (d.parent != RDGPU_DEPHIER_NONE) std::fprintf(f, "%u,%zu,0\n", d.parent + 1, i + 1);
      else std::fprintf(f, "%u,%zu,1\n", d.geolink == RDGPU_DEPHIER_NONE ? 0u : d.geolink + 1, i + 1);
    }
    if (std::fclose(f) != 0) {
      std::cerr << "Cannot write " << graph << std::endl;
      return -1;
    }
    label.saveToCache(prefix + "-label");
    return 0;
  }
};

static int body(int argc, char **argv) {
  if (argc < 4 || argc > 5) {
    std::cerr << "Syntax: " << argv[0] << " <Input> <Output Prefix> <Ocean Level> [type = f32]" << std::endl;
    return -1;
  }
  return apps::route<Hierarchy>(argc > 4 ? argv[4] : "f32", std::string(argv[1]), std::string(argv[2]), std::stod(argv[3]));
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
