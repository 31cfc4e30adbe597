// rd_terrain_property on the GPU engine, native raster files instead of GDAL ones.
// Mirrors reference apps/rd_terrain_property.cpp: <DEM> <Output> <Algorithm #> <Z scaling factor>, algorithms 1..8 in the
// reference's order; the result raster starts as result(dem), so it keeps the DEM's NoData value (cast to float).
#include "common.hpp"

template <class T>
struct Terrain {
  static int run(const std::string &in, const std::string &out, int algorithm, float z_scale) {
    apps::Array2D<T> dem(in, true);
    apps::Array2D<float> result;
    result.setNoData((float)dem.noData());
    switch (algorithm) {
    case 1: rdgpu::TA_slope_riserun(dem, result, z_scale); break;
    case 2: rdgpu::TA_slope_percentage(dem, result, z_scale); break;
    case 3: rdgpu::TA_slope_degrees(dem, result, z_scale); break;
    case 4: rdgpu::TA_slope_radians(dem, result, z_scale); break;
    case 5: rdgpu::TA_aspect(dem, result, z_scale); break;
    case 6: rdgpu::TA_curvature(dem, result, z_scale); break;
    case 7: rdgpu::TA_planform_curvature(dem, result, z_scale); break;
    case 8: rdgpu::TA_profile_curvature(dem, result, z_scale); break;
    default: throw std::runtime_error("Unknown algorithm number (1..8)!");
    }
    result.saveToCache(out);
    return 0;
  }
};

static int body(int argc, char **argv) {
  if (argc < 5 || argc > 6) {
    std::cerr << "Calculate terrain attributes. Ensure that vertical and horizontal axes have the same units!" << std::endl;
    std::cerr << argv[0] << " <DEM native raster> <Output native raster (float32)> <Algorithm #> <Z scaling factor> [element type: f32]" << std::endl;
    std::cerr << "Algorithms:" << std::endl;
    std::cerr << " 1: Slope (Rise/Run)   - Horn (1981)" << std::endl;
    std::cerr << " 2: Slope (Percentage) - Horn (1981)" << std::endl;
    std::cerr << " 3: Slope (Degrees)    - Horn (1981)" << std::endl;
    std::cerr << " 4: Slope (Radians)    - Horn (1981)" << std::endl;
    std::cerr << " 5: Aspect             - Horn (1981)" << std::endl;
    std::cerr << " 6: Curvature          - Zevenbergen and Thorne (1987)" << std::endl;
    std::cerr << " 7: Planform Curvature - Zevenbergen and Thorne (1987)" << std::endl;
    std::cerr << " 8: Profile Curvature  - Zevenbergen and Thorne (1987)" << std::endl;
    return -1;
  }
  return apps::route<Terrain>(argc == 6 ? argv[5] : "f32", std::string(argv[1]), std::string(argv[2]), std::stoi(argv[3]),
                              std::stof(argv[4]));
}
int main(int argc, char **argv) { return apps::guarded_main(body, argc, argv); }
