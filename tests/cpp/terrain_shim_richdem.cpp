// compile-only: rdgpu::TA_* bind to the unmodified richdem::Array2D<T> (tests/cpp/Makefile.terrain check_richdem)
#include <richdem/common/Array2D.hpp>

#include "rdgpu/richdem_gpu.hpp"

void bind(richdem::Array2D<int16_t> &dem, richdem::Array2D<double> &acc, richdem::Array2D<float> &out) {
  rdgpu::TA_slope_riserun(dem, out);
  rdgpu::TA_slope_percentage(dem, out, 2.0f);
  rdgpu::TA_slope_degrees(dem, out);
  rdgpu::TA_slope_radians(dem, out);
  rdgpu::TA_aspect(dem, out);
  rdgpu::TA_curvature(dem, out);
  rdgpu::TA_planform_curvature(dem, out);
  rdgpu::TA_profile_curvature(dem, out);
  richdem::Array2D<float> spi;
  rdgpu::TA_SPI(acc, out, spi);
  rdgpu::TA_CTI(acc, out, spi);
}
