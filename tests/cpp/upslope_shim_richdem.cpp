// compile-only: rdgpu::d8_upslope_cells / d8_catchments / d8_outlets bind to the unmodified richdem::Array2D<T>
// (tests/cpp/Makefile.upslope check_richdem)
#include <richdem/common/Array2D.hpp>

#include "rdgpu/richdem_gpu.hpp"

void bind(const richdem::Array2D<uint8_t> &dirs, richdem::Array2D<uint8_t> &up, richdem::Array2D<int32_t> &labels,
          richdem::Array2D<uint32_t> &outlets) {
  rdgpu::d8_upslope_cells(1, 2, 3, 4, dirs, up);
  rdgpu::d8_upslope_cells(1, 2, 3, 4, dirs, labels);
  rdgpu::d8_catchments(dirs, {1u, 2u}, {3, 4}, labels, -1);
  rdgpu::d8_outlets(dirs, outlets);
}
