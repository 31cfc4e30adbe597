// flats.hpp -- internal interface of flats.hip
#pragma once
#include "common.hpp"

namespace rdgpu {
// Barnes' flat_mask (M) of the DEM; d_dirs must hold d8_flow_directions output.  Returns workspace pointers through the
// out parameters: M is written for every cell; L (a cell's flat: the lowest cell index of its equal-elevation region) and
// fh (per L value: >= 0 where that flat has a low edge) are null where no flat has an outlet.  A cell's label, as
// k_flat_labels_out exports it, is L[c] + 1 where fh[L[c]] >= 0 and 0 otherwise.  Reads counts back: synchronises s.
template <class T>
void resolve_flats_device(const T *d_z, const uint8_t *d_dirs, int w, int h, int32_t **outM, uint32_t **outL, int32_t **outFh,
                          hipStream_t s);
}  // namespace rdgpu
