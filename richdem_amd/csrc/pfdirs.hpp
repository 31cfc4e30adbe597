// pfdirs.hpp -- the Priority-Flood tree of pfdirs.hip for the other engines (breach.hip).
#pragma once

#include "common.hpp"

namespace rdgpu {
namespace pfd {

// How the stable queue (elevation, then insertion order) is fed -- which decides the tree where elevations are equal:
//   PFD_CONV_BARNES   PriorityFloodFlowdirs_Barnes2014: the border cells are pushed by its two set-up loops (top and bottom
//                     row cell by cell, then the side columns), a popped cell pushes its neighbours in d8_order
//                     (1, 3, 5, 7, 2, 4, 6, 8), and interior cells equal to NoData carry no direction.
//   PFD_CONV_LINDSAY  CompleteBreaching_Lindsay2016: the border cells are pushed in raster order, a popped cell pushes its
//                     neighbours in the order 1 .. 8, and no cell is NoData.
enum { PFD_CONV_BARNES = 0, PFD_CONV_LINDSAY = 1 };

// The flood's tree of the raster d_z (no NoData) under the convention conv: every interior cell's direction points at the
// neighbour that pushed it; the border cells hold the outward codes of rdgpu_pf_flowdirs.  stats: what
// rdgpu_pf_flowdirs_get_stats would report for this flood (that entry's own record is left as it was).  Synchronises s.
template <class T>
void pf_tree_device(const T *d_z, int w, int h, uint8_t *d_dirs, int conv, hipStream_t s, rdgpu_pf_flowdirs_stats *stats);

}  // namespace pfd
}  // namespace rdgpu
