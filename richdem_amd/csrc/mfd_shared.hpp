// mfd_shared.hpp -- what the engines on D-infinity / MFD proportions share: the neighbour numbering, the two proportions
// accessors and the compact D-infinity form from a DEM (mfd.hip: accumulation; mfd_distance.hip: distance and drop down
// to the stop cells; mfd_distance_up.hip: distance and rise up to the sources; mfd_reverse.hip: reverse accumulation and
// upslope dependence).  The work list that the engines run on is mfd_worklist.hpp.
#pragma once

#include "common.hpp"

#include <algorithm>

namespace rdgpu {

constexpr int NTHR = 256;
static inline uint32_t sgrid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + NTHR - 1) / NTHR, 256u * 32u); }

__device__ __forceinline__ int mdx(int n) { return (n == 1 || n == 2 || n == 8) ? -1 : (n >= 4 && n <= 6) ? 1 : 0; }
__device__ __forceinline__ int mdy(int n) { return (n >= 2 && n <= 4) ? -1 : (n >= 6 && n <= 8) ? 1 : 0; }

// ------------------------------------------------------------------------------------------
// proportions accessors
// ------------------------------------------------------------------------------------------
struct PropsAcc {   // the reference's Array3D<float>
  const float *props;
  __device__ __forceinline__ bool nodata(uint64_t c) const { return props[9 * c] == -2.0f; }
  __device__ __forceinline__ float share(uint64_t c, int n) const { return props[9 * c + n]; }
};
struct DinfAcc {    // compact D-infinity form
  const uint8_t *rcv;
  const float *sh1, *sh2;
  __device__ __forceinline__ bool nodata(uint64_t c) const { return rcv[c] == 255; }
  __device__ __forceinline__ float share(uint64_t c, int n) const {
    const int rr = rcv[c], r = rr & 0xF;
    if (rr == 255 || r < 1 || r > 8) return -1.0f;
    if (n == r) return sh1[c];
    if ((rr & 0x10) && n == (r == 8 ? 1 : r + 1)) return sh2[c];
    return -1.0f;
  }
};

// FM_Tarboton in compact form into workspace planes (mfd.hip): 5 B/cell, the 36 B/cell array is never materialised
template <class T>
DinfAcc tarboton_device(const T *d_z, T nodata, int w, int h, hipStream_t s);

// The same planes with the cells of drainable flats patched from Barnes' flat mask (mfd.hip: k_tarboton_flats; the rule is
// in DESIGN.md): tarboton_device, d8 directions and resolve_flats_device (flats.hpp) run first.  Synchronises s (the flat
// resolution reads counts back).  The four counts of rdgpu_dinf_flats_get_stats are this call's.
template <class T>
DinfAcc tarboton_flats_device(const T *d_z, T nodata, int w, int h, hipStream_t s);

static inline void check_dims(int w, int h, const char *who, uint64_t max_cells = 0xFFFF0000ull) {
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, std::string(who) + ": width and height must be positive");
  if ((uint64_t)w * (uint64_t)h > max_cells) throw Error(RDGPU_ERR_ARG, std::string(who) + ": raster too large");
}
constexpr uint64_t FLATS_MAX_CELLS = 0x7FFF0000ull;   // the flat resolution's limit: the smaller of the two engines'

// tarboton_device or tarboton_flats_device: what tells an entry point from its `_flats` twin
template <class T>
using TarbotonFn = DinfAcc (*)(const T *, T, int, int, hipStream_t);

}  // namespace rdgpu
