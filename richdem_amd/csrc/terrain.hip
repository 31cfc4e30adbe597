// terrain.hip -- the reference's TerrainAttribute family (include/richdem/methods/terrain_attributes.hpp):
//
//  * rdgpu_terrain_attribute[s]_*   TA_slope_riserun / _percentage / _degrees / _radians, TA_aspect, TA_curvature,
//                                   TA_planform_curvature, TA_profile_curvature (terrain_attributes.hpp:182-562)
//  * rdgpu_ta_spi_* / _cti_*        TA_SPI / TA_CTI (terrain_attributes.hpp:30-112)
//
// One pass of a 3 x 3 stencil, HBM-bound: sizeof(T) B read + 4 B written per cell and per requested attribute.  The tile
// load is k_flowdirs' (flowdirs.hip); the window a..i, the substitution of the centre for off-grid / NoData neighbours and
// the zscale multiply are shared by every attribute of a launch, and each attribute is one float store to its own plane.
// The arithmetic is the reference's, operation by operation, in double (the build passes -ffp-contract=off: no FMA is
// formed, as on the reference's baseline x86-64): + - * / sqrt are correctly rounded on both sides, so the five
// algebraic attributes are bit-equal; atan / atan2 / log come from the device's libm against glibc's.
#include <cmath>

#include "common.hpp"

namespace rdgpu {

namespace {

constexpr int TW = 64, TH = 32, LW = TW + 2, LH = TH + 2, NTHR = 256;

enum : unsigned {
  M_RISERUN = 1u << RDGPU_TA_SLOPE_RISERUN, M_PERCENT = 1u << RDGPU_TA_SLOPE_PERCENTAGE,
  M_DEGREES = 1u << RDGPU_TA_SLOPE_DEGREES, M_RADIANS = 1u << RDGPU_TA_SLOPE_RADIANS, M_ASPECT = 1u << RDGPU_TA_ASPECT,
  M_CURV = 1u << RDGPU_TA_CURVATURE, M_PLANFORM = 1u << RDGPU_TA_PLANFORM_CURVATURE,
  M_PROFILE = 1u << RDGPU_TA_PROFILE_CURVATURE,
  M_SLOPES = M_RISERUN | M_PERCENT | M_DEGREES | M_RADIANS, M_CURVS = M_CURV | M_PLANFORM | M_PROFILE,
  M_ALL = M_SLOPES | M_ASPECT | M_CURVS
};

struct TaOut {
  float *p[RDGPU_TA_COUNT];   // by attribute id; null where the attribute is not requested
};

constexpr double PI = 3.14159265358979323846;   // M_PI

// MASK: the attributes this instantiation CAN store (compile time: nothing else is computed).  A fused launch uses the
// instantiation of the families it touches and stores the planes whose pointer is set (a block-uniform test).
template <class T, unsigned MASK>
__global__ __launch_bounds__(NTHR) void k_terrain(const T *__restrict__ z, T nodata, TaOut out, float out_nodata,
                                                  double cx, double cy, float zscale_f, int w, int h, uint32_t tilesX,
                                                  uint32_t ntiles) {
  __shared__ T sz[LH * LW];
  const uint32_t t = xcd_tile(blockIdx.x, ntiles);
  if (t >= ntiles) return;
  const int x0 = (int)(t % tilesX) * TW, y0 = (int)(t / tilesX) * TH;
  if (window_inside(x0, y0, w, h, TW, TH, 1)) {
    stage_window_inside<T, TW, TH, 1, LW, NTHR>(z, w, x0, y0, sz);
  } else {
    constexpr int IPT = (LH * LW + NTHR - 1) / NTHR;
    T zv[IPT];
#pragma unroll
    for (int r = 0; r < IPT; r++) {   // clamped addresses: a cell outside the raster is never used as a neighbour
      const int i = min((int)threadIdx.x + r * NTHR, LH * LW - 1);
      const int ly = i / LW, lx = i - ly * LW;
      const int gx = min(max(x0 - 1 + lx, 0), w - 1), gy = min(max(y0 - 1 + ly, 0), h - 1);
      zv[r] = z[(size_t)gy * w + gx];
    }
#pragma unroll
    for (int r = 0; r < IPT; r++) {
      const int i = (int)threadIdx.x + r * NTHR;
      if (i < LH * LW) sz[i] = zv[r];
    }
  }
  __syncthreads();
  const int lx = threadIdx.x & (TW - 1), yb = (int)(threadIdx.x >> 6) * (TH / 4);
  const int gx = x0 + lx;
  const bool left = gx > 0, right = gx < w - 1;   // the neighbour column exists
  const double zscale = (double)zscale_f;
  T r0[3], r1[3], r2[3];
#pragma unroll
  for (int e = 0; e < 3; e++) { r0[e] = sz[yb * LW + lx + e]; r1[e] = sz[(yb + 1) * LW + lx + e]; }
#pragma unroll
  for (int j = 0; j < TH / 4; j++) {
    const int gy = y0 + yb + j;
#pragma unroll
    for (int e = 0; e < 3; e++) r2[e] = sz[(yb + j + 2) * LW + lx + e];
    const bool up = gy > 0, down = gy < h - 1;
    const T ce = r1[1];
    // TerrainSetup (terrain_attributes.hpp:182-207): a neighbour off the grid or == NoData (in T) takes the centre's value
    const double a = (double)((up && left && r0[0] != nodata) ? r0[0] : ce) * zscale;
    const double b = (double)((up && r0[1] != nodata) ? r0[1] : ce) * zscale;
    const double c = (double)((up && right && r0[2] != nodata) ? r0[2] : ce) * zscale;
    const double d = (double)((left && r1[0] != nodata) ? r1[0] : ce) * zscale;
    const double e = (double)ce * zscale;
    const double f = (double)((right && r1[2] != nodata) ? r1[2] : ce) * zscale;
    const double g = (double)((down && left && r2[0] != nodata) ? r2[0] : ce) * zscale;
    const double hh = (double)((down && r2[1] != nodata) ? r2[1] : ce) * zscale;
    const double i = (double)((down && right && r2[2] != nodata) ? r2[2] : ce) * zscale;
    const bool data = !(ce == nodata);
    const bool inside = gx < w && gy < h;
    const size_t o = (size_t)gy * w + gx;
    if (MASK & (M_SLOPES | M_ASPECT)) {   // Horn 1981 (terrain_attributes.hpp:236-263)
      const double dzdx = ((c + 2 * f + i) - (a + 2 * d + g)) / 8 / cx;
      const double dzdy = ((g + 2 * hh + i) - (a + 2 * b + c)) / 8 / cy;
      if (MASK & M_SLOPES) {
        const double rr = sqrt(dzdx * dzdx + dzdy * dzdy);
        if ((MASK & M_RISERUN) && out.p[RDGPU_TA_SLOPE_RISERUN] && inside)
          out.p[RDGPU_TA_SLOPE_RISERUN][o] = data ? (float)rr : out_nodata;
        if ((MASK & M_PERCENT) && out.p[RDGPU_TA_SLOPE_PERCENTAGE] && inside)
          out.p[RDGPU_TA_SLOPE_PERCENTAGE][o] = data ? (float)(rr * 100) : out_nodata;
        if ((MASK & (M_DEGREES | M_RADIANS)) &&
            (out.p[RDGPU_TA_SLOPE_DEGREES] || out.p[RDGPU_TA_SLOPE_RADIANS])) {
          const double at = atan(rr);
          if ((MASK & M_DEGREES) && out.p[RDGPU_TA_SLOPE_DEGREES] && inside)
            out.p[RDGPU_TA_SLOPE_DEGREES][o] = data ? (float)(at * 180 / PI) : out_nodata;
          if ((MASK & M_RADIANS) && out.p[RDGPU_TA_SLOPE_RADIANS] && inside)
            out.p[RDGPU_TA_SLOPE_RADIANS][o] = data ? (float)at : out_nodata;
        }
      }
      if ((MASK & M_ASPECT) && out.p[RDGPU_TA_ASPECT]) {
        // a level window gives atan2(+0, -0) = pi: 270, as the reference computes (not the -1 its comment promises)
        const double t2 = 180.0 / PI * atan2(dzdy, -dzdx);
        double asp;
        if (t2 < 0) asp = 90 - t2;
        else if (t2 > 90.0) asp = 360.0 - t2 + 90.0;
        else asp = 90.0 - t2;
        if (inside) out.p[RDGPU_TA_ASPECT][o] = data ? (float)asp : out_nodata;
      }
    }
    if (MASK & M_CURVS) {   // Zevenbergen and Thorne 1987 (terrain_attributes.hpp:209-228, :265-292); L is cellX only
      const double L = cx;
      const double D = ((d + f) / 2 - e) / L / L;
      const double E = ((b + hh) / 2 - e) / L / L;
      if ((MASK & M_CURV) && out.p[RDGPU_TA_CURVATURE] && inside)
        out.p[RDGPU_TA_CURVATURE][o] = data ? (float)(-2 * (D + E) * 100) : out_nodata;
      if ((MASK & (M_PLANFORM | M_PROFILE)) &&
          (out.p[RDGPU_TA_PLANFORM_CURVATURE] || out.p[RDGPU_TA_PROFILE_CURVATURE])) {
        const double F = (-a + c + g - i) / 4 / L / L;
        const double G = (-d + f) / 2 / L;
        const double H = (b - hh) / 2 / L;
        const bool level = G == 0 && H == 0;
        if ((MASK & M_PLANFORM) && out.p[RDGPU_TA_PLANFORM_CURVATURE] && inside) {
          const double v = level ? 0.0 : (-2 * (D * H * H + E * G * G - F * G * H) / (G * G + H * H) * 100);
          out.p[RDGPU_TA_PLANFORM_CURVATURE][o] = data ? (float)v : out_nodata;
        }
        if ((MASK & M_PROFILE) && out.p[RDGPU_TA_PROFILE_CURVATURE] && inside) {
          const double v = level ? 0.0 : (2 * (D * G * G + E * H * H + F * G * H) / (G * G + H * H) * 100);
          out.p[RDGPU_TA_PROFILE_CURVATURE][o] = data ? (float)v : out_nodata;
        }
      }
    }
#pragma unroll
    for (int e2 = 0; e2 < 3; e2++) { r0[e2] = r1[e2]; r1[e2] = r2[e2]; }
  }
}

// TA_SPI / TA_CTI (terrain_attributes.hpp:44-57, :98-111): log((fa / cellArea) * or / (slope + 0.001)) in double
template <bool CTI>
__global__ __launch_bounds__(256) void k_spi_cti(const double *__restrict__ fa, double fa_nodata,
                                                 const float *__restrict__ slope, float slope_nodata,
                                                 float *__restrict__ out, double area, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double a = fa[i];
    const float s = slope[i];
    float r = -1.0f;   // the NoData the reference sets on its result
    if (!(a == fa_nodata || s == slope_nodata))
      r = CTI ? (float)log((a / area) / (s + 0.001)) : (float)log((a / area) * (s + 0.001));
    out[i] = r;
  }
}

const char *const ATTR_NAME[RDGPU_TA_COUNT] = {"terrain.slope_riserun", "terrain.slope_percentage",
                                               "terrain.slope_degrees", "terrain.slope_radians", "terrain.aspect",
                                               "terrain.curvature", "terrain.planform_curvature",
                                               "terrain.profile_curvature"};

void check_args(const void *dem, int w, int h, double cx, double cy, float zscale, unsigned mask,
                float *const *outs) {
  if (!dem || !outs) throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: null pointer");
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: width and height must be positive");
  if (mask == 0 || (mask & ~(unsigned)M_ALL))
    throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: unknown attribute id (valid ids are 0.." +
                                   std::to_string(RDGPU_TA_COUNT - 1) + ", masks 1.." + std::to_string((unsigned)M_ALL) + ")");
  if (!std::isfinite(cx) || !std::isfinite(cy) || cx == 0 || cy == 0)
    throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: the cell lengths must be finite and non-zero");
  if (!std::isfinite(zscale)) throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: zscale must be finite");
  for (int k = 0; k < RDGPU_TA_COUNT; k++)
    if ((mask >> k & 1u) && !outs[k]) throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: null output pointer");
}

template <class T, unsigned MASK>
void launch(const char *name, const T *d_z, T nodata, const TaOut &o, float out_nodata, double cx, double cy,
            float zscale, int w, int h, hipStream_t s) {
  const uint32_t tilesX = (w + TW - 1) / TW, tilesY = (h + TH - 1) / TH, ntiles = tilesX * tilesY;
  RD_LAUNCH(name, (k_terrain<T, MASK>), dim3(xcd_grid(ntiles)), dim3(NTHR), 0, s, d_z, nodata, o, out_nodata, cx, cy,
            zscale, w, h, tilesX, ntiles);
}

// d_outs[k]: device plane of attribute k for every bit k of mask (other entries are ignored)
template <class T>
void terrain_device(const T *d_z, T nodata, int w, int h, double cx, double cy, float zscale, unsigned mask,
                    float *const *d_outs, float out_nodata, hipStream_t s) {
  check_args(d_z, w, h, cx, cy, zscale, mask, d_outs);
  cx = std::fabs(cx);   // getCellLengthX / Y are |geotransform[1]|, |geotransform[5]|
  cy = std::fabs(cy);
  TaOut o;
  for (int k = 0; k < RDGPU_TA_COUNT; k++) o.p[k] = (mask >> k & 1u) ? d_outs[k] : nullptr;
#define RD_TA_CASE(M, NAME) case M: launch<T, M>(NAME, d_z, nodata, o, out_nodata, cx, cy, zscale, w, h, s); return;
  if ((mask & (mask - 1)) == 0) {   // one attribute: its own instantiation
    switch (mask) {
      RD_TA_CASE(M_RISERUN, ATTR_NAME[0]) RD_TA_CASE(M_PERCENT, ATTR_NAME[1]) RD_TA_CASE(M_DEGREES, ATTR_NAME[2])
      RD_TA_CASE(M_RADIANS, ATTR_NAME[3]) RD_TA_CASE(M_ASPECT, ATTR_NAME[4]) RD_TA_CASE(M_CURV, ATTR_NAME[5])
      RD_TA_CASE(M_PLANFORM, ATTR_NAME[6]) RD_TA_CASE(M_PROFILE, ATTR_NAME[7])
    }
  }
  // several: the instantiation of the families (slopes / aspect / curvatures) the mask touches
  const unsigned fam = ((mask & M_SLOPES) ? M_SLOPES : 0u) | (mask & M_ASPECT) | ((mask & M_CURVS) ? M_CURVS : 0u);
  switch (fam) {
    RD_TA_CASE(M_SLOPES, "terrain.fused") RD_TA_CASE(M_CURVS, "terrain.fused")
    RD_TA_CASE((M_SLOPES | M_ASPECT), "terrain.fused") RD_TA_CASE((M_SLOPES | M_CURVS), "terrain.fused")
    RD_TA_CASE((M_ASPECT | M_CURVS), "terrain.fused") RD_TA_CASE(M_ALL, "terrain.fused")
  }
#undef RD_TA_CASE
  throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: unknown attribute id");
}

template <class T>
void terrain_host(const T *dem, T nodata, int w, int h, double cx, double cy, float zscale, unsigned mask,
                  float *const *outs, float out_nodata) {
  check_args(dem, w, h, cx, cy, zscale, mask, outs);
  const size_t n = (size_t)w * h;
  const int k_out = __builtin_popcount(mask);
  HostStage st;
  const T *d = st.in("host.dem", dem, n);
  float *dd = Workspace::get().buf<float>("host.terrain", n * k_out);   // the planes asked for, back to back in one buffer
  float *planes[RDGPU_TA_COUNT] = {};
  for (int k = 0, j = 0; k < RDGPU_TA_COUNT; k++)
    if (mask >> k & 1u) planes[k] = dd + n * (j++);
  terrain_device<T>(d, nodata, w, h, cx, cy, zscale, mask, planes, out_nodata, nullptr);
  st.finish();
  for (int k = 0; k < RDGPU_TA_COUNT; k++)
    if (mask >> k & 1u) st.fetch(outs[k], planes[k], n);
}

unsigned id_mask(int attribute) {
  if (attribute < 0 || attribute >= RDGPU_TA_COUNT)
    throw Error(RDGPU_ERR_ARG, "rdgpu_terrain_attribute: unknown attribute id " + std::to_string(attribute) +
                                   " (valid ids are 0.." + std::to_string(RDGPU_TA_COUNT - 1) + ")");
  return 1u << attribute;
}

void spi_cti_check(const void *fa, const void *slope, const void *out, int w, int h, double cx, double cy) {
  if (!fa || !slope || !out) throw Error(RDGPU_ERR_ARG, "rdgpu_ta_spi / _cti: null pointer");
  if (w <= 0 || h <= 0) throw Error(RDGPU_ERR_ARG, "rdgpu_ta_spi / _cti: width and height must be positive");
  if (!std::isfinite(cx) || !std::isfinite(cy) || cx == 0 || cy == 0)
    throw Error(RDGPU_ERR_ARG, "rdgpu_ta_spi / _cti: the cell lengths must be finite and non-zero");
}

// arguments checked by the caller (spi_cti_check)
void spi_cti_device(const double *d_fa, double fa_nodata, const float *d_slope, float slope_nodata, int w, int h,
                    double cx, double cy, float *d_out, bool cti, hipStream_t s) {
  const double area = std::fabs(cx * cy);   // getCellArea (Array2D.hpp:1378-1381)
  const size_t n = (size_t)w * h;
  const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 256u * 32u);
  if (cti)
    RD_LAUNCH("terrain.cti", (k_spi_cti<true>), dim3(grid), dim3(256), 0, s, d_fa, fa_nodata, d_slope, slope_nodata,
              d_out, area, n);
  else
    RD_LAUNCH("terrain.spi", (k_spi_cti<false>), dim3(grid), dim3(256), 0, s, d_fa, fa_nodata, d_slope, slope_nodata,
              d_out, area, n);
}

void spi_cti_host(const double *fa, double fa_nodata, const float *slope, float slope_nodata, int w, int h, double cx,
                  double cy, float *out, bool cti) {
  spi_cti_check(fa, slope, out, w, h, cx, cy);
  const size_t n = (size_t)w * h;
  HostStage st;
  const double *dfa = st.in("host.ta_fa", fa, n);
  const float *ds = st.in("host.ta_slope", slope, n);
  float *dout = st.out("host.terrain", out, n);
  spi_cti_device(dfa, fa_nodata, ds, slope_nodata, w, h, cx, cy, dout, cti, nullptr);
  st.finish();
}

}  // namespace

}  // namespace rdgpu

using namespace rdgpu;

#define RD_TERRAIN_API(SUF, T)                                                                                       \
  extern "C" int rdgpu_terrain_attribute_##SUF(const T *dem, T nodata, int w, int h, double cell_x, double cell_y,   \
                                               float zscale, int attribute, float *out, float out_nodata) {          \
    return guarded([&] {                                                                                             \
      float *outs[RDGPU_TA_COUNT] = {};                                                                              \
      const unsigned m = id_mask(attribute);                                                                         \
      outs[attribute] = out;                                                                                         \
      terrain_host<T>(dem, nodata, w, h, cell_x, cell_y, zscale, m, outs, out_nodata);                               \
    });                                                                                                              \
  }                                                                                                                  \
  extern "C" int rdgpu_terrain_attribute_dev_##SUF(const T *d_dem, T nodata, int w, int h, double cell_x,            \
                                                   double cell_y, float zscale, int attribute, float *d_out,         \
                                                   float out_nodata, void *stream) {                                 \
    return guarded([&] {                                                                                             \
      float *outs[RDGPU_TA_COUNT] = {};                                                                              \
      const unsigned m = id_mask(attribute);                                                                         \
      outs[attribute] = d_out;                                                                                       \
      terrain_device<T>(d_dem, nodata, w, h, cell_x, cell_y, zscale, m, outs, out_nodata, (hipStream_t)stream);      \
    });                                                                                                              \
  }                                                                                                                  \
  extern "C" int rdgpu_terrain_attributes_##SUF(const T *dem, T nodata, int w, int h, double cell_x, double cell_y,  \
                                                float zscale, unsigned mask, float *const *outs, float out_nodata) { \
    return guarded([&] { terrain_host<T>(dem, nodata, w, h, cell_x, cell_y, zscale, mask, outs, out_nodata); });     \
  }                                                                                                                  \
  extern "C" int rdgpu_terrain_attributes_dev_##SUF(const T *d_dem, T nodata, int w, int h, double cell_x,           \
                                                    double cell_y, float zscale, unsigned mask,                      \
                                                    float *const *d_outs, float out_nodata, void *stream) {          \
    return guarded([&] {                                                                                             \
      terrain_device<T>(d_dem, nodata, w, h, cell_x, cell_y, zscale, mask, d_outs, out_nodata, (hipStream_t)stream); \
    });                                                                                                              \
  }
RD_TERRAIN_API(u8, uint8_t)
RD_TERRAIN_API(i16, int16_t)
RD_TERRAIN_API(u16, uint16_t)
RD_TERRAIN_API(i32, int32_t)
RD_TERRAIN_API(u32, uint32_t)
RD_TERRAIN_API(f32, float)
RD_TERRAIN_API(f64, double)
RD_TERRAIN_API(i8, int8_t)
RD_TERRAIN_API(i64, int64_t)
RD_TERRAIN_API(u64, uint64_t)

#define RD_SPI_API(NAME, CTI)                                                                                         \
  extern "C" int rdgpu_ta_##NAME(const double *fa, double fa_nodata, const float *slope, float slope_nodata, int w,   \
                                 int h, double cell_x, double cell_y, float *out) {                                   \
    return guarded([&] { spi_cti_host(fa, fa_nodata, slope, slope_nodata, w, h, cell_x, cell_y, out, CTI); });        \
  }                                                                                                                   \
  extern "C" int rdgpu_ta_##NAME##_dev(const double *d_fa, double fa_nodata, const float *d_slope,                    \
                                       float slope_nodata, int w, int h, double cell_x, double cell_y, float *d_out,  \
                                       void *stream) {                                                                \
    return guarded([&] {                                                                                              \
      spi_cti_check(d_fa, d_slope, d_out, w, h, cell_x, cell_y);                                                      \
      spi_cti_device(d_fa, fa_nodata, d_slope, slope_nodata, w, h, cell_x, cell_y, d_out, CTI, (hipStream_t)stream);  \
    });                                                                                                               \
  }
RD_SPI_API(spi, false)
RD_SPI_API(cti, true)
