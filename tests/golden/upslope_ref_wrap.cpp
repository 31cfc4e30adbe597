// tests/golden/upslope_ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY (make_golden_upslope.py).
//
// An extern "C" entry over the UNMODIFIED reference's methods/d8_methods.hpp (d8_upslope_cells), compiled by
// make_golden_upslope.py into a temporary directory with the flags of oracle/Makefile.  The directions are wrapped in
// place with the reference's Array2D(T*, w, h).  Returns the output's NoData as the reference set it.
#include <richdem/common/Array2D.hpp>
// d8_upslope_cells hands `flowdirs.data_cells` to its progress bar, a member Array2D no longer has: the template does not
// instantiate as it stands.  The token occurs nowhere else in the reference's headers; spelled as the cell count here it
// feeds the (disabled) progress bar only and the header stays untouched.
#define data_cells size()
#include <richdem/methods/d8_methods.hpp>
#undef data_cells

#include <cstdint>
#include <cstring>

using namespace richdem;

extern "C" int uref_d8_upslope_cells(const uint8_t *dirs, uint8_t nodata, int w, int h, int x0, int y0, int x1, int y1,
                                     uint8_t *out) {
  Array2D<uint8_t> d(const_cast<uint8_t *>(dirs), w, h);
  d.setNoData(nodata);
  Array2D<uint8_t> r;
  d8_upslope_cells(x0, y0, x1, y1, d, r);
  std::memcpy(out, r.data(), (size_t)w * h);
  return (int)r.noData();
}
