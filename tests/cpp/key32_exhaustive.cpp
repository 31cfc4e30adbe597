// Key32<float>: the compare-free key (to_fold, what the device code uses) against the key by selects (to, the
// definition), over all 2^32 bit patterns on the host.  Every non-NaN pattern must give the same key, from(key) must give
// the pattern back (-0.0f: +0.0f), and the keys must order the floats as the floats order themselves at the places
// where that can go wrong.  NaN patterns are unsupported input and skipped.  Exit status 0: all equal.
//
//   make -C tests/cpp -f Makefile.key32 key32_exhaustive && tests/cpp/key32_exhaustive
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../richdem_amd/csrc/common.hpp"

using K = rdgpu::Key32<float>;

static float f_of(uint32_t b) {
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}

int main() {
  uint64_t bad = 0, checked = 0;
  uint32_t first_bad = 0;
  for (uint64_t i = 0; i < (1ull << 32); i++) {
    const uint32_t b = (uint32_t)i;
    if ((b & 0x7F800000u) == 0x7F800000u && (b & 0x007FFFFFu)) continue;   // NaN
    const float v = f_of(b);
    const uint32_t ks = K::to(v), kf = K::to_fold(v);
    const float back = K::from(kf);
    uint32_t bb;
    std::memcpy(&bb, &back, 4);
    const uint32_t want = b == 0x80000000u ? 0u : b;
    if (ks != kf || bb != want) {
      if (!bad) first_bad = b;
      bad++;
    }
    checked++;
  }
  // the order at the seams: -inf < -max < -min normal < -max denormal < -min denormal < -0 = +0 < +min denormal < ... < +inf
  const uint32_t seq[] = {0xFF800000u, 0xFF7FFFFFu, 0x80800000u, 0x807FFFFFu, 0x80000001u, 0x80000000u, 0x00000000u,
                          0x00000001u, 0x007FFFFFu, 0x00800000u, 0x7F7FFFFFu, 0x7F800000u};
  const int n = (int)(sizeof(seq) / sizeof(seq[0]));
  for (int a = 0; a + 1 < n; a++) {
    const uint32_t ka = K::to_fold(f_of(seq[a])), kb = K::to_fold(f_of(seq[a + 1]));
    const bool eq = f_of(seq[a]) == f_of(seq[a + 1]);
    if (eq ? ka != kb : !(ka < kb)) {
      std::printf("order broken between %08x and %08x: keys %08x %08x\n", seq[a], seq[a + 1], ka, kb);
      bad++;
    }
  }
  std::printf("key32_exhaustive: %llu non-NaN patterns checked, %llu differ", (unsigned long long)checked, (unsigned long long)bad);
  if (bad) std::printf(" (first: %08x)", first_bad);
  std::printf("\n");
  return bad ? 1 : 0;
}
