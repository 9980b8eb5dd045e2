// Host check of lm_logf_pos_k (csrc/lora_libm.h), the lockstep logf of the impairment kernel's
// Box-Muller step, against this host's glibc: every u = (2 m + 1) * 2^-24, m = 0 .. 2^23 - 1 -
// all the values the kernel can ask for - plus a strided sweep of the positive normal floats.
// Prints "<name> <inputs> <mismatches>" per sweep.  Built by tests/test_libm_logf_pos.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../lora-sdr-lightweight-standalone-library-_amd/csrc/lora_libm.h"

static long differ(const float* x) {
  float got[2];
  lm_logf_pos_k<2>(x, got);
  long bad = 0;
  for (int k = 0; k < 2; ++k) {
    const float want = logf(x[k]);
    bad += memcmp(&want, &got[k], 4) != 0;
  }
  return bad;
}

int main() {
  long n = 0, bad = 0;
  for (uint32_t m = 0; m < (1u << 23); m += 2, n += 2) {
    const float x[2] = {(float)(2 * m + 1) * 0x1p-24f, (float)(2 * m + 3) * 0x1p-24f};
    bad += differ(x);
  }
  printf("box_muller_u %ld %ld\n", n, bad);
  n = bad = 0;
  for (uint32_t b = 0x00800000u; b < 0x7f800000u - 122u; b += 122u, n += 2) {  // positive normals, 1.0f left out
    const uint32_t b1 = b + 61u;
    if (b == 0x3f800000u || b1 == 0x3f800000u) continue;
    float x[2];
    memcpy(&x[0], &b, 4);
    memcpy(&x[1], &b1, 4);
    bad += differ(x);
  }
  printf("positive_normals %ld %ld\n", n, bad);
  return 0;
}
