// Stand-alone host check of csrc/quantile_select.h (tests/test_extremes_cpu.py builds and runs it, plainly and with
// -fsanitize=address,undefined): the key map, the scan step and the position arithmetic, without a GPU.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "quantile_select.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static float as_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

static void check_keys() {
  // round trip: every 2^16-th pattern plus the patterns around every edge of the format
  std::vector<uint32_t> pats;
  for (uint64_t b = 0; b < (1ull << 32); b += 65521) pats.push_back((uint32_t)b);
  const uint32_t edges[] = {0x00000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x3f800000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u,
                            0x7fffffffu, 0x80000000u, 0x80000001u, 0x807fffffu, 0x80800000u, 0xbf800000u, 0xff7fffffu, 0xff800000u,
                            0xffc00000u, 0xffffffffu};
  for (uint32_t e : edges) pats.push_back(e);
  for (uint32_t b : pats) CHECK(qs_unkey(qs_key(b)) == b && qs_key(qs_unkey(b)) == b);
  // monotone: the non-NaN patterns in float order -- negatives from -inf up to -0.0, then +0.0 up to +inf -- have rising keys
  uint32_t prev = qs_key(0xff800000u);
  for (uint32_t b = 0xff800000u - 65521; b > 0x80000000u && b < 0xff800000u; b -= 65521) {
    CHECK(as_float(b) > as_float(b + 65521) && qs_key(b) > prev);
    prev = qs_key(b);
  }
  CHECK(qs_key(0x80000000u) > prev);
  prev = qs_key(0x80000000u);
  CHECK(qs_key(0x00000000u) == prev + 1);                       // -0.0 directly below +0.0
  prev = qs_key(0u);
  for (uint32_t b = 1; b <= 0x7f800000u; b += 65521) {
    CHECK(qs_key(b) > prev);
    prev = qs_key(b);
  }
  CHECK(qs_key(0x7f800000u) >= prev);
  // denormals order among themselves and against the smallest normal, as integers
  CHECK(qs_key(0x00000001u) < qs_key(0x00000002u) && qs_key(0x007fffffu) < qs_key(0x00800000u));
  CHECK(qs_key(0x80000002u) < qs_key(0x80000001u) && qs_key(0x80800000u) < qs_key(0x807fffffu));
  // NaNs lie beyond the infinities of their sign
  CHECK(qs_key(0x7fc00000u) > qs_key(0x7f800000u) && qs_key(0xffc00000u) < qs_key(0xff800000u));
}

static void check_scan() {
  uint32_t bin, rem;
  {                                                             // ranks at the bin boundaries, empty bins between
    const uint32_t h[8] = {0, 3, 0, 0, 2, 0, 1, 0};
    const uint32_t want_bin[6] = {1, 1, 1, 4, 4, 6}, want_rem[6] = {0, 1, 2, 0, 1, 0};
    for (uint32_t r = 0; r < 6; ++r) {
      qs_scan_step(h, 8, r, &bin, &rem);
      CHECK(bin == want_bin[r] && rem == want_rem[r]);
    }
    qs_scan_step(h, 8, 6, &bin, &rem);                          // a rank beyond the total: the last bin, in range
    CHECK(bin == 7);
  }
  {                                                             // all mass in the last bin
    uint32_t h[QS_BINS] = {0};
    h[QS_BINS - 1] = 1000;
    qs_scan_step(h, QS_BINS, 0, &bin, &rem);
    CHECK(bin == QS_BINS - 1 && rem == 0);
    qs_scan_step(h, QS_BINS, 999, &bin, &rem);
    CHECK(bin == QS_BINS - 1 && rem == 999);
  }
  {                                                             // all mass in the first bin; counts near 2^31
    uint32_t h[QS_BINS] = {0};
    h[0] = 0x7fffffffu;
    qs_scan_step(h, QS_BINS, 0x7ffffffeu, &bin, &rem);
    CHECK(bin == 0 && rem == 0x7ffffffeu);
    h[1] = 0x7fffffffu;
    qs_scan_step(h, QS_BINS, 0x7fffffffu, &bin, &rem);
    CHECK(bin == 1 && rem == 0);
  }
  {                                                             // exhaustive on small histograms: against a sorted expansion
    for (uint32_t code = 0; code < 4 * 4 * 4 * 4; ++code) {
      const uint32_t h[4] = {code & 3, (code >> 2) & 3, (code >> 4) & 3, (code >> 6) & 3};
      std::vector<uint32_t> owner, within;
      for (uint32_t b = 0; b < 4; ++b)
        for (uint32_t k = 0; k < h[b]; ++k) { owner.push_back(b); within.push_back(k); }
      for (uint32_t r = 0; r < owner.size(); ++r) {
        qs_scan_step(h, 4, r, &bin, &rem);
        CHECK(bin == owner[r] && rem == within[r]);
      }
    }
  }
}

static void check_position() {
  uint32_t lo, hi;
  double f;
  qs_position(0.5, 1, &lo, &hi, &f);      CHECK(lo == 0 && hi == 0 && f == 0.0);            // m = 1
  qs_position(0.0, 1, &lo, &hi, &f);      CHECK(lo == 0 && hi == 0 && f == 0.0);
  qs_position(1.0, 1, &lo, &hi, &f);      CHECK(lo == 0 && hi == 0 && f == 0.0);
  qs_position(0.0, 10, &lo, &hi, &f);     CHECK(lo == 0 && hi == 1 && f == 0.0);            // q = 0: the minimum
  qs_position(1.0, 10, &lo, &hi, &f);     CHECK(lo == 9 && hi == 9 && f == 0.0);            // q = 1: the maximum
  qs_position(0.5, 9, &lo, &hi, &f);      CHECK(lo == 4 && hi == 5 && f == 0.0);            // q (m - 1) integral
  qs_position(0.25, 5, &lo, &hi, &f);     CHECK(lo == 1 && hi == 2 && f == 0.0);
  qs_position(0.5, 10, &lo, &hi, &f);     CHECK(lo == 4 && hi == 5 && f == 0.5);
  qs_position(1.0, 0x7fffffffu, &lo, &hi, &f);  CHECK(lo == 0x7ffffffeu && hi == 0x7ffffffeu && f == 0.0);
  qs_position(-3.0, 10, &lo, &hi, &f);    CHECK(lo == 0 && hi == 1 && f == 0.0);            // outside [0, 1]: clamped, in range
  qs_position(7.0, 10, &lo, &hi, &f);     CHECK(lo == 9 && hi == 9);
  qs_position(nan(""), 10, &lo, &hi, &f); CHECK(lo == 0 && hi == 1);
  for (uint32_t m = 1; m <= 40; ++m)                                                         // always lo <= hi < m, frac in [0, 1)
    for (int k = 0; k <= 1000; ++k) {
      qs_position(k / 1000.0, m, &lo, &hi, &f);
      CHECK(lo <= hi && hi < m && hi - lo <= 1 && f >= 0.0 && f < 1.0);
    }
  CHECK(qs_lerp(1.0f, 3.0f, 0.5) == 2.0f && qs_lerp(1.0f, 3.0f, 0.0) == 1.0f);
  const float big = as_float(0x7f7fffffu);
  CHECK(qs_lerp(-big, big, 0.5) == 0.0f);                                                    // no overflow: the lerp is in double
  CHECK(qs_lerp(2.0f, as_float(0x7f800000u), 0.0) == 2.0f);
}

int main() {
  check_keys();
  check_scan();
  check_position();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("quantile_select ok\n");
  return 0;
}
