// The three host-testable pieces of the radix select (extremes.hip): the order-preserving key of an fp32 bit
// pattern, one scan step (rank -> bin, remaining rank) and the position arithmetic of a linear quantile.  Plain integer and
// double arithmetic, compiled for host and device alike: tests/quantile_select_host.cpp exercises them without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QS_HD __host__ __device__ inline
#else
#define QS_HD inline
#endif

constexpr int QS_DIGIT_BITS = 8;                 // four reads of 8 bits, top digit first
constexpr int QS_BINS = 1 << QS_DIGIT_BITS;
constexpr int QS_PASSES = 32 / QS_DIGIT_BITS;
constexpr int QS_MAX_LEVELS = 8;                 // ORBIT2_MASKED_MAX_LEVELS
constexpr int QS_MAX_RANKS = 2 * QS_MAX_LEVELS;  // lo and hi of every level

// fp32 bit pattern -> unsigned key with the floats' order: all bits of a negative flipped, the sign bit of a non-negative set.
// -0.0 (0x7fffffff) < +0.0 (0x80000000); denormals order exactly whatever the float mode; a NaN sorts beyond the infinity of its
// sign.  Every bit pattern has a key and every key a pattern.
QS_HD uint32_t qs_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
QS_HD uint32_t qs_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }

// One scan step over a histogram of `nbins` counts: the bin in which the cumulative count first exceeds `rank` (0-based), and
// the rank inside that bin.  A rank at or beyond the total lands in the last bin: the result is in range for every input.
QS_HD void qs_scan_step(const uint32_t* hist, int nbins, uint32_t rank, uint32_t* bin, uint32_t* rem) {
  uint32_t before = 0;
  int b = 0;
  for (; b < nbins - 1; ++b) {
    const uint32_t c = hist[b];
    if (rank - before < c) break;               // before <= rank always holds here
    before += c;
  }
  *bin = (uint32_t)b;
  *rem = rank - before;
}

// The two bracketing ranks of level q among m >= 1 sorted values and the weight of the upper one: pos = q (m - 1) in double,
// lo = floor(pos), hi = min(lo + 1, m - 1), frac = pos - lo.  q outside [0, 1] (NaN included) is clamped into it.
QS_HD void qs_position(double q, uint32_t m, uint32_t* lo, uint32_t* hi, double* frac) {
  if (!(q >= 0.0)) q = 0.0;
  if (q > 1.0) q = 1.0;
  const double pos = q * (double)(m - 1);
  uint32_t l = (uint32_t)floor(pos);
  if (l > m - 1) l = m - 1;
  *lo = l;
  *hi = l + 1 < m ? l + 1 : m - 1;
  *frac = pos - (double)l;
}

// the linear quantile between its brackets, in double, rounded once; at frac == 0 the lower bracket itself (an infinite upper
// bracket in pred must not turn 0 * inf into NaN)
QS_HD float qs_lerp(float xlo, float xhi, double frac) {
  if (frac == 0.0) return xlo;
  return (float)((double)xlo + frac * ((double)xhi - (double)xlo));
}
