// The position arithmetic of the fractions skill score (fss.hip): the bit-plane workspace and its size, the clamped
// span of a window, the prefix popcount P with its rule for a position on a word boundary, the word table a strip of columns
// reads, and the partition of a plane into strips and bands with a band's warm-up range.  Plain integer arithmetic, compiled for
// host and device alike: tests/fss_window_host.cpp exercises it without a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSS_HD __host__ __device__ inline
#else
#define FSS_HD inline
#endif

constexpr int FSS_MAX_WINDOW = 255;              // ORBIT2_FSS_MAX_WINDOW: 255^4 fits 32 bits, so a pixel's term is one word
constexpr int FSS_MAX_LEVELS = 8;                // ORBIT2_MASKED_MAX_LEVELS
constexpr int FSS_STRIP = 256;                   // columns of a workgroup: one thread each
constexpr int FSS_TABLE_WORDS = 8;               // words of a row a strip can touch: (FSS_STRIP + FSS_MAX_WINDOW) / 64 rounded out
constexpr int FSS_CHUNK = 16;                    // rows staged per barrier pair
constexpr int FSS_MAX_BAND = 128;                // centre rows of a workgroup ...
constexpr int FSS_MIN_BAND = 32;                 // ... halved down to this while the launch has fewer than
constexpr int FSS_FILL = 1024;                   // this many workgroups (four per CU of 256)

// ---- the workspace: bit planes [B*C][2 T + 1][H][ceil(W / 64)] of 64-bit words; plane 0 = valid, 1 + k = the target's indicator
// of threshold k, 1 + T + k = the prediction's.  Bit x & 63 of word x >> 6 is column x; bits at or beyond W are 0.
FSS_HD int fss_row_words(int W) { return (W + 63) >> 6; }
FSS_HD int fss_planes(int T) { return 2 * T + 1; }
FSS_HD long long fss_ws_words(int B, int C, int H, int W, int T) {      // four-byte words: ORBIT2_FSS_WS_WORDS
  return 2ll * B * C * fss_planes(T) * H * fss_row_words(W);
}
FSS_HD size_t fss_word_index(int image, int plane, int y, int q, int T, int H, int Wq) {
  return (((size_t)image * fss_planes(T) + plane) * H + y) * Wq + q;
}

// ---- a window's columns around x: [a, b) = [max(x - r, 0), min(x + r + 1, W)).  A column at or beyond W (a thread of the last
// strip without a pixel) keeps 0 <= a <= b <= W: its count is in range and never used, its valid bit being 0.
FSS_HD void fss_span(int x, int r, int W, int* a, int* b) {
  const int hi = x + r + 1 < W ? x + r + 1 : W;
  int lo = x - r > 0 ? x - r : 0;
  if (lo > hi) lo = hi;
  *a = lo;
  *b = hi;
}

// the bits below position s of a word, s in 0..63: s = 0 gives 0 with no shift by 64
FSS_HD uint64_t fss_lowmask(int s) { return (1ull << s) - 1ull; }
FSS_HD uint32_t fss_popcount(uint64_t w) { return (uint32_t)__builtin_popcountll(w); }

// P(a) = the set bits of a row at columns below a, from the number of set bits in the words before word a >> 6 (`before`) and
// that word.  The word's part is 0 when a is on a word boundary, whatever the word holds: a caller may then pass anything, and
// fss_row_prefix does not read the word (a = W with W % 64 == 0 names the word one past the row).
FSS_HD uint32_t fss_prefix_at(uint32_t before, uint64_t word, int a) { return before + fss_popcount(word & fss_lowmask(a & 63)); }
FSS_HD uint32_t fss_row_prefix(const uint64_t* words, const uint32_t* wordprefix, int a) {
  return (a & 63) ? fss_prefix_at(wordprefix[a >> 6], words[a >> 6], a) : wordprefix[a >> 6];
}

// ---- the words a strip reads.  The strip's columns x0 .. x0 + FSS_STRIP - 1 (x0 a multiple of FSS_STRIP) ask for P at positions
// max(x0 - r, 0) .. min(x0 + FSS_STRIP + r, W): words base .. base + FSS_TABLE_WORDS - 1 at most, so a table of that many words
// (zero beyond the row) with prefixes counted from `base` serves every thread, and a difference of two P is independent of base.
FSS_HD int fss_strip_base_word(int x0, int r) { return (x0 - r > 0 ? x0 - r : 0) >> 6; }

// ---- the partition.  Strips of FSS_STRIP columns; bands of fss_band_rows centre rows: FSS_MAX_BAND, halved while the launch
// would have fewer than FSS_FILL workgroups.  groups = images x thresholds x strips.
FSS_HD int fss_strips(int W) { return (W + FSS_STRIP - 1) / FSS_STRIP; }
FSS_HD int fss_band_rows(long long groups, int H) {
  int band = FSS_MAX_BAND;
  while (band > FSS_MIN_BAND && groups * ((H + band - 1) / band) < FSS_FILL) band >>= 1;
  return band;
}
// A band of centres y0 .. y1 - 1 walks the steps s = fss_first_step(y0, r) .. y1 - 1: step s adds row s + r to the running sums;
// from s = y0 on it is a centre, and after it row s - r leaves.  Before the first centre the rows y0 - r .. y0 + r - 1 that lie
// in the plane have entered: rows above the plane are skipped, not walked.
FSS_HD int fss_first_step(int y0, int r) { return y0 - 2 * r > -r ? y0 - 2 * r : -r; }
