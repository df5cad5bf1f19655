// Stand-alone host check of csrc/fss_window.h (tests/test_fss_cpu.py builds and runs it, plainly and with
// -fsanitize=address,undefined): the clamped span, the prefix popcount with its word-boundary rule, the word table of a strip,
// the band partition with its warm-up, and the workspace layout, against brute force, without a GPU.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fss_window.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void check_masks_and_span() {
  CHECK(fss_lowmask(0) == 0ull && fss_lowmask(1) == 1ull && fss_lowmask(63) == 0x7fffffffffffffffull);
  for (int s = 0; s < 64; ++s) CHECK(fss_popcount(fss_lowmask(s)) == (uint32_t)s);
  for (int W : {1, 3, 63, 64, 65, 129, 300})
    for (int r : {0, 1, 3, 16, 32, 64, 127})
      for (int x = 0; x < W + 300; ++x) {
        int a, b;
        fss_span(x, r, W, &a, &b);
        CHECK(0 <= a && a <= b && b <= W);
        if (x < W) CHECK(a == (x - r > 0 ? x - r : 0) && b == (x + r + 1 < W ? x + r + 1 : W) && b > a);
        else CHECK(b == W);
      }
}

// P and the row counts against a bit-by-bit count; the words array has exactly fss_row_words(W) entries, so a read one past the
// row (a = W, W % 64 == 0) is an error the address sanitizer reports
static void check_prefix() {
  for (int W : {1, 3, 63, 64, 65, 71, 128, 129, 200, 256, 257, 640}) {
    const int Wq = fss_row_words(W);
    CHECK(Wq == (W + 63) / 64);
    std::vector<int> bit(W);
    std::vector<uint64_t> words(Wq, 0ull);
    std::vector<uint32_t> prefix(Wq + 1, 0u);
    for (int x = 0; x < W; ++x) {
      bit[x] = (rnd() % 3) != 0;
      if (bit[x]) words[x >> 6] |= 1ull << (x & 63);
    }
    for (int q = 0; q < Wq; ++q) prefix[q + 1] = prefix[q] + fss_popcount(words[q]);
    uint32_t below = 0;
    for (int a = 0; a <= W; ++a) {
      CHECK(fss_row_prefix(words.data(), prefix.data(), a) == below);
      if (a < W) below += bit[a];
    }
    for (int r : {0, 1, 3, 16, 32, 64, 127})
      for (int x = 0; x < W; ++x) {
        int a, b, want = 0;
        fss_span(x, r, W, &a, &b);
        for (int j = x - r; j <= x + r; ++j) want += (j >= 0 && j < W) ? bit[j] : 0;
        CHECK((int)(fss_row_prefix(words.data(), prefix.data(), b) - fss_row_prefix(words.data(), prefix.data(), a)) == want);
      }
  }
}

// the table of FSS_TABLE_WORDS words a strip stages (zero beyond the row, prefixes counted from the strip's base word) serves
// every column of the strip at every window, and the table index never leaves 0 .. FSS_TABLE_WORDS - 1
static void check_strip_table() {
  for (int W : {1, 65, 255, 256, 257, 449, 512, 700, 1440}) {
    const int Wq = fss_row_words(W);
    std::vector<int> bit(W);
    std::vector<uint64_t> words(Wq, 0ull);
    for (int x = 0; x < W; ++x) {
      bit[x] = rnd() & 1;
      if (bit[x]) words[x >> 6] |= 1ull << (x & 63);
    }
    CHECK(fss_strips(W) == (W + FSS_STRIP - 1) / FSS_STRIP);
    for (int r : {0, 1, 2, 31, 32, 33, 63, 64, 65, 126, FSS_MAX_WINDOW / 2})
      for (int strip = 0; strip < fss_strips(W); ++strip) {
        const int x0 = strip * FSS_STRIP, base = fss_strip_base_word(x0, r);
        uint64_t tw[FSS_TABLE_WORDS];
        uint32_t before[FSS_TABLE_WORDS];
        uint32_t run = 0;
        for (int i = 0; i < FSS_TABLE_WORDS; ++i) {
          tw[i] = base + i < Wq ? words[base + i] : 0ull;
          before[i] = run;
          run += fss_popcount(tw[i]);
        }
        for (int t = 0; t < FSS_STRIP; ++t) {
          const int x = x0 + t;
          int a, b, want = 0;
          fss_span(x, r, W, &a, &b);
          const int ia = (a >> 6) - base, ib = (b >> 6) - base;
          CHECK(ia >= 0 && ia < FSS_TABLE_WORDS && ib >= 0 && ib < FSS_TABLE_WORDS);
          if (ia < 0 || ia >= FSS_TABLE_WORDS || ib < 0 || ib >= FSS_TABLE_WORDS) continue;
          const uint32_t h = fss_prefix_at(before[ib], tw[ib], b) - fss_prefix_at(before[ia], tw[ia], a);
          for (int j = x - r; j <= x + r; ++j) want += (j >= 0 && j < W) ? bit[j] : 0;      // x >= W: in range, never a centre
          CHECK((int)h == want);
        }
      }
  }
}

// a band's steps: every row of every centre's window that lies in the plane has entered and not left when the centre is read
static void check_bands() {
  CHECK(fss_band_rows(1, 1) == FSS_MIN_BAND && fss_band_rows(FSS_FILL, 1) == FSS_MAX_BAND);
  CHECK(fss_band_rows(576, 512) == FSS_MAX_BAND);                       // 16 x 3 images, 3 thresholds, 4 strips of 512 rows
  for (long long groups : {1ll, 12ll, 100ll, 500ll, 5000ll})
    for (int H : {1, 31, 33, 64, 65, 200, 721}) {
      const int band = fss_band_rows(groups, H);
      CHECK(band >= FSS_MIN_BAND && band <= FSS_MAX_BAND && (band & (band - 1)) == 0);
      CHECK(band == FSS_MIN_BAND || groups * ((H + band - 1) / band) >= FSS_FILL);              // small enough, or at the floor
      CHECK(band == FSS_MAX_BAND || groups * ((H + 2 * band - 1) / (2 * band)) < FSS_FILL);     // and no smaller than needed
      for (int r : {0, 1, 3, 16, 64, 127}) {
        std::vector<int> seen(H, 0);
        for (int y0 = 0; y0 < H; y0 += band) {
          const int y1 = y0 + band < H ? y0 + band : H;
          std::vector<int> in(H, 0);
          const int first = fss_first_step(y0, r);
          CHECK(first <= y0 && first + r >= 0 && first + r <= (y0 - r > 0 ? y0 - r : 0));
          for (int s = first; s < y1; ++s) {
            if (s + r >= 0 && s + r < H) in[s + r] += 1;
            if (s >= y0) {
              for (int y = 0; y < H; ++y) CHECK(in[y] == ((y >= s - r && y <= s + r) ? 1 : 0));
              seen[s] += 1;
              if (s - r >= 0 && s - r < H) in[s - r] -= 1;
            }
          }
        }
        for (int y = 0; y < H; ++y) CHECK(seen[y] == 1);
      }
    }
}

static void check_workspace() {
  CHECK(fss_planes(1) == 3 && fss_planes(8) == 17);
  for (int T : {1, 3, 8})
    for (int W : {1, 64, 65, 1024}) {
      const int B = 2, C = 3, H = 5, Wq = fss_row_words(W);
      CHECK(fss_ws_words(B, C, H, W, T) == 2ll * B * C * (2 * T + 1) * H * Wq);
      size_t next = 0;                                                  // the layout is dense and in order
      for (int im = 0; im < B * C; ++im)
        for (int p = 0; p < fss_planes(T); ++p)
          for (int y = 0; y < H; ++y)
            for (int q = 0; q < Wq; ++q) CHECK(fss_word_index(im, p, y, q, T, H, Wq) == next++);
      CHECK((long long)next * 2 == fss_ws_words(B, C, H, W, T));
    }
  CHECK(fss_ws_words(65535, 1, 32768, 65536, 8) == 2ll * 65535 * 17 * 32768 * 1024);      // no 32-bit step on the way
}

int main() {
  check_masks_and_span();
  check_prefix();
  check_strip_table();
  check_bands();
  check_workspace();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("fss_window ok\n");
  return 0;
}
