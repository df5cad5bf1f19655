// The fractions skill score over the VALID pixels of a scored pair (gfx950): neighbourhood verification with windows of up to 255
// pixels at a cost that does not grow with the window.  include/orbit2_hip.h: ORBIT2_FSS_KIND of orbit2_masked_loss_fwd (loss.hip
// dispatches); metrics/functional.py fss, fss_profile; DESIGN 4.10j.
//
// Pass 1 turns the fields into bit planes: a wave reads 64 consecutive pixels of a row once and its ballots ARE the 64-pixel
// words of the valid plane and of the target's and the prediction's indicator at every threshold.  Pass 2 gives one thread a
// column and one workgroup a strip of columns, a band of rows and one threshold.  The number of set bits in a window's columns
// of one row is a difference of two prefix popcounts over that row's words (fss_window.h), whatever the window; the window's
// rows are a running sum that the row entering at the bottom is added to and the row leaving at the top is taken from, both
// recomputed from the bit words.  Everything is an integer: the sums are exact and the same from call to call.
#include "masked_rows.h"
#include "fss_window.h"
#include "../../include/orbit2_hip.h"

static_assert(FSS_MAX_WINDOW == ORBIT2_FSS_MAX_WINDOW && FSS_MAX_LEVELS == ORBIT2_MASKED_MAX_LEVELS, "header constants");
static_assert(FSS_STRIP == 256 && FSS_STRIP / 64 == 4, "one thread per column, four waves");
static_assert(FSS_CHUNK * 2 * FSS_TABLE_WORDS == 256, "one staged word per thread and set");
// whole words back to x0 - r, whole words on to x0 + FSS_STRIP + r, and the word of that last position
static_assert((FSS_MAX_WINDOW / 2 + 63) / 64 + (FSS_STRIP + FSS_MAX_WINDOW / 2) / 64 + 1 <= FSS_TABLE_WORDS, "words a strip can touch");

namespace {
// ---- pass 1: a wave per 64 pixels of a row; lanes 0 .. 2 T store the 2 T + 1 ballots ------------------------------------------
template <bool LOWER>
__global__ __launch_bounds__(256) void fss_bits_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int Ht, int Wt,
                                                       MaskArg mk, const float* __restrict__ thr, uint64_t* __restrict__ planes,
                                                       int C, int H, int W, int T, int per_image) {
  const int image = blockIdx.y, c = image % C, b = image / C;
  const int g = per_image ? image : c;
  const int Wq = fss_row_words(W), lane = threadIdx.x & 63;
  const float* p = pred + (size_t)image * H * W;
  const float* t = tgt + (size_t)image * Ht * Wt;
  const uint8_t* m = mk.m ? mk.m + b * mk.sb + c * mk.sc : nullptr;
  float th[FSS_MAX_LEVELS];
#pragma unroll
  for (int k = 0; k < FSS_MAX_LEVELS; ++k) th[k] = k < T ? thr[(size_t)g * T + k] : 0.f;
  const int items = H * Wq;
  for (int it = blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += gridDim.x * 4) {      // uniform in the wave
    const int y = it / Wq, q = it - y * Wq, x = q * 64 + lane;
    float pv = 0.f, tv = 0.f;
    bool v = false;
    if (x < W) {
      pv = p[(size_t)y * W + x];
      tv = t[(size_t)y * Wt + x];
      v = finite_f(tv) && (!m || m[(size_t)y * mk.pitch + x] != 0);
    }
    unsigned long long mine = __ballot(v);
#pragma unroll
    for (int k = 0; k < FSS_MAX_LEVELS; ++k) {
      if (k < T) {
        const unsigned long long bo = __ballot(v && (LOWER ? tv <= th[k] : tv >= th[k]));    // a NaN compares false
        const unsigned long long bm = __ballot(v && (LOWER ? pv <= th[k] : pv >= th[k]));
        mine = lane == 1 + k ? bo : mine;
        mine = lane == 1 + T + k ? bm : mine;
      }
    }
    if (lane < fss_planes(T)) planes[fss_word_index(image, lane, y, q, T, H, Wq)] = mine;
  }
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------------
struct FssEnt {
  uint64_t w;                        // a word of the row
  uint32_t before;                   // the set bits of the table's words before it
  uint32_t pad;
};

// one staged word per thread: row `row` (zero outside the plane), word column q (zero beyond the row); the prefix over the
// table's 8 words by a segmented scan in the wave
__device__ __forceinline__ void fss_stage(FssEnt* dst, const uint64_t* __restrict__ plane, int row, int q, int wi, int H, int Wq) {
  uint64_t w = 0;
  if (row >= 0 && row < H && q < Wq) w = plane[(size_t)row * Wq + q];
  const uint32_t pc = fss_popcount(w);
  uint32_t incl = pc;
#pragma unroll
  for (int o = 1; o < FSS_TABLE_WORDS; o <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, o, FSS_TABLE_WORDS);
    incl += wi >= o ? up : 0u;
  }
  dst->w = w;
  dst->before = incl - pc;
  dst->pad = 0;
}

// the set bits of a row's field in the thread's span [a, b): P(b) - P(a)
__device__ __forceinline__ uint32_t fss_row_count(const FssEnt* row, int ia, int ib, int a, int b) {
  const FssEnt ea = row[ia], eb = row[ib];
  return fss_prefix_at(eb.before, eb.w, b) - fss_prefix_at(ea.before, ea.w, a);
}

// blockIdx.x = band * strips + strip, blockIdx.y = image, blockIdx.z = threshold
__global__ __launch_bounds__(256) void fss_window_kernel(const uint64_t* __restrict__ planes, unsigned long long* __restrict__ cnt,
                                                         int H, int W, int T, int r, int strips, int band) {
  __shared__ FssEnt ent[2][FSS_CHUNK][2][FSS_TABLE_WORDS];         // [entering, leaving][row of the chunk][target, pred][word]
  __shared__ uint64_t vw[FSS_CHUNK][FSS_STRIP / 64];               // the valid words of the chunk's centre rows
  __shared__ unsigned long long red[4][4];
  const int strip = blockIdx.x % strips, y0 = (blockIdx.x / strips) * band, image = blockIdx.y, k = blockIdx.z;
  const int y1 = y0 + band < H ? y0 + band : H;
  const int Wq = fss_row_words(W), x0 = strip * FSS_STRIP, x = x0 + (int)threadIdx.x;
  const int base = fss_strip_base_word(x0, r);
  int a, b;
  fss_span(x, r, W, &a, &b);
  const int ia = (a >> 6) - base, ib = (b >> 6) - base;             // 0 .. FSS_TABLE_WORDS - 1 (fss_window.h)
  const int vword = threadIdx.x >> 6, vbit = threadIdx.x & 63;
  const uint64_t* pv = planes + fss_word_index(image, 0, 0, 0, T, H, Wq);
  // the word this thread stages in each set
  const int srow = threadIdx.x >> 4, sfield = (threadIdx.x >> 3) & 1, swi = threadIdx.x & (FSS_TABLE_WORDS - 1);
  const uint64_t* sp = planes + fss_word_index(image, 1 + sfield * T + k, 0, 0, T, H, Wq);
  uint32_t cO = 0, cM = 0;
  unsigned long long nv = 0, sO = 0, sM = 0, sD = 0;
  for (int s0 = fss_first_step(y0, r); s0 < y1; s0 += FSS_CHUNK) {
    const bool live = s0 + FSS_CHUNK > y0;                         // the chunk holds centres
    __syncthreads();
    fss_stage(&ent[0][srow][sfield][swi], sp, s0 + srow + r, base + swi, swi, H, Wq);
    if (live) {
      fss_stage(&ent[1][srow][sfield][swi], sp, s0 + srow - r, base + swi, swi, H, Wq);
      if (threadIdx.x < FSS_CHUNK * 4) {
        const int row = s0 + (int)(threadIdx.x >> 2), q = (x0 >> 6) + (int)(threadIdx.x & 3);
        vw[threadIdx.x >> 2][threadIdx.x & 3] = (row >= 0 && row < H && q < Wq) ? pv[(size_t)row * Wq + q] : 0ull;
      }
    }
    __syncthreads();
    const int rows = y1 - s0 < FSS_CHUNK ? y1 - s0 : FSS_CHUNK;
    for (int i = 0; i < rows; ++i) {
      cO += fss_row_count(ent[0][i][0], ia, ib, a, b);
      cM += fss_row_count(ent[0][i][1], ia, ib, a, b);
      if (s0 + i >= y0) {                                          // uniform: a centre row
        if ((vw[i][vword] >> vbit) & 1ull) {
          const uint32_t d = cO > cM ? cO - cM : cM - cO;
          nv += 1;
          sO += (unsigned long long)(cO * cO);                     // <= 255^4 < 2^32
          sM += (unsigned long long)(cM * cM);
          sD += (unsigned long long)(d * d);
        }
        cO -= fss_row_count(ent[1][i][0], ia, ib, a, b);
        cM -= fss_row_count(ent[1][i][1], ia, ib, a, b);
      }
    }
  }
  const unsigned long long v4[4] = {nv, sO, sM, sD};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned long long s = (unsigned long long)wave_sum_i64((int64_t)v4[j]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const unsigned long long s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (s) atomicAdd(cnt + ((size_t)image * T + k) * 4 + threadIdx.x, s);
  }
}

// out[e] = 1 - cnt[e][3] / (cnt[e][1] + cnt[e][2]) in double, NaN where both are 0
__global__ __launch_bounds__(256) void fss_final_kernel(const int64_t* __restrict__ cnt, float* __restrict__ out, int64_t total) {
  O2_GRID_STRIDE(e, total) {
    const int64_t c1 = cnt[e * 4 + 1], c2 = cnt[e * 4 + 2], c3 = cnt[e * 4 + 3];
    out[e] = (c1 == 0 && c2 == 0) ? __uint_as_float(0x7fc00000u) : (float)(1.0 - (double)c3 / ((double)c1 + (double)c2));
  }
}
}  // namespace

int o2_masked_fss(const float* pred, const float* target, int Ht, int Wt, const MaskArg& mk, const float* lat_w,
                  const float* chan_w, float* out, int64_t* cnt, float* ws, int B, int C, int H, int W, int flags, int T, int n,
                  hipStream_t s) {
  if (!chan_w || lat_w || T < 1 || T > ORBIT2_MASKED_MAX_LEVELS) return O2_ERR_ARG;
  if (n < 1 || n > ORBIT2_FSS_MAX_WINDOW || !(n & 1) || !aligned(ws, 8)) return O2_ERR_ARG;
  const int per_image = (flags & ORBIT2_MASKED_PER_IMAGE) ? 1 : 0;
  if ((int64_t)(per_image ? 1 : B) * H * W > 0x7fffffff) return O2_ERR_ARG;      // an int64 sum holds fewer than 2^31 terms of 255^4
  if ((int64_t)B * C > 65535) return O2_ERR_ARG;                                 // images are blockIdx.y
  const int Wq = fss_row_words(W), r = n / 2, strips = fss_strips(W);
  const int band = fss_band_rows((long long)B * C * T * strips, H);
  const int64_t wgs = (int64_t)strips * ((H + band - 1) / band);
  if (wgs > 0x7fffffff) return O2_ERR_ARG;
  uint64_t* planes = reinterpret_cast<uint64_t*>(ws);
  if (hipMemsetAsync(cnt, 0, sizeof(int64_t) * (size_t)B * C * T * 4, s) != hipSuccess) return O2_ERR_LAUNCH;
  const int nblk = grid_for((int64_t)H * Wq, 4 * 8, 256);                        // a wave takes about eight words
  o2_with_flags(
      [&](auto low) {
        hipLaunchKernelGGL((fss_bits_kernel<decltype(low)::value>), dim3(nblk, B * C), dim3(256), 0, s, pred, target, Ht, Wt, mk,
                           chan_w, planes, C, H, W, T, per_image);
      },
      (flags & ORBIT2_MASKED_LOWER) != 0);
  O2_CHECK_LAUNCH();
  hipLaunchKernelGGL(fss_window_kernel, dim3((unsigned)wgs, B * C, T), dim3(256), 0, s, planes,
                     reinterpret_cast<unsigned long long*>(cnt), H, W, T, r, strips, band);
  O2_CHECK_LAUNCH();
  const int64_t total = (int64_t)B * C * T;
  hipLaunchKernelGGL(fss_final_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, cnt, out, total);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
