// Extreme-value scores over the VALID pixels of a scored pair (gfx950): exact field quantiles by a radix select, and the sums
// and counts beyond thresholds.  include/orbit2_hip.h: ORBIT2_MASKED_QUANTILES / ORBIT2_MASKED_TAIL of orbit2_masked_loss_fwd
// (loss.hip dispatches); metrics/functional.py field_quantiles, tail_rmse, exceedance_scores; DESIGN 4.10i.
//
// The select.  A value's key is its bit pattern mapped to an unsigned integer of the same order (quantile_select.h).  The key is
// read in four digits of 8 bits, top digit first.  Pass 1 bins the top digit of every valid value of a (field, group) into one
// 256-bin histogram; a scan kernel finds, for each of the up to 2 Q ranks (lo and hi of every level), the bin in which the
// cumulative count crosses the rank, and records that digit as the rank's prefix and the rank inside the bin.  Equal prefixes
// share one slot.  Each later pass bins the next digit of the keys that match a slot's prefix into that slot's histogram; after
// the fourth scan a prefix is a whole key, i.e. the order statistic itself.  Only integers are compared, binned and added, so the
// result is exact and the same from call to call.
//
// Work items, the float4 / scalar path and the validity rule are loss.hip's (masked_rows.h); the grid is score_sums.h's.
#include "masked_rows.h"
#include "quantile_select.h"
#include "../../include/orbit2_hip.h"

namespace {
// the state words of a (field, group) problem: the valid count, the number of slots, every slot's prefix, and for every rank
// (2 j = lo, 2 j + 1 = hi of level j) its slot and its rank among the keys of that prefix
constexpr int QS_STATE = 64, ST_M = 0, ST_NS = 1, ST_PRE = 2, ST_SLOT = ST_PRE + QS_MAX_RANKS, ST_REM = ST_SLOT + QS_MAX_RANKS;
static_assert(ST_REM + QS_MAX_RANKS <= QS_STATE, "state block");
static_assert(QS_MAX_LEVELS == ORBIT2_MASKED_MAX_LEVELS, "levels");
constexpr int QS_PEEL = 4;          // bins a wave adds by popcount before its lanes fall back to one atomic each

// h[idx] += 1 for every lane with `active`, idx < the histogram's size.  Skewed fields put most lanes of a wave into one bin (a
// field at 280 K shares its top digit everywhere; precipitation is mostly exact zeros) and 64 LDS atomics on one word run one
// after the other.  So the wave takes the bin of its first active lane, counts the lanes that share it with one ballot and adds
// the count once, up to QS_PEEL times; what is left goes lane by lane.
__device__ __forceinline__ void bin_add(uint32_t* h, bool active, uint32_t idx) {
  unsigned long long todo = __ballot(active);
  for (int r = 0; r < QS_PEEL && todo; ++r) {
    const int leader = __builtin_ctzll(todo);
    const uint32_t lidx = (uint32_t)__builtin_amdgcn_readlane((int)idx, leader);
    const unsigned long long same = __ballot(active && idx == lidx);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(h + lidx, (uint32_t)__popcll(same));
    active = active && idx != lidx;
    todo &= ~same;
  }
  if (active) atomicAdd(h + idx, 1u);
}

// One digit pass over one (b, c) plane: histograms in LDS, then one global atomicAdd per non-empty bin and workgroup, adjacent
// lanes to adjacent words.  Field 0 = target, 1 = pred.  FIRST: the top digit, one histogram per field; otherwise the digit at
// `shift` of the keys whose higher bits equal a slot's prefix, one histogram per slot (slots = the histograms a problem owns).
template <bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int Ht,
                                                          int Wt, MaskArg mk, uint32_t* __restrict__ hist,
                                                          const uint32_t* __restrict__ state, int C, int H, int W, int G,
                                                          int per_image, int shift, int slots) {
  constexpr int LS = FIRST ? 1 : QS_MAX_RANKS;
  __shared__ uint32_t h[2][LS * QS_BINS];
  __shared__ uint32_t pre[2][QS_MAX_RANKS];
  __shared__ int nsl[2];
  const int plane = blockIdx.y, c = plane % C, b = plane / C;
  const int g = per_image ? plane : c;
  if (FIRST) {
    if (threadIdx.x < 2) nsl[threadIdx.x] = 1;
  } else {
    if (threadIdx.x < 2) {
      const int n = (int)state[(size_t)(threadIdx.x * G + g) * QS_STATE + ST_NS];
      nsl[threadIdx.x] = n < slots ? n : slots;                       // slots <= QS_MAX_RANKS
    }
    if (threadIdx.x < 2 * QS_MAX_RANKS)
      pre[threadIdx.x / QS_MAX_RANKS][threadIdx.x % QS_MAX_RANKS] =
          state[(size_t)((threadIdx.x / QS_MAX_RANKS) * G + g) * QS_STATE + ST_PRE + threadIdx.x % QS_MAX_RANKS];
  }
  __syncthreads();
  const int ns0 = nsl[0], ns1 = nsl[1];
  for (int s = 0; s < ns0; ++s) h[0][s * QS_BINS + threadIdx.x] = 0;
  for (int s = 0; s < ns1; ++s) h[1][s * QS_BINS + threadIdx.x] = 0;
  __syncthreads();
  const float* p = pred + (size_t)plane * H * W;
  const float* t = tgt + (size_t)plane * Ht * Wt;
  const uint8_t* m = mk.m ? mk.m + b * mk.sb + c * mk.sc : nullptr;
  const int W4 = (W + 3) >> 2;
  if (ns0 + ns1 > 0) {
    O2_IMAGE_STRIDE(e, H * W4) {
      const int i = e / W4, j0 = (e - i * W4) << 2;
      float p0[6], t0[4];
      bool v0[6];
      load_row<VEC, false>(p, t, m, i, j0, H, W, Wt, mk.pitch, p0, v0, t0);
      uint32_t kt[4], kp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        kt[k] = qs_key(__float_as_uint(t0[k]));
        kp[k] = qs_key(__float_as_uint(p0[k + 1]));
      }
      if (FIRST) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          bin_add(h[0], v0[k + 1], kt[k] >> shift);
          bin_add(h[1], v0[k + 1], kp[k] >> shift);
        }
      } else {
        int st[4] = {-1, -1, -1, -1}, sp[4] = {-1, -1, -1, -1};          // the slot whose prefix a key carries: at most one
        for (int s = 0; s < ns0; ++s) {
          const uint32_t x = pre[0][s];
#pragma unroll
          for (int k = 0; k < 4; ++k) st[k] = (kt[k] >> (shift + QS_DIGIT_BITS)) == x ? s : st[k];
        }
        for (int s = 0; s < ns1; ++s) {
          const uint32_t x = pre[1][s];
#pragma unroll
          for (int k = 0; k < 4; ++k) sp[k] = (kp[k] >> (shift + QS_DIGIT_BITS)) == x ? s : sp[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          bin_add(h[0], v0[k + 1] && st[k] >= 0, (uint32_t)st[k] * QS_BINS + ((kt[k] >> shift) & (QS_BINS - 1)));
          bin_add(h[1], v0[k + 1] && sp[k] >= 0, (uint32_t)sp[k] * QS_BINS + ((kp[k] >> shift) & (QS_BINS - 1)));
        }
      }
    }
  }
  __syncthreads();
  for (int s = 0; s < ns0; ++s) {
    const uint32_t v = h[0][s * QS_BINS + threadIdx.x];
    if (v) atomicAdd(hist + ((size_t)g * slots + s) * QS_BINS + threadIdx.x, v);
  }
  for (int s = 0; s < ns1; ++s) {
    const uint32_t v = h[1][s * QS_BINS + threadIdx.x];
    if (v) atomicAdd(hist + ((size_t)(G + g) * slots + s) * QS_BINS + threadIdx.x, v);
  }
}

// One workgroup (one wave) per (field, group): thread r < 2 Q follows rank r through this pass's histogram of its slot.  FIRST:
// the histogram's sum is m, and the ranks come from the levels.  LAST: a prefix is a whole key; out and cnt are written.
// Otherwise thread 0 gives equal prefixes one slot each and stores the state of the next pass.
__global__ __launch_bounds__(64) void select_scan_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                         const float* __restrict__ levels, int Q, int G, int slots, int first,
                                                         int last, float* __restrict__ out, int64_t* __restrict__ cnt) {
  __shared__ uint32_t npre[QS_MAX_RANKS], nrem[QS_MAX_RANKS];
  const int prob = blockIdx.x, r = threadIdx.x;
  uint32_t* st = state + (size_t)prob * QS_STATE;
  uint32_t m = 0;
  if (r < 2 * Q) {
    uint32_t rank, slot = 0, prefix = 0;
    if (first) {
      const uint32_t* h0 = hist + (size_t)prob * slots * QS_BINS;
      for (int k = 0; k < QS_BINS; ++k) m += h0[k];
    } else {
      m = st[ST_M];
      slot = st[ST_SLOT + r];
      slot = slot < (uint32_t)slots ? slot : 0;
      prefix = st[ST_PRE + slot];
    }
    if (m) {
      if (first) {
        uint32_t lo, hi;
        double frac;
        qs_position((double)levels[r >> 1], m, &lo, &hi, &frac);
        rank = (r & 1) ? hi : lo;
      } else {
        rank = st[ST_REM + r];
      }
      uint32_t bin, rem;
      qs_scan_step(hist + ((size_t)prob * slots + slot) * QS_BINS, QS_BINS, rank, &bin, &rem);
      npre[r] = (prefix << QS_DIGIT_BITS) | bin;
      nrem[r] = rem;
    }
  }
  __syncthreads();                                   // every read of the old state is done
  if (last) {
    if (r < Q) {
      float* o = out + ((size_t)prob * Q + r) * 3;
      if (!m) {
        o[0] = o[1] = o[2] = __uint_as_float(0x7fc00000u);
      } else {
        uint32_t lo, hi;
        double frac;
        qs_position((double)levels[r], m, &lo, &hi, &frac);
        const float xlo = __uint_as_float(qs_unkey(npre[2 * r])), xhi = __uint_as_float(qs_unkey(npre[2 * r + 1]));
        o[0] = qs_lerp(xlo, xhi, frac);
        o[1] = xlo;
        o[2] = xhi;
      }
      if (r == 0 && prob < G) cnt[prob] = (int64_t)m;     // field 0; field 1 counts the same pixels
    }
  } else if (r == 0) {
    int ns = 0;
    uint32_t sp[QS_MAX_RANKS];
    if (m) {
      for (int k = 0; k < 2 * Q; ++k) {
        int s = 0;
        while (s < ns && sp[s] != npre[k]) ++s;
        if (s == ns) { sp[ns] = npre[k]; st[ST_PRE + ns] = npre[k]; ++ns; }
        st[ST_SLOT + k] = (uint32_t)s;
        st[ST_REM + k] = nrem[k];
      }
    }
    st[ST_M] = m;
    st[ST_NS] = (uint32_t)ns;
  }
}

// ---- the tail: per (b, c) plane and threshold the four sums and three counts over the valid pixels whose target is in the tail,
// and the valid count; per-workgroup partials (fp32 sums: the four waves added in the order w0 + w1 + w2 + w3; int counts) -----
constexpr int TL_T = ORBIT2_MASKED_MAX_LEVELS, TL_V = TL_T * 8;       // values a workgroup reduces: [T][4] sums, [T][4] counts

template <bool VEC, bool LOWER>
__global__ __launch_bounds__(256) void tail_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int Ht, int Wt,
                                                   MaskArg mk, const float* __restrict__ latw, const float* __restrict__ thr,
                                                   float* __restrict__ part, int* __restrict__ partn, int C, int H, int W,
                                                   int T, int per_image) {
  __shared__ float reds[4][TL_T * 4];
  __shared__ int redn[4][TL_T * 4];
  const int plane = blockIdx.y, c = plane % C, b = plane / C;
  const int g = per_image ? plane : c;
  const float* p = pred + (size_t)plane * H * W;
  const float* t = tgt + (size_t)plane * Ht * Wt;
  const uint8_t* m = mk.m ? mk.m + b * mk.sb + c * mk.sc : nullptr;
  const int W4 = (W + 3) >> 2;
  float th[TL_T], s[TL_T][4];
  int n[TL_T][3], nv = 0;
#pragma unroll
  for (int k = 0; k < TL_T; ++k) {
    th[k] = k < T ? thr[(size_t)g * T + k] : 0.f;
    s[k][0] = s[k][1] = s[k][2] = s[k][3] = 0.f;
    n[k][0] = n[k][1] = n[k][2] = 0;
  }
  O2_IMAGE_STRIDE(e, H * W4) {
    const int i = e / W4, j0 = (e - i * W4) << 2;
    float p0[6], t0[4];
    bool v0[6];
    load_row<VEC, false>(p, t, m, i, j0, H, W, Wt, mk.pitch, p0, v0, t0);
    const float w = latw ? latw[i] : 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool v = v0[k + 1];
      const float tv = t0[k], pv = p0[k + 1];
      nv += v ? 1 : 0;
#pragma unroll
      for (int q = 0; q < TL_T; ++q) {
        if (q < T) {
          const bool tin = v && (LOWER ? tv <= th[q] : tv >= th[q]);
          const bool pin = v && (LOWER ? pv <= th[q] : pv >= th[q]);
          const float d = tin ? pv - tv : 0.f, wd = tin ? w : 0.f;         // selects: nothing outside the tail enters a sum
          s[q][0] += wd; s[q][1] += wd * d * d; s[q][2] += wd * fabsf(d); s[q][3] += d;
          n[q][0] += tin ? 1 : 0; n[q][1] += (tin && pin) ? 1 : 0; n[q][2] += (!tin && pin) ? 1 : 0;
        }
      }
    }
  }
  const int wv = threadIdx.x >> 6;
  nv = wave_sum_i(nv);
#pragma unroll
  for (int q = 0; q < TL_T; ++q) {
    if (q < T) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float a = wave_sum(s[q][k]);
        const int c3 = k < 3 ? wave_sum_i(n[q][k < 3 ? k : 0]) : nv;
        if ((threadIdx.x & 63) == 0) { reds[wv][q * 4 + k] = a; redn[wv][q * 4 + k] = c3; }
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < T * 4) {
    const size_t o = ((size_t)plane * ORBIT2_LOSS_BLOCKS + blockIdx.x) * (T * 4) + threadIdx.x;
    part[o] = reds[0][threadIdx.x] + reds[1][threadIdx.x] + reds[2][threadIdx.x] + reds[3][threadIdx.x];
    partn[o] = redn[0][threadIdx.x] + redn[1][threadIdx.x] + redn[2][threadIdx.x] + redn[3][threadIdx.x];
  }
}

// out[e] / cnt[e], e over [B*C][T][4]: the image's nblk partials in workgroup order, sums in double
__global__ __launch_bounds__(256) void tail_final_kernel(const float* __restrict__ part, const int* __restrict__ partn, int nblk,
                                                         int T4, int64_t total, float* __restrict__ out,
                                                         int64_t* __restrict__ cnt) {
  O2_GRID_STRIDE(e, total) {
    const int64_t plane = e / T4;
    const int j = (int)(e - plane * T4);
    double a = 0.0;
    int64_t n = 0;
    for (int k = 0; k < nblk; ++k) {
      const size_t o = ((size_t)plane * ORBIT2_LOSS_BLOCKS + k) * T4 + j;
      a += (double)part[o];
      n += partn[o];
    }
    out[e] = (float)a;
    cnt[e] = n;
  }
}
}  // namespace

int o2_masked_extremes(const float* pred, const float* target, int Ht, int Wt, const MaskArg& mk, const float* lat_w,
                       const float* chan_w, float* out, int64_t* cnt, float* ws, int B, int C, int H, int W, int base, int flags,
                       int n, hipStream_t s) {
  if (!chan_w || n < 1 || n > ORBIT2_MASKED_MAX_LEVELS) return O2_ERR_ARG;
  const int per_image = (flags & ORBIT2_MASKED_PER_IMAGE) ? 1 : 0;
  const bool lower = (flags & ORBIT2_MASKED_LOWER) != 0;
  if ((int64_t)(per_image ? 1 : B) * H * W > 0x7fffffff) return O2_ERR_ARG;      // a group's counts and ranks are 32-bit
  if ((int64_t)B * C > 65535) return O2_ERR_ARG;                                 // planes are blockIdx.y
  const int G = per_image ? B * C : C;
  const int nblk = o2_image_blocks((int64_t)H * ((W + 3) / 4) * 4);              // an item is four pixels
  const bool vec = vec_ok(pred, target, mk, W, Wt);
  if (base == ORBIT2_MASKED_QUANTILES) {
    if (lat_w || lower) return O2_ERR_ARG;
    const int Q = n, S = 2 * Q, P = 2 * G;
    uint32_t* state = reinterpret_cast<uint32_t*>(ws);
    uint32_t* hist1 = state + (size_t)P * QS_STATE;
    uint32_t* histn = hist1 + (size_t)P * QS_BINS;
    if (hipMemsetAsync(ws, 0, sizeof(uint32_t) * (size_t)ORBIT2_QUANTILE_WS_WORDS(G, Q), s) != hipSuccess) return O2_ERR_LAUNCH;
    for (int pass = 0; pass < QS_PASSES; ++pass) {
      const int shift = 32 - QS_DIGIT_BITS * (pass + 1), slots = pass ? S : 1;
      uint32_t* hist = pass ? histn + (size_t)(pass - 1) * P * S * QS_BINS : hist1;
      o2_with_flags(
          [&](auto v, auto first) {
            hipLaunchKernelGGL((select_hist_kernel<decltype(v)::value, decltype(first)::value>), dim3(nblk, B * C), dim3(256), 0,
                               s, pred, target, Ht, Wt, mk, hist, state, C, H, W, G, per_image, shift, slots);
          },
          vec, pass == 0);
      O2_CHECK_LAUNCH();
      hipLaunchKernelGGL(select_scan_kernel, dim3(P), dim3(64), 0, s, hist, state, chan_w, Q, G, slots, pass == 0,
                         pass == QS_PASSES - 1, out, cnt);
      O2_CHECK_LAUNCH();
    }
    return O2_OK;
  }
  const int T = n;
  int* partn = reinterpret_cast<int*>(ws + (size_t)B * C * ORBIT2_LOSS_BLOCKS * 4 * T);
  o2_with_flags(
      [&](auto v, auto low) {
        hipLaunchKernelGGL((tail_kernel<decltype(v)::value, decltype(low)::value>), dim3(nblk, B * C), dim3(256), 0, s, pred,
                           target, Ht, Wt, mk, lat_w, chan_w, ws, partn, C, H, W, T, per_image);
      },
      vec, lower);
  O2_CHECK_LAUNCH();
  const int64_t total = (int64_t)B * C * T * 4;
  hipLaunchKernelGGL(tail_final_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, ws, partn, nblk, T * 4, total, out, cnt);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
