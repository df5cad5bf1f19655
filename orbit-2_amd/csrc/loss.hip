// The fused training losses (mse / bayesian_tv / image gradient with latitude and variable weights) and the twelve evaluation
// moments, each plain and over the VALID pixels only (gfx950).  include/orbit2_hip.h: orbit2_loss_*, orbit2_eval_moments,
// orbit2_masked_*; metrics/functional.py; DESIGN 4.10d.  orbit2_loss_bwd hands kind ORBIT2_LOSS_SSIM_VJP on to ssim.hip.
//
//   valid(b,c,i,j) = isfinite(target[b,c,i,j]) and (mask == NULL or mask[b,c,i,j] != 0)
//
// At an invalid pixel neither pred nor target enters any arithmetic: every use is a SELECT (v ? x : 0), never a product with
// the validity -- 0 * NaN is NaN, and clip_replace_constant copies NaN targets of constant channels into pred.
//
// One work item is 4 consecutive pixels of one row.  When every row of pred, target and mask starts on a 16-byte (mask:
// 4-byte) boundary the item's centre is one float4 / one dword per operand (VEC); otherwise the same item is read by four
// guarded scalar lanes (masked_rows.h: load_row, vec_ok).  The total-variation stencil needs the pixels left and right of the
// group and the rows above (backward) and below: those edge pixels are scalar loads, and a pixel outside the plane is invalid.
//
// orbit2_masked_loss_fwd hands the kinds ORBIT2_MASKED_QUANTILES and ORBIT2_MASKED_TAIL on to extremes.hip.
#include "masked_rows.h"
#include "../../include/orbit2_hip.h"

namespace {
// ---- shared by the plain and the masked kernels -------------------------------------------------------------------------------
// flat index over [B][C][H][Wq] -> its four coordinates (Wq = W, or the four-pixel items of a row)
__device__ __forceinline__ void plane_of(int64_t q, int C, int H, int Wq, int& b, int& c, int& i, int& j) {
  j = (int)(q % Wq); q /= Wq;
  i = (int)(q % H); q /= H;
  c = (int)(q % C); b = (int)(q / C);
}

// the epilogue of a forward workgroup (256 threads, all of them call it): its sums of a and of b, one LDS word per wave and
// value, the four waves added by thread 0 in the order w0 + w1 + w2 + w3, stored in the workgroup's slot of the plane's partials
template <class T>
__device__ __forceinline__ void block_part2(float a, T b, float* __restrict__ part_a, T* __restrict__ part_b, int plane) {
  a = wave_sum(a);
  if constexpr (std::is_same<T, int>::value) b = wave_sum_i(b); else b = wave_sum(b);
  __shared__ float sw[4];
  __shared__ T sb[4];
  if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6] = a; sb[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part_a[(size_t)plane * gridDim.x + blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
    part_b[(size_t)plane * gridDim.x + blockIdx.x] = sb[0] + sb[1] + sb[2] + sb[3];
  }
}

// one wave: the sum of channel c's B * nblk partials (COUNT: and of their counts; a channel may hold more than 2^31 pixels)
template <bool COUNT>
__device__ __forceinline__ float channel_part_sum(const float* __restrict__ part, int nblk, int B, int C, int c,
                                                  const int* __restrict__ partn = nullptr, int64_t* count = nullptr) {
  float s = 0.f;
  int64_t n = 0;
  for (int e = threadIdx.x; e < B * nblk; e += 64) {
    const int b = e / nblk, k = e - b * nblk;
    s += part[(size_t)(b * C + c) * nblk + k];
    if (COUNT) n += partn[(size_t)(b * C + c) * nblk + k];
  }
  s = wave_sum(s);
  if (COUNT) *count = wave_sum_i64(n);
  return s;
}

// ---- losses ---------------------------------------------------------------------------------------
// err(b,c,i,j) = [(p-t)^2 + 0.02*(dv + dh + 0.7*d1 + 0.7*d2)] * latw[i] * chanw[c]     (kind 1; kind 0: no TV)
//   dv = |p[i+1][j]-p[i][j]| (i<H-1)        dh = |p[i][j+1]-p[i][j]| (j<W-1)
//   d1 = |p[i+1][j+1]-p[i][j]| (i<H-1,j<W-1)   d2 = |p[i+1][j-1]-p[i][j]| (i<H-1, j>=1)

__global__ __launch_bounds__(256) void loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       int Ht, int Wt, const float* __restrict__ latw,
                                                       const float* __restrict__ chanw, float* __restrict__ part,
                                                       float* __restrict__ part2, int C, int H, int W, int kind) {
  const int plane = blockIdx.y;  // b*C + c
  const int c = plane % C, b = plane / C;
  const float* p = pred + (size_t)plane * H * W;
  const float* t = tgt + ((size_t)b * C + c) * Ht * Wt;
  const float cw = chanw ? chanw[c] : 1.f;
  float s = 0.f, s2 = 0.f;
  O2_IMAGE_STRIDE(e, H * W) {
    const int i = e / W, j = e - i * W;
    const float pv = p[e];
    const float tv0 = t[(size_t)i * Wt + j];
    const float d = pv - tv0;
    float err = d * d;
    if (kind == 2) {   // image-gradient term (metrics/functional.py:59-114): forward differences, last row/col zero
      if (j < W - 1) s2 += fabsf((t[(size_t)i * Wt + j + 1] - tv0) - (p[e + 1] - pv));
      if (i < H - 1) s2 += fabsf((t[(size_t)(i + 1) * Wt + j] - tv0) - (p[e + W] - pv));
    }
    if (kind == 1) {
      float tv = 0.f;
      if (i < H - 1) {
        tv += fabsf(p[e + W] - pv);
        if (j < W - 1) tv += 0.7f * fabsf(p[e + W + 1] - pv);
        if (j >= 1) tv += 0.7f * fabsf(p[e + W - 1] - pv);
      }
      if (j < W - 1) tv += fabsf(p[e + 1] - pv);
      err += 0.02f * tv;
    }
    s += err * (latw ? latw[i] : 1.f) * cw;
  }
  block_part2(s, s2, part, part2, plane);
}

__global__ void loss_final_kernel(const float* __restrict__ part, const float* __restrict__ part2, int nblk, int B,
                                  int C, int HW, const float* __restrict__ chanw, int kind, float* __restrict__ out) {
  // one wave; out[c] = mean over (b, pixels) of channel c; out[C] = mean over everything
  float tot = 0.f;
  for (int c = 0; c < C; ++c) {
    const float s = channel_part_sum<false>(part, nblk, B, C, c);
    if (threadIdx.x == 0) out[c] = s / ((float)B * (float)HW);
    tot += s;
  }
  float agg = tot / ((float)B * (float)C * (float)HW);
  if (kind == 2) {   // + 0.1 * mean(|grad diff|) * mean(channel weights)
    float s2 = 0.f;
    for (int e = threadIdx.x; e < B * C * nblk; e += 64) s2 += part2[e];
    s2 = wave_sum(s2);
    float cwm = 1.f;
    if (chanw) { cwm = 0.f; for (int c = 0; c < C; ++c) cwm += chanw[c]; cwm /= (float)C; }
    agg += 0.1f * (s2 / ((float)B * (float)C * (float)HW)) * cwm;
  }
  if (threadIdx.x == 0) out[C] = agg;
}

__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       int Ht, int Wt, const float* __restrict__ latw,
                                                       const float* __restrict__ chanw,
                                                       const float* __restrict__ gscale, float* __restrict__ dpred,
                                                       int B, int C, int H, int W, int kind) {
  const int64_t n = (int64_t)B * C * H * W;
  const float g0 = gscale[0] / (float)n;
  O2_GRID_STRIDE(e, n) {
    int b, c, i, j;
    plane_of(e, C, H, W, b, c, i, j);
    const float* p = pred + ((size_t)b * C + c) * H * W;
    const int o = i * W + j;
    const float pv = p[o];
    const float wi = latw ? latw[i] : 1.f;
    const float wim = (latw && i > 0) ? latw[i - 1] : 1.f;
    float g = 2.f * (pv - tgt[(((size_t)b * C + c) * Ht + i) * Wt + j]) * wi;
    if (kind == 2) {
      const float* t = tgt + ((size_t)b * C + c) * Ht * Wt;
      const float tv0 = t[(size_t)i * Wt + j];
      float gs = 0.f;
      if (j < W - 1) gs += sgn((t[(size_t)i * Wt + j + 1] - tv0) - (p[o + 1] - pv));
      if (j > 0) gs -= sgn((tv0 - t[(size_t)i * Wt + j - 1]) - (pv - p[o - 1]));
      if (i < H - 1) gs += sgn((t[(size_t)(i + 1) * Wt + j] - tv0) - (p[o + W] - pv));
      if (i > 0) gs -= sgn((tv0 - t[(size_t)(i - 1) * Wt + j]) - (pv - p[o - W]));
      float cwm = 1.f;
      if (chanw) { cwm = 0.f; for (int cc = 0; cc < C; ++cc) cwm += chanw[cc]; cwm /= (float)C; }
      dpred[e] = (g * (chanw ? chanw[c] : 1.f) + 0.1f * cwm * gs) * g0;
      continue;
    }
    if (kind == 1) {
      float tv = 0.f;
      // terms stored at row i (weight wi) in which p[i][j] is the subtrahend
      if (i < H - 1) {
        tv -= sgn(p[o + W] - pv) * wi;
        if (j < W - 1) tv -= 0.7f * sgn(p[o + W + 1] - pv) * wi;
        if (j >= 1) tv -= 0.7f * sgn(p[o + W - 1] - pv) * wi;
      }
      if (j < W - 1) tv -= sgn(p[o + 1] - pv) * wi;
      // terms in which p[i][j] is the minuend
      if (j > 0) tv += sgn(pv - p[o - 1]) * wi;                              // dh stored at (i, j-1)
      if (i > 0) {
        tv += sgn(pv - p[o - W]) * wim;                                      // dv stored at (i-1, j)
        if (j > 0) tv += 0.7f * sgn(pv - p[o - W - 1]) * wim;                // d1 stored at (i-1, j-1)
        if (j < W - 1) tv += 0.7f * sgn(pv - p[o - W + 1]) * wim;            // d2 stored at (i-1, j+1)
      }
      g += 0.02f * tv;
    }
    dpred[e] = g * (chanw ? chanw[c] : 1.f) * g0;
  }
}

// ---- evaluation metrics (metrics/functional.py:219-324: mae, rmse, acc, pearson, mean_bias) ------------------------------
// the twelve sums of score_sums.h (o2_moments_add) per (b, c) image, clim optional [C][H][W]; one pixel per lane and trip.
// orbit2_masked_moments with no mask is NOT this kernel with a count: on rows that are not 16-byte aligned its four-pixel items
// of guarded scalar loads take 1.36 x the time of this sweep (profiles/score_sums.md), so both stay.
__global__ __launch_bounds__(256) void eval_moments_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           int Ht, int Wt, const float* __restrict__ lat_w,
                                                           const float* __restrict__ clim, double* __restrict__ out,
                                                           int C, int H, int W) {
  const int bc = blockIdx.y;
  const float* p = pred + (size_t)bc * H * W;
  const float* t = target + (size_t)bc * Ht * Wt;
  const float* cl = clim ? clim + (size_t)(bc % C) * H * W : nullptr;
  float s[O2_NMOMENTS];
#pragma unroll
  for (int k = 0; k < O2_NMOMENTS; ++k) s[k] = 0.f;
  O2_IMAGE_STRIDE(i, H * W) {
    const int y = i / W, x = i - y * W;
    const float c0 = cl ? cl[i] : 0.f;
    o2_moments_add(s, p[i] - c0, t[(size_t)y * Wt + x] - c0, lat_w ? lat_w[y] : 1.f);
  }
  o2_block_sums_add(s, out + (size_t)bc * O2_NMOMENTS);
}

constexpr int MM_NM = O2_NMOMENTS + 1;   // the twelve sums of orbit2_eval_moments + the valid count

// |a - b| if both pixels are valid, else 0 (select: a and b may be NaN where invalid)
__device__ __forceinline__ float absdiff_if(bool v, float a, float b) { return v ? fabsf(a - b) : 0.f; }
__device__ __forceinline__ float sgndiff_if(bool v, float a, float b) { return v ? sgn(a - b) : 0.f; }

// ---- forward: per-workgroup partials of num = sum v w cw err and of the valid count per (b, c) plane ----------------------
//   err(i,j) = (p - t)^2 + [TV] 0.02 (|p[i+1][j]-p| + |p[i][j+1]-p| + 0.7 |p[i+1][j+1]-p| + 0.7 |p[i+1][j-1]-p|), each
//   difference only if its neighbour is valid too
template <bool VEC, bool TV>
__global__ __launch_bounds__(256) void masked_loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                              int Ht, int Wt, MaskArg mk, const float* __restrict__ latw,
                                                              const float* __restrict__ chanw, float* __restrict__ part,
                                                              int* __restrict__ partn, int C, int H, int W) {
  const int plane = blockIdx.y, c = plane % C, b = plane / C;
  const float* p = pred + (size_t)plane * H * W;
  const float* t = tgt + (size_t)plane * Ht * Wt;
  const uint8_t* m = mk.m ? mk.m + b * mk.sb + c * mk.sc : nullptr;
  const int W4 = (W + 3) >> 2;
  float s = 0.f;
  int n = 0;
  O2_IMAGE_STRIDE(e, H * W4) {
    const int i = e / W4, j0 = (e - i * W4) << 2;
    float p0[6], p1[6], t0[4], t1[4];
    bool v0[6], v1[6];
    load_row<VEC, TV>(p, t, m, i, j0, H, W, Wt, mk.pitch, p0, v0, t0);
    if (TV) load_row<VEC, true>(p, t, m, i + 1, j0, H, W, Wt, mk.pitch, p1, v1, t1);
    float acc = 0.f;
#pragma unroll
    for (int k = 1; k <= 4; ++k) {
      const bool v = v0[k];
      const float d = v ? p0[k] - t0[k - 1] : 0.f;
      float err = d * d;
      if (TV) {
        const float tv = absdiff_if(v && v1[k], p1[k], p0[k]) + absdiff_if(v && v0[k + 1], p0[k + 1], p0[k]) +
                         0.7f * absdiff_if(v && v1[k + 1], p1[k + 1], p0[k]) +
                         0.7f * absdiff_if(v && v1[k - 1], p1[k - 1], p0[k]);
        err += 0.02f * tv;
      }
      acc += err;
      n += v ? 1 : 0;
    }
    s += acc * (latw ? latw[i] : 1.f);
  }
  block_part2(s * (chanw ? chanw[c] : 1.f), n, part, partn, plane);
}

// one wave: out[c] = num_c / n_c (0 if n_c == 0), out[C] = sum num / sum n (0 if nothing is valid); cnt[c] = n_c, cnt[C] = sum n
__global__ void masked_loss_final_kernel(const float* __restrict__ part, const int* __restrict__ partn, int nblk, int B, int C,
                                         float* __restrict__ out, int64_t* __restrict__ cnt) {
  float tot = 0.f;
  int64_t ntot = 0;
  for (int c = 0; c < C; ++c) {
    int64_t n;
    const float s = channel_part_sum<true>(part, nblk, B, C, c, partn, &n);
    if (threadIdx.x == 0) { out[c] = n ? s / (float)n : 0.f; cnt[c] = n; }
    tot += s;
    ntot += n;
  }
  if (threadIdx.x == 0) { out[C] = ntot ? tot / (float)ntot : 0.f; cnt[C] = ntot; }
}

// ---- backward: dpred = gscale[0] / cnt[C] * d(sum_c num_c)/dpred; exactly 0 at an invalid pixel and when nothing is valid --
template <bool VEC, bool TV>
__global__ __launch_bounds__(256) void masked_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                              int Ht, int Wt, MaskArg mk, const float* __restrict__ latw,
                                                              const float* __restrict__ chanw,
                                                              const float* __restrict__ gscale,
                                                              const int64_t* __restrict__ cnt, float* __restrict__ dpred,
                                                              int B, int C, int H, int W) {
  const int W4 = (W + 3) >> 2;
  const int64_t items = (int64_t)B * C * H * W4;
  const int64_t ntot = cnt[C];
  const float g0 = ntot ? gscale[0] / (float)ntot : 0.f;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;           // one item per thread: the grid covers them all
  if (e < items) {
    int b, c, i, j0;
    plane_of(e, C, H, W4, b, c, i, j0);
    j0 <<= 2;
    const size_t plane = (size_t)b * C + c;
    const float* p = pred + plane * H * W;
    const float* t = tgt + plane * Ht * Wt;
    const uint8_t* m = mk.m ? mk.m + b * mk.sb + c * mk.sc : nullptr;
    float p0[6], pa[6], pb[6], t0[4], tx[4];
    bool v0[6], va[6], vb[6];
    load_row<VEC, TV>(p, t, m, i, j0, H, W, Wt, mk.pitch, p0, v0, t0);
    if (TV) {
      load_row<VEC, true>(p, t, m, i - 1, j0, H, W, Wt, mk.pitch, pa, va, tx);      // the row above
      load_row<VEC, true>(p, t, m, i + 1, j0, H, W, Wt, mk.pitch, pb, vb, tx);      // the row below
    }
    const float wi = latw ? latw[i] : 1.f;
    const float wim = (TV && latw && i > 0) ? latw[i - 1] : 1.f;
    const float sc = (chanw ? chanw[c] : 1.f) * g0;
    float g[4];
#pragma unroll
    for (int k = 1; k <= 4; ++k) {
      const bool v = v0[k];
      const float x = p0[k];
      float gk = v ? 2.f * (x - t0[k - 1]) * wi : 0.f;
      if (TV) {
        // terms stored at (i, j) (weight wi), in which p[i][j] is the subtrahend
        float tv = -(sgndiff_if(v && vb[k], pb[k], x) + sgndiff_if(v && v0[k + 1], p0[k + 1], x) +
                     0.7f * sgndiff_if(v && vb[k + 1], pb[k + 1], x) + 0.7f * sgndiff_if(v && vb[k - 1], pb[k - 1], x)) * wi;
        // terms in which p[i][j] is the minuend: dh stored at (i, j-1); dv at (i-1, j), d1 at (i-1, j-1), d2 at (i-1, j+1)
        tv += sgndiff_if(v && v0[k - 1], x, p0[k - 1]) * wi;
        tv += (sgndiff_if(v && va[k], x, pa[k]) + 0.7f * sgndiff_if(v && va[k - 1], x, pa[k - 1]) +
               0.7f * sgndiff_if(v && va[k + 1], x, pa[k + 1])) * wim;
        gk += 0.02f * tv;
      }
      g[k - 1] = v ? gk * sc : 0.f;
    }
    float* dp = dpred + plane * H * W + (size_t)i * W + j0;
    if (VEC) {
      f32x4 o = {g[0], g[1], g[2], g[3]};
      *reinterpret_cast<f32x4*>(dp) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < W) dp[k] = g[k];
    }
  }
}

// ---- the twelve sums of orbit2_eval_moments (score_sums.h: o2_moments_add) over the valid pixels, and their number, which must
// stay exact: an integer beside the epilogue's floats, not a thirteenth of them ------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void masked_moments_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                             int Ht, int Wt, MaskArg mk, const float* __restrict__ latw,
                                                             const float* __restrict__ clim, double* __restrict__ out,
                                                             int C, int H, int W) {
  __shared__ int redn[4];
  const int plane = blockIdx.y, c = plane % C, b = plane / C;
  const float* p = pred + (size_t)plane * H * W;
  const float* t = tgt + (size_t)plane * Ht * Wt;
  const uint8_t* m = mk.m ? mk.m + b * mk.sb + c * mk.sc : nullptr;
  const float* cl = clim ? clim + (size_t)c * H * W : nullptr;
  const int W4 = (W + 3) >> 2;
  float s[O2_NMOMENTS];
#pragma unroll
  for (int k = 0; k < O2_NMOMENTS; ++k) s[k] = 0.f;
  int n = 0;
  O2_IMAGE_STRIDE(e, H * W4) {
    const int i = e / W4, j0 = (e - i * W4) << 2;
    float p0[6], t0[4], c0[4] = {0.f, 0.f, 0.f, 0.f};
    bool v0[6];
    load_row<VEC, false>(p, t, m, i, j0, H, W, Wt, mk.pitch, p0, v0, t0);
    if (cl) {
      if (VEC) {
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(cl + (size_t)i * W + j0);
#pragma unroll
        for (int k = 0; k < 4; ++k) c0[k] = c4[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (j0 + k < W) c0[k] = cl[(size_t)i * W + j0 + k];
      }
    }
    const float w = latw ? latw[i] : 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool v = v0[k + 1];
      const float a = v ? p0[k + 1] - c0[k] : 0.f, bb = v ? t0[k] - c0[k] : 0.f;      // zeros add nothing to any sum
      o2_moments_add(s, a, bb, w);
      n += v ? 1 : 0;
    }
  }
  n = wave_sum_i(n);
  if ((threadIdx.x & 63) == 0) redn[threadIdx.x >> 6] = n;
  o2_block_sums_add(s, out + (size_t)plane * MM_NM);                 // its barrier orders redn as well
  if (threadIdx.x == MM_NM - 1)
    atomicAdd(out + (size_t)plane * MM_NM + MM_NM - 1, (double)(redn[0] + redn[1] + redn[2] + redn[3]));   // exact below 2^53
}

}  // namespace

extern "C" int orbit2_loss_fwd(const float* pred, const float* target, int Ht, int Wt, const float* lat_w,
                               const float* chan_w, float* out, float* ws, int B, int C, int H, int W, int kind,
                               void* stream) {
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !out || !ws) return O2_ERR_ARG;
  if (kind < 0 || kind > 2) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* ws2 = ws + (size_t)B * C * ORBIT2_LOSS_BLOCKS;
  hipLaunchKernelGGL(loss_fwd_kernel, dim3(ORBIT2_LOSS_BLOCKS, B * C), dim3(256), 0, s, pred, target, Ht, Wt, lat_w, chan_w, ws,
                     ws2, C, H, W, kind);
  O2_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, s, ws, ws2, ORBIT2_LOSS_BLOCKS, B, C, H * W, chan_w, kind, out);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_loss_bwd(const float* pred, const float* target, int Ht, int Wt, const float* lat_w,
                               const float* chan_w, const float* gscale, float* dpred, int B, int C, int H, int W,
                               int kind, void* stream) {
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !gscale || !dpred) return O2_ERR_ARG;
  if (kind == ORBIT2_LOSS_SSIM_VJP)
    return chan_w ? O2_ERR_ARG : o2_ssim_vjp(pred, target, Ht, Wt, lat_w, gscale, dpred, B, C, H, W, (hipStream_t)stream);
  if (kind < 0 || kind > 2) return O2_ERR_ARG;
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(grid_for((int64_t)B * C * H * W, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                     pred, target, Ht, Wt, lat_w, chan_w, gscale, dpred, B, C, H, W, kind);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_eval_moments(const float* pred, const float* target, int Ht, int Wt, const float* lat_w,
                                   const float* clim, double* out, int B, int C, int H, int W, void* stream) {
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !out) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)B * C * O2_NMOMENTS, s) != hipSuccess) return O2_ERR_LAUNCH;
  hipLaunchKernelGGL(eval_moments_kernel, dim3(o2_image_blocks((int64_t)H * W), B * C), dim3(256), 0, s, pred, target, Ht, Wt,
                     lat_w, clim, out, C, H, W);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_masked_loss_fwd(const float* pred, const float* target, int Ht, int Wt, const uint8_t* mask,
                                      int mask_pitch, int64_t mask_sb, int64_t mask_sc, const float* lat_w,
                                      const float* chan_w, float* out, int64_t* cnt, float* ws, int B, int C, int H, int W,
                                      int kind, void* stream) {
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !out || !cnt || !ws) return O2_ERR_ARG;
  // the kind word: bits 0-3 the kind proper, bits 4-5 the flags, bits 8-15 a count; kinds 0 / 1 take neither flag nor count;
  // ORBIT2_FSS_KIND alone takes bits 16-23, its window
  constexpr int FLAGS = ORBIT2_MASKED_PER_IMAGE | ORBIT2_MASKED_LOWER;
  const int base = kind & 15;
  if (kind < 0 || (kind & ~(15 | FLAGS | 0xff00 | (base == ORBIT2_FSS_KIND ? 0xff0000 : 0)))) return O2_ERR_ARG;
  if (base != ORBIT2_MASKED_QUANTILES && base != ORBIT2_MASKED_TAIL && base != ORBIT2_FSS_KIND && kind != 0 && kind != 1)
    return O2_ERR_ARG;
  MaskArg mk;
  if (!mask_arg(mk, mask, mask_pitch, mask_sb, mask_sc, Ht, Wt, W)) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (base == ORBIT2_FSS_KIND)
    return o2_masked_fss(pred, target, Ht, Wt, mk, lat_w, chan_w, out, cnt, ws, B, C, H, W, kind & FLAGS, (kind >> 8) & 0xff,
                         (kind >> 16) & 0xff, s);
  if (base >= ORBIT2_MASKED_QUANTILES)
    return o2_masked_extremes(pred, target, Ht, Wt, mk, lat_w, chan_w, out, cnt, ws, B, C, H, W, base, kind & FLAGS,
                              (kind >> 8) & 0xff, s);
  int* wsn = reinterpret_cast<int*>(ws + (size_t)B * C * ORBIT2_LOSS_BLOCKS);
  o2_with_flags(
      [&](auto vec, auto tv) {
        hipLaunchKernelGGL((masked_loss_fwd_kernel<decltype(vec)::value, decltype(tv)::value>), dim3(ORBIT2_LOSS_BLOCKS, B * C),
                           dim3(256), 0, s, pred, target, Ht, Wt, mk, lat_w, chan_w, ws, wsn, C, H, W);
      },
      vec_ok(pred, target, mk, W, Wt), kind == 1);
  O2_CHECK_LAUNCH();
  hipLaunchKernelGGL(masked_loss_final_kernel, dim3(1), dim3(64), 0, s, ws, wsn, ORBIT2_LOSS_BLOCKS, B, C, out, cnt);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_masked_loss_bwd(const float* pred, const float* target, int Ht, int Wt, const uint8_t* mask,
                                      int mask_pitch, int64_t mask_sb, int64_t mask_sc, const float* lat_w,
                                      const float* chan_w, const float* gscale, const int64_t* cnt, float* dpred, int B,
                                      int C, int H, int W, int kind, void* stream) {
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !gscale || !cnt || !dpred) return O2_ERR_ARG;
  if (kind != 0 && kind != 1) return O2_ERR_ARG;
  MaskArg mk;
  if (!mask_arg(mk, mask, mask_pitch, mask_sb, mask_sc, Ht, Wt, W)) return O2_ERR_ARG;
  const int64_t items = (int64_t)B * C * H * ((W + 3) / 4);
  const int64_t nblk = (items + 255) / 256;
  if (nblk > 0x7fffffff) return O2_ERR_ARG;
  o2_with_flags(
      [&](auto vec, auto tv) {
        hipLaunchKernelGGL((masked_loss_bwd_kernel<decltype(vec)::value, decltype(tv)::value>), dim3((unsigned)nblk), dim3(256),
                           0, (hipStream_t)stream, pred, target, Ht, Wt, mk, lat_w, chan_w, gscale, cnt, dpred, B, C, H, W);
      },
      vec_ok(pred, target, mk, W, Wt) && aligned(dpred, 16), kind == 1);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_masked_moments(const float* pred, const float* target, int Ht, int Wt, const uint8_t* mask,
                                     int mask_pitch, int64_t mask_sb, int64_t mask_sc, const float* lat_w, const float* clim,
                                     double* out, int B, int C, int H, int W, void* stream) {
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !out) return O2_ERR_ARG;
  MaskArg mk;
  if (!mask_arg(mk, mask, mask_pitch, mask_sb, mask_sc, Ht, Wt, W)) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)B * C * MM_NM, s) != hipSuccess) return O2_ERR_LAUNCH;
  const int nblk = o2_image_blocks((int64_t)H * ((W + 3) / 4) * 4);   // an item is four pixels
  o2_with_flags(
      [&](auto vec) {
        hipLaunchKernelGGL((masked_moments_kernel<decltype(vec)::value>), dim3(nblk, B * C), dim3(256), 0, s, pred, target, Ht,
                           Wt, mk, lat_w, clim, out, C, H, W);
      },
      vec_ok(pred, target, mk, W, Wt) && (!clim || aligned(clim, 16)));
  O2_CHECK_LAUNCH();
  return O2_OK;
}
