// Ensembles: the all-member scores, then the streamed MC-dropout statistics and the scores of their Gaussian.
// All-member (non-Gaussian) scores of an ensemble: CRPS, rank histogram, quantile fields (include/orbit2_hip.h:
// orbit2_ensemble_scores; metrics/functional.py ensemble_*).
//
// One pixel per lane, consecutive lanes on consecutive pixels: every member load is one coalesced wave access, the N values of
// a pixel live in registers and are read exactly once.  blockIdx.y = the (b, c) image, grid-stride over its pixels.  The raw
// values are sorted by a bitonic network on the padded size P (a template parameter: every index is a compile-time constant,
// so the array never goes to scratch; pads are +inf and end up behind the N members).  Rounding is monotone, so the sorted raw
// values centred on the target, d_(k) = x_(k) - y, are sorted too: the quantiles come from the raw values (q = 0 and q = 1 are
// the minimum and the maximum bit for bit), every sum from the centred ones -- a field in kelvin is 280 +- 1, and the pair term
// sum_k (2k - N - 1) x_(k) on raw values loses its low bits to cancellation.
#include "score_sums.h"
#include "../../include/orbit2_hip.h"

namespace {
constexpr int ES_NM = 4;
constexpr int ES_MAX_Q = 16;

template <int P>
__device__ __forceinline__ void bitonic_sort(float (&v)[P]) {
#pragma unroll
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
          const bool up = (i & k) == 0;
          v[i] = up ? lo : hi;
          v[l] = up ? hi : lo;
        }
      }
    }
  }
}

// P / 2 < N <= P (P = 2: N = 2).  Outputs that are NULL are not computed (wave-uniform branches).
template <int P>
__global__ __launch_bounds__(256) void ensemble_scores_kernel(const float* __restrict__ members, int64_t member_stride, int N,
                                                              const float* __restrict__ target, int Ht, int Wt,
                                                              const float* __restrict__ lat_w, double* __restrict__ sums,
                                                              float* __restrict__ crps_field, int fair,
                                                              unsigned long long* __restrict__ hist, uint64_t seed,
                                                              float* __restrict__ quant, const float* __restrict__ levels, int Q,
                                                              int64_t field, int H, int W) {
  __shared__ unsigned int bins[ORBIT2_ENSEMBLE_MAX_MEMBERS + 1];
  __shared__ int q_lo[ES_MAX_Q];
  __shared__ float q_fr[ES_MAX_Q];
  const int bc = blockIdx.y;
  const int HW = H * W;
  const float* m = members + (size_t)bc * HW;
  const float* t = target + (size_t)bc * Ht * Wt;
  if (hist)
    for (int k = threadIdx.x; k <= N; k += 256) bins[k] = 0u;
  // the quantile levels as (lower order statistic, weight of the upper one), once per workgroup: double, so that the position
  // q (N - 1) is the one numpy / torch compute
  if (quant && threadIdx.x < Q) {
    double pos = (double)levels[threadIdx.x] * (double)(N - 1);
    pos = !(pos > 0.0) ? 0.0 : (pos > (double)(N - 1) ? (double)(N - 1) : pos);   // (a NaN level: 0)
    const int lo = (int)pos;
    q_lo[threadIdx.x] = lo;
    q_fr[threadIdx.x] = (float)(pos - (double)lo);
  }
  __syncthreads();
  const float fN = (float)N, inv_n = 1.f / fN;
  const float inv_pairs = fair ? 1.f / (fN * (fN - 1.f)) : 1.f / (fN * fN);
  float s[ES_NM] = {0.f, 0.f, 0.f, 0.f};
  O2_IMAGE_STRIDE(i, HW) {
    const int y = i / W, x = i - y * W;
    float v[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      v[k] = __builtin_inff();
      if (k < P / 2 || k < N) v[k] = m[(size_t)k * member_stride + i];
    }
    const float tv = t[(size_t)y * Wt + x];
    if (hist) {
      unsigned lt = 0, eq = 0;
#pragma unroll
      for (int k = 0; k < P; ++k) {                     // pads are +inf: neither below nor equal to a finite target
        lt += v[k] < tv ? 1u : 0u;
        eq += v[k] == tv ? 1u : 0u;
      }
      const uint32_t h = o2_hash64(seed, (uint64_t)bc * (uint64_t)HW + (uint64_t)i);      // NOT salted: a score is a pure function
      unsigned rank = lt + (unsigned)(((uint64_t)h * (uint64_t)(eq + 1u)) >> 32);
      rank = rank > (unsigned)N ? (unsigned)N : rank;   // (non-finite members: stay inside the bins)
      atomicAdd(&bins[rank], 1u);
    }
    if (!sums && !crps_field && !quant) continue;
    bitonic_sort<P>(v);
    if (quant) {
      for (int j = 0; j < Q; ++j) {
        const int lo = __builtin_amdgcn_readfirstlane(q_lo[j]), hi = lo + 1 < N ? lo + 1 : lo;        // wave-uniform
        float a = v[0], b = v[0];
#pragma unroll
        for (int k = 1; k < P; ++k) {                   // selects on a uniform condition, no runtime-indexed array
          a = k == lo ? v[k] : a;
          b = k == hi ? v[k] : b;
        }
        const float fr = q_fr[j];
        quant[(size_t)j * field + (size_t)bc * HW + i] = fr == 0.f ? a : fmaf(fr, b - a, a);
      }
    }
    if (sums || crps_field) {
      float sa = 0.f, sd = 0.f, pair = 0.f;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        if (k < P / 2 || k < N) {
          const float d = v[k] - tv;
          v[k] = d;
          sa += fabsf(d);
          sd += d;
          pair = fmaf((float)(2 * k + 1 - N), d, pair);                    // (2k - N - 1) d_(k), k 1-based
        }
      }
      const float mabs = sa * inv_n;
      if (crps_field) crps_field[(size_t)bc * HW + i] = mabs - pair * inv_pairs;
      if (sums) {
        const float md = sd * inv_n;
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < P; ++k) {
          if (k < P / 2 || k < N) {
            const float e = v[k] - md;
            ss = fmaf(e, e, ss);
          }
        }
        const float w = lat_w ? lat_w[y] : 1.f;
        s[0] += w * mabs;
        s[1] += w * pair;
        s[2] += w * md * md;
        s[3] += w * ss / (fN - 1.f);
      }
    }
  }
  if (sums) o2_block_sums_add(s, sums + (size_t)bc * ES_NM);          // grid-uniform; holds the workgroup's barrier
  else __syncthreads();                                                 // bins[] is complete
  if (hist) {
    for (int k = threadIdx.x; k <= N; k += 256) {
      const unsigned int c = bins[k];
      if (c) atomicAdd(hist + (size_t)bc * (N + 1) + k, (unsigned long long)c);
    }
  }
}

// ---- MC-dropout ensembles (utils/mc_dropout.py; metrics/functional.py:340-386 gaussian_crps / _spread / _spread_skill_ratio) ----
// The k-th (1-based) Welford step of the running per-element mean and sum of squared deviations, in place:
//   d = x - mean;  mean += d / k;  m2 += d * (x - mean)          (k = 1: mean = x, m2 = 0 -- neither is read)
// so N members of a [B, C, H, W] field leave mean and m2 = (N - 1) * unbiased variance without N fields being held.  A pure
// stream (12 bytes read, 8 written per element): float4 per lane when the three bases are 16-byte aligned, grid-stride over at
// most 2048 workgroups, the n % 4 tail (or everything, for unaligned bases) by scalar lanes.
__device__ __forceinline__ void welford_step(float x, float& mean, float& m2, float kf) {
  const float d = x - mean;
  mean += d / kf;
  m2 = fmaf(d, x - mean, m2);
}

__global__ __launch_bounds__(256) void ensemble_update_kernel(const float* __restrict__ member, float* __restrict__ mean,
                                                              float* __restrict__ m2, int64_t n, int64_t n4, int k) {
  const float kf = (float)k;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(member);
  f32x4* mean4 = reinterpret_cast<f32x4*>(mean);
  f32x4* m24 = reinterpret_cast<f32x4*>(m2);
  if (k == 1) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = tid; i < n4; i += nthr) {
      mean4[i] = x4[i];
      m24[i] = zero;
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += nthr) {
      mean[i] = member[i];
      m2[i] = 0.f;
    }
    return;
  }
  for (int64_t i = tid; i < n4; i += nthr) {
    const f32x4 x = x4[i];
    f32x4 mu = mean4[i], s = m24[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = mu[j], sj = s[j];
      welford_step(x[j], mj, sj, kf);
      mu[j] = mj;
      s[j] = sj;
    }
    mean4[i] = mu;
    m24[i] = s;
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += nthr) {
    float mu = mean[i], s = m2[i];
    welford_step(member[i], mu, s, kf);
    mean[i] = mu;
    m2[i] = s;
  }
}

// Scores of a Gaussian prediction N(mean, std^2) against a target, four sums per (b, c) image (target: top-left crop,
// w = lat_w[y] or 1), added up by o2_block_sums_add as in orbit2_eval_moments:
//   0 sum w crps, 1 sum w std^2, 2 sum w (mean - target)^2, 3 sum 1{|target - mean| <= std}
// crps is the closed form of the Gaussian CRPS, std (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)) with z = (target - mean) / std
// (functional.py:353 there has 1 / pi, and cannot be called: see metrics/functional.py:gaussian_crps here).  It is evaluated as
//   |d| erf(|z| / sqrt 2) + std (2 phi(z) - 1 / sqrt(pi)),  d = target - mean,
// the same expression with std z = d multiplied out: no product of a huge z with a tiny std, and at std == 0 (constant output
// channels are copied from the target into every member) it IS the limit |d| -- no NaN, no Inf, and such a point counts as
// covered only where target == mean.
constexpr int GS_NM = 4;
__global__ __launch_bounds__(256) void gaussian_scores_kernel(const float* __restrict__ mean, const float* __restrict__ std_,
                                                              const float* __restrict__ target, int Ht, int Wt,
                                                              const float* __restrict__ lat_w, double* __restrict__ out, int H,
                                                              int W) {
  const int bc = blockIdx.y;
  const float* m = mean + (size_t)bc * H * W;
  const float* sd = std_ + (size_t)bc * H * W;
  const float* t = target + (size_t)bc * Ht * Wt;
  float s[GS_NM] = {0.f, 0.f, 0.f, 0.f};
  O2_IMAGE_STRIDE(i, H * W) {
    const int y = i / W, x = i - y * W;
    const float sg = sd[i];
    const float d = t[(size_t)y * Wt + x] - m[i];
    const float w = lat_w ? lat_w[y] : 1.f;
    const float ad = fabsf(d);
    float crps = ad;
    if (sg > 0.f) {
      const float z = ad / sg;                         // may be +inf (a denormal std): erf -> 1, phi -> 0, crps -> |d| - std / sqrt(pi)
      const float phi = 0.3989422804014327f * expf(-0.5f * z * z);
      crps = ad * erff(z * 0.70710678118654752f) + sg * (2.f * phi - 0.5641895835477563f);
    }
    s[0] += w * crps;
    s[1] += w * sg * sg;
    s[2] += w * d * d;
    s[3] += ad <= sg ? 1.f : 0.f;
  }
  o2_block_sums_add(s, out + (size_t)bc * GS_NM);
}
}  // namespace

extern "C" int orbit2_ensemble_scores(const float* members, int64_t member_stride, int N, const float* target, int Ht, int Wt,
                                      const float* lat_w, double* sums, float* crps_field, int fair, int64_t* hist,
                                      uint64_t seed, float* quant, const float* levels, int Q, int B, int C, int H, int W,
                                      void* stream) {
  if (!sums && !crps_field && !hist && !quant) return O2_ERR_ARG;
  if (N < 2 || N > ORBIT2_ENSEMBLE_MAX_MEMBERS || !o2_pair_ok(members, target, B, C, H, W, Ht, Wt)) return O2_ERR_ARG;
  if ((int64_t)B * C > 65535 || (int64_t)H * W > (int64_t)INT32_MAX - 1024 * 256) return O2_ERR_ARG;
  const int64_t field = (int64_t)B * C * H * W;
  if (member_stride < field) return O2_ERR_ARG;
  if (quant && (!levels || Q < 1 || Q > ES_MAX_Q)) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (sums && hipMemsetAsync(sums, 0, sizeof(double) * (size_t)B * C * ES_NM, s) != hipSuccess) return O2_ERR_LAUNCH;
  if (hist && hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)B * C * (N + 1), s) != hipSuccess) return O2_ERR_LAUNCH;
  const int cap = o2_image_block_cap(B * C), nblk = (H * W + 255) / 256;       // one pixel per lane and trip
  const dim3 grid(nblk < cap ? nblk : cap, B * C);
  auto launch = [&](auto p) {                                                  // p = the padded size
    hipLaunchKernelGGL(ensemble_scores_kernel<decltype(p)::value>, grid, dim3(256), 0, s, members, member_stride, N, target, Ht, Wt,
                       lat_w, sums, crps_field, fair, reinterpret_cast<unsigned long long*>(hist), seed, quant, levels, Q, field, H, W);
  };
  if (N <= 2) launch(o2_int<2>{});
  else if (N <= 4) launch(o2_int<4>{});
  else if (N <= 8) launch(o2_int<8>{});
  else if (N <= 16) launch(o2_int<16>{});
  else if (N <= 32) launch(o2_int<32>{});
  else launch(o2_int<64>{});
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_ensemble_update(const float* member, float* mean, float* m2, int64_t n, int k, void* stream) {
  if (!member || !mean || !m2 || n <= 0 || k < 1 || member == mean || member == m2 || mean == m2) return O2_ERR_ARG;
  const bool aligned = (((uintptr_t)member | (uintptr_t)mean | (uintptr_t)m2) & 15) == 0;
  const int64_t n4 = aligned ? n / 4 : 0;
  const int64_t lanes = n4 > 0 ? n4 : n;
  int64_t nblk = (lanes + 255) / 256;
  if (nblk > 2048) nblk = 2048;
  hipLaunchKernelGGL(ensemble_update_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, member, mean, m2, n, n4,
                     k);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_gaussian_scores(const float* mean, const float* std_, const float* target, int Ht, int Wt,
                                      const float* lat_w, double* out, int B, int C, int H, int W, void* stream) {
  if (!o2_pair_ok(mean, target, B, C, H, W, Ht, Wt) || !std_ || !out) return O2_ERR_ARG;
  if ((int64_t)B * C > 65535 || (int64_t)H * W > (int64_t)INT32_MAX - 64 * 256) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(double) * (size_t)B * C * GS_NM, s) != hipSuccess) return O2_ERR_LAUNCH;
  hipLaunchKernelGGL(gaussian_scores_kernel, dim3(o2_image_blocks((int64_t)H * W), B * C), dim3(256), 0, s, mean, std_, target, Ht,
                     Wt, lat_w, out, H, W);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
