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
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
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

template <int P>
void launch(dim3 grid, hipStream_t s, const float* members, int64_t member_stride, int N, const float* target, int Ht, int Wt,
            const float* lat_w, double* sums, float* crps_field, int fair, int64_t* hist, uint64_t seed, float* quant,
            const float* levels, int Q, int64_t field, int H, int W) {
  hipLaunchKernelGGL(ensemble_scores_kernel<P>, grid, dim3(256), 0, s, members, member_stride, N, target, Ht, Wt, lat_w, sums,
                     crps_field, fair, reinterpret_cast<unsigned long long*>(hist), seed, quant, levels, Q, field, H, W);
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
#define ES_LAUNCH(P) \
  launch<P>(grid, s, members, member_stride, N, target, Ht, Wt, lat_w, sums, crps_field, fair, hist, seed, quant, levels, Q, field, H, W)
  if (N <= 2) ES_LAUNCH(2);
  else if (N <= 4) ES_LAUNCH(4);
  else if (N <= 8) ES_LAUNCH(8);
  else if (N <= 16) ES_LAUNCH(16);
  else if (N <= 32) ES_LAUNCH(32);
  else ES_LAUNCH(64);
#undef ES_LAUNCH
  O2_CHECK_LAUNCH();
  return O2_OK;
}
