// What the evaluation kernels share (loss.hip, ensemble.hip, ssim.hip, resample.hip): the twelve evaluation moments,
// the per-image block-sum epilogue, the grid rules and the operand check of a scored pair.  common.h keeps what GEMM and attention
// need as well.
#pragma once
#include "common.h"

// true unless x is NaN or +-Inf
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float sgn(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }

// ---- the twelve evaluation moments (metrics/functional.py: mae, rmse, acc, pearson, mean_bias index them as m[..., k]) ---------
// One pixel's summands, a = pred - clim, b = target - clim (clim optional), w = lat_w[y] or 1:
//   0 sum a, 1 sum b, 2 sum a^2, 3 sum b^2, 4 sum a*b, 5 sum w (a-b)^2, 6 sum w |a-b|,
//   7 sum w a, 8 sum w b, 9 sum w a*b, 10 sum w a^2, 11 sum w b^2
// The order is a contract with metrics/functional.py and with tests/resample_ref.py (_terms), tests/masked_ref.py.
constexpr int O2_NMOMENTS = 12;
__device__ __forceinline__ void o2_moments_add(float (&s)[O2_NMOMENTS], float a, float b, float w) {
  const float d = a - b;
  s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
  s[5] += w * d * d; s[6] += w * fabsf(d);
  s[7] += w * a; s[8] += w * b; s[9] += w * a * b; s[10] += w * a * a; s[11] += w * b * b;
}

// ---- the block-sum epilogue of a 256-thread workgroup: dst[k] += the workgroup's sum of s[k] ----------------------------------
// per-thread fp32 partials -> wave_sum -> one LDS word per wave -> lane k adds the four waves in double -> one double atomicAdd:
// fp32 only inside a wave's share of an image, double across waves, workgroups and launches.  Every thread of the workgroup
// calls it (it holds a barrier); dst is the image's K sums, zeroed before the launch.
template <int K>
__device__ __forceinline__ void o2_block_sums_add(const float (&s)[K], double* dst) {
  __shared__ float red[4][K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float v = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    atomicAdd(dst + k, (double)red[0][k] + (double)red[1][k] + (double)red[2][k] + (double)red[3][k]);
  }
}

// ---- grid rules -----------------------------------------------------------------------------------------------------------------
// workgroups per image of a grid-stride sweep: 8 pixels per thread, and at most 64 -- with B * C images in blockIdx.y that fills
// the card, and every further workgroup is one more round of double atomics per image
inline int o2_image_blocks(int64_t pixels) {
  const int64_t n = (pixels + 256 * 8 - 1) / (256 * 8);
  return n > 64 ? 64 : (int)n;
}
// the loop header of such a sweep inside one image (blockIdx.y): 32-bit, the entries keep pixels + gridDim.x * 256 below 2^31
#define O2_IMAGE_STRIDE(i, n) for (int i = blockIdx.x * 256 + threadIdx.x; i < (n); i += gridDim.x * 256)
// the cap where a thread takes one pixel (or row) per trip: at most 64 workgroups per image, more only where B * C images alone
// would not fill the card
inline int o2_image_block_cap(int BC) { return BC >= 16 ? 64 : 1024 / BC; }

// ---- what every entry that scores pred [B,C,H,W] against target [B,C,Ht,Wt] (top-left crop) requires of the pair ---------------
inline bool o2_pair_ok(const void* pred, const void* target, int B, int C, int H, int W, int Ht, int Wt) {
  return pred && target && B > 0 && C > 0 && H > 0 && W > 0 && Ht >= H && Wt >= W;
}

// ---- the SSIM vector-Jacobian product (ssim.hip), reached through orbit2_loss_bwd (loss.hip) at kind ORBIT2_LOSS_SSIM_VJP: not
// an export, so the library's dynamic symbols stay those of the header
__attribute__((visibility("hidden"))) int o2_ssim_vjp(const float* pred, const float* target, int Ht, int Wt, const float* lat_w,
                                                      const float* gscale, float* dpred, int B, int C, int H, int W,
                                                      hipStream_t s);
