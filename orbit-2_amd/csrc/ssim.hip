// Structural similarity and the squared-error sum of [B,C,H,W] fields on the device (include/orbit2_hip.h: orbit2_ssim;
// metrics/functional.py ssim / psnr).
//
// A workgroup owns a tile of SS_TH x SS_TW window centres (the "valid" centres, whose 7 x 7 window lies inside the image) and
// stages the (SS_TH + 6) x (SS_TW + 6) pixels under them, of both fields, in LDS once: one linear sweep, consecutive lanes on
// consecutive pixels of a row (coalesced along W), stored at the sweep's own pitch SS_IW, so every LDS write and every LDS read
// of the kernel has consecutive lanes on consecutive dwords -- no bank conflict at any pitch.  Wave w then owns centre rows
// 8 w .. 8 w + 7 of the tile, one column per lane: for each of the 8 + 6 pixel rows under them it forms the five 7-tap row sums
// (a, b, a^2, b^2, a b) from LDS and keeps the last seven in registers (every index is a compile-time constant: no scratch); a
// centre's window sums are the seven row sums added oldest first.  Each pixel is read from memory once per tile that covers it
// (1.3 x at 32 x 64); a quantity costs 7 adds in the row pass, for 14 rows per 8 centres, and 6 in the column pass.
//
// CENTRING IS PART OF THE CONTRACT.  Both fields are stored in LDS minus one shared pivot, the target's value at the tile's
// first pixel, and every lane subtracts a second shared pivot from what it reads: the stored target under the middle of the
// 14 x 7 pixels its eight windows cover.  The variances and the covariance come from the centred sums, and the means get the
// two pivots added back for the luminance term only.  A field in kelvin is 280 +- 3: sum x^2 / 49 - mean^2 on raw fp32 values
// loses the variance to cancellation (per-pixel error 4.8e-1 at offset 280 raw, 2e-6 centred; the tile's pivot alone leaves
// 1e-4 on a field that spans its range inside a tile: DESIGN 4.10b).
//
// The data range (max - min of the image's target crop, unless given) is found by a launch of its own in front and handed over
// in sums[3..4]: stream order, no host synchronisation.  A range of 0 is NOT special-cased: C1 = C2 = 0 and a flat window is
// 0 / 0 = NaN, as in scikit-image; no address depends on a value, so non-finite inputs give unspecified scores, never a fault.
#include "score_sums.h"
#include "../../include/orbit2_hip.h"

namespace {
constexpr int SS_WIN = ORBIT2_SSIM_WIN, SS_HALO = SS_WIN - 1;
constexpr int SS_TH = ORBIT2_SSIM_TILE_H, SS_TW = ORBIT2_SSIM_TILE_W;
constexpr int SS_IH = SS_TH + SS_HALO, SS_IW = SS_TW + SS_HALO;      // the staged pixels of a tile: 38 x 70
constexpr int SS_STRIP = SS_TH / 4;                                  // centre rows per wave
constexpr int SS_NS = 6;
static_assert(SS_WIN == 7 && SS_TW == 64 && SS_TH % 4 == 0, "one column per lane, four waves, a 7-deep register ring");

// sums[bc] = {0, 0, 0, +inf, -inf, 0}: the zeroing of the entry, with the neutral elements of min and max
__global__ void ssim_init_kernel(double* __restrict__ sums, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double* s = sums + (size_t)i * SS_NS;
  s[0] = s[1] = s[2] = s[5] = 0.0;
  s[3] = (double)__builtin_inff();
  s[4] = -(double)__builtin_inff();
}

// min and max of the target crop of image blockIdx.y: rows strided over the workgroups, lanes along W
__global__ __launch_bounds__(256) void ssim_range_kernel(const float* __restrict__ target, int Ht, int Wt,
                                                         double* __restrict__ sums, int H, int W) {
  __shared__ float red[4][2];
  const int bc = blockIdx.y;
  const float* t = target + (size_t)bc * Ht * Wt;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int y = blockIdx.x; y < H; y += gridDim.x) {
    const float* row = t + (size_t)y * Wt;
    for (int x = threadIdx.x; x < W; x += 256) {
      const float v = row[x];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = lo;
    red[threadIdx.x >> 6][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMin(sums + (size_t)bc * SS_NS + 3, (double)fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0])));
  if (threadIdx.x == 1)
    atomicMax(sums + (size_t)bc * SS_NS + 4, (double)fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1])));
}

__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ pred, const float* __restrict__ target, int Ht,
                                                   int Wt, const float* __restrict__ lat_w,
                                                   const float* __restrict__ data_range, double* sums,
                                                   float* __restrict__ ssim_map, int H, int W, int ntx) {
  __shared__ float sa[SS_IH * SS_IW], sb[SS_IH * SS_IW];
  const int bc = blockIdx.y;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int y0 = ty * SS_TH, x0 = tx * SS_TW;         // first centre of the tile in valid coordinates = its first pixel
  const int Hv = H - SS_HALO, Wv = W - SS_HALO;
  const float* p = pred + (size_t)bc * H * W;
  const float* t = target + (size_t)bc * Ht * Wt;
  double* S = sums + (size_t)bc * SS_NS;
  const float pivot = t[(size_t)y0 * Wt + x0];
  // the squared error is summed over ALL pixels: a tile owns the pixels under its own centres' first taps, the last tile of a
  // row / column of tiles the six behind them as well
  const int own_h = y0 + SS_TH >= Hv ? SS_IH : SS_TH, own_w = x0 + SS_TW >= Wv ? SS_IW : SS_TW;
  float se = 0.f;
  for (int i = threadIdx.x; i < SS_IH * SS_IW; i += 256) {
    const int r = i / SS_IW, c = i - r * SS_IW;
    const int y = y0 + r, x = x0 + c;
    float a = 0.f, b = 0.f;
    if (y < H && x < W) {
      const float pv = p[(size_t)y * W + x], tv = t[(size_t)y * Wt + x];
      if (r < own_h && c < own_w) {
        const float d = pv - tv;
        se = fmaf(d, d, se);
      }
      a = pv - pivot;
      b = tv - pivot;
    }
    sa[i] = a;
    sb[i] = b;
  }
  const double range = data_range ? (double)data_range[bc] : S[4] - S[3];
  if (blockIdx.x == 0 && threadIdx.x == 0) S[5] = range;
  const float R = (float)range;
  const float c1 = (0.01f * R) * (0.01f * R), c2 = (0.03f * R) * (0.03f * R);
  __syncthreads();

  const int lx = threadIdx.x & 63, ry0 = (threadIdx.x >> 6) * SS_STRIP;
  const bool col_ok = x0 + lx < Wv;
  // the tile's pivot is up to 38 x 70 pixels away, too far for a smooth field that spans its range inside a tile: every lane
  // centres once more, on the (centred) target under the middle of the 14 x 7 pixels its windows cover
  const int prow = min(ry0 + SS_WIN / 2 + SS_STRIP / 2, H - 1 - y0);
  const float local = sb[prow * SS_IW + lx + SS_WIN / 2];
  const float shift = local + pivot;
  float ring[SS_WIN][5];
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < SS_STRIP + SS_HALO; ++j) {
    const float* ra = sa + (ry0 + j) * SS_IW + lx;
    const float* rb = sb + (ry0 + j) * SS_IW + lx;
    float ua = 0.f, ub = 0.f, uaa = 0.f, ubb = 0.f, uab = 0.f;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {
      const float a = ra[k] - local, b = rb[k] - local;
      ua += a;
      ub += b;
      uaa = fmaf(a, a, uaa);
      ubb = fmaf(b, b, ubb);
      uab = fmaf(a, b, uab);
    }
    ring[j % SS_WIN][0] = ua, ring[j % SS_WIN][1] = ub, ring[j % SS_WIN][2] = uaa, ring[j % SS_WIN][3] = ubb,
    ring[j % SS_WIN][4] = uab;
    if (j < SS_HALO) continue;
    float w[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float v = ring[(j + 1) % SS_WIN][q];              // oldest first
#pragma unroll
      for (int k = 2; k <= SS_WIN; ++k) v += ring[(j + k) % SS_WIN][q];
      w[q] = v;
    }
    const float inv_n = 1.f / (SS_WIN * SS_WIN), inv_n1 = 1.f / (SS_WIN * SS_WIN - 1);
    const float ma = w[0] * inv_n, mb = w[1] * inv_n;                       // centred means
    const float va = (w[2] - w[0] * ma) * inv_n1, vb = (w[3] - w[1] * mb) * inv_n1, vab = (w[4] - w[0] * mb) * inv_n1;
    const float ux = ma + shift, uy = mb + shift;
    const float num = (2.f * ux * uy + c1) * (2.f * vab + c2);
    const float den = (ux * ux + uy * uy + c1) * (va + vb + c2);
    const float ssim = num / den;
    const int cy = y0 + ry0 + j - SS_HALO;              // the centre in valid coordinates; its pixel row is cy + 3
    if (col_ok && cy < Hv) {
      s0 += ssim;
      s1 += (lat_w ? lat_w[cy + SS_WIN / 2] : 1.f) * ssim;
      if (ssim_map) ssim_map[((size_t)bc * Hv + cy) * Wv + x0 + lx] = ssim;
    }
  }
  const float s[3] = {s0, s1, se};
  o2_block_sums_add(s, S);
}
}  // namespace

extern "C" int orbit2_ssim(const float* pred, const float* target, int Ht, int Wt, const float* lat_w, const float* data_range,
                           double* sums, float* ssim_map, int B, int C, int H, int W, void* stream) {
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !sums || H < SS_WIN || W < SS_WIN) return O2_ERR_ARG;
  if ((int64_t)B * C > 65535) return O2_ERR_ARG;
  const int ntx = (W - SS_HALO + SS_TW - 1) / SS_TW, nty = (H - SS_HALO + SS_TH - 1) / SS_TH;
  if ((int64_t)ntx * nty > INT32_MAX) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int BC = B * C;
  hipLaunchKernelGGL(ssim_init_kernel, dim3((BC + 255) / 256), dim3(256), 0, s, sums, BC);
  const int cap = o2_image_block_cap(BC);
  hipLaunchKernelGGL(ssim_range_kernel, dim3(H < cap ? H : cap, BC), dim3(256), 0, s, target, Ht, Wt, sums, H, W);
  hipLaunchKernelGGL(ssim_kernel, dim3(ntx * nty, BC), dim3(256), 0, s, pred, target, Ht, Wt, lat_w, data_range, sums, ssim_map,
                     H, W, ntx);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
