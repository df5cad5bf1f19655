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

// ---- the window arithmetic, stated once: ssim_kernel and ssim_vjp_kernel both go through these four steps, so the S a training
// loss differentiates is the metric's S (tests/ssim_loss_ref.emulate restates the order in numpy).  PITCH: the kernel's LDS pitch
constexpr float SS_INV_N = 1.f / (SS_WIN * SS_WIN), SS_INV_N1 = 1.f / (SS_WIN * SS_WIN - 1);
struct SsConsts { float c1, c2; };
__device__ __forceinline__ SsConsts ss_consts(float R) { return {(0.01f * R) * (0.01f * R), (0.03f * R) * (0.03f * R)}; }
// the row step: the five 7-tap sums (a, b, a^2, b^2, a b) of one staged row minus the thread's second pivot, into a ring slot
template <int PITCH>
__device__ __forceinline__ void ss_row_sums(const float* sa, const float* sb, int row, int col, float local, float (&slot)[5]) {
  const float* ra = sa + row * PITCH + col;
  const float* rb = sb + row * PITCH + col;
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
  slot[0] = ua, slot[1] = ub, slot[2] = uaa, slot[3] = ubb, slot[4] = uab;
}
// the window step: the sums of the window whose last row went into slot j % 7 (j a constant of an unrolled loop: every index is
// a compile-time constant), the seven row sums added oldest first
__device__ __forceinline__ void ss_window_sums(const float (&ring)[SS_WIN][5], int j, float (&w)[5]) {
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float v = ring[(j + 1) % SS_WIN][q];                // oldest first
#pragma unroll
    for (int k = 2; k <= SS_WIN; ++k) v += ring[(j + k) % SS_WIN][q];
    w[q] = v;
  }
}
// the moments step: centred means, the variances and the covariance from the centred sums, and the means with both pivots
// (shift = local + the tile's pivot) added back for the luminance term
struct SsMoments { float ma, mb, va, vb, vab, ux, uy; };
__device__ __forceinline__ SsMoments ss_moments(const float (&w)[5], float shift) {
  const float ma = w[0] * SS_INV_N, mb = w[1] * SS_INV_N;                   // centred means
  const float va = (w[2] - w[0] * ma) * SS_INV_N1, vb = (w[3] - w[1] * mb) * SS_INV_N1, vab = (w[4] - w[0] * mb) * SS_INV_N1;
  return {ma, mb, va, vb, vab, ma + shift, mb + shift};
}

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
  const auto [c1, c2] = ss_consts((float)range);
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
    ss_row_sums<SS_IW>(sa, sb, ry0 + j, lx, local, ring[j % SS_WIN]);
    if (j < SS_HALO) continue;
    float w[5];
    ss_window_sums(ring, j, w);
    const auto [ma, mb, va, vb, vab, ux, uy] = ss_moments(w, shift);
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
// ---- the vector-Jacobian product of the sums: orbit2_loss_bwd(kind = ORBIT2_LOSS_SSIM_VJP) -----------------------
// dpred[p] = g sum over the valid centres k whose window holds p of w_k dS_k / dpred[p].  A workgroup owns SV_TH x SV_TW OUTPUT
// pixels of one image.  It stages the pixels under them plus a halo of 6, of both fields, minus the tile's pivot (the target at
// the tile's first pixel); forms, at the centres under the tile plus a halo of 3, three maps -- by the forward's own steps (the
// ss_ functions above) and its second, per-thread pivot, so S is the forward's S --; box-sums the maps 7 x 7, rows then columns,
// through LDS (the row sums take the place of the staged pixels, whose tile part every thread has read into registers); and
// writes every pixel of its tile once: no atomics, the same bits on every call.  With alpha, beta, gamma of the header and the
// means mx = ux - v, my = uy - v relative to the tile's pivot v, the header's five box sums fold by linearity into three:
//   E0 = w (alpha / 49 - (2 beta mx + gamma my) / 48),  E1 = 2 w beta / 48,  E2 = w gamma / 48
//   d[p] = g (box(E0) + (x_p - v) box(E1) + (y_p - v) box(E2)).
// alpha's factor uy - ux A1 / B1 is formed as (uy - ux) (uy (ux + uy) + C1) / B1 with uy - ux from the centred means: at 280 K
// the literal form cancels seven digits away.  An invalid centre's maps are 0 by selection, never by a product.
constexpr int SV_TH = ORBIT2_SSIM_VJP_TILE_H, SV_TW = ORBIT2_SSIM_VJP_TILE_W;
constexpr int SV_PH = SV_TH + 2 * SS_HALO, SV_PW = SV_TW + 2 * SS_HALO;     // the staged pixels of a tile: 28 x 76
constexpr int SV_MH = SV_TH + SS_HALO, SV_MW = SV_TW + SS_HALO;             // the centres whose windows touch the tile: 22 x 70
constexpr int SV_NMAP = 3;
constexpr int SV_STRIPS = 3, SV_RS = (SV_MH + SV_STRIPS - 1) / SV_STRIPS;   // a thread owns one column of SV_RS centre rows
constexpr int SV_HB = SV_NMAP * SV_MH * SV_TW;                              // the row-summed maps
constexpr int SV_PIX = 2 * SV_PH * SV_PW > SV_HB ? 2 * SV_PH * SV_PW : SV_HB;
static_assert(SV_TW == 64 && SV_TH % 16 == 0 && SV_STRIPS * SV_MW <= 256, "16 x 16 threads of four pixels; a thread per column");
static_assert((SV_PIX + SV_NMAP * SV_MH * SV_MW) * 4 <= 64 * 1024, "static LDS");

__device__ __forceinline__ void sv_store4(float* __restrict__ d, int y, int x, int H, int W, bool vec, float4 v) {
  if (y >= H || x >= W) return;
  float* o = d + (size_t)y * W + x;
  if (vec) {                                            // W % 4 == 0 and x % 4 == 0: the four pixels are inside, 16-byte aligned
    *reinterpret_cast<float4*>(o) = v;
    return;
  }
  o[0] = v.x;
  if (x + 1 < W) o[1] = v.y;
  if (x + 2 < W) o[2] = v.z;
  if (x + 3 < W) o[3] = v.w;
}

__global__ __launch_bounds__(256) void ssim_vjp_kernel(const float* __restrict__ pred, const float* __restrict__ target, int Ht,
                                                       int Wt, const float* __restrict__ lat_w,
                                                       const float* __restrict__ gscale, float* __restrict__ dpred, int BC,
                                                       int H, int W, int ntx) {
  __shared__ __attribute__((aligned(16))) float pix[SV_PIX];
  __shared__ float maps[SV_NMAP * SV_MH * SV_MW];
  const int bc = blockIdx.y;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int py0 = ty * SV_TH, px0 = tx * SV_TW;         // the tile's first pixel
  float* d = dpred + (size_t)bc * H * W;
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(dpred) & 15) == 0;
  const int orow = threadIdx.x >> 4, oc = (threadIdx.x & 15) * 4;   // output: rows orow + 16 k, four pixels from column oc
  const float g = gscale[bc];
  if (g == 0.f) {                                       // nothing of this image is read: its values may be anything
    for (int r = orow; r < SV_TH; r += 16) sv_store4(d, py0 + r, px0 + oc, H, W, vec, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  const float* p = pred + (size_t)bc * H * W;
  const float* t = target + (size_t)bc * Ht * Wt;
  const auto [c1, c2] = ss_consts(gscale[BC + bc]);
  const float pivot = t[(size_t)py0 * Wt + px0];
  float* sa = pix;
  float* sb = pix + SV_PH * SV_PW;
  for (int i = threadIdx.x; i < SV_PH * SV_PW; i += 256) {
    const int r = i / SV_PW, c = i - r * SV_PW;
    const int y = py0 - SS_HALO + r, x = px0 - SS_HALO + c;
    float a = 0.f, b = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      a = p[(size_t)y * W + x] - pivot;
      b = t[(size_t)y * Wt + x] - pivot;
    }
    sa[i] = a;
    sb[i] = b;
  }
  __syncthreads();

  float xa[SV_TH / 16][4], ya[SV_TH / 16][4];           // the thread's own pixels, centred on the tile's pivot
#pragma unroll
  for (int k = 0; k < SV_TH / 16; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = (orow + 16 * k + SS_HALO) * SV_PW + oc + q + SS_HALO;
      xa[k][q] = sa[i];
      ya[k][q] = sb[i];
    }

  if (threadIdx.x < SV_STRIPS * SV_MW) {
    const int strip = threadIdx.x / SV_MW, c = threadIdx.x - strip * SV_MW, mr0 = strip * SV_RS;
    // the second pivot, as in the forward: the stored target under the middle of the pixels this thread's windows cover,
    // moved inside the image
    const int prow = max(min(min(mr0 + SS_WIN / 2 + SV_RS / 2, SV_PH - 1), H - 1 - py0 + SS_HALO), SS_HALO - py0);
    const int pcol = max(min(c + SS_WIN / 2, W - 1 - px0 + SS_HALO), SS_HALO - px0);
    const float local = sb[prow * SV_PW + pcol];
    const float shift = local + pivot;
    const int cx = px0 - SS_WIN / 2 + c;                // the centre's pixel column
    float ring[SS_WIN][5];
#pragma unroll
    for (int j = 0; j < SV_RS + SS_HALO; ++j) {
      ss_row_sums<SV_PW>(sa, sb, min(mr0 + j, SV_PH - 1), c, local, ring[j % SS_WIN]);
      if (j < SS_HALO) continue;
      float w[5];
      ss_window_sums(ring, j, w);
      const int mr = mr0 + j - SS_HALO;                 // the centre's map row; its pixel row is cy
      const int cy = py0 - SS_WIN / 2 + mr;
      if (mr >= SV_MH) continue;
      const bool valid = cy >= SS_WIN / 2 && cy < H - SS_WIN / 2 && cx >= SS_WIN / 2 && cx < W - SS_WIN / 2;
      const auto [ma, mb, va, vb, vab, ux, uy] = ss_moments(w, shift);
      const float A1 = 2.f * ux * uy + c1, A2 = 2.f * vab + c2;
      const float B1 = ux * ux + uy * uy + c1, B2 = va + vb + c2;
      const float rB = 1.f / (B1 * B2);
      const float S = A1 * A2 * rB;
      const float alpha = 2.f * A2 * rB * ((mb - ma) * (uy * (ux + uy) + c1)) / B1;
      const float beta = -S / B2;
      const float gamma = 2.f * A1 * rB;
      const float mx = ma + local, my = mb + local;     // the means relative to the tile's pivot
      const float wk = (valid && lat_w) ? lat_w[cy] : 1.f;
      const float e0 = wk * (alpha * SS_INV_N - (2.f * beta * mx + gamma * my) * SS_INV_N1);
      const float e1 = wk * (2.f * beta * SS_INV_N1);
      const float e2 = wk * (gamma * SS_INV_N1);
      float* m = maps + mr * SV_MW + c;
      m[0] = valid ? e0 : 0.f;
      m[SV_MH * SV_MW] = valid ? e1 : 0.f;
      m[2 * SV_MH * SV_MW] = valid ? e2 : 0.f;
    }
  }
  __syncthreads();

  float* hb = pix;                                      // [map][centre row][tile column]: the seven centres across a pixel
  for (int i = threadIdx.x; i < SV_HB; i += 256) {
    const int qr = i / SV_TW, c = i - qr * SV_TW;
    const float* m = maps + qr * SV_MW + c;
    float v = m[0];
#pragma unroll
    for (int k = 1; k < SS_WIN; ++k) v += m[k];
    hb[i] = v;
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < SV_TH / 16; ++k) {
    const int r = orow + 16 * k;
    float4 bx[SV_NMAP];
#pragma unroll
    for (int q = 0; q < SV_NMAP; ++q) {
      const float4* col = reinterpret_cast<const float4*>(hb + (q * SV_MH + r) * SV_TW + oc);
      float4 v = col[0];
#pragma unroll
      for (int dy = 1; dy < SS_WIN; ++dy) {
        const float4 u = col[dy * (SV_TW / 4)];
        v.x += u.x, v.y += u.y, v.z += u.z, v.w += u.w;
      }
      bx[q] = v;
    }
    float4 o;
    o.x = g * fmaf(ya[k][0], bx[2].x, fmaf(xa[k][0], bx[1].x, bx[0].x));
    o.y = g * fmaf(ya[k][1], bx[2].y, fmaf(xa[k][1], bx[1].y, bx[0].y));
    o.z = g * fmaf(ya[k][2], bx[2].z, fmaf(xa[k][2], bx[1].z, bx[0].z));
    o.w = g * fmaf(ya[k][3], bx[2].w, fmaf(xa[k][3], bx[1].w, bx[0].w));
    sv_store4(d, py0 + r, px0 + oc, H, W, vec, o);
  }
}
// what both entries refuse: an image smaller than one window, more images than blockIdx.y holds, more tiles (ntx along W, nty
// along H, of the entry's own tile) than the int that blockIdx.x is decoded in
inline bool ss_grid_ok(int B, int C, int H, int W, int ntx, int nty) {
  return H >= SS_WIN && W >= SS_WIN && (int64_t)B * C <= 65535 && (int64_t)ntx * nty <= INT32_MAX;
}
}  // namespace

// the kind ORBIT2_LOSS_SSIM_VJP of orbit2_loss_bwd (loss.hip), which has checked the pair, gscale and dpred
int o2_ssim_vjp(const float* pred, const float* target, int Ht, int Wt, const float* lat_w, const float* gscale, float* dpred,
                int B, int C, int H, int W, hipStream_t s) {
  const int ntx = (W + SV_TW - 1) / SV_TW, nty = (H + SV_TH - 1) / SV_TH;
  if (!ss_grid_ok(B, C, H, W, ntx, nty)) return O2_ERR_ARG;
  hipLaunchKernelGGL(ssim_vjp_kernel, dim3(ntx * nty, B * C), dim3(256), 0, s, pred, target, Ht, Wt, lat_w, gscale, dpred, B * C,
                     H, W, ntx);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_ssim(const float* pred, const float* target, int Ht, int Wt, const float* lat_w, const float* data_range,
                           double* sums, float* ssim_map, int B, int C, int H, int W, void* stream) {
  const int ntx = (W - SS_HALO + SS_TW - 1) / SS_TW, nty = (H - SS_HALO + SS_TH - 1) / SS_TH;
  if (!o2_pair_ok(pred, target, B, C, H, W, Ht, Wt) || !sums || !ss_grid_ok(B, C, H, W, ntx, nty)) return O2_ERR_ARG;
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
