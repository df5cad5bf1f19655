// Interpolation baselines: F.interpolate(size=(H, W), mode=nearest | bilinear | bicubic, align_corners=False, no antialiasing)
// of gathered channels of an fp32 [B, in_ctotal, h, w] field, with an optional per-channel affine, either stored
// (orbit2_resample_fwd) or scored against a target without ever being stored (orbit2_resample_moments: the twelve sums of
// orbit2_eval_moments).  include/orbit2_hip.h: orbit2_resample_*; models/hub/interpolation.py; DESIGN 4.10c.
//
// A workgroup owns one RS_TH x RS_TW tile of one (b, c) output image.  A lane owns FOUR CONSECUTIVE output columns, so a wave
// covers the tile's 256 columns and stores (or reads the target as) one float4 per lane and row; wave v takes rows v, v + 4, ...
// of the tile.  The column taps (source indices and weights of the lane's four columns) are computed once and stay in registers
// for all rows; the row taps are computed once per row from a wave-uniform row number.  The source pixels under the tile are
// staged in LDS once when the call's full-tile footprint fits ORBIT2_RESAMPLE_LDS_FLOATS (every upsampling ratio and the
// identity), else the taps are read straight from global memory (a downsampling footprint can be arbitrarily large).
//
// COORDINATES ARE PART OF THE CONTRACT: fp32, every product and difference rounded on its own (rs_rounded in rs_taps:
// hipcc contracts a * b - c into one fma otherwise, which moves a coordinate that sits on an integer to the other side of it).
//   ratio = (float)in / (float)out
//   nearest   i = min((int)floorf(o * ratio), in - 1)
//   bilinear  s = max(ratio * (o + 0.5f) - 0.5f, 0);  i0 = (int)s, i1 = min(i0 + 1, in - 1), l1 = s - i0, l0 = 1 - l1
//   bicubic   s = ratio * (o + 0.5f) - 0.5f;  b = floorf(s), t = s - b, taps b - 1 .. b + 2 clamped, cubic convolution A = -0.75,
//             the weight polynomials in Horner form, their products rounded on their own too
// Summation order: a row interpolant is its taps left to right (first product, then fmaf), a pixel its row interpolants top to
// bottom in the same way, then fmaf(scale[c], r, shift[c]).  Every source index is clamped into the grid and no address depends
// on a data value: non-finite inputs give unspecified values, never a fault.
#include "score_sums.h"
#include "../../include/orbit2_hip.h"

namespace {
constexpr int RS_TH = ORBIT2_RESAMPLE_TILE_H, RS_TW = ORBIT2_RESAMPLE_TILE_W, RS_LDS = ORBIT2_RESAMPLE_LDS_FLOATS;
constexpr int RS_NM = O2_NMOMENTS;
static_assert(RS_TW == 256 && RS_TH % 4 == 0, "a wave's 64 lanes x 4 columns span the tile, four waves share its rows");

template <int MODE> struct rs_ntaps { static constexpr int value = MODE == 0 ? 1 : (MODE == 1 ? 2 : 4); };

__device__ __forceinline__ int rs_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// A product that stays a product.  hipcc's __fmul_rn / __fsub_rn are plain operators and `#pragma clang fp contract(off)` does not
// reach the back end's own contraction: with either, the listing has v_fma_f32 s, ratio, o + 0.5, -0.5.  An empty asm statement
// that claims to modify the value costs no instruction and leaves nothing to fuse with.
__device__ __forceinline__ float rs_rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// source indices (clamped into 0 .. n_in - 1, ascending) and weights of output coordinate o
template <int MODE>
__device__ __forceinline__ void rs_taps(int o, int n_in, float ratio, int* idx, float* w) {
  if (MODE == 0) {
    idx[0] = rs_clamp((int)floorf(rs_rounded((float)o * ratio)), n_in);
    w[0] = 1.f;
  } else if (MODE == 1) {
    const float s = fmaxf(rs_rounded(ratio * ((float)o + 0.5f)) - 0.5f, 0.f);
    const int i0 = rs_clamp((int)s, n_in);
    idx[0] = i0;
    idx[1] = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
    w[1] = s - (float)i0;
    w[0] = 1.f - w[1];
  } else {
    const float s = rs_rounded(ratio * ((float)o + 0.5f)) - 0.5f;
    const float fl = floorf(s);
    const float t = s - fl;
    // finite coordinates give -1 .. n_in - 1; the conversion of anything else saturates, and base - 1 + k must not wrap
    const int base = max(-2, min((int)fl, n_in + 1));
    constexpr float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    // ((A x - 5A) x + 8A) x - 4A and ((A + 2) x - (A + 3)) x x + 1 with every product rounded on its own as well: 8A x - 4A
    // cancels, so a weight carries several ulp(1) of its evaluation order, and sixteen of them 25 ulp(max|x|) of a pixel (measured
    // at 6x10 -> 17x23).  Unfused, the weights are bit for bit those of the float64 replica the tests compare with.
    auto outer = [](float x) { return rs_rounded((rs_rounded((rs_rounded(A * x) - 5.0f * A) * x) + 8.0f * A) * x) - 4.0f * A; };
    auto inner = [](float x) { return rs_rounded(rs_rounded((rs_rounded((A + 2.0f) * x) - (A + 3.0f)) * x) * x) + 1.0f; };
    w[0] = outer(x0), w[1] = inner(x1), w[2] = inner(x2), w[3] = outer(x3);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = rs_clamp(base - 1 + k, n_in);
  }
}

// The tile's rows.  SRC is the image in global memory (pitch w, offsets 0) or the staged window in LDS (pitch ww, offsets ylo, xlo).
template <int MODE, bool MOMENTS, bool STAGED>
__device__ __forceinline__ void rs_rows(const float* __restrict__ src, int pitch, int yoff, int xoff, int h, int w, int H,
                                        int W, float ry, float rx, int y0, int x0, bool affine, float sc, float sh,
                                        float* __restrict__ orow0, const float* __restrict__ trow0, int Wt,
                                        const float* __restrict__ lat_w, const float* __restrict__ crow0, float (&s)[RS_NM]) {
  constexpr int NT = rs_ntaps<MODE>::value;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xl = x0 + 4 * lane;                    // the lane's first output column
  int cx[4][NT];
  float wx[4][NT];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // a column past the image takes the last column's taps: in range, never stored or summed
    rs_taps<MODE>(xl + j < W ? xl + j : W - 1, w, rx, cx[j], wx[j]);
#pragma unroll
    for (int k = 0; k < NT; ++k) cx[j][k] -= xoff;
  }
  for (int r = wave; r < RS_TH; r += 4) {
    const int y = y0 + r;
    if (y >= H) break;
    int cy[NT];
    float wy[NT];
    rs_taps<MODE>(y, h, ry, cy, wy);
    float v[4];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const float* row = src + (size_t)(cy[k] - yoff) * pitch;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t;
        if (MODE == 0) {
          t = row[cx[j][0]];
        } else {
          t = wx[j][0] * row[cx[j][0]];
#pragma unroll
          for (int q = 1; q < NT; ++q) t = fmaf(wx[j][q], row[cx[j][q]], t);
        }
        if (MODE == 0) v[j] = t;
        else v[j] = k == 0 ? wy[0] * t : fmaf(wy[k], t, v[j]);
      }
    }
    if (affine) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaf(sc, v[j], sh);
    }
    if (!MOMENTS) {
      float* o = orow0 + (size_t)y * W + xl;
      // one float4 where the lane's four columns exist and sit on a 16-byte boundary (an odd W misaligns every second row)
      if (xl + 3 < W && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (xl + j < W) o[j] = v[j];
      }
    } else {
      const float* t = trow0 + (size_t)y * Wt + xl;
      const float* c = crow0 ? crow0 + (size_t)y * W + xl : nullptr;
      float tv[4], cv[4] = {0.f, 0.f, 0.f, 0.f};
      const bool full = xl + 3 < W;
      if (full && ((uintptr_t)t & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(t);
        tv[0] = q.x, tv[1] = q.y, tv[2] = q.z, tv[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) tv[j] = xl + j < W ? t[j] : 0.f;
      }
      if (c) {
        if (full && ((uintptr_t)c & 15) == 0) {
          const float4 q = *reinterpret_cast<const float4*>(c);
          cv[0] = q.x, cv[1] = q.y, cv[2] = q.z, cv[3] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) cv[j] = xl + j < W ? c[j] : 0.f;
        }
      }
      const float lw = lat_w ? lat_w[y] : 1.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (xl + j < W) o2_moments_add(s, v[j] - cv[j], tv[j] - cv[j], lw);
      }
    }
  }
}

template <int MODE, bool MOMENTS>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, const int* __restrict__ chan_idx,
                                                       int in_ctotal, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, float* __restrict__ out,
                                                       const float* __restrict__ target, int Ht, int Wt,
                                                       const float* __restrict__ lat_w, const float* __restrict__ clim,
                                                       double* __restrict__ sums, int C, int h, int w, int H, int W, int ntx,
                                                       int stage, float ry, float rx) {
  constexpr int NT = rs_ntaps<MODE>::value;
  __shared__ float win[RS_LDS];
  const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int y0 = ty * RS_TH, x0 = tx * RS_TW;
  const int ci = chan_idx ? chan_idx[c] : c;
  const float* src = x + ((size_t)b * in_ctotal + ci) * h * w;
  const bool affine = scale != nullptr;
  const float sc = affine ? scale[c] : 1.f, sh = affine ? shift[c] : 0.f;
  float* orow0 = MOMENTS ? nullptr : out + (size_t)bc * H * W;
  const float* trow0 = MOMENTS ? target + (size_t)bc * Ht * Wt : nullptr;
  const float* crow0 = MOMENTS && clim ? clim + (size_t)c * H * W : nullptr;
  float s[RS_NM];
#pragma unroll
  for (int k = 0; k < RS_NM; ++k) s[k] = 0.f;

  // the source window under the tile: the coordinate is monotone in o, so the first tap of the tile's first row / column and
  // the last tap of its last ones bound every tap in between
  int lo[NT], hi[NT];
  float wgt[NT];
  rs_taps<MODE>(y0, h, ry, lo, wgt);
  rs_taps<MODE>(min(y0 + RS_TH, H) - 1, h, ry, hi, wgt);
  const int ylo = lo[0], wh = hi[NT - 1] - ylo + 1;
  rs_taps<MODE>(x0, w, rx, lo, wgt);
  rs_taps<MODE>(min(x0 + RS_TW, W) - 1, w, rx, hi, wgt);
  const int xlo = lo[0], ww = hi[NT - 1] - xlo + 1;
  // `stage` is the host's rule (the full-tile footprint of this ratio fits); the window itself is checked all the same
  if (stage && wh > 0 && ww > 0 && (int64_t)wh * ww <= RS_LDS) {
    // a wave per window row, lanes along it: coalesced, and no division by the window's width
    for (int r = threadIdx.x >> 6; r < wh; r += 4)
      for (int q = threadIdx.x & 63; q < ww; q += 64) win[r * ww + q] = src[(size_t)(ylo + r) * w + xlo + q];
    __syncthreads();
    rs_rows<MODE, MOMENTS, true>(win, ww, ylo, xlo, h, w, H, W, ry, rx, y0, x0, affine, sc, sh, orow0, trow0, Wt, lat_w, crow0,
                                 s);
  } else {
    rs_rows<MODE, MOMENTS, false>(src, w, 0, 0, h, w, H, W, ry, rx, y0, x0, affine, sc, sh, orow0, trow0, Wt, lat_w, crow0, s);
  }
  if (MOMENTS) o2_block_sums_add(s, sums + (size_t)bc * RS_NM);
}

// ceil(tile * in / out) + 4: no window of a tile at this ratio is larger (a bicubic footprint is the span of the floors + 4)
inline int64_t rs_footprint(int tile, int n_in, int n_out) { return ((int64_t)tile * n_in + n_out - 1) / n_out + 4; }

template <bool MOMENTS>
int rs_launch(const float* x, const int* chan_idx, int in_ctotal, const float* scale, const float* shift, float* out,
              const float* target, int Ht, int Wt, const float* lat_w, const float* clim, double* sums, int B, int C, int h,
              int w, int H, int W, int mode, hipStream_t s) {
  if (!x || (MOMENTS ? (!sums || !target) : !out) || (scale == nullptr) != (shift == nullptr)) return O2_ERR_ARG;
  if (B <= 0 || C <= 0 || in_ctotal <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 2) return O2_ERR_ARG;
  if (!chan_idx && C != in_ctotal) return O2_ERR_ARG;
  if (MOMENTS && (Ht < H || Wt < W)) return O2_ERR_ARG;
  if ((int64_t)B * C > 65535) return O2_ERR_ARG;
  const int ntx = (W + RS_TW - 1) / RS_TW, nty = (H + RS_TH - 1) / RS_TH;
  if ((int64_t)ntx * nty > INT32_MAX) return O2_ERR_ARG;
  if (MOMENTS && hipMemsetAsync(sums, 0, sizeof(double) * (size_t)B * C * RS_NM, s) != hipSuccess) return O2_ERR_LAUNCH;
  const int stage = rs_footprint(RS_TH, h, H) * rs_footprint(RS_TW, w, W) <= RS_LDS;
  const dim3 grid(ntx * nty, B * C);
  // the two ratios of the contract, one correctly rounded fp32 division each: formed here once, not by every thread
  const float ry = (float)h / (float)H, rx = (float)w / (float)W;
#define RS_GO(M)                                                                                                             \
  hipLaunchKernelGGL((resample_kernel<M, MOMENTS>), grid, dim3(256), 0, s, x, chan_idx, in_ctotal, scale, shift, out, target, \
                     Ht, Wt, lat_w, clim, sums, C, h, w, H, W, ntx, stage, ry, rx)
  if (mode == 0) RS_GO(0);
  else if (mode == 1) RS_GO(1);
  else RS_GO(2);
#undef RS_GO
  O2_CHECK_LAUNCH();
  return O2_OK;
}
}  // namespace

extern "C" int orbit2_resample_fwd(const float* x, const int* chan_idx, int in_ctotal, const float* scale, const float* shift,
                                   float* out, int B, int C, int h, int w, int H, int W, int mode, void* stream) {
  return rs_launch<false>(x, chan_idx, in_ctotal, scale, shift, out, nullptr, 0, 0, nullptr, nullptr, nullptr, B, C, h, w, H, W,
                          mode, (hipStream_t)stream);
}

extern "C" int orbit2_resample_moments(const float* x, const int* chan_idx, int in_ctotal, const float* scale,
                                       const float* shift, const float* target, int Ht, int Wt, const float* lat_w,
                                       const float* clim, double* out, int B, int C, int h, int w, int H, int W, int mode,
                                       void* stream) {
  return rs_launch<true>(x, chan_idx, in_ctotal, scale, shift, nullptr, target, Ht, Wt, lat_w, clim, out, B, C, h, w, H, W, mode,
                         (hipStream_t)stream);
}
