// The per-step image-grid ops of Res_Slim_ViT (fp32, HBM-bound, tiny): unpatchify in its three forms (bf16 / fp32 tokens forward,
// bf16 backward), the three 3x3 conv kernels (forward with GELU + PixelShuffle or an addend, data gradient, weight / bias
// gradient), the precipitation clamp and its backward, the position-embedding re-grid.  Losses: loss.hip; scores: ensemble.hip.
#include "common.h"
#include "../../include/orbit2_hip.h"

namespace {
inline int img_grid(int64_t n) { return grid_for(n, 256, 8192); }   // this file's grid-stride launches: up to 8192 blocks of 256

// ---- unpatchify (res_slimvit.py:167-179): pure index permutation -------------------------------
// img[b][c][hh*p+pp][ww*p+qq] = t[b][ (((hh*wf + ww)*p + pp)*p + qq)*C + c ],  hf = h*s/p, wf = w*s/p
// T_FP32 (forward only): t holds fp32 tokens (the fp32 forward path)
template <bool BWD, bool T_FP32 = false>
__global__ __launch_bounds__(256) void unpatchify_kernel(bf16_t* __restrict__ t, float* __restrict__ img, int B, int C,
                                                         int Hh, int Wh, int p) {
  const int64_t per = (int64_t)C * Hh * Wh;
  const int64_t n = (int64_t)B * per;
  const int wf = Wh / p;
  O2_GRID_STRIDE(e, n) {
    const int b = (int)(e / per);
    int64_t r = e - (int64_t)b * per;
    if (!BWD) {
      // e enumerates img elements
      const int c = (int)(r / ((int64_t)Hh * Wh));
      r -= (int64_t)c * Hh * Wh;
      const int y = (int)(r / Wh), x = (int)(r - (int64_t)y * Wh);
      const int hh = y / p, pp = y - hh * p, ww = x / p, qq = x - ww * p;
      const int64_t ti = ((((int64_t)hh * wf + ww) * p + pp) * p + qq) * C + c;
      img[e] = T_FP32 ? reinterpret_cast<const float*>(t)[(int64_t)b * per + ti] : bf2f(t[(int64_t)b * per + ti]);
    } else {
      // e enumerates t elements
      const int c = (int)(r % C);
      int64_t q = r / C;
      const int qq = (int)(q % p); q /= p;
      const int pp = (int)(q % p); q /= p;
      const int ww = (int)(q % wf);
      const int hh = (int)(q / wf);
      t[e] = f2bf(img[(int64_t)b * per + ((int64_t)c * Hh + (hh * p + pp)) * Wh + (ww * p + qq)]);
    }
  }
}

// PixelShuffle(r): conv channel co = oc * r^2 + sub of pixel (y, x) is pixel (y r + sub / r, x r + sub % r) of channel oc of the
// [B][Cout / r^2][H r][W r] image -- the forward's destination, the backward's source
__device__ __forceinline__ size_t ps_index(int b, int co, int y, int x, int Cout, int H, int W, int r) {
  const int rr = r * r;
  const int oc = co / rr, sub = co - oc * rr;
  return (((size_t)b * (Cout / rr) + oc) * (H * r) + (y * r + sub / r)) * (size_t)(W * r) + (x * r + sub % r);
}

// ---- 3x3 conv forward: one thread per output pixel, COB output channels per pass ---------------
constexpr int CONV_MAXCIN = 8;
constexpr int COB = 16;
__global__ __launch_bounds__(256) void conv3x3_fwd_kernel(const float* __restrict__ in, const int* __restrict__ cidx,
                                                          int in_ctotal, const float* __restrict__ wgt,
                                                          const float* __restrict__ bias, float* __restrict__ out,
                                                          float* __restrict__ pre, const float* __restrict__ addend,
                                                          int Ha, int Wa, int B, int Cin, int Cout, int H, int W,
                                                          int mode, int r) {
  __shared__ float sw[COB * CONV_MAXCIN * 9 + COB];
  const int co0 = blockIdx.y * COB;
  const int nco = (Cout - co0) < COB ? (Cout - co0) : COB;
  for (int e = threadIdx.x; e < nco * Cin * 9; e += 256) sw[e] = wgt[(size_t)co0 * Cin * 9 + e];
  for (int e = threadIdx.x; e < nco; e += 256) sw[COB * CONV_MAXCIN * 9 + e] = bias[co0 + e];
  __syncthreads();
  const int64_t npix = (int64_t)B * H * W;
  O2_GRID_STRIDE(px, npix) {
    const int b = (int)(px / ((int64_t)H * W));
    const int rem = (int)(px - (int64_t)b * H * W);
    const int y = rem / W, x = rem - y * W;
    float nb[CONV_MAXCIN][9];
#pragma unroll
    for (int ci = 0; ci < CONV_MAXCIN; ++ci) {
      if (ci < Cin) {
        const int cs = cidx ? cidx[ci] : ci;
        const float* pl = in + ((size_t)b * in_ctotal + cs) * H * W;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
          nb[ci][k] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? pl[(size_t)yy * W + xx] : 0.f;
        }
      }
    }
    for (int co = 0; co < nco; ++co) {
      float acc = sw[COB * CONV_MAXCIN * 9 + co];
#pragma unroll
      for (int ci = 0; ci < CONV_MAXCIN; ++ci) {
        if (ci < Cin) {
#pragma unroll
          for (int k = 0; k < 9; ++k) acc = fmaf(sw[(co * Cin + ci) * 9 + k], nb[ci][k], acc);
        }
      }
      const int cg = co0 + co;
      if (mode == 0) {
        if (addend) acc += addend[(((size_t)b * Cout + cg) * Ha + y) * Wa + x];
        out[(((size_t)b * Cout + cg) * H + y) * W + x] = acc;
      } else {
        pre[(((size_t)b * Cout + cg) * H + y) * W + x] = acc;
        out[ps_index(b, cg, y, x, Cout, H, W, r)] = gelu_f(acc);
      }
    }
  }
}

// dpre value at (b, co, y, x) for either mode
__device__ __forceinline__ float conv_dpre(const float* __restrict__ dout, const float* __restrict__ pre, int b,
                                           int co, int y, int x, int Cout, int H, int W, int mode, int r) {
  if (mode == 0) return dout[(((size_t)b * Cout + co) * H + y) * W + x];
  return dout[ps_index(b, co, y, x, Cout, H, W, r)] * dgelu_f(pre[(((size_t)b * Cout + co) * H + y) * W + x]);
}

// ---- input gradient: one thread per (b, ci, y, x) ------------------------------------------------
__global__ __launch_bounds__(256) void conv3x3_bwd_data_kernel(const float* __restrict__ dout,
                                                               const float* __restrict__ pre,
                                                               const float* __restrict__ wgt, float* __restrict__ din,
                                                               int B, int Cin, int Cout, int H, int W, int mode,
                                                               int r) {
  const int64_t n = (int64_t)B * Cin * H * W;
  O2_GRID_STRIDE(e, n) {
    int64_t q = e;
    const int x = (int)(q % W); q /= W;
    const int y = (int)(q % H); q /= H;
    const int ci = (int)(q % Cin);
    const int b = (int)(q / Cin);
    float acc = 0.f;
    for (int co = 0; co < Cout; ++co) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int yy = y + 1 - k / 3, xx = x + 1 - k % 3;  // output pixel that saw (y,x) through tap k
        if (yy >= 0 && yy < H && xx >= 0 && xx < W)
          acc = fmaf(conv_dpre(dout, pre, b, co, yy, xx, Cout, H, W, mode, r), wgt[((size_t)co * Cin + ci) * 9 + k],
                     acc);
      }
    }
    din[e] = acc;
  }
}

// ---- weight / bias gradient: 16x16 pixel tile per block, one thread per (co, ci, tap) entry -------
// Every block stores its Cout*Cin*9 + Cout partial sums in its own slab of `ws`; o2_sum_parts adds the slabs in a fixed
// order (round 4: the fp32 atomics this replaced made the step's last digits differ from run to run).
constexpr int TW = 16, TH = 16;
__global__ __launch_bounds__(256) void conv3x3_bwd_weight_kernel(const float* __restrict__ dout,
                                                                 const float* __restrict__ pre,
                                                                 const float* __restrict__ in,
                                                                 const int* __restrict__ cidx, int in_ctotal,
                                                                 float* __restrict__ ws,
                                                                 int B, int Cin, int Cout, int H, int W, int mode,
                                                                 int r) {
  float* dw = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ((size_t)Cout * Cin * 9 + Cout);
  float* dbias = dw + (size_t)Cout * Cin * 9;
  __shared__ float sd[COB][TH][TW];
  __shared__ float si[CONV_MAXCIN][TH + 2][TW + 2];
  const int tiles_x = (W + TW - 1) / TW;
  const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int b = blockIdx.y;
  for (int e = threadIdx.x; e < Cin * (TH + 2) * (TW + 2); e += 256) {
    const int ci = e / ((TH + 2) * (TW + 2));
    const int rem = e - ci * (TH + 2) * (TW + 2);
    const int yy = ty0 + rem / (TW + 2) - 1, xx = tx0 + rem % (TW + 2) - 1;
    const int cs = cidx ? cidx[ci] : ci;
    si[ci][rem / (TW + 2)][rem % (TW + 2)] =
        (yy >= 0 && yy < H && xx >= 0 && xx < W) ? in[(((size_t)b * in_ctotal + cs) * H + yy) * W + xx] : 0.f;
  }
  for (int co0 = 0; co0 < Cout; co0 += COB) {
    const int nco = (Cout - co0) < COB ? (Cout - co0) : COB;
    __syncthreads();
    for (int e = threadIdx.x; e < nco * TH * TW; e += 256) {
      const int co = e / (TH * TW);
      const int rem = e - co * TH * TW;
      const int y = ty0 + rem / TW, x = tx0 + rem % TW;
      sd[co][rem / TW][rem % TW] =
          (y < H && x < W) ? conv_dpre(dout, pre, b, co0 + co, y, x, Cout, H, W, mode, r) : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nco * Cin * 9; e += 256) {
      const int co = e / (Cin * 9);
      const int rem = e - co * Cin * 9;
      const int ci = rem / 9, k = rem - ci * 9;
      const int ky = k / 3, kx = k - ky * 3;
      float s = 0.f;
      for (int y = 0; y < TH; ++y)
#pragma unroll
        for (int x = 0; x < TW; ++x) s = fmaf(sd[co][y][x], si[ci][y + ky][x + kx], s);
      dw[((size_t)(co0 + co) * Cin + ci) * 9 + k] = s;
    }
    for (int co = threadIdx.x; co < nco; co += 256) {
      float s = 0.f;
      for (int y = 0; y < TH; ++y)
        for (int x = 0; x < TW; ++x) s += sd[co][y][x];
      dbias[co0 + co] = s;
    }
  }
}

__global__ __launch_bounds__(256) void clamp_channel_kernel(float* __restrict__ img, const float* __restrict__ ref,
                                                            float* __restrict__ dimg, int B, int C, int HW,
                                                            int chan) {
  const int64_t n = (int64_t)B * HW;
  O2_GRID_STRIDE(e, n) {
    const int b = (int)(e / HW);
    const size_t off = ((size_t)b * C + chan) * HW + (e - (int64_t)b * HW);
    if (dimg) { if (!(ref[off] > 0.f)) dimg[off] = 0.f; }
    else img[off] = fmaxf(img[off], 0.f);
  }
}

// ---- position-embedding table of a step: bicubic re-grid + resolution embedding --------------------------------------------
// out[(oy nw + ox)][:] = bicubic(pe)[oy][ox][:] + sw[:] * res + sb[:]
// (components/pos_embed.py:103-138 interpolate_pos_embed_on_the_fly: the [1, L0, D] table seen as a channel-last [oh][ow][D] grid,
// F.interpolate(mode="bicubic", align_corners=False) to [nh][nw], only when the heights differ; res_slimvit.py:277-281: + the
// Linear(1, D) spatial embedding of the scalar resolution.)  fp32 throughout, the table is a parameter.
// Bicubic as ATen defines it: source coordinate s = (in / out) (o + 0.5) - 0.5 (not clamped), base = floor(s), t = s - base, taps
// base - 1 .. base + 2 with indices clamped to the grid, cubic-convolution weights with A = -0.75; a pixel = the four row
// interpolants (left to right) combined top to bottom.  Channel-last, so a pixel's D values are contiguous: one workgroup per
// pixel, lanes over D in float4.
constexpr int PE_MAX_SIDE = 2048;

// acc += v * w per component: products and sums the compiler may fuse (the golden files hold what it does)
__device__ __forceinline__ void axpy4(float4& acc, const float4 v, float w) {
  acc.x += v.x * w; acc.y += v.y * w; acc.z += v.z * w; acc.w += v.w * w;
}

__device__ __forceinline__ void cubic_taps(int o, int n_in, int n_out, int idx[4], float w[4]) {
  const float scale = (float)n_in / (float)n_out;
  const float s = scale * ((float)o + 0.5f) - 0.5f;
  const float fl = floorf(s);
  const float t = s - fl;
  const int base = (int)fl;
  constexpr float A = -0.75f;
  const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
  w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int i = base - 1 + k;
    idx[k] = i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i);
  }
}

template <bool SAME>
__global__ __launch_bounds__(256) void posembed_fwd_kernel(const float* __restrict__ pe, const float* __restrict__ sw,
                                                           const float* __restrict__ sb, float res, float* __restrict__ out,
                                                           int oh, int ow, int nh, int nw, int D) {
  const int pix = blockIdx.x, oy = pix / nw, ox = pix - oy * nw;
  int iy[4], ix[4];
  float wy[4], wx[4];
  if (!SAME) {
    cubic_taps(oy, oh, nh, iy, wy);
    cubic_taps(ox, ow, nw, ix, wx);
  }
  float* o = out + (size_t)pix * D;
  for (int d = threadIdx.x * 4; d < D; d += 256 * 4) {
    float4 acc;
    if (SAME) {
      acc = *reinterpret_cast<const float4*>(pe + (size_t)pix * D + d);
    } else {
      acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float* row = pe + ((size_t)iy[a] * ow) * D + d;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float4 v = *reinterpret_cast<const float4*>(row + (size_t)ix[b] * D);
          axpy4(r, v, wx[b]);
        }
        axpy4(acc, r, wy[a]);
      }
    }
    if (sw) {
      const float4 w4 = *reinterpret_cast<const float4*>(sw + d), b4 = *reinterpret_cast<const float4*>(sb + d);
      acc.x += w4.x * res + b4.x; acc.y += w4.y * res + b4.y; acc.z += w4.z * res + b4.z; acc.w += w4.w * res + b4.w;
    }
    *reinterpret_cast<float4*>(o + d) = acc;
  }
}

// tab[o] = the weight output row / column o gives source row / column src (dense over n_out, mostly zero)
__device__ __forceinline__ void source_weights(float* tab, int src, int n_in, int n_out) {
  for (int o = threadIdx.x; o < n_out; o += 256) {
    int idx[4];
    float w[4], s = 0.f;
    cubic_taps(o, n_in, n_out, idx, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (idx[k] == src) ? w[k] : 0.f;
    tab[o] = s;
  }
}

// transpose of the re-grid: dpe[iy][ix][:] = sum_{oy, ox} Wy[oy][iy] Wx[ox][ix] dout[oy][ox][:].  One workgroup per SOURCE pixel:
// it first tabulates, in LDS, the weight every output row / column gives this source row / column (dense over nh / nw, mostly
// zero: a source row feeds ~4 in/out ... 4 out/in output rows, more at a clamped border), then walks the non-zero pairs in
// ascending (oy, ox) order -- a fixed summation order, no atomics (the same bits on every run and every rank).
__global__ __launch_bounds__(256) void posembed_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dpe, int oh, int ow,
                                                           int nh, int nw, int D) {
  __shared__ float wyd[PE_MAX_SIDE], wxd[PE_MAX_SIDE];
  const int pix = blockIdx.x, sy = pix / ow, sx = pix - sy * ow;
  source_weights(wyd, sy, oh, nh);
  source_weights(wxd, sx, ow, nw);
  __syncthreads();
  for (int d = threadIdx.x * 4; d < D; d += 256 * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = 0; oy < nh; ++oy) {
      const float wy = wyd[oy];
      if (wy == 0.f) continue;
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int ox = 0; ox < nw; ++ox) {
        const float wx = wxd[ox];
        if (wx == 0.f) continue;
        const float4 v = *reinterpret_cast<const float4*>(dout + ((size_t)oy * nw + ox) * D + d);
        axpy4(r, v, wx);
      }
      axpy4(acc, r, wy);
    }
    *reinterpret_cast<float4*>(dpe + (size_t)pix * D + d) = acc;
  }
}

// ---- host: the checks and launches that several entries share.  The three unpatchify entries: check, count, launch
template <bool BWD, bool T_FP32>
int unpatchify_launch(const void* t, const float* img, int B, int C, int h, int w, int p, int s, void* stream) {
  if (!t || !img || B <= 0 || C <= 0 || p <= 0 || s <= 0 || (h * s) % p || (w * s) % p) return O2_ERR_ARG;
  hipLaunchKernelGGL((unpatchify_kernel<BWD, T_FP32>), dim3(img_grid((int64_t)B * C * h * s * w * s)), dim3(256), 0,
                     (hipStream_t)stream, (bf16_t*)t, (float*)img, B, C, h * s, w * s, p);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

// what both conv entries require of mode / r / Cout (mode 1 = GELU + PixelShuffle(r), which keeps `pre`)
inline bool conv_shape_ok(int mode, int r, int Cout, const float* pre) {
  return mode == 0 || (mode == 1 && pre && r > 0 && Cout % (r * r) == 0);
}

// forward (img, in place) or backward (ref = the clamped image, dimg): the entry has checked its pointers
int clamp_launch(float* img, const float* ref, float* dimg, int B, int C, int HW, int chan, void* stream) {
  if (B <= 0 || C <= 0 || HW <= 0 || chan < 0 || chan >= C) return O2_ERR_ARG;
  hipLaunchKernelGGL(clamp_channel_kernel, dim3(img_grid((int64_t)B * HW)), dim3(256), 0, (hipStream_t)stream, img, ref, dimg,
                     B, C, HW, chan);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

// O2_OK, or the code both entries return: the reference re-grids only when the HEIGHTS differ (pos_embed.py:117), other widths alone are an error
inline int posembed_dims_ok(int oh, int ow, int nh, int nw, int D) {
  if (oh <= 0 || ow <= 0 || nh <= 0 || nw <= 0 || D <= 0 || (D & 3)) return O2_ERR_ARG;
  if (nh > PE_MAX_SIDE || nw > PE_MAX_SIDE || oh > PE_MAX_SIDE || ow > PE_MAX_SIDE) return O2_ERR_UNSUPPORTED;
  return (oh == nh && ow != nw) ? O2_ERR_ARG : O2_OK;
}
}  // namespace

extern "C" int orbit2_unpatchify_fwd(const void* t, float* img, int B, int C, int h, int w, int p, int s, void* stream) {
  return unpatchify_launch<false, false>(t, img, B, C, h, w, p, s, stream);
}
extern "C" int orbit2_unpatchify_fwd_f32(const float* t, float* img, int B, int C, int h, int w, int p, int s, void* stream) {
  return unpatchify_launch<false, true>(t, img, B, C, h, w, p, s, stream);
}
extern "C" int orbit2_unpatchify_bwd(const float* dimg, void* dt, int B, int C, int h, int w, int p, int s, void* stream) {
  return unpatchify_launch<true, false>(dt, dimg, B, C, h, w, p, s, stream);
}

extern "C" int orbit2_conv3x3_fwd(const float* in, const int* chan_idx, int in_ctotal, const float* weight,
                                  const float* bias, float* out, float* pre, const float* addend, int Ha, int Wa,
                                  int B, int Cin, int Cout, int H, int W, int mode, int r, void* stream) {
  if (!in || !weight || !bias || !out || B <= 0 || Cin <= 0 || Cin > CONV_MAXCIN || Cout <= 0 || H <= 0 || W <= 0)
    return O2_ERR_ARG;
  if (!conv_shape_ok(mode, r, Cout, pre)) return O2_ERR_ARG;
  if (addend && (mode != 0 || Ha < H || Wa < W)) return O2_ERR_ARG;
  dim3 grid(img_grid((int64_t)B * H * W), (Cout + COB - 1) / COB);
  hipLaunchKernelGGL(conv3x3_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, chan_idx, in_ctotal, weight,
                     bias, out, pre, addend, Ha, Wa, B, Cin, Cout, H, W, mode, r);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int64_t orbit2_conv3x3_bwd_ws_floats(int B, int Cin, int Cout, int H, int W) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)B * ((W + TW - 1) / TW) * ((H + TH - 1) / TH) * ((int64_t)Cout * Cin * 9 + Cout);
}

extern "C" int orbit2_conv3x3_bwd(const float* dout, const float* in, const int* chan_idx, int in_ctotal,
                                  const float* weight, const float* pre, float* din, float* dweight, float* dbias,
                                  int B, int Cin, int Cout, int H, int W, int mode, int r, float* ws, void* stream) {
  if (!dout || !in || !weight || !dweight || !dbias || !ws || B <= 0 || Cin <= 0 || Cin > CONV_MAXCIN || Cout <= 0)
    return O2_ERR_ARG;
  if (!conv_shape_ok(mode, r, Cout, pre)) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (din) {
    hipLaunchKernelGGL(conv3x3_bwd_data_kernel, dim3(img_grid((int64_t)B * Cin * H * W)), dim3(256), 0, s, dout,
                       pre, weight, din, B, Cin, Cout, H, W, mode, r);
    O2_CHECK_LAUNCH();
  }
  dim3 grid(((W + TW - 1) / TW) * ((H + TH - 1) / TH), B);
  hipLaunchKernelGGL(conv3x3_bwd_weight_kernel, grid, dim3(256), 0, s, dout, pre, in, chan_idx, in_ctotal, ws,
                     B, Cin, Cout, H, W, mode, r);
  const int nparts = (int)(grid.x * grid.y);
  const int64_t nw = (int64_t)Cout * Cin * 9, slab = nw + Cout;
  o2_sum_parts(ws, nparts, slab, dweight, nw, 1.0f, 1, s);          // dweight / dbias += (as the atomics did)
  o2_sum_parts(ws + nw, nparts, slab, dbias, Cout, 1.0f, 1, s);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_clamp_channel(float* img, int B, int C, int HW, int chan, void* stream) {
  return img ? clamp_launch(img, nullptr, nullptr, B, C, HW, chan, stream) : O2_ERR_ARG;
}
extern "C" int orbit2_clamp_channel_bwd(const float* img_clamped, float* dimg, int B, int C, int HW, int chan, void* stream) {
  return img_clamped && dimg ? clamp_launch(nullptr, img_clamped, dimg, B, C, HW, chan, stream) : O2_ERR_ARG;
}

extern "C" int orbit2_posembed_fwd(const float* pe, const float* sw, const float* sb, float res, float* out, int oh, int ow,
                                   int nh, int nw, int D, void* stream) {
  if (!pe || !out || (sw == nullptr) != (sb == nullptr)) return O2_ERR_ARG;
  if (const int rc = posembed_dims_ok(oh, ow, nh, nw, D)) return rc;
  o2_with_flags([&](auto same) {
    hipLaunchKernelGGL((posembed_fwd_kernel<decltype(same)::value>), dim3(nh * nw), dim3(256), 0, (hipStream_t)stream, pe, sw, sb,
                       res, out, oh, ow, nh, nw, D);
  }, oh == nh);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_posembed_bwd(const float* dout, float* dpe, int oh, int ow, int nh, int nw, int D, void* stream) {
  if (!dout || !dpe) return O2_ERR_ARG;
  if (const int rc = posembed_dims_ok(oh, ow, nh, nw, D)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (oh == nh) {
    if (hipMemcpyAsync(dpe, dout, sizeof(float) * (size_t)nh * nw * D, hipMemcpyDeviceToDevice, s) != hipSuccess) return O2_ERR_LAUNCH;
    return O2_OK;
  }
  hipLaunchKernelGGL(posembed_bwd_kernel, dim3(oh * ow), dim3(256), 0, s, dout, dpe, oh, ow, nh, nw, D);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
