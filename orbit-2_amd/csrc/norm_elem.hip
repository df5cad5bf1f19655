// LayerNorm fwd/bwd + HBM-bound elementwise / reduction kernels (bf16 rows, 16-byte accesses).
#include "common.h"
#include "../../include/orbit2_hip.h"

namespace {

constexpr int LN_MAXD = 8192;  // up to 16 16-byte chunks per lane

// one wave per row; 4 rows per 256-thread block; NC = 16-byte chunks per lane (compile time)
template <int NC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ gamma,
                                                     const bf16_t* __restrict__ beta, bf16_t* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int rows,
                                                     int D, float eps, int ldy) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nch = D >> 3;
  const bf16_t* xr = x + (size_t)row * D;
  float v[NC][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
      unpack8(*reinterpret_cast<const u32x4*>(xr + ch * 8), v[c]);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[c][j];
    }
  }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[c][j] - mu; q += d * d; }
    }
  }
  const float rs = rsqrtf(wave_sum(q) / (float)D + eps);
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  bf16_t* yr = y + (size_t)row * ldy;      // ldy: row pitch of y (>= D)
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
      float g[8], b[8];
      unpack8(*reinterpret_cast<const u32x4*>(gamma + ch * 8), g);
      unpack8(*reinterpret_cast<const u32x4*>(beta + ch * 8), b);
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = pack_bf2((v[c][2 * j] - mu) * rs * g[2 * j] + b[2 * j],
                        (v[c][2 * j + 1] - mu) * rs * g[2 * j + 1] + b[2 * j + 1]);
      *reinterpret_cast<u32x4*>(yr + ch * 8) = o;
    }
  }
}

// fp32 twin of ln_fwd_kernel (the fp32 forward path): one wave per row, NC float4 chunks per lane, two-pass variance from the
// register-resident row; mean / rstd optional
template <int NC>
__global__ __launch_bounds__(256) void ln_fwd_f32_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ y,
                                                         float* __restrict__ mean, float* __restrict__ rstd, int rows,
                                                         int D, float eps, int ldy) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nch = D >> 2;
  const float* xr = x + (size_t)row * D;
  f32x4 v[NC];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
      v[c] = *reinterpret_cast<const f32x4*>(xr + ch * 4);
      s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
  }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = v[c][j] - mu; q = fmaf(d, d, q); }
    }
  }
  const float rs = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
  float* yr = y + (size_t)row * ldy;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = lane + c * 64;
    if (ch < nch) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + ch * 4);
      const f32x4 b = *reinterpret_cast<const f32x4*>(beta + ch * 4);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = fmaf((v[c][j] - mu) * rs, g[j], b[j]);
      *reinterpret_cast<f32x4*>(yr + ch * 4) = o;
    }
  }
}

// Each wave walks LN_RPW consecutive rows (two passes per row: statistics, then dx from the L1/L2-hot
// lines) and keeps its dgamma/dbeta partial sums in registers; one partial row per block (D % 4 == 0).
constexpr int LN_RPW = 16;
#ifndef O2_LN_FMA
#define O2_LN_FMA 1      // row-shared backward: the fused-multiply-add form of xhat and of dx (0: the expressions of rounds 2-5, A/B builds)
#endif
template <int NC>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                     const bf16_t* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const bf16_t* __restrict__ dres,
                                                     bf16_t* __restrict__ dx, float* __restrict__ part, int rows,
                                                     int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = D >> 3;
  const int pw = blockIdx.x * 4 + wave;
  float dg[NC][8], db[NC][8];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) { dg[c][j] = 0.f; db[c][j] = 0.f; }
  // gamma is row-invariant: unpacked once per wave would cost 48 VGPRs; it stays packed (6 x 16 B per lane)
  u32x4 gp[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = lane + c * 64;
    gp[c] = ch < nch ? *reinterpret_cast<const u32x4*>(gamma + ch * 8) : (u32x4){0u, 0u, 0u, 0u};
  }
  for (int rr = 0; rr < LN_RPW; ++rr) {
    const int row = pw * LN_RPW + rr;
    if (row >= rows) break;
    const float mu = mean[row], rs = rstd[row];
    const bf16_t* xr = x + (size_t)row * D;
    const bf16_t* dyr = dy + (size_t)row * D;
    // every global load of the row is issued here, up front (x, dy and the residual-stream gradient), and the row
    // stays PACKED in registers between the statistics pass and the dx pass: one HBM round trip per row instead
    // of a second trip through L1/L2 plus a late dres fetch
    u32x4 xp[NC], dp[NC], rp[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int ch = lane + c * 64;
      if (ch < nch) {
        xp[c] = *reinterpret_cast<const u32x4*>(xr + ch * 8);
        dp[c] = *reinterpret_cast<const u32x4*>(dyr + ch * 8);
        if (dres) rp[c] = *reinterpret_cast<const u32x4*>(dres + (size_t)row * D + ch * 8);
      }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int ch = lane + c * 64;
      if (ch < nch) {
        float xv[8], dv[8], gv[8];
        unpack8(xp[c], xv);
        unpack8(dp[c], dv);
        unpack8(gp[c], gv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xhat = (xv[j] - mu) * rs;
          const float g = dv[j] * gv[j];
          s1 += g; s2 += g * xhat;
          dg[c][j] += dv[j] * xhat; db[c][j] += dv[j];
        }
      }
    }
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
    bf16_t* dxr = dx + (size_t)row * D;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int ch = lane + c * 64;
      if (ch < nch) {
        float xv[8], dv[8], gv[8], o[8];
        unpack8(xp[c], xv);
        unpack8(dp[c], dv);
        unpack8(gp[c], gv);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = rs * (dv[j] * gv[j] - s1 - (xv[j] - mu) * rs * s2);
        if (dres) {
          float rv[8];
          unpack8(rp[c], rv);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += rv[j];
        }
        *reinterpret_cast<u32x4*>(dxr + ch * 8) = pack8(o);
      }
    }
  }
  // the four waves' partial sums are combined in LDS (wave 0 stores, waves 1..3 add in turn): one partial row per
  // block instead of four -> the reduce kernel reads a quarter of the data
  extern __shared__ float ln_red[];            // [2][D]
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nch) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float* a = ln_red + ch * 8 + j;
            float* b = ln_red + D + ch * 8 + j;
            *a = (w ? *a : 0.f) + dg[c][j];
            *b = (w ? *b : 0.f) + db[c][j];
          }
        }
      }
    }
    __syncthreads();
  }
  float* pout = part + (size_t)blockIdx.x * 2 * D;
  for (int e = threadIdx.x * 4; e < 2 * D; e += 256 * 4)
    *reinterpret_cast<f32x4*>(pout + e) = *reinterpret_cast<const f32x4*>(ln_red + e);
}

// Row-shared form.  Wide rows (D > 4096, interm_10b: D = 8192): the per-wave form above would keep 2 x 8 x 16 gradient
// accumulators plus the packed row in registers and spill.  Here the TPB/64 waves of the block share every row, each
// thread owning the chunks tid, tid + TPB, ..: a quarter of the accumulators per thread, one LDS exchange + barrier per row for the two
// row statistics (double-buffered slots), the next row's loads issued before that barrier, and the block's partial
// dgamma / dbeta row written straight from registers (the waves own disjoint columns).
// EXACT: D == 8 NCW TPB -- no chunk is ever out of range, so no lane is ever masked off: without the tests the loop loses its
// exec-mask bookkeeping (19 s_and_saveexec + 20 s_or + the copies that merge the masked paths)
template <int NCW, int TPB = 256, int RPB = 4 * LN_RPW, bool EXACT = false>
__global__ __launch_bounds__(TPB) void ln_bwd_wide_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                          const bf16_t* __restrict__ gamma,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd,
                                                          const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx,
                                                          float* __restrict__ part, int rows, int D) {
  __shared__ float red[2][TPB / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = D >> 3;
  const int row0 = blockIdx.x * RPB;
  const int nrow = (rows - row0) < RPB ? (rows - row0) : RPB;
  float dg[NCW][8], db[NCW][8];
  u32x4 gp[NCW];
#pragma unroll
  for (int c = 0; c < NCW; ++c) {
    const int ch = tid + c * TPB;
    gp[c] = (EXACT || ch < nch) ? *reinterpret_cast<const u32x4*>(gamma + ch * 8) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) { dg[c][j] = 0.f; db[c][j] = 0.f; }
  }
  u32x4 xp[NCW], dp[NCW], rp[NCW], xn[NCW], dn[NCW], rn[NCW];
  auto load_row = [&](int row, u32x4* xo, u32x4* dyo, u32x4* ro) {
#pragma unroll
    for (int c = 0; c < NCW; ++c) {
      const int ch = tid + c * TPB;
      if (EXACT || ch < nch) {
        xo[c] = *reinterpret_cast<const u32x4*>(x + (size_t)row * D + ch * 8);
        dyo[c] = *reinterpret_cast<const u32x4*>(dy + (size_t)row * D + ch * 8);
        if (dres) ro[c] = *reinterpret_cast<const u32x4*>(dres + (size_t)row * D + ch * 8);
      }
    }
  };
  if (nrow > 0) load_row(row0, xp, dp, rp);
  for (int rr = 0; rr < nrow; ++rr) {
    const int row = row0 + rr;
    const float mu = mean[row], rs = rstd[row];
    const float nmurs = -mu * rs;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NCW; ++c) {
      if (EXACT || tid + c * TPB < nch) {
        float xv[8], dv[8], gv[8];
        unpack8(xp[c], xv); unpack8(dp[c], dv); unpack8(gp[c], gv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xhat = O2_LN_FMA ? fmaf(xv[j], rs, nmurs) : (xv[j] - mu) * rs;     // (x - mu) rs as ONE fma
          const float g = dv[j] * gv[j];
          s1 += g; s2 += g * xhat;
          dg[c][j] += dv[j] * xhat; db[c][j] += dv[j];
        }
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) { red[rr & 1][wave][0] = s1; red[rr & 1][wave][1] = s2; }
    if (rr + 1 < nrow) load_row(row + 1, xn, dn, rn);      // in flight across the barrier
    __syncthreads();
    s1 = 0.f; s2 = 0.f;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) { s1 += red[rr & 1][w][0]; s2 += red[rr & 1][w][1]; }
    s1 /= (float)D; s2 /= (float)D;
    // dx = rs (dy g - s1 - xhat s2) = dy (g rs) + x c2 + c0 with the row's c2 = -rs^2 s2, c0 = rs (mu rs s2 - s1): three
    // instructions per element (one multiply, two fused multiply-adds) instead of seven -- the kernel is co-limited by vector issue
    const float c2 = -rs * rs * s2, c0 = rs * (mu * rs * s2 - s1);
#pragma unroll
    for (int c = 0; c < NCW; ++c) {
      const int ch = tid + c * TPB;
      if (EXACT || ch < nch) {
        float xv[8], dv[8], gv[8], o[8];
        unpack8(xp[c], xv); unpack8(dp[c], dv); unpack8(gp[c], gv);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = O2_LN_FMA ? fmaf(xv[j], c2, fmaf(dv[j], gv[j] * rs, c0)) : rs * (dv[j] * gv[j] - s1 - (xv[j] - mu) * rs * s2);
        if (dres) {
          float rv[8];
          unpack8(rp[c], rv);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += rv[j];
        }
        *reinterpret_cast<u32x4*>(dx + (size_t)row * D + ch * 8) = pack8(o);
      }
    }
#pragma unroll
    for (int c = 0; c < NCW; ++c) { xp[c] = xn[c]; dp[c] = dn[c]; rp[c] = rn[c]; }
  }
  float* pout = part + (size_t)blockIdx.x * 2 * D;
#pragma unroll
  for (int c = 0; c < NCW; ++c) {
    const int ch = tid + c * TPB;
    if (EXACT || ch < nch) {
      *reinterpret_cast<f32x4*>(pout + ch * 8) = (f32x4){dg[c][0], dg[c][1], dg[c][2], dg[c][3]};
      *reinterpret_cast<f32x4*>(pout + ch * 8 + 4) = (f32x4){dg[c][4], dg[c][5], dg[c][6], dg[c][7]};
      *reinterpret_cast<f32x4*>(pout + D + ch * 8) = (f32x4){db[c][0], db[c][1], db[c][2], db[c][3]};
      *reinterpret_cast<f32x4*>(pout + D + ch * 8 + 4) = (f32x4){db[c][4], db[c][5], db[c][6], db[c][7]};
    }
  }
}

// ---- what the two-stage sums of this file share (LayerNorm dgamma / dbeta, the column sums, batch_sum) -----------------
// stage 2, one of the eight row-lanes ty of a block: the sum of src[p * step] over p = ty, ty + 8, .. < n.
// eight partial rows in flight per thread (one dependent add chain per row kept the launch at 0.5 TB/s: 100 us for
// 50 MB at the interm_1b shape); fixed order: the eight chains, then their tree
template <class S>
__device__ __forceinline__ float sum_parts8(const float* src, S step, int n, int ty) {
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int p = ty;
  for (; p + 56 < n; p += 64) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += src[(size_t)(p + 8 * k) * step];
  }
  for (int k = 0; p < n; p += 8, ++k) a[k] += src[(size_t)p * step];
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}
// dst[i] = t + beta * dst[i] into an fp32 or a bf16 sink (beta = 0: dst is not read)
template <class I>
__device__ __forceinline__ void store_beta(void* dst, int fp32, I i, float t, float beta) {
  if (fp32) {
    float* o = (float*)dst + i;
    *o = t + (beta != 0.f ? beta * *o : 0.f);
  } else {
    bf16_t* o = (bf16_t*)dst + i;
    *o = f2bf(t + (beta != 0.f ? beta * bf2f(*o) : 0.f));
  }
}

// out[which][col] = beta*out + sum_p part[p][which][col]; 32 columns x 8 partial-groups per block
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ part, int nblk, int D,
                                                            void* dgamma, void* dbeta, int fp32, float beta) {
  __shared__ float red[8][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + tx;          // flat (which, col) index in [0, 2D)
  float s = 0.f;
  if (e < 2 * D) {
    const int which = e / D, col = e - which * D;
    s = sum_parts8(part + (size_t)which * D + col, (size_t)2 * D, nblk, ty);
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && e < 2 * D) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][tx];
    const int which = e / D, col = e - which * D;
    store_beta(which ? dbeta : dgamma, fp32, col, t, beta);
  }
}

// ---- what a GEMM epilogue does AFTER a cross-rank reduction of partial products -----------
// y = residual + rowscale[m / rps] * dropout(x + addend[m % res_mod])   (every term optional; same mask hash and
// order of operations as gemm.hip's epilogue, so a tensor-parallel block equals the single-rank fused one)
__global__ __launch_bounds__(256) void post_reduce_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ addend,
                                                          int res_mod, const bf16_t* __restrict__ residual,
                                                          bf16_t* __restrict__ y, int M, int N, unsigned thr,
                                                          float dscale, uint64_t seed,
                                                          const float* __restrict__ rowscale, int rows_per_scale) {
  const int64_t nch = (int64_t)M * N / 8;
  for (int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x; ch < nch; ch += (int64_t)gridDim.x * 256) {
    const int64_t idx = ch * 8;
    const int m = (int)(idx / N);
    const int n = (int)(idx - (int64_t)m * N);
    float f[8], t[8];
    unpack8(*reinterpret_cast<const u32x4*>(x + idx), f);
    if (addend) {
      const int rm = res_mod > 0 ? (m % res_mod) : m;
      unpack8(*reinterpret_cast<const u32x4*>(addend + (size_t)rm * N + n), t);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += t[j];
    }
    if (thr) o2_drop8(f, seed ^ o2_seed_salt, idx, thr, dscale);
    if (rowscale) {
      const float s = rowscale[m / rows_per_scale];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] *= s;
    }
    if (residual) {
      unpack8(*reinterpret_cast<const u32x4*>(residual + idx), t);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += t[j];
    }
    *reinterpret_cast<u32x4*>(y + idx) = pack8(f);
  }
}

// ---- dropout backward ---------------------------------------------------------------------
// dym = rowscale[m / rows_per_scale] * dropout(dy) on the eight values of row m from flat index idx (both optional), stored and
// returned as packed: the one row transform of dropout_bwd_kernel and of its twin with the fused column sums
__device__ __forceinline__ u32x4 dropout_bwd8(const bf16_t* __restrict__ dy, bf16_t* __restrict__ dym, int64_t idx, int m,
                                              unsigned thr, float dscale, uint64_t seed,
                                              const float* __restrict__ rowscale, int rows_per_scale) {
  float f[8];
  unpack8(*reinterpret_cast<const u32x4*>(dy + idx), f);
  if (thr) o2_drop8(f, seed ^ o2_seed_salt, idx, thr, dscale);
  if (rowscale) {
    const float s = rowscale[m / rows_per_scale];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= s;
  }
  const u32x4 o = pack8(f);
  *reinterpret_cast<u32x4*>(dym + idx) = o;
  return o;
}
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ dym,
                                                          int M, int N, unsigned thr, float dscale, uint64_t seed,
                                                          const float* __restrict__ rowscale, int rows_per_scale) {
  const int64_t nch = (int64_t)M * N / 8;
  for (int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x; ch < nch; ch += (int64_t)gridDim.x * 256) {
    const int64_t idx = ch * 8;
    dropout_bwd8(dy, dym, idx, (int)(idx / N), thr, dscale, seed, rowscale, rows_per_scale);
  }
}

// ---- column sums: stage 1 partials [P][N] (16-byte loads, 8 row-lanes per block), stage 2 reduce ----------
// rows per partial sum: 128 for the large problems; 32 when there are few rows (the 32 x 64-grid presets: 4096 rows x 1024 columns
// were 128 workgroups walking 16 rows each one after the other -- half the CUs, latency-bound; 512 workgroups of 4 rows now).
// One function decides for the workspace query and both launchers.
static inline int cs_rows(int M) { return M >= 32768 ? 128 : 32; }
// stage 1, the block's tail: the eight row-lanes' sums acc[8] of the columns c0 .. c0 + 7 go through LDS, row-lane 0 adds them in
// order 0 .. 7 and stores the block's partial sums.  Every thread of the block calls it (a barrier inside).
__device__ __forceinline__ void colsum_store_part(const float* acc, float* __restrict__ part, int N, int c0, int tx, int ty) {
  __shared__ float red[8][32][9];
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ty][tx][j] = acc[j];
  __syncthreads();
  if (ty == 0 && c0 < N) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) t += red[k][tx][j];
      part[(size_t)blockIdx.y * N + c0 + j] = t;
    }
  }
}
template <bool FP32>
__global__ __launch_bounds__(256) void colsum_part_kernel(const void* __restrict__ xv, int M, int N, int ldx,
                                                          float* __restrict__ part, int rpp) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = (blockIdx.x * 32 + tx) * 8;
  const int r0 = blockIdx.y * rpp;
  const int r1 = r0 + rpp < M ? r0 + rpp : M;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < N) {
    if (FP32) {
      const float* x = (const float*)xv;
      for (int r = r0 + ty; r < r1; r += 8) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + (size_t)r * ldx + c0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(x + (size_t)r * ldx + c0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[j] += a[j]; acc[4 + j] += b[j]; }
      }
    } else {
      const bf16_t* x = (const bf16_t*)xv;
      for (int r = r0 + ty; r < r1; r += 8) {
        float f[8];
        unpack8(*reinterpret_cast<const u32x4*>(x + (size_t)r * ldx + c0), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
      }
    }
  }
  colsum_store_part(acc, part, N, c0, tx, ty);
}
// dropout / DropPath backward FUSED with the column sums of its result (the bias gradient of the Linear whose output
// gradient this is): the same [128 rows x 256 columns] blocks, thread mapping and summation order as colsum_part_kernel, so
// the partials -- and the bias gradient -- are bit-identical to dropout_bwd + colsum, without re-reading dym from HBM.  The row
// transform (dropout_bwd8) and the block's tail (colsum_store_part) ARE the two kernels' code.
__global__ __launch_bounds__(256) void dropout_bwd_colsum_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ dym,
                                                                 int M, int N, unsigned thr, float dscale, uint64_t seed,
                                                                 const float* __restrict__ rowscale, int rows_per_scale,
                                                                 float* __restrict__ part, int rpp) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = (blockIdx.x * 32 + tx) * 8;
  const int r0 = blockIdx.y * rpp;
  const int r1 = r0 + rpp < M ? r0 + rpp : M;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < N) {
    for (int r = r0 + ty; r < r1; r += 8) {
      float f[8];
      // the sum is over the ROUNDED values (what colsum would read back)
      unpack8(dropout_bwd8(dy, dym, (int64_t)r * N + c0, r, thr, dscale, seed, rowscale, rows_per_scale), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  }
  colsum_store_part(acc, part, N, c0, tx, ty);
}
__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ part, int P, int N, void* out,
                                                            int out_fp32, float beta) {
  __shared__ float red[8][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + tx;
  float s = 0.f;
  if (col < N) s = sum_parts8(part + col, N, P, ty);
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && col < N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][tx];
    store_beta(out, out_fp32, col, t, beta);
  }
}

__global__ __launch_bounds__(256) void batch_sum_kernel(const bf16_t* __restrict__ x, void* out, int B, int64_t n,
                                                        int out_fp32, float beta) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += bf2f(x[(size_t)b * n + i]);
    store_beta(out, out_fp32, i, s, beta);
  }
}

__global__ __launch_bounds__(256) void cast_f2b_kernel(const float* __restrict__ s, bf16_t* __restrict__ d, int64_t n) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(s + i * 4);
    u32x2 o; o[0] = pack_bf2(v[0], v[1]); o[1] = pack_bf2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(d + i * 4) = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) d[n4 * 4 + threadIdx.x] = f2bf(s[n4 * 4 + threadIdx.x]);
}
__global__ __launch_bounds__(256) void cast_b2f_kernel(const bf16_t* __restrict__ s, float* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d[i] = bf2f(s[i]);
}
__global__ __launch_bounds__(256) void add_rowvec_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ vec,
                                                         bf16_t* __restrict__ y, int rows, int N) {
  const int64_t n = (int64_t)rows * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = f2bf(bf2f(a[i]) + bf2f(vec[i % N]));
}

// ---- bf16 matrix transpose through LDS: dst[C][R] = src[R][C]  (transposed compute copies of the weights so
//      that the input-gradient GEMM dX = dY . W runs in the K-contiguous form) ---------------------------------
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                             int R, int C) {
  __shared__ bf16_t tile[64][66];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < R && c < C) ? src[(size_t)r * C + c] : (bf16_t)0;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (c < C && r < R) dst[(size_t)c * R + r] = tile[tx][i];
  }
}

// ---- AdamW ---------------------------------------------------------------------------------
template <bool GFP32>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                    const void* __restrict__ gv, bf16_t* __restrict__ p16, int64_t n,
                                                    float lr, float b1, float b2, float eps, float wd, float bc1,
                                                    float rsbc2, float gs, const float* __restrict__ found_inf) {
  if (found_inf && *found_inf != 0.f) return;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 1024) {
    float g[4], pp[4], mm[4], vv[4];
    const int cnt = (n - i) >= 4 ? 4 : (int)(n - i);
    if (cnt == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + i), b = *reinterpret_cast<const f32x4*>(m + i),
                  c = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) { pp[j] = a[j]; mm[j] = b[j]; vv[j] = c[j]; }
      if (GFP32) {
        const f32x4 gg = *reinterpret_cast<const f32x4*>((const float*)gv + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = gg[j];
      } else {
        const u32x2 gg = *reinterpret_cast<const u32x2*>((const bf16_t*)gv + i);
        g[0] = bf2f((bf16_t)(gg[0] & 0xffff)); g[1] = bf2f((bf16_t)(gg[0] >> 16));
        g[2] = bf2f((bf16_t)(gg[1] & 0xffff)); g[3] = bf2f((bf16_t)(gg[1] >> 16));
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        pp[j] = p[i + j]; mm[j] = m[i + j]; vv[j] = v[i + j];
        g[j] = GFP32 ? ((const float*)gv)[i + j] : bf2f(((const bf16_t*)gv)[i + j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        const float gj = g[j] * gs;
        pp[j] *= (1.f - lr * wd);
        mm[j] = b1 * mm[j] + (1.f - b1) * gj;
        vv[j] = b2 * vv[j] + (1.f - b2) * gj * gj;
        const float denom = sqrtf(vv[j]) * rsbc2 + eps;
        pp[j] -= (lr / bc1) * (mm[j] / denom);
      }
    }
    if (cnt == 4) {
      *reinterpret_cast<f32x4*>(p + i) = (f32x4){pp[0], pp[1], pp[2], pp[3]};
      *reinterpret_cast<f32x4*>(m + i) = (f32x4){mm[0], mm[1], mm[2], mm[3]};
      *reinterpret_cast<f32x4*>(v + i) = (f32x4){vv[0], vv[1], vv[2], vv[3]};
      if (p16) {
        u32x2 o; o[0] = pack_bf2(pp[0], pp[1]); o[1] = pack_bf2(pp[2], pp[3]);
        *reinterpret_cast<u32x2*>(p16 + i) = o;
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        p[i + j] = pp[j]; m[i + j] = mm[j]; v[i + j] = vv[j];
        if (p16) p16[i + j] = f2bf(pp[j]);
      }
    }
  }
}

template <bool GFP32>
__global__ __launch_bounds__(256) void check_finite_kernel(const void* __restrict__ gv, int64_t n, float* found) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float g = GFP32 ? ((const float*)gv)[i] : bf2f(((const bf16_t*)gv)[i]);
    bad |= !(fabsf(g) <= 3.0e38f);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) *found = 1.f;
}

// per-sample DropPath scales (timm DropPath semantics: Bernoulli(keep)/keep per sample), 32-bit threshold
__global__ void droppath_scales_kernel(float* __restrict__ out, int B, float p, uint64_t seed) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint32_t h = o2_hash64(seed ^ o2_seed_salt ^ 0xD1B54A32D192ED03ull, (uint64_t)b);
  const float u = (float)(h >> 8) * (1.0f / 16777216.0f);
  out[b] = (u >= p) ? 1.0f / (1.0f - p) : 0.f;
}

// the one-wave-per-row kernels (ln_fwd_kernel, ln_bwd_kernel) are compiled for 1, 2, 4, 6, 8 and 16 chunks per lane:
// ln_chunks(D) is the smallest of them that holds a row of D bf16, ln_with_chunks(nc, f) calls f(o2_int<nc>)
inline int ln_chunks(int D) {
  const int nc = (D / 8 + 63) / 64;
  return nc <= 1 ? 1 : nc <= 2 ? 2 : nc <= 4 ? 4 : nc <= 6 ? 6 : nc <= 8 ? 8 : 16;
}
template <class F> inline void ln_with_chunks(int nc, F&& f) {
  switch (nc) {
    case 1: f(o2_int<1>{}); break;
    case 2: f(o2_int<2>{}); break;
    case 4: f(o2_int<4>{}); break;
    case 6: f(o2_int<6>{}); break;
    case 8: f(o2_int<8>{}); break;
    default: f(o2_int<16>{});
  }
}

}  // namespace

extern "C" int orbit2_layernorm_fwd_ld(const void* x, const void* gamma, const void* beta, void* y, float* mean,
                                       float* rstd, int rows, int D, int ldy, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || !mean || !rstd || rows <= 0 || D <= 0 || (D & 7) || D > LN_MAXD || ldy < D || (ldy & 7))
    return O2_ERR_ARG;
  ln_with_chunks(ln_chunks(D), [&](auto NC) {
    hipLaunchKernelGGL(ln_fwd_kernel<NC>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)gamma, (const bf16_t*)beta, (bf16_t*)y, mean, rstd, rows, D, eps, ldy);
  });
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_layernorm_fwd_f32(const void* x, const void* gamma, const void* beta, void* y, float* mean,
                                        float* rstd, int rows, int D, int ldy, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || rows <= 0 || D <= 0 || (D & 3) || D > LN_MAXD || ldy < D || (ldy & 3)) return O2_ERR_ARG;
  const int nc = (D / 4 + 63) / 64;                                  // float4 chunks per lane: up to 32 at D = 8192
  auto call = [&](auto NC) {
    hipLaunchKernelGGL(ln_fwd_f32_kernel<NC>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)gamma, (const float*)beta, (float*)y, mean, rstd, rows, D, eps, ldy);
  };
  if (nc <= 2) call(o2_int<2>{}); else if (nc <= 4) call(o2_int<4>{}); else if (nc <= 8) call(o2_int<8>{}); else if (nc <= 16) call(o2_int<16>{}); else call(o2_int<32>{});
  O2_CHECK_LAUNCH();
  return O2_OK;
}

// ---- LayerNorm backward: which kernel on which partition.  ln_bwd_plan decides everything and launches nothing ------------
// few rows (the 32 x 64-grid presets): LN_FEW_RPB rows per workgroup of the row-shared form -- 4096 rows at 16 per workgroup were
// 256 workgroups of two waves walking their rows one global-load latency after the other (18 us at D = 1024, a quarter of it
// bandwidth); 4 per workgroup put four workgroups on every CU
constexpr int LN_FEW_RPB = 4;
constexpr int LN_WAVE_RPB = 4 * LN_RPW;      // the per-wave form: four waves of LN_RPW rows each
static inline int ln_shared_rpb(int rows) { return rows < 32768 ? LN_FEW_RPB : 64; }
static inline int ln_blocks(int rows, int rpb) { return (rows + rpb - 1) / rpb; }
struct LnBwdPlan {
  bool shared;       // ln_bwd_wide_kernel<nc, tpb, rpb, exact>; else ln_bwd_kernel<nc> (tpb = 256, rpb = LN_WAVE_RPB)
  int nc, tpb, rpb;  // 16-byte chunks per thread, threads and rows per block
  bool exact;        // D == 8 nc tpb: no chunk of the row-shared form is ever out of range
  int grid;          // blocks = partial dgamma / dbeta rows in the workspace (one per block)
  size_t lds;        // dynamic LDS (the per-wave form's [2][D] exchange)
};
static LnBwdPlan ln_bwd_plan(int rows, int D) {
  LnBwdPlan p = {};
  // row-shared form for the model widths (8m / 117m / 1b / 10b); 64 rows per block, LN_FEW_RPB when there are few rows (the
  // small grids: 4096 rows would otherwise occupy 64 CUs)
  if (D == 3072) { p.shared = true; p.nc = 3; p.tpb = 128; }          // 363 vs 414 us (per-wave form) at 65536 rows
  else if (D == 1024) { p.shared = true; p.nc = 1; p.tpb = 128; }
  else if (D == 256) { p.shared = true; p.nc = 1; p.tpb = 64; }
  else if (D > 4096) { p.shared = true; p.nc = 4; p.tpb = 256; }      // the per-wave form spills (1127 -> 115 us at D = 8192)
  if (p.shared) {
    p.rpb = ln_shared_rpb(rows);
    p.exact = D == 8 * p.nc * p.tpb;
  } else {                                                            // other widths: per-wave form, its partition
    p.nc = ln_chunks(D);
    p.tpb = 256;
    p.rpb = LN_WAVE_RPB;
    p.lds = 2 * D * sizeof(float);
  }
  p.grid = ln_blocks(rows, p.rpb);
  return p;
}
// The workspace holds 4 partial rows per 64 input rows, or the row-shared form's one per LN_FEW_RPB when that is more: enough
// for every form at these rows, whatever the width.
extern "C" int orbit2_layernorm_bwd_ws_floats(int rows, int D) {
  const int a = 4 * ln_blocks(rows, LN_WAVE_RPB), b = ln_blocks(rows, ln_shared_rpb(rows));
  return (a > b ? a : b) * 2 * D;
}

extern "C" int orbit2_layernorm_bwd(const void* dy, const void* x, const void* gamma, const float* mean,
                                    const float* rstd, const void* dres, void* dx, void* dgamma, void* dbeta,
                                    int grads_fp32, float beta_acc, float* ws, int ws_floats, int rows, int D,
                                    void* stream) {
  if (!dy || !x || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || !ws) return O2_ERR_ARG;
  if (rows <= 0 || (D & 7) || D > LN_MAXD) return O2_ERR_ARG;
  if (ws_floats < orbit2_layernorm_bwd_ws_floats(rows, D)) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const LnBwdPlan p = ln_bwd_plan(rows, D);
#define O2_LN_BWD_LAUNCH(KERN)                                                                                              \
  hipLaunchKernelGGL(KERN, dim3(p.grid), dim3(p.tpb), p.lds, s, (const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)gamma, mean, \
                     rstd, (const bf16_t*)dres, (bf16_t*)dx, ws, rows, D)
  auto shared = [&](auto NCW_, auto TPB_) {
    constexpr int NCW = NCW_, TPB = TPB_;
    o2_with_flags([&](auto FEW, auto EX) { O2_LN_BWD_LAUNCH((ln_bwd_wide_kernel<NCW, TPB, FEW ? LN_FEW_RPB : 64, EX>)); },
                  p.rpb == LN_FEW_RPB, p.exact);
  };
  if (!p.shared) ln_with_chunks(p.nc, [&](auto NC) { O2_LN_BWD_LAUNCH(ln_bwd_kernel<NC>); });
  else if (p.nc == 3) shared(o2_int<3>{}, o2_int<128>{});
  else if (p.nc == 4) shared(o2_int<4>{}, o2_int<256>{});
  else if (p.tpb == 128) shared(o2_int<1>{}, o2_int<128>{});
  else shared(o2_int<1>{}, o2_int<64>{});
#undef O2_LN_BWD_LAUNCH
  O2_CHECK_LAUNCH();
  hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((2 * D + 31) / 32), dim3(256), 0, s, ws, p.grid, D, dgamma, dbeta, grads_fp32,
                     beta_acc);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_dropout_bwd(const void* dy, void* dym, int M, int N, float drop_p, uint64_t seed,
                                  const float* rowscale, int rows_per_scale, void* stream) {
  if (!dy || !dym || M <= 0 || N <= 0 || (N & 7) || drop_p < 0.f || drop_p >= 1.f) return O2_ERR_ARG;
  if (rowscale && rows_per_scale <= 0) return O2_ERR_ARG;
  const unsigned thr = (unsigned)(drop_p * 256.0f + 0.5f);
  hipLaunchKernelGGL(dropout_bwd_kernel, dim3(grid_for((int64_t)M * N / 8, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)dy, (bf16_t*)dym, M, N, thr, 256.0f / (256.0f - (float)thr), seed, rowscale,
                     rows_per_scale);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_post_reduce(const void* x, const void* addend, int res_mod, const void* residual, void* y, int M,
                                  int N, float drop_p, uint64_t seed, const float* rowscale, int rows_per_scale,
                                  void* stream) {
  if (!x || !y || M <= 0 || N <= 0 || (N & 7) || drop_p < 0.f || drop_p >= 1.f || res_mod < 0) return O2_ERR_ARG;
  if (rowscale && rows_per_scale <= 0) return O2_ERR_ARG;
  const unsigned thr = (unsigned)(drop_p * 256.0f + 0.5f);
  hipLaunchKernelGGL(post_reduce_kernel, dim3(grid_for((int64_t)M * N / 8, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (const bf16_t*)addend, res_mod, (const bf16_t*)residual, (bf16_t*)y, M, N, thr,
                     256.0f / (256.0f - (float)thr), seed, rowscale, rows_per_scale);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_colsum_ws_floats(int M, int N) { return ((M + cs_rows(M) - 1) / cs_rows(M)) * N; }

extern "C" int orbit2_colsum(const void* x, int x_fp32, int M, int N, int ldx, void* out, int out_fp32, float beta,
                             float* ws, int ws_floats, void* stream) {
  if (!x || !out || !ws || M <= 0 || N <= 0) return O2_ERR_ARG;
  const int rpp = cs_rows(M), P = (M + rpp - 1) / rpp;
  if (ws_floats < P * N) return O2_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if ((N & 7) || (ldx & 7)) return O2_ERR_ARG;
  dim3 g1((N + 255) / 256, P);
  o2_with_flags([&](auto FP32) { hipLaunchKernelGGL(colsum_part_kernel<FP32>, g1, dim3(256), 0, s, x, M, N, ldx, ws, rpp); },
                x_fp32 != 0);
  O2_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3((N + 31) / 32), dim3(256), 0, s, ws, P, N, out, out_fp32, beta);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_dropout_bwd_colsum(const void* dy, void* dym, int M, int N, float drop_p, uint64_t seed,
                                         const float* rowscale, int rows_per_scale, void* colsum_out, int out_fp32, float beta,
                                         float* ws, int ws_floats, void* stream) {
  if (!dy || !dym || !colsum_out || !ws || M <= 0 || N <= 0 || (N & 7)) return O2_ERR_ARG;
  if (drop_p < 0.f || drop_p >= 1.f || (rowscale && rows_per_scale <= 0)) return O2_ERR_ARG;
  const int rpp = cs_rows(M), P = (M + rpp - 1) / rpp;
  if (ws_floats < P * N) return O2_ERR_ARG;
  const unsigned thr = (unsigned)(drop_p * 256.0f + 0.5f);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dropout_bwd_colsum_kernel, dim3((N + 255) / 256, P), dim3(256), 0, s, (const bf16_t*)dy, (bf16_t*)dym, M, N,
                     thr, 256.0f / (256.0f - (float)thr), seed, rowscale, rows_per_scale, ws, rpp);
  O2_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3((N + 31) / 32), dim3(256), 0, s, ws, P, N, colsum_out, out_fp32, beta);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_batch_sum(const void* x, void* out, int B, int rows, int N, int out_fp32, float beta,
                                void* stream) {
  if (!x || !out || B <= 0 || rows <= 0 || N <= 0) return O2_ERR_ARG;
  const int64_t n = (int64_t)rows * N;
  hipLaunchKernelGGL(batch_sum_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     out, B, n, out_fp32, beta);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
  if (!src || !dst || n <= 0 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 7)) return O2_ERR_ARG;
  hipLaunchKernelGGL(cast_f2b_kernel, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     (bf16_t*)dst, n);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
extern "C" int orbit2_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream) {
  if (!src || !dst || n <= 0) return O2_ERR_ARG;
  hipLaunchKernelGGL(cast_b2f_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src,
                     dst, n);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
extern "C" int orbit2_add_rowvec(const void* a, const void* vec, void* y, int rows, int N, void* stream) {
  if (!a || !vec || !y || rows <= 0 || N <= 0) return O2_ERR_ARG;
  hipLaunchKernelGGL(add_rowvec_kernel, dim3(grid_for((int64_t)rows * N, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)a, (const bf16_t*)vec, (bf16_t*)y, rows, N);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_adamw(float* p, float* m, float* v, const void* g, int g_fp32, void* p16, int64_t n, float lr,
                            float beta1, float beta2, float eps, float wd, float bc1, float bc2, float grad_scale,
                            const float* found_inf, void* stream) {
  if (!p || !m || !v || !g || n <= 0) return O2_ERR_ARG;
  if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) & 15) return O2_ERR_ARG;
  if (p16 && ((uintptr_t)p16 & 7)) return O2_ERR_ARG;
  const float rsbc2 = 1.0f / sqrtf(bc2);
  dim3 grid(grid_for((n + 3) / 4, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  o2_with_flags([&](auto GFP32) {
    hipLaunchKernelGGL(adamw_kernel<GFP32>, grid, block, 0, s, p, m, v, g, (bf16_t*)p16, n, lr, beta1, beta2, eps, wd, bc1,
                       rsbc2, grad_scale, found_inf);
  }, g_fp32 != 0);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_check_finite(const void* g, int g_fp32, int64_t n, float* found_inf, void* stream) {
  if (!g || !found_inf || n <= 0) return O2_ERR_ARG;
  dim3 grid(grid_for(n, 256 * 8)), block(256);
  o2_with_flags([&](auto GFP32) { hipLaunchKernelGGL(check_finite_kernel<GFP32>, grid, block, 0, (hipStream_t)stream, g, n, found_inf); },
                g_fp32 != 0);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

O2_DEFINE_SALT_OP(elem)

extern "C" int orbit2_seed_salt(uint64_t value, int add, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  o2_salt_op_gemm(value, add, s);
  o2_salt_op_attn(value, add, s);
  o2_salt_op_elem(value, add, s);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_droppath_scales(float* out, int B, float p, uint64_t seed, void* stream) {
  if (!out || B <= 0 || p < 0.f || p >= 1.f) return O2_ERR_ARG;
  hipLaunchKernelGGL(droppath_scales_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, out, B, p, seed);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_transpose_bf16(const void* src, void* dst, int R, int C, void* stream) {
  if (!src || !dst || R <= 0 || C <= 0) return O2_ERR_ARG;
  hipLaunchKernelGGL(transpose_bf16_kernel, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)src, (bf16_t*)dst, R, C);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
