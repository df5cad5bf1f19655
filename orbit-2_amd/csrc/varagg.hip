// Folded per-variable patch-embedding + variable-aggregation cross-attention (gfx950).
//
// Reference math (res_slimvit.py:250-265 + :205-230, patch_embed.py:44-52, attention.py:132-176):
//   e_v  = W_v p_v + b_v + var_embed_v            (p_v = the token's 2x2 patch of variable v, 4 values)
//   k_v  = Wk e_v, val_v = Wv e_v, q = Wq var_query           (no bias, no dropout)
//   a_hv = softmax_v( scale * q_h . k_vh ),   z_h = sum_v a_hv val_vh ,   out = proj(z)
// Because e_v is affine in the 4 patch values, with pt_v = (p_v, 1) in R^5:
//   score_hv = sum_c stab[h][v][c] * pt_v[c]          stab = scale * (Wk_h^T q_h) . [W_v | b_v + var_embed_v]
//   z[i]     = sum_v a_{h(i)v} sum_c gtab[v][c][i] * pt_v[c]      gtab[v][c][:] = Wv [W_v | b_v+var_embed_v][:,c]
// The two tables depend on the weights only (built per step by small fp32 GEMMs with autograd); this kernel
// does the per-token work and never materialises the [B,V,L,D] tensor (1.16 GB/sample at interm_1b) nor runs
// the M = B*L*V "kv" GEMM.  Exact algebra; only the rounding order differs from the reference.
//
// Patch sizes P in {1, 2, 4} (the kernels are templates on P): a token's patch of variable v has P*P values, taken row-major
// inside the patch (c = r*P + col, the order of Conv2d(1, D, P, P).weight.view(D, P*P)), pt_v = (p_v, 1) in R^C with
// C = P*P + 1, and the tables are stab [H][V][C], gtab [V][C][D].  Everything written with 5 above is C.  P = 2 is the form
// all interm_* configurations use; its instantiations, entries and summation order are those the file had before P existed.
#include <stdlib.h>
#include "tiles32.h"
#include "../../include/orbit2_hip.h"

namespace {

constexpr int VA_T = 16;      // tokens per workgroup
constexpr int VA_MAXV = 32;   // max variables
constexpr int VA_MAXH = 32;   // max heads

// one channel of the value row of (token, variable): sum_c gtab[v][c][i] * pt[c], the patch terms in the order c = 0 .. P*P-1,
// the constant term last (for P = 2: g0 p0 + g1 p1 + g2 p2 + g3 p3 + g4, the order the kernel has always used)
template <int P>
__device__ __forceinline__ float va_row(const f32x4* g, const float* p, int j) {
  float val = g[0][j] * p[0];
#pragma unroll
  for (int c = 1; c < P * P; ++c) val += g[c][j] * p[c];
  return val + g[P * P][j];
}

constexpr int VA_LDS_LIMIT = 160 * 1024;   // LDS of a gfx950 CU: a launch that needs more is refused on the host

// ---- the steps that the scalar kernel, the ds kernel and the table-gradient kernel share --------------------------------------
// (the staging of aw / da, the score dot and the scalar softmax backward stay written out in their kernels: as helpers they give
// the same instructions in another order in the P = 2 kernels, which are kept as they were: profiles/varagg_shared_parts_equivalence.txt)
// one patch value of (token, variable): x[b][v][P*pr + c/P][P*pc + c%P], the token being (pr, pc) of sample b's [h/P][w/P] grid.
// The caller has checked tok < the token count and c < P*P (stated to the compiler too: without it c / P and c % P are compiled
// for a negative c).  TOK is the kernel's token type (int64_t, or int where the host guarantees the count fits).
template <int P, class TOK>
__device__ __forceinline__ float va_patch_value(const float* x, TOK tok, int v, int c, int V, int h, int w, int L, int Lw) {
  __builtin_assume(c >= 0 && c < P * P);
  const int b = (int)(tok / L), l = (int)(tok - (TOK)b * L);
  const int pr = l / Lw, pc = l - pr * Lw;
  return x[(((size_t)b * V + v) * h + (P * pr + c / P)) * w + P * pc + c % P];
}

// the patch image of a workgroup's VA_T tokens: pt[t][v][c] = the patch value for c < P*P, 1 at c == P*P (the constant term of
// the tables), 0 for a token past the last
template <int P>
__device__ __forceinline__ void va_stage_patches(const float* x, float* pt, int64_t tok0, int64_t ntok, int V, int h, int w,
                                                 int L, int Lw) {
  constexpr int PP = P * P, C = PP + 1;
  const int tid = threadIdx.x;
  for (int e = tid; e < VA_T * V * C; e += 256) {
    const int c = e % C, v = (e / C) % V, t = e / (C * V);
    const int64_t tok = tok0 + t;
    float val = 0.f;
    if (tok < ntok) {
      if (c == PP) val = 1.f;
      else val = va_patch_value<P>(x, tok, v, c, V, h, w, L, Lw);
    }
    pt[e] = val;
  }
}

// four consecutive bf16 of dz (one 8-byte load; p is 8-byte aligned: D % 4 == 0) as four floats
__device__ __forceinline__ void va_load_dz4(const bf16_t* p, float* o) {
  const u32x2 r = *reinterpret_cast<const u32x2*>(p);
  o[0] = bf2f((bf16_t)(r[0] & 0xffff)); o[1] = bf2f((bf16_t)(r[0] >> 16));
  o[2] = bf2f((bf16_t)(r[1] & 0xffff)); o[3] = bf2f((bf16_t)(r[1] >> 16));
}

// LDS: pt[T][V][C], aw[T][H][V]  (+ da[T][H][V] in the backward)
// ZF32 (forward only): z is written as fp32 and attw may be NULL (the fp32 forward path saves nothing for a backward)
template <bool BWD, bool ZF32 = false, int P = 2>
__global__ __launch_bounds__(256) void varagg_kernel(const float* __restrict__ x, const float* __restrict__ stab,
                                                     const float* __restrict__ gtab, bf16_t* __restrict__ z,
                                                     float* __restrict__ attw, const bf16_t* __restrict__ dz,
                                                     float* __restrict__ dstab, float* __restrict__ dgtab, int B,
                                                     int V, int h, int w, int H, int D) {
  constexpr int PP = P * P, C = PP + 1;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* pt = sm;                       // [T][V][C]
  float* aw = pt + VA_T * V * C;        // [T][H][V]
  float* da = aw + VA_T * H * V;        // [T][H][V] (backward only)
  const int tid = threadIdx.x;
  const int Lw = w / P, L = (h / P) * Lw;
  const int64_t tok0 = (int64_t)blockIdx.x * VA_T;
  const int64_t ntok = (int64_t)B * L;
  const int dh = D / H;

  // ---- patches ---------------------------------------------------------------------------------
  va_stage_patches<P>(x, pt, tok0, ntok, V, h, w, L, Lw);
  __syncthreads();
  // ---- scores + softmax over variables (one thread per (token, head)) -----------------------------
  if (!BWD) {
    for (int e = tid; e < VA_T * H; e += 256) {
      const int hh = e % H, t = e / H;
      const float* st = stab + (size_t)hh * V * C;
      const float* pp = pt + (size_t)t * V * C;
      float mx = -1e30f;
      for (int v = 0; v < V; ++v) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += st[v * C + c] * pp[v * C + c];
        mx = fmaxf(mx, s);
      }
      float sum = 0.f;
      for (int v = 0; v < V; ++v) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += st[v * C + c] * pp[v * C + c];
        sum += __expf(s - mx);
      }
      const float inv = 1.f / sum;
      const int64_t tok = tok0 + t;
      for (int v = 0; v < V; ++v) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += st[v * C + c] * pp[v * C + c];
        const float a = __expf(s - mx) * inv;
        aw[(t * H + hh) * V + v] = a;
        if (tok < ntok && (!ZF32 || attw)) attw[((size_t)tok * H + hh) * V + v] = a;
      }
    }
  } else {
    for (int e = tid; e < VA_T * H * V; e += 256) {
      const int64_t tok = tok0 + e / (H * V);
      aw[e] = tok < ntok ? attw[(size_t)tok0 * H * V + e] : 0.f;
      da[e] = 0.f;
    }
  }
  __syncthreads();
  // ---- channel work: thread owns 4-channel chunks ch = tid + 256*k -----------------------------------
  const int nchunk = D / 4;
  for (int ch = tid; ch < nchunk; ch += 256) {
    const int i0 = ch * 4;
    const int hh = i0 / dh;
    if (!BWD) {
      float acc[VA_T][4];
#pragma unroll
      for (int t = 0; t < VA_T; ++t) { acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f; }
      for (int v = 0; v < V; ++v) {
        f32x4 g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = *reinterpret_cast<const f32x4*>(gtab + ((size_t)(v * C + c)) * D + i0);
#pragma unroll
        for (int t = 0; t < VA_T; ++t) {
          const float* p = pt + (t * V + v) * C;
          const float a = aw[(t * H + hh) * V + v];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[t][j] += a * va_row<P>(g, p, j);
        }
      }
#pragma unroll
      for (int t = 0; t < VA_T; ++t) {
        const int64_t tok = tok0 + t;
        if (tok < ntok) {
          if (ZF32) {
            const f32x4 o = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(z) + (size_t)tok * D + i0) = o;
          } else {
            u32x2 o; o[0] = pack_bf2(acc[t][0], acc[t][1]); o[1] = pack_bf2(acc[t][2], acc[t][3]);
            *reinterpret_cast<u32x2*>(z + (size_t)tok * D + i0) = o;
          }
        }
      }
    } else {
      float dzv[VA_T][4];
#pragma unroll
      for (int t = 0; t < VA_T; ++t) {
        const int64_t tok = tok0 + t;
        if (tok < ntok) va_load_dz4(dz + (size_t)tok * D + i0, dzv[t]);
        else { dzv[t][0] = dzv[t][1] = dzv[t][2] = dzv[t][3] = 0.f; }
      }
      for (int v = 0; v < V; ++v) {
        f32x4 g[C];
        float dg[C][4];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          g[c] = *reinterpret_cast<const f32x4*>(gtab + ((size_t)(v * C + c)) * D + i0);
          dg[c][0] = dg[c][1] = dg[c][2] = dg[c][3] = 0.f;
        }
#pragma unroll
        for (int t = 0; t < VA_T; ++t) {
          const float* p = pt + (t * V + v) * C;
          const float a = aw[(t * H + hh) * V + v];
          float dav = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float val = va_row<P>(g, p, j);
            dav += dzv[t][j] * val;
            const float ad = a * dzv[t][j];
#pragma unroll
            for (int c = 0; c < C; ++c) dg[c][j] += ad * p[c];
          }
          atomicAdd(&da[(t * H + hh) * V + v], dav);   // LDS atomic: reduce over the head's channels
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int j = 0; j < 4; ++j) atomicAdd(dgtab + ((size_t)(v * C + c)) * D + i0 + j, dg[c][j]);
      }
    }
  }
  if (BWD) {
    __syncthreads();
    // softmax backward per (token, head): ds_v = a_v (da_v - sum_u a_u da_u); result overwrites da
    for (int e = tid; e < VA_T * H; e += 256) {
      float dot = 0.f;
      for (int v = 0; v < V; ++v) dot += aw[e * V + v] * da[e * V + v];
      for (int v = 0; v < V; ++v) da[e * V + v] = aw[e * V + v] * (da[e * V + v] - dot);
    }
    __syncthreads();
    // dstab[h][v][c] += sum_t ds[t][h][v] * pt[t][v][c]
    for (int e = tid; e < H * V * C; e += 256) {
      const int c = e % C, v = (e / C) % V, hh = e / (C * V);
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < VA_T; ++t) s += da[(t * H + hh) * V + v] * pt[(t * V + v) * C + c];
      atomicAdd(dstab + e, s);
    }
  }
}


// ---------------------------------------------------------------------------------------------------------
// Backward on the matrix cores (head dims 64 / 128 / 256, 5V <= 128).  Per head h and 32-token chunk:
//   G[t,(v,c)]   = sum_{d in h} dz[t,d] * gtab[(v,c),d]                       (MFMA, contraction over the head dim)
//   da[t,v]      = sum_c pt[t,v,c] * G[t,(v,c)] ;  ds = a * (da - sum_u a_u da_u)       (softmax backward, VALU)
//   dstab[h,v,c] += sum_t ds[t,v] * pt[t,v,c]
//   dgtab[(v,c),d] += sum_t (a[t,v] pt[t,v,c]) * dz[t,d]                     (MFMA, contraction over the tokens)
// One workgroup owns (head, token range); its dgtab block lives in MFMA accumulators for the whole range and
// is added to HBM once (fp32 atomics: 5V x DH floats per workgroup instead of 5V x D per 16 tokens).
// dz is bf16 as stored; the fp32 operands (gtab, a*pt) enter as bf16 hi + bf16 lo pairs (two MFMAs, ~16 mantissa
// bits), accumulation is fp32.  The gtab fragments are loop-invariant and live in registers.
constexpr int VM_NV = 128;    // padded (v,c) extent
constexpr int VM_GS = 132;    // fp32 row stride of the G image
constexpr int VM_T = 32;      // tokens per chunk

// stage a [32 rows][D] tile (same image as stage64's, half the rows); rows >= nvalid repeat row nvalid-1
template <int D>
__device__ __forceinline__ void stage32(const bf16_t* __restrict__ base, size_t stride, char* tile, int wave,
                                        int lane, int nvalid) {
  using C = Cfg<D>;
  constexpr int NI = VM_T * C::RB / 1024;  // LDS-DMA instructions per tile: 4 / 8 / 16
#pragma unroll
  for (int t = 0; t < NI / 4; ++t) {
    const int i = wave * (NI / 4) + t;
    const int row = i * C::RPI + lane / C::CPR;
    const int c = (lane % C::CPR) ^ swz<D>(row);
    const int rsrc = row < nvalid ? row : nvalid - 1;
    const uint32_t off = ((uint32_t)rsrc * (uint32_t)stride + (uint32_t)(c * 8)) * 2u;
    glds16(reinterpret_cast<const char*>(base) + off, tile + i * 1024);
  }
}

__device__ __forceinline__ void split_bf16(float v, bf16_t& hi, bf16_t& lo) {
  hi = f2bf(v);
  lo = f2bf(v - bf2f(hi));
}

template <int DH>
__global__ __launch_bounds__(256, (DH == 256 ? 1 : 2)) void varagg_bwd_mfma_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ gtab,
                                                                 const float* __restrict__ attw,
                                                                 const bf16_t* __restrict__ dz,
                                                                 float* __restrict__ dstab, float* __restrict__ dgtab,
                                                                 int B, int V, int h, int w, int H, int D,
                                                                 int chunks_per_wg) {
  using CZ = Cfg<DH>;
  using CA = Cfg<VM_NV>;
  constexpr int A2_BYTES = VM_T * CA::RB;
  constexpr int NDBZ = DH / 32;
  extern __shared__ __attribute__((aligned(16))) char vsm[];
  char* zt = vsm;                                             // [32][DH] bf16 (LDS-DMA, swizzled)
  char* a2hi = zt + VM_T * CZ::RB;                            // [32][128] bf16 (swizzled)
  char* a2lo = a2hi + A2_BYTES;
  float* gimg = reinterpret_cast<float*>(a2lo + A2_BYTES);    // [32][VM_GS] fp32
  float* pt = gimg + VM_T * VM_GS;                            // [32][V][4]
  float* aw = pt + VM_T * V * 4;                              // [32][V]
  float* dsv = aw + VM_T * V;                                 // [32][V]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hq = lane >> 5;
  const int hh = blockIdx.x;
  const int Lw = w / 2, L = (h / 2) * Lw;
  const int ntok = B * L;
  const int nchunk = (ntok + VM_T - 1) / VM_T;
  const int c0 = blockIdx.y * chunks_per_wg;
  const int c1 = min(nchunk, c0 + chunks_per_wg);
  if (c0 >= c1) return;                                       // (never: the launch gives every token range a chunk)
  const int NV5 = 5 * V;
  // this token range's slabs of the workspace: [range][H][V][5] and [range][5V][D]; orbit2_varagg_bwd adds the ranges in order
  dstab += (size_t)blockIdx.y * H * NV5;
  dgtab += (size_t)blockIdx.y * NV5 * D;
  const int NB = (NV5 + 31) / 32;
  const bool wave_on = wave < NB;                             // wave <-> 32-row block of (v,c)
  const bf16_t* zbase = dz + (size_t)hh * DH;

  // gtab rows [32*wave, +32) of this head as MFMA operand fragments, bf16 hi + lo, held in registers for the whole
  // kernel (rows >= 5V are zero): lane (i, hq) owns row 32*wave + i, columns 16*ds + 8*hq + {0..7}
  bf16x8 gfh[CZ::NDS], gfl[CZ::NDS];
  {
    const int row = wave * 32 + (lane & 31);
#pragma unroll
    for (int ds = 0; ds < CZ::NDS; ++ds) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { gfh[ds][j] = 0; gfl[ds][j] = 0; }
      if (row < NV5) {
        const float* src = gtab + (size_t)row * D + (size_t)hh * DH + ds * 16 + 8 * hq;
        const f32x4 lo4 = *reinterpret_cast<const f32x4*>(src), hi4 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          bf16_t hi, lo;
          split_bf16(j < 4 ? lo4[j] : hi4[j - 4], hi, lo);
          gfh[ds][j] = (short)hi; gfl[ds][j] = (short)lo;
        }
      }
    }
  }
  // the a*pt images: columns >= 5V stay zero for the whole kernel
  for (int e = tid; e < 2 * A2_BYTES / 16; e += 256) {
    bf16x8 zz;
#pragma unroll
    for (int j = 0; j < 8; ++j) zz[j] = 0;
    reinterpret_cast<bf16x8*>(a2hi)[e] = zz;
  }

  f32x16 acc[NDBZ];                                           // dgtab rows [32*wave, +32) x the head's DH columns
#pragma unroll
  for (int i = 0; i < NDBZ; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  // dstab partial of this thread: (v,c) = tid % 128 (if < 5V), tokens [16*(tid/128), +16) of every chunk
  const int se = tid & 127, shalf = tid >> 7;
  const int sv = se / 5, sc = se - 5 * sv;
  float sacc = 0.f;

  for (int ch = c0; ch < c1; ++ch) {
    const int tok0 = ch * VM_T;
    stage32<DH>(zbase + (size_t)tok0 * D, (size_t)D, zt, wave, lane, ntok - tok0);
    // ---- patches + attention weights of the chunk: thread -> (token, k); loops over variables ----------------
    {
      const int t = tid >> 3, k = tid & 7, c = k & 3;
      const int tok = tok0 + t;
      const bool ok = tok < ntok;
      const int tk = ok ? tok : ntok - 1;
      const int b = tk / L, l = tk - b * L;
      const int pr = l / Lw, pc = l - pr * Lw;
      const float* xp = x + ((size_t)b * V * h + (2 * pr + (c >> 1))) * w + 2 * pc + (c & 1);
      const float* ap = attw + ((size_t)tk * H + hh) * V;
      for (int v = k >> 2; v < V; v += 2) pt[(t * V + v) * 4 + c] = ok ? xp[(size_t)v * h * w] : 0.f;
      for (int v = k; v < V; v += 8) aw[t * V + v] = ok ? ap[v] : 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // B1: z tile, pt, aw visible
    // ---- G = dz . gtab^T : wave -> (v,c) block ------------------------------------------------------------------
    if (wave_on) {
      f32x16 g;
#pragma unroll
      for (int r = 0; r < 16; ++r) g[r] = 0.f;
#pragma unroll
      for (int ds = 0; ds < CZ::NDS; ++ds) {
        const bf16x8 zf = row_frag<DH>(zt, lane & 31, ds, hq);
        g = MFMA32(zf, gfh[ds], g);
        g = MFMA32(zf, gfl[ds], g);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = (r & 3) + 8 * (r >> 2) + 4 * hq;
        gimg[t * VM_GS + wave * 32 + (lane & 31)] = g[r];
      }
    }
    __syncthreads();                                   // B2: G visible
    // ---- softmax backward; 8 threads per token ------------------------------------------------------------------
    {
      const int t = tid >> 3, sub = tid & 7;
      float dav[4];
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = sub + 8 * k;
        dav[k] = 0.f;
        if (v < V) {
          const float* gp = gimg + t * VM_GS + 5 * v;
          const f32x4 p4 = *reinterpret_cast<const f32x4*>(pt + (t * V + v) * 4);
          dav[k] = p4[0] * gp[0] + p4[1] * gp[1] + p4[2] * gp[2] + p4[3] * gp[3] + gp[4];
          dot += aw[t * V + v] * dav[k];
        }
      }
      dot += __shfl_xor(dot, 1);
      dot += __shfl_xor(dot, 2);
      dot += __shfl_xor(dot, 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = sub + 8 * k;
        if (v < V) {
          const float a = aw[t * V + v];
          dsv[t * V + v] = a * (dav[k] - dot);
          const f32x4 p4 = *reinterpret_cast<const f32x4*>(pt + (t * V + v) * 4);
#pragma unroll
          for (int c = 0; c < 5; ++c) {
            const int col = 5 * v + c;
            bf16_t hi, lo;
            split_bf16(c < 4 ? a * p4[c] : a, hi, lo);
            const int off = t * CA::RB + (((col >> 3) ^ swz<VM_NV>(t)) << 4) + (col & 7) * 2;
            *reinterpret_cast<bf16_t*>(a2hi + off) = hi;
            *reinterpret_cast<bf16_t*>(a2lo + off) = lo;
          }
        }
      }
    }
    __syncthreads();                                   // B3: ds and the a*pt images visible
    // ---- dgtab += (a pt)^T . dz  (contraction over the chunk's tokens) ----------------------------------------------
    if (wave_on) {
#pragma unroll
      for (int ks = 0; ks < VM_T / 16; ++ks) {
        const bf16x8 ah = tr_frag<VM_NV>(a2hi, ks * 16, wave, lane);
        const bf16x8 al = tr_frag<VM_NV>(a2lo, ks * 16, wave, lane);
#pragma unroll
        for (int db = 0; db < NDBZ; ++db) {
          const bf16x8 zf = tr_frag<DH>(zt, ks * 16, db, lane);
          acc[db] = MFMA32(ah, zf, acc[db]);
          acc[db] = MFMA32(al, zf, acc[db]);
        }
      }
    }
    // ---- dstab partial ------------------------------------------------------------------------------------------
    if (se < NV5) {
#pragma unroll 4
      for (int t = shalf * (VM_T / 2); t < (shalf + 1) * (VM_T / 2); ++t)
        sacc += dsv[t * V + sv] * (sc < 4 ? pt[(t * V + sv) * 4 + sc] : 1.f);
    }
    __syncthreads();                                   // B4: chunk consumed; the images may be overwritten
  }
  // the two token halves of the workgroup (threads se and se + 128) add in a fixed order through LDS, then one plain store
  // into this workgroup's slab
  if (se < NV5 && shalf == 1) dsv[se] = sacc;
  __syncthreads();
  if (se < NV5 && shalf == 0) dstab[((size_t)hh * V + sv) * 5 + sc] = sacc + dsv[se];
  if (wave_on) {
#pragma unroll
    for (int db = 0; db < NDBZ; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hq;
        if (row < NV5) dgtab[(size_t)row * D + (size_t)hh * DH + db * 32 + (lane & 31)] = acc[db][r];
      }
  }
}

// token ranges of the MFMA backward: ~3 workgroups per CU over (heads x ranges)
static int varagg_bwd_splits(int ntok, int H, int* cpw_out) {
  const int nchunk = (ntok + VM_T - 1) / VM_T;
  int splits = (768 + H - 1) / H;
  if (splits > nchunk) splits = nchunk;
  const int cpw = (nchunk + splits - 1) / splits;
  if (cpw_out) *cpw_out = cpw;
  return (nchunk + cpw - 1) / cpw;
}


// ---------------------------------------------------------------------------------------------------------
// Backward for P != 2 (C = 2 or 17): two stages, no float atomics anywhere, every sum in an order fixed by the shape.
// The scalar kernel above adds its [V*C, D] table partial to HBM once per 16 tokens, and the MFMA form needs C*V <= 128 rows;
// neither fits C = 17.  Here
//   (1) varagg_ds_kernel    per 16 tokens:  da[t,h,v] = sum_{i in h} dz[t,i] * sum_c gtab[v,c,i] pt[t,v,c]  (the scalar kernel's
//       channel loop without the table part; the per-thread partials of a head's channels meet in LDS and ONE thread adds them
//       in a fixed order), then the softmax backward ds = a * (da - sum_u a_u da_u) per (token, head) -> ds [tokens, H, V] in HBM
//   (2) varagg_tabgrad_kernel  one workgroup per (variable v, token range):
//         dgtab[v][c][i] = sum_t a[t,h(i),v] * pt[t,v,c] * dz[t,i]      (does not depend on the softmax backward)
//         dstab[h][v][c] = sum_t ds[t,h,v] * pt[t,v,c]
//       a thread owns its 4-channel chunks; dg[C][4] stays in registers over the whole token range and is stored once into the
//       range's slab, as is the [H][C] piece of dstab; o2_sum_parts then adds the ranges in order (+= into dstab / dgtab).
// ---------------------------------------------------------------------------------------------------------
constexpr int VT_T = 32;      // tokens staged per round of the table-gradient kernel

template <int P>
__global__ __launch_bounds__(256) void varagg_ds_kernel(const float* __restrict__ x, const float* __restrict__ gtab,
                                                        const float* __restrict__ attw, const bf16_t* __restrict__ dz,
                                                        float* __restrict__ ds, int B, int V, int h, int w, int H, int D) {
  constexpr int PP = P * P, C = PP + 1;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* pt = sm;                       // [T][V][C]
  float* aw = pt + VA_T * V * C;        // [T][H][V]
  float* da = aw + VA_T * H * V;        // [T][H][V]
  float* part = da + VA_T * H * V;      // [2][T][256]: per-thread partials of da, double-buffered over v
  const int tid = threadIdx.x;
  const int Lw = w / P, L = (h / P) * Lw;
  const int64_t tok0 = (int64_t)blockIdx.x * VA_T;
  const int64_t ntok = (int64_t)B * L;
  const int dh = D / H;
  const int gs = dh / 4;                // threads (4-channel chunks) per head

  va_stage_patches<P>(x, pt, tok0, ntok, V, h, w, L, Lw);
  for (int e = tid; e < VA_T * H * V; e += 256) {
    const int64_t tok = tok0 + e / (H * V);
    aw[e] = tok < ntok ? attw[(size_t)tok0 * H * V + e] : 0.f;
    da[e] = 0.f;
  }
  __syncthreads();
  const int nchunk = D / 4;
  for (int cb = 0; cb < nchunk; cb += 256) {          // (one round for D <= 1024)
    const int ch = cb + tid;
    const bool on = ch < nchunk;
    const int i0 = on ? ch * 4 : 0;
    float dzv[VA_T][4];
#pragma unroll
    for (int t = 0; t < VA_T; ++t) {
      const int64_t tok = tok0 + t;
      if (on && tok < ntok) va_load_dz4(dz + (size_t)tok * D + i0, dzv[t]);
      else { dzv[t][0] = dzv[t][1] = dzv[t][2] = dzv[t][3] = 0.f; }
    }
    // the heads whose chunks lie in [cb, cb + 256): head hh owns chunks [hh * gs, (hh + 1) * gs)
    const int h_lo = cb / gs, h_hi = min(H, (min(nchunk, cb + 256) + gs - 1) / gs);
    for (int v = 0; v < V; ++v) {
      f32x4 g[C];
#pragma unroll
      for (int c = 0; c < C; ++c) g[c] = *reinterpret_cast<const f32x4*>(gtab + ((size_t)(v * C + c)) * D + i0);
      float* pb = part + (v & 1) * (VA_T * 256);
#pragma unroll
      for (int t = 0; t < VA_T; ++t) {
        const float* p = pt + (t * V + v) * C;
        float dav = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) dav += dzv[t][j] * va_row<P>(g, p, j);
        pb[t * 256 + tid] = dav;                       // (0 for a thread without a chunk: its dz is 0)
      }
      __syncthreads();     // one barrier per v: round v + 2 reuses this buffer only after every thread has passed round v + 1's
      // the owner of (token, head) adds the head's partials in a fixed order (the start is rotated by the head so that the
      // threads of a wave read different banks); da is touched by its owner only
      for (int e = tid; e < VA_T * (h_hi - h_lo); e += 256) {
        const int t = e / (h_hi - h_lo), hh = h_lo + e % (h_hi - h_lo);
        const int lo = max(hh * gs, cb) - cb, n = min((hh + 1) * gs, cb + 256) - cb - lo;
        const float* src = pb + t * 256 + lo;
        float sum = 0.f;
        int k = hh % n;
        for (int i = 0; i < n; ++i) {
          sum += src[k];
          k = k + 1 == n ? 0 : k + 1;
        }
        da[(t * H + hh) * V + v] += sum;
      }
    }
    __syncthreads();
  }
  // softmax backward per (token, head): ds_v = a_v (da_v - sum_u a_u da_u)
  for (int e = tid; e < VA_T * H; e += 256) {
    const int64_t tok = tok0 + e / H;
    if (tok >= ntok) continue;
    float dot = 0.f;
    for (int v = 0; v < V; ++v) dot += aw[e * V + v] * da[e * V + v];
    float* o = ds + (size_t)tok0 * H * V + (size_t)e * V;
    for (int v = 0; v < V; ++v) o[v] = aw[e * V + v] * (da[e * V + v] - dot);
  }
}

template <int P>
__global__ __launch_bounds__(256) void varagg_tabgrad_kernel(const float* __restrict__ x, const float* __restrict__ attw,
                                                             const float* __restrict__ ds, const bf16_t* __restrict__ dz,
                                                             float* __restrict__ ws_s, float* __restrict__ ws_g, int B, int V,
                                                             int h, int w, int H, int D, int rounds_per_wg) {
  constexpr int PP = P * P, C = PP + 1;
  constexpr int NS = (VA_MAXH * C + 255) / 256;       // dstab entries of this variable a thread owns: [H][C] over 256 threads
  __shared__ float pt[VT_T][C];
  __shared__ float aw[VT_T][VA_MAXH];
  __shared__ float dsv[VT_T][VA_MAXH];
  const int tid = threadIdx.x;
  const int v = blockIdx.x;
  const int Lw = w / P, L = (h / P) * Lw;
  const int ntok = B * L;
  const int nround = (ntok + VT_T - 1) / VT_T;
  const int r0 = blockIdx.y * rounds_per_wg, r1 = min(nround, r0 + rounds_per_wg);
  const int dh = D / H, nchunk = D / 4;
  // this token range's slabs: [range][H][V][C] and [range][V][C][D]
  ws_s += (size_t)blockIdx.y * H * V * C;
  ws_g += ((size_t)blockIdx.y * V + v) * C * D;
  float sacc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sacc[k] = 0.f;

  for (int cb = 0; cb < nchunk; cb += 256) {          // (one pass over the range for D <= 1024)
    const int ch = cb + tid;
    const bool on = ch < nchunk;
    const int i0 = on ? ch * 4 : 0;
    const int hh = i0 / dh;
    float dg[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) dg[c][0] = dg[c][1] = dg[c][2] = dg[c][3] = 0.f;
    for (int r = r0; r < r1; ++r) {
      const int tok0 = r * VT_T;
      const int nt = min(VT_T, ntok - tok0);
      for (int e = tid; e < VT_T * C; e += 256) {
        const int t = e / C, c = e - t * C;
        float val = 0.f;
        if (t < nt) {
          if (c == PP) val = 1.f;
          else val = va_patch_value<P>(x, tok0 + t, v, c, V, h, w, L, Lw);
        }
        pt[t][c] = val;
      }
      for (int e = tid; e < VT_T * H; e += 256) {
        const int t = e / H, h2 = e - t * H;
        const size_t src = ((size_t)(tok0 + t) * H + h2) * V + v;
        aw[t][h2] = t < nt ? attw[src] : 0.f;
        dsv[t][h2] = t < nt ? ds[src] : 0.f;
      }
      __syncthreads();
      if (on) {
#pragma unroll 4
        for (int t = 0; t < nt; ++t) {
          float q[4];
          va_load_dz4(dz + (size_t)(tok0 + t) * D + i0, q);
          const float a = aw[t][hh];
          const float ad[4] = {a * q[0], a * q[1], a * q[2], a * q[3]};
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float pc_ = pt[t][c];
#pragma unroll
            for (int j = 0; j < 4; ++j) dg[c][j] += ad[j] * pc_;
          }
        }
      }
      if (cb == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          const int e = tid + 256 * k;
          if (e < H * C) {
            const int h2 = e / C, c = e - h2 * C;
            float sum = sacc[k];
            for (int t = 0; t < VT_T; ++t) sum += dsv[t][h2] * pt[t][c];     // (rows >= nt are zero)
            sacc[k] = sum;
          }
        }
      }
      __syncthreads();
    }
    if (on) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const f32x4 o = {dg[c][0], dg[c][1], dg[c][2], dg[c][3]};
        *reinterpret_cast<f32x4*>(ws_g + (size_t)c * D + i0) = o;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int e = tid + 256 * k;
    if (e < H * C) {
      const int h2 = e / C, c = e - h2 * C;
      ws_s[((size_t)h2 * V + v) * C + c] = sacc[k];
    }
  }
}

// token ranges of the table-gradient kernel: ~2 workgroups per CU over (variables x ranges)
static int varagg_tabgrad_splits(int ntok, int V, int* rpw_out) {
  const int nround = (ntok + VT_T - 1) / VT_T;
  int splits = (512 + V - 1) / V;
  if (splits > nround) splits = nround;
  const int rpw = (nround + splits - 1) / splits;
  if (rpw_out) *rpw_out = rpw;
  return (nround + rpw - 1) / rpw;
}

// dynamic LDS of each kernel form, bytes.  The scalar kernel lays out pt + aw + da; the forward at P = 2 asks for that too although
// it never touches da, the second T*H*V half (the request it has always made: dropping it changes how many workgroups share a CU)
enum va_form { VA_FWD, VA_BWD_SCALAR, VA_BWD_DS, VA_BWD_MFMA };
static size_t va_lds(va_form form, int P, int V, int H, int DH = 0) {
  const size_t pt = (size_t)VA_T * V * (P * P + 1), thv = (size_t)VA_T * H * V;
  switch (form) {
    case VA_FWD: return sizeof(float) * (pt + (P == 2 ? 2 : 1) * thv);               // pt + aw (+ the unused half at P = 2)
    case VA_BWD_SCALAR: return sizeof(float) * (pt + 2 * thv);                        // pt + aw + da
    case VA_BWD_DS: return sizeof(float) * (pt + 2 * thv + 2 * (size_t)VA_T * 256);   // pt + aw + da + part
    default:                                                                          // zt + a2hi + a2lo + gimg + pt + aw + dsv
      return (size_t)VM_T * DH * 2 + 2 * (size_t)VM_T * VM_NV * 2 + sizeof(float) * (size_t)(VM_T * VM_GS + VM_T * V * 4 + 2 * VM_T * V);
  }
}

// lets a kernel ask for up to a CU's whole LDS; one host call on the first launch of each instantiation
template <auto KERNEL>
static void va_allow_large_lds() {
  static bool attr_set = false;   // one flag per instantiation
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, VA_LDS_LIMIT);
    attr_set = true;
  }
}

// f(o2_int<P>) for the patch size the host has checked (va_check: 1, 2 or 4)
template <class F>
static void va_with_patch(int P, F&& f) {
  if (P == 1) f(o2_int<1>{});
  else if (P == 2) f(o2_int<2>{});
  else f(o2_int<4>{});
}

// the token ranges' slabs of a two-stage backward, added in order: += into the caller's tables, as the atomics did
static void va_sum_ranges(const float* ws_s, const float* ws_g, int splits, int V, int H, int D, int C, float* dstab,
                          float* dgtab, hipStream_t s) {
  o2_sum_parts(ws_s, splits, (int64_t)H * V * C, dstab, (int64_t)H * V * C, 1.0f, 1, s);
  o2_sum_parts(ws_g, splits, (int64_t)V * C * D, dgtab, (int64_t)V * C * D, 1.0f, 1, s);
}

}  // namespace

static int va_check(int B, int V, int h, int w, int H, int D, int P = 2) {
  if (P != 1 && P != 2 && P != 4) return O2_ERR_ARG;
  if (B <= 0 || V <= 0 || V > VA_MAXV || H <= 0 || H > VA_MAXH || D <= 0 || h <= 0 || w <= 0) return O2_ERR_ARG;
  if ((h % P) || (w % P) || (D % 4) || (D % H) || ((D / H) % 4)) return O2_ERR_ARG;
  return O2_OK;
}

// ---- the forward of every patch size, z as bf16 or (zf32) as fp32 -----------------------------------------------------------------
static int va_forward(int P, bool zf32, const float* x, const float* stab, const float* gtab, void* z, float* attw, int B, int V,
                      int h, int w, int H, int D, void* stream) {
  int rc = va_check(B, V, h, w, H, D, P);
  if (rc) return rc;
  const int64_t ntok = (int64_t)B * (h / P) * (w / P);
  const size_t shm = va_lds(VA_FWD, P, V, H);
  if (shm > (size_t)VA_LDS_LIMIT) return O2_ERR_UNSUPPORTED;          // (P = 4 only: at most 138 KiB at P = 2, V = H = 32)
  va_with_patch(P, [&](auto PC) {
    o2_with_flags([&](auto ZF32) {
      va_allow_large_lds<varagg_kernel<false, ZF32, PC>>();
      hipLaunchKernelGGL((varagg_kernel<false, ZF32, PC>), dim3((unsigned)((ntok + VA_T - 1) / VA_T)), dim3(256), shm,
                         (hipStream_t)stream, x, stab, gtab, (bf16_t*)z, attw, (const bf16_t*)nullptr, (float*)nullptr,
                         (float*)nullptr, B, V, h, w, H, D);
    }, zf32);
  });
  O2_CHECK_LAUNCH();
  return O2_OK;
}

// ---- the backward.  P = 2: the MFMA kernel where it serves the shape, the scalar kernel with its atomics otherwise.  P = 1, 4:
// the two-stage kernels or a refusal.  Both fixed-order forms store per token range into `ws` and add the ranges in order -----------
static bool varagg_bwd_fixed_order(int64_t ntok, int V, int H, int D) {
  static const bool force_scalar = getenv("ORBIT2_VARAGG_SCALAR") != nullptr;   // debugging aid: the fp32 VALU kernel
  const int dh = D / H;
  return !force_scalar && (dh == 64 || dh == 128 || dh == 256) && 5 * V <= VM_NV && ntok < (1ll << 31) - 64;
}

// whether the backward at patch != 2 serves the shape: valid arguments, token count in int range, LDS within a CU's
static bool varagg_bwd_p_served(int B, int V, int h, int w, int patch, int H, int D) {
  if (va_check(B, V, h, w, H, D, patch)) return false;
  if ((int64_t)B * (h / patch) * (w / patch) >= (1ll << 31) - 64) return false;
  return va_lds(VA_BWD_DS, patch, V, H) <= (size_t)VA_LDS_LIMIT;
}

static int va_backward(int P, const float* x, const float* gtab, const float* attw, const void* dz, float* dstab, float* dgtab,
                       int B, int V, int h, int w, int H, int D, float* ws, void* stream) {
  int rc = va_check(B, V, h, w, H, D, P);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t ntok = (int64_t)B * (h / P) * (w / P);
  const dim3 tok_grid((unsigned)((ntok + VA_T - 1) / VA_T));
  if (P != 2) {
    if (!varagg_bwd_p_served(B, V, h, w, P, H, D)) return O2_ERR_UNSUPPORTED;
    va_with_patch(P, [&](auto PC) {
      if constexpr (PC != 2) {
        constexpr int C = PC * PC + 1;
        int rpw;
        const int splits = varagg_tabgrad_splits((int)ntok, V, &rpw);
        float* ws_ds = ws;                                           // [tokens][H][V]
        float* ws_s = ws_ds + (size_t)ntok * H * V;                  // [range][H][V][C]
        float* ws_g = ws_s + (size_t)splits * H * V * C;             // [range][V][C][D]
        va_allow_large_lds<varagg_ds_kernel<PC>>();
        hipLaunchKernelGGL(varagg_ds_kernel<PC>, tok_grid, dim3(256), va_lds(VA_BWD_DS, PC, V, H), s, x, gtab, attw,
                           (const bf16_t*)dz, ws_ds, B, V, h, w, H, D);
        hipLaunchKernelGGL(varagg_tabgrad_kernel<PC>, dim3((unsigned)V, (unsigned)splits), dim3(256), 0, s, x, attw, ws_ds,
                           (const bf16_t*)dz, ws_s, ws_g, B, V, h, w, H, D, rpw);
        va_sum_ranges(ws_s, ws_g, splits, V, H, D, C, dstab, dgtab, s);
      }
    });
  } else if (varagg_bwd_fixed_order(ntok, V, H, D)) {
    // every (head, token range) workgroup stores its partial tables in the range's slab of `ws`; the ranges are then added in
    // a fixed order (round 4: instead of one fp32 atomic flush per workgroup -- bitwise reproducible)
    int cpw;
    const int splits = varagg_bwd_splits((int)ntok, H, &cpw);
    float* ws_s = ws;
    float* ws_g = ws + (size_t)splits * H * V * 5;
    auto launch = [&](auto DH) {
      va_allow_large_lds<varagg_bwd_mfma_kernel<DH>>();
      hipLaunchKernelGGL(varagg_bwd_mfma_kernel<DH>, dim3((unsigned)H, (unsigned)splits), dim3(256),
                         va_lds(VA_BWD_MFMA, 2, V, H, DH), s, x, gtab, attw, (const bf16_t*)dz, ws_s, ws_g, B, V, h, w, H, D, cpw);
    };
    if (D / H == 64) launch(o2_int<64>{});
    else if (D / H == 128) launch(o2_int<128>{});
    else launch(o2_int<256>{});
    va_sum_ranges(ws_s, ws_g, splits, V, H, D, 5, dstab, dgtab, s);
  } else {
    va_allow_large_lds<varagg_kernel<true>>();
    hipLaunchKernelGGL(varagg_kernel<true>, tok_grid, dim3(256), va_lds(VA_BWD_SCALAR, 2, V, H), s, x, (const float*)nullptr, gtab,
                       (bf16_t*)nullptr, (float*)attw, (const bf16_t*)dz, dstab, dgtab, B, V, h, w, H, D);
  }
  O2_CHECK_LAUNCH();
  return O2_OK;
}

// floats of `ws` that va_backward writes; 0 for what it refuses.  At P = 2 the MFMA form's, whichever kernel then runs
static int64_t va_backward_ws_floats(int P, int B, int V, int h, int w, int H, int D) {
  if (va_check(B, V, h, w, H, D, P)) return 0;
  const int64_t ntok = (int64_t)B * (h / P) * (w / P);
  if (ntok >= (1ll << 31) - 64) return 0;
  if (P != 2 && va_lds(VA_BWD_DS, P, V, H) > (size_t)VA_LDS_LIMIT) return 0;
  const int64_t C = P * P + 1;
  if (P == 2) return (int64_t)varagg_bwd_splits((int)ntok, H, nullptr) * ((int64_t)H * V * C + (int64_t)V * C * D);
  return ntok * H * V + (int64_t)varagg_tabgrad_splits((int)ntok, V, nullptr) * ((int64_t)H * V * C + (int64_t)V * C * D);
}

// 1 when va_backward takes a two-stage fixed-order path for this shape (bitwise reproducible gradients), 0 when it falls back to the
// scalar kernel whose table gradients are accumulated with fp32 atomics, or refuses; the only path at patch 1 / 4 is fixed-order
static int va_backward_is_fixed_order(int P, int B, int V, int h, int w, int H, int D) {
  if (P != 2) return varagg_bwd_p_served(B, V, h, w, P, H, D) ? 1 : 0;
  if (va_check(B, V, h, w, H, D)) return 0;
  return varagg_bwd_fixed_order((int64_t)B * (h / 2) * (w / 2), V, H, D) ? 1 : 0;
}

// ---- the entries: NULL checks and a call.  The plain ones are patch 2; the `_p` ones carry the patch size (1, 2 or 4) and at 2 are
// the plain call: same kernels, same launch ----------------------------------------------------------------------------------
extern "C" int orbit2_varagg_fwd(const float* x, const float* stab, const float* gtab, void* z, float* attw, int B,
                                 int V, int h, int w, int H, int D, void* stream) {
  if (!x || !stab || !gtab || !z || !attw) return O2_ERR_ARG;
  return va_forward(2, false, x, stab, gtab, z, attw, B, V, h, w, H, D, stream);
}

extern "C" int orbit2_varagg_fwd_f32(const float* x, const float* stab, const float* gtab, float* z, float* attw, int B,
                                     int V, int h, int w, int H, int D, void* stream) {
  if (!x || !stab || !gtab || !z) return O2_ERR_ARG;              // attw may be NULL
  return va_forward(2, true, x, stab, gtab, z, attw, B, V, h, w, H, D, stream);
}

extern "C" int orbit2_varagg_fwd_p(const float* x, const float* stab, const float* gtab, void* z, float* attw, int B, int V,
                                   int h, int w, int patch, int H, int D, void* stream) {
  if (!x || !stab || !gtab || !z || !attw) return O2_ERR_ARG;
  return va_forward(patch, false, x, stab, gtab, z, attw, B, V, h, w, H, D, stream);
}

extern "C" int orbit2_varagg_fwd_f32_p(const float* x, const float* stab, const float* gtab, float* z, float* attw, int B,
                                       int V, int h, int w, int patch, int H, int D, void* stream) {
  if (!x || !stab || !gtab || !z) return O2_ERR_ARG;              // attw may be NULL
  return va_forward(patch, true, x, stab, gtab, z, attw, B, V, h, w, H, D, stream);
}

extern "C" int orbit2_varagg_bwd(const float* x, const float* gtab, const float* attw, const void* dz, float* dstab,
                                 float* dgtab, int B, int V, int h, int w, int H, int D, float* ws, void* stream) {
  if (!x || !gtab || !attw || !dz || !dstab || !dgtab || !ws) return O2_ERR_ARG;
  return va_backward(2, x, gtab, attw, dz, dstab, dgtab, B, V, h, w, H, D, ws, stream);
}

extern "C" int orbit2_varagg_bwd_p(const float* x, const float* gtab, const float* attw, const void* dz, float* dstab,
                                   float* dgtab, int B, int V, int h, int w, int patch, int H, int D, float* ws, void* stream) {
  if (!x || !gtab || !attw || !dz || !dstab || !dgtab || !ws) return O2_ERR_ARG;
  return va_backward(patch, x, gtab, attw, dz, dstab, dgtab, B, V, h, w, H, D, ws, stream);
}

extern "C" int64_t orbit2_varagg_bwd_ws_floats(int B, int V, int h, int w, int H, int D) {
  return va_backward_ws_floats(2, B, V, h, w, H, D);
}
extern "C" int64_t orbit2_varagg_bwd_p_ws_floats(int B, int V, int h, int w, int patch, int H, int D) {
  return va_backward_ws_floats(patch, B, V, h, w, H, D);
}
extern "C" int orbit2_varagg_bwd_is_fixed_order(int B, int V, int h, int w, int H, int D) {
  return va_backward_is_fixed_order(2, B, V, h, w, H, D);
}
extern "C" int orbit2_varagg_bwd_p_is_fixed_order(int B, int V, int h, int w, int patch, int H, int D) {
  return va_backward_is_fixed_order(patch, B, V, h, w, H, D);
}

// ---------------------------------------------------------------------------------------------------------
// The per-variable rows the two tables are built from:  cmat[(v, c)][D],  c = 0..3: the patch-embed weight of variable ids[v]
// seen as [D][4] (res_slimvit.py:64-66: PatchEmbed Conv2d(1, D, 2, 2).weight), transposed;  c = 4: its bias + var_embed[ids[v]]
// (res_slimvit.py:182-201, 251-262).  The V_total per-variable parameters are separate tensors in the reference's state dict;
// here they are addressed as base + index * stride (the engine lays them out at a uniform pitch in its flat buffers; the host
// checks that before taking this path), so ONE launch replaces a stack + transpose + index_select + add + cat -- and its
// transpose below replaces their autograd: per step 2 V + 1 gradient accumulations of a few KiB each.
// ---------------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void tables_gather_kernel(const float* __restrict__ wb, int64_t ws, const float* __restrict__ bb,
                                                            int64_t bs, const float* __restrict__ ve, const int* __restrict__ ids,
                                                            float* __restrict__ cmat, int D) {
  const int v = blockIdx.x, id = ids[v];
  const float* w = wb + (int64_t)id * ws;
  const float* b = bb + (int64_t)id * bs;
  const float* e = ve + (int64_t)id * D;
  float* o = cmat + (size_t)v * 5 * D;
  for (int d = threadIdx.x; d < D; d += 256) {
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + (size_t)d * 4);
    o[d] = w4[0]; o[D + d] = w4[1]; o[2 * D + d] = w4[2]; o[3 * D + d] = w4[3];
    o[4 * D + d] = b[d] + e[d];
  }
}
// gradients ACCUMULATE (the engine memsets its fp32 gradient bucket at the start of a step; distinct ids: no two workgroups touch
// the same parameter)
__global__ __launch_bounds__(256) void tables_scatter_kernel(const float* __restrict__ dc, float* __restrict__ dwb, int64_t ws,
                                                             float* __restrict__ dbb, int64_t bs, float* __restrict__ dve,
                                                             const int* __restrict__ ids, int D) {
  const int v = blockIdx.x, id = ids[v];
  float* dw = dwb + (int64_t)id * ws;
  float* db = dbb + (int64_t)id * bs;
  float* de = dve + (int64_t)id * D;
  const float* g = dc + (size_t)v * 5 * D;
  for (int d = threadIdx.x; d < D; d += 256) {
    f32x4 w4 = *reinterpret_cast<const f32x4*>(dw + (size_t)d * 4);
    w4[0] += g[d]; w4[1] += g[D + d]; w4[2] += g[2 * D + d]; w4[3] += g[3 * D + d];
    *reinterpret_cast<f32x4*>(dw + (size_t)d * 4) = w4;
    const float gb = g[4 * D + d];
    db[d] += gb;
    de[d] += gb;
  }
}
}  // namespace

extern "C" int orbit2_tables_gather(const float* w_base, int64_t w_stride, const float* b_base, int64_t b_stride,
                                    const float* var_embed, const int* ids, float* cmat, int V, int D, void* stream) {
  if (!w_base || !b_base || !var_embed || !ids || !cmat || V <= 0 || D <= 0) return O2_ERR_ARG;
  if (((uintptr_t)w_base & 15) || (w_stride & 3)) return O2_ERR_ARG;          // 16-byte rows of four patch weights
  hipLaunchKernelGGL(tables_gather_kernel, dim3(V), dim3(256), 0, (hipStream_t)stream, w_base, w_stride, b_base, b_stride, var_embed,
                     ids, cmat, D);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_tables_scatter(const float* dcmat, float* dw_base, int64_t w_stride, float* db_base, int64_t b_stride,
                                     float* dvar_embed, const int* ids, int V, int D, void* stream) {
  if (!dcmat || !dw_base || !db_base || !dvar_embed || !ids || V <= 0 || D <= 0) return O2_ERR_ARG;
  if (((uintptr_t)dw_base & 15) || (w_stride & 3)) return O2_ERR_ARG;
  hipLaunchKernelGGL(tables_scatter_kernel, dim3(V), dim3(256), 0, (hipStream_t)stream, dcmat, dw_base, w_stride, db_base, b_stride,
                     dvar_embed, ids, D);
  O2_CHECK_LAUNCH();
  return O2_OK;
}
