// fp32 forward path (inference / evaluation in true float32): GEMM with fused epilogue and the attention core, both on the
// f32-input MFMA v_mfma_f32_32x32x2_f32 (exact fp32: every product rounded once, fp32 accumulate).  Forward only.
//
// Operand lane map of the 32x32x2 form: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; the result has
// its column j on the lane and row i = (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r.  Both kernels read their K-contiguous
// operands from LDS as one float4 per lane at k = 8 kb + 4 (l >> 5) .. + 3 and spend element e on MFMA e of the group: the
// contraction index of MFMA e is then {8 kb + e, 8 kb + 4 + e}, the same on the A and the B side, so the sum is complete and
// only its order differs from 0, 1, 2, ...  
#include "common.h"
#include "../../include/orbit2_hip.h"

namespace {

constexpr int F32_BK = 32;             // contraction depth of an LDS tile
constexpr int F32_LDK = F32_BK + 4;    // LDS row pitch (floats): rows 144 B apart put the 16 lanes of a ds_read_b128 phase on 64 distinct banks

struct GemmF32P {
  const float* A; const float* B; float* C;
  const float* bias; const float* residual;
  int M, N, K, lda, ldb, ldc, ldr, res_mod, act, colscale_n;
  float colscale, beta;
};

// C[M,N] = epilogue(A[M][lda] x B[N][ldb]^T).  256 threads = 2 x 2 waves, each wave (BM/2) x (BN/2) as TM x TN tiles of 32 x 32
// (TM * TN independent accumulator chains).  Global -> registers -> LDS, the next tile's loads in flight during the MFMAs.
template <int BM, int BN>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const GemmF32P p) {
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int LA = BM / 32, LB = BN / 32;            // float4 loads per thread and tile
  __shared__ __attribute__((aligned(16))) float As[BM * F32_LDK];
  __shared__ __attribute__((aligned(16))) float Bs[BN * F32_LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hl = lane >> 5;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int lrow = tid >> 3, lc4 = (tid & 7) * 4;

  const float* ap[LA];
  const float* bp[LB];
#pragma unroll
  for (int i = 0; i < LA; ++i) ap[i] = p.A + (size_t)min(m0 + lrow + i * 32, p.M - 1) * p.lda + lc4;     // rows past M: clamped, never stored
#pragma unroll
  for (int i = 0; i < LB; ++i) bp[i] = p.B + (size_t)min(n0 + lrow + i * 32, p.N - 1) * p.ldb + lc4;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 ra[LA], rb[LB];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int nk = (p.K + F32_BK - 1) / F32_BK;
  {
    const bool in = lc4 < p.K;                         // K % 4 == 0: a float4 is inside or outside as a whole
#pragma unroll
    for (int i = 0; i < LA; ++i) ra[i] = in ? *reinterpret_cast<const f32x4*>(ap[i]) : zero4;
#pragma unroll
    for (int i = 0; i < LB; ++i) rb[i] = in ? *reinterpret_cast<const f32x4*>(bp[i]) : zero4;
  }
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int i = 0; i < LA; ++i) *reinterpret_cast<f32x4*>(&As[(lrow + i * 32) * F32_LDK + lc4]) = ra[i];
#pragma unroll
    for (int i = 0; i < LB; ++i) *reinterpret_cast<f32x4*>(&Bs[(lrow + i * 32) * F32_LDK + lc4]) = rb[i];
    __syncthreads();
    if (kt + 1 < nk) {
      const int k1 = (kt + 1) * F32_BK;
      const bool in = k1 + lc4 < p.K;
#pragma unroll
      for (int i = 0; i < LA; ++i) ra[i] = in ? *reinterpret_cast<const f32x4*>(ap[i] + k1) : zero4;
#pragma unroll
      for (int i = 0; i < LB; ++i) rb[i] = in ? *reinterpret_cast<const f32x4*>(bp[i] + k1) : zero4;
    }
#pragma unroll
    for (int kb = 0; kb < F32_BK / 8; ++kb) {
      f32x4 a4[TM], b4[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a4[i] = *reinterpret_cast<const f32x4*>(&As[(wm * (BM / 2) + i * 32 + l31) * F32_LDK + kb * 8 + hl * 4]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        b4[j] = *reinterpret_cast<const f32x4*>(&Bs[(wn * (BN / 2) + j * 32 + l31) * F32_LDK + kb * 8 + hl * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][e], b4[j][e], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: +bias -> *colscale (n < colscale_n) -> GELU -> +residual[m % res_mod] -> C = beta*C + v   (the header's order with
  // drop_p = 0, where res_first makes no difference).  A register holds one row of 32 consecutive columns across the lanes.
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * (BN / 2) + j * 32 + l31;
    if (n >= p.N) continue;
    const float bv = p.bias ? p.bias[n] : 0.f;
    const float cs = n < p.colscale_n ? p.colscale : 1.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
        if (m >= p.M) continue;
        float v = acc[i][j][r] + bv;
        if (n < p.colscale_n) v *= cs;
        if (p.act == 1) v = gelu_f(v);
        if (p.residual) v += p.residual[(size_t)(p.res_mod > 0 ? m % p.res_mod : m) * p.ldr + n];
        float* c = p.C + (size_t)m * p.ldc + n;
        if (p.beta != 0.f) v = fmaf(p.beta, *c, v);
        *c = v;
      }
    }
  }
}

// ---- attention forward, fp32 ---------------------------------------------------------------------------------------------
// One workgroup = 4 waves x 32 query rows of one (batch, head); key tiles of 32 shared through LDS.  Transposed formulation
// with the QUERY on the MFMA lane: S^T = K Q^T (A = K tile from LDS, B = the wave's Q rows, register-resident), so lane
// (q, hl) holds in register r the score of key (r & 3) + 8 (r >> 2) + 4 hl -- which is exactly the B operand P^T[k = hl][q] of
// O^T += V^T P^T when MFMA t of the second product contracts over the key pair {kt(0), kt(1)} = {(t & 3) + 8 (t >> 2), .. + 4}
// and the A operand reads V[kt(hl)][column] from LDS.  P goes from the first product's accumulator into the second product
// as it is: no LDS round trip, no lane movement.  The softmax statistics of a query live on its lane (two halves, one shuffle).
template <int D>
struct AttnF32Cfg {
  static constexpr int LDK = D + 4;       // K rows: float4 reads, 16 lanes on 64 distinct banks
  static constexpr int LDV = D + 8;       // V rows: b32 reads, the two lane halves (rows 4 apart) 32 banks apart
  static constexpr int NL = D / 32;       // float4 loads per thread, tile and matrix
  static constexpr bool PREFETCH = D <= 128;
  static constexpr size_t LDS_BYTES = sizeof(float) * 32 * (LDK + LDV);
};

template <int D>
__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                           float* __restrict__ lse, int L, int H, int ldq, int ldo,
                                                           float qmul) {
  using C = AttnF32Cfg<D>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* Ks = sm;
  float* Vs = sm + 32 * C::LDK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hl = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * 128 + wave * 32 + l31;
  const int qc = min(q, L - 1);                                    // rows past L: clamped loads, no stores
  const float* base = qkv + (size_t)b * L * ldq + (size_t)head * D;
  const float* kbase = base + (size_t)H * D;
  const float* vbase = base + 2 * (size_t)H * D;

  f32x4 q4[D / 8];
  {
    const float* qr = base + (size_t)qc * ldq + hl * 4;
#pragma unroll
    for (int kb = 0; kb < D / 8; ++kb) q4[kb] = *reinterpret_cast<const f32x4*>(qr + kb * 8) * qmul;
  }
  f32x16 o[D / 32];
#pragma unroll
  for (int dc = 0; dc < D / 32; ++dc)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dc][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 rk[C::NL], rv[C::NL];
  auto load_tile = [&](int key0) {
#pragma unroll
    for (int i = 0; i < C::NL; ++i) {
      const int idx = tid + i * 256, row = idx / (D / 4), c4 = (idx % (D / 4)) * 4;
      const int key = key0 + row;
      const bool in = key < L;                                      // keys past L: zero V rows (0 x finite), masked scores
      rk[i] = in ? *reinterpret_cast<const f32x4*>(kbase + (size_t)key * ldq + c4) : zero4;
      rv[i] = in ? *reinterpret_cast<const f32x4*>(vbase + (size_t)key * ldq + c4) : zero4;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < C::NL; ++i) {
      const int idx = tid + i * 256, row = idx / (D / 4), c4 = (idx % (D / 4)) * 4;
      *reinterpret_cast<f32x4*>(&Ks[row * C::LDK + c4]) = rk[i];
      *reinterpret_cast<f32x4*>(&Vs[row * C::LDV + c4]) = rv[i];
    }
  };

  if (C::PREFETCH) load_tile(0);
  for (int key0 = 0; key0 < L; key0 += 32) {
    if (!C::PREFETCH) load_tile(key0);
    store_tile();
    __syncthreads();
    if (C::PREFETCH && key0 + 32 < L) load_tile(key0 + 32);

    // two partial sums over the head dim (even / odd groups of 8), added once: half the length of the sequential fmaf chain
    // (its rounding error grows with the chain, and scores of tens of nats turn it into output error), same MFMA count
    f32x16 s, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = s1[r] = 0.f;
#pragma unroll
    for (int kb = 0; kb < D / 8; kb += 2) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(&Ks[l31 * C::LDK + kb * 8 + hl * 4]);
      const f32x4 k5 = *reinterpret_cast<const f32x4*>(&Ks[l31 * C::LDK + kb * 8 + 8 + hl * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4[e], q4[kb][e], s, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k5[e], q4[kb + 1][e], s1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] += s1[r];
    // streaming softmax in the exp2 domain (q carries log2(e) / sqrt(d))
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * hl;
      s[r] = key < L ? s[r] : -INFINITY;
      mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);        // finite: key0 < L, so every tile has a valid key
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = __builtin_amdgcn_exp2f(s[r] - m_new); ps += s[r]; }
    l_run = fmaf(l_run, alpha, ps);              // this lane half's part of the row sum; the halves are added at the end
    m_run = m_new;
#pragma unroll
    for (int dc = 0; dc < D / 32; ++dc) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dc][r] *= alpha;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const float* vr = &Vs[((t & 3) + 8 * (t >> 2) + 4 * hl) * C::LDV + l31];
#pragma unroll
      for (int dc = 0; dc < D / 32; ++dc) o[dc] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[dc * 32], s[t], o[dc], 0, 0, 0);
    }
    __syncthreads();
  }

  const float l_tot = l_run + __shfl_xor(l_run, 32);
  if (q >= L) return;
  if (hl == 0) lse[((size_t)b * H + head) * L + q] = (m_run + log2f(l_tot)) * 0.6931471805599453f;
  const float inv = 1.0f / l_tot;
  float* orow = out + ((size_t)b * L + q) * (size_t)ldo + (size_t)head * D + hl * 4;
  // O^T tile dc: register r = column dc * 32 + (r & 3) + 8 (r >> 2) + 4 hl of this lane's query row
#pragma unroll
  for (int dc = 0; dc < D / 32; ++dc)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = {o[dc][4 * g] * inv, o[dc][4 * g + 1] * inv, o[dc][4 * g + 2] * inv, o[dc][4 * g + 3] * inv};
      *reinterpret_cast<f32x4*>(orow + dc * 32 + g * 8) = v;
    }
}

template <int D>
int attn_f32_launch(const float* qkv, float* out, float* lse, int B, int L, int H, int ldq, int ldo, float qmul,
                    hipStream_t st) {
  using C = AttnF32Cfg<D>;
  static bool attr_set = false;       // > 48 KiB of dynamic LDS needs the attribute once per process (idempotent: a race repeats it)
  if (C::LDS_BYTES > 48 * 1024 && !attr_set) {
    if (hipFuncSetAttribute((const void*)attn_fwd_f32_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)C::LDS_BYTES) != hipSuccess)
      return O2_ERR_LAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(attn_fwd_f32_kernel<D>, dim3((L + 127) / 128, H, B), dim3(256), C::LDS_BYTES, st, qkv, out, lse, L, H,
                     ldq, ldo, qmul);
  O2_CHECK_LAUNCH();
  return O2_OK;
}

}  // namespace

extern "C" int orbit2_gemm_f32(const orbit2_gemm_args* a, void* stream) {
  if (!a || !a->A || !a->B || !a->C) return O2_ERR_ARG;
  if (a->M <= 0 || a->N <= 0 || a->K <= 0) return O2_ERR_ARG;
  // what this kernel does not implement is refused before any launch, never ignored
  if (a->a_kc != 1 || a->b_kc != 1) return O2_ERR_UNSUPPORTED;                  // forward form only
  if (a->drop_p != 0.f || a->save_pre || a->save_dact || a->mul || a->dgelu_pre || a->rowscale || a->colsum_ws)
    return O2_ERR_UNSUPPORTED;
  if (a->act != 0 && a->act != 1) return O2_ERR_UNSUPPORTED;
  if (a->out_fp32 != 1) return O2_ERR_UNSUPPORTED;                              // C is fp32, and the caller has to say so
  if (a->tile_hint != 0 && a->tile_hint != 64 && a->tile_hint != 128) return O2_ERR_UNSUPPORTED;
  if ((a->N & 3) || (a->K & 3) || (a->lda & 3) || (a->ldb & 3) || (a->ldc & 3)) return O2_ERR_ARG;
  if (a->lda < a->K || a->ldb < a->K || a->ldc < a->N) return O2_ERR_ARG;
  if (((uintptr_t)a->A | (uintptr_t)a->B | (uintptr_t)a->C) & 15) return O2_ERR_ARG;
  if (a->colscale_n < 0 || a->colscale_n > a->N || (a->colscale_n & 3)) return O2_ERR_ARG;
  if (a->residual && (a->ldr < a->N || a->res_mod < 0)) return O2_ERR_ARG;
  GemmF32P p;
  p.A = (const float*)a->A; p.B = (const float*)a->B; p.C = (float*)a->C;
  p.bias = (const float*)a->bias; p.residual = (const float*)a->residual;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc; p.ldr = a->ldr; p.res_mod = a->res_mod;
  p.act = a->act; p.colscale_n = a->colscale_n; p.colscale = a->colscale; p.beta = a->beta;
  // 128 x 128 tiles (four accumulator chains per wave) when they give every CU a workgroup; 64 x 64 tiles for narrow or small
  // problems (the head's last layer, a few hundred tokens)
  int tile = a->tile_hint;
  if (tile == 0) {
    const long t128 = (long)((a->M + 127) / 128) * ((a->N + 127) / 128);
    tile = (a->N <= 64 || a->M <= 64 || t128 < 256) ? 64 : 128;
  }
  const hipStream_t st = (hipStream_t)stream;
  if (tile == 128) {
    const dim3 grid((a->N + 127) / 128, (a->M + 127) / 128);
    if (grid.y > 65535) return O2_ERR_ARG;
    hipLaunchKernelGGL((gemm_f32_kernel<128, 128>), grid, dim3(256), 0, st, p);
  } else {
    const dim3 grid((a->N + 63) / 64, (a->M + 63) / 64);
    if (grid.y > 65535) return O2_ERR_ARG;
    hipLaunchKernelGGL((gemm_f32_kernel<64, 64>), grid, dim3(256), 0, st, p);
  }
  O2_CHECK_LAUNCH();
  return O2_OK;
}

extern "C" int orbit2_attn_fwd_f32(const void* qkv, void* out, float* lse, int B, int L, int H, int d, float drop_p,
                                   uint64_t seed, int flags, int ldq, int ldo, void* stream) {
  (void)seed;
  if (!qkv || !out || !lse || B <= 0 || L <= 0 || H <= 0) return O2_ERR_ARG;
  if (drop_p != 0.f) return O2_ERR_UNSUPPORTED;                                 // no fp32 dropout (forward-only path)
  if (d != 64 && d != 128 && d != 256) return O2_ERR_UNSUPPORTED;
  if (flags & ~ORBIT2_ATTN_Q_PRESCALED) return O2_ERR_UNSUPPORTED;              // the bf16 kernels' variant flags mean nothing here
  if (ldq < 3 * H * d || ldo < H * d || (ldq & 3) || (ldo & 3)) return O2_ERR_ARG;
  if (((uintptr_t)qkv | (uintptr_t)out) & 15) return O2_ERR_ARG;
  if (H > 65535 || B > 65535) return O2_ERR_ARG;
  const float qmul = (flags & ORBIT2_ATTN_Q_PRESCALED) ? 1.0f : 1.4426950408889634f / sqrtf((float)d);
  const hipStream_t st = (hipStream_t)stream;
  const float* x = (const float*)qkv;
  float* y = (float*)out;
  if (d == 64) return attn_f32_launch<64>(x, y, lse, B, L, H, ldq, ldo, qmul, st);
  if (d == 128) return attn_f32_launch<128>(x, y, lse, B, L, H, ldq, ldo, qmul, st);
  return attn_f32_launch<256>(x, y, lse, B, L, H, ldq, ldo, qmul, st);
}
