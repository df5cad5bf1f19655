/* liborbit2_hip.so -- C ABI of the MI355X-native (gfx950) hot path of ORBIT-2's
 * intermediate_downscaling training step (Res_Slim_ViT forward/backward + losses + AdamW).
 *
 * The reference (/root/reference) is 100 % Python and has no FFI seam; its operator seams are
 * the nn.Module forward()s and the FusedAttn switch.  Each entry point below names the reference
 * interface (file:line, relative to /root/reference) whose arithmetic it replaces.
 *
 * Conventions: every pointer is caller-owned DEVICE memory, row-major contiguous
 * unless a leading dimension is given; bf16 tensors are raw uint16; no allocation, no sync;
 * asynchronous on `stream` (a hipStream_t passed as void*); returns 0 on success, <0 on error
 * (never throws).  RNG = counter-based hash of (seed, element index) -- the caller advances
 * `seed` per call site and per step.
 *
 * State: the library keeps NO host-side mutable state and exactly ONE piece of device-side
 * mutable state, the 64-bit seed salt written by orbit2_seed_salt() (see there): one value per
 * device per process, 0 unless set, read by every seeded kernel on every stream.  Everything else
 * a call touches is passed in.  Calls are re-entrant across streams and threads as long as no
 * call that WRITES the salt is in flight concurrently with seeded kernels of another stream whose
 * forward and backward must agree (the salt is read at kernel run time, not at launch).
 */
#ifndef ORBIT2_HIP_H
#define ORBIT2_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORBIT2_ABI_VERSION 8
/* Version 8: orbit2_gemm_bf16, orbit2_gemm_bf16_grouped, orbit2_attn_fwd_ld and orbit2_attn_bwd_ld take the path gate and the tail
 * queue as ARGUMENTS; the _gated and _tq entries that version 7 had beside them are gone.  A version-7 build exports the same
 * four names with shorter argument lists, so the number had to change: a binding of one version refuses a build of the other.
 * Everything else is as at version 7, the entries that were added during it included (the fp32 forward entries orbit2_gemm_f32,
 * orbit2_attn_fwd_f32, orbit2_layernorm_fwd_f32, orbit2_varagg_fwd_f32, orbit2_unpatchify_fwd_f32; orbit2_ensemble_update and
 * orbit2_gaussian_scores).  Added during version 8, changing nothing that exists: orbit2_ensemble_scores; the folded patch-embed
 * entries that carry the patch size (orbit2_varagg_fwd_p, orbit2_varagg_fwd_f32_p, orbit2_varagg_bwd_p and its two queries);
 * orbit2_ssim; orbit2_resample_fwd and orbit2_resample_moments; the mode values 5 and 6 of those two (bilinear and bicubic with
 * ORBIT2_ANTIALIAS), which earlier builds of version 8 refuse with O2_ERR_ARG; the mode values 21 and 22 of orbit2_resample_fwd
 * (those two with ORBIT2_TRANSPOSE: the adjoint of the coarsening), which earlier builds of version 8 refuse as well; the kind
 * value 3 of orbit2_loss_bwd (ORBIT2_LOSS_SSIM_VJP: the backward of orbit2_ssim's sums), which earlier builds refuse too; the
 * kinds 3 and 4 of orbit2_masked_loss_fwd with the flag and count bits of its kind word (ORBIT2_MASKED_QUANTILES,
 * ORBIT2_MASKED_TAIL: exact field quantiles and tail sums), which earlier builds refuse with O2_ERR_ARG as well; the kind 5 of
 * that entry with the window bits 16-23 of its kind word (ORBIT2_FSS_KIND: the fractions skill score), refused by earlier builds
 * in the same way. */
int orbit2_abi_version(void);

/* ---- bf16 MFMA GEMM with fused epilogue ------------------------------------------------
 * C[M,N] = epilogue( sum_k A(m,k) * B(n,k) ),   fp32 accumulate.
 * a_kc=1: A stored [M][lda] (K contiguous);  a_kc=0: A stored [K][lda] (M contiguous).
 * b_kc=1: B stored [N][ldb] (K contiguous);  b_kc=0: B stored [K][ldb] (N contiguous).
 * Replaces every nn.Linear on the path: attention.py:36,40,50,81; mlp.py:50,54,63,67;
 * res_slimvit.py:115-120,326 (head); var_agg.proj attention.py:129,177 -- forward (a_kc=b_kc=1),
 * input-gradient (a_kc=1,b_kc=0) and weight-gradient (a_kc=b_kc=0) forms.
 * Epilogue order: +bias -> *colscale (columns n < colscale_n) -> save_pre -> GELU -> [+residual if res_first] -> dropout
 *   [-> save_dact] -> *gelu'(dgelu_pre) -> *mul -> *rowscale[m / rows_per_scale] -> [+residual] -> C = beta*C + v.
 * Requirements: N % 8 == 0; M % 8 == 0 unless a_kc (any M then); K % 8 == 0 if an operand is K-contiguous, any K when
 * both are K-strided (the weight-gradient form: K = tokens); lda/ldb/ldc % 8 == 0, 16-byte aligned bases. */
typedef struct {
  const void* A; const void* B; void* C;
  int M, N, K;
  int lda, ldb, ldc;
  int a_kc, b_kc;
  const void* bias;        /* bf16 [N] or NULL */
  int act;                 /* 0 none, 1 GELU(erf)  (nn.GELU default, mlp.py:64), 2 ReLU (VGG16 convs of LPIPS) */
  void* save_pre;          /* bf16 [M][ldc] pre-activation copy, or NULL */
  const void* dgelu_pre;   /* bf16 [M][ldc]: multiply by GELU'(pre), or NULL */
  float drop_p;            /* nn.Dropout on the output element (attention.py:82, mlp.py:65,68) */
  uint64_t seed;
  const float* rowscale;   /* DropPath (vit_blocks.py:78-79): fp32 [M / rows_per_scale], or NULL */
  int rows_per_scale;
  const void* residual;    /* bf16 [res_mod][ldr] added at row (m % res_mod), or NULL */
  int ldr, res_mod, res_first;
  int out_fp32;            /* 0: C is bf16, 1: C is fp32 */
  float beta;              /* C = beta*C + result (gradient accumulation) */
  int tile_hint;           /* 0 = auto; tests / tuning: 128 = 128-tile kernel on 128 x 128 tiles, 64 = the same kernel on 64-row tiles
                              (A K-contiguous; auto takes them when the 128 x 128 grid is under two tiles per CU), 256 = 8-wave 8-phase kernel (K % 64 == 0),
                              260 = 4-wave kernel (M, N % 256 == 0, K % 64 == 0), 262 = 4-wave kernel with the runtime epilogue in
                              place of the compile-time kinds; also accepted: 257, 258 = 256 (hints of older A/B tools), 261 = the stamped
                              form of 260 (O2_ERR_UNSUPPORTED unless built with O2_W4_STAMP); any other value = 0 */
  int colscale_n;          /* columns n < colscale_n (a multiple of 8; 0 = none) are multiplied by colscale in fp32 right after */
  float colscale;          /*   the bias: the qkv Linear stores q * log2(e)/sqrt(d) (attention.py:50,54: q * scale), rounded ONCE */
  void* save_dact;         /* int16 [M][ldc] or NULL (needs act == 1): GELU'(pre) x (kept ? 1 / (1 - p) : 0) of THIS element as signed
                              fixed point with 14 fraction bits, range [-2, 2), saturating (at drop_p = 0.1 the factor lies in
                              [-0.15, 1.26]: 3e-5 absolute, where bf16 would give 4e-3; drop_p >= 0.434, where 1.13 / (1 - p)
                              reaches 2, is refused with O2_ERR_UNSUPPORTED: use save_pre / dgelu_pre there) -- what the backward multiplies the input gradient by (autograd of mlp.py:64-65), computed
                              here, where the pre-activation and the dropout decision are in registers, instead of GELU' + the
                              mask again in the backward */
  const void* mul;         /* int16 q14 [M][ldc] or NULL: multiply the result elementwise (the backward's use of a save_dact tensor) */
  float* colsum_ws;        /* fp32 [orbit2_gemm_bf16_colsum_rows(args)][N] or NULL (ABI 5): row t receives the column sums of the STORED
                              (bf16-rounded) output over rows 256 t .. 256 t + 255 -- the bias gradient of the layer below a GELU
                              (autograd of mlp.py:50,63) without a second pass over the 3 GB tensor: add the rows (orbit2_colsum on the
                              workspace).  Only the multiply-by-factor input gradient on whole tiles fills it: a call for which
                              orbit2_gemm_bf16_colsum_rows returns 0 is refused with O2_ERR_UNSUPPORTED when colsum_ws is set */
} orbit2_gemm_args;
/* gate / rows_per_gate, the PATH GATE: gate = fp32 [ceil(M / rows_per_gate)] or NULL (none, whatever rows_per_gate is; a gate
 * with rows_per_gate <= 0: O2_ERR_ARG), entry e covering rows e * rows_per_gate onwards (the per-sample DropPath scales of a Block
 * and its token count: vit_blocks.py:77,80 / timm DropPath).  gate[e] == 0.0f says that everything computed from these rows is
 * multiplied by 0 further down the branch.  The gate is a HINT: an output tile whose rows all lie in one such entry MAY skip its
 * contraction and epilogue and store what annihilated inputs give -- zeros in C, save_pre, save_dact and its colsum_ws row; the
 * residual rows when rowscale == gate and rows_per_scale == rows_per_gate (the row scale would have multiplied the product by 0)
 * -- so nothing a later kernel reads is left unwritten.  A tile that straddles entries, a kernel family without the check (today
 * every family but the 4-wave 256 x 256 kernel) and an epilogue outside that list (fp32 output, beta, another row scale) compute
 * as without a gate; kept rows are bit-identical, and the kernel, grid and block are those of the ungated call
 * (orbit2_gemm_bf16_colsum_rows answers for both).
 * sched_ws / tail, the TAIL QUEUE (csrc/tail_queue.h) of the one-workgroup-per-CU kernels (the 4-wave 256 x 256 GEMM,
 * single and grouped; the generated d = 128 attention kernels): their LAST ROUNDS of tiles handed out by ticket instead of by
 * workgroup number.  Workgroup b always runs on XCD b & 7, so a static walk ends when the slowest XCD ends; here an XCD that gets
 * to the tail first takes more of it.  The first T - tail tiles keep their static ids; 2 * tail further workgroups each draw one
 * ticket (one relaxed agent-scope atomic) and either take one of the last `tail` tiles or return.  No workgroup waits.  Every tile
 * computes what it computes in a static launch: the results are bit-identical.
 *   tail: < 0 = static, sched_ws is not read and may be NULL -- the plain call is (gate = NULL, 0, sched_ws = NULL, tail = -1);
 *     0 = sized by the library per kernel family (0, 2 or 4 whole rounds of the device's 256 workgroup slots, from
 *     profiles/r08_tail_idle.txt; a launch that would keep fewer than 4 static rounds in front of its tail, and any device that
 *     is not 256 CUs on 8 XCDs, stay static); > 0 = that many tiles (tests: small problems with a queued part; more than the
 *     launch has: static).
 *   sched_ws: one 32-bit device word (4-byte aligned, or O2_ERR_ARG at any tail), ZERO before the call; the launch leaves it zero
 *     (the drawer of the last ticket clears it), so back-to-back calls on one stream and replays of a captured graph reuse it as
 *     it is.  Calls that may run at the same time (different streams) need different words.  A launch aborted half-way leaves the
 *     number of tickets drawn so far: zero the word before it is used again.  NULL with tail >= 0: O2_ERR_ARG before any launch.
 * A call whose plan is another kernel family launches exactly what the static call launches. */
int orbit2_gemm_bf16(const orbit2_gemm_args* args, const float* gate, int rows_per_gate, void* sched_ws, int tail, void* stream);
int orbit2_gemm_bf16_colsum_rows(const orbit2_gemm_args* args);   /* 0: this call cannot fuse the column sums (colsum_ws must be NULL) */

/* ---- fp32 GEMM with fused epilogue (the fp32 forward path) ---------------------------------
 * The same argument block with EVERY tensor pointer (A, B, C, bias, residual) read as fp32; out_fp32 must be 1.  fp32 operands,
 * fp32 accumulate on v_mfma_f32_32x32x2_f32 (every product rounded once; the contraction is summed within groups of 8 in the order
 * 0, 4, 1, 5, 2, 6, 3, 7), fp32 out.  Replaces the same nn.Linear forwards as orbit2_gemm_bf16 when the reference runs with
 * trainer.data_type: float32 (examples/intermediate_downscaling.py:593-607; examples/visualize.py:251 hard-codes it): attention.py:36,40,
 * 50,81; mlp.py:50,54,63,67; res_slimvit.py:115-120,326; attention.py:129,177.  B is the fp32 master weight [N][ldb] as stored.
 * Implemented: a_kc = b_kc = 1; any M; N, K, lda, ldb, ldc % 4 == 0; 16-byte aligned bases; bias, colscale / colscale_n (% 4), act 0 / 1,
 * residual with ldr / res_mod / res_first, beta; tile_hint 0 (auto), 64 (64 x 64 tiles), 128 (128 x 128 tiles).
 * Everything else (other operand forms, drop_p != 0, save_pre, save_dact, mul, dgelu_pre, rowscale, colsum_ws, act 2, out_fp32 = 0,
 * other tile_hint values) returns O2_ERR_UNSUPPORTED (-3) before any launch. */
int orbit2_gemm_f32(const orbit2_gemm_args* args, void* stream);

/* n (<= ORBIT2_GEMM_MAX_GROUP) independent problems of ONE operand form (same a_kc, b_kc) in one launch (the 256x256
 * 8-phase kernel when every problem has K % 64 == 0, M, N >= 256 and the group fills the chip; the 128x128 kernel
 * otherwise): the partially filled last round of each problem is filled with the next one's tiles.  Used for
 * the four weight-gradient GEMMs of a Block (reference: autograd of attention.py:36,40 + mlp.py:50,54).
 * Up to 12 problems (since ABI 7), so that a caller can hand over the tiles beyond the group's last whole round of 256 as
 * part-length problems over slices of the contraction (the Python layer's balanced weight-gradient launch: 3 full problems +
 * 2 x 4 quarter-length ones, partial products summed by orbit2_batch_sum).  When every problem sweeps >= 512 K-tiles of 64 the
 * workgroups of an XCD start their tiles together
 * (a bounded wait on a self-cleaning counter in a static device array: a pacing hint, never needed for correctness;
 * ORBIT2_W4_PACE = 0 / 1 / 2: off / on (default) / plus check points inside the sweep).
 * kgates / k_per_gate, a K GATE per problem (weight gradients dW = dY^T . X, a_kc = b_kc = 0); either NULL: none.  kgates[i] =
 * fp32 [K_i / k_per_gate[i]] or NULL, entry e covering rows e * k_per_gate[i] onwards of problem i's contraction (the tokens of
 * one sample; for a problem over a slice of the tokens, the entries of that slice).  kgates[i][e] == 0.0f says that those rows of
 * dY are ZEROS (the path gate of orbit2_gemm_bf16 left them so): the 4-wave kernel sweeps the kept ranges only.  A hint like the
 * path gate: other kernel families, other operand forms and entries that are not whole 64-deep K-tiles ignore it; the products
 * are the same (a skipped range adds zeros).
 * sched_ws / tail: the tail queue, as in orbit2_gemm_bf16 (the plain call: kgates = k_per_gate = sched_ws = NULL, tail = -1). */
#define ORBIT2_GEMM_MAX_GROUP 12
int orbit2_gemm_bf16_grouped(const orbit2_gemm_args* args, int n, const float* const* kgates, const int* k_per_gate,
                             void* sched_ws, int tail, void* stream);

/* small fp32 GEMM (parameter-table algebra of the folded variable aggregation):
 * C[M,N] = alpha * op(A) * op(B) + beta*C, row-major fp32; ta/tb: 0 = as stored, 1 = transposed.
 * ws: caller-owned fp32 workspace of orbit2_sgemm_f32_ws_floats(M,N,K) floats: skinny problems (a few rows against a D x D
 * weight) are split over K into ws_floats / (M*N) slabs and combined deterministically; 0 floats = no split is planned (ws may
 * then be NULL) */
int64_t orbit2_sgemm_f32_ws_floats(int M, int N, int K);
int orbit2_sgemm_f32_ws(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                        int ta, int tb, float alpha, float beta, float* ws, int64_t ws_floats, void* stream);

/* ---- LayerNorm (vit_blocks.py:46,63; res_slimvit.py:104,294): eps 1e-5, affine ------------ */
/* y has a row pitch (ldy >= D elements, a multiple of 8; ldy = D: contiguous): the output is the A operand of the next GEMM, and
 * rows a multiple of 8 KiB apart (D % 4096 == 0: interm_10b) put every row's k-offset on one memory channel */
int orbit2_layernorm_fwd_ld(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                            int rows, int D, int ldy, float eps, void* stream);
/* the same with fp32 x, gamma, beta, y (vit_blocks.py:46,63; res_slimvit.py:104,294 under data_type float32): D, ldy % 4 == 0,
 * two-pass variance; mean / rstd may be NULL (nothing reads them without a backward) */
int orbit2_layernorm_fwd_f32(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                             int rows, int D, int ldy, float eps, void* stream);
/* dx = LN'(dy) [+ dres];  dgamma/dbeta: bf16 or fp32 [D] (beta_acc accumulates).  ws: fp32 >= 2*D*nblk */
int orbit2_layernorm_bwd(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                         const void* dres, void* dx, void* dgamma, void* dbeta, int grads_fp32, float beta_acc,
                         float* ws, int ws_floats, int rows, int D, void* stream);
int orbit2_layernorm_bwd_ws_floats(int rows, int D);

/* ---- multi-head self-attention core (attention.py:54-78): softmax(q k^T / sqrt(d)) v --------
 * qkv: bf16 [B, L, 3, H, d] (the qkv Linear output as stored, no permute copies);
 * out: bf16 [B, L, H, d]; lse: fp32 [B, H, L].  d in {64, 128, 256}; any L >= 1 (ragged tails are masked).
 * drop_p: dropout on P (attention.py:57,69,76).
 * dqkv: bf16 [B, L, 3, H, d];  delta: fp32 workspace of orbit2_attn_bwd_ws_floats(B, L, H) floats (two per-row statistics
 * tables, -lse log2(e) and -rowsum(dO o O) / dropout scale, padded per (b, h): the dK / dV kernels copy their tiles of it into
 * LDS by LDS-DMA) */
int64_t orbit2_attn_bwd_ws_floats(int B, int L, int H);
/* flags: the kernel variant as an ARGUMENT (0 = the default kernels; A/B timing and the bit-equality tests of the fused
 * d = 128 dK+dV pass).  Nothing on the launch path reads the environment or any other process-global switch. */
#define ORBIT2_ATTN_4WAVES 1     /* 4-wave / 128-row workgroups (round-1 geometry) instead of 8-wave / 256-row ones */
#define ORBIT2_ATTN_SPLIT_DKV 2  /* d = 128: dK and dV as two passes instead of the fused one */
/* The q third of qkv already holds q * log2(e)/sqrt(d) (written so by the qkv GEMM's colscale epilogue: ONE rounding to
 * bf16, products with k exact, like the reference's fp32 scaling of q k^T).  Without the flag the kernels multiply their
 * register-resident operand (q, or k in the dK/dV pass) by that factor themselves and round it to bf16 a second time
 * (relative 2^-9 per element of that operand: harmless at ordinary score magnitudes, ~1e-2 of the output when scores reach
 * tens of nats).  dqkv is in both cases the gradient with respect to the UNSCALED q, k, v. */
#define ORBIT2_ATTN_Q_PRESCALED 4
/* Forward and the dQ pass of the backward at d = 128 with ORBIT2_ATTN_Q_PRESCALED and L a multiple of 256 (<= 16384) run the
 * generated one-wave-per-SIMD kernels (csrc/attn_fwd_asm.h, attn_dq_asm.h; tools/gen_attn_fwd.py, gen_attn_dq.py); this flag
 * keeps the compiler-scheduled kernels instead (A/B timing, tests). */
#define ORBIT2_ATTN_NO_W4 8
/* Token-row pitches (elements, multiples of 8): qkv[b, l] and dqkv[b, l] start at (b * L + l) * ldq (ldq >= 3 * H * d),
 * out[b, l] at (b * L + l) * ldo (ldo >= H * d); the natural pitches ldq = 3 * H * d, ldo = H * d are the contiguous layouts
 * above.  These tensors are GEMM operands on the other side, and rows a multiple of 8 KiB apart put every row's k-offset on one
 * memory channel (see orbit2_layernorm_fwd_ld).  dout stays [B, L, H, d]. */
/* gate, the path gate (see orbit2_gemm_bf16): fp32 [B], one entry per sample, or NULL.  A workgroup of a sample with
 * gate[b] == 0.0f MAY skip its work and zero-fill what it owns: its rows of out and lse (forward), of the q third (dQ pass), of
 * the k and v thirds (dK + dV pass) of dqkv.  The generated d = 128 kernels implement it; every other kernel (and the statistics
 * pass) ignores the gate.
 * sched_ws / tail: the tail queue, as in orbit2_gemm_bf16 (the backward's dQ and dK + dV passes use the one word in turn); the
 * plain call is (gate = NULL, sched_ws = NULL, tail = -1). */
int orbit2_attn_fwd_ld(const void* qkv, void* out, float* lse, int B, int L, int H, int d, float drop_p,
                       uint64_t seed, int flags, int ldq, int ldo, const float* gate, void* sched_ws, int tail, void* stream);
int orbit2_attn_bwd_ld(const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                       void* dqkv, int B, int L, int H, int d, float drop_p, uint64_t seed, int flags, int ldq, int ldo,
                       const float* gate, void* sched_ws, int tail, void* stream);
/* orbit2_attn_fwd_ld with fp32 qkv / out (attention.py:54-78 under data_type float32, components/attention.py:66-70): streaming
 * softmax in fp32, both products on v_mfma_f32_32x32x2_f32.  ldq, ldo % 4 == 0.  No dropout: drop_p != 0 returns
 * O2_ERR_UNSUPPORTED, as does any flag other than ORBIT2_ATTN_Q_PRESCALED (honoured as above: without it the kernel multiplies
 * q by log2(e)/sqrt(d) in fp32 when it loads it). */
int orbit2_attn_fwd_f32(const void* qkv, void* out, float* lse, int B, int L, int H, int d, float drop_p,
                        uint64_t seed, int flags, int ldq, int ldo, void* stream);

/* ---- folded patch-embed + variable aggregation (res_slimvit.py:250-265, 205-230;
 *      patch_embed.py:44-52; attention.py:132-176) ---------------------------------------------
 * x: fp32 [B, V, h, w]; stab: fp32 [H][V][5] score table; gtab: fp32 [V][5][D] value table
 * (both functions of the weights only);  z: bf16 [B*L, D] (input of var_agg.proj);
 * attw: fp32 [B*L, H, V] softmax weights saved for backward.  The patch size is 2 (other sizes: the _p entries below). */
int orbit2_varagg_fwd(const float* x, const float* stab, const float* gtab, void* z, float* attw, int B, int V,
                      int h, int w, int H, int D, void* stream);
/* the same forward with z written as fp32 [B*L, D] (the fp32 forward path; same reference lines); attw may be NULL */
int orbit2_varagg_fwd_f32(const float* x, const float* stab, const float* gtab, float* z, float* attw, int B, int V,
                          int h, int w, int H, int D, void* stream);
/* dstab/dgtab are ACCUMULATED into (caller zeroes them).  ws: fp32 workspace of orbit2_varagg_bwd_ws_floats(...) floats (ABI 4):
 * every (head, token range) workgroup stores its partial tables in its own slab and the ranges are added in a fixed order --
 * no float atomics, bitwise reproducible. */
int64_t orbit2_varagg_bwd_ws_floats(int B, int V, int h, int w, int H, int D);
int orbit2_varagg_bwd(const float* x, const float* gtab, const float* attw, const void* dz, float* dstab,
                      float* dgtab, int B, int V, int h, int w, int H, int D, float* ws, void* stream);
/* The per-variable rows both tables are built from (ABI 6): cmat[(v, c)][D], c = 0..3 = the 2x2 patch-embed weight of variable
 * ids[v] transposed ([D][4] -> 4 rows), c = 4 = its bias + var_embed[ids[v]]  (res_slimvit.py:64-66 PatchEmbed x V, :182-201
 * var-embed gather, :251-262).  The V_total per-variable parameters are addressed as base + index * stride (elements): a caller
 * whose parameters lie at a uniform pitch (a flat parameter buffer) builds the rows in one launch; _scatter is the transpose and
 * ACCUMULATES into the gradient buffers at the same pitches (ids distinct). */
int orbit2_tables_gather(const float* w_base, int64_t w_stride, const float* b_base, int64_t b_stride, const float* var_embed,
                         const int* ids, float* cmat, int V, int D, void* stream);
int orbit2_tables_scatter(const float* dcmat, float* dw_base, int64_t w_stride, float* db_base, int64_t b_stride,
                          float* dvar_embed, const int* ids, int V, int D, void* stream);
/* 1 if orbit2_varagg_bwd sums the table gradients in a fixed order for this shape (bitwise reproducible), 0 if it takes the
 * scalar fallback that accumulates them with fp32 atomics (head dim not 64 / 128 / 256, 5 V > 128, ORBIT2_VARAGG_SCALAR set):
 * callers that keep replicas of the tables in lock-step without exchanging gradients need to know (dist/tp.py ReplicaGuard) */
int orbit2_varagg_bwd_is_fixed_order(int B, int V, int h, int w, int H, int D);
/* The same five calls with the patch size as an argument (components/patch_embed.py:22-53: PatchEmbed is generic in it).
 * patch in {1, 2, 4}, anything else is O2_ERR_ARG, as is a grid with h % patch or w % patch != 0.  With C = patch * patch + 1:
 * stab: fp32 [H][V][C], gtab: fp32 [V][C][D]; coefficient c < patch * patch multiplies patch element (c / patch, c % patch)
 * (row-major inside the patch: the order of Conv2d(1, D, patch, patch).weight.view(D, patch * patch)), c = patch * patch is the
 * constant term.  z: [B * (h / patch) * (w / patch), D] bf16 (_fwd_p) or fp32 (_fwd_f32_p, attw may be NULL); attw: fp32
 * [tokens, H, V]; dstab [H][V][C] and dgtab [V][C][D] are ACCUMULATED into.
 * patch == 2 IS the call above: same kernels, same launch, same workspace, same answer of _is_fixed_order.
 * patch 1 and 4: the forward kernels are the same template; the backward is a two-stage form of its own with NO float atomics
 * (ds per 16 tokens -> ws; then one workgroup per (variable, token range) holds its dgtab / dstab partial in registers and
 * stores it into the range's slab; the ranges are added in a fixed order).  orbit2_varagg_bwd_p_ws_floats = tokens * H * V +
 * ranges * (H V C + V C D) floats, 0 for a shape the backward does not serve; orbit2_varagg_bwd_p_is_fixed_order = 1 for every
 * shape it serves (bitwise reproducible), 0 otherwise.  A shape whose dynamic LDS need exceeds the 160 KiB of a CU is refused
 * with O2_ERR_UNSUPPORTED before anything is launched (backward: 16 * (V C + 2 H V + 512) floats, e.g. V = H = 32 at patch 4;
 * forward: 16 * (V C + H V) floats, within the limit for every V, H <= 32). */
int orbit2_varagg_fwd_p(const float* x, const float* stab, const float* gtab, void* z, float* attw, int B, int V, int h,
                        int w, int patch, int H, int D, void* stream);
int orbit2_varagg_fwd_f32_p(const float* x, const float* stab, const float* gtab, float* z, float* attw, int B, int V,
                            int h, int w, int patch, int H, int D, void* stream);
int64_t orbit2_varagg_bwd_p_ws_floats(int B, int V, int h, int w, int patch, int H, int D);
int orbit2_varagg_bwd_p(const float* x, const float* gtab, const float* attw, const void* dz, float* dstab, float* dgtab,
                        int B, int V, int h, int w, int patch, int H, int D, float* ws, void* stream);
int orbit2_varagg_bwd_p_is_fixed_order(int B, int V, int h, int w, int patch, int H, int D);

/* ---- elementwise / reductions ------------------------------------------------------------- */
/* dym = dy * dropmask * rowscale (backward of the dropout/DropPath epilogue); dym may alias dy */
int orbit2_dropout_bwd(const void* dy, void* dym, int M, int N, float drop_p, uint64_t seed, const float* rowscale,
                       int rows_per_scale, void* stream);
/* the same, fused with colsum_out[N] = beta*colsum_out + sum_m dym[m][n] (the bias gradient of the Linear whose output
 * gradient dym is: reference autograd of attention.py:40,80-82 / mlp.py:54,66-68): dym is not re-read from HBM; result
 * bit-identical to orbit2_dropout_bwd + orbit2_colsum.  ws: fp32 >= orbit2_colsum_ws_floats(M, N) */
int orbit2_dropout_bwd_colsum(const void* dy, void* dym, int M, int N, float drop_p, uint64_t seed, const float* rowscale,
                              int rows_per_scale, void* colsum_out, int out_fp32, float beta, float* ws, int ws_floats,
                              void* stream);
/* y = residual + rowscale[m/rows_per_scale] * dropout(x + addend[m % res_mod]) (bf16; every term optional): the part of
 * the GEMM epilogue that has to wait for the all-reduce of tensor-parallel partial products (row-parallel proj / fc2,
 * reference attention.py:81-85, mlp.py:66-71).  Same mask hash as the epilogue; y may alias x. */
int orbit2_post_reduce(const void* x, const void* addend, int res_mod, const void* residual, void* y, int M, int N,
                       float drop_p, uint64_t seed, const float* rowscale, int rows_per_scale, void* stream);
/* out[N] = beta*out + sum_m x[m][n]  (bias gradients; sum over batch).  ws: fp32 >= colsum_ws_floats */
int orbit2_colsum(const void* x, int x_fp32, int M, int N, int ldx, void* out, int out_fp32, float beta, float* ws,
                  int ws_floats, void* stream);
int orbit2_colsum_ws_floats(int M, int N);
/* out[r][n] = sum_b x[b][r][n]  (pos_embed gradient over the batch, res_slimvit.py:273) */
int orbit2_batch_sum(const void* x, void* out, int B, int rows, int N, int out_fp32, float beta, void* stream);
/* DropPath (timm 0.9.2, vit_blocks.py:61,74): out[b] = 0 with prob p else 1/(1-p), from hash(seed, b) */
int orbit2_droppath_scales(float* out, int B, float p, uint64_t seed, void* stream);
/* dst[C][R] = src[R][C] (bf16): transposed compute copy of a weight so that dX = dY.W runs K-contiguous */
int orbit2_transpose_bf16(const void* src, void* dst, int R, int C, void* stream);
int orbit2_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int orbit2_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* y = a + b (bf16), used for pos_embed + spatial_embed table (res_slimvit.py:273-281) */
int orbit2_add_rowvec(const void* a, const void* vec, void* y, int rows, int N, void* stream);

/* ---- position-embedding table of a step (ABI 6) ------------------------------------------------ */
/* out[nh*nw][D] = bicubic(pe seen as [oh][ow][D]) + sw[:] * res + sb[:]  (fp32; sw, sb both NULL: plain re-grid).
 * Replaces components/pos_embed.py:103-138 interpolate_pos_embed_on_the_fly (F.interpolate mode="bicubic",
 * align_corners=False on the [1, L0, D] table, taken only when oh != nh -- otherwise the table is used as it is) and the
 * Linear(1, D) resolution embedding res_slimvit.py:62,277-281.  D % 4 == 0, sides <= 2048. */
int orbit2_posembed_fwd(const float* pe, const float* sw, const float* sb, float res, float* out, int oh, int ow, int nh,
                        int nw, int D, void* stream);
/* transpose of the re-grid (autograd of the call above w.r.t. pe): dpe[oh*ow][D] from dout[nh*nw][D]; fixed summation
 * order, no atomics.  (d sb = column sums of dout, d sw = res * d sb: orbit2_colsum.) */
int orbit2_posembed_bwd(const float* dout, float* dpe, int oh, int ow, int nh, int nw, int D, void* stream);

/* ---- hi-res tail -------------------------------------------------------------------------- */
/* unpatchify (res_slimvit.py:167-179): t bf16 [B, L, C*(s*p)^2] -> img [B, C, h*s, w*s] (fp32) */
int orbit2_unpatchify_fwd(const void* t, float* img, int B, int C, int h, int w, int p, int s, void* stream);
/* the same with t fp32 (res_slimvit.py:167-179 under data_type float32) */
int orbit2_unpatchify_fwd_f32(const float* t, float* img, int B, int C, int h, int w, int p, int s, void* stream);
int orbit2_unpatchify_bwd(const float* dimg, void* dt, int B, int C, int h, int w, int p, int s, void* stream);
/* 3x3 conv, stride 1, zero pad 1 (res_slimvit.py:108,111,122).  in: fp32 [B,Cin,H,W] gathered through
 * chan_idx (NULL = identity; res_slimvit.py:237 channel gather); weight fp32 [Cout,Cin,3,3]; bias [Cout].
 * mode 0: out[B,Cout,H,W];  mode 1: GELU then PixelShuffle(r) -> out[B,Cout/r^2,H*r,W*r]
 * (pre-activation saved to `pre` [B,Cout,H,W] for backward);  addend: optional fp32 image
 * [B,Cout,Ha,Wa] whose top-left HxW crop is added (res_slimvit.py:333-336). */
int orbit2_conv3x3_fwd(const float* in, const int* chan_idx, int in_ctotal, const float* weight, const float* bias,
                       float* out, float* pre, const float* addend, int Ha, int Wa, int B, int Cin, int Cout,
                       int H, int W, int mode, int r, void* stream);
/* backward: dout is [B,Cout,H,W] (mode 0) or the shuffled [B,Cout/r^2,H*r,W*r] (mode 1, needs pre).
 * din (may be NULL) fp32 [B,Cin,H,W]; dweight/dbias fp32, ACCUMULATED into (caller zeroes).
 * ws: fp32 workspace of orbit2_conv3x3_bwd_ws_floats(...) floats (ABI 4): one slab of Cout*Cin*9 + Cout partial sums per
 * 16x16-pixel tile, added in a fixed order (no float atomics: the gradients are bitwise reproducible). */
int64_t orbit2_conv3x3_bwd_ws_floats(int B, int Cin, int Cout, int H, int W);
int orbit2_conv3x3_bwd(const float* dout, const float* in, const int* chan_idx, int in_ctotal, const float* weight,
                       const float* pre, float* din, float* dweight, float* dbias, int B, int Cin, int Cout, int H,
                       int W, int mode, int r, float* ws, void* stream);
/* in-place clamp of one channel at 0 (examples/intermediate_downscaling.py:267-272) */
int orbit2_clamp_channel(float* img, int B, int C, int HW, int chan, void* stream);
int orbit2_clamp_channel_bwd(const float* img_clamped, float* dimg, int B, int C, int HW, int chan, void* stream);

/* ---- losses (metrics/functional.py:59-202): kind 0 = mse, 1 = bayesian_tv, 2 = image_gradient ------
 * pred fp32 [B,C,H,W]; target fp32 [B,C,Ht,Wt] (top-left crop used); lat_w fp32 [H] or NULL;
 * chan_w fp32 [C] or NULL.  out: fp32 [C+1] (per-channel means, aggregate mean). ws fp32 >= 2*B*C*ORBIT2_LOSS_BLOCKS */
/* workgroups per (b, c) plane of orbit2_loss_fwd and orbit2_masked_loss_fwd; their partial sums are added in this order */
#define ORBIT2_LOSS_BLOCKS 64
int orbit2_loss_fwd(const float* pred, const float* target, int Ht, int Wt, const float* lat_w, const float* chan_w,
                    float* out, float* ws, int B, int C, int H, int W, int kind, void* stream);
/* kinds 0..2: dpred = gscale[0] * d(aggregate)/dpred.
 *
 * kind ORBIT2_LOSS_SSIM_VJP (3): the vector-Jacobian product of orbit2_ssim's sums with respect to pred (csrc/ssim.hip; DESIGN
 * 4.10h; metrics.functional.ssim_loss).  It has no forward here: orbit2_loss_fwd refuses kind 3, the value is orbit2_ssim's.
 *   pred fp32 [B,C,H,W]; target fp32 [B,C,Ht,Wt] (top-left crop); lat_w fp32 [H] or NULL (w = 1); chan_w must be NULL.
 *   gscale fp32 [2][B*C]: gscale[bc] the coefficient g of image bc, gscale[B*C + bc] its data range R.
 *   dpred fp32 [B,C,H,W]: every element written exactly once, no atomics: two calls give the same bits.
 * With S_k the SSIM at valid centre k exactly as orbit2_ssim defines it (7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample
 * covariance, C1 = (K1 R)^2, C2 = (K2 R)^2) and w_k = lat_w[row of k] or 1,
 *   dpred[bc][p] = g_bc * sum over the valid centres k whose window holds p of w_k * dS_k / dpred[p],
 * the gradient of sum_bc g_bc sums[bc][1] of orbit2_ssim (of sums[bc][0] with lat_w NULL); the target and R are constants.
 * Closed form, with N = 49, A1 = 2 ux uy + C1, A2 = 2 vxy + C2, B1 = ux^2 + uy^2 + C1, B2 = vx + vy + C2 per centre:
 *   alpha = 2 A2 / (B1 B2) (uy - ux A1 / B1),   beta = -S / B2,   gamma = 2 A1 / (B1 B2)
 *   d[p] = g { box(w alpha) / 49 + [2 ((x_p - v) box(w beta) - box(w beta (ux - v)))
 *                                   + (y_p - v) box(w gamma) - box(w gamma (uy - v))] / 48 }
 * for any pivot v, box(E)[p] the sum of E over the valid centres within 3 rows and 3 columns of p.  The kernel folds the three
 * box sums that no pixel value multiplies into one (box is linear), so it takes three.
 * CENTRING IS PART OF THE CONTRACT, as in orbit2_ssim: v is a target value inside the workgroup's tile
 * (ORBIT2_SSIM_VJP_TILE_H x ORBIT2_SSIM_VJP_TILE_W pixels of dpred); x_p - v, ux - v, the variances and the covariance come
 * from centred values, never from raw ones, and uy - ux in alpha is the difference of the centred means: a field at 280 K with
 * a range of 5 meets the tolerance of one at offset 0.
 * An image with g_bc == 0.0f is zero-filled and none of its values enter any arithmetic (a constant target with R = 0, or NaN
 * in that image, does not leak).  No address depends on a value.
 * At kind 3, chan_w != NULL, H < 7 or W < 7, or B * C > 65535 return O2_ERR_ARG before any launch, with nothing written, as
 * does everything kinds 0..2 refuse (NULL pred, target, gscale or dpred, a non-positive size, a target smaller than pred). */
#define ORBIT2_LOSS_SSIM_VJP 3
#ifndef ORBIT2_SSIM_VJP_TILE_H
#define ORBIT2_SSIM_VJP_TILE_H 16       /* 16 or 32: chosen by measurement, profiles/ssim_loss.md */
#endif
#define ORBIT2_SSIM_VJP_TILE_W 64
int orbit2_loss_bwd(const float* pred, const float* target, int Ht, int Wt, const float* lat_w, const float* chan_w,
                    const float* gscale, float* dpred, int B, int C, int H, int W, int kind, void* stream);

/* evaluation metrics (metrics/functional.py:219-324 mae / rmse / acc / pearson / mean_bias): out[b][c][12] (double),
 * with a = pred - clim, b = target - clim (clim fp32 [C][H][W] or NULL; target: top-left crop), w = lat_w[y] or 1:
 * {sum a, sum b, sum a^2, sum b^2, sum ab, sum w(a-b)^2, sum w|a-b|, sum wa, sum wb, sum w ab, sum w a^2, sum w b^2} */
int orbit2_eval_moments(const float* pred, const float* target, int Ht, int Wt, const float* lat_w, const float* clim,
                        double* out, int B, int C, int H, int W, void* stream);

/* ---- missing-data masks (csrc/loss.hip; metrics/functional.py masked_mse / masked_bayesian_tv / rmse(mask=) ...) ------
 * A pixel is VALID where the target is finite and the mask (if any) is non-zero:
 *   v[b][c][i][j] = isfinite(target[b][c][i][j]) && (mask == NULL || mask[b * mask_sb + c * mask_sc + i * mask_pitch + j] != 0)
 * mask: bytes, read through its top-left H x W crop; mask_pitch >= W elements between rows; mask_sb / mask_sc the batch and
 * channel strides, 0 = the same plane for every batch entry / channel (a broadcast mask is never expanded).  At an invalid pixel
 * neither pred nor target enters any arithmetic (they may be NaN / Inf there).  pred, target, lat_w, chan_w as orbit2_loss_fwd.
 * When pred and target are 16-byte aligned with W % 4 == Wt % 4 == 0 and the mask, its pitch and its strides are multiples of 4,
 * the kernels read float4 / dword groups; any other layout is read by scalar lanes (same results to rounding of the sums' order).
 *
 * orbit2_masked_loss_fwd: kind 0 = mse, 1 = bayesian_tv (a difference term of the prior counts only if both of its pixels are
 * valid); kinds 3 / 4 are the extreme-value scores and kind 5 the fractions skill score below; any other kind is O2_ERR_ARG.  With num_c = sum_{b,i,j} v w_i cw_c err and n_c = sum_{b,i,j} v:
 *   out[c] = num_c / n_c (0 if n_c == 0), out[C] = sum_c num_c / sum_c n_c (0 if nothing is valid); cnt[c] = n_c, cnt[C] = sum_c n_c.
 * out fp32 [C+1], cnt int64 [C+1] (counted as integers: exact), ws >= 2*B*C*ORBIT2_LOSS_BLOCKS four-byte words.
 * Fixed-order sums, no atomics: two calls give the same bits.
 * orbit2_masked_loss_bwd: dpred = gscale[0] * d(out[C])/dpred with the divisor cnt[C] read on the device; exactly 0.0 at every
 * invalid pixel, and everywhere when cnt[C] == 0.
 * orbit2_masked_moments: out[b][c][13] (double) = the twelve sums of orbit2_eval_moments over the valid pixels, then their number. */
int orbit2_masked_loss_fwd(const float* pred, const float* target, int Ht, int Wt, const uint8_t* mask, int mask_pitch,
                           int64_t mask_sb, int64_t mask_sc, const float* lat_w, const float* chan_w, float* out, int64_t* cnt,
                           float* ws, int B, int C, int H, int W, int kind, void* stream);
int orbit2_masked_loss_bwd(const float* pred, const float* target, int Ht, int Wt, const uint8_t* mask, int mask_pitch,
                           int64_t mask_sb, int64_t mask_sc, const float* lat_w, const float* chan_w, const float* gscale,
                           const int64_t* cnt, float* dpred, int B, int C, int H, int W, int kind, void* stream);
int orbit2_masked_moments(const float* pred, const float* target, int Ht, int Wt, const uint8_t* mask, int mask_pitch,
                          int64_t mask_sb, int64_t mask_sc, const float* lat_w, const float* clim, double* out, int B, int C,
                          int H, int W, void* stream);

/* ---- extreme-value scores (csrc/extremes.hip, csrc/quantile_select.h; metrics/functional.py field_quantiles / tail_rmse /
 * exceedance_scores): two further kinds of orbit2_masked_loss_fwd, additive within ABI 8 -------------------------
 * The entry's `kind` is a bit field: bits 0-3 the kind proper, bit 4 ORBIT2_MASKED_PER_IMAGE, bit 5 ORBIT2_MASKED_LOWER, bits
 * 8-15 a count n (ORBIT2_MASKED_KIND(kind, flags, n)).  Any other set bit, a kind proper other than 0, 1, 3, 4 (and 5, further below), any flag or
 * count on kinds 0 / 1, and ORBIT2_MASKED_LOWER on kind 3 are O2_ERR_ARG.  Validity, pred / target / mask and the float4 / scalar
 * path choice are those of kinds 0 / 1.  Pixels are grouped: G = C groups by default (a channel pooled over the batch and all
 * pixels), G = B * C with ORBIT2_MASKED_PER_IMAGE; invalid pixels enter nothing; a group of 2^31 or more pixels is refused.
 *
 * kind ORBIT2_MASKED_QUANTILES (3), n = Q in 1..ORBIT2_MASKED_MAX_LEVELS: exact order statistics by a radix select.
 *   chan_w is read as levels fp32 [Q], each in [0, 1] (a level outside, or NaN, is clamped into it); lat_w must be NULL.
 *   For field f (0 = target, 1 = pred) and group g with m valid pixels of sorted values x_(0) <= ... <= x_(m-1):
 *   pos = q (m - 1) in double, lo = floor(pos), hi = min(lo + 1, m - 1),
 *     out[f][g][q][3] = { (float)((double)x_(lo) + (pos - lo) ((double)x_(hi) - (double)x_(lo))), x_(lo), x_(hi) }
 *   out fp32 [2][G][Q][3]; the two brackets are data values bit for bit (-0.0 and +0.0 are ordered -0.0 < +0.0 and either may
 *   stand for the other); q = 0 / 1 give the minimum / maximum; cnt int64 [G] = m; m = 0 gives NaN in all three slots.  Values
 *   are ordered by their bit patterns (sign-magnitude to unsigned), so denormals order exactly and a NaN in a valid pred pixel
 *   sorts beyond the infinities of its sign.  pred == target (one pointer) is allowed.
 *   ws >= ORBIT2_QUANTILE_WS_WORDS(G, Q) four-byte words, zeroed by the entry on the stream.  Nothing synchronises with the
 *   host: m, the ranks, the digit prefixes and the interpolation stay on the device.  Integer atomics only: two calls give the
 *   same bits.
 *
 * kind ORBIT2_MASKED_TAIL (4), n = T in 1..ORBIT2_MASKED_MAX_LEVELS: sums and counts beyond thresholds, one pass for all T.
 *   chan_w is read as thresholds fp32 [G][T] (typically column 1 or 2 of kind 3's target rows, still on the device); lat_w is
 *   optional.  A value v is IN THE TAIL of threshold t when v >= t, with ORBIT2_MASKED_LOWER when v <= t.  Per image (b, c) and
 *   threshold, with d = pred - target and w = lat_w[row] or 1, over the valid pixels whose TARGET is in the tail:
 *     out fp32 [B][C][T][4]  = { sum w, sum w d^2, sum w |d|, sum d }
 *     cnt int64 [B][C][T][4] = { tail pixels, of those: pred in the tail too (hits), valid pixels outside the tail whose pred is
 *                                in it (false alarms), valid pixels }
 *   ws >= ORBIT2_TAIL_WS_WORDS(B, C, T).  Per-workgroup fp32 partials, added in a fixed order in double; counts are integers; no
 *   float atomics: two calls give the same bits.
 *
 * Refused before any launch with nothing written: NULL chan_w, n outside 1..8, lat_w at kind 3, a group of 2^31 pixels or more,
 * and everything kinds 0 / 1 refuse. */
#define ORBIT2_MASKED_QUANTILES 3
#define ORBIT2_MASKED_TAIL 4
#define ORBIT2_MASKED_PER_IMAGE 16
#define ORBIT2_MASKED_LOWER 32
#define ORBIT2_MASKED_MAX_LEVELS 8
#define ORBIT2_MASKED_KIND(kind, flags, n) ((kind) | (flags) | ((n) << 8))
/* per (field, group): 64 state words, the 256-bin histogram of the top digit, and for each of the three lower digits one
 * 256-bin histogram per tracked prefix (at most 2 Q: the two brackets of every level) */
#define ORBIT2_QUANTILE_WS_WORDS(G, Q) (2 * (long long)(G) * (64 + 256 + 3 * 2 * (Q) * 256))
/* per image and workgroup: T x 4 fp32 sums, then T x 4 int32 counts */
#define ORBIT2_TAIL_WS_WORDS(B, C, T) ((long long)(B) * (C) * ORBIT2_LOSS_BLOCKS * 8 * (T))

/* ---- the fractions skill score (csrc/fss.hip, csrc/fss_window.h; metrics/functional.py fss / fss_profile): one more
 * kind of orbit2_masked_loss_fwd, additive within ABI 8 -----------------------------------------------------------------------
 * Neighbourhood verification (Roberts & Lean 2008): the fraction of a window in which an event occurs, compared between target
 * and prediction.  A pixel is VALID exactly as for the other kinds (target finite, mask NULL or non-zero); the target is read
 * through the prediction's top-left crop.  For a threshold t the INDICATOR of a field value v at a pixel is valid && v >= t,
 * with ORBIT2_MASKED_LOWER valid && v <= t; a NaN prediction at a valid pixel compares false; invalid pixels and pixels outside
 * the plane hold 0 in both indicators (zero padding).  For the odd window n = 2 r + 1, cO(i, j) and cM(i, j) are the integer
 * numbers of set target and prediction indicators in rows i - r .. i + r and columns j - r .. j + r.  Per image (b, c) and
 * threshold, summed over the VALID centres only:
 *   cnt int64 [B][C][T][4] = { valid centres, sum cO^2, sum cM^2, sum (cO - cM)^2 }
 *   out fp32  [B][C][T]    = (float)(1.0 - (double)cnt[3] / ((double)cnt[1] + (double)cnt[2])), NaN when cnt[1] + cnt[2] == 0
 * The factor n^4 of the fractions cancels, so the score is a ratio of exact integers; a score pooled over images is formed by
 * the caller from the summed integers.  n = 1 is the grid-scale score; a window larger than the plane is clamped to it.
 *
 * The kind word, ORBIT2_FSS_WORD(flags, T, n): bits 0-3 = ORBIT2_FSS_KIND (5); bit 4 ORBIT2_MASKED_PER_IMAGE: the thresholds
 * are [B*C][T] instead of [C][T], as at ORBIT2_MASKED_TAIL; bit 5 ORBIT2_MASKED_LOWER; bits 8-15 T in
 * 1..ORBIT2_MASKED_MAX_LEVELS; bits 16-23 the window n, odd, 1..ORBIT2_FSS_MAX_WINDOW.  No other kind takes bits 16 and up.
 * chan_w is read as thresholds fp32 [G][T] (G = C, or B * C with ORBIT2_MASKED_PER_IMAGE); lat_w must be NULL: the score is
 * unweighted, integer sums are what make it exact.  ws holds ORBIT2_FSS_WS_WORDS(B, C, H, W, T) four-byte words and is 8-byte
 * aligned: the valid plane and the 2 T indicator planes as bits, [B*C][2 T + 1][H][ceil(W / 64)] 64-bit words.  cnt is zeroed by
 * the entry on the stream.  255^2 = 65025 and 65025^2 = 4 228 250 625 < 2^32, so a pixel's term fits an unsigned 32-bit word;
 * (2^63 - 1) / 255^4 = 2 181 368 337 > 2^31, so an int64 sum over fewer than 2^31 pixels cannot overflow, per image or pooled.
 * Integer atomics only: two calls give the same bits.  No address depends on a data value.
 *
 * Refused before any launch with nothing written: any other set bit, an even or zero window, T outside 1..8, NULL chan_w,
 * non-NULL lat_w, a ws that is not 8-byte aligned, a group (a channel over the batch, or with ORBIT2_MASKED_PER_IMAGE an image)
 * of 2^31 pixels or more, and everything kinds 0 / 1 refuse. */
#define ORBIT2_FSS_KIND 5
#define ORBIT2_FSS_MAX_WINDOW 255
#define ORBIT2_FSS_WORD(flags, T, n) (ORBIT2_FSS_KIND | (flags) | ((T) << 8) | ((n) << 16))
#define ORBIT2_FSS_WS_WORDS(B, C, H, W, T) (2 * (long long)(B) * (C) * (2 * (T) + 1) * (H) * (((W) + 63) / 64))

/* ---- MC-dropout ensembles (utils/mc_dropout.py) and the Gaussian scores (metrics/functional.py:340-386) ------
 * orbit2_ensemble_update: the k-th (1-based) Welford step over n fp32 elements, in place:
 *   d = member - mean; mean += d / k; m2 += d * (member - mean).   k = 1 initialises (mean = member, m2 = 0; neither is read).
 * After N steps m2 / (N - 1) is the unbiased variance.  The three buffers must be distinct; 16-byte aligned bases take the
 * float4 path.  NULL, n <= 0, k < 1 or aliased buffers return O2_ERR_ARG before any launch. */
int orbit2_ensemble_update(const float* member, float* mean, float* m2, int64_t n, int k, void* stream);
/* mean, std fp32 [B,C,H,W]; target fp32 [B,C,Ht,Wt] (top-left crop; Ht >= H, Wt >= W); lat_w fp32 [H] or NULL (w = 1).
 * out[b][c][4] (double) = {sum w crps, sum w std^2, sum w (mean - target)^2, sum 1{|target - mean| <= std}} with the closed-form
 * Gaussian CRPS std (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)), z = (target - mean) / std; at std == 0 crps = |target - mean|
 * and the point is covered only if target == mean (no NaN / Inf for finite inputs).  NULL mean / std / target / out, a
 * non-positive size, a target smaller than the prediction or B * C > 65535 return O2_ERR_ARG before any launch. */
int orbit2_gaussian_scores(const float* mean, const float* std_, const float* target, int Ht, int Wt, const float* lat_w,
                           double* out, int B, int C, int H, int W, void* stream);
/* orbit2_ensemble_scores: the all-member (non-Gaussian) scores of an ensemble, from the N members of every pixel held in
 * registers, in one pass that reads each member once.
 * members fp32: member i is the contiguous [B,C,H,W] field at members + i * member_stride (member_stride >= B*C*H*W, in
 * elements); 2 <= N <= ORBIT2_ENSEMBLE_MAX_MEMBERS.  target fp32 [B,C,Ht,Wt] (top-left crop; Ht >= H, Wt >= W); lat_w fp32 [H]
 * or NULL (w = 1).  All inputs are finite; non-finite members give unspecified scores but never a fault.
 * With y the target, d_i = x_i - y and d_(1) <= ... <= d_(N) sorted -- everything summed is centred on the target first (a
 * field in kelvin is 280 +- 1: the pair term on raw values cancels its low bits away) -- each output is optional (NULL = not
 * computed), at least one must be given:
 *   sums       double [B][C][4], zeroed by the entry, accumulated across workgroups as orbit2_gaussian_scores does:
 *                0 sum_pix w (1/N) sum_i |d_i|        1 sum_pix w sum_{i<j} |x_i - x_j|  ( = sum_k (2k - N - 1) d_(k), k 1-based)
 *                2 sum_pix w (mean_i d_i)^2           3 sum_pix w (unbiased variance of the members; two passes over the d_i)
 *              host forms: empirical CRPS = [0] - [1] / N^2, fair CRPS = [0] - [1] / (N (N - 1)), spread / skill from [3], [2].
 *   crps_field fp32 [B,C,H,W], the per-pixel CRPS, unweighted: empirical (fair == 0) or fair (fair != 0).
 *   hist       int64 [B][C][N + 1], zeroed by the entry: counts of the rank of the target among the members,
 *                rank = lt + ((uint64) h * (eq + 1) >> 32),  lt = #{x_i < y}, eq = #{x_i == y},
 *                h = hash(seed, flat index of the pixel in the [B,C,H,W] prediction)   (the RNG of every seeded entry).
 *              Ties are broken by the hash because constant output channels are copied from the target into every member: a
 *              lowest-rank rule would pile those pixels into bin 0 and read as a bias.  UNLIKE EVERY OTHER SEEDED ENTRY THE SEED
 *              SALT (orbit2_seed_salt) IS NOT MIXED IN: a score is a pure function of its arguments, and the salt advances
 *              under graph replay.  Integer counts, added by integer atomics: bit-repeatable.
 *   quant      fp32 [Q][B][C][H][W], the quantiles at levels[Q] (device fp32, 1 <= Q <= 16, each in [0, 1]) as numpy / torch
 *              "linear" define them: pos = q (N - 1), lo = floor(pos), value = x_(lo) + (pos - lo) (x_(lo+1) - x_(lo)) on the
 *              raw members; q = 0 and q = 1 are the minimum and the maximum bit for bit.
 * NULL members or target, all four outputs NULL, N < 2 or > ORBIT2_ENSEMBLE_MAX_MEMBERS, member_stride < B*C*H*W, a
 * non-positive size, a target smaller than the prediction, B * C > 65535, quant without levels or Q outside 1..16 return
 * O2_ERR_ARG before any launch, with nothing written. */
#define ORBIT2_ENSEMBLE_MAX_MEMBERS 64
int orbit2_ensemble_scores(const float* members, int64_t member_stride, int N, const float* target, int Ht, int Wt,
                           const float* lat_w, double* sums, float* crps_field, int fair, int64_t* hist, uint64_t seed,
                           float* quant, const float* levels, int Q, int B, int C, int H, int W, void* stream);

/* orbit2_ssim: structural similarity (and the squared-error sum that PSNR needs) of every (b, c) image of a prediction against
 * a target, as scikit-image's structural_similarity defines it by default: a 7 x 7 uniform window (ORBIT2_SSIM_WIN, the only
 * size built), K1 = 0.01, K2 = 0.03, sample covariance (factor 49 / 48), and the score of an image the mean of S over the
 * centres whose window lies wholly inside it, rows 3 .. H - 4 and columns 3 .. W - 4 ("valid centres").  With the window means
 * ux, uy, the variances vx, vy, the covariance vxy, C1 = (K1 R)^2 and C2 = (K2 R)^2 for the data range R:
 *   S = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2)).
 * pred fp32 [B,C,H,W]; target fp32 [B,C,Ht,Wt] (top-left crop; Ht >= H, Wt >= W); lat_w fp32 [H] or NULL (w = 1).
 * data_range device fp32 [B][C] or NULL: NULL = every image uses max - min of its own target crop, found on the device by a
 * first launch of the entry and handed to the SSIM pass through sums[3..4] (no host synchronisation); given = that value is
 * used, min and max are reported all the same.
 *   sums     double [B][C][6], initialised by the entry, accumulated across workgroups as orbit2_gaussian_scores does (fp32
 *            per-thread partials, wave and workgroup reduction, one double atomic per workgroup and sum):
 *              0 sum of S over the valid centres      1 sum of lat_w[y] S (y the centre's row)
 *              2 sum of (pred - target)^2 over ALL H x W pixels
 *              3 target min    4 target max    5 the data range actually used (R; max - min in double when not given)
 *            host forms: SSIM = [0] / ((H - 6) (W - 6)), weighted = [1] / ((W - 6) sum_{y = 3}^{H - 4} lat_w[y]),
 *            PSNR = 10 log10([5]^2 H W / [2]).
 *   ssim_map fp32 [B][C][H - 6][W - 6] or NULL: S at every valid centre (scikit-image's full=True map without its border).
 * CENTRING IS PART OF THE CONTRACT: both fields are centred on one shared pivot, a target value inside the workgroup's tile
 * (ORBIT2_SSIM_TILE_H x ORBIT2_SSIM_TILE_W centres; in fact one under the 14 x 7 pixels a lane's windows cover), before
 * anything is squared or summed; variances and covariance come from the centred sums, the means get the pivot added back for
 * the luminance term.  Why: on a 39 x 71 field at offset 280 (kelvin) with range 5 the raw fp32 form is off by up to 4.8e-1
 * per pixel, the centred one by 2e-6.
 * R == 0 (a wholly constant target image) is not special-cased: C1 = C2 = 0, a flat window is 0 / 0, and sums[0..1] of that
 * image are NaN, as scikit-image's would be; the other images of the call are not affected.  Non-finite inputs give unspecified
 * scores and never a fault: no address depends on a value.
 * NULL pred, target or sums, a non-positive size, H < 7 or W < 7, a target smaller than the prediction or B * C > 65535 return
 * O2_ERR_ARG before any launch, with nothing written. */
#define ORBIT2_SSIM_WIN 7
#define ORBIT2_SSIM_TILE_H 32
#define ORBIT2_SSIM_TILE_W 64
int orbit2_ssim(const float* pred, const float* target, int Ht, int Wt, const float* lat_w, const float* data_range,
                double* sums, float* ssim_map, int B, int C, int H, int W, void* stream);

/* ---- interpolation baselines (models/hub/interpolation.py) ------------------------------------------------
 * orbit2_resample_fwd: out[b][c] = scale[c] * resample(x[b][chan_idx[c]]) + shift[c], the resampling being
 * F.interpolate(size = (H, W), align_corners = False) without antialiasing, for any h, w, H, W >= 1 (integer and non-integer
 * upsampling, identity, downsampling).  mode: 0 nearest, 1 bilinear, 2 bicubic.
 *   x        fp32 [B][in_ctotal][h][w]
 *   chan_idx device int[C] or NULL (identity; then C == in_ctotal), as in orbit2_conv3x3_fwd.  It lives on the device, so the
 *            entry trusts it: the caller checks 0 <= idx < in_ctotal.
 *   scale, shift  device fp32 [C], both or neither: the pixel is fmaf(scale[c], r, shift[c]), or r.
 *   out      fp32 [B][C][H][W]
 * THE COORDINATES ARE PART OF THE CONTRACT: fp32, every product and difference rounded on its own (no fused multiply-add).
 *   ratio = (float)in / (float)out
 *   nearest   i = min((int)floorf(o * ratio), in - 1)
 *   bilinear  s = max(ratio * (o + 0.5f) - 0.5f, 0), i0 = (int)s, i1 = min(i0 + 1, in - 1), l1 = s - i0, l0 = 1 - l1
 *   bicubic   s = ratio * (o + 0.5f) - 0.5f, b = floorf(s), t = s - b, taps b - 1 .. b + 2 with clamped indices,
 *             cubic-convolution weights with A = -0.75: ((A x - 5A) x + 8A) x - 4A at x = t + 1 and 2 - t,
 *             ((A + 2) x - (A + 3)) x x + 1 at x = t and 1 - t, every product rounded on its own here too
 * A row interpolant is its taps left to right (a product, then fused multiply-adds), a pixel its row interpolants top to bottom.
 * Nearest picks ATen's source pixel; identity is exact in all three modes.
 * A workgroup owns an ORBIT2_RESAMPLE_TILE_H x ORBIT2_RESAMPLE_TILE_W tile of one image and stages the source pixels under it in
 * LDS when (ceil(TILE_H h / H) + 4) (ceil(TILE_W w / W) + 4) <= ORBIT2_RESAMPLE_LDS_FLOATS, which holds for every upsampling
 * ratio and the identity; otherwise it reads the taps from global memory.  Same values either way.
 * orbit2_resample_moments: out[b][c][12] (double) = the twelve sums of orbit2_eval_moments, in its order, of that same field
 * WITHOUT storing it: a = value - clim, b = target - clim (clim fp32 [C][H][W] or NULL; target fp32 [B][C][Ht][Wt] through its
 * top-left crop; w = lat_w[y] or 1).  The entry zeroes out and accumulates as orbit2_eval_moments does (fp32 per-lane
 * partials, here over at most TILE_H / 4 x 4 pixels, a wave and workgroup reduction, one double atomic per workgroup and sum).
 * No address depends on a value: non-finite inputs give unspecified values, never a fault.
 * NULL x, out or target, exactly one of scale and shift, chan_idx NULL with C != in_ctotal, a mode outside 0..2 (and 5, 6: below), a non-positive
 * size, a target smaller than H x W or B * C > 65535 return O2_ERR_ARG before any launch, with nothing written.
 *
 * ANTIALIASED MODES: mode = base | ORBIT2_ANTIALIAS with base 1 (bilinear: 5) or 2 (bicubic: 6) is
 * F.interpolate(size = (H, W), align_corners = False, antialias = True).  Nearest has no antialiased form: 3, 4, 7, anything
 * above and anything negative stay O2_ERR_ARG, and 0, 1, 2 run the kernels above, unchanged.  Everything else in this comment
 * (chan_idx, scale / shift, the target crop, lat_w, clim, the twelve sums, the zeroing of out by the moments entry, every other
 * refusal) holds for 5 and 6 as it stands; orbit2_resample_moments scores exactly the values orbit2_resample_fwd stores.
 * An output coordinate o reads a window of the source axis, clipped to the grid (NOT index-clamped) and renormalised; per axis,
 * fp32, with interp = 2 (bilinear) or 4 (bicubic):
 *   ratio   = (float)in / (float)out
 *   support = ratio >= 1 ? (interp / 2) * ratio : interp / 2;    inv = ratio >= 1 ? 1 / ratio : 1
 *   center  = ratio * (o + 0.5f)
 *   lo      = max((int)((center - support) + 0.5f), 0);    n = min((int)((center + support) + 0.5f), in) - lo
 *   raw_j   = f((((float)(j + lo) - center) + 0.5f) * inv),  j = 0 .. n - 1;    weight_j = raw_j / sum_j raw_j
 *   f bilinear: |x| < 1 ? 1 - |x| : 0
 *   f bicubic (A = -0.5, not the plain mode's -0.75): |x| < 1 ? ((1.5 |x| - 2.5) |x|) |x| + 1
 *                                                    : |x| < 2 ? (((|x| - 5) |x| + 8) |x| - 4) * -0.5 : 0
 * Rounded on their own, never fused: every product above (ratio * (o + 0.5f), the product by inv, each product of the two
 * polynomials) and every sum and difference.  sum_j raw_j adds the taps in ascending order, starting from 0; the normalisation
 * is a DIVISION by that sum (skipped if the sum is 0), correctly rounded.  At most 2 ceil(support) + 1 taps, possibly the whole
 * axis.  A tap on the edge of the support has weight 0 in both filters, so which side of an integer lo or lo + n falls on moves
 * a pixel by rounding only.
 * The pixel is separable, horizontal pass first: a row interpolant is weight_0 * src[lo] (a product), then one fused multiply-add
 * per tap in ascending order, and is ROUNDED TO fp32; the pixel is its rows' interpolants top to bottom in the same way (a
 * product, then fused multiply-adds), then fmaf(scale[c], r, shift[c]).  The identity (in == out) is exact for finite input; an
 * antialiased bilinear upsample is the plain one to rounding (two clipped taps are the clamped index), a bicubic one differs
 * by A and near the borders.
 * A workgroup owns an ORBIT2_AA_TILE_H x ORBIT2_AA_TILE_W tile and keeps the windows' normalised weights in LDS when the tile's
 * longest windows KX (columns) and KY (rows) satisfy TILE_W KX <= ORBIT2_AA_WX_FLOATS and TILE_H KY <= ORBIT2_AA_WY_FLOATS and
 * one row of the tile's source footprint fits ORBIT2_AA_SRC_FLOATS; it then works through the source rows under the tile in
 * chunks of min(ORBIT2_AA_CHUNK_ROWS, SRC_FLOATS / footprint width) rows staged in LDS.  Otherwise (bicubic beyond a ratio of
 * about 11, bilinear beyond 23, a long axis reduced to a few pixels) it forms the weights where it uses them and reads the taps
 * from global memory, in chunks of CHUNK_ROWS rows.  The choice is per workgroup; the operations and their order are the same,
 * so are the bits.  LDS use does not depend on the sizes.  Per-lane fp32 partial sums of the moments cover 4 pixels here.
 * No window index depends on a value: non-finite inputs give unspecified values, never a fault.
 *
 * THE ADJOINT OF THE ANTIALIASED MODES: orbit2_resample_fwd with mode = base | ORBIT2_ANTIALIAS | ORBIT2_TRANSPOSE,
 * base 1 (21) or 2 (22), applies the transpose of the antialiased resample that takes an (H, W) grid to an (h, w) grid.  The
 * operands keep their places: x is the gradient g on the COARSE grid, fp32 [B][C][h][w]; out is the gradient d on the FINE
 * grid, fp32 [B][C][H][W].  With (lo_o, n_o, Wy[o][j]) the window rule above for the forward call that resamples H -> h rows
 * (in = H, out = h) and (lo_p, n_p, Wx[p][q]) the same for W -> w columns,
 *   d[Y][X] = sum over o with lo_o <= Y < lo_o + n_o, sum over p with lo_p <= X < lo_p + n_p, of
 *             Wy[o][Y - lo_o] * Wx[p][X - lo_p] * g[o][p]
 * and the weights are that forward call's fp32 weights bit for bit, so <A p, g> = <p, A^T g> holds to summation error only.
 * ORDER: t[o][X] is the sum over the windows p that hold X, p ascending: the first is a product, every later one a fused
 * multiply-add, and t is ROUNDED TO fp32; d[Y][X] is the sum over the windows o that hold Y, o ascending, of Wy * t[o][X] in the
 * same way.  Every element of out is written, and the result is the same bits from call to call (no atomics).  The identity
 * (h == H, w == W) returns g exactly for finite g that holds no negative zero.
 * Only coarsening is built: at every ratio >= 1 a fine coordinate lies in at least 1 and at most 3 (bilinear) or 5 (bicubic)
 * windows, and lo and lo + n do not decrease with o, so the footprint of a fine pixel is fixed.  A workgroup owns an
 * ORBIT2_AT_TILE_H x ORBIT2_AT_TILE_W tile of the fine grid and keeps at most ORBIT2_AT_COVER windows per fine coordinate.
 * Refused with O2_ERR_ARG before any launch: h > H or w > W; chan_idx != NULL or C != in_ctotal; scale or shift non-NULL;
 * ORBIT2_TRANSPOSE with any base other than 5 or 6 (16, 17, 18, 20, 23, ...), and in orbit2_resample_moments always; a pair of
 * sizes whose windows decrease or cover a fine coordinate more than ORBIT2_AT_COVER times; and everything the plain call
 * refuses (null pointers, non-positive sizes, B * C > 65535). */
#define ORBIT2_ANTIALIAS 4
#define ORBIT2_TRANSPOSE 16
#define ORBIT2_AT_TILE_H 32
#define ORBIT2_AT_TILE_W 64
#define ORBIT2_AT_COVER 5
#define ORBIT2_AA_TILE_H 16
#define ORBIT2_AA_TILE_W 64
#define ORBIT2_AA_CHUNK_ROWS 32
#define ORBIT2_AA_SRC_FLOATS 6144
#define ORBIT2_AA_WX_FLOATS 3072
#define ORBIT2_AA_WY_FLOATS 768
#define ORBIT2_RESAMPLE_TILE_H 32
#define ORBIT2_RESAMPLE_TILE_W 256
#define ORBIT2_RESAMPLE_LDS_FLOATS 10240
int orbit2_resample_fwd(const float* x, const int* chan_idx, int in_ctotal, const float* scale, const float* shift,
                        float* out, int B, int C, int h, int w, int H, int W, int mode, void* stream);
int orbit2_resample_moments(const float* x, const int* chan_idx, int in_ctotal, const float* scale, const float* shift,
                            const float* target, int Ht, int Wt, const float* lat_w, const float* clim, double* out,
                            int B, int C, int h, int w, int H, int W, int mode, void* stream);

/* ---- perceptual loss = L1 + 0.5 * mean_b LPIPS-VGG16 (metrics/functional.py:17-33, metrics.py:119-187) ------
 * Feature maps are NHWC bf16, so each 3x3 VGG convolution is im2col + orbit2_gemm_bf16 (bias, act = 2) forward and
 * orbit2_gemm_bf16 + col2im backward (input gradient only: LPIPS weights are frozen, metrics.py:127-128).
 * Tap order of a 3x3 window: t = ky*3 + kx, offsets (ky-1, kx-1), zero padding.  C % 8 == 0. */
/* col[p][t][c] = x[p + off_t][c];  x: [N][H][W][C], col: [N*H*W][9*C] */
int orbit2_im2col3x3(const void* x, void* col, int N, int H, int W, int C, void* stream);
/* g[p][c] = sum_t dcol[p - off_t][t][c]; with act != NULL: out = (g + tapg) * (act > 0)  (ReLU backward of the layer
 * that produced act, plus the LPIPS tap gradient at that layer; tapg may be NULL) */
int orbit2_col2im3x3(const void* dcol, const void* act, const void* tapg, void* out, int N, int H, int W, int C,
                     void* stream);
/* 2x2 / stride 2 max-pool (torchvision VGG16 features 4, 9, 16, 23); backward routes to the first maximum of the
 * window (ATen's index rule) and fuses the ReLU mask of x and the tap gradient like col2im */
int orbit2_maxpool2_fwd(const void* x, void* y, int N, int H, int W, int C, void* stream);
int orbit2_maxpool2_bwd(const void* g, const void* x, const void* tapg, void* dz, int N, int H, int W, int C,
                        void* stream);
/* first convolution 3 -> 64 (+ReLU) straight from the NCHW fp32 image with the LPIPS ScalingLayer fused;
 * w1: fp32 [(t*3 + ci)][64], b1: fp32 [64]; out: [N][H][W][64] bf16 */
int orbit2_lpips_conv1_fwd(const float* img, const float* w1, const float* b1, void* out, int N, int H, int W,
                           void* stream);
/* dimg (NCHW fp32) = conv1 input gradient / scale + l1_coef * gscale[0] * sign(pred - target)   (the L1 term of the loss).
 * gscale (here and in orbit2_lpips_tap_bwd): device pointer to the scalar upstream gradient of the loss (loss scale included)
 * or NULL for 1 -- the backward never reads it on the host, so the loss can be captured in a hipGraph. */
int orbit2_lpips_conv1_bwd(const void* dz, const float* w1, const float* pred, const float* target, float l1_coef,
                           const float* gscale, float* dimg, int N, int H, int W, void* stream);
/* LPIPS head of one tap.  feats: [2B][HW][C] bf16, images 0..B-1 = prediction, B..2B-1 = target; lin: fp32 [C].
 * fwd: val[b] += mean_px sum_c lin_c (f0_c/(|f0|+1e-10) - f1_c/(|f1|+1e-10))^2.   C in {64,128,256,512}.
 * bwd: gout[b][px][c] = coef * gscale[0] * d(sum_c ...)/d f0_c * (f0_c > 0)  -- the gradient w.r.t. the tap's PRE-ReLU output
 * (bf16; a pixel whose prediction features are all zero gets 0 where autograd of sqrt at 0 would produce NaN)
 * ws (fwd, ABI 4): fp32 workspace of orbit2_lpips_tap_ws_floats(B, HW, C) floats -- per-block partial sums added in a fixed order */
int64_t orbit2_lpips_tap_ws_floats(int B, int HW, int C);
int orbit2_lpips_tap_fwd(const void* feats, const float* lin, float* val, int B, int HW, int C, float* ws, void* stream);
int orbit2_lpips_tap_bwd(const void* feats, const float* lin, void* gout, float coef, const float* gscale, int B, int HW, int C,
                         void* stream);
/* out[0] += mean |a - b|   (F.l1_loss, metrics/functional.py:30); ws: orbit2_l1_mean_ws_floats(n) floats (fixed-order sum, ABI 4) */
int64_t orbit2_l1_mean_ws_floats(int64_t n);
int orbit2_l1_mean(const float* a, const float* b, float* out, int64_t n, float* ws, void* stream);

/* ---- optimizer (utils/loaders.py:398-399 AdamW; ShardedGradScaler :732-742) ------------------ */
/* flat fused AdamW over n elements: fp32 master p/m/v, gradient g (bf16 or fp32) multiplied by
 * grad_scale; writes the bf16 compute copy p16 (may be NULL).  Skips everything when *found_inf != 0. */
int orbit2_adamw(float* p, float* m, float* v, const void* g, int g_fp32, void* p16, int64_t n, float lr,
                 float beta1, float beta2, float eps, float wd, float bc1, float bc2, float grad_scale,
                 const float* found_inf, void* stream);
/* found_inf[0] = 1 if any element is inf/nan (never cleared here) */
int orbit2_check_finite(const void* g, int g_fp32, int64_t n, float* found_inf, void* stream);

/* Device-side seed salt -- the library's only device-global mutable state: every seeded kernel (GEMM-epilogue dropout,
 * attention dropout, dropout backward, DropPath scales) xors it into the seed argument.  add = 0 sets it, add = 1 advances it
 * by `value`; stream-ordered (a one-thread kernel per library module).  0 by default, i.e. the seeds are used as passed.
 * Purpose: a training step captured in a hipGraph begins with orbit2_seed_salt(odd constant, 1, stream), so each replay draws
 * new masks (seeds are kernel arguments, frozen at capture).
 * Consequences of it being per device and not per engine: (1) the salt must not change between a step's forward and the
 * backward that regenerates its masks -- within one stream the stream order guarantees it; two engines stepping CONCURRENTLY on
 * different streams of one device must not both use salted (graph-captured) steps; (2) engines that take turns on one device
 * share the counter: each one's mask sequence then depends on how many replays the others ran (still fresh masks every step,
 * still forward/backward-consistent, but not reproducible per engine); (3) eager steps that follow replays see the salt the
 * last replay left (set it back with add = 0 when bit-reproducing an eager run).  One process per GPU with one training
 * engine -- the reference's layout (examples/intermediate_downscaling.py:161-262) -- meets none of these cases. */
int orbit2_seed_salt(uint64_t value, int add, void* stream);

/* hardware self-test of the MFMA / LDS-transpose / LDS-DMA layouts the kernels assume; returns a
 * bitmask of failed checks in result[0] (0 = all good). */
int orbit2_selftest(int* result, void* stream);
/* diagnostic: sweep `bytes` of buf with 16-byte loads from `blocks` workgroups, `inflight` (1, 4 or 8) loads per lane at a time --
 * the calibration streams of the memory-side latency probe (tools/mall_probe.py, bench.py --mall-probe); sink: one float */
int orbit2_probe_read(const void* buf, int64_t bytes, int blocks, int inflight, float* sink, void* stream);

#ifdef __cplusplus
}
#endif
#endif
