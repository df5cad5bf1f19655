// Interpolation baselines: F.interpolate(size=(H, W), mode=nearest | bilinear | bicubic, align_corners=False) of gathered channels
// of an fp32 [B, in_ctotal, h, w] field, with an optional per-channel affine, either stored (orbit2_resample_fwd) or scored
// against a target without ever being stored (orbit2_resample_moments: the twelve sums of orbit2_eval_moments).
// include/orbit2_hip.h: orbit2_resample_*; models/hub/interpolation.py; DESIGN 4.10c, 4.10g.
// Three kernels: the plain modes' (no antialiasing); further down, the antialiased forms of bilinear and bicubic
// (mode | ORBIT2_ANTIALIAS); and the adjoint of those when they coarsen (mode | ORBIT2_ANTIALIAS | ORBIT2_TRANSPOSE: the backward
// of the consistency training loss).  They differ in how a pixel is formed and in their tiles.  What they share is stated once:
//   RsArgs     the operands of a call, one struct by value; what only one kernel needs stays an argument of that kernel
//   rs_frame   a workgroup's place in the call: its (b, c) image, tile origin, gathered source plane, the channel's affine pair
//   rs_load4   four consecutive floats of a row: one float4 where all four exist and sit on a 16-byte boundary
//   rs_emit    the epilogue of a thread's FOUR CONSECUTIVE output columns of one row: the affine, then the store, or the target
//              and climatology quads and the twelve moments, columns ascending
//   rs_launch  the argument checks, tile sizes, grid and mode dispatch of both entries
// and the adjoint forms its windows and weights with the antialiased kernel's aa_window / aa_weight: the same bits.
//
// The plain kernel: a workgroup owns one RS_TH x RS_TW tile of one (b, c) output image.  A lane owns four consecutive output
// columns, so a wave covers the tile's 256 columns and stores (or reads the target as) one float4 per lane and row; wave v takes
// rows v, v + 4, ... of the tile.  The column taps (source indices and weights of the lane's four columns) are computed once and
// stay in registers for all rows; the row taps are computed once per row from a wave-uniform row number.  The source pixels under
// the tile are staged in LDS once when the call's full-tile footprint fits ORBIT2_RESAMPLE_LDS_FLOATS (every upsampling ratio and
// the identity), else the taps are read straight from global memory (a downsampling footprint can be arbitrarily large).
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
#include <algorithm>
#include "score_sums.h"
#include "../../include/orbit2_hip.h"

namespace {
constexpr int RS_TH = ORBIT2_RESAMPLE_TILE_H, RS_TW = ORBIT2_RESAMPLE_TILE_W, RS_LDS = ORBIT2_RESAMPLE_LDS_FLOATS;
constexpr int RS_NM = O2_NMOMENTS;
static_assert(RS_TW == 256 && RS_TH % 4 == 0, "a wave's 64 lanes x 4 columns span the tile, four waves share its rows");

// ---- what the two kernels share -----------------------------------------------------------------------------------------------
// The operands of a call, as the two entries take them: out for orbit2_resample_fwd; target [B, C, Ht, Wt], lat_w, clim and sums
// for orbit2_resample_moments.  ntx (tiles across), ry and rx (the contract's ratios) are filled in by rs_launch.  The members
// carry no __restrict__; the source plane reaches the pixel loops through a __restrict__ parameter (rs_rows, aa_chunks).
struct RsArgs {
  const float* x; const int* chan_idx; const float* scale; const float* shift;
  float* out; const float* target; const float* lat_w; const float* clim; double* sums;
  int in_ctotal, Ht, Wt, C, h, w, H, W, ntx;
  float ry, rx;
};

struct rs_frame {
  int bc, c, y0, x0;                              // the image (b * C + c), its channel, the tile's first row and column
  const float* src;                               // the gathered source plane
  bool affine;
  float sc, sh;
};
template <int TH, int TW>
__device__ __forceinline__ rs_frame rs_frame_of(const RsArgs& p) {
  rs_frame f;
  f.bc = blockIdx.y;
  const int b = f.bc / p.C, ty = blockIdx.x / p.ntx, tx = blockIdx.x - ty * p.ntx;
  f.c = f.bc - b * p.C;
  f.y0 = ty * TH, f.x0 = tx * TW;
  const int ci = p.chan_idx ? p.chan_idx[f.c] : f.c;
  f.src = p.x + ((size_t)b * p.in_ctotal + ci) * p.h * p.w;
  f.affine = p.scale != nullptr;
  f.sc = f.affine ? p.scale[f.c] : 1.f, f.sh = f.affine ? p.shift[f.c] : 0.f;
  return f;
}

// v = q[0 .. 3], q at column xl of a row of W: a column past the image reads 0 (an odd W misaligns every second row)
__device__ __forceinline__ void rs_load4(const float* __restrict__ q, int xl, int W, float (&v)[4]) {
  if (xl + 3 < W && ((uintptr_t)q & 15) == 0) {
    const float4 t = *reinterpret_cast<const float4*>(q);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = xl + j < W ? q[j] : 0.f;
  }
}

// columns xl .. xl + 3 of output row y (y < H, xl < W) of the frame's image
template <bool MOMENTS>
__device__ __forceinline__ void rs_emit(const RsArgs& p, const rs_frame& f, int y, int xl, float (&v)[4], float (&s)[RS_NM]) {
  if (f.affine) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaf(f.sc, v[j], f.sh);
  }
  if (!MOMENTS) {
    float* o = p.out + ((size_t)f.bc * p.H + y) * p.W + xl;
    // one float4 where the four columns exist and sit on a 16-byte boundary, as rs_load4 reads one
    if (xl + 3 < p.W && ((uintptr_t)o & 15) == 0) {
      *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xl + j < p.W) o[j] = v[j];
    }
  } else {
    float tv[4], cv[4] = {0.f, 0.f, 0.f, 0.f};
    rs_load4(p.target + ((size_t)f.bc * p.Ht + y) * p.Wt + xl, xl, p.W, tv);
    if (p.clim) rs_load4(p.clim + ((size_t)f.c * p.H + y) * p.W + xl, xl, p.W, cv);
    const float lw = p.lat_w ? p.lat_w[y] : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (xl + j < p.W) o2_moments_add(s, v[j] - cv[j], tv[j] - cv[j], lw);
  }
}

// ---- the plain modes ----------------------------------------------------------------------------------------------------------
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
__device__ __forceinline__ void rs_rows(const float* __restrict__ src, int pitch, int yoff, int xoff, const RsArgs& p,
                                        const rs_frame& f, float (&s)[RS_NM]) {
  constexpr int NT = rs_ntaps<MODE>::value;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xl = f.x0 + 4 * lane;                  // the lane's first output column
  int cx[4][NT];
  float wx[4][NT];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // a column past the image takes the last column's taps: in range, never stored or summed
    rs_taps<MODE>(xl + j < p.W ? xl + j : p.W - 1, p.w, p.rx, cx[j], wx[j]);
#pragma unroll
    for (int k = 0; k < NT; ++k) cx[j][k] -= xoff;
  }
  for (int r = wave; r < RS_TH; r += 4) {
    const int y = f.y0 + r;
    if (y >= p.H) break;
    int cy[NT];
    float wy[NT];
    rs_taps<MODE>(y, p.h, p.ry, cy, wy);
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
    rs_emit<MOMENTS>(p, f, y, xl, v, s);
  }
}

template <int MODE, bool MOMENTS>
__global__ __launch_bounds__(256) void resample_kernel(const RsArgs p, int stage) {
  constexpr int NT = rs_ntaps<MODE>::value;
  __shared__ float win[RS_LDS];
  const rs_frame f = rs_frame_of<RS_TH, RS_TW>(p);
  float s[RS_NM];
#pragma unroll
  for (int k = 0; k < RS_NM; ++k) s[k] = 0.f;

  // the source window under the tile: the coordinate is monotone in o, so the first tap of the tile's first row / column and
  // the last tap of its last ones bound every tap in between
  int lo[NT], hi[NT];
  float wgt[NT];
  rs_taps<MODE>(f.y0, p.h, p.ry, lo, wgt);
  rs_taps<MODE>(min(f.y0 + RS_TH, p.H) - 1, p.h, p.ry, hi, wgt);
  const int ylo = lo[0], wh = hi[NT - 1] - ylo + 1;
  rs_taps<MODE>(f.x0, p.w, p.rx, lo, wgt);
  rs_taps<MODE>(min(f.x0 + RS_TW, p.W) - 1, p.w, p.rx, hi, wgt);
  const int xlo = lo[0], ww = hi[NT - 1] - xlo + 1;
  // `stage` is the host's rule (the full-tile footprint of this ratio fits); the window itself is checked all the same
  if (stage && wh > 0 && ww > 0 && (int64_t)wh * ww <= RS_LDS) {
    // a wave per window row, lanes along it: coalesced, and no division by the window's width
    for (int r = threadIdx.x >> 6; r < wh; r += 4)
      for (int q = threadIdx.x & 63; q < ww; q += 64) win[r * ww + q] = f.src[(size_t)(ylo + r) * p.w + xlo + q];
    __syncthreads();
    rs_rows<MODE, MOMENTS, true>(win, ww, ylo, xlo, p, f, s);
  } else {
    rs_rows<MODE, MOMENTS, false>(f.src, p.w, 0, 0, p, f, s);
  }
  if (MOMENTS) o2_block_sums_add(s, p.sums + (size_t)f.bc * RS_NM);
}

// ---- antialiased bilinear / bicubic (mode | ORBIT2_ANTIALIAS): F.interpolate(..., antialias=True) -----------------------------
// An output coordinate o reads a WINDOW of the source axis whose length grows with the downsampling ratio (include/orbit2_hip.h
// states the rule): lo .. lo + n - 1, clipped to the grid, with weights f(.) / sum f(.) (aa_weight).  The pixel is separable,
// horizontal pass first.  A workgroup owns an AA_TH x AA_TW output tile of one (b, c) image; thread t owns row t / 16 and the four
// consecutive columns 4 (t % 16) .. + 3 of it, which it hands to rs_emit once.
//   1. threads 0 .. AA_TW - 1 form the window and the weight sum of one tile column each, the next AA_TH threads those of a
//      tile row; when the tile's longest windows fit (AA_TW KX <= AA_WX, AA_TH KY <= AA_WY, KX / KY the longest window of a
//      column / row) the normalised weights go into LDS tables of pitch KX / KY, once per workgroup.
//   2. the source rows under the tile, ylo .. yhi - 1, are worked through in chunks of at most AA_CR rows, and of as many as
//      AA_SRC floats hold at the tile's footprint width: staged coalesced (a wave per row), then the horizontal pass writes
//      mid[chunk row][tile column], then every thread adds the rows of the chunk that its own vertical window covers to its four
//      accumulators.  Chunks ascend, so a pixel's rows are still added top to bottom.  LDS is bounded whatever the ratio.
//   3. a tile whose windows or footprint width do not fit (a ratio beyond about 11 for bicubic, 23 for bilinear, or a whole long
//      axis reduced to a few pixels) runs the same loops with the weights formed where they are used and the taps read from
//      global memory: the same operations in the same order, hence the same bits.
// Every window index is formed from the sizes alone and clipped into the grid: no address depends on a data value.
constexpr int AA_TH = ORBIT2_AA_TILE_H, AA_TW = ORBIT2_AA_TILE_W, AA_CR = ORBIT2_AA_CHUNK_ROWS, AA_SRC = ORBIT2_AA_SRC_FLOATS;
constexpr int AA_WX = ORBIT2_AA_WX_FLOATS, AA_WY = ORBIT2_AA_WY_FLOATS;
constexpr int AA_MP = AA_TW + 4;                  // pitch of mid: float4 reads stay aligned, a column's rows spread over banks
static_assert(AA_TW == 64 && AA_TH == 16, "256 threads: sixteen rows of sixteen float4 columns");
static_assert(AA_TW + AA_TH <= 256 && AA_CR >= 1 && AA_SRC >= 1, "one thread per tile column and row forms its window");

// the filter at x: bilinear 1 - |x|; bicubic the cubic convolution with A = -0.5, in Horner form, every product on its own
template <int MODE>
__device__ __forceinline__ float aa_filter(float x) {
  x = fabsf(x);
  if (MODE == 1) return x < 1.f ? 1.f - x : 0.f;
  if (x < 1.f) return rs_rounded(rs_rounded((rs_rounded(1.5f * x) - 2.5f) * x) * x) + 1.f;
  if (x < 2.f) return rs_rounded((rs_rounded((rs_rounded((x - 5.f) * x) + 8.f) * x) - 4.f) * -0.5f);
  return 0.f;
}

// the weight of tap j of a window that starts at lo, before (aa_raw) and after (aa_weight) normalisation by the window's sum
template <int MODE>
__device__ __forceinline__ float aa_raw(int j, int lo, float center, float inv) {
  return aa_filter<MODE>(rs_rounded((((float)(j + lo) - center) + 0.5f) * inv));
}
template <int MODE>
__device__ __forceinline__ float aa_weight(int j, int lo, float center, float inv, float total) {
  const float raw = aa_raw<MODE>(j, lo, center, inv);
  return total != 0.f ? raw / total : raw;
}

// window (lo, n), centre and weight sum of output coordinate o
template <int MODE>
__device__ __forceinline__ void aa_window(int o, int n_in, float ratio, float sup, float inv, int& lo, int& n, float& center,
                                          float& total) {
  center = rs_rounded(ratio * ((float)o + 0.5f));
  const int a = (int)((center - sup) + 0.5f), b = (int)((center + sup) + 0.5f);
  lo = min(max(a, 0), n_in - 1);                  // finite sizes give 0 <= lo < hi <= n_in already; the clips are the guarantee
  n = max(min(b, n_in), lo + 1) - lo;
  total = 0.f;
  for (int j = 0; j < n; ++j) total += aa_raw<MODE>(j, lo, center, inv);
}

struct aa_axes {                                  // the tile's windows, in LDS
  int xlo[AA_TW], xn[AA_TW], ylo[AA_TH], yn[AA_TH];
  float xc[AA_TW], xt[AA_TW], yc[AA_TH], yt[AA_TH];
  int kmax[2];
};

// the chunk loop.  FIT: weights from the tables, taps from the staged chunk; else weights formed in place, taps from global memory
template <int MODE, bool FIT>
__device__ __forceinline__ void aa_chunks(const float* __restrict__ src, int w, const aa_axes& ax, float* win, float* mid,
                                          const float* tabx, const float* taby, int KX, int KY, float invy, float invx,
                                          int ncol, bool live, float (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int xlo = ax.xlo[0], fw = ax.xlo[AA_TW - 1] + ax.xn[AA_TW - 1] - xlo, fwp = fw | 1;     // odd pitch: rows spread over banks
  const int ylo = ax.ylo[0], yhi = ax.ylo[AA_TH - 1] + ax.yn[AA_TH - 1];
  const int cr_max = FIT ? min(AA_CR, AA_SRC / fwp) : AA_CR;
  const int i = tid >> 4, c4 = 4 * (tid & 15);
  const int mylo = ax.ylo[i], myhi = live ? mylo + ax.yn[i] : mylo;       // a thread past the image adds nothing
  const float myc = ax.yc[i], myt = ax.yt[i];
  for (int r0 = ylo; r0 < yhi; r0 += cr_max) {
    const int cr = min(cr_max, yhi - r0);
    if (FIT) {
      for (int r = tid >> 6; r < cr; r += 4)
        for (int q = lane; q < fw; q += 64) win[r * fwp + q] = src[(size_t)(r0 + r) * w + xlo + q];
    }
    __syncthreads();                              // the chunk is staged, and the previous chunk's mid has been read
    // horizontal pass: a thread takes one tile column inside the image (mid beyond them is never used) and the four chunk rows
    // g, g + ng, g + 2 ng, g + 3 ng, so a weight is read (or formed) once for four taps; g runs fastest, so a wave reads
    // consecutive rows of a few columns, which the odd pitch spreads over the banks
    const int ng = (cr + 3) >> 2;
    for (int idx = tid; idx < ng * ncol; idx += 256) {
      const int c = idx / ng, g = idx - c * ng;
      const int lo = ax.xlo[c], n = ax.xn[c];
      const float* row[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = g + k * ng < cr ? g + k * ng : g;        // a row past the chunk repeats row g and is not stored
        row[k] = FIT ? win + r * fwp + (lo - xlo) : src + (size_t)(r0 + r) * w + lo;
      }
      const float* wt = tabx + c * KX;
      const float ctr = ax.xc[c], tot = ax.xt[c];
      float t[4];
      const float w0 = FIT ? wt[0] : aa_weight<MODE>(0, lo, ctr, invx, tot);
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = w0 * row[k][0];
      for (int q = 1; q < n; ++q) {
        const float wq = FIT ? wt[q] : aa_weight<MODE>(q, lo, ctr, invx, tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = fmaf(wq, row[k][q], t[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (g + k * ng < cr) mid[(g + k * ng) * AA_MP + c] = t[k];
    }
    __syncthreads();
    const int ka = max(r0, mylo), kb = min(r0 + cr, myhi);
    for (int r = ka; r < kb; ++r) {
      const float wy = FIT ? taby[i * KY + (r - mylo)] : aa_weight<MODE>(r - mylo, mylo, myc, invy, myt);
      const float4 m = *reinterpret_cast<const float4*>(mid + (r - r0) * AA_MP + c4);
      const float mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = r == mylo ? wy * mv[j] : fmaf(wy, mv[j], acc[j]);
    }
  }
}

template <int MODE, bool MOMENTS>
__global__ __launch_bounds__(256) void resample_aa_kernel(const RsArgs p, float supy, float supx, float invy, float invx) {
  __shared__ float win[AA_SRC];
  __shared__ __attribute__((aligned(16))) float mid[AA_CR * AA_MP];
  __shared__ float tabx[AA_WX], taby[AA_WY];
  __shared__ aa_axes ax;
  const int tid = threadIdx.x;
  const rs_frame f = rs_frame_of<AA_TH, AA_TW>(p);
  if (tid < 2) ax.kmax[tid] = 0;
  __syncthreads();
  // a column or row past the image takes the last one's window: in range, never stored or summed
  if (tid < AA_TW) {
    aa_window<MODE>(min(f.x0 + tid, p.W - 1), p.w, p.rx, supx, invx, ax.xlo[tid], ax.xn[tid], ax.xc[tid], ax.xt[tid]);
    atomicMax(&ax.kmax[0], ax.xn[tid]);
  } else if (tid < AA_TW + AA_TH) {
    const int i = tid - AA_TW;
    aa_window<MODE>(min(f.y0 + i, p.H - 1), p.h, p.ry, supy, invy, ax.ylo[i], ax.yn[i], ax.yc[i], ax.yt[i]);
    atomicMax(&ax.kmax[1], ax.yn[i]);
  }
  __syncthreads();
  const int KX = ax.kmax[0], KY = ax.kmax[1];
  const int fwp = (ax.xlo[AA_TW - 1] + ax.xn[AA_TW - 1] - ax.xlo[0]) | 1;
  const bool fit = (int64_t)KX * AA_TW <= AA_WX && (int64_t)KY * AA_TH <= AA_WY && fwp <= AA_SRC;     // the same in every thread
  const int y = f.y0 + (tid >> 4), xl = f.x0 + 4 * (tid & 15);
  const int ncol = min(AA_TW, p.W - f.x0);
  const bool live = y < p.H && xl < p.W;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (fit) {
    if (tid < AA_TW) {
      for (int j = 0; j < ax.xn[tid]; ++j) tabx[tid * KX + j] = aa_weight<MODE>(j, ax.xlo[tid], ax.xc[tid], invx, ax.xt[tid]);
    } else if (tid < AA_TW + AA_TH) {
      const int i = tid - AA_TW;
      for (int j = 0; j < ax.yn[i]; ++j) taby[i * KY + j] = aa_weight<MODE>(j, ax.ylo[i], ax.yc[i], invy, ax.yt[i]);
    }
    // its first barrier publishes the tables
    aa_chunks<MODE, true>(f.src, p.w, ax, win, mid, tabx, taby, KX, KY, invy, invx, ncol, live, acc);
  } else {
    aa_chunks<MODE, false>(f.src, p.w, ax, win, mid, tabx, taby, KX, KY, invy, invx, ncol, live, acc);
  }

  float s[RS_NM];
#pragma unroll
  for (int k = 0; k < RS_NM; ++k) s[k] = 0.f;
  if (live) rs_emit<MOMENTS>(p, f, y, xl, acc, s);
  if (MOMENTS) o2_block_sums_add(s, p.sums + (size_t)f.bc * RS_NM);
}

// ---- the adjoint of the antialiased modes (mode | ORBIT2_ANTIALIAS | ORBIT2_TRANSPOSE), coarsening only ------------------------
// x is the gradient g on the coarse (h, w) grid, out the gradient d on the fine (H, W) grid of the forward call that resamples
// (H, W) -> (h, w):  d[Y][X] = sum_o sum_p Wy[o][Y - lo_o] Wx[p][X - lo_p] g[o][p]  over the windows that hold Y and X, the
// windows and weights being aa_window / aa_weight of that forward call (n_in = H or W, n_out = h or w), bit for bit.
// A fine pixel lies in at most 3 (bilinear) or 5 (bicubic) windows per axis at every ratio >= 1, and in at least one; lo and
// lo + n do not decrease with o.  So the adjoint is a gather with a fixed footprint: no atomics, one path, LDS use that does not
// depend on the sizes.  A workgroup owns an AT_TH x AT_TW tile of the FINE grid of one (b, c) image:
//   1. one thread per candidate forms the window of coarse column at_base + i (i < AT_NX) or coarse row (i < AT_NY): at_base is
//      at least one below the first window that can reach the tile, and tile / ratio + 2 (interp / 2) + 3 candidates reach past
//      the last one.  The candidates that meet the tile are one range per axis (first .. last, by atomicMin / atomicMax in LDS).
//   2. one thread per fine column and row of the tile scans that range for the first window that holds it, counts the windows
//      that follow and hold it too (at most AT_COVER), and forms their weights: the tables first / cnt / wgt.
//   3. the coarse patch of g under those ranges is staged in LDS, a wave per row.
//   4. horizontal pass: mid[o][X] = sum over the windows p of X, ascending, of wgt * g[o][p] (a product, then fused
//      multiply-adds), rounded to fp32; a thread keeps its column's table in registers and takes every fourth coarse row.
//   5. vertical pass: thread t owns the four columns 4 (t % 16) .. + 3 of tile rows t / 16 and t / 16 + 16; a pixel is the sum
//      over the windows o of Y, ascending, of wgt * mid[o][X] in the same way, handed to rs_emit (one 16-byte store).
// Every index is formed from the sizes alone and every range is clipped to its table: no address depends on a data value.
constexpr int AT_TH = ORBIT2_AT_TILE_H, AT_TW = ORBIT2_AT_TILE_W, AT_COVER = ORBIT2_AT_COVER;
constexpr int AT_NY = AT_TH + 10, AT_NX = AT_TW + 10;        // candidate windows per axis: tile / ratio + 2 * 2 + 3 at ratio 1, and slack
constexpr int AT_PP = AT_NX | 1;                             // pitch of the staged patch: odd, its rows spread over the banks
constexpr int AT_MP = AT_TW + 4;                             // pitch of mid: float4 reads stay aligned, rows shift by one 16-byte slot
static_assert(AT_TW == 64 && AT_TH == 32, "256 threads: sixteen float4 columns, two rows each of sixteen");
static_assert(AT_NX <= 128 && AT_NY <= 128 && AT_COVER == 5, "threads 0 .. 127 serve the columns, 128 .. 255 the rows");

template <int NC, int NT>
struct at_axis {                                  // one axis of a tile, in LDS
  int lo[NC], n[NC];                              // the candidates' windows
  float ctr[NC], tot[NC];
  int range[2];                                   // first and last candidate that meets the tile
  int first[NT], cnt[NT];                         // per fine coordinate: its first window (counted from range[0]) and how many
  float wgt[AT_COVER][NT];
};

// the first candidate: (c0 + 0.5) / ratio - 0.5 - interp / 2 bounds the first window that reaches fine coordinate c0 from below
template <int MODE>
__device__ __forceinline__ int at_base(int c0, float ratio) {
  return max((int)floorf((float)c0 / ratio - 0.5f - (MODE == 1 ? 1.f : 2.f)) - 1, 0);
}

// step 1, thread i of an axis: the tile holds the fine coordinates c0 .. c1 - 1
template <int MODE, int NC, int NT>
__device__ __forceinline__ void at_candidate(at_axis<NC, NT>& ax, int i, int base, int c0, int c1, int n_fine, int n_coarse,
                                             float ratio, float sup, float inv) {
  if (i >= NC || base + i >= n_coarse) return;
  aa_window<MODE>(base + i, n_fine, ratio, sup, inv, ax.lo[i], ax.n[i], ax.ctr[i], ax.tot[i]);
  if (ax.lo[i] < c1 && ax.lo[i] + ax.n[i] > c0) {
    atomicMin(&ax.range[0], i);
    atomicMax(&ax.range[1], i);
  }
}

// step 2, thread j of an axis: fine coordinate c0 + j
template <int MODE, int NC, int NT>
__device__ __forceinline__ void at_table(at_axis<NC, NT>& ax, int j, int c0, int c1, float inv) {
  if (j >= NT) return;
  const int c = c0 + j, r0 = ax.range[0], r1 = ax.range[1];
  int i = r0, cnt = 0;
  if (c < c1) {
    while (i <= r1 && !(ax.lo[i] <= c && c < ax.lo[i] + ax.n[i])) ++i;
    while (cnt < AT_COVER && i + cnt <= r1 && ax.lo[i + cnt] <= c && c < ax.lo[i + cnt] + ax.n[i + cnt]) {
      const int k = i + cnt;
      ax.wgt[cnt][j] = aa_weight<MODE>(c - ax.lo[k], ax.lo[k], ax.ctr[k], inv, ax.tot[k]);
      ++cnt;
    }
  }
  ax.first[j] = cnt ? i - r0 : 0;
  ax.cnt[j] = cnt;
  for (int k = cnt; k < AT_COVER; ++k) ax.wgt[k][j] = 0.f;
}

template <int MODE>
__global__ __launch_bounds__(256) void resample_aa_adjoint_kernel(const RsArgs p, float supy, float supx, float invy, float invx) {
  __shared__ at_axis<AT_NX, AT_TW> axx;
  __shared__ at_axis<AT_NY, AT_TH> axy;
  __shared__ float patch[AT_NY * AT_PP];
  __shared__ __attribute__((aligned(16))) float mid[AT_NY * AT_MP];
  const int tid = threadIdx.x, lane = tid & 63;
  const rs_frame f = rs_frame_of<AT_TH, AT_TW>(p);            // f.src: the (b, c) plane of g, h x w
  const int y1 = min(f.y0 + AT_TH, p.H), x1 = min(f.x0 + AT_TW, p.W);
  const int basey = at_base<MODE>(f.y0, p.ry), basex = at_base<MODE>(f.x0, p.rx);
  if (tid == 0) axx.range[0] = AT_NX, axx.range[1] = -1, axy.range[0] = AT_NY, axy.range[1] = -1;
  __syncthreads();
  if (tid < 128) at_candidate<MODE>(axx, tid, basex, f.x0, x1, p.W, p.w, p.rx, supx, invx);
  else at_candidate<MODE>(axy, tid - 128, basey, f.y0, y1, p.H, p.h, p.ry, supy, invy);
  __syncthreads();
  if (tid < 128) at_table<MODE>(axx, tid, f.x0, x1, invx);
  else at_table<MODE>(axy, tid - 128, f.y0, y1, invy);
  // the coarse patch: rows oy0 .. oy0 + ny - 1, columns ox0 .. ox0 + nx - 1 of g (both ranges hold at least one window)
  const int ny = axy.range[1] - axy.range[0] + 1, nx = axx.range[1] - axx.range[0] + 1;
  const int oy0 = basey + axy.range[0], ox0 = basex + axx.range[0];
  for (int r = tid >> 6; r < ny; r += 4)
    for (int q = lane; q < nx; q += 64) patch[r * AT_PP + q] = f.src[(size_t)(oy0 + r) * p.w + ox0 + q];
  __syncthreads();                                // the tables and the patch

  {                                               // horizontal pass: this thread's fine column, every fourth coarse row
    const int fx = axx.first[lane], cx = axx.cnt[lane];
    float wx[AT_COVER];
#pragma unroll
    for (int k = 0; k < AT_COVER; ++k) wx[k] = axx.wgt[k][lane];
    for (int o = tid >> 6; o < ny; o += 4) {
      const float* row = patch + o * AT_PP + fx;
      float t = 0.f;
      if (cx > 0) {
        t = wx[0] * row[0];
#pragma unroll
        for (int k = 1; k < AT_COVER; ++k)
          if (k < cx) t = fmaf(wx[k], row[k], t);
      }
      mid[o * AT_MP + lane] = t;
    }
  }
  __syncthreads();

  const int xl = f.x0 + 4 * (tid & 15);
  float none[RS_NM];                              // rs_emit's sums: not touched when it stores
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int i = (tid >> 4) + 16 * half, y = f.y0 + i;
    if (y >= p.H || xl >= p.W) continue;
    const int fy = axy.first[i], cy = axy.cnt[i];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < AT_COVER; ++k) {
      if (k < cy) {
        const float wy = axy.wgt[k][i];
        const float4 m = *reinterpret_cast<const float4*>(mid + (fy + k) * AT_MP + 4 * (tid & 15));
        const float mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = k == 0 ? wy * mv[j] : fmaf(wy, mv[j], acc[j]);
      }
    }
    rs_emit<false>(p, f, y, xl, acc, none);
  }
}

// ---- the launch of both entries -------------------------------------------------------------------------------------------------
// ceil(tile * in / out) + 4: no window of a tile at this ratio is larger (a bicubic footprint is the span of the floors + 4)
inline int64_t rs_footprint(int tile, int n_in, int n_out) { return ((int64_t)tile * n_in + n_out - 1) / n_out + 4; }

// The adjoint kernel's tables hold AT_COVER windows per fine coordinate.  The windows of one axis, lo and hi by aa_window's
// arithmetic: true when lo and hi do not decrease with o and no fine coordinate lies in more than AT_COVER of them (window
// o - AT_COVER ends at or before window o begins).  O(n_out) on the host, per call.
inline bool at_windows_fit(int n_in, int n_out, float ratio, float sup) {
  int his[AT_COVER], plo = 0, phi = 0;
  for (int o = 0; o < n_out; ++o) {
    const float center = ratio * ((float)o + 0.5f);
    const int a = (int)((center - sup) + 0.5f), b = (int)((center + sup) + 0.5f);
    const int lo = std::min(std::max(a, 0), n_in - 1), hi = std::max(std::min(b, n_in), lo + 1);
    if (lo < plo || hi < phi) return false;
    if (o >= AT_COVER && his[o % AT_COVER] > lo) return false;
    his[o % AT_COVER] = hi, plo = lo, phi = hi;
  }
  return true;
}

template <bool MOMENTS>
int rs_launch(RsArgs p, int B, int mode, hipStream_t s) {
  if (!p.x || (MOMENTS ? (!p.sums || !p.target) : !p.out) || (p.scale == nullptr) != (p.shift == nullptr)) return O2_ERR_ARG;
  if (B <= 0 || p.C <= 0 || p.in_ctotal <= 0 || p.h <= 0 || p.w <= 0 || p.H <= 0 || p.W <= 0) return O2_ERR_ARG;
  // 0, 1, 2 plain; bilinear and bicubic also with ORBIT2_ANTIALIAS (5, 6); nearest has no antialiased form.  ORBIT2_TRANSPOSE
  // goes with 5 and 6 of orbit2_resample_fwd alone (21, 22): the adjoint of the coarsening (H, W) -> (h, w), no gather, no affine
  const bool tr = !MOMENTS && (mode == (1 | ORBIT2_ANTIALIAS | ORBIT2_TRANSPOSE) || mode == (2 | ORBIT2_ANTIALIAS | ORBIT2_TRANSPOSE));
  const int base = tr ? mode ^ ORBIT2_TRANSPOSE : mode;
  const bool aa = base == (1 | ORBIT2_ANTIALIAS) || base == (2 | ORBIT2_ANTIALIAS);
  if (!aa && (mode < 0 || mode > 2)) return O2_ERR_ARG;
  if (!p.chan_idx && p.C != p.in_ctotal) return O2_ERR_ARG;
  if (tr && (p.chan_idx || p.C != p.in_ctotal || p.scale || p.shift || p.h > p.H || p.w > p.W)) return O2_ERR_ARG;
  if (MOMENTS && (p.Ht < p.H || p.Wt < p.W)) return O2_ERR_ARG;
  if ((int64_t)B * p.C > 65535) return O2_ERR_ARG;
  const int th = tr ? AT_TH : (aa ? AA_TH : RS_TH), tw = tr ? AT_TW : (aa ? AA_TW : RS_TW);
  p.ntx = (p.W + tw - 1) / tw;
  const int nty = (p.H + th - 1) / th;
  if ((int64_t)p.ntx * nty > INT32_MAX) return O2_ERR_ARG;
  if (MOMENTS && hipMemsetAsync(p.sums, 0, sizeof(double) * (size_t)B * p.C * RS_NM, s) != hipSuccess) return O2_ERR_LAUNCH;
  const int stage = rs_footprint(RS_TH, p.h, p.H) * rs_footprint(RS_TW, p.w, p.W) <= RS_LDS;
  const dim3 grid(p.ntx * nty, B * p.C);
  // the two ratios of the contract, one correctly rounded fp32 division each: formed here once, not by every thread
  // (the adjoint's windows are those of the forward call that coarsens out's grid to x's: its ratios are that call's)
  const float ry = p.ry = tr ? (float)p.H / (float)p.h : (float)p.h / (float)p.H;
  const float rx = p.rx = tr ? (float)p.W / (float)p.w : (float)p.w / (float)p.W;
  // support and inverse scale of the antialiased contract, one fp32 operation each: a window spans interp / 2 source pixels per
  // unit of max(ratio, 1) to either side of its centre
  const float half = base == (1 | ORBIT2_ANTIALIAS) ? 1.f : 2.f;
  const float supy = ry >= 1.f ? half * ry : half, supx = rx >= 1.f ? half * rx : half;
  const float invy = ry >= 1.f ? 1.f / ry : 1.f, invx = rx >= 1.f ? 1.f / rx : 1.f;
  // more windows on a fine pixel than the adjoint's tables hold: refused, never clipped in silence
  if (tr && !(at_windows_fit(p.H, p.h, ry, supy) && at_windows_fit(p.W, p.w, rx, supx))) return O2_ERR_ARG;
  switch (mode) {
    case 0: hipLaunchKernelGGL((resample_kernel<0, MOMENTS>), grid, dim3(256), 0, s, p, stage); break;
    case 1: hipLaunchKernelGGL((resample_kernel<1, MOMENTS>), grid, dim3(256), 0, s, p, stage); break;
    case 2: hipLaunchKernelGGL((resample_kernel<2, MOMENTS>), grid, dim3(256), 0, s, p, stage); break;
    case 1 | ORBIT2_ANTIALIAS:
      hipLaunchKernelGGL((resample_aa_kernel<1, MOMENTS>), grid, dim3(256), 0, s, p, supy, supx, invy, invx); break;
    case 2 | ORBIT2_ANTIALIAS:
      hipLaunchKernelGGL((resample_aa_kernel<2, MOMENTS>), grid, dim3(256), 0, s, p, supy, supx, invy, invx); break;
    case 1 | ORBIT2_ANTIALIAS | ORBIT2_TRANSPOSE:
      hipLaunchKernelGGL((resample_aa_adjoint_kernel<1>), grid, dim3(256), 0, s, p, supy, supx, invy, invx); break;
    default: hipLaunchKernelGGL((resample_aa_adjoint_kernel<2>), grid, dim3(256), 0, s, p, supy, supx, invy, invx); break;
  }
  O2_CHECK_LAUNCH();
  return O2_OK;
}
}  // namespace

extern "C" int orbit2_resample_fwd(const float* x, const int* chan_idx, int in_ctotal, const float* scale, const float* shift,
                                   float* out, int B, int C, int h, int w, int H, int W, int mode, void* stream) {
  const RsArgs p{x, chan_idx, scale, shift, out, nullptr, nullptr, nullptr, nullptr, in_ctotal, 0, 0, C, h, w, H, W};
  return rs_launch<false>(p, B, mode, (hipStream_t)stream);
}

extern "C" int orbit2_resample_moments(const float* x, const int* chan_idx, int in_ctotal, const float* scale,
                                       const float* shift, const float* target, int Ht, int Wt, const float* lat_w,
                                       const float* clim, double* out, int B, int C, int h, int w, int H, int W, int mode,
                                       void* stream) {
  const RsArgs p{x, chan_idx, scale, shift, nullptr, target, lat_w, clim, out, in_ctotal, Ht, Wt, C, h, w, H, W};
  return rs_launch<true>(p, B, mode, (hipStream_t)stream);
}
