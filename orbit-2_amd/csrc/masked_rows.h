// What the kernels that sweep the VALID pixels of a scored pair share (loss.hip, extremes.hip): the mask operand, the four-pixel
// work item with its float4 / scalar path choice and alignment rule, and the entry point of the extreme-value kernels.
// score_sums.h keeps what every evaluation kernel needs.
//
//   valid(b,c,i,j) = isfinite(target[b,c,i,j]) and (mask == NULL or mask[b,c,i,j] != 0)
#pragma once
#include "score_sums.h"

struct MaskArg {
  const uint8_t* m;                  // NULL: no mask
  int pitch;                         // bytes (= elements) between two rows
  int64_t sb, sc;                    // batch and channel strides; 0 = broadcast
};

// One row of one (b, c) plane around the item's columns j0 .. j0+3:
//   pv[k], vv[k]  k = 0..5  <->  column j0 - 1 + k   (pv = 0 and vv = false outside the plane or where invalid is irrelevant:
//                                                    pv is only ever used under vv)
//   tc[k]         k = 0..3  <->  target at column j0 + k (only meaningful where vv[k + 1])
// EDGES = false: columns j0-1 and j0+4 are not read (vv false).
template <bool VEC, bool EDGES>
__device__ __forceinline__ void load_row(const float* __restrict__ p, const float* __restrict__ t, const uint8_t* __restrict__ m,
                                         int i, int j0, int H, int W, int Wt, int mp, float (&pv)[6], bool (&vv)[6],
                                         float (&tc)[4]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) { pv[k] = 0.f; vv[k] = false; }
#pragma unroll
  for (int k = 0; k < 4; ++k) tc[k] = 0.f;
  if (i < 0 || i >= H) return;
  const float* pr = p + (size_t)i * W;
  const float* tr = t + (size_t)i * Wt;
  const uint8_t* mr = m ? m + (size_t)i * mp : nullptr;
  if (VEC) {                                           // W % 4 == 0: the whole group is inside the row
    const f32x4 p4 = *reinterpret_cast<const f32x4*>(pr + j0);
    const f32x4 t4 = *reinterpret_cast<const f32x4*>(tr + j0);
    const uint32_t m4 = mr ? *reinterpret_cast<const uint32_t*>(mr + j0) : 0x01010101u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pv[k + 1] = p4[k];
      tc[k] = t4[k];
      vv[k + 1] = finite_f(t4[k]) && ((m4 >> (8 * k)) & 0xffu) != 0;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k;
      if (j < W) {
        pv[k + 1] = pr[j];
        tc[k] = tr[j];
        vv[k + 1] = finite_f(tc[k]) && (!mr || mr[j] != 0);
      }
    }
  }
  if (EDGES) {
    if (j0 > 0) {
      pv[0] = pr[j0 - 1];
      vv[0] = finite_f(tr[j0 - 1]) && (!mr || mr[j0 - 1] != 0);
    }
    if (j0 + 4 < W) {
      pv[5] = pr[j0 + 4];
      vv[5] = finite_f(tr[j0 + 4]) && (!mr || mr[j0 + 4] != 0);
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the mask argument as given; false if it cannot be what it says
inline bool mask_arg(MaskArg& mk, const uint8_t* mask, int pitch, int64_t sb, int64_t sc, int Ht, int Wt, int W) {
  mk.m = mask; mk.pitch = pitch; mk.sb = sb; mk.sc = sc;
  if ((int64_t)Ht * Wt > 0x7fffffff) return false;                   // a plane is indexed with 32 bits
  return !mask || (pitch >= W && sb >= 0 && sc >= 0);
}
// float4 / dword centres: every row of every operand starts aligned (and W % 4 == 0: no partial group)
inline bool vec_ok(const float* pred, const float* target, const MaskArg& mk, int W, int Wt) {
  if (W % 4 || Wt % 4 || !aligned(pred, 16) || !aligned(target, 16)) return false;
  return !mk.m || (aligned(mk.m, 4) && mk.pitch % 4 == 0 && mk.sb % 4 == 0 && mk.sc % 4 == 0);
}

// ---- the extreme-value kernels (extremes.hip), reached through orbit2_masked_loss_fwd (loss.hip) at the kinds
// ORBIT2_MASKED_QUANTILES and ORBIT2_MASKED_TAIL: not an export, so the library's dynamic symbols stay those of the header.
// The caller has checked the pair, out, cnt, ws and the mask operand; base / flags / n are the fields of the entry's kind word.
__attribute__((visibility("hidden"))) int o2_masked_extremes(const float* pred, const float* target, int Ht, int Wt,
                                                             const MaskArg& mk, const float* lat_w, const float* chan_w,
                                                             float* out, int64_t* cnt, float* ws, int B, int C, int H, int W,
                                                             int base, int flags, int n, hipStream_t s);

// ---- the fractions skill score (fss.hip), reached the same way at the kind ORBIT2_FSS_KIND; T and n are the threshold count and
// the window of the kind word, flags its ORBIT2_MASKED_PER_IMAGE / ORBIT2_MASKED_LOWER bits
__attribute__((visibility("hidden"))) int o2_masked_fss(const float* pred, const float* target, int Ht, int Wt, const MaskArg& mk,
                                                        const float* lat_w, const float* chan_w, float* out, int64_t* cnt,
                                                        float* ws, int B, int C, int H, int W, int flags, int T, int n,
                                                        hipStream_t s);
