"""numpy references of the antialiased modes of orbit2_resample_fwd / orbit2_resample_moments (mode | ORBIT2_ANTIALIAS;
include/orbit2_hip.h), in the manner of tests/resample_ref.py.

taps_aa()       the contract's fp32 window rule: first source index, tap count and normalised fp32 weights (zero-padded to the
                longest window) of every output coordinate
replica_aa()    the resampled field, the taps weighted and summed in float64: what the kernel approximates
emulate_aa()    the same field in the kernel's stated fp32 order: a row interpolant is a product then fused multiply-adds over
                ascending taps, rounded to fp32; a pixel its rows' interpolants top to bottom in the same way; then the affine
emulate_moments_aa()  the twelve sums with the antialiased kernel's fp32 part: a thread's four pixels added in fp32, the 64 lanes
                of a wave (four tile rows of sixteen threads) by the xor butterfly in fp32, everything above in float64
The float64 sums are resample_ref.moments64.  No torch, no GPU."""
import math

import numpy as np

from tests import resample_ref as R

MODES = ("bilinear", "bicubic")
ANTIALIAS = 4                                       # ORBIT2_ANTIALIAS
TILE_H, TILE_W, CHUNK_ROWS = 16, 64, 32             # ORBIT2_AA_TILE_H, _TILE_W, _CHUNK_ROWS (checked against the header)
SRC_FLOATS, WX_FLOATS, WY_FLOATS = 6144, 3072, 768  # ORBIT2_AA_SRC_FLOATS, _WX_FLOATS, _WY_FLOATS
F = np.float32

# the pairs of sizes of the issue, (h, w), (H, W), and one that shrinks the rows and grows the columns
SHAPES = (((40, 56), (5, 7)), ((128, 256), (32, 64)), ((17, 23), (6, 10)), ((721, 1440), (91, 180)), ((9, 13), (1, 1)),
          ((8, 8), (8, 8)), ((5, 7), (40, 56)), ((30, 64), (8, 16)), ((24, 5), (7, 19)))
OFFSETS = R.OFFSETS


def _filter(mode, x):
    """f(x) in fp32, every product rounded on its own"""
    x = np.abs(x).astype(F)
    if mode == "bilinear":
        return np.where(x < 1, F(1) - x, F(0)).astype(F)
    assert mode == "bicubic", mode
    inner = (F(1.5) * x - F(2.5)) * x * x + F(1)
    outer = (((x - F(5)) * x + F(8)) * x - F(4)) * F(-0.5)
    return np.where(x < 1, inner, np.where(x < 2, outer, F(0))).astype(F)


def windows(mode, n_in, n_out):
    """(lo int64 [n_out], n int64 [n_out], center fp32 [n_out], inv fp32): every line is one fp32 operation"""
    half = F(1) if mode == "bilinear" else F(2)
    ratio = F(n_in) / F(n_out)
    sup = half * ratio if ratio >= 1 else half
    inv = F(1) / ratio if ratio >= 1 else F(1)
    o = np.arange(n_out, dtype=F)
    center = ratio * (o + F(0.5))
    a = ((center - sup) + F(0.5)).astype(np.int64)
    b = ((center + sup) + F(0.5)).astype(np.int64)
    lo = np.minimum(np.maximum(a, 0), n_in - 1)
    hi = np.maximum(np.minimum(b, n_in), lo + 1)
    assert center.dtype == F and F(sup).dtype == F
    return lo, hi - lo, center, F(inv)


def taps_aa(mode, n_in, n_out):
    """(lo int64 [n_out], n int64 [n_out], w fp32 [n_out, K]): K the longest window, the weights past a window's end are 0"""
    lo, n, center, inv = windows(mode, n_in, n_out)
    K = int(n.max())
    j = np.arange(K, dtype=np.int64)[None, :]
    arg = (((j + lo[:, None]).astype(F) - center[:, None]) + F(0.5)) * inv
    raw = np.where(j < n[:, None], _filter(mode, arg), F(0)).astype(F)
    total = np.zeros(n_out, F)
    for q in range(K):                                               # ascending taps, fp32
        total = total + raw[:, q]
    w = np.where(total[:, None] != 0, raw / np.where(total == 0, F(1), total)[:, None], raw).astype(F)
    return lo, n, w


def max_taps(mode, n_in, n_out):
    """the header's bound on a window: 2 ceil(support) + 1, or the whole axis"""
    ratio = n_in / n_out
    sup = (1 if mode == "bilinear" else 2) * max(ratio, 1.0)
    return min(n_in, 2 * math.ceil(sup) + 1)


def _gather(x, lo, q, axis):
    idx = np.minimum(lo + q, x.shape[axis] - 1)                      # a padded tap has weight 0 and reads the last pixel
    return np.take(x, idx, axis=axis)


def replica_aa(x, size, mode, channels=None, scale=None, shift=None):
    """float64 [B,C,H,W]"""
    x = R._select(x, channels).astype(np.float64)
    (ylo, _, wy), (xlo, _, wx) = taps_aa(mode, x.shape[2], size[0]), taps_aa(mode, x.shape[3], size[1])
    rows = sum(wx[:, q].astype(np.float64) * _gather(x, xlo, q, 3) for q in range(wx.shape[1]))                 # [B,C,h,W]
    out = sum(wy[:, k].astype(np.float64)[:, None] * _gather(rows, ylo, k, 2) for k in range(wy.shape[1]))
    if scale is not None:
        out = np.asarray(scale, np.float64)[None, :, None, None] * out + np.asarray(shift, np.float64)[None, :, None, None]
    return out


def emulate_aa(x, size, mode, channels=None, scale=None, shift=None):
    """fp32 [B,C,H,W] in the built order (a padded tap adds 0 * finite = 0: it changes no bit)"""
    x = R._select(x, channels).astype(F)
    (ylo, _, wy), (xlo, _, wx) = taps_aa(mode, x.shape[2], size[0]), taps_aa(mode, x.shape[3], size[1])
    rows = wx[:, 0] * _gather(x, xlo, 0, 3)
    for q in range(1, wx.shape[1]):
        rows = R._fma(np.broadcast_to(wx[:, q], rows.shape), _gather(x, xlo, q, 3), rows)
    out = wy[:, 0][:, None] * _gather(rows, ylo, 0, 2)
    for k in range(1, wy.shape[1]):
        out = R._fma(np.broadcast_to(wy[:, k][:, None], out.shape), _gather(rows, ylo, k, 2), out)
    if scale is not None:
        sc = np.broadcast_to(np.asarray(scale, F)[None, :, None, None], out.shape)
        sh = np.broadcast_to(np.asarray(shift, F)[None, :, None, None], out.shape)
        out = R._fma(sc, out, sh)
    return out.astype(F)


def tile_fits(mode, hw, HW):
    """whether every tile of the pair keeps its weights and a staged chunk in LDS (the header's rule, with the bound on the
    windows in place of their lengths: the tests use it to know which path a case exercises, nothing more)"""
    (h, w), (H, W) = hw, HW
    kx, ky = max_taps(mode, w, W), max_taps(mode, h, H)
    lo, n, _ = taps_aa(mode, w, W)
    fw = max(int(lo[min(c + TILE_W, W) - 1] + n[min(c + TILE_W, W) - 1] - lo[c]) for c in range(0, W, TILE_W))
    return TILE_W * kx <= WX_FLOATS and TILE_H * ky <= WY_FLOATS and (fw | 1) <= SRC_FLOATS


def emulate_moments_aa(field, target, lat_w=None, clim=None):
    """[B,C,12] float64: fp32 summands, a thread's four columns added in fp32, the wave's 64 lanes (lane = 16 (row % 4) + column
    group) by the butterfly in fp32, waves and tiles in float64"""
    field = np.asarray(field, F)
    a, b, w = R._ab(field, np.asarray(target, F), None if lat_w is None else np.asarray(lat_w, F),
                    None if clim is None else np.asarray(clim, F))
    t = R._terms(a.astype(F), b.astype(F), np.broadcast_to(w.astype(F), a.shape))
    assert t.dtype == F
    _, B, C, H, W = t.shape
    nty, ntx = -(-H // TILE_H), -(-W // TILE_W)
    pad = np.zeros((12, B, C, nty * TILE_H, ntx * TILE_W), F)
    pad[..., :H, :W] = t
    # [12,B,C, ty, wave, row in wave, tx, column group, j]
    v = pad.reshape(12, B, C, nty, 4, 4, ntx, 16, 4)
    lane = np.zeros(v.shape[:-1], F)
    for j in range(4):
        lane = lane + v[..., j]
    lane = np.moveaxis(lane, 6, 5).reshape(12, B, C, nty, 4, ntx, 64)             # lane index = 16 row + column group
    for _ in range(6):
        lane = lane[..., : lane.shape[-1] // 2] + lane[..., lane.shape[-1] // 2:]
    return np.moveaxis(lane.astype(np.float64).sum((3, 4, 5, 6)), 0, -1)


# ---- the cases the GPU tests run (tests/test_resample_aa_gpu.py), shared with the CPU test that derives their bounds ------------
# (h, w), (H, W): B = 2, five input channels of which resample_ref.GPU_CHANNELS are read
GPU_CASES = (
    ((40, 56), (5, 7)),                        # integer 8x: row windows that straddle the chunks of 32 rows
    ((80, 24), (8, 5)),                        # 10x: a bicubic row window of 41 rows, longer than a chunk
    ((64, 512), (16, 128)),                    # integer 4x, two tiles across, several chunks down
    ((17, 23), (6, 10)),                       # non-integer, window lengths differ between neighbours, odd w
    ((40, 150), (TILE_H + 1, TILE_W + 1)),     # one row and one column past a whole tile
    ((40, 150), (TILE_H - 1, TILE_W - 1)),     # one short of it, odd W: every second row misaligned
    ((300, 7), (1, 1)),                        # the whole axis in one window: weights formed in place, taps from global memory
    ((7, 300), (1, 1)),
    ((1, 6500), (2, 3)),                       # a footprint row longer than ORBIT2_AA_SRC_FLOATS
    ((8, 8), (8, 8)),                          # the identity
    ((5, 7), (40, 56)),                        # an upsample
    ((24, 5), (7, 19)),                        # rows shrink, columns grow
    ((6, 70), (13, 9)),                        # rows grow, columns shrink
)
GPU_CHANNELS, GPU_SCALE, GPU_SHIFT = R.GPU_CHANNELS, R.GPU_SCALE, R.GPU_SHIFT


def gpu_input(hw, offset):
    return (R.make_input(hw, 2, 5, seed=hw[0] * 1000 + hw[1]) + F(offset)).astype(F)


# ---- bounds (derived in tests/test_resample_aa_cpu.py, used by the GPU tests) ------------------------------------------------------
ULP = R.ULP


def ceiling(mode, hw, HW):
    """a derivable bound on |fp32 in the built order - replica| / max|x| for one pair of sizes.  Both use the same fp32
    weights (their rounding is in neither difference), so only the sums differ.  With u = 2^-24 and S the largest sum of
    |weight| of a window (1 for bilinear; the cubic's negative lobes give 1.25 at most over these cases, checked in
    tests/test_resample_aa_cpu.py, taken as 1.5): each of the n operations of a row interpolant rounds a partial sum bounded
    by S max|x|, an error of at most u S max|x|; each of the m operations of the vertical pass rounds a partial sum bounded by
    S^2 max|x|, and the pass carries the row interpolants' errors times S.  Together (n + m) S^2 u."""
    S = 1.0 if mode == "bilinear" else 1.5
    n, m = max_taps(mode, hw[1], HW[1]), max_taps(mode, hw[0], HW[0])
    return (n + m) * S * S * ULP


# the worst the emulation shows, in units of max|x|, over SHAPES and GPU_CASES at offsets 0 and 280, rounded up
# (test_emulation_against_replica measures and holds these).  The error of a long fp32 sum grows with its length, so the pairs
# whose windows are too long for the LDS tables (tile_fits false: hundreds to thousands of taps) are recorded on their own.
EMUL_WORST = {("bilinear", True): 5.1 * ULP, ("bicubic", True): 7.8 * ULP,
              ("bilinear", False): 28.2 * ULP, ("bicubic", False): 73.7 * ULP}


def field_tol(mode, hw, HW):
    """GPU bound on |kernel - replica| / max|x|: 4 x the emulation's worst, capped by the pair's ceiling"""
    return min(4 * EMUL_WORST[(mode, tile_fits(mode, hw, HW))], ceiling(mode, hw, HW))


# the twelve sums: worst |emulate_moments_aa(emulate_aa(x)) - moments64(replica_aa(x))| / sum |summand| over the GPU cases, per
# (offset, tile_fits), rounded up; the GPU bound is 4 x.  What shows is the field's own rounding on a difference of order 1
# (a - b, a - clim), so the long windows and the offset stand out.
MOMENTS_EMUL_WORST = {(0, True): 2.5e-7, (280, True): 4.8e-5, (0, False): 9.1e-6, (280, False): 1.07e-2}
MOMENTS_RTOL = {k: 4 * v for k, v in MOMENTS_EMUL_WORST.items()}
