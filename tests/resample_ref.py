"""numpy references of orbit2_resample_fwd / orbit2_resample_moments (include/orbit2_hip.h).

taps()          the contract's fp32 coordinate rule: source indices and fp32 weights of every output coordinate
replica()       the resampled field, the taps weighted and summed in float64: what the kernel approximates
emulate()       the same field in the kernel's own fp32 summation order (a product, then fused multiply-adds, left to right and
                top to bottom, then the affine): how far fp32 in that order can be from the replica
moments64()     the twelve sums of orbit2_eval_moments over a float64 field
emulate_moments()  those sums with the kernel's fp32 part: a lane's at most TILE_H / 4 x 4 pixels added in fp32, the 64 lanes of a
                wave by the xor butterfly in fp32, everything above in float64
No torch, no GPU: the CPU tests compare these with ATen and the golden file, the GPU tests compare the kernels with these."""
import numpy as np

MODES = ("nearest", "bilinear", "bicubic")
TILE_H, TILE_W, LDS_FLOATS = 32, 256, 10240       # ORBIT2_RESAMPLE_TILE_H, _TILE_W, _LDS_FLOATS (checked against the header)
F = np.float32

# the eight pairs of sizes of the issue: (h, w), (H, W)
SHAPES = (((5, 7), (40, 56)), ((16, 32), (128, 256)), ((6, 10), (17, 23)), ((32, 64), (180, 360)), ((91, 180), (721, 1440)),
          ((9, 13), (4, 5)), ((3, 4), (3, 4)), ((1, 1), (8, 8)))
OFFSETS = (0.0, 280.0)


def case_key(hw, HW, mode=None, offset=None):
    key = "%dx%d_%dx%d" % (hw + HW)
    if mode is not None:
        key += ".%s.%d" % (mode, int(offset))
    return key


def taps(mode, n_in, n_out):
    """(idx int64 [n_out, T], w fp32 [n_out, T]), T = 1, 2, 4: every line is one fp32 operation, rounded on its own"""
    o = np.arange(n_out, dtype=F)
    ratio = F(n_in) / F(n_out)
    if mode == "nearest":
        i = np.minimum(np.floor(o * ratio).astype(np.int64), n_in - 1)
        return i[:, None], np.ones((n_out, 1), F)
    s = ratio * (o + F(0.5))
    s = s - F(0.5)
    if mode == "bilinear":
        s = np.maximum(s, F(0))
        i0 = s.astype(np.int64)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = s - i0.astype(F)
        l0 = F(1) - l1
        return np.stack([i0, i1], 1), np.stack([l0, l1], 1).astype(F)
    assert mode == "bicubic", mode
    fl = np.floor(s)
    t = s - fl
    base = fl.astype(np.int64)
    A = F(-0.75)
    x0, x1, x2, x3 = t + F(1), t, F(1) - t, F(2) - t
    w = np.stack([((A * x0 - F(5) * A) * x0 + F(8) * A) * x0 - F(4) * A,
                  ((A + F(2)) * x1 - (A + F(3))) * x1 * x1 + F(1),
                  ((A + F(2)) * x2 - (A + F(3))) * x2 * x2 + F(1),
                  ((A * x3 - F(5) * A) * x3 + F(8) * A) * x3 - F(4) * A], 1)
    assert w.dtype == F
    idx = np.clip(base[:, None] - 1 + np.arange(4)[None, :], 0, n_in - 1)
    return idx, w


def _select(x, channels):
    x = np.asarray(x)
    return x if channels is None else x[:, list(channels)]


def replica(x, size, mode, channels=None, scale=None, shift=None):
    """float64 [B,C,H,W]"""
    x = _select(x, channels).astype(np.float64)
    (iy, wy), (ix, wx) = taps(mode, x.shape[2], size[0]), taps(mode, x.shape[3], size[1])
    rows = sum(wx[:, q].astype(np.float64) * x[..., ix[:, q]] for q in range(ix.shape[1]))            # [B,C,h,W]
    out = sum(wy[:, k].astype(np.float64)[:, None] * rows[..., iy[:, k], :] for k in range(iy.shape[1]))
    if scale is not None:
        out = np.asarray(scale, np.float64)[None, :, None, None] * out + np.asarray(shift, np.float64)[None, :, None, None]
    return out


def _fma(a, b, c):
    """fmaf: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def emulate(x, size, mode, channels=None, scale=None, shift=None):
    """fp32 [B,C,H,W] in the built summation order"""
    x = _select(x, channels).astype(F)
    (iy, wy), (ix, wx) = taps(mode, x.shape[2], size[0]), taps(mode, x.shape[3], size[1])
    if mode == "nearest":
        out = x[..., iy[:, 0], :][..., ix[:, 0]]
    else:
        rows = wx[:, 0] * x[..., ix[:, 0]]                       # a row interpolant depends on the source row and the column only
        for q in range(1, ix.shape[1]):
            rows = _fma(np.broadcast_to(wx[:, q], rows.shape), x[..., ix[:, q]], rows)
        out = wy[:, 0][:, None] * rows[..., iy[:, 0], :]
        for k in range(1, iy.shape[1]):
            out = _fma(np.broadcast_to(wy[:, k][:, None], out.shape), rows[..., iy[:, k], :], out)
    if scale is not None:
        sc = np.broadcast_to(np.asarray(scale, F)[None, :, None, None], out.shape)
        sh = np.broadcast_to(np.asarray(shift, F)[None, :, None, None], out.shape)
        out = _fma(sc, out, sh)
    return out.astype(F)


def staged(h, w, H, W):
    """the header's rule for staging a tile's source window in LDS"""
    return (-(-TILE_H * h // H) + 4) * (-(-TILE_W * w // W) + 4) <= LDS_FLOATS


def _terms(a, b, w):
    """the twelve summands of orbit2_eval_moments, [12, ...] in the dtype of a"""
    d = a - b
    return np.stack([a, b, a * a, b * b, a * b, w * d * d, w * np.abs(d), w * a, w * b, w * a * b, w * a * a, w * b * b])


def _ab(field, target, lat_w, clim):
    B, C, H, W = field.shape
    t = np.asarray(target)[:, :, :H, :W]
    c = 0 if clim is None else np.asarray(clim)[None]
    w = np.ones(H, F) if lat_w is None else np.asarray(lat_w)[:H]
    return field - c, t - c, w[None, None, :, None]


def moments64(field, target, lat_w=None, clim=None):
    """([B,C,12] float64 sums, [B,C,12] sums of the summands' magnitudes: the scale a rounding error is measured on)"""
    a, b, w = _ab(np.asarray(field, np.float64), np.asarray(target, np.float64), None if lat_w is None else
                  np.asarray(lat_w, np.float64), None if clim is None else np.asarray(clim, np.float64))
    t = _terms(a, b, np.broadcast_to(w, a.shape))
    return np.moveaxis(t.sum((-2, -1)), 0, -1), np.moveaxis(np.abs(t).sum((-2, -1)), 0, -1)


def emulate_moments(field, target, lat_w=None, clim=None):
    """[B,C,12] float64: fp32 summands, a lane's pixels (rows wave, wave + 4, ... of the tile, four columns each) added in fp32
    in the kernel's order, the wave's 64 lanes by the butterfly in fp32, waves and tiles in float64"""
    field = np.asarray(field, F)
    a, b, w = _ab(field, np.asarray(target, F), None if lat_w is None else np.asarray(lat_w, F),
                  None if clim is None else np.asarray(clim, F))
    a, b = a.astype(F), b.astype(F)
    t = _terms(a, b, np.broadcast_to(w.astype(F), a.shape))
    assert t.dtype == F
    _, B, C, H, W = t.shape
    nty, ntx = -(-H // TILE_H), -(-W // TILE_W)
    pad = np.zeros((12, B, C, nty * TILE_H, ntx * TILE_W), F)       # a pixel outside the image adds nothing
    pad[..., :H, :W] = t
    # [12,B,C, ty, i, wave, tx, lane, j]: row = ty TILE_H + 4 i + wave, column = tx TILE_W + 4 lane + j
    v = pad.reshape(12, B, C, nty, TILE_H // 4, 4, ntx, 64, 4)
    lane = np.zeros(v.shape[:4] + (4, ntx, 64), F)
    for i in range(TILE_H // 4):
        for j in range(4):
            lane = lane + v[:, :, :, :, i, :, :, :, j]
    for _ in range(6):                                               # xor butterfly: every level adds the two halves
        lane = lane[..., : lane.shape[-1] // 2] + lane[..., lane.shape[-1] // 2:]
    return np.moveaxis(lane.astype(np.float64).sum((3, 4, 5, 6)), 0, -1)


def make_input(hw, B, C, seed):
    """the fp32 randn field of a pair of sizes at offset 0; offset 280 is (x + 280) rounded to fp32"""
    return np.random.default_rng(seed).standard_normal((B, C) + tuple(hw)).astype(F)


# ---- the cases the GPU tests run (tests/test_resample_gpu.py), shared with the CPU test that derives their bounds ----------------
# (h, w), (H, W), B, Cin, channels: five pairs of the golden file, whose B = 2, C = 3 inputs sit in input channels 4, 0, 2 of a
# five-channel field, and one pair of 3 x 3 tiles (non-integer ratio, odd W: two whole tiles and a partial one each way)
GPU_CHANNELS = (4, 0, 2)
GPU_CASES = (((5, 7), (40, 56)), ((6, 10), (17, 23)), ((9, 13), (4, 5)), ((1, 1), (8, 8)), ((3, 4), (3, 4)),
             ((9, 130), (2 * TILE_H + 3, 2 * TILE_W + 5)))
GPU_SCALE, GPU_SHIFT = (1.75, -0.5, 0.03125), (-3.0, 0.25, 100.0)


def gpu_input(hw, HW, offset, golden=None):
    """fp32 [2, 5, h, w]: the golden file's input of the pair (or a seeded randn field where it has none) in channels 4, 0, 2,
    other values in channels 1 and 3, everything at `offset`"""
    x = make_input(hw, 2, 5, seed=hw[0] * 1000 + hw[1])
    key = case_key(hw, HW) + ".x"
    if golden is not None and key in golden:
        x[:, list(GPU_CHANNELS)] = golden[key]
    return (x + F(offset)).astype(F)


def gpu_target(HW, offset, seed=5):
    """(target fp32 [2, 3, H + 3, W + 5] with NaN outside the H x W crop, lat_w fp32 [H], clim fp32 [3, H, W])"""
    H, W = HW
    rng = np.random.default_rng(seed + H * 7 + W)
    t = np.full((2, 3, H + 3, W + 5), np.nan, F)
    t[:, :, :H, :W] = rng.standard_normal((2, 3, H, W)) + offset
    lat = np.cos(np.deg2rad(np.linspace(-80.0, 75.0, H))).astype(F)
    clim = (0.5 * rng.standard_normal((3, H, W)) + offset).astype(F)
    return t, lat, clim


# ---- bounds (derived in tests/test_resample_cpu.py, used by the GPU tests) --------------------------------------------------------
ULP = 2.0 ** -24
# derivable ceilings of |fp32 in the built order - replica| / max|x|: bilinear 4 taps with non-negative weights that sum to 1,
# bicubic 16 taps with sum |w| <= 1.375^2 plus the rounding of the weight polynomials
CEILING = {"nearest": 0.0, "bilinear": 8 * ULP, "bicubic": 64 * ULP}
# the worst the emulation shows over the eight pairs of the golden file and the GPU cases at offsets 0 and 280, rounded up
# (test_emulation_against_replica measures 3.29 and 4.91 ulp and holds these)
EMUL_WORST = {"nearest": 0.0, "bilinear": 3.3 * ULP, "bicubic": 5.0 * ULP}
# GPU bound on |kernel - replica| / max|x|: a factor 4 for what the emulation leaves out (the compiler's own contraction of the
# weight polynomials, double rounding in the emulated fmaf), capped by the ceiling
FIELD_TOL = {m: min(4 * EMUL_WORST[m], CEILING[m]) for m in MODES}
# the twelve sums: worst |emulate_moments(emulate(x)) - moments64(replica(x))| / sum |summand| over the GPU cases, per offset
# (at 280 the field's own rounding, half an ulp of 280 on a difference of order 1, is what shows), rounded up; the GPU bound is 4 x
MOMENTS_EMUL_WORST = {0: 1.6e-7, 280: 2.9e-5}
MOMENTS_RTOL = {k: 4 * v for k, v in MOMENTS_EMUL_WORST.items()}
