"""Plain references for the nine kernels of csrc/lpips.hip (the `perceptual` losses), and the shapes and inputs their edge tests share.

Every function takes `dtype`: torch.float64 is the reference; torch.float32 is the *fp32 baseline*, the same formulas in fp32 on
the CPU, whose distance from the float64 result is what the tolerances of the GPU tests are taken from (never the kernel's own
output).  Inputs are rounded to the kernel's storage type by the caller (bf16 feature maps, fp32 images and weights).

Feature maps are NHWC, handed over as [N*H*W, C]; images are NCHW.  Where a bound needs one, a function also returns a companion
`A` / `G`: the same sum over the absolute values of its terms, as conv_fwd / conv_bwd of rowimage_ref do.
"""
import torch
import torch.nn.functional as F

from oracle import orbit2_oracle as O
from tests.rowimage_ref import BF, EPS8, EPS24, F32, F64, base_err, excess, fp32_floor, rt  # noqa: F401  (shared helpers)

TAP_EPS = 1e-10
TRIP = 8192 * 256                         # items of one trip of grid_for's grid-stride loops


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def baseline(base, ref, A):
    """b per element: the fp32 baseline's largest error in units of the companion A, over the tensor, times A; never below one
    fp32 rounding of A (rowimage_ref.fp32_floor).  One element's own baseline error is a single sample of a rounding error and
    bounds nothing; the largest over the tensor, scaled by each element's magnitude, does."""
    A = A.double()
    err = (base.double() - ref).abs()
    rel = torch.where(A > 0, err / A.clamp_min(1e-300), torch.zeros_like(err))
    rel = float(rel.max()) if rel.numel() else 0.0
    return fp32_floor(rel * A, A)


def bound_bf16(base, ref, A):
    """a bf16 output of fp32 arithmetic: one bf16 rounding of the result + 4 b"""
    return EPS8 * ref.abs() + 4.0 * baseline(base, ref, A)


def bound_f32(base, ref, A):
    return 4.0 * baseline(base, ref, A)


def f32(s):
    """a scalar as a C `float` argument receives it"""
    return float(torch.tensor(s, dtype=F32))


def nhwc(t):
    """[N,C,H,W] -> [N*H*W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def nchw(t, N, H, W):
    """[N*H*W, C] -> [N,C,H,W]"""
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ---- im2col / col2im ---------------------------------------------------------------------------------------------------------
def im2col(x, N, H, W, C):
    """col[p][t][c] = x[p + off_t][c], zero outside the image; t = ky*3 + kx, off = (ky-1, kx-1).  Moves values: any dtype."""
    pad = F.pad(x.reshape(N, H, W, C), (0, 0, 1, 1, 1, 1))
    return torch.stack([pad[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 3).reshape(N * H * W, 9 * C)


def col2im(dcol, N, H, W, C, act=None, tapg=None, dtype=F64):
    """g[p][c] = sum_t dcol[p - off_t][t][c]; with act: (g + tapg) * (act > 0).  Returns g, A.  The nine terms are added in the
    order of t, one tap at a time (the 300 MB case never holds more than one tap in `dtype`)."""
    d = dcol.reshape(N, H, W, 9, C)
    g = torch.zeros(N, H + 2, W + 2, C, dtype=dtype)
    A = torch.zeros(N, H + 2, W + 2, C, dtype=dtype)
    for t in range(9):
        ky, kx = t // 3, t % 3
        term = d[:, :, :, t].to(dtype)
        g[:, ky:ky + H, kx:kx + W] += term
        A[:, ky:ky + H, kx:kx + W] += term.abs()
    g, A = g[:, 1:H + 1, 1:W + 1].reshape(N * H * W, C), A[:, 1:H + 1, 1:W + 1].reshape(N * H * W, C)
    if act is None:
        assert tapg is None
        return g, A
    keep = act.reshape(N * H * W, C) > 0
    if tapg is not None:
        tg = tapg.reshape(N * H * W, C).to(dtype)
        g, A = g + tg, A + tg.abs()
    return g * keep, A * keep


# ---- 2x2 max-pool ------------------------------------------------------------------------------------------------------------
def _windows(x, N, H, W, C):
    """[N, H/2, W/2, 4, C]: the four positions of every window in row-major order"""
    return x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def _unwindows(w, N, H, W, C):
    return w.reshape(N, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N * H * W, C)


def maxpool_fwd(x, N, H, W, C):
    """selects values: exact in any dtype"""
    return _windows(x, N, H, W, C).amax(3).reshape(N * (H // 2) * (W // 2), C)


def first_argmax(x, N, H, W, C):
    """am [N, H/2, W/2, C]: the first position, in row-major window order, that holds the window's maximum; tied: whether a
    later position holds the same value"""
    w = _windows(x if x.dtype == F64 else x.float(), N, H, W, C)
    m, am = w[:, :, :, 0].clone(), torch.zeros(w[:, :, :, 0].shape, dtype=torch.int64)
    for j in range(1, 4):
        up = w[:, :, :, j] > m
        m, am = torch.where(up, w[:, :, :, j], m), torch.where(up, torch.full_like(am, j), am)
    tied = (w == m.unsqueeze(3)).sum(3) > 1
    return am, tied


def maxpool_bwd(g, x, N, H, W, C, tapg=None):
    """dz[pos] = ((pos == first argmax ? g : 0) + tapg[pos]) * (x[pos] > 0), as bf16.  g + tapg is formed in fp32 and rounded
    once to bf16, as the kernel does: routing, mask and that one rounding are all exact, so the result is compared bit for bit."""
    am, _ = first_argmax(x, N, H, W, C)
    gw = g.float().reshape(N, H // 2, W // 2, 1, C)
    v = torch.where(am.unsqueeze(3) == torch.arange(4).view(1, 1, 1, 4, 1), gw, torch.zeros(()))
    v = _unwindows(v, N, H, W, C)
    if tapg is not None:
        v = v + tapg.float().reshape(N * H * W, C)
    return torch.where(x.reshape(N * H * W, C) > 0, v, torch.zeros(())).to(BF)


# ---- first convolution -------------------------------------------------------------------------------------------------------
def _w1_oihw(w1, dtype):
    """w1 [(t*3 + ci)][co] -> [co][ci][ky][kx]"""
    return w1.to(dtype).reshape(3, 3, 3, 64).permute(3, 2, 0, 1).contiguous()


def _scaling(dtype):
    return (torch.tensor(O.LPIPS_SHIFT, dtype=dtype).view(1, 3, 1, 1), torch.tensor(O.LPIPS_SCALE, dtype=dtype).view(1, 3, 1, 1))


def conv1_fwd(img, w1, b1, dtype=F64):
    """relu(conv3x3((img - shift) / scale) + b1) as [N*H*W, 64], and A"""
    shift, scale = _scaling(dtype)
    x, w, b = (img.to(dtype) - shift) / scale, _w1_oihw(w1, dtype), b1.to(dtype)
    out = F.relu(F.conv2d(x, w, b, padding=1))
    return nhwc(out), nhwc(F.conv2d(x.abs(), w.abs(), b.abs(), padding=1))


def conv1_bwd_parts(dz, w1, N, H, W, dtype=F64):
    """the transposed convolution before the division by the scale, [N,3,H,W], and the same over absolute values: the 64-channel
    products of every tap as one matrix product, the nine taps placed by col2im.  With dz and w1 on a grid on which every
    576-term sum is exact in fp32, dtype = float32 gives the exact result (the 2 M-pixel case, where float64 would take
    gigabytes)."""
    d, w = dz.to(dtype), w1.to(dtype)
    lp, _ = col2im(d @ w.t(), N, H, W, 3, dtype=dtype)
    G, _ = col2im(d.abs() @ w.abs().t(), N, H, W, 3, dtype=dtype)
    return nchw(lp, N, H, W), nchw(G, N, H, W)


def conv1_bwd(dz, w1, pred, target, l1_coef, gscale=None, dtype=F64, parts=None):
    """dimg [N,3,H,W] = conv_transpose(dz) / scale + l1_coef * gscale * sign(pred - target), sign(0) = 0; and G.  l1_coef is
    taken as the C entry receives it (fp32).  parts: conv1_bwd_parts computed beforehand (exact-grid inputs)."""
    N, _, H, W = pred.shape
    _, scale = _scaling(dtype)
    lp, G = parts if parts is not None else conv1_bwd_parts(dz, w1, N, H, W, dtype)
    c = f32(l1_coef) * (1.0 if gscale is None else float(gscale))
    sgn = torch.sign(pred.to(dtype) - target.to(dtype))
    return lp.to(dtype) / scale + c * sgn, G.to(dtype) / scale + abs(c) * sgn.abs()


# ---- LPIPS head of one tap -----------------------------------------------------------------------------------------------------
def _tap_parts(f, lin, B, dtype):
    a, t, w = f[:B].to(dtype), f[B:].to(dtype), lin.to(dtype)
    r0, r1 = a.pow(2).sum(-1, keepdim=True).sqrt(), t.pow(2).sum(-1, keepdim=True).sqrt()
    i0, i1 = 1.0 / (r0 + TAP_EPS), 1.0 / (r1 + TAP_EPS)
    return a, w, r0, i0, a * i0 - t * i1, a.abs() * i0 + t.abs() * i1


def tap_fwd(f, lin, B, dtype=F64):
    """f [2B, HW, C] (prediction images first).  val [B] = mean over pixels of sum_c lin_c (n0_c - n1_c)^2, and A: the same with
    |n0_c| + |n1_c| for the difference (the difference cancels: its rounding error is measured by the sum, not by itself)"""
    a, w, r0, i0, e, ea = _tap_parts(f, lin, B, dtype)
    return (w * e * e).sum(-1).mean(-1), (w.abs() * ea * ea).sum(-1).mean(-1)


def tap_bwd(f, lin, coef, B, gscale=None, dtype=F64):
    """gradient [B, HW, C] of coef * gscale * sum_pixels sum_c lin_c (n0_c - n1_c)^2 with respect to the prediction half, with the
    +1e-10 in the norm, times the ReLU mask a > 0; 0 at an all-zero pixel.  coef as the C entry receives it (fp32).  And G."""
    a, w, r0, i0, e, ea = _tap_parts(f, lin, B, dtype)
    c = f32(coef) * (1.0 if gscale is None else float(gscale))
    live = r0 > 0
    rs = torch.where(live, r0, torch.ones_like(r0))
    k2 = torch.where(live, (2.0 * w * e * a).sum(-1, keepdim=True) * i0 * i0 / rs, torch.zeros_like(r0))
    k2a = torch.where(live, (2.0 * w.abs() * ea * a.abs()).sum(-1, keepdim=True) * i0 * i0 / rs, torch.zeros_like(r0))
    keep = a > 0
    g = c * (2.0 * w * e * i0 - a * k2)
    G = abs(c) * (2.0 * w.abs() * ea * i0 + a.abs() * k2a)
    return g * keep, G * keep


def l1_mean(a, b, dtype=F64):
    return (a.to(dtype) - b.to(dtype)).abs().mean()


# ---- shapes the GPU tests and the CPU baseline test share ------------------------------------------------------------------------
COL_SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (4, 7))
POOL_SIZES = ((2, 2), (2, 6), (6, 2), (4, 8))
CONV1_SIZES = ((1, 1), (1, 4), (3, 1), (2, 2), (5, 7), (16, 16))
BATCHES = (1, 3)
CHANNELS = (8, 64, 512)
TAP_CHANNELS = (64, 128, 256, 512)
TAP_SWITCH = ((512, 256), (512, 257), (64, 2048), (64, 2049))      # (C, HW): 64 | 65 partials
TAP_TRIP = ((512, 4099), (64, 32771))                              # past the 1024-block cap
L1_SIZES = (1, 255, 256, 257, 16384, 16385)                        # the last two: 64 | 65 partials
L1_PREFILL = 0.625
TAP_COEF, GSCALE = 0.25, 0.375


def tap_ppb(C):
    """pixels per block of the tap kernels: 256 lanes, C / 8 lanes per pixel"""
    return 256 // (C // 8)


def tap_blocks(C, HW):
    return min(1024, (HW * (C // 8) + 255) // 256)


def tap_hws(C):
    return tuple(sorted({1, 3, tap_ppb(C) - 1, tap_ppb(C) + 1}))


def col_inputs(N, H, W, C, grid):
    """x, dcol, act, tapg (bf16 values as fp32).  grid: dcol and tapg are multiples of 1/4 in [-1, 1], so every sum of nine terms
    plus tapg is a multiple of 1/4 below 64: exact in fp32 and in bf16.  act has zeros and negative values."""
    g = torch.Generator().manual_seed(31 + 7 * H + W + 3 * N + C)
    x = rt(torch.randn(N * H * W, C, generator=g))
    if grid:
        dcol = torch.randint(-4, 5, (N * H * W, 9 * C), generator=g).float() / 4
        tapg = torch.randint(-4, 5, (N * H * W, C), generator=g).float() / 4
    else:
        dcol, tapg = rt(torch.randn(N * H * W, 9 * C, generator=g)), rt(torch.randn(N * H * W, C, generator=g) * 0.3)
    act = torch.randint(-1, 3, (N * H * W, C), generator=g).float() / 2
    return x, dcol, act, tapg


def pool_inputs(N, H, W, C):
    """x on five levels {-1, -1/2, 0, 1/2, 1} (ties in most windows, zeros and negative values), g and tapg bf16 normals"""
    g = torch.Generator().manual_seed(41 + 7 * H + W + 3 * N + C)
    x = torch.randint(-2, 3, (N * H * W, C), generator=g).float() / 2
    gy = rt(torch.randn(N * (H // 2) * (W // 2), C, generator=g))
    return x, gy, rt(torch.randn(N * H * W, C, generator=g))


def conv1_weights():
    g = torch.Generator().manual_seed(51)
    return torch.randn(27, 64, generator=g) * (2.0 / 27) ** 0.5, torch.randn(64, generator=g) * 0.5


def conv1_inputs(N, H, W):
    """img with channel 2 offset by 3 (a swapped shift, scale or channel shows); pred and target multiples of 2^-6 that agree
    wherever the flat element index is a multiple of 3; dz bf16 normals"""
    g = torch.Generator().manual_seed(61 + 7 * H + W + 3 * N)
    img = torch.randn(N, 3, H, W, generator=g) * 0.6
    img[:, 2] += 3.0
    pred = torch.randint(-256, 257, (N, 3, H, W), generator=g).float() / 64
    target = torch.randint(-256, 257, (N, 3, H, W), generator=g).float() / 64
    tie = (torch.arange(pred.numel()) % 3 == 0).view(pred.shape)
    target = torch.where(tie, pred, torch.where(target == pred, target + 0.5, target))
    dz = rt(torch.randn(N * H * W, 64, generator=g))
    return img, pred, target, tie, dz


def tap_inputs(C, HW, B):
    """f [2B, HW, C] = relu(normal) in bf16, lin >= 0; an all-zero prediction pixel (image 0, pixel 0), an all-zero target pixel
    (image B-1, the last pixel), and from HW = 3 a prediction pixel with one nonzero channel (image 0, pixel HW // 2)"""
    g = torch.Generator().manual_seed(71 + C + 5 * HW + B)
    f = rt(torch.relu(torch.randn(2 * B, HW, C, generator=g)))
    f[0, 0] = 0.0
    f[2 * B - 1, HW - 1] = 0.0
    if HW >= 3:
        f[0, HW // 2] = 0.0
        f[0, HW // 2, C // 3] = 1.5
    return f, torch.rand(C, generator=g) * (2.0 / C)


def l1_inputs(n):
    g = torch.Generator().manual_seed(81 + n % 1000)
    a = torch.randint(-256, 257, (n,), generator=g).float() / 64
    b = torch.randint(-256, 257, (n,), generator=g).float() / 64
    b[::5] = a[::5]
    return a, b
