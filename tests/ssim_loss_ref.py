"""References of the SSIM vector-Jacobian product (orbit2_loss_bwd at kind ORBIT2_LOSS_SSIM_VJP = 3; include/orbit2_hip.h,
DESIGN 4.10h), the backward of orbit2_ssim's sums.

ssim_sum64()     float64 torch: sum over the valid centres of w_k S_k of one image, S by box filters as the header defines it
vjp64()          d [B,C,H,W] float64 = coef[bc] * autograd gradient of ssim_sum64 with respect to pred: what the kernel approximates
closed_form64()  the header's closed form (alpha, beta, gamma, five box sums, any pivot) in float64 numpy
emulate()        the kernel's operations in the kernel's order, every one rounded to fp32: tile by tile, the two pivots, the
                 row sums and the seven-deep ring added oldest first, the three folded maps, the box sums rows then columns
No GPU."""
import numpy as np
import torch

F = np.float32
WIN, HALO, RAD = 7, 6, 3
LOSS_SSIM_VJP = 3                                   # ORBIT2_LOSS_SSIM_VJP
TILE_H, TILE_W = 16, 64                             # ORBIT2_SSIM_VJP_TILE_H, _TILE_W (checked against the header)
STRIPS = 3                                          # centre-row strips of a tile: a thread owns one column of one strip
OFFSETS = (0.0, 280.0)

# the shapes the field tolerance is measured on (pred (H, W); the target is two rows and four columns larger and cropped)
TOL_SHAPES = ((7, 7), (13, 9), (39, 71))
# the worst |emulate - vjp64| / max|d of the image| over TOL_SHAPES, offsets 0 and 280, with and without lat_w, rounded up
# (tests/test_ssim_loss_cpu.py::test_emulation_against_float64 measures it and holds it within 0.5x .. 1x)
EMUL_WORST = 7.8e-7
# GPU bound on |kernel - vjp64| / max|d of the image|: 4 x, the margin of tests/coarsen_ref.py, for the same reason -- the
# device may contract a product and a sum into an fma, and reorder, within what the contract leaves free
FIELD_TOL = 4 * EMUL_WORST

# ---- the cases the GPU tests run: pred (H, W), target (Ht, Wt), offsets -------------------------------------------------------------
GPU_CASES = (
    ((7, 7), (7, 7), (0.0,)),                       # exactly one window
    ((7, 200), (7, 200), (0.0,)),                   # thin bands: one centre row, four tiles across, W % 4 == 0
    ((200, 7), (200, 7), (0.0,)),                   # one centre column, thirteen tiles down
    ((39, 71), (41, 75), OFFSETS),                  # a cropped target, tile seams in both axes at either tile height, W % 4 == 3
    ((33, 132), (33, 132), (280.0,)),               # W % 4 == 0 with seams in both axes: the 16-byte stores next to a seam
)
GPU_B, GPU_C = 2, 3
GPU_COEF = ((0.75, -1.25, 2.0), (0.03125, 1.0, -0.5))          # distinct, both signs
GPU_RANGE = ((5.0, 4.0, 6.5), (3.5, 8.0, 5.5))                # distinct given ranges


def make_pair(hw, thw, offset, seed=None, B=GPU_B, C=GPU_C):
    """(pred [B,C,H,W], target [B,C,Ht,Wt]) fp32: a smooth field of range about 5 plus noise, at `offset`; the prediction is the
    target's crop plus noise"""
    (H, W), (Ht, Wt) = hw, thw
    rng = np.random.default_rng(H * 1000 + W + 31 if seed is None else seed)
    yy, xx = np.arange(Ht)[:, None] / 11.0, np.arange(Wt)[None, :] / 17.0
    ph = rng.uniform(0, 6.28, (B, C, 1, 1))
    target = offset + 1.5 * np.sin(yy + ph) + 1.0 * np.cos(xx - ph) + 0.3 * rng.standard_normal((B, C, Ht, Wt))
    pred = target[..., :H, :W] + 0.4 * rng.standard_normal((B, C, H, W))
    return pred.astype(F), target.astype(F)


def lat_weights(H):
    w = np.cos(np.deg2rad(np.linspace(-80, 80, H)))
    return (w / w.mean()).astype(F)


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
def _box_windows(t):
    """sum over every 7 x 7 window that lies inside t [H,W] (torch): [H-6, W-6], the 49 shifted views added"""
    H, W = t.shape
    out = torch.zeros(H - HALO, W - HALO, dtype=t.dtype)
    for dy in range(WIN):
        for dx in range(WIN):
            out = out + t[dy:dy + H - HALO, dx:dx + W - HALO]
    return out


def ssim_map64(x, y, R):
    """S at every valid centre, float64 torch [H-6, W-6]; the variances from fields centred on the target's mean"""
    c = y.mean().detach()
    a, b = x - c, y - c
    n = WIN * WIN
    ma, mb = _box_windows(a) / n, _box_windows(b) / n
    va = (_box_windows(a * a) - n * ma * ma) / (n - 1)
    vb = (_box_windows(b * b) - n * mb * mb) / (n - 1)
    vab = (_box_windows(a * b) - n * ma * mb) / (n - 1)
    ux, uy = ma + c, mb + c
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    return (2 * ux * uy + c1) * (2 * vab + c2) / ((ux * ux + uy * uy + c1) * (va + vb + c2))


def ssim_sum64(x, y, R, lat_w=None):
    S = ssim_map64(x, y, R)
    if lat_w is not None:
        S = S * torch.as_tensor(np.asarray(lat_w, np.float64))[RAD:RAD + S.shape[0], None]
    return S.sum()


def vjp64(pred, target, lat_w, coef, R):
    """float64 numpy [B,C,H,W]: coef[b][c] * d ssim_sum64 / d pred, the target read through its top-left crop"""
    pred = np.asarray(pred)
    B, C, H, W = pred.shape
    out = np.zeros(pred.shape, np.float64)
    for b in range(B):
        for c in range(C):
            if coef[b][c] == 0:
                continue
            x = torch.tensor(pred[b, c].astype(np.float64), requires_grad=True)
            y = torch.tensor(np.asarray(target)[b, c, :H, :W].astype(np.float64))
            (g,) = torch.autograd.grad(ssim_sum64(x, y, float(R[b][c]), lat_w), x)
            out[b, c] = float(coef[b][c]) * g.numpy()
    return out


def _np_box(a):
    """numpy: sum of a [h,w] over the centres within 3 rows and 3 columns of every pixel of the (h + 6) x (w + 6) image"""
    p = np.pad(a, HALO)
    h, w = a.shape
    out = np.zeros((h + HALO, w + HALO), a.dtype)
    for dy in range(WIN):
        for dx in range(WIN):
            out += p[dy:dy + h + HALO, dx:dx + w + HALO]
    return out


def closed_form64(x, y, R, lat_w=None, g=1.0, pivot=None):
    """the header's closed form for one image in float64 numpy: x, y [H,W] (y the target's crop)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    H, W = x.shape
    v = float(y[0, 0]) if pivot is None else float(pivot)
    a, b = torch.tensor(x - v), torch.tensor(y - v)
    n = WIN * WIN
    ma, mb = (_box_windows(a) / n).numpy(), (_box_windows(b) / n).numpy()
    va = (_box_windows(a * a).numpy() - n * ma * ma) / (n - 1)
    vb = (_box_windows(b * b).numpy() - n * mb * mb) / (n - 1)
    vab = (_box_windows(a * b).numpy() - n * ma * mb) / (n - 1)
    ux, uy = ma + v, mb + v
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + c1, 2 * vab + c2, ux * ux + uy * uy + c1, va + vb + c2
    S = A1 * A2 / (B1 * B2)
    alpha = 2 * A2 / (B1 * B2) * (uy - ux * A1 / B1)
    beta = -S / B2
    gamma = 2 * A1 / (B1 * B2)
    w = np.ones((H - HALO, 1)) if lat_w is None else np.asarray(lat_w, np.float64)[RAD:RAD + H - HALO, None]
    d = _np_box(w * alpha) / n + (2 * ((x - v) * _np_box(w * beta) - _np_box(w * beta * ma))
                                  + (y - v) * _np_box(w * gamma) - _np_box(w * gamma * mb)) / (n - 1)
    return g * d


# ---- the kernel's fp32 order --------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf: the product of two fp32 values is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _emulate_tile(p, t, lat_w, g, R, py0, px0, TH, TW):
    """the TH x TW values a workgroup computes for the tile at (py0, px0) of one image (p [H,W], t [Ht,Wt] fp32)"""
    H, W = p.shape
    PH, PW, MH, MW = TH + 2 * HALO, TW + 2 * HALO, TH + HALO, TW + HALO
    RS = (MH + STRIPS - 1) // STRIPS
    inv_n, inv_n1 = F(1.0) / F(WIN * WIN), F(1.0) / F(WIN * WIN - 1)
    R = F(R)
    c1, c2 = (F(0.01) * R) * (F(0.01) * R), (F(0.03) * R) * (F(0.03) * R)
    pivot = t[py0, px0]
    sa, sb = np.zeros((PH, PW), F), np.zeros((PH, PW), F)
    ys, xs = np.arange(py0 - HALO, py0 - HALO + PH), np.arange(px0 - HALO, px0 - HALO + PW)
    iy, ix = np.flatnonzero((ys >= 0) & (ys < H)), np.flatnonzero((xs >= 0) & (xs < W))
    sa[np.ix_(iy, ix)] = p[np.ix_(ys[iy], xs[ix])] - pivot
    sb[np.ix_(iy, ix)] = t[np.ix_(ys[iy], xs[ix])] - pivot
    maps = np.zeros((3, MH, MW), F)
    cols = np.arange(MW)
    cx = px0 - RAD + cols
    pcol = np.maximum(np.minimum(cols + RAD, W - 1 - px0 + HALO), HALO - px0)
    for strip in range(STRIPS):
        mr0 = strip * RS
        prow = max(min(min(mr0 + RAD + RS // 2, PH - 1), H - 1 - py0 + HALO), HALO - py0)
        local = sb[prow, pcol]                                              # [MW]
        shift = local + pivot
        rows = []
        for j in range(RS + HALO):
            pr = min(mr0 + j, PH - 1)
            a = np.stack([sa[pr, cols + k] - local for k in range(WIN)])
            b = np.stack([sb[pr, cols + k] - local for k in range(WIN)])
            s = [np.zeros(MW, F) for _ in range(5)]
            for k in range(WIN):
                s[0] = s[0] + a[k]
                s[1] = s[1] + b[k]
                s[2] = _fma(a[k], a[k], s[2])
                s[3] = _fma(b[k], b[k], s[3])
                s[4] = _fma(a[k], b[k], s[4])
            rows.append(s)
            mr = mr0 + j - HALO
            if j < HALO or mr >= MH:
                continue
            w = []
            for q in range(5):
                v = rows[j - HALO][q]                                       # oldest first
                for k in range(j - HALO + 1, j + 1):
                    v = v + rows[k][q]
                w.append(v)
            cy = py0 - RAD + mr
            valid = (RAD <= cy < H - RAD) & (cx >= RAD) & (cx < W - RAD)
            ma, mb = w[0] * inv_n, w[1] * inv_n
            va, vb, vab = (w[2] - w[0] * ma) * inv_n1, (w[3] - w[1] * mb) * inv_n1, (w[4] - w[0] * mb) * inv_n1
            ux, uy = ma + shift, mb + shift
            A1, A2 = F(2) * ux * uy + c1, F(2) * vab + c2
            B1, B2 = ux * ux + uy * uy + c1, va + vb + c2
            rB = F(1) / (B1 * B2)
            S = A1 * A2 * rB
            alpha = F(2) * A2 * rB * ((mb - ma) * (uy * (ux + uy) + c1)) / B1
            beta = -S / B2
            gamma = F(2) * A1 * rB
            mx, my = ma + local, mb + local
            wk = F(lat_w[cy]) if (lat_w is not None and 0 <= cy < H) else F(1)
            e0 = wk * (alpha * inv_n - (F(2) * beta * mx + gamma * my) * inv_n1)
            e1 = wk * (F(2) * beta * inv_n1)
            e2 = wk * (gamma * inv_n1)
            for q, e in enumerate((e0, e1, e2)):
                maps[q, mr] = np.where(valid, e, F(0))
    hb = maps[:, :, 0:TW].copy()
    for k in range(1, WIN):
        hb = hb + maps[:, :, k:k + TW]
    bx = hb[:, 0:TH].copy()
    for dy in range(1, WIN):
        bx = bx + hb[:, dy:dy + TH]
    xa, ya = sa[HALO:HALO + TH, HALO:HALO + TW], sb[HALO:HALO + TH, HALO:HALO + TW]
    return F(g) * _fma(ya, bx[2], _fma(xa, bx[1], bx[0]))


def emulate(pred, target, lat_w, coef, R, tile=(TILE_H, TILE_W)):
    """fp32 [B,C,H,W] in the built order; an image of coefficient 0 is zero-filled without being read"""
    pred, target = np.asarray(pred, F), np.asarray(target, F)
    lat_w = None if lat_w is None else np.asarray(lat_w, F)
    B, C, H, W = pred.shape
    TH, TW = tile
    out = np.zeros(pred.shape, F)
    with np.errstate(all="ignore"):
        for b in range(B):
            for c in range(C):
                if F(coef[b][c]) == 0:
                    continue
                for py0 in range(0, H, TH):
                    for px0 in range(0, W, TW):
                        d = _emulate_tile(pred[b, c], target[b, c], lat_w, coef[b][c], R[b][c], py0, px0, TH, TW)
                        out[b, c, py0:py0 + TH, px0:px0 + TW] = d[:H - py0, :W - px0]
    return out


def worst_error(got, want):
    """the largest |got - want| / max|want of the image| over the images whose reference is not all zero"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    B, C = want.shape[:2]
    worst = 0.0
    for b in range(B):
        for c in range(C):
            top = np.abs(want[b, c]).max()
            if top > 0:
                worst = max(worst, float(np.abs(got[b, c] - want[b, c]).max() / top))
    return worst
