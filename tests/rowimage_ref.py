"""Plain references for the row kernels (LayerNorm, AdamW) and the image-tail kernels (3x3 convolution, losses), and the inputs
the edge tests share.

Every function takes `dtype`: torch.float64 is the reference; torch.float32 is the *fp32 baseline*, the same formulas in fp32 on
the CPU, whose distance from the float64 result is what the fp32 tolerances of the GPU tests are taken from (never the kernel's
own output).  Inputs are rounded to the kernel's storage type by the caller (bf16 rows for LayerNorm, fp32 images), so reference
and kernel read the same numbers.
"""
import math

import torch
import torch.nn.functional as F

from oracle import orbit2_oracle as O

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
EPS24 = 2.0 ** -24          # one fp32 rounding (half an ulp, relative)
EPS8 = 2.0 ** -8            # one bf16 rounding


def rt(t):
    """round trip through bf16: what a bf16 kernel reads, as fp32"""
    return t.to(BF).float()


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def base_err(base, ref, dim=None):
    """largest absolute error of an fp32 baseline against the float64 reference: over `dim` (per row / per column), or over all"""
    e = (base.double() - ref).abs()
    return e.amax(dim) if dim is not None else e.max()


def fp32_floor(b, ref_scale):
    """A measured baseline error below one fp32 rounding of the quantity is luck, not a measure (sums of few bf16 values are
    often exact in fp32, and then 4 x 0 would ask the kernel for the exact result): the baseline is never taken smaller than
    2^-24 of the quantity's magnitude."""
    return torch.maximum(torch.as_tensor(b, dtype=F64), EPS24 * torch.as_tensor(ref_scale, dtype=F64))


def excess(got, ref, bound):
    """the share of its bound the worst element uses, max |got - ref| / bound: <= 1 passes; NaN, or an error under a zero bound: inf"""
    err = (got.detach().cpu().double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps=1e-5, dtype=F64):
    """y [rows, D], mean [rows], rstd [rows]"""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1) + eps)
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def ln_bwd(dy, x, gamma, dres=None, sinks=None, beta_acc=0.0, eps=1e-5, dtype=F64):
    """dx [rows, D] (+ dres), dgamma [D], dbeta [D]; with sinks = (dgamma0, dbeta0) the sums are added to beta_acc * sink"""
    dy, x, gamma = dy.to(dtype), x.to(dtype), gamma.to(dtype)
    _, mean, rstd = ln_fwd(x, gamma, torch.zeros_like(gamma), eps, dtype)
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    s1, s2 = g.mean(-1, keepdim=True), (g * xhat).mean(-1, keepdim=True)
    dx = rstd[:, None] * (g - s1 - xhat * s2)
    if dres is not None:
        dx = dx + dres.to(dtype)
    dgamma, dbeta = (dy * xhat).sum(0), dy.sum(0)
    if sinks is not None and beta_acc != 0.0:
        dgamma = dgamma + beta_acc * sinks[0].to(dtype)
        dbeta = dbeta + beta_acc * sinks[1].to(dtype)
    return dx, dgamma, dbeta


LN_WIDTHS = (8, 200, 512, 768, 1024, 2560, 3080, 4096, 4104, 8184, 8192)
LN_ROWS = (1, 3, 5, 17, 63, 65, 130)
LN_SWITCH = tuple((D, rows) for D in (256, 64) for rows in (32767, 32768, 32769))
LN_SINK_WIDTHS = (200, 1024, 4104)


def ln_inputs(D, rows):
    """bf16-exact x, gamma, beta, dy, dres: the first `rows` rows of one fixed draw of 130 rows (of 32769 for the longer cases), so
    what depends on the row alone is computed once per width and shared"""
    g = torch.Generator().manual_seed(1000 + D)
    gam, bet = rt(1 + 0.1 * torch.randn(D, generator=g)), rt(0.1 * torch.randn(D, generator=g))
    n = max(LN_ROWS) if rows <= max(LN_ROWS) else 32769
    assert rows <= n
    x = rt(torch.randn(n, D, generator=g) * 2 + 0.5)
    dy, dres = rt(torch.randn(n, D, generator=g)), rt(torch.randn(n, D, generator=g))
    return x[:rows].contiguous(), gam, bet, dy[:rows].contiguous(), dres[:rows].contiguous()


# ---- 3x3 convolution (+ GELU + PixelShuffle) ---------------------------------------------------------------------------------
def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def conv_fwd(x, w, b, mode=0, r=1, addend=None, dtype=F64):
    """x [B, Cin, H, W] (the selected channels).  Returns out, pre, A: A = conv2d(|x|, |w|) + |b| (+ |addend|), the sum of the
    absolute values of the terms of every element of pre (mode 0: of out)"""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    pre = F.conv2d(x, w, b, padding=1)
    A = F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)
    if mode == 0:
        if addend is not None:
            a = addend.to(dtype)[:, :, :x.shape[2], :x.shape[3]]
            return pre + a, pre, A + a.abs()
        return pre, pre, A
    return F.pixel_shuffle(F.gelu(pre), r), pre, A


def conv_bwd(dout, x, w, pre, mode=0, r=1, dtype=F64):
    """din, dweight, dbias and their absolute-value companions A_din, A_dw, A_db (the same sums over |dpre|, |w|, |x|)"""
    dout, x, w = dout.to(dtype), x.to(dtype), w.to(dtype)
    dpre = dout if mode == 0 else F.pixel_unshuffle(dout, r) * gelu_grad(pre.to(dtype))

    def grads(d, xx, ww):
        din = torch.nn.grad.conv2d_input(xx.shape, ww, d, padding=1)
        dw = torch.nn.grad.conv2d_weight(xx, ww.shape, d, padding=1)
        return din, dw, d.sum((0, 2, 3))
    return grads(dpre, x, w) + grads(dpre.abs(), x.abs(), w.abs())


CONV_SIZES = ((1, 1), (1, 5), (2, 3), (16, 16), (15, 31), (17, 33), (35, 18))
# mode, Cin, Cout, r, chan_idx (None or in_ctotal), addend (None, "same", "larger")
CONV_CHANNELS = ((0, 1, 1, 1, None, None), (0, 8, 17, 1, 11, None), (0, 3, 3, 1, None, "same"), (0, 3, 3, 1, None, "larger"),
                 (1, 8, 36, 2, None, None), (1, 2, 18, 3, None, None), (1, 5, 5, 1, None, None))


def conv_inputs(B, H, W, mode, Cin, Cout, r, ctot, addend, seed=0):
    g = torch.Generator().manual_seed(77 + seed + 13 * H + W + 101 * Cout + 7 * B)
    idx = None
    if ctot is not None:
        idx = torch.randperm(ctot, generator=g)[:Cin].to(torch.int32)
    x = torch.randn(B, ctot or Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2
    b = torch.randn(Cout, generator=g)
    add = None
    if addend == "same":
        add = torch.randn(B, Cout, H, W, generator=g)
    elif addend == "larger":
        add = torch.randn(B, Cout, H + 3, W + 2, generator=g)
    oshape = (B, Cout, H, W) if mode == 0 else (B, Cout // (r * r), H * r, W * r)
    dout = torch.randn(oshape, generator=g)
    return x, idx, w, b, add, dout


# ---- losses ----------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = ((1, 1), (1, 9), (9, 1), (24, 40), (129, 128))
LOSS_CHANW = (0.5, 3.0)
LOSS_GSCALE = 0.37


def loss_inputs(H, W, larger, B=2, C=2):
    """pred, target: multiples of 2^-6 in [-4, 4] (every difference exact in fp32), one constant 5 x 5 block in pred (ties)"""
    g = torch.Generator().manual_seed(5 + 3 * H + W + int(larger))
    pred = torch.randint(-256, 257, (B, C, H, W), generator=g).float() / 64
    Ht, Wt = (H + 5, W + 7) if larger else (H, W)
    tgt = torch.randint(-256, 257, (B, C, Ht, Wt), generator=g).float() / 64
    if H >= 9 and W >= 9:
        pred[:, :, 2:7, 3:8] = 1.25
        tgt[0, 0, 2:7, 3:8] = -0.5        # a constant target block too: the image-gradient differences tie as well
    return pred, tgt


def loss_latw(H, Ht):
    return O.lat_weights(torch.linspace(-80, 80, Ht).numpy(), H).view(-1)


def loss_fwd(pred, tgt, latw, chanw, kind, dtype=F64):
    """the C + 1 outputs of orbit2_loss_fwd (kind 0 mse, 1 bayesian_tv, 2 image gradient) through the oracle's functions"""
    pred = pred.to(dtype)
    t = O.crop_target(tgt.to(dtype), pred)
    C = pred.shape[1]
    names = ["c%d" % c for c in range(C)] if chanw is not None else None
    vw = {n: float(v) for n, v in zip(names, chanw)} if chanw is not None else None
    lw = None if latw is None else latw.to(dtype).view(1, 1, -1, 1)
    if kind == 1:
        return O.bayesian_tv(pred, t, names, vw, False, lw)
    out = O.mse(pred, t, names, vw, False, lw)
    if kind == 2:
        # O.image_gradient's second term, 0.1 * mean(|gradient difference|) * mean(channel weights), on the aggregate
        dy = (t[:, :, 1:, :] - t[:, :, :-1, :]) - (pred[:, :, 1:, :] - pred[:, :, :-1, :])
        dx = (t[:, :, :, 1:] - t[:, :, :, :-1]) - (pred[:, :, :, 1:] - pred[:, :, :, :-1])
        e2 = (dy.abs().sum() + dx.abs().sum()) / pred.numel()
        cwm = 1.0 if chanw is None else torch.as_tensor(chanw, dtype=dtype).mean()
        out = torch.cat((out[:-1], (out[-1] + 0.1 * e2 * cwm).view(1)))
    return out


def loss_bwd(pred, tgt, latw, chanw, gscale, kind):
    """float64 gradient of gscale * (aggregate loss) and G, the sum of the absolute values of its terms, per element;
    sign(0) = 0 (a tie contributes nothing).  Returns grad, G, ties (the number of zero differences met)."""
    p = pred.double()
    B, C, H, W = p.shape
    t = tgt.double()[:, :, :H, :W]
    lw = torch.ones(H, dtype=F64) if latw is None else latw.double()
    lwc = lw.view(1, 1, H, 1)
    cw = torch.ones(C, dtype=F64) if chanw is None else torch.as_tensor(chanw, dtype=F64)
    g0 = float(gscale) / p.numel()
    sq = 2.0 * (p - t) * lwc
    grad, G = sq.clone(), sq.abs()
    ties = 0

    def pair(rmin, cmin, rsub, csub, coef, wrow):
        """coef * w * |p[min] - p[sub]| (kind 2: the same of target-minus-pred differences)"""
        nonlocal ties
        d = p[:, :, rmin, cmin] - p[:, :, rsub, csub]
        if kind == 2:
            d = d - (t[:, :, rmin, cmin] - t[:, :, rsub, csub])
        ties += int((d == 0).sum())
        s = torch.sign(d) * coef * wrow
        grad[:, :, rmin, cmin] += s
        grad[:, :, rsub, csub] -= s
        G[:, :, rmin, cmin] += s.abs()
        G[:, :, rsub, csub] += s.abs()

    up, dn, lf, rg, al = slice(0, H - 1), slice(1, H), slice(0, W - 1), slice(1, W), slice(None)
    if kind == 1:
        wu = lw[:H - 1].view(1, 1, H - 1, 1)
        pair(dn, al, up, al, 0.02, wu)                 # dv
        pair(al, rg, al, lf, 0.02, lwc)                # dh
        pair(dn, rg, up, lf, 0.02 * 0.7, wu)           # d1
        pair(dn, lf, up, rg, 0.02 * 0.7, wu)           # d2
        scale = cw.view(1, C, 1, 1) * g0
        return grad * scale, G * scale.abs(), ties
    if kind == 2:
        e1, G1 = grad * cw.view(1, C, 1, 1), G * cw.view(1, C, 1, 1)
        grad, G = torch.zeros_like(p), torch.zeros_like(p)
        one = torch.ones(1, dtype=F64)
        pair(al, rg, al, lf, 0.1 * float(cw.mean()), one)
        pair(dn, al, up, al, 0.1 * float(cw.mean()), one)
        return (e1 + grad) * g0, (G1 + G) * abs(g0), ties
    scale = cw.view(1, C, 1, 1) * g0
    return grad * scale, G * scale.abs(), ties


# ---- AdamW -----------------------------------------------------------------------------------------------------------------
ADAMW = dict(lr=5e-4, beta1=0.9, beta2=0.99, eps=1e-8, wd=1e-5)


def adamw_step(p, g, m, v, step, grad_scale=1.0, dtype=F64, as_kernel_args=True, lr=5e-4, beta1=0.9, beta2=0.99, eps=1e-8,
               wd=1e-5):
    """one decoupled-decay Adam step (torch.optim.AdamW's arithmetic) on copies in `dtype`; g is what the kernel reads (fp32, or
    bf16 values).  as_kernel_args: the scalars are rounded to fp32 first, as the C entry receives them -- the bias corrections
    from the unrounded betas, as climate_learn._hip.adamw computes them (1 - float32(0.99) is 1e-6 away from 0.01)"""
    def f(s):
        return float(torch.tensor(s, dtype=F32)) if as_kernel_args else float(s)
    bc1, bc2 = f(1.0 - beta1 ** step), f(1.0 - beta2 ** step)
    lr, beta1, beta2, eps, wd, grad_scale = (f(s) for s in (lr, beta1, beta2, eps, wd, grad_scale))
    p, m, v, g = p.to(dtype), m.to(dtype), v.to(dtype), g.to(dtype) * grad_scale
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    return p, m, v
