"""torch float64 restatement of the missing-data semantics (include/orbit2_hip.h: orbit2_masked_*) -- TEST
INFRASTRUCTURE.  Deliberately whole-tensor (torch.where, shifted slices), so that it shares no loop structure with the kernels.

valid = isfinite(target) and (mask is None or mask != 0); at an invalid pixel neither pred nor target enters any arithmetic:
both are REPLACED by 0 before anything is computed (never multiplied by the validity: 0 * NaN is NaN)."""
import torch

F64 = torch.float64


def validity(pred, target, mask=None):
    """bool [B,C,H,W]; mask: [H,W], [1,1,H,W], [B,1,H,W] or [B,C,H,W] at the prediction's or the target's size (top-left crop)"""
    H, W = pred.shape[2:]
    v = torch.isfinite(target[:, :, :H, :W])
    if mask is not None:
        m = torch.as_tensor(mask)
        m = (m != 0)[..., :H, :W]
        v = v & m.expand(v.shape) if m.dim() == 4 else v & m.reshape(1, 1, H, W).expand(v.shape)
    return v


def _operands(pred, target, mask):
    H, W = pred.shape[2:]
    v = validity(pred, target, mask)
    zero = torch.zeros((), dtype=F64)
    p = torch.where(v, pred.to(F64), zero)
    t = torch.where(v, target[:, :, :H, :W].to(F64), zero)
    return p, t, v


def _weights(pred, lat_w, chan_w):
    B, C, H, W = pred.shape
    w = torch.ones(H, dtype=F64) if lat_w is None else torch.as_tensor(lat_w).reshape(-1)[:H].to(F64)
    cw = torch.ones(C, dtype=F64) if chan_w is None else torch.as_tensor(chan_w).to(F64)
    return w.view(1, 1, H, 1), cw.view(1, C, 1, 1)


def error_map(p, v, t, kind):
    """float64 [B,C,H,W]: the unweighted term stored at every pixel (0 where invalid); p and t are already zeroed there.
    kind 0 = mse, 1 = bayesian_tv: a difference term counts only if both of its pixels are valid"""
    err = (p - t) ** 2
    if kind == 1:
        def term(di, dj):                       # |p[i+di, j+dj] - p[i, j]| stored at (i, j), zero outside and where invalid
            H, W = p.shape[2:]
            i0, i1 = max(0, -di), H - max(0, di)
            j0, j1 = max(0, -dj), W - max(0, dj)
            out = torch.zeros_like(p)
            a, b = p[:, :, i0 + di:i1 + di, j0 + dj:j1 + dj], p[:, :, i0:i1, j0:j1]
            both = v[:, :, i0 + di:i1 + di, j0 + dj:j1 + dj] & v[:, :, i0:i1, j0:j1]
            out[:, :, i0:i1, j0:j1] = torch.where(both, (a - b).abs(), torch.zeros((), dtype=F64))
            return out
        err = err + 0.02 * (term(1, 0) + term(0, 1) + 0.7 * term(1, 1) + 0.7 * term(1, -1))
    return torch.where(v, err, torch.zeros((), dtype=F64))


def loss(pred, target, kind, lat_w=None, chan_w=None, mask=None, grad=False):
    """(out float64 [C+1], cnt int64 [C+1]) and, with grad=True, d out[C] / d pred (float64, 0 where invalid)"""
    p, t, v = _operands(pred, target, mask)
    if grad:
        p = p.clone().requires_grad_(True)
    w, cw = _weights(pred, lat_w, chan_w)
    num = (error_map(p, v, t, kind) * w * cw).sum((0, 2, 3))
    n = v.sum((0, 2, 3))
    per = torch.where(n > 0, num / n.clamp_min(1), torch.zeros((), dtype=F64))
    agg = num.sum() / n.sum() if int(n.sum()) > 0 else num.sum() * 0.0
    out, cnt = torch.cat((per, agg.reshape(1))), torch.cat((n, n.sum().reshape(1)))
    if not grad:
        return out, cnt
    (g,) = torch.autograd.grad(agg, p)
    return out.detach(), cnt, torch.where(v, g, torch.zeros((), dtype=F64))


def moments(pred, target, lat_w=None, clim=None, mask=None):
    """float64 [B,C,13]: the twelve sums of orbit2_eval_moments over the valid pixels, then their number"""
    H, W = pred.shape[2:]
    v = validity(pred, target, mask)
    zero = torch.zeros((), dtype=F64)
    c0 = zero if clim is None else torch.as_tensor(clim).to(F64).reshape(1, -1, H, W)
    a = torch.where(v, pred.to(F64) - c0, zero)
    b = torch.where(v, target[:, :, :H, :W].to(F64) - c0, zero)
    w, _ = _weights(pred, lat_w, None)
    wv = torch.where(v, w.expand(v.shape), zero)
    d = a - b
    parts = (a, b, a * a, b * b, a * b, wv * d * d, wv * d.abs(), wv * a, wv * b, wv * a * b, wv * a * a, wv * b * b, v.to(F64))
    return torch.stack([x.sum((2, 3)) for x in parts], dim=-1)


def _nan_aggregate(per):
    has = ~torch.isnan(per)
    agg = per[has].mean() if bool(has.any()) else torch.full((), float("nan"), dtype=F64)
    return torch.cat((per, agg.reshape(1)))


def rmse(pred, target, lat_w=None, mask=None):
    """the reference's masked rmse (metrics/functional.py:243-255) with the validity as its mask"""
    p, t, v = _operands(pred, target, mask)
    w, _ = _weights(pred, lat_w, None)
    err = torch.where(v, (p - t) ** 2 * w, torch.zeros((), dtype=F64))
    err = err / (v.to(F64).mean((1, 2, 3), keepdim=True) + 1e-9)
    per = err.mean((2, 3)).sqrt().mean(0)
    return torch.cat((per, per.mean().reshape(1)))


def mae(pred, target, lat_w=None, mask=None):
    m = moments(pred, target, lat_w, None, mask).sum(0)
    return _nan_aggregate(m[:, 6] / m[:, 12])


def mean_bias(pred, target, mask=None):
    m = moments(pred, target, None, None, mask).sum(0)
    return _nan_aggregate((m[:, 1] - m[:, 0]) / m[:, 12])


def pearson(pred, target, mask=None):
    """cosine similarity of the mean-removed valid pixels of each channel (both means over the valid pixels)"""
    p, t, v = _operands(pred, target, mask)
    C = pred.shape[1]
    per = torch.full((C,), float("nan"), dtype=F64)
    for c in range(C):
        vc = v[:, c]
        if not bool(vc.any()):
            continue
        a, b = p[:, c][vc], t[:, c][vc]
        a, b = a - a.mean(), b - b.mean()
        per[c] = (a * b).sum() / (a.norm().clamp_min(1e-8) * b.norm().clamp_min(1e-8))
    return _nan_aggregate(per)
