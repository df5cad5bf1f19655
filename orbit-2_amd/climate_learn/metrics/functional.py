"""Functional losses of the hot path on the fused HIP kernels (reference: metrics/functional.py:117-202).

mse / bayesian_tv: one forward kernel (error map + latitude / variable weights + reduction) and one backward
kernel, instead of ~15-25 elementwise ATen launches.  Argument order matches the reference."""
from typing import Dict, List, Optional

import torch

from .. import _ops


_CW_CACHE = {}


def _chan_weights(pred, var_names, var_weights):
    if var_names is None:
        return None
    assert len(var_names) == pred.shape[1], "Number of variable names must match channel dimension"
    w = tuple(float((var_weights or {}).get(v, 1.0)) for v in var_names)
    key = (w, str(pred.device))
    t = _CW_CACHE.get(key)       # cached: no host-to-device copy inside a step (a captured hipGraph forbids one)
    if t is None:
        t = _CW_CACHE[key] = torch.tensor(w, dtype=torch.float32, device=pred.device)
    return t


def _lat(lat_weights, pred):
    if lat_weights is None:
        return None
    w = lat_weights.reshape(-1).to(device=pred.device, dtype=torch.float32)
    return w[: pred.shape[2]].contiguous()      # prediction may be a top-left crop of the target grid


def _fused(pred, target, var_names, var_weights, aggregate_only, lat_weights, kind):
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    out = _ops.LossFn.apply(pred, target.float(), _lat(lat_weights, pred), _chan_weights(pred, var_names, var_weights),
                            kind)
    return out[-1] if aggregate_only else out


def mse(pred, target, var_names: Optional[List[str]] = None, var_weights: Optional[Dict[str, float]] = None,
        aggregate_only: bool = False, lat_weights=None):
    return _fused(pred, target, var_names, var_weights, aggregate_only, lat_weights, 0)


def bayesian_tv(pred, target, var_names: Optional[List[str]] = None, var_weights: Optional[Dict[str, float]] = None,
                aggregate_only: bool = False, lat_weights=None):
    return _fused(pred, target, var_names, var_weights, aggregate_only, lat_weights, 1)


def image_gradient(pred, target, var_names: Optional[List[str]] = None, var_weights: Optional[Dict[str, float]] = None,
                   aggregate_only: bool = False, lat_weights=None):
    """mean((pred-target)^2 * w_var) + 0.1 * mean(|grad(target) - grad(pred)|) * mean(w_var)  (reference :59-114;
    forward-difference gradients as torchmetrics.functional.image.image_gradients defines them).  Scalar."""
    return _fused(pred, target, var_names, var_weights, True, None, 2)


# ---- consistency with the input: the prediction, coarsened WITH antialiasing, against the field the model was
# given.  The training form of utils.visualize.consistency_scores: the coarsening has a backward (_ops.CoarsenFn, the adjoint
# kernel of the antialiased resample), the score is the fused mse. ----------------------------------------------------------------
_CONSISTENCY_IDX = {}               # (channels, device) -> the device int64 index of index_select


def _consistency_given(source, channels, rescale, device):
    """source[:, channels] * scale + shift, fp32 on `device`; the index and the affine pair are cached device tensors, so a step
    copies nothing from the host (a captured hipGraph forbids it)"""
    given = source.detach()
    if given.device != device:
        given = given.to(device)
    given = given.float()
    if channels is not None:
        chans = tuple(int(c) for c in channels)
        bad = [c for c in chans if not 0 <= c < source.shape[1]]
        if bad or not chans:
            raise ValueError("consistency_mse: channels %s outside 0..%d" % (list(chans), source.shape[1] - 1))
        key = (chans, str(device))
        idx = _CONSISTENCY_IDX.get(key)
        if idx is None:
            idx = _CONSISTENCY_IDX[key] = torch.tensor(chans, dtype=torch.int64, device=device)
        given = given.index_select(1, idx)
    if rescale is not None and rescale[0] is not None:
        scale, shift = rescale
        if not torch.is_tensor(scale):
            key = (tuple(float(v) for v in scale), tuple(float(v) for v in shift), str(device))
            pair = _CW_CACHE.get(key)
            if pair is None:
                pair = _CW_CACHE[key] = (torch.tensor(key[0], dtype=torch.float32, device=device).view(1, -1, 1, 1),
                                         torch.tensor(key[1], dtype=torch.float32, device=device).view(1, -1, 1, 1))
            scale, shift = pair
        else:
            scale, shift = scale.reshape(1, -1, 1, 1), shift.reshape(1, -1, 1, 1)
        if scale.shape[1] != given.shape[1] or shift.shape[1] != given.shape[1]:
            raise ValueError("consistency_mse: rescale needs one (scale, shift) per channel (%d), got %d and %d"
                             % (given.shape[1], scale.shape[1], shift.shape[1]))
        given = given * scale + shift
    return given.contiguous()


def consistency_mse(pred, source, var_names: Optional[List[str]] = None, var_weights: Optional[Dict[str, float]] = None,
                    aggregate_only: bool = False, lat_weights=None, mode: str = "bilinear", channels=None, rescale=None):
    """mse(coarsen(pred), given), [C + 1] as mse returns it, differentiable in pred.  pred [B,C,H,W]; source [B,V,h,w] the
    (normalised) input of the model.  With s = H // h the prediction is coarsened to (H // s, W // s) in `mode` (bilinear or
    bicubic) with antialiasing, and scored against given = source[:, channels] * scale + shift (`rescale` = (scale, shift) per
    channel moves the inputs' normalisation to the outputs', utils.loaders._interpolation_rescale), read through its top-left
    crop where the prediction covers less: the arithmetic of utils.visualize.consistency_scores.  `lat_weights` are those of
    the LOW-resolution rows.  The gradient reaches pred through the adjoint kernel of the antialiased resample."""
    from ..models.hub.interpolation import Resampled
    if isinstance(pred, Resampled):
        raise TypeError("consistency_mse: a Resampled prediction (an interpolation baseline) has no backward -- score it with "
                        "utils.visualize.consistency_scores")
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    if pred.dim() != 4 or source.dim() != 4 or source.shape[0] != pred.shape[0]:
        raise ValueError("consistency_mse takes a prediction [B,C,H,W] and a source [B,V,h,w], got %s and %s"
                         % (tuple(pred.shape), tuple(source.shape)))
    H, W = pred.shape[-2:]
    s = H // source.shape[2]
    if s < 1 or H // s > source.shape[2] or W // s > source.shape[3]:
        raise ValueError("consistency_mse: a prediction of %s does not coarsen onto a source of %s"
                         % (tuple(pred.shape), tuple(source.shape)))
    given = _consistency_given(source, channels, rescale, pred.device)
    if given.shape[1] != pred.shape[1]:
        raise ValueError("consistency_mse: %d source channels for %d predicted ones -- name them with `channels`"
                         % (given.shape[1], pred.shape[1]))
    coarse = _ops.CoarsenFn.apply(pred, (H // s, W // s), mode)
    out = _ops.LossFn.apply(coarse, given, _lat(lat_weights, coarse), _chan_weights(coarse, var_names, var_weights), 0)
    return out[-1] if aggregate_only else out


# ---- the SSIM training loss: 1 - SSIM per variable, differentiable in pred through _ops.SSIMFn, whose backward is
# the windowed vector-Jacobian kernel (orbit2_loss_bwd at kind 3) --------------------------------------------------------------------
SSIM_LOSS_TARGET_RANGE = "target"   # as a `data_range`: every image's own target range, found on the device, held constant


def _ssim_loss_range(data_range, var_names, pred):
    """None for "target", else the cached fp32 [B,C] device tensor of a float or of a dict per variable"""
    if isinstance(data_range, str):
        if data_range != SSIM_LOSS_TARGET_RANGE:
            raise ValueError("ssim_loss: data_range is a number, a dict per variable or %r, got %r"
                             % (SSIM_LOSS_TARGET_RANGE, data_range))
        return None
    B, C = pred.shape[:2]
    if isinstance(data_range, dict):
        missing = [v for v in (var_names or ()) if v not in data_range]
        if var_names is None or missing:
            raise ValueError("ssim_loss: a data_range per variable needs var_names and a range for each of them (missing: %s)"
                             % (missing if var_names is not None else "var_names"))
        per = tuple(float(data_range[v]) for v in var_names)
    else:
        per = (float(data_range),) * C
    key = ("ssim_range", per, B, str(pred.device))
    t = _CW_CACHE.get(key)          # cached: no host-to-device copy inside a step
    if t is None:
        t = _CW_CACHE[key] = torch.tensor(per, dtype=torch.float32, device=pred.device).expand(B, C).contiguous()
    return t


def ssim_loss(pred, target, var_names: Optional[List[str]] = None, var_weights: Optional[Dict[str, float]] = None,
              aggregate_only: bool = False, lat_weights=None, data_range=SSIM_LOSS_TARGET_RANGE):
    """out[c] = cw_c * mean_b (1 - SSIM(pred[b, c], target[b, c])), out[C] = mean_c out[c]: [C + 1] as mse returns it,
    differentiable in pred.  The SSIM is metrics.functional.ssim's (7 x 7 uniform window, scikit-image's defaults; with
    `lat_weights` the mean over the centres weighted by the centre row's weight).  `data_range`: a number, a dict per variable,
    or "target" = every image's own target range, a constant of the gradient.  A variable in CONSTANTS or of weight 0 has
    coefficient 0: it contributes exactly 0 to the value and its gradient is exactly 0, whatever its SSIM (a constant target
    with range 0 scores 0 / 0)."""
    from ..data.processing.era5_constants import CONSTANTS
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    if pred.dim() != 4:
        raise ValueError("ssim_loss takes a prediction [B,C,H,W], got %s" % (tuple(pred.shape),))
    C = pred.shape[1]
    if var_names is not None:
        assert len(var_names) == C, "Number of variable names must match channel dimension"
        w = tuple(0.0 if v in CONSTANTS else float((var_weights or {}).get(v, 1.0)) for v in var_names)
    else:
        w = (1.0,) * C
    key = (w, str(pred.device))
    cw = _CW_CACHE.get(key)
    if cw is None:
        cw = _CW_CACHE[key] = torch.tensor(w, dtype=torch.float32, device=pred.device)
    s = _ops.SSIMFn.apply(pred, target.float(), _lat(lat_weights, pred), _ssim_loss_range(data_range, var_names, pred))
    per = torch.where(cw != 0, cw * (1.0 - s).mean(0), torch.zeros_like(cw))     # a select: 0 x NaN would be NaN
    out = torch.cat((per, per.mean().reshape(1)))
    return out[-1] if aggregate_only else out


# ---- missing data: losses and metrics over the VALID pixels only (csrc/loss.hip) ------------------------------
# valid = the target is finite there, and the mask (if one is given) is non-zero.  The reference has no such loss
# (examples/era5_daymet_downscaling.py names `masked_mse` but its metrics package has none) and a `mask` argument on rmse /
# lat_rmse / acc only.
TARGET_FINITE = "target_finite"       # as a `mask`: the masked form of a metric with no mask operand (metrics.Masked*)


def _mask_operand(mask, pred, target):
    """`mask` -> (uint8 bytes, row pitch, batch stride, channel stride) as the masked kernels address it, or (None, 0, 0, 0).
    mask: bool, integer or float (non-zero = keep) of shape [H,W], [1,1,H,W], [B,1,H,W] or [B,C,H,W], its spatial size the
    prediction's or the target's (then read through its top-left crop, as the target is).  A stride of 0 broadcasts: the mask is
    never expanded to [B,C,H,W].  A bool or uint8 mask is used in place; any other dtype costs one `!= 0` of the mask's own size
    (once, for a static mask: metrics.Masked*.set_mask)."""
    from ..models.hub.interpolation import Resampled
    if isinstance(pred, Resampled):
        raise TypeError("a Resampled prediction cannot be scored over a mask or a target with missing values: its fused scoring "
                        "pass has no mask -- materialize() it first")
    if mask is None or mask is TARGET_FINITE:
        return None, 0, 0, 0
    B, C, H, W = pred.shape
    ok_hw = ((H, W), tuple(target.shape[-2:]))
    shape = tuple(mask.shape)
    if len(shape) == 2 and shape in ok_hw:
        sb = sc = 0
    elif len(shape) == 4 and shape[2:] in ok_hw and shape[:2] in ((1, 1), (B, 1), (B, C)):
        plane = shape[2] * shape[3]
        sb = 0 if shape[0] == 1 else shape[1] * plane
        sc = 0 if shape[1] == 1 else plane
    else:
        raise ValueError("mask of shape %s: a mask is [H,W], [1,1,H,W], [B,1,H,W] or [B,C,H,W] with B, C = %d, %d and H, W = %s "
                         "(the prediction's) or %s (the target's)" % (shape, B, C, ok_hw[0], ok_hw[1]))
    m = mask.detach()
    if m.device != pred.device:
        m = m.to(pred.device)
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype != torch.uint8:
        m = (m != 0).view(torch.uint8)
    return m.contiguous(), shape[-1], sb, sc


def _fused_masked(pred, target, var_names, var_weights, aggregate_only, lat_weights, mask, kind):
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    m, pitch, sb, sc = _mask_operand(mask, pred, target)
    out = _ops.MaskedLossFn.apply(pred, target.float(), _lat(lat_weights, pred), _chan_weights(pred, var_names, var_weights),
                                  kind, m, pitch, sb, sc)
    return out[-1] if aggregate_only else out


def masked_mse(pred, target, var_names: Optional[List[str]] = None, var_weights: Optional[Dict[str, float]] = None,
               aggregate_only: bool = False, lat_weights=None, mask=None):
    """mse over the valid pixels: per channel sum(v w_lat w_var (pred - target)^2) / sum(v), 0 for a channel without data; the
    aggregate is the sum of the numerators over the sum of the counts (0 if nothing is valid).  Latitude weights are not
    renormalised over the valid set.  With everything valid this is mse.  The gradient is exactly 0 at an invalid pixel, where
    pred and target may hold NaN or Inf."""
    return _fused_masked(pred, target, var_names, var_weights, aggregate_only, lat_weights, mask, 0)


def masked_bayesian_tv(pred, target, var_names: Optional[List[str]] = None, var_weights: Optional[Dict[str, float]] = None,
                       aggregate_only: bool = False, lat_weights=None, mask=None):
    """bayesian_tv over the valid pixels: masked_mse plus the total-variation prior stored at every valid pixel, a difference
    term of which counts only if its neighbour is valid too.  With the valid region one top-left rectangle this is bayesian_tv
    of the cropped fields."""
    return _fused_masked(pred, target, var_names, var_weights, aggregate_only, lat_weights, mask, 1)


def _masked_sums(pred, target, lat_weights=None, mask=None):
    """[B,C,13] float64: the twelve sums of _moments over the valid pixels, then their number"""
    from .. import _hip
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    m, pitch, sb, sc = _mask_operand(mask, pred, target)
    return _hip.masked_moments(pred.detach().float().contiguous(), target.detach().float().contiguous(),
                               _lat(lat_weights, pred), None, m, (pitch, sb, sc))


def _with_nan_aggregate(per_channel, aggregate_only):
    """a channel without data is NaN; the aggregate is the mean over the channels that have data"""
    agg = per_channel.nanmean()
    return agg if aggregate_only else torch.cat((per_channel, agg.unsqueeze(0)))


def _masked_rmse(pred, target, aggregate_only=False, lat_weights=None, mask=None):
    """the reference's masked rmse (:243-255) with the validity as its mask: per (b, c)
    sqrt((sum_ij v w d^2 / (H W)) / (mean_{c,i,j} v[b] + 1e-9)), mean over b, then over c"""
    m = _masked_sums(pred, target, lat_weights, mask)
    n = pred.shape[2] * pred.shape[3]
    frac = m[..., 12].sum(1, keepdim=True) / (m.shape[1] * n) + 1e-9             # [B,1]
    return _with_aggregate((m[..., 5] / n / frac).sqrt().mean(0).float(), aggregate_only)


# ---- evaluation metrics (reference :236-324); one reduction kernel, the [B,C,6] -> [C+1] algebra on the host ----------
def _moments(pred, target, lat_weights=None, climatology=None):
    from .. import _hip
    from ..models.hub.interpolation import Resampled
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    clim = None
    if climatology is not None:
        clim = climatology.detach().to(device=pred.device, dtype=torch.float32)
        clim = clim.reshape(-1, *clim.shape[-2:])[:, : pred.shape[2], : pred.shape[3]].contiguous()
    if isinstance(pred, Resampled):             # an interpolation baseline: scored in the pass that resamples it, never stored
        return pred.moments(target.detach().float().contiguous(), _lat(lat_weights, pred), clim), \
            pred.shape[2] * pred.shape[3]
    return _hip.eval_moments(pred.detach().float().contiguous(), target.detach().float().contiguous(),
                             _lat(lat_weights, pred), clim), pred.shape[2] * pred.shape[3]


def _with_aggregate(per_channel, aggregate_only):
    agg = per_channel.mean()
    return agg if aggregate_only else torch.cat((per_channel, agg.unsqueeze(0)))


def _channel_sums(pred, target, lat_weights=None, mask=None):
    """(s, N, aggregate): s [C,>=12] float64, the sums over the batch; N the pixels of a channel they run over -- B H W, or with a
    `mask` the [C] counts of the valid ones; aggregate the rule that goes with it: without a mask a NaN channel makes the
    aggregate NaN, with one a channel without data is NaN and the aggregate is the mean of the others"""
    if mask is not None:
        s = _masked_sums(pred, target, lat_weights, mask).sum(0)
        return s, s[:, 12], _with_nan_aggregate
    m, n = _moments(pred, target, lat_weights)
    return m.sum(0), n * pred.shape[0], _with_aggregate


def rmse(pred, target, aggregate_only: bool = False, lat_weights=None, mask=None):
    """sqrt(mean_hw((pred-target)^2 * w_lat)) per (b, c), mean over b, then over c (reference :236-255).  With a `mask`
    (_mask_operand) the reference's masked form over the valid pixels -- mask non-zero and target finite: the squared error of
    an image is divided by the valid fraction of its batch entry + 1e-9 before the root."""
    if mask is not None:
        return _masked_rmse(pred, target, aggregate_only, lat_weights, mask)
    m, n = _moments(pred, target, lat_weights)
    return _with_aggregate((m[..., 5] / n).sqrt().mean(0).float(), aggregate_only)


def pearson(pred, target, aggregate_only: bool = False, mask=None):
    """cosine similarity of the mean-removed, channel-wise flattened [C, B*H*W] fields (reference :294-308).  With a `mask`:
    over the valid pixels of each channel (NaN for a channel without any; the aggregate is the mean of the others)."""
    s, N, aggregate = _channel_sums(pred, target, None, mask)
    cov = s[:, 4] - s[:, 0] * s[:, 1] / N
    vp = (s[:, 2] - s[:, 0] ** 2 / N).clamp_min(0).sqrt().clamp_min(1e-8)      # F.cosine_similarity's eps
    vt = (s[:, 3] - s[:, 1] ** 2 / N).clamp_min(0).sqrt().clamp_min(1e-8)
    return aggregate((cov / (vp * vt)).float(), aggregate_only)


def mean_bias(pred, target, aggregate_only: bool = False, mask=None):
    """mean(target) - mean(pred) per channel (reference :311-324).  With a `mask`: means over the valid pixels of each channel
    (NaN for a channel without any; the aggregate is the mean of the others)."""
    s, N, aggregate = _channel_sums(pred, target, None, mask)
    return aggregate(((s[:, 1] - s[:, 0]) / N).float(), aggregate_only)


def mae(pred, target, aggregate_only: bool = False, lat_weights=None, mask=None):
    """mean |pred - target| (x latitude weight) per channel and over everything (reference :219-232; with equal
    channel sizes the overall mean is the mean of the channel means).  With a `mask`: the mean over the valid pixels of each
    channel (NaN for a channel without any; the aggregate is the mean of the others)."""
    s, N, aggregate = _channel_sums(pred, target, lat_weights, mask)
    return aggregate((s[:, 6] / N).float(), aggregate_only)


def acc(pred, target, climatology, aggregate_only: bool = False, lat_weights=None, mask=None):
    """anomaly correlation (reference :259-291): anomalies w.r.t. the climatology, each channel centred by its
    unweighted mean over (B,H,W), latitude-weighted covariance / sqrt(variances).  The reference's `mask` argument has
    no effect there (its masked sums are overwritten by the unmasked ones, :282-284) and is ignored here; without
    latitude weights the reference raises (None * tensor) -- unit weights are used instead."""
    m, n = _moments(pred, target, lat_weights, climatology)
    s = m.sum(0)                                        # [C,12] over the batch
    N = n * pred.shape[0]
    ma, mb = s[:, 0] / N, s[:, 1] / N
    if lat_weights is None:
        sw = torch.full_like(ma, float(N))
    else:
        sw = _lat(lat_weights, pred).double().sum() * pred.shape[3] * pred.shape[0]
    cov = s[:, 9] - ma * s[:, 8] - mb * s[:, 7] + ma * mb * sw
    va = s[:, 10] - 2 * ma * s[:, 7] + ma * ma * sw
    vb = s[:, 11] - 2 * mb * s[:, 8] + mb * mb * sw
    return _with_aggregate((cov / (va * vb).sqrt()).float(), aggregate_only)


def mse_skill(pred, target, baseline, aggregate_only: bool = False, lat_weights=None):
    """Mean-squared-error skill score of `pred` against a baseline prediction of the same target: per channel
    1 - MSE_c(pred) / MSE_c(baseline), and as the aggregate 1 - MSE(pred) / MSE(baseline) over all channels; 1 is a perfect
    prediction, 0 no better than the baseline, negative worse.  The mean squared errors are means over (b, h, w), latitude
    weighted if `lat_weights` is given.  This is the reference's msess (metrics/functional.py:205-215) with a baseline field in
    place of the climatology; the reference's body hands its arguments to mse in the wrong positions (the climatology lands
    in var_names), so its evident meaning is built, not its text.  `baseline` is a tensor or a Resampled (an interpolation
    baseline that is scored without being stored: models.hub.Interpolation.lazy); so is `pred`.
    Not in METRICS_REGISTRY: evaluate_func calls a registry metric as (pred, target), and this one has a third operand.
    A channel the baseline predicts exactly is 1 - x / 0: -inf, or NaN where the prediction is exact too."""
    num = _moments(pred, target, lat_weights)[0][..., 5].sum(0)         # [C] sums of w (pred - target)^2 over the batch
    # the same object is scored once: its skill is 0 exactly, not to the last bit of two atomic accumulations
    den = num if baseline is pred else _moments(baseline, target, lat_weights)[0][..., 5].sum(0)
    per_channel = (1.0 - num / den).float()
    agg = (1.0 - num.sum() / den.sum()).float()
    return agg if aggregate_only else torch.cat((per_channel, agg.unsqueeze(0)))


# ---- probabilistic scores of a Gaussian prediction (reference :340-386); `pred` is a torch.distributions.Normal, e.g.
# utils.mc_dropout.mc_dropout_statistics(...).as_normal().  One reduction kernel (orbit2_gaussian_scores: [B,C,4] double sums
# of w crps, w std^2, w (mean - target)^2 and the 1-sigma hits), the reference's reductions on the host. --------------------
def _gaussian_sums(pred, target, lat_weights=None):
    from .. import _hip
    if not isinstance(pred, torch.distributions.Normal):
        raise TypeError("the Gaussian scores take a torch.distributions.Normal prediction, got %s" % type(pred).__name__)
    mean = pred.loc.detach().float().contiguous()
    std = pred.scale.detach().float().contiguous()
    if target is None:
        target = mean                                   # gaussian_spread has no target: sums 0 and 2 are not used then
    return _hip.gaussian_scores(mean, std, target.detach().float().contiguous(), _lat(lat_weights, mean)), \
        mean.shape[2] * mean.shape[3]


def gaussian_crps(pred, target, aggregate_only: bool = False, lat_weights=None):
    """Continuous ranked probability score of N(pred.loc, pred.scale^2) against `target`: mean over (b, h, w) of
    crps (x latitude weight) per channel, and the mean over everything (reference :340-360).
    One decision: the reference's function cannot be called (`torch.zeros_like(pred)` on a Normal raises TypeError, :349) and
    its text has `- 1 / torch.pi` (:353) where the closed form of the Gaussian CRPS, the integral of (F(x) - 1{x >= y})^2, has
    `- 1 / sqrt(pi)`: crps = std (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)), z = (target - mean) / std.  The closed form is
    what is built here.  Where std == 0 the limit |target - mean| is taken (no NaN / Inf)."""
    s, n = _gaussian_sums(pred, target, lat_weights)
    return _with_aggregate((s[..., 0].sum(0) / (n * s.shape[0])).float(), aggregate_only)


def gaussian_spread(pred, aggregate_only: bool = False, lat_weights=None):
    """per channel mean_b sqrt(mean_hw(w std^2)); the aggregate entry is mean(w std^2) over everything -- a variance, not a
    standard deviation: the reference's reductions exactly (:363-375), odd as they are."""
    s, n = _gaussian_sums(pred, None, lat_weights)
    var = s[..., 1]
    agg = (var.sum() / (n * var.numel())).float()
    if aggregate_only:
        return agg
    return torch.cat(((var / n).sqrt().mean(0).float(), agg.unsqueeze(0)))


def gaussian_spread_skill_ratio(pred, target, aggregate_only: bool = False, lat_weights=None):
    """gaussian_spread / rmse of the mean, entry by entry (reference :378-386; the aggregate entry therefore divides a
    variance by an rmse, as there)."""
    s, n = _gaussian_sums(pred, target, lat_weights)
    var = s[..., 1]
    agg = (var.sum() / (n * var.numel())).float()
    spread = agg if aggregate_only else torch.cat(((var / n).sqrt().mean(0).float(), agg.unsqueeze(0)))
    error = _with_aggregate((s[..., 2] / n).sqrt().mean(0).float(), aggregate_only)
    return spread / error


def gaussian_coverage(pred, target):
    """fraction of points with |target - mean| <= std per channel, and over everything (68.3 % for a calibrated Gaussian);
    not in the reference: the fourth sum of the score kernel, reported by examples/visualize.py"""
    s, n = _gaussian_sums(pred, target)
    return _with_aggregate((s[..., 3].sum(0) / (n * s.shape[0])).float(), False)


# ---- all-member (non-Gaussian) scores of an ensemble; `pred` is a utils.mc_dropout.EnsembleMembers (e.g. from
# utils.mc_dropout_members) or an [N, B, C, H, W] fp32 device tensor.  One kernel (orbit2_ensemble_scores) reads every member
# once and sorts the N values of a pixel in registers; the reductions are those of the Gaussian scores above: per channel the
# mean over (b, h, w), then the aggregate.  No reference counterpart: the reference scores its ensembles through a Gaussian fit
# only. ------------------------------------------------------------------------------------------------------------------------
def _ensemble(pred):
    from ..utils.mc_dropout import EnsembleMembers
    if isinstance(pred, EnsembleMembers):
        pred = pred.members
    if not torch.is_tensor(pred) or pred.dim() != 5:
        raise TypeError("the all-member scores take an EnsembleMembers or an [N, B, C, H, W] fp32 device tensor, got %s"
                        % (type(pred).__name__ if not torch.is_tensor(pred) else "a tensor of shape %s" % (tuple(pred.shape),)))
    return pred.detach()


def _ensemble_sums(pred, target, lat_weights=None):
    from .. import _hip
    m = _ensemble(pred)
    s = _hip.ensemble_scores(m, target.detach().float().contiguous(), _lat(lat_weights, m[0]), sums=True)["sums"]
    return s, m.shape[0], m.shape[3] * m.shape[4]


def ensemble_crps(pred, target, aggregate_only: bool = False, lat_weights=None, fair: bool = False):
    """Continuous ranked probability score of the empirical distribution of the N members against `target`,
    mean_i |x_i - y| - sum_{i<j} |x_i - x_j| / N^2 (the integral of (F_ens(x) - 1{x >= y})^2), or with fair=True the fair form
    that divides the pair term by N (N - 1) (unbiased for an ensemble of finite size): per channel the mean over (b, h, w)
    (x latitude weight), and the mean over everything."""
    s, N, n = _ensemble_sums(pred, target, lat_weights)
    pairs = float(N * (N - 1)) if fair else float(N * N)
    return _with_aggregate(((s[..., 0] - s[..., 1] / pairs).sum(0) / (n * s.shape[0])).float(), aggregate_only)


def ensemble_spread_skill_ratio(pred, target, aggregate_only: bool = False, lat_weights=None):
    """sqrt(mean w var) / sqrt(mean w err^2) per channel, means over (b, h, w): var the unbiased variance of the members, err
    the error of the ensemble mean; the aggregate is formed the same way from the totals over all channels.  Both are a
    standard deviation over an rmse.  This has no reference counterpart, so it does NOT copy the variance-over-rmse aggregate
    of gaussian_spread_skill_ratio, which mirrors a reference function.  A channel every member of which equals the target (a
    constant output channel) has neither spread nor error: its entry is 0 / 0 = NaN, and it adds nothing to the totals."""
    s, N, n = _ensemble_sums(pred, target, lat_weights)
    var, err = s[..., 3].sum(0), s[..., 2].sum(0)
    per_channel = (var / err).sqrt().float()
    agg = (var.sum() / err.sum()).sqrt().float()
    return agg if aggregate_only else torch.cat((per_channel, agg.unsqueeze(0)))


def ensemble_crps_field(pred, target, fair: bool = False):
    """the per-pixel CRPS (empirical, or fair), fp32 [B, C, H, W], unweighted"""
    from .. import _hip
    return _hip.ensemble_scores(_ensemble(pred), target.detach().float().contiguous(), sums=False,
                                crps_field="fair" if fair else "empirical")["crps_field"]


def ensemble_rank_histogram(pred, target, seed: int = 0):
    """int64 [C + 1, N + 1]: per channel the counts of the rank of the target among the N members over (b, h, w), the last row
    their sum over the channels.  A calibrated ensemble gives a flat histogram.  Ties (constant output channels equal the
    target in every member) are broken uniformly by a hash of (`seed`, pixel): the same seed gives the same counts, bit for
    bit."""
    from .. import _hip
    h = _hip.ensemble_scores(_ensemble(pred), target.detach().float().contiguous(), sums=False, hist=True, seed=seed)["hist"]
    h = h.sum(0)
    return torch.cat((h, h.sum(0, keepdim=True)))


def ensemble_quantiles(pred, q):
    """fp32 [Q, B, C, H, W]: the quantiles of the members at the levels `q` (a number, a sequence or a tensor, in [0, 1]) as
    torch.quantile / numpy define them ("linear"); q = 0 and q = 1 are the minimum and the maximum bit for bit"""
    from .. import _hip
    m = _ensemble(pred)
    return _hip.ensemble_scores(m, m[0], sums=False, quantiles=q)["quantiles"]


# ---- image-quality scores of a downscaled field (reference utils/visualize.py:366-372, through scikit-image there): SSIM and
# PSNR per (b, c) image from one windowed kernel (orbit2_ssim: [B,C,6] double sums of S, w S, the squared error, the target's
# min and max and the data range used), the means on the host.  `data_range`: None = max - min of every image's own target, as
# the reference passes it; a number or a tensor that broadcasts to [B,C] otherwise. ------------------------------------------------
def _ssim_sums(pred, target, lat_weights=None, data_range=None):
    from .. import _hip
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    pred = pred.detach().float().contiguous()
    return _hip.ssim_sums(pred, target.detach().float().contiguous(), _lat(lat_weights, pred), data_range), pred


def _ssim_per_image(s, pred, lat_weights=None):
    """[B,C] SSIM from the sums: the mean of S over the valid centres, weighted by the centre row's latitude weight if given"""
    hv, wv = pred.shape[2] - 6, pred.shape[3] - 6
    if lat_weights is None:
        return s[..., 0] / (hv * wv)
    return s[..., 1] / (wv * _lat(lat_weights, pred)[3:3 + hv].double().sum())


def _psnr_per_image(s, pred):
    """[B,C] PSNR in dB from the sums, in double on the host"""
    s = s.cpu()
    mse = s[..., 2] / (pred.shape[2] * pred.shape[3])
    return torch.where(mse == 0, torch.full_like(mse, float("inf")),
                       10.0 * torch.log10(s[..., 5] ** 2 / mse.clamp_min(torch.finfo(torch.float64).tiny)))


def ssim(pred, target, aggregate_only: bool = False, lat_weights=None, data_range=None):
    """Structural similarity with scikit-image's defaults (7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance): per
    (b, c) image the mean of S over the centres whose window lies inside it -- with latitude weights the mean weighted by the
    centre row's weight, normalised over those rows -- then the mean over b, then over c.  A wholly constant target image with
    data_range=None has range 0 and scores NaN, as scikit-image's would."""
    s, pred = _ssim_sums(pred, target, lat_weights, data_range)
    return _with_aggregate(_ssim_per_image(s, pred, lat_weights).mean(0).float(), aggregate_only)


def psnr(pred, target, aggregate_only: bool = False, data_range=None):
    """Peak signal-to-noise ratio in dB, 10 log10(range^2 / mse) per (b, c) image (inf at mse == 0), in double on the host from
    the kernel's sums; the mean over b, then over c."""
    s, pred = _ssim_sums(pred, target, None, data_range)
    return _with_aggregate(_psnr_per_image(s, pred).mean(0).float().to(pred.device), aggregate_only)


# ---- extreme-value scores: what a downscaled field does in its tails.  Exact quantiles of a field over its valid
# pixels from a radix select (orbit2_masked_loss_fwd at ORBIT2_MASKED_QUANTILES: no sort, no host copy, no size limit below 2^31
# pixels per group), and the error and the exceedance counts beyond a threshold from one pass for up to eight thresholds
# (ORBIT2_MASKED_TAIL).  The levels of the reference's quantile loss (metrics/functional.py:45) at +1, +2, +3 sigma; its extreme
# subsets are cut at the 5th / 95th percentile (data/processing/era5_extreme.py:84-88).  A pixel counts where the target is
# finite and the `mask` (as rmse's, _mask_operand) is non-zero.  Nothing here copies to the host. --------------------------------
SIGMA_LEVELS = (0.8413, 0.9772, 0.9987)


def _level_tensor(q, device):
    """levels as the fp32 device vector the kernels read; (vector, whether `q` was a single number)"""
    if torch.is_tensor(q):
        t = q.detach().to(device=device, dtype=torch.float32).reshape(-1)
        return t.contiguous(), q.dim() == 0
    single = not isinstance(q, (tuple, list))
    return torch.tensor([float(q)] if single else [float(v) for v in q], dtype=torch.float32, device=device), single


def _extreme_pair(pred, target):
    if isinstance(pred, torch.distributions.Normal):
        pred = pred.loc
    return pred.detach().float().contiguous(), target.detach().float().contiguous()


def _quantiles(pred, target, q, mask=None, per_image=False):
    """(out [2,G,Q,3], cnt [G]) of _hip.masked_quantiles for levels given as numbers or a tensor"""
    from .. import _hip
    pred, target = _extreme_pair(pred, target)
    m, pitch, sb, sc = _mask_operand(mask, pred, target)
    return _hip.masked_quantiles(pred, target, _level_tensor(q, pred.device)[0], m, (pitch, sb, sc), per_image)


def field_quantiles(x, q, mask=None, per_image=False):
    """[G, Q]: the linear-interpolation quantiles (numpy's default) of x [B,C,H,W] at the levels q over its finite, unmasked
    pixels; G = C groups, a channel pooled over the batch and all pixels, or per_image G = B * C.  Exact: the two order
    statistics around every level are found by selection, the interpolation is done in double.  NaN for a group without data."""
    return _quantiles(x, x, q, mask, per_image)[0][0, :, :, 0]


def quantile_bias(pred, target, q, aggregate_only: bool = False, mask=None):
    """[C+1, Q]: quantile of the prediction minus quantile of the target at every level of q (the Q-Q bias), per channel pooled
    over the batch, both over the pixels where the target is valid; the last row is the mean over the channels"""
    out = _quantiles(pred, target, q, mask)[0][..., 0]
    per = out[1] - out[0]
    agg = per.mean(0, keepdim=True)
    return agg[0] if aggregate_only else torch.cat((per, agg))


def _tail(pred, target, q, lower, lat_weights, mask, thresholds):
    """(sums [C,T,4] float64, cnt [C,T,4] int64) over the batch: the tail of every channel beyond its own pooled target quantile
    at the levels q (lower: the level 1 - q is NOT taken -- q is the level itself), or beyond explicit `thresholds` [C] / [C,T]"""
    from .. import _hip
    pred, target = _extreme_pair(pred, target)
    m, pitch, sb, sc = _mask_operand(mask, pred, target)
    if thresholds is None:
        levels, _ = _level_tensor(q, pred.device)
        out, _ = _hip.masked_quantiles(pred, target, levels, m, (pitch, sb, sc))      # field 0: the target through the pred's crop
        thr = out[0, :, :, 0].contiguous()                       # the quantile itself, still on the device
    else:
        thr = torch.as_tensor(thresholds).detach().to(device=pred.device, dtype=torch.float32)
        thr = thr.reshape(pred.shape[1], -1).contiguous()
    s, n = _hip.masked_tail(pred, target, thr, _lat(lat_weights, pred), m, (pitch, sb, sc), lower)
    return s.double().sum(0), n.sum(0)


def _tail_score(per_channel, aggregate_only):
    """[C] (one threshold per channel) -> [C+1] with the mean of the channels, or that mean alone"""
    per_channel = per_channel[:, 0].float()
    return _with_aggregate(per_channel, aggregate_only)


def tail_rmse(pred, target, q=0.9772, lower: bool = False, aggregate_only: bool = False, lat_weights=None, mask=None,
              thresholds=None):
    """[C+1]: sqrt(sum_b sum w d^2 / sum_b sum w) per channel over the valid pixels whose TARGET is at or beyond the channel's own
    pooled target quantile at level q (lower: at or below it), d = pred - target; the last entry is the mean of the channels.
    `thresholds` [C] replaces the quantile (e.g. a climatological percentile).  An empty tail gives NaN."""
    s, _ = _tail(pred, target, q, lower, lat_weights, mask, thresholds)
    return _tail_score((s[..., 1] / s[..., 0]).sqrt(), aggregate_only)


def tail_mae(pred, target, q=0.9772, lower: bool = False, aggregate_only: bool = False, lat_weights=None, mask=None,
             thresholds=None):
    """[C+1]: sum w |d| / sum w over the tail of tail_rmse"""
    s, _ = _tail(pred, target, q, lower, lat_weights, mask, thresholds)
    return _tail_score(s[..., 2] / s[..., 0], aggregate_only)


def tail_bias(pred, target, q=0.9772, lower: bool = False, aggregate_only: bool = False, mask=None, thresholds=None):
    """[C+1]: mean of pred - target over the pixels of the tail of tail_rmse (unweighted: sum d / their number)"""
    s, n = _tail(pred, target, q, lower, None, mask, thresholds)
    return _tail_score(s[..., 3] / n[..., 0].double(), aggregate_only)


def exceedance_scores(pred, target, q=0.9772, lower: bool = False, mask=None, thresholds=None):
    """{"csi", "pod", "far", "frequency_bias"}, each [C]: the contingency scores of the event "the value is at or beyond the
    channel's pooled target quantile at level q" (or `thresholds` [C]) over the valid pixels and the batch.  With hits h, misses m
    and false alarms f: csi = h / (h + m + f), pod = h / (h + m), far = f / (h + f), frequency_bias = (h + f) / (h + m).
    0 / 0 is NaN."""
    _, n = _tail(pred, target, q, lower, None, mask, thresholds)
    n = n[:, 0].double()
    h, f = n[:, 1], n[:, 2]
    ms = n[:, 0] - h
    return {"csi": (h / (h + ms + f)).float(), "pod": (h / (h + ms)).float(), "far": (f / (h + f)).float(),
            "frequency_bias": ((h + f) / (h + ms)).float()}


# ---- neighbourhood verification: the fractions skill score of Roberts & Lean (2008).  An event placed a few pixels
# aside is a miss and a false alarm to csi, and a field without the event is neither; the FSS compares the FRACTION of a window
# in which the event occurs, so it answers at which scale a field places its events rightly.  The event is "at or beyond the
# channel's pooled target quantile" (or explicit thresholds), the window counts come from orbit2_masked_loss_fwd at
# ORBIT2_FSS_KIND as exact integers, at a cost that does not grow with the window.  Nothing here copies to the host. --------------
def _fss_thresholds(pred, target, q, m, strides, thresholds):
    """[C, T] fp32 on the device: the pooled target quantiles at the levels q, exactly as _tail obtains them, or `thresholds`"""
    from .. import _hip
    if thresholds is None:
        out, _ = _hip.masked_quantiles(pred, target, _level_tensor(q, pred.device)[0], m, strides)
        return out[0, :, :, 0].contiguous()
    thr = torch.as_tensor(thresholds).detach().to(device=pred.device, dtype=torch.float32)
    return thr.reshape(pred.shape[1], -1).contiguous()


def _fss_ratio(n):
    """[..., 4] integer sums -> 1 - sum (cO - cM)^2 / (sum cO^2 + sum cM^2) in double; 0 / 0 is NaN"""
    n = n.double()
    return 1.0 - n[..., 3] / (n[..., 1] + n[..., 2])


def fss(pred, target, window: int = 9, q=0.9772, lower: bool = False, aggregate_only: bool = False, mask=None, thresholds=None):
    """[C+1]: the fractions skill score of the event "at or beyond the channel's own pooled target quantile at level q" (lower:
    at or below; `thresholds` [C] replaces the quantile) in windows of `window` x `window` pixels (odd, 1 .. 255; zero beyond
    the field and at invalid pixels), per channel from the integer sums over the batch and the valid centres:
    1 - sum (cO - cM)^2 / (sum cO^2 + sum cM^2); the last entry is the mean of the channels.  1 is a perfect placement at that
    scale, 0 no overlap at all; no event in either field gives NaN."""
    from .. import _hip
    pred, target = _extreme_pair(pred, target)
    m, pitch, sb, sc = _mask_operand(mask, pred, target)
    thr = _fss_thresholds(pred, target, q, m, (pitch, sb, sc), thresholds)
    _, n = _hip.masked_fss(pred, target, thr, int(window), m, (pitch, sb, sc), lower)
    return _with_aggregate(_fss_ratio(n.sum(0))[:, 0].float(), aggregate_only)


def fss_profile(pred, target, windows, q=SIGMA_LEVELS, lower: bool = False, mask=None, thresholds=None):
    """The score across scales, one kernel call per window of `windows` (S of them, each odd in 1 .. 255) for all levels of q
    (Q <= 8; or `thresholds` [C, Q]): {"fss": [C, Q, S]; "base_rate": [C, Q], f0 = the fraction of the valid pixels at which the
    target has the event; "uniform": [C, Q] = 0.5 + f0 / 2, the score above which a field counts as skilful at a scale;
    "skilful_window": [C, Q] int64, the smallest of `windows` with fss >= uniform, 0 if none}."""
    from .. import _hip
    pred, target = _extreme_pair(pred, target)
    m, pitch, sb, sc = _mask_operand(mask, pred, target)
    thr = _fss_thresholds(pred, target, q, m, (pitch, sb, sc), thresholds)
    windows = [int(w) for w in windows]
    # at window 1 cO is the indicator itself, so sum cO^2 counts the target's events
    n1 = _hip.masked_fss(pred, target, thr, 1, m, (pitch, sb, sc), lower)[1].sum(0).double()
    base = n1[..., 1] / n1[..., 0]
    uniform = 0.5 + 0.5 * base
    score = torch.stack([_fss_ratio(n1 if w == 1 else _hip.masked_fss(pred, target, thr, w, m, (pitch, sb, sc), lower)[1].sum(0))
                         for w in windows], dim=-1)
    sizes = torch.tensor(windows, dtype=torch.int64, device=score.device)
    big = torch.iinfo(torch.int64).max
    first = torch.where(score >= uniform.unsqueeze(-1), sizes, torch.full_like(sizes, big)).amin(-1)
    return {"fss": score.float(), "base_rate": base.float(), "uniform": uniform.float(),
            "skilful_window": torch.where(first == big, torch.zeros_like(first), first)}
