"""Callable loss objects (reference: metrics/metrics.py).  Training-path losses only: mse, bayesian_tv, perceptual and the
*intended* lat_mse (the reference's LatWeightedMSE passes its arguments positionally into
the wrong slots and rejects the var_names/var_weights kwargs training_step always passes; here it computes
mse(pred, target, var_names, var_weights, aggregate_only, lat_weights[:H_pred]))."""
from typing import Dict, List, Optional

import numpy as np
import torch

from . import functional as _F
from .functional import acc, bayesian_tv, image_gradient, mae, mean_bias, mse, pearson, psnr, rmse, ssim
from .utils import MetricsMetaInfo, register


class Metric:
    def __init__(self, aggregate_only: bool = False, metainfo: Optional[MetricsMetaInfo] = None):
        self.aggregate_only = aggregate_only
        self.metainfo = metainfo

    def __call__(self, pred, target):
        raise NotImplementedError()


class LatitudeWeightedMetric(Metric):
    def __init__(self, aggregate_only: bool = False, metainfo: Optional[MetricsMetaInfo] = None):
        super().__init__(aggregate_only, metainfo)
        w = np.cos(np.deg2rad(np.asarray(self.metainfo.lat, dtype=np.float64)))
        self.lat_weights = torch.from_numpy(w / w.mean()).float().view(1, 1, -1, 1)

    def cast_to_device(self, pred):
        self.lat_weights = self.lat_weights.to(device=pred.device)


@register("mse")
class MSE(Metric):
    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        return mse(pred, target, var_names, var_weights, self.aggregate_only)


@register("bayesian_tv")
class Bayesian_TV(Metric):
    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        return bayesian_tv(pred, target, var_names, var_weights, self.aggregate_only)


class _WithConsistency:
    """base loss + weight x functional.consistency_mse(pred, source): the prediction, coarsened with antialiasing, is held to the
    field the model was given.  Per channel and in aggregate, as the base loss returns them.
    set_source(x, in_variables) hands over a step's input (trainer.training_step does, for a loss with `takes_source`);
    set_rescale(scale, shift) the affine that moves the inputs' normalisation to the outputs', once (utils.loaders).  A constant
    output variable (CONSTANTS) has weight 0 in the term: clip_replace_constant overwrites it with the truth.  Every output
    variable must be among the inputs."""

    takes_source = True
    graph_capturable = True       # no host read and no host-to-device copy per step: the index and weights are cached device tensors
    weight = 1.0
    mode = "bilinear"
    _source = _in_variables = _rescale = None
    _base = None                  # the functional of the base loss

    def set_source(self, x, in_variables):
        self._source, self._in_variables = x, list(in_variables)
        return self

    def set_rescale(self, scale, shift):
        self._rescale = None if scale is None else (tuple(float(v) for v in scale), tuple(float(v) for v in shift))
        return self

    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        from ..data.processing.era5_constants import CONSTANTS
        if self._source is None:
            raise RuntimeError("%s: set_source(x, in_variables) must be called with the step's input before the loss"
                               % getattr(self, "name", type(self).__name__))
        names = list(var_names) if var_names is not None else list(self.metainfo.out_vars)
        if any(v not in self._in_variables for v in names):
            raise RuntimeError("consistency_scores requires the output variables to be among the input variables.")
        base = type(self)._base(pred, target, var_names, var_weights, False)
        weights = {v: (0.0 if v in CONSTANTS else float((var_weights or {}).get(v, 1.0))) for v in names}
        term = _F.consistency_mse(pred, self._source, names, weights, False, None, self.mode,
                                  [self._in_variables.index(v) for v in names], self._rescale)
        out = base + self.weight * term
        return out[-1] if self.aggregate_only else out


@register("mse_consistency")
class MSEConsistency(_WithConsistency, Metric):
    _base = staticmethod(mse)


@register("bayesian_tv_consistency")
class BayesianTVConsistency(_WithConsistency, Metric):
    _base = staticmethod(bayesian_tv)


class _WithSSIM:
    """base loss + weight x functional.ssim_loss(pred, target): the usual `mse + lambda (1 - SSIM)` objective of super-resolution
    (DESIGN 4.10h).  Per channel and in aggregate, as the base loss returns them.  `data_range`: a number, a dict per variable,
    or "target" (every image's own target range).  A constant output variable (CONSTANTS) or one of weight 0 has coefficient 0 in
    the term.  weight 0 is the base loss alone: the term is not computed."""

    graph_capturable = True       # no host read and no host-to-device copy per step: weights and ranges are cached device tensors
    weight = 1.0
    data_range = _F.SSIM_LOSS_TARGET_RANGE
    _base = None                  # the functional of the base loss; None: the term alone

    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        base = type(self)._base
        out = None if base is None else base(pred, target, var_names, var_weights, False)
        if out is None or self.weight != 0:
            term = self.weight * _F.ssim_loss(pred, target, var_names, var_weights, False, None, self.data_range)
            out = term if out is None else out + term
        return out[-1] if self.aggregate_only else out


@register("ssim_loss")
class SSIMLoss(_WithSSIM, Metric):
    """weight x (1 - SSIM), per variable and in aggregate"""


@register("mse_ssim")
class MSESSIM(_WithSSIM, Metric):
    _base = staticmethod(mse)


@register("bayesian_tv_ssim")
class BayesianTVSSIM(_WithSSIM, Metric):
    _base = staticmethod(bayesian_tv)


@register("imagegradient")
class IMAGEGRADIENT(Metric):
    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        return image_gradient(pred, target, var_names, var_weights)


@register("lat_mse")
class LatWeightedMSE(LatitudeWeightedMetric):
    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        self.cast_to_device(pred)
        return mse(pred, target, var_names, var_weights, self.aggregate_only, self.lat_weights)


@register("perceptual")
class PERCEPTUAL(Metric):
    """L1 + 0.5 * mean LPIPS-VGG16 (reference: metrics.py:119-187, functional.py:17-33).  Same constructor as the
    reference (device, model, aggregate_only, metainfo).  The reference's __call__ takes (pred, target) only, while
    training_step always passes var_names= / var_weights=: they are accepted and ignored here.
    LPIPS weights: a state dict file named by $ORBIT2_LPIPS_WEIGHTS (lpips / torchvision key names).  The reference
    loads lpips' PRETRAINED VGG16 (`lpips.LPIPS(net='vgg')`); training against anything else is a different loss, so a
    missing file is an error.  Seeded random stand-in weights (synthetic throughput runs, parity tests against the
    restated graph) must be asked for explicitly: `synthetic_weights=True` or ORBIT2_LPIPS_SYNTHETIC=1.
    Export the real ones on a machine that has the packages:
        import lpips, torch; torch.save(lpips.LPIPS(net='vgg').state_dict(), 'lpips_vgg.pt')"""

    graph_capturable = True       # the backward keeps the upstream scalar on the device (lpips_hip._PerceptualFn.backward)

    def __init__(self, device, model, aggregate_only: bool = False, metainfo: Optional[MetricsMetaInfo] = None,
                 synthetic_weights: Optional[bool] = None):
        import os
        from .lpips_hip import LPIPSVGG16
        super().__init__(aggregate_only, metainfo)
        self.model = model
        path = os.environ.get("ORBIT2_LPIPS_WEIGHTS")
        if synthetic_weights is None:
            synthetic_weights = os.environ.get("ORBIT2_LPIPS_SYNTHETIC", "0") == "1"
        state = None
        if path:
            state = torch.load(path, map_location="cpu", weights_only=True)
        elif not synthetic_weights:
            raise RuntimeError(
                "perceptual loss: no LPIPS-VGG16 weights.  Set $ORBIT2_LPIPS_WEIGHTS to a state-dict file exported from "
                "lpips.LPIPS(net='vgg') (or torchvision vgg16 + lpips lins); seeded random stand-in weights are only "
                "used when asked for explicitly (synthetic_weights=True / ORBIT2_LPIPS_SYNTHETIC=1): a run that "
                "optimises 0.5*LPIPS against a random network is not the reference's loss.")
        self.loss_fn = LPIPSVGG16(device, state)

    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        return self.loss_fn.perceptual(pred, target)


@register("perceptual_lat_mse")
class PerceptualLatMSE(PERCEPTUAL, LatitudeWeightedMetric):
    """BASELINE.json configs[4] names a "hybrid perceptual + lat-weighted MSE loss" (SURVEY 8d-5): the sum of the reference's
    `perceptual` (metrics.py:119-187: L1 + 0.5 * mean LPIPS-VGG16) and its intended `lat_mse` (metrics.py:295-316: the
    variable- and latitude-weighted MSE, aggregate over channels).  The reference has no object for the sum; this one takes
    the perceptual loss's constructor (device, model, ...) and training_step's keyword arguments."""

    def __init__(self, device, model, aggregate_only: bool = False, metainfo: Optional[MetricsMetaInfo] = None,
                 synthetic_weights: Optional[bool] = None):
        PERCEPTUAL.__init__(self, device, model, aggregate_only, metainfo, synthetic_weights)
        w = np.cos(np.deg2rad(np.asarray(self.metainfo.lat, dtype=np.float64)))
        self.lat_weights = torch.from_numpy(w / w.mean()).float().view(1, 1, -1, 1)

    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None):
        self.cast_to_device(pred)
        per = self.loss_fn.perceptual(pred, target)
        lat = mse(pred, target, var_names, var_weights, True, self.lat_weights)
        return per + lat


@register("rmse")
class RMSE(Metric):
    """reference metrics.py RMSE: unweighted root mean squared error (validation / test metric of the downscaling task)"""
    def __call__(self, pred, target, mask=None):
        return rmse(pred, target, self.aggregate_only, mask=mask)


@register("pearson")
class Pearson(Metric):
    def __call__(self, pred, target):
        return pearson(pred, target, self.aggregate_only)


@register("mean_bias")
class MeanBias(Metric):
    def __call__(self, pred, target):
        return mean_bias(pred, target, self.aggregate_only)


@register("lat_rmse")
class LatWeightedRMSE(LatitudeWeightedMetric):
    def __call__(self, pred, target, mask=None):
        self.cast_to_device(pred)
        return rmse(pred, target, self.aggregate_only, self.lat_weights, mask)


@register("mae")
class MAE(Metric):
    def __call__(self, pred, target):
        return mae(pred, target, self.aggregate_only)


@register("ssim")
class SSIM(Metric):
    """structural similarity of every (b, c) image, scikit-image's defaults, data range = max - min of the image's target (the
    score the reference prints for a stitched field, utils/visualize.py:366-372)"""
    def __call__(self, pred, target):
        return ssim(pred, target, self.aggregate_only)


@register("lat_ssim")
class LatWeightedSSIM(LatitudeWeightedMetric):
    def __call__(self, pred, target):
        self.cast_to_device(pred)
        return ssim(pred, target, self.aggregate_only, self.lat_weights)


@register("psnr")
class PSNR(Metric):
    def __call__(self, pred, target):
        return psnr(pred, target, self.aggregate_only)


# ---- extreme values (functional.tail_rmse / quantile_bias): called as (pred, target) like ssim / psnr, so
# evaluate_func runs them unchanged; the level is an attribute
class _AtLevel:
    """level: the quantile level of the score (default +2 sigma, functional.SIGMA_LEVELS[1]); set_level(q) changes it"""

    level = 0.9772

    def set_level(self, q):
        self.level = float(q)
        return self


@register("tail_rmse")
class TailRMSE(_AtLevel, Metric):
    """rmse over the pixels whose target is at or beyond the channel's own target quantile at `level`"""
    def __call__(self, pred, target):
        return _F.tail_rmse(pred, target, self.level, False, self.aggregate_only)


@register("lat_tail_rmse")
class LatWeightedTailRMSE(_AtLevel, LatitudeWeightedMetric):
    def __call__(self, pred, target):
        self.cast_to_device(pred)
        return _F.tail_rmse(pred, target, self.level, False, self.aggregate_only, self.lat_weights)


@register("quantile_bias")
class QuantileBias(_AtLevel, Metric):
    """quantile of the prediction minus quantile of the target at `level`, per channel and their mean"""
    def __call__(self, pred, target):
        out = _F.quantile_bias(pred, target, self.level, self.aggregate_only)
        return out[..., 0]


@register("fss")
class FSS(_AtLevel, Metric):
    """the fractions skill score of the event "at or beyond the channel's own target quantile at `level`" in windows of
    `window` x `window` pixels (odd, 1 .. 255; default 9); set_window(n) changes it"""

    window = 9

    def set_window(self, n):
        self.window = int(n)
        return self

    def __call__(self, pred, target):
        return _F.fss(pred, target, self.window, self.level, False, self.aggregate_only)


# ---- missing data (functional.masked_*): the same call signatures as their unmasked namesakes, so that
# training_step and evaluate_func run unchanged on targets that are NaN where there is no data (land-only Daymet / PRISM).
# A pixel counts where the target is finite AND the mask (if any) is non-zero; without any mask the finite test alone decides.
class _Masked:
    """set_mask(mask): a static mask (e.g. the high-resolution land_sea_mask) for every later call, converted and uploaded
    once; `mask=` on a call overrides it.  Shapes: [H,W], [1,1,H,W], [B,1,H,W], [B,C,H,W] (functional._mask_operand)."""

    graph_capturable = True       # the valid count stays on the device: forward and backward read it there

    _static_mask = None

    def set_mask(self, mask):
        if mask is not None:
            mask = torch.as_tensor(mask)
            mask = mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0
        self._static_mask = mask
        return self

    def _mask(self, mask, pred):
        if mask is not None:
            return mask
        m = self._static_mask
        device = pred.loc.device if isinstance(pred, torch.distributions.Normal) else pred.device
        if m is not None and m.device != device:
            m = self._static_mask = m.to(device)               # once: later calls find it there
        return _F.TARGET_FINITE if m is None else m            # no mask at all: still the masked form, over the finite targets


@register("masked_mse")
class MaskedMSE(_Masked, Metric):
    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None, mask=None):
        return _F.masked_mse(pred, target, var_names, var_weights, self.aggregate_only, None, self._mask(mask, pred))


@register("masked_lat_mse")
class MaskedLatWeightedMSE(_Masked, LatitudeWeightedMetric):
    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None, mask=None):
        self.cast_to_device(pred)
        return _F.masked_mse(pred, target, var_names, var_weights, self.aggregate_only, self.lat_weights,
                             self._mask(mask, pred))


@register("masked_bayesian_tv")
class MaskedBayesian_TV(_Masked, Metric):
    def __call__(self, pred, target, var_names: Optional[List[str]] = None,
                 var_weights: Optional[Dict[str, float]] = None, mask=None):
        return _F.masked_bayesian_tv(pred, target, var_names, var_weights, self.aggregate_only, None, self._mask(mask, pred))


@register("masked_rmse")
class MaskedRMSE(_Masked, Metric):
    def __call__(self, pred, target, mask=None):
        return _F._masked_rmse(pred, target, self.aggregate_only, None, self._mask(mask, pred))


@register("masked_lat_rmse")
class MaskedLatWeightedRMSE(_Masked, LatitudeWeightedMetric):
    """the reference's RMSE object passes its mask into the lat_weights slot (metrics.py:319-372); the evident meaning is built"""
    def __call__(self, pred, target, mask=None):
        self.cast_to_device(pred)
        return _F._masked_rmse(pred, target, self.aggregate_only, self.lat_weights, self._mask(mask, pred))


@register("masked_mae")
class MaskedMAE(_Masked, Metric):
    def __call__(self, pred, target, mask=None):
        return _F.mae(pred, target, self.aggregate_only, None, self._mask(mask, pred))


@register("masked_pearson")
class MaskedPearson(_Masked, Metric):
    def __call__(self, pred, target, mask=None):
        return _F.pearson(pred, target, self.aggregate_only, self._mask(mask, pred))


@register("masked_mean_bias")
class MaskedMeanBias(_Masked, Metric):
    def __call__(self, pred, target, mask=None):
        return _F.mean_bias(pred, target, self.aggregate_only, self._mask(mask, pred))


class ClimatologyBasedMetric(Metric):
    """metrics that subtract the split's climatology (reference metrics.py:78-97): metainfo.climatology is [C,H,W]"""

    def __init__(self, aggregate_only: bool = False, metainfo: Optional[MetricsMetaInfo] = None):
        Metric.__init__(self, aggregate_only, metainfo)
        self.climatology = self.metainfo.climatology.unsqueeze(0)


@register("acc")
class ACC(ClimatologyBasedMetric):
    def __call__(self, pred, target, mask=None):
        return acc(pred, target, self.climatology, self.aggregate_only, None, mask)


@register("lat_acc")
class LatWeightedACC(LatitudeWeightedMetric, ClimatologyBasedMetric):
    def __init__(self, aggregate_only: bool = False, metainfo: Optional[MetricsMetaInfo] = None):
        LatitudeWeightedMetric.__init__(self, aggregate_only, metainfo)
        ClimatologyBasedMetric.__init__(self, aggregate_only, metainfo)

    def __call__(self, pred, target, mask=None):
        self.cast_to_device(pred)
        return acc(pred, target, self.climatology, self.aggregate_only, self.lat_weights, mask)
