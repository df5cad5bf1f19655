"""Interpolation baselines of the downscaling task (reference: models/hub/interpolation.py, `Interpolation(size, mode)` =
F.interpolate(x, size, mode=mode)) on the fused resample kernels (include/orbit2_hip.h: orbit2_resample_fwd /
orbit2_resample_moments).

Beyond the reference's module: the output channels can be picked from the inputs by name or by index (a downscaling data module
has more input than output variables), a per-channel affine moves the field from the inputs' normalisation to the outputs', and
`lazy()` returns a `Resampled` descriptor that metrics.functional scores without the field ever being stored."""
from dataclasses import dataclass, replace
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn

from ... import _hip
from .utils import register

MODES = tuple(_hip.RESAMPLE_MODES)


def _vec(v, n, device, what):
    """a per-output-channel vector as fp32 [n] on `device`"""
    t = torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1).to(device)
    if t.numel() == 1 and n != 1:
        t = t.expand(n)
    if t.numel() != n:
        raise ValueError("%s has %d entries, the field %d output channels" % (what, t.numel(), n))
    return t.contiguous()


@dataclass(frozen=True)
class Resampled:
    """A resampled field that has not been computed: scale[c] * interpolate(x[:, channels[c]], size, mode) + shift[c].
    `materialize()` computes it; metrics.functional's rmse / mae / pearson / mean_bias / acc and mse_skill take it as it is and
    score it in the pass that resamples it."""
    x: torch.Tensor
    size: Tuple[int, int]
    mode: str = "bilinear"
    channels: Optional[Tuple[int, ...]] = None
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    antialias: bool = False

    @property
    def shape(self):
        C = self.x.shape[1] if self.channels is None else len(self.channels)
        return torch.Size((self.x.shape[0], C, int(self.size[0]), int(self.size[1])))

    @property
    def device(self):
        return self.x.device

    def materialize(self, out=None):
        return _hip.resample(self.x, self.size, self.mode, self.channels, self.scale, self.shift, out=out,
                             antialias=self.antialias)

    def moments(self, target, lat_w=None, clim=None):
        """[B,C,12] float64 sums of _hip.eval_moments(self.materialize(), target, lat_w, clim), without the field"""
        return _hip.resample_moments(self.x, self.size, self.mode, target, self.channels, self.scale, self.shift, lat_w, clim,
                                     antialias=self.antialias)

    def affine(self, std, mean):
        """this field times std[c] plus mean[c] (a Denormalize), folded into scale and shift: still one pass, nothing stored"""
        C = self.shape[1]
        std, mean = _vec(std, C, self.device, "std"), _vec(mean, C, self.device, "mean")
        if self.scale is None:
            return replace(self, scale=std, shift=mean)
        return replace(self, scale=self.scale.to(self.device) * std, shift=self.shift.to(self.device) * std + mean)


@register("interpolation")
class Interpolation(nn.Module):
    """size: the output (H, W); or superres_mag: the output is the input's size times it (what tiled_predict and
    trainer.evaluate_func expect of a model).  Exactly one of the two.  mode: nearest, bilinear or bicubic, as F.interpolate
    defines them at align_corners=False; antialias: its antialias=True (bilinear and bicubic only: the filter widens with a
    downsampling ratio).  channels: the input channel of every output channel; scale, shift: per output channel, both or
    neither.  No parameters, no autograd."""

    def __init__(self, size=None, mode: str = "bilinear", superres_mag: Optional[int] = None,
                 channels: Optional[Sequence[int]] = None, scale=None, shift=None, antialias: bool = False):
        super().__init__()
        if (size is None) == (superres_mag is None):
            raise ValueError("Interpolation takes exactly one of size and superres_mag")
        if mode not in MODES:
            raise ValueError("Interpolation mode is one of %s, got %r" % (", ".join(MODES), mode))
        if antialias and mode == "nearest":
            raise ValueError("Interpolation: antialias goes with bilinear or bicubic, nearest has no antialiased form")
        if (scale is None) != (shift is None):
            raise ValueError("Interpolation takes scale and shift together or not at all")
        if superres_mag is not None and (int(superres_mag) != superres_mag or superres_mag < 1):
            raise ValueError("superres_mag is a positive integer, got %r" % (superres_mag,))
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.mode = mode
        self.antialias = bool(antialias)
        self.superres_mag = None if superres_mag is None else int(superres_mag)
        self.channels = None if channels is None else tuple(int(c) for c in channels)
        self.scale = None if scale is None else torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
        self.shift = None if shift is None else torch.as_tensor(shift, dtype=torch.float32).reshape(-1)

    def _channels(self, in_variables, out_variables):
        if self.channels is not None or in_variables is None or out_variables is None:
            return self.channels
        in_variables = list(in_variables)
        if any(v not in in_variables for v in out_variables):
            raise RuntimeError("Interpolation requires the output variables to match the input variables.")
        return tuple(in_variables.index(v) for v in out_variables)

    def lazy(self, x, in_variables=None, out_variables=None) -> Resampled:
        if x.requires_grad:
            raise RuntimeError("Interpolation has no autograd: the input requires_grad")
        size = self.size if self.size is not None else (x.shape[2] * self.superres_mag, x.shape[3] * self.superres_mag)
        x = x.detach().float().contiguous()
        scale = None if self.scale is None else self.scale.to(x.device)
        shift = None if self.shift is None else self.shift.to(x.device)
        return Resampled(x, size, self.mode, self._channels(in_variables, out_variables), scale, shift, self.antialias)

    def forward(self, x, in_variables=None, out_variables=None):
        return self.lazy(x, in_variables, out_variables).materialize()

    def extra_repr(self):
        return "size=%s, mode=%s, superres_mag=%s, channels=%s, affine=%s, antialias=%s" % (
            self.size, self.mode, self.superres_mag, self.channels, self.scale is not None, self.antialias)
