"""MC-dropout ensembles (reference: utils/mc_dropout.py:4-19 `enable_dropout`, `get_monte_carlo_predictions`).

The reference's helper walks `modules()` for nn.Dropout objects and puts them back into train mode after `eval()`.  Here
dropout is not a module but a probability handed to the fused kernels, so the mode is a flag on the modules that decide one
(`McDropoutMode`: Res_Slim_ViT, Block, Attention, Mlp); which sites it wakes is the reference's behaviour, DESIGN 4.10:
the element dropouts are on, DropPath stays off, attention-probability dropout follows the backend.  Any later `train()` /
`eval()` leaves the mode.  Seeds come from the package's stream (`climate_learn.manual_seed`), in the forward's own order, so
one seed reproduces a whole ensemble bit for bit while its members differ from each other.

`mc_dropout_statistics` is the form built for the card: the reference stacks N full-resolution predictions and reduces them
afterwards (N x 100 MB at [16, 3, 512, 1024]); here each member updates a running mean and sum of squared deviations in
place (`orbit2_ensemble_update`, one Welford step per member), so peak memory does not grow with N.

`mc_dropout_members` is the form for what only the members themselves can give -- order statistics: the all-member CRPS, the
rank histogram and quantile fields of metrics.functional (`ensemble_*`, one pass of `orbit2_ensemble_scores`).  It holds N
fields, in one stack allocated once.
"""
from __future__ import annotations

import torch

from .. import _hip
from ..models.hub.components.mlp import McDropoutMode


def enable_dropout(model_module):
    """Switch `model_module` (a Res_Slim_ViT, a stand-alone Block / Attention / Mlp, or any wrapper that holds one as a
    sub-module, e.g. HipDataParallel) to MC-dropout mode.  Call it after `eval()`, as the reference does; the next `train()`
    or `eval()` switches the mode off again."""
    sites = [m for m in model_module.modules() if isinstance(m, McDropoutMode)]
    if not sites:
        raise TypeError("enable_dropout: %s holds no module that decides a dropout probability (Res_Slim_ViT, Block, "
                        "Attention, Mlp)" % type(model_module).__name__)
    # the two configurations whose MC-mode forward is not covered by a test are refused by name rather than run unverified
    if any(getattr(m, "tensor_par_size", 1) > 1 for m in sites):
        raise RuntimeError("MC dropout is not built for tensor parallelism (tensor_par_size > 1)")
    if any(getattr(p, "_o2_sharded", False) for p in model_module.parameters()):
        raise RuntimeError("MC dropout is not built for the parameter-sharding engine (this model's parameters are 1/N chunks)")
    for m in sites:
        m.mc_dropout = True


def _member(batch, model_module, div, overlap):
    """one prediction of the batch, clipped as in training; div > 1: the stitched field of utils.visualize.tiled_predict"""
    from ..trainer import clip_replace_constant
    from .visualize import tiled_predict
    x, y, in_variables, out_variables = batch[:4]
    dev = next(model_module.parameters()).device
    x, y = x.to(dev, non_blocking=True), y.to(dev, non_blocking=True)
    if div > 1:
        return tiled_predict(model_module, x.float(), y, in_variables, out_variables, div, overlap)
    pred = model_module.forward(x, in_variables, out_variables)
    return clip_replace_constant(y, pred, out_variables).float().contiguous()


def get_monte_carlo_predictions(batch, model_module, n_ensemble_members):
    """[N, B, C, H, W] fp32 on the device: N forwards of `batch` = (x, y, in_variables, out_variables, ...) in MC-dropout mode
    (reference :10-19: eval(), enable_dropout(), torch.no_grad(), stack).  The prediction is clipped as `training_step` clips
    it (precipitation >= 0, constant output channels from `y`)."""
    model_module.eval()
    enable_dropout(model_module)
    ensemble_predictions = []
    for _ in range(int(n_ensemble_members)):
        with torch.no_grad():
            ensemble_predictions.append(_member(batch, model_module, 1, 0))
    return torch.stack(ensemble_predictions)


class EnsembleStatistics:
    """running moments of an ensemble: `mean`, `std` = sqrt(m2 / (n - 1)) (the unbiased estimate of
    torch.stack(members).std(0)), `n` members; `as_normal()` is what the Gaussian scores of metrics.functional take"""

    def __init__(self, mean, m2, n):
        self.mean, self.m2, self.n = mean, m2, int(n)

    @property
    def std(self):
        return (self.m2 / (self.n - 1)).clamp_min_(0.0).sqrt_()

    def as_normal(self):
        # validate_args=False: a spread of exactly 0 (constant output channels, copied from the target into every member) is a
        # normal case here and handled by the score kernel; Normal's own check would refuse scale == 0
        return torch.distributions.Normal(self.mean, self.std, validate_args=False)


def mc_dropout_statistics(batch, model_module, n_ensemble_members, *, div=1, overlap=0):
    """Mean and spread of an MC-dropout ensemble of `n_ensemble_members` predictions of `batch`, streamed: every member is
    folded into the running moments by one `orbit2_ensemble_update` and dropped.  div > 1: each member is the stitched field
    of `utils.visualize.tiled_predict(model, x, y, ..., div, overlap)`."""
    n = int(n_ensemble_members)
    if n < 2:
        raise ValueError("mc_dropout_statistics needs at least 2 ensemble members to estimate a spread, got %d" % n)
    model_module.eval()
    enable_dropout(model_module)
    mean = m2 = None
    with torch.no_grad():
        for k in range(1, n + 1):
            member = _member(batch, model_module, int(div), int(overlap))
            if mean is None:
                mean, m2 = torch.empty_like(member), torch.empty_like(member)
            _hip.ensemble_update(member, mean, m2, k)
            del member
    return EnsembleStatistics(mean, m2, n)


class EnsembleMembers:
    """the members of an ensemble themselves: `members` fp32 [N, B, C, H, W] on the device, `n` = N; what the all-member scores
    of metrics.functional (`ensemble_crps`, `ensemble_rank_histogram`, `ensemble_quantiles`, ...) take.  `statistics()` folds
    the stack into the running moments of `mc_dropout_statistics` (one `orbit2_ensemble_update` per member)."""

    def __init__(self, members):
        if not torch.is_tensor(members) or members.dim() != 5:
            raise TypeError("EnsembleMembers takes an [N, B, C, H, W] tensor")
        self.members, self.n = members, int(members.shape[0])

    def statistics(self):
        mean, m2 = torch.empty_like(self.members[0]), torch.empty_like(self.members[0])
        for k in range(self.n):
            _hip.ensemble_update(self.members[k], mean, m2, k + 1)
        return EnsembleStatistics(mean, m2, self.n)


def mc_dropout_members(batch, model_module, n_ensemble_members, *, div=1, overlap=0):
    """The `n_ensemble_members` MC-dropout predictions of `batch` themselves, as an `EnsembleMembers`.  THIS FORM HOLDS N
    FIELDS: order statistics (all-member CRPS, ranks, quantiles) need every member of a pixel at once, so that is inherent;
    `mc_dropout_statistics` remains the form whose memory does not grow with N.  The stack is allocated once and each member
    written into its slice (a torch.stack of a list would hold 2 N fields at its peak).  Mode handling, seeding order and
    clipping are those of `mc_dropout_statistics`: under one `climate_learn.manual_seed` the stack equals
    `get_monte_carlo_predictions` bit for bit (div = 1), or the stitched fields of `tiled_predict` (div > 1)."""
    n = int(n_ensemble_members)
    if not 2 <= n <= _hip.ENSEMBLE_MAX_MEMBERS:
        raise ValueError("mc_dropout_members serves 2 to %d ensemble members, got %d" % (_hip.ENSEMBLE_MAX_MEMBERS, n))
    model_module.eval()
    enable_dropout(model_module)
    stack = None
    with torch.no_grad():
        for k in range(n):
            member = _member(batch, model_module, int(div), int(overlap))
            if stack is None:
                stack = torch.empty((n,) + tuple(member.shape), dtype=torch.float32, device=member.device)
            stack[k].copy_(member)
            del member
    return EnsembleMembers(stack)
