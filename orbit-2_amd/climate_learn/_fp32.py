"""Forward-only fp32 pipeline of Res_Slim_ViT (`model.set_compute_dtype(torch.float32)`).

The reference's `trainer.data_type: float32` (examples/intermediate_downscaling.py:593-607) and its inference driver
(examples/visualize.py:251) run fp32 parameters, fp32 GEMMs and fp32 attention.  This module is that computation on
the HIP kernels `orbit2_gemm_f32`, `orbit2_attn_fwd_f32`, `orbit2_layernorm_fwd_f32` and the fp32 token entries of the
variable aggregation and `unpatchify`: every token tensor between the folded variable aggregation and `unpatchify` is
fp32, and the GEMMs read the fp32 master parameters as they are stored (no compute copy, `_ops.cw` is never called).

There is no backward: nothing is saved, no autograd node is built, dropout / DropPath are not implemented.  The bf16
autograd functions of `_ops.py` are not touched by this path.
"""
from __future__ import annotations

import math

import torch

from . import _hip
from ._ops import _Q_PRESCALE

F32 = torch.float32


def _w(p: torch.Tensor) -> torch.Tensor:
    """the fp32 master parameter itself"""
    t = p.detach()
    return t if t.is_contiguous() else t.contiguous()


def linear(x2d, W, b, **kw):
    """x2d [M, K] fp32 (rows contiguous, any pitch) x W [N, K]^T + b, fused epilogue of orbit2_gemm_f32"""
    M, K = x2d.shape
    N = W.shape[0]
    out = torch.empty(M, N, dtype=F32, device=x2d.device)
    return _hip.gemm_f32(x2d, _w(W), out, M, N, K, x2d.stride(0), K, N, bias=None if b is None else _w(b), **kw)


def refuse(model):
    """the cases the fp32 path does not serve, each named"""
    if model.training:
        raise RuntimeError("Res_Slim_ViT fp32 compute is forward-only inference: dropout / DropPath are not built in fp32 "
                           "(training mode is set; call model.eval())")
    if any(getattr(m, "mc_dropout", False) for m in model.modules()):
        raise RuntimeError("Res_Slim_ViT fp32 compute has no dropout kernels: MC dropout is built for the bf16 path "
                           "(enable_dropout() was called; model.eval() leaves the mode, or set_compute_dtype(torch.bfloat16))")
    if model.tensor_par_size > 1:
        raise RuntimeError("Res_Slim_ViT fp32 compute is not built for tensor parallelism (tensor_par_size > 1)")
    prm = list(model.parameters())
    if any(getattr(p, "_o2_sharded", False) for p in prm):
        raise RuntimeError("Res_Slim_ViT fp32 compute needs whole fp32 master parameters: this model is managed by the "
                           "parameter-sharding engine, which keeps 1/N chunks of them")
    if torch.is_grad_enabled() and any(p.requires_grad for p in prm):
        raise RuntimeError("Res_Slim_ViT fp32 compute is forward-only (no fp32 backward is built): call it under "
                           "torch.no_grad()")


def block(blk, x2d, B, L):
    """LN -> qkv GEMM (q third scaled) -> attention -> proj GEMM + residual -> LN -> fc1 GEMM + GELU -> fc2 GEMM + residual"""
    a, m = blk.attn, blk.mlp
    H = a.num_heads
    D = x2d.shape[1]
    d = D // H
    h1 = _hip.layernorm_fwd_f32(x2d, _w(blk.norm1.weight), _w(blk.norm1.bias))
    qkv = linear(h1, a.qkv.weight, a.qkv.bias, colscale=(D, _Q_PRESCALE / math.sqrt(d)))
    o, _ = _hip.attn_fwd_f32(qkv, B, L, H, d, flags=_hip.ATTN_Q_PRESCALED)
    x1 = linear(o.view(B * L, D), a.proj.weight, a.proj.bias, residual=x2d, ldr=D)
    h2 = _hip.layernorm_fwd_f32(x1, _w(blk.norm2.weight), _w(blk.norm2.bias))
    hm = linear(h2, m.fc1.weight, m.fc1.bias, act=1)
    return linear(hm, m.fc2.weight, m.fc2.bias, residual=x1, ldr=D)


@torch.no_grad()
def forward(model, x, in_variables, out_variables):
    """Res_Slim_ViT.forward in fp32 (reference res_slimvit.py:245-338); x: fp32 [B, V, h, w] on the device"""
    from . import _ops
    from .models.hub.components.mlp import HipLinear
    B, V, h, w = x.shape
    cidx = model._chan_idx(in_variables, out_variables, x.device)
    c0, c3 = model.path2[0], model.path2[3]
    r = _ops.Conv3x3Fn.apply(x, c0.weight, c0.bias, cidx, 1, model.superres_mag, None)
    r = _ops.Conv3x3Fn.apply(r, c3.weight, c3.bias, None, 0, 1, None)
    # front-end: folded patch-embed + variable aggregation (fp32 tables as in the bf16 path), tokens fp32
    stab, gtab = model._tables(model.get_var_ids(tuple(in_variables)))
    D = model.embed_dim
    L = (h // model.patch_size) * (w // model.patch_size)
    z = _hip.varagg_fwd_f32(x, stab.contiguous(), gtab.contiguous(), model.num_heads, D)
    posres = model._posres().contiguous()                                    # [L, D] fp32, added as it is
    t = linear(z, model.var_agg.proj.weight, model.var_agg.proj.bias, residual=posres, ldr=D, res_mod=L, res_first=True)
    for blk in model.blocks:
        t = block(blk, t, B, L)
    # head: final LN + decoder_depth x (Linear + GELU) + Linear
    t = _hip.layernorm_fwd_f32(t, _w(model.norm.weight), _w(model.norm.bias))
    lins = [m for m in model.head if isinstance(m, HipLinear)]
    for i, m in enumerate(lins):
        t = linear(t, m.weight, m.bias, act=0 if i == len(lins) - 1 else 1)
    img = _hip.unpatchify_fwd_f32(t, B, model.out_channels, model.img_size[0], model.img_size[1], model.patch_size,
                                  model.superres_mag)
    co = model.conv_out
    return _ops.Conv3x3Fn.apply(img, co.weight, co.bias, None, 0, 1, r)
