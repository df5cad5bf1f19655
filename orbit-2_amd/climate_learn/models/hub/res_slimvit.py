"""Res_Slim_ViT on MI355X (reference: models/hub/res_slimvit.py).

Same constructor, attributes, forward signature, `data_config` and `state_dict` keys as the reference; the
compute is the hand-written HIP path:

    residual branch : 3x3 conv (+GELU+PixelShuffle fused) -> 3x3 conv                     (csrc/image.hip)
    front-end       : folded patch-embed + variable aggregation -> proj GEMM whose epilogue adds
                      pos+resolution embedding and applies pos_drop                         (csrc/varagg.hip, gemm.hip)
    encoder         : depth x Block (one fused autograd node each)                        (gemm/attn/norm_elem.hip)
    head            : final LN + decoder_depth x (Linear+GELU) + Linear                    (one autograd node)
    tail            : unpatchify -> 3x3 conv with the residual branch added in its epilogue

`set_compute_dtype(torch.float32)` switches the built model to the forward-only fp32 pipeline (climate_learn/_fp32.py:
fp32 tokens, fp32 GEMM / attention / LayerNorm kernels reading the fp32 master parameters); the default is bf16.

There is no CPU / eager fallback: inputs must live on a gfx950 device.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch
import torch.nn as nn

from ... import _fp32, _hip, _ops
from ...dist import tp as _tp
from ...utils.fused_attn import FusedAttn
from .components.attention import VariableMapping_Attention
from .components.mlp import HipLinear, McDropoutMode
from .components.patch_embed import PatchEmbed, _ConvParams
from .components.pos_embed import _orig_grid, get_2d_sincos_pos_embed
from .components.vit_blocks import Block, HipLayerNorm
from .utils import register

_CONSTS = ("land_sea_mask", "orography", "lattitude", "landcover")


class _Gelu(nn.Module):
    """placeholder keeping nn.Sequential indices (`head.0, head.2, ...`, `path2.0, path2.3`) identical to the
    reference's Sequential(Linear, GELU, ...) layout; the activation itself is fused into the kernels."""

    def forward(self, x):  # pragma: no cover - never called on the fused path
        raise RuntimeError("fused in the producing kernel")


class _PixelShuffle(_Gelu):
    pass


@register("res_slimvit")
class Res_Slim_ViT(McDropoutMode, nn.Module):
    def __init__(self, default_vars, img_size, in_channels, out_channels, history, superres_mag=4, cnn_ratio=4,
                 patch_size=16, drop_path=0.1, drop_rate=0.1, learn_pos_emb=False, embed_dim=1024, depth=24,
                 decoder_depth=8, num_heads=16, mlp_ratio=4.0, tensor_par_size=1, tensor_par_group=None,
                 FusedAttn_option=FusedAttn.HIP):
        super().__init__()
        if patch_size not in _hip.PATCH_SIZES:
            raise NotImplementedError(
                "patch_size=%r: the folded patch-embed kernels serve patch_size in %s (at 8 the 65 float4 table rows a thread "
                "holds and the patch tile in LDS no longer fit the kernel's shape)" % (patch_size, _hip.PATCH_SIZES))
        if patch_size != 2 and tensor_par_size > 1:
            raise NotImplementedError("tensor_par_size=%d with patch_size=%d: tensor parallelism is built and tested for "
                                      "patch_size=2 only" % (tensor_par_size, patch_size))
        if tensor_par_size > 1:
            if tensor_par_group is None or _tp.group_size(tensor_par_group) != tensor_par_size:
                raise ValueError("tensor_par_size=%d needs a tensor_par_group of that many ranks" % tensor_par_size)
            assert num_heads % tensor_par_size == 0, "model heads % tensor parallel size must be 0"
        else:
            tensor_par_group = None
        self.default_vars = list(default_vars)
        self.img_size = tuple(img_size)
        self.cnn_ratio, self.superres_mag = cnn_ratio, superres_mag
        self.in_channels = in_channels * history
        self.out_channels = out_channels
        self.patch_size, self.history, self.embed_dim = patch_size, history, embed_dim
        self.num_heads, self.decoder_depth = num_heads, decoder_depth
        self.spatial_resolution = 0
        self.tensor_par_size, self.tensor_par_group = tensor_par_size, tensor_par_group
        D = embed_dim

        self.spatial_embed = HipLinear(1, D)
        self.token_embeds = nn.ModuleList([PatchEmbed(img_size, patch_size, 1, D) for _ in self.default_vars])
        self.num_patches = self.token_embeds[0].num_patches
        self.var_map = {v: i for i, v in enumerate(self.default_vars)}
        self.var_embed = nn.Parameter(torch.zeros(1, len(self.default_vars), D))
        self.var_query = nn.Parameter(torch.zeros(1, 1, D))
        self.var_agg = VariableMapping_Attention(D, fused_attn=FusedAttn_option, num_heads=num_heads, qkv_bias=False,
                                                 tensor_par_size=tensor_par_size, tensor_par_group=tensor_par_group)
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches, D), requires_grad=learn_pos_emb)
        self.pos_drop_p = float(drop_rate)
        rates = torch.linspace(0, drop_path, depth).tolist()
        self.blocks = nn.ModuleList([
            Block(D, num_heads=num_heads, fused_attn=FusedAttn_option, mlp_ratio=mlp_ratio, qkv_bias=True,
                  drop_path=rates[i], proj_drop=drop_rate, attn_drop=drop_rate, tensor_par_size=tensor_par_size,
                  tensor_par_group=tensor_par_group) for i in range(depth)])
        self.norm = HipLayerNorm(D)

        s = superres_mag
        self.path2 = nn.Sequential(_ConvParams(out_channels + 4, cnn_ratio * s * s, 3), _Gelu(), _PixelShuffle(),
                                   _ConvParams(cnn_ratio, out_channels, 3))
        head: List[nn.Module] = []
        for _ in range(decoder_depth):
            head += [HipLinear(D, D), _Gelu()]
        head.append(HipLinear(D, out_channels * (s * patch_size) ** 2))
        self.head = nn.Sequential(*head)
        self.conv_out = _ConvParams(out_channels, out_channels, 3)
        # fp32-compute parameters (tables / convs / embeddings) are flagged on the tensors themselves
        for p in (self.spatial_embed.weight, self.spatial_embed.bias):
            p._o2_lowp = False
        self.initialize_weights()
        self._idx_cache = {}
        self._compute_dtype = torch.bfloat16
        if tensor_par_size > 1:
            _tp.tag_sharded(self)

    # ------------------------------------------------------------------ compute precision
    @property
    def compute_dtype(self):
        """precision of the token path: torch.bfloat16 (default; training and inference) or torch.float32 (forward-only
        inference, the reference's `data_type: float32`).  A plain attribute of the object: not part of `state_dict`."""
        return self._compute_dtype

    def set_compute_dtype(self, dtype):
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("compute_dtype must be torch.bfloat16 or torch.float32, got %r" % (dtype,))
        self._compute_dtype = dtype
        return self

    # ------------------------------------------------------------------ init (res_slimvit.py:125-145)
    def initialize_weights(self):
        pe = get_2d_sincos_pos_embed(self.embed_dim, self.img_size[0] // self.patch_size,
                                     self.img_size[1] // self.patch_size)
        with torch.no_grad():
            self.pos_embed.copy_(torch.from_numpy(pe).float().unsqueeze(0))

    def data_config(self, res, img_size, in_channels, out_channels):
        """Rebinds the run-time data attributes only; no weights change (res_slimvit.py:148-165)."""
        self.spatial_resolution = res
        self.img_size = tuple(img_size)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_patches = img_size[0] * img_size[1] // self.patch_size ** 2

    # ------------------------------------------------------------------ helpers
    def get_var_ids(self, variables: Sequence[str]):
        return [self.var_map[v] for v in variables]

    def find_var_index(self, in_variables, out_variables):
        idx = [in_variables.index(v) for v in out_variables]
        for c in _CONSTS:
            idx.append(in_variables.index(c))          # ValueError if a constant is missing, as in the reference
        return idx

    def _chan_idx(self, in_variables, out_variables, device):
        key = (tuple(in_variables), tuple(out_variables), str(device))
        t = self._idx_cache.get(key)
        if t is None:
            t = torch.tensor(self.find_var_index(list(in_variables), list(out_variables)), dtype=torch.int32,
                             device=device)
            self._idx_cache[key] = t
        return t

    def unpatchify(self, x, scaling=1, out_channels=1):
        return _ops.UnpatchifyFn.apply(x, out_channels, self.img_size[0], self.img_size[1], self.patch_size, scaling)

    def _tables(self, ids):
        """Score / value tables of the folded variable aggregation (fp32, autograd through the HIP sgemm)."""
        D, grp = self.embed_dim, self.tensor_par_group
        dh = D // self.num_heads
        H = self.num_heads // self.tensor_par_size       # heads of this tensor-parallel rank; Dl = H * dh columns
        Dl = H * dh
        wq, wkv = self.var_agg.q.weight, self.var_agg.kv.weight                  # [Dl, D], [2 Dl, D]
        vq = self.var_query.view(1, D)
        if grp is not None:    # replicated inputs of a head-split attention: their gradients are partial per rank
            vq = _tp.IdentityFwdAllReduceBwd.apply(vq, grp)            # (attention.py:134-137)
        qv = _ops.sgemm(vq, wq, tb=True)                                         # [1, Dl] = var_query Wq^T
        ekey = ("eye", H, str(wq.device))
        eye = self._idx_cache.get(ekey)
        if eye is None:
            eye = self._idx_cache[ekey] = torch.eye(H, dtype=torch.float32, device=wq.device).unsqueeze(-1)
        qblk = (eye * qv.view(1, H, dh)).view(H, Dl)                             # [H, Dl], head-block structure (one launch)
        u = _ops.sgemm(qblk, wkv[:Dl]) * (dh ** -0.5)                            # [H, D] = scale * q_h^T Wk_h
        # rows (v, c): the p*p patch weights of variable v (row-major inside the patch, the order of Conv2d(1, D, p, p).weight
        # .view(D, p*p)) and its bias + variable embedding -- built for all variables at once
        # (five launches forward; the per-variable form was ~12 tiny launches per variable and step, 10 % of an interm_117m step)
        tes = [self.token_embeds[v].proj for v in ids]
        key = (tuple(ids), str(wq.device))
        ids_t = self._idx_cache.get(key)
        if ids_t is None:
            ids_t = self._idx_cache[key] = torch.tensor(list(ids), dtype=torch.long, device=wq.device)
        PP = self.patch_size ** 2
        # the fused gather / scatter (orbit2_tables_gather / _scatter) is 4-wide, tied to the engines' flat buffers at
        # patch_size=2: every other patch size takes the ATen path below, whose gradients accumulate through autograd
        lay = self._token_tables_layout() if torch.is_grad_enabled() and self.patch_size == 2 else None
        # the fused path's backward adds into the gradient rows WITHOUT atomics, one workgroup per id, and announces the parameters
        # to the engine itself: it needs distinct variable ids (a duplicated id would make two workgroups race on one row -- the
        # ATen path accumulates duplicates correctly) and at most ONE instance per backward (two forwards feeding one backward: the
        # first node's `grad_ready` would launch the bucket's all-reduce before the second node's rows have landed).  (advisor r5)
        pending = self.__dict__.setdefault("_tables_pending", [0])
        if lay is not None and pending[0] > 0:
            eng = getattr(self.var_embed, "_o2_engine", None)
            reduces = getattr(eng, "comm", None)              # (sharding engine) / world, force_comm (replicated engine)
            if reduces is None:
                reduces = getattr(eng, "world", 1) > 1 or getattr(eng, "force_comm", False)
            if reduces and getattr(self, "fused_tables", True):
                # with collectives the outstanding fused node will announce the table parameters when ITS backward has run: a
                # second use of them in the same backward (this forward) could land after the bucket's all-reduce was launched
                raise RuntimeError("Res_Slim_ViT: a second forward before the previous one's backward, under a data-parallel engine: "
                                   "set model.fused_tables = False (the ATen table path accumulates any number of uses)")
            lay = None
        if lay is not None and (len(set(ids)) != len(ids) or not getattr(self, "fused_tables", True)):
            lay = None
        if lay is not None:
            # engine-managed parameters at a uniform pitch: one launch forward, one backward that accumulates straight into
            # the engine's gradient bucket (no stack / transpose / cat, no per-parameter autograd accumulation)
            k32 = key + ("i32",)
            ids32 = self._idx_cache.get(k32)
            if ids32 is None:
                ids32 = self._idx_cache[k32] = ids_t.to(torch.int32)
            flat = [te.weight for te in tes] + [te.bias for te in tes]
            lay = dict(lay, pending=pending)
            cmat = _ops.TokenTablesFn.apply(lay, ids32, len(ids), D, self.var_embed, *flat)
        else:
            w4 = torch.stack([te.weight.view(D, PP) for te in tes]).transpose(1, 2)   # [V, p*p, D]
            b1 = torch.stack([te.bias for te in tes]) + self.var_embed[0].index_select(0, ids_t)        # [V, D]
            cmat = torch.cat([w4, b1.unsqueeze(1)], 1).reshape(len(ids) * (PP + 1), D)   # [(v,c), D]
        if grp is not None:
            cmat = _tp.IdentityFwdAllReduceBwd.apply(cmat, grp)
        stab = _ops.sgemm(u, cmat, tb=True).view(H, len(ids), PP + 1)
        gtab = _ops.sgemm(cmat, wkv[Dl:], tb=True).view(len(ids), PP + 1, Dl)
        return stab, gtab

    def _token_tables_layout(self):
        """cached `_ops.token_tables_layout` (re-derived when the parameters move: another engine, a re-wrap)"""
        w0 = self.token_embeds[0].proj.weight
        sig = (id(getattr(w0, "_o2_engine", None)), w0.data_ptr(), w0.grad.data_ptr() if w0.grad is not None else 0)
        hit = self._idx_cache.get("te_layout")
        if hit is None or hit[0] != sig:
            hit = self._idx_cache["te_layout"] = (sig, _ops.token_tables_layout(list(self.token_embeds), self.var_embed))
        return hit[1]

    def _posres(self):
        """[L, D] fp32: pos_embed on the run's token grid (bicubic re-grid when the grid differs from the one the table
        was built on, reference pos_embed.py:103-138) + spatial_embed(resolution) (reference :277-281) -- one HIP launch"""
        oh, ow = _orig_grid(self.pos_embed.shape[-2])
        nh, nw = self.img_size[0] // self.patch_size, self.img_size[1] // self.patch_size
        if oh == nh:
            ow = nw                                      # (the reference uses the table as it is whenever the heights agree)
        return _ops.PosResFn.apply(self.pos_embed, self.spatial_embed.weight, self.spatial_embed.bias,
                                   float(self.spatial_resolution), oh, ow, nh, nw)

    def pos_p(self):
        """pos_drop probability actually applied: train mode or MC-dropout mode (utils/mc_dropout.py)"""
        return self.pos_drop_p if (self.training or self.mc_dropout) else 0.0

    # ------------------------------------------------------------------ forward (res_slimvit.py:245-338)
    def forward_encoder(self, x, variables):
        ids = self.get_var_ids(tuple(variables))
        stab, gtab = self._tables(ids)
        p = self.pos_p()
        t = _ops.EmbedFn.apply(x, stab, gtab, self._posres(), self.var_agg.proj.weight, self.var_agg.proj.bias,
                               self.num_heads // self.tensor_par_size, p, self.tensor_par_group)
        for blk in self.blocks:
            t = blk(t)
        return t

    def forward(self, x, in_variables, out_variables):
        if x.dim() == 5:
            x = x.flatten(1, 2)
        if self.patch_size != 2 and any(getattr(p, "_o2_sharded", False) for p in self.parameters()):
            raise NotImplementedError("Res_Slim_ViT with patch_size=%d under the parameter-sharding engine "
                                      "(HipFullyShardedDataParallel): that engine is built and tested for patch_size=2 only; "
                                      "HipDataParallel serves 1, 2 and 4" % self.patch_size)
        if not x.is_cuda:
            raise RuntimeError("Res_Slim_ViT (HIP build) needs its input on a gfx950 device; there is no CPU path")
        x = x.float().contiguous()
        B, V, h, w = x.shape
        if (h, w) != tuple(self.img_size):
            raise ValueError("input grid %s differs from data_config'd img_size %s" % ((h, w), self.img_size))
        if h % self.patch_size or w % self.patch_size:
            raise ValueError("input grid %s is not a multiple of patch_size=%d" % ((h, w), self.patch_size))
        if self._compute_dtype == torch.float32:
            _fp32.refuse(self)
            return _fp32.forward(self, x, in_variables, out_variables)
        cidx = self._chan_idx(in_variables, out_variables, x.device)
        c0, c3 = self.path2[0], self.path2[3]
        r = _ops.Conv3x3Fn.apply(x, c0.weight, c0.bias, cidx, 1, self.superres_mag, None)
        r = _ops.Conv3x3Fn.apply(r, c3.weight, c3.bias, None, 0, 1, None)
        t = self.forward_encoder(x, in_variables)
        prm = [self.norm.weight, self.norm.bias]
        for m in self.head:
            if isinstance(m, HipLinear):
                prm += [m.weight, m.bias]
        t = _ops.unit_enter(self.head, t)
        t = _ops.unit_exit(self.head, _ops.ChainFn.apply(t, {"ln": True}, *prm))
        img = self.unpatchify(t, scaling=self.superres_mag, out_channels=self.out_channels)
        co = self.conv_out
        return _ops.Conv3x3Fn.apply(img, co.weight, co.bias, None, 0, 1, r)
