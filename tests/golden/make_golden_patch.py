#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's Res_Slim_ViT at patch sizes 1 and 4 (make_golden.py pins patch size 2 only).

Runs only where the reference tree exists (make_golden.REF); nothing under tests/, bench.py or smoke() imports this module,
they read the .npz files it wrote.  No reference source text is stored -- only numeric inputs and outputs.  The import shims
are make_golden.install_shims, reused as they are.

Per case: the state dict ("p." + name), the input x, the target y, the prediction, the per-channel + aggregate bayesian_tv loss
and the gradients of one bayesian_tv step ("g.bayesian_tv." + name), as in model_*.npz.  Token grids are 2:1 (W:H), which the
reference's pos-embed re-grid assumes.

Usage:  python tests/golden/make_golden_patch.py          (writes tests/golden/model_patch{1,4}.npz)
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402

CONST = ["land_sea_mask", "orography", "lattitude", "landcover"]
CASES = {
    "patch1": dict(patch=1, grid=(4, 8)),
    "patch4": dict(patch=4, grid=(16, 32)),
}
IN_VARS = CONST + ["total_precipitation_24hr"]
OUT_VARS = ["total_precipitation_24hr"]
D, DEPTH, HEADS, DD, B = 64, 1, 2, 1, 2
VW = {"total_precipitation_24hr": 1.0}


def main():
    MG.install_shims()
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    rs = importlib.import_module("climate_learn.models.hub.res_slimvit")
    fa = importlib.import_module("climate_learn.utils.fused_attn")
    fn = importlib.import_module("climate_learn.metrics.functional")
    for tag, c in CASES.items():
        torch.manual_seed(0)
        Vn, C = len(IN_VARS), len(OUT_VARS)
        model = rs.Res_Slim_ViT(IN_VARS, c["grid"], Vn, C, history=1, superres_mag=4, cnn_ratio=4, patch_size=c["patch"],
                                drop_path=0.1, drop_rate=0.1, learn_pos_emb=True, embed_dim=D, depth=DEPTH,
                                decoder_depth=DD, num_heads=HEADS, mlp_ratio=4, FusedAttn_option=fa.FusedAttn.NONE)
        gg = torch.Generator().manual_seed(4321 + c["patch"])
        MG.randomize_(model, gg, 0.08)
        model.data_config(156.0, c["grid"], Vn, C)
        model.eval()
        h, w = c["grid"]
        x = torch.randn(B, Vn, h, w, generator=gg)
        y = torch.randn(B, C, 4 * h + 3, 4 * w + 5, generator=gg)      # bigger than 4x -> cropped by the step
        y[:, 0] = torch.log1p(torch.relu(y[:, 0]))
        out = {"x": MG.t2n(x), "y": MG.t2n(y)}
        pred = model(x, IN_VARS, OUT_VARS)
        out["pred"] = MG.t2n(pred)
        yhat = pred.clone()
        yhat[:, 0] = torch.clamp(pred[:, 0], min=0.0)
        yc = y[:, :, : yhat.shape[2], : yhat.shape[3]]
        model.zero_grad()
        full = fn.bayesian_tv(yhat, yc, OUT_VARS, VW, False)
        out["loss.bayesian_tv"] = MG.t2n(full)
        full[-1].backward()
        for n, prm in model.named_parameters():
            if prm.grad is not None:
                out["g.bayesian_tv." + n] = MG.t2n(prm.grad)
        for n, prm in model.state_dict().items():
            out["p." + n] = MG.t2n(prm)
        path = os.path.join(HERE, "model_%s.npz" % tag)
        np.savez_compressed(path, **out)
        print("  %-20s %8.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
