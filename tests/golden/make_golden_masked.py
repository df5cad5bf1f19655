#!/usr/bin/env python3
"""Golden vectors for the missing-data masks, produced by the REFERENCE's own functions
(metrics/functional.py: rmse with `mask`, :236-255; mse and bayesian_tv, :117-202) with the same import recipe as
make_golden_eval.py.  Build container only (needs the reference); writes tests/golden/masked.npz (arrays only).

  rmse.*   the reference's masked rmse for a [B,1,H,W] and a [B,C,H,W] mask, with and without latitude weights, on a FINITE
           target: the test puts NaN where `nan_where` says and the reference was given a zero there (it multiplies by the mask,
           so any finite value gives the same result).
  rect.*   mse / bayesian_tv of the reference on the 11 x 23 top-left crop of pred, target and the latitude weights: what the
           masked losses must give when the valid region is exactly that rectangle.
Everything is computed by the reference in float64 on the fp32-rounded inputs stored here, and stored as float64."""
import importlib
import os

import numpy as np
import torch

from make_golden import OUT, install_shims, t2n

B, C, H, W = 2, 3, 19, 37
H0, W0 = 11, 23
VAR_NAMES = ["a", "b", "c"]
VAR_WEIGHTS = {"a": 1.0, "b": 10.0, "c": 10.0}


def main():
    install_shims()
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        dist.init_process_group("gloo", rank=0, world_size=1)
    fn = importlib.import_module("climate_learn.metrics.functional")
    g = torch.Generator().manual_seed(321)
    pred = torch.randn(B, C, H, W, generator=g) * 1.7 + 0.3
    target = 0.6 * pred + torch.randn(B, C, H, W, generator=g)
    lat = np.linspace(-80.0, 80.0, H)
    wl = np.cos(np.deg2rad(lat))
    wl = torch.from_numpy(wl / wl.mean()).view(1, 1, -1, 1).float()
    mask_b1 = (torch.rand(B, 1, H, W, generator=g) > 0.4).float()
    mask_bc = (torch.rand(B, C, H, W, generator=g) > 0.4).float()
    nan_where = torch.zeros(B, C, H, W, dtype=torch.bool)
    nan_where[0, 1, 3:9, 5:17] = True
    nan_where[1, 2, :, 30:] = True
    nan_where[1, 0, 0, :] = True
    n64 = lambda t: t.detach().numpy().astype(np.float64)            # outputs: float64 as computed
    pred64, target64, wl64 = pred.double(), target.double(), wl.double()
    finite_target = torch.where(nan_where, torch.zeros((), dtype=torch.float64), target64)
    out = {"pred": t2n(pred), "target": t2n(target), "lat": lat, "lat_w": t2n(wl.reshape(-1)), "mask_b1": t2n(mask_b1),
           "mask_bc": t2n(mask_bc), "nan_where": nan_where.numpy()}
    for tag, m in (("b1", mask_b1), ("bc", mask_bc)):
        valid = m.double().expand(B, C, H, W) * (~nan_where).double()           # the validity: the reference's "mask"
        out["rmse." + tag] = n64(fn.rmse(pred64, finite_target, False, None, valid))
        out["lat_rmse." + tag] = n64(fn.rmse(pred64, finite_target, False, wl64, valid))
    out["rmse.ones"] = n64(fn.rmse(pred64, target64, False, None, torch.ones(B, C, H, W, dtype=torch.float64)))
    out["rmse.plain"] = n64(fn.rmse(pred64, target64, False))
    pc, tc, wc = pred64[:, :, :H0, :W0], target64[:, :, :H0, :W0], wl64[:, :, :H0]
    out["rect_hw"] = np.array([H0, W0])
    out["var_weights"] = np.array([VAR_WEIGHTS[v] for v in VAR_NAMES])
    for name in ("mse", "bayesian_tv"):
        f = getattr(fn, name)
        out["rect.%s" % name] = n64(f(pc, tc))
        out["rect.%s.lat" % name] = n64(f(pc, tc, None, None, False, wc))
        out["rect.%s.var" % name] = n64(f(pc, tc, VAR_NAMES, VAR_WEIGHTS))
        out["rect.%s.lat.var" % name] = n64(f(pc, tc, VAR_NAMES, VAR_WEIGHTS, False, wc))
    np.savez_compressed(os.path.join(OUT, "masked.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
