#!/usr/bin/env python3
"""Golden vectors for the probabilistic scores (gaussian_spread / gaussian_spread_skill_ratio, reference
metrics/functional.py:363-386), produced by the REFERENCE's own functions with the same import recipe as make_golden.py.
Build container only (needs /root/reference); writes tests/golden/probabilistic.npz (numeric inputs and outputs only).
The reference's gaussian_crps is not recorded: it cannot be called (torch.zeros_like on a Normal raises TypeError); the test
compares against the closed form instead."""
import importlib
import os

import numpy as np
import torch

from make_golden import OUT, install_shims, t2n


def main():
    install_shims()
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        dist.init_process_group("gloo", rank=0, world_size=1)
    fn = importlib.import_module("climate_learn.metrics.functional")
    g = torch.Generator().manual_seed(321)
    mean = torch.randn(3, 3, 24, 40, generator=g) * 1.7 + 0.3
    std = torch.rand(3, 3, 24, 40, generator=g) * 0.9 + 0.05
    target = mean + std * torch.randn(3, 3, 24, 40, generator=g) * 1.3
    lat = np.linspace(-88.0, 88.0, 24)
    wl = np.cos(np.deg2rad(lat))
    wl = torch.from_numpy(wl / wl.mean()).view(1, 1, -1, 1).float()
    pred = torch.distributions.Normal(mean, std)
    try:
        fn.gaussian_crps(pred, target)
        crps_callable = 1.0
    except TypeError:
        crps_callable = 0.0
    out = {"mean": t2n(mean), "std": t2n(std), "target": t2n(target), "lat": lat,
           "reference_crps_callable": np.array(crps_callable),
           "spread": t2n(fn.gaussian_spread(pred, False)), "spread.agg": t2n(fn.gaussian_spread(pred, True)),
           "lat_spread": t2n(fn.gaussian_spread(pred, False, wl)), "lat_spread.agg": t2n(fn.gaussian_spread(pred, True, wl)),
           "ratio": t2n(fn.gaussian_spread_skill_ratio(pred, target, False)),
           "ratio.agg": t2n(fn.gaussian_spread_skill_ratio(pred, target, True)),
           "lat_ratio": t2n(fn.gaussian_spread_skill_ratio(pred, target, False, wl)),
           "lat_ratio.agg": t2n(fn.gaussian_spread_skill_ratio(pred, target, True, wl))}
    np.savez_compressed(os.path.join(OUT, "probabilistic.npz"), **out)
    print({k: (v.shape, v.reshape(-1)[:4]) for k, v in out.items() if k not in ("mean", "std", "target")})


if __name__ == "__main__":
    main()
