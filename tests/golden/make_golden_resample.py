#!/usr/bin/env python3
"""Golden vectors for the interpolation baselines (reference models/hub/interpolation.py: Interpolation(size, mode) =
F.interpolate(x, size, mode=mode)), produced by the REFERENCE's own module with the same import recipe as make_golden.py.
Build container only (needs /root/reference); writes tests/golden/resample.npz (numeric inputs and outputs only).

Eight pairs of sizes (tests/resample_ref.py: SHAPES) x {nearest, bilinear, bicubic} x offsets {0, 280}; B = 2, C = 3 where the
output is small, B = C = 1 for the three pairs whose output has more than 20 000 pixels.  Of those three only SAMPLE pixels of
every output are kept (the four corners and a fixed random draw, `<pair>.sample` = their flat indices in [H*W]): one whole
721 x 1440 field is 4 MiB, four times what a committed file may hold.  Keys: `<pair>.x` the input at offset 0 (the input at 280 is
(x + 280) in fp32), `<pair>.<mode>.<offset>` the output."""
import importlib
import os
import sys

import numpy as np
import torch

from make_golden import OUT, install_shims

sys.path.insert(0, os.path.dirname(OUT))
from resample_ref import OFFSETS, MODES, SHAPES, case_key  # noqa: E402

SAMPLE = 4096
BIG = 20000


def main():
    install_shims()
    Interpolation = importlib.import_module("climate_learn.models.hub.interpolation").Interpolation
    g = torch.Generator().manual_seed(2024)
    rng = np.random.default_rng(7)
    out = {}
    for hw, HW in SHAPES:
        big = HW[0] * HW[1] > BIG
        B, C = (1, 1) if big else (2, 3)
        x = torch.randn(B, C, *hw, generator=g)
        pair = case_key(hw, HW)
        out[pair + ".x"] = x.numpy()
        if big:
            n = HW[0] * HW[1]
            corners = np.array([0, HW[1] - 1, n - HW[1], n - 1])
            sample = np.unique(np.concatenate([corners, rng.choice(n, SAMPLE - 4, replace=False)])).astype(np.int32)
            out[pair + ".sample"] = sample
        for off in OFFSETS:
            xo = torch.from_numpy((x.numpy() + np.float32(off)).astype(np.float32))
            for mode in MODES:
                y = Interpolation(HW, mode)(xo).numpy()
                assert y.dtype == np.float32 and y.shape == (B, C) + HW
                out[case_key(hw, HW, mode, off)] = y.reshape(B, C, -1)[..., sample] if big else y
    path = os.path.join(OUT, "resample.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
