"""orbit2_resample_fwd / orbit2_resample_moments on the device (through _hip.resample / _hip.resample_moments) against the
float64 replica of the coordinate contract (tests/resample_ref.py) and, for nearest, the golden file bit for bit.

Cases (resample_ref.GPU_CASES), each in three modes, at offsets 0 and 280, with and without the affine, five input channels of
which 4, 0, 2 are read, B = 2: 5x7 -> 40x56 (clamped taps on all four edges, a partial tile), 6x10 -> 17x23 (non-integer, odd W:
scalar stores, every second row misaligned), 9x13 -> 4x5 (downsampling: the global-memory path), 1x1 -> 8x8, 3x4 -> 3x4
(identity) and 9x130 -> 35x517 (3 x 3 tiles).  The output is written into a NaN-filled buffer with guards on both sides, once
on a 16-byte boundary and once off it.

Bounds (derived in tests/test_resample_cpu.py): |kernel - replica| <= FIELD_TOL * max|x| = 8 * 2^-24 (bilinear) and
20 * 2^-24 (bicubic), 0 for nearest and the identity; with the affine that bound times |scale[c]| plus one ulp of the result.
The twelve sums of resample_moments: within MOMENTS_RTOL = 6.4e-7 (offset 0) / 1.16e-4 (offset 280) of the sum of their
summands' magnitudes -- 4 x the worst of the fp32 emulation of the built per-lane trip count against float64 -- of the float64
sums of the replica field, and of _hip.eval_moments(_hip.resample(...)) on the same operands."""
import os

import numpy as np
import pytest
import torch

from tests import resample_gpu_body as B
from tests import resample_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
CASE_IDS = B.case_ids(R.GPU_CASES)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "resample.npz")))


def _exact(mode, hw, HW):
    return mode == "nearest" or hw == HW


@pytest.mark.parametrize("hw,HW", R.GPU_CASES, ids=CASE_IDS)
def test_resample_fwd(golden, hw, HW):
    from climate_learn import _hip
    assert _hip.resample_staged(*hw, *HW) == (hw != (9, 13)), "9x13 -> 4x5 is the case that must read from global memory"
    if hw == (9, 130):
        assert -(-HW[0] // _hip.RESAMPLE_TILE[0]) >= 3 and -(-HW[1] // _hip.RESAMPLE_TILE[1]) >= 3

    def golden_bits(got, xh, mode, off):
        key = R.case_key(hw, HW, mode, off)
        if mode == "nearest" and key in golden:
            assert np.array_equal(got, golden[key]), "nearest differs from the reference's bits"

    B.check_fwd(hw, HW, lambda off: R.gpu_input(hw, HW, off, golden), R.replica,
                lambda mode: 0.0 if _exact(mode, hw, HW) else R.FIELD_TOL[mode], R.MODES, False, golden_bits)


@pytest.mark.parametrize("hw,HW", R.GPU_CASES, ids=CASE_IDS)
def test_resample_moments(golden, hw, HW):
    B.check_moments(hw, HW, lambda off: R.gpu_input(hw, HW, off, golden), R.replica,
                    lambda mode, off: R.MOMENTS_RTOL[int(off)], R.MODES, False)


def test_resample_binding_refusals():
    from climate_learn import _hip
    x = torch.zeros(2, 5, 5, 7, device="cuda")
    with pytest.raises(_hip.HipBackendError, match="together"):
        _hip.resample(x, (8, 8), scale=torch.ones(5, device="cuda"))
    with pytest.raises(_hip.HipBackendError, match="one entry per output channel"):
        _hip.resample(x, (8, 8), channels=[0, 1], scale=[1.0] * 5, shift=[0.0] * 5)
    with pytest.raises(_hip.HipBackendError, match="out is"):
        _hip.resample(x, (8, 8), out=torch.zeros(2, 5, 8, 9, device="cuda"))
    with pytest.raises(_hip.HipBackendError, match="contiguous"):
        _hip.resample(x.transpose(2, 3), (8, 8))
    with pytest.raises(_hip.HipBackendError, match="requires grad"):
        _hip.resample(x.clone().requires_grad_(), (8, 8))
    with pytest.raises(_hip.HipBackendError, match="smaller than the prediction"):
        _hip.resample_moments(x, (8, 8), "nearest", torch.zeros(2, 5, 8, 7, device="cuda"))
    with pytest.raises(_hip.HipBackendError, match=r"does not match the prediction's \[B,C\]"):
        _hip.resample_moments(x, (8, 8), "nearest", torch.zeros(2, 4, 8, 8, device="cuda"))
