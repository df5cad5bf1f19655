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

from tests import resample_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
CASE_IDS = ["%dx%d-%dx%d" % (hw + HW) for hw, HW in R.GPU_CASES]
GUARD = 64


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "resample.npz")))


def _affine(on):
    return (R.GPU_SCALE, R.GPU_SHIFT) if on else (None, None)


def _run_into_guards(x, HW, mode, scale, shift, lead):
    """_hip.resample into the middle of a NaN-filled buffer; returns the field and checks that nothing else was written"""
    from climate_learn import _hip
    n = x.shape[0] * len(R.GPU_CHANNELS) * HW[0] * HW[1]
    buf = torch.full((lead + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[lead:lead + n].view(x.shape[0], len(R.GPU_CHANNELS), *HW)
    sc = None if scale is None else torch.tensor(scale, device="cuda")
    sh = None if shift is None else torch.tensor(shift, device="cuda")
    got = _hip.resample(x, HW, mode, channels=R.GPU_CHANNELS, scale=sc, shift=sh, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[:lead]).all() and np.isnan(host[lead + n:]).all(), "wrote outside the output"
    field = host[lead:lead + n].reshape(out.shape)
    assert not np.isnan(field).any(), "left pixels unwritten"
    return field


@pytest.mark.parametrize("hw,HW", R.GPU_CASES, ids=CASE_IDS)
def test_resample_fwd(golden, hw, HW):
    from climate_learn import _hip
    assert _hip.resample_staged(*hw, *HW) == (hw != (9, 13)), "9x13 -> 4x5 is the case that must read from global memory"
    if hw == (9, 130):
        assert -(-HW[0] // _hip.RESAMPLE_TILE[0]) >= 3 and -(-HW[1] // _hip.RESAMPLE_TILE[1]) >= 3
    worst = dict.fromkeys(R.MODES, 0.0)
    for off in R.OFFSETS:
        xh = R.gpu_input(hw, HW, off, golden)
        x = torch.from_numpy(xh).cuda()
        xmax = float(np.abs(xh[:, list(R.GPU_CHANNELS)]).max())
        for mode in R.MODES:
            for aff in (False, True):
                scale, shift = _affine(aff)
                rep = R.replica(xh, HW, mode, R.GPU_CHANNELS, scale, shift)
                for lead in (GUARD, GUARD - 3):              # the output on a 16-byte boundary, and off it
                    got = _run_into_guards(x, HW, mode, scale, shift, lead)
                    err = np.abs(got.astype(np.float64) - rep)
                    exact = mode == "nearest" or hw == HW
                    tol = 0.0 if exact else R.FIELD_TOL[mode] * xmax
                    if aff:
                        bound = np.abs(np.asarray(scale))[None, :, None, None] * tol + 2.0 ** -23 * np.abs(rep)
                    else:
                        bound = np.full_like(rep, tol)
                        worst[mode] = max(worst[mode], float(err.max()) / xmax)
                    print("%s %s offset %d affine %d lead %d: worst %.4g = %.3g ulp(max|x|), bound %.4g"
                          % (R.case_key(hw, HW), mode, off, aff, lead, err.max(), err.max() / xmax / R.ULP, bound.max()))
                    assert (err <= bound).all()
                    key = R.case_key(hw, HW, mode, off)
                    if mode == "nearest" and not aff and key in golden:
                        assert np.array_equal(got, golden[key]), "nearest differs from the reference's bits"
                    if exact and not aff:
                        assert np.array_equal(got.astype(np.float64), rep)
    print("worst |kernel - replica| / max|x| in ulp:", {m: round(v / R.ULP, 3) for m, v in worst.items()})


@pytest.mark.parametrize("hw,HW", R.GPU_CASES, ids=CASE_IDS)
def test_resample_moments(golden, hw, HW):
    from climate_learn import _hip
    worst = 0.0
    for off in R.OFFSETS:
        xh = R.gpu_input(hw, HW, off, golden)
        th, lat, clim = R.gpu_target(HW, off)
        x, t = torch.from_numpy(xh).cuda(), torch.from_numpy(th).cuda()
        for mode in R.MODES:
            for aff in ((False, True) if off == 0 else (False,)):
                scale, shift = _affine(aff)
                sc = None if scale is None else torch.tensor(scale, device="cuda")
                sh = None if shift is None else torch.tensor(shift, device="cuda")
                rep = R.replica(xh, HW, mode, R.GPU_CHANNELS, scale, shift)
                field = _hip.resample(x, HW, mode, channels=R.GPU_CHANNELS, scale=sc, shift=sh)
                for lw in (None, lat):
                    for cl in (None, clim):
                        lwd = None if lw is None else torch.from_numpy(lw).cuda()
                        cld = None if cl is None else torch.from_numpy(cl).cuda()
                        got = _hip.resample_moments(x, HW, mode, t, channels=R.GPU_CHANNELS, scale=sc, shift=sh, lat_w=lwd,
                                                    clim=cld).cpu().numpy()
                        two = _hip.eval_moments(field, t, lwd, cld).cpu().numpy()
                        want, mag = R.moments64(rep, th, lw, cl)
                        assert got.shape == want.shape == (2, 3, 12) and np.isfinite(got).all()
                        e1, e2 = float((np.abs(got - want) / mag).max()), float((np.abs(got - two) / mag).max())
                        worst = max(worst, e1 / R.MOMENTS_RTOL[int(off)])
                        print("%s %s offset %d affine %d lat %d clim %d: against float64 %.3g, against the two-step path %.3g "
                              "(bound %.3g)" % (R.case_key(hw, HW), mode, off, aff, lw is not None, cl is not None, e1, e2,
                                                R.MOMENTS_RTOL[int(off)]))
                        assert e1 <= R.MOMENTS_RTOL[int(off)] and e2 <= R.MOMENTS_RTOL[int(off)]
    print("worst error of the twelve sums as a fraction of its bound: %.3g" % worst)


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
