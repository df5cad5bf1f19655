"""The twelve evaluation sums on the device (csrc/score_sums.h: o2_moments_add, o2_block_sums_add; _hip.eval_moments, and
_hip.masked_moments with everything valid) against tests/resample_ref.moments64, the float64 statement of the same sums, and the
operand checks every scored pair shares (_hip._scored_pair).

The error of a sum is |got - want| / mag, mag the float64 sum of its summands' magnitudes (the scale a rounding error lives on).
Shapes are the smallest that reach each path: nothing 16-byte aligned (scalar lanes), everything aligned (float4 items), and two
planes of 33 540 four-pixel items, more than one sweep of 64 workgroups x 256 threads (16 384), one of each kind."""
import numpy as np
import pytest
import torch

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

# The bound the project already applies to these twelve sums (fields at offset 0): 6.4e-7.  eval_moments of the commit before
# csrc/score_sums.h existed (the epilogue and the moments typed out in csrc/image.hip, now csrc/loss.hip) measured 6.35e-8 at worst over every case
# below, inside that bound, so this is the bound.
BOUND = R.MOMENTS_RTOL[0]
SCALAR = ((2, 3, 19, 37), (2, 3, 23, 41))
VEC = ((2, 2, 16, 64), (2, 2, 20, 64))
CASES = (SCALAR, VEC, ((1, 1, 260, 515), (1, 1, 261, 517)), ((1, 1, 260, 516), (1, 1, 261, 516)))
NAN_SUMS, FINITE_SUMS = [1, 3, 4, 5, 6, 8, 9, 11], [0, 2, 7, 10]          # those with the target in them, and the others

_cache = {}


def case(shapes):
    """CPU fp32 (pred, target, lat_w, clim) and the float64 (sums, magnitudes) with and without the weights; computed once"""
    if shapes not in _cache:
        shape, tshape = shapes
        B, C, H, W = shape
        g = torch.Generator().manual_seed(H * 1000 + W)
        pred = torch.randn(shape, generator=g) * 1.7 + 0.3
        target = 1e3 * torch.randn(tshape, generator=g)            # outside the crop: never read
        target[:, :, :H, :W] = 0.6 * pred + torch.randn(shape, generator=g)
        lat = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-80.0, 75.0, H)))).float()
        clim = 0.5 * torch.randn(C, H, W, generator=g)
        want = {False: R.moments64(pred.numpy(), target.numpy()),
                True: R.moments64(pred.numpy(), target.numpy(), lat.numpy(), clim.numpy())}
        _cache[shapes] = (pred, target, lat, clim, want)
    return _cache[shapes]


def err(got, want, mag):
    return np.abs(got.cpu().numpy() - want) / mag


@pytest.mark.parametrize("weighted", (False, True), ids=("plain", "lat_clim"))
@pytest.mark.parametrize("shapes", CASES, ids=lambda s: "x".join(map(str, s[0][2:])))
def test_eval_moments_against_float64(shapes, weighted):
    from climate_learn import _hip
    pred, target, lat, clim, want = case(shapes)
    got = _hip.eval_moments(pred.cuda(), target.cuda(), lat.cuda() if weighted else None, clim.cuda() if weighted else None)
    assert got.shape == pred.shape[:2] + (12,) and got.dtype == torch.float64
    e = err(got, *want[weighted])
    print("eval_moments %s weighted=%s: worst |got - want| / mag = %.3g (bound %.3g)" % (shapes[0], weighted, e.max(), BOUND))
    assert e.max() <= BOUND


@pytest.mark.parametrize("shapes", (SCALAR, VEC), ids=("scalar", "float4"))
def test_nan_propagates_as_before(shapes):
    """the unmasked sums do not look at validity: a NaN of the target inside the crop reaches exactly the sums that hold the
    target, in its own image only, and one outside the crop reaches nothing"""
    from climate_learn import _hip
    pred, target, lat, clim, want = case(shapes)
    H, W = pred.shape[2:]
    target = target.clone()
    target[1, 0, 3, 5] = float("nan")                  # inside the crop
    target[1, 0, H, 0] = float("nan")                  # outside it: the row below, in the same image and in another one
    target[0, 1, H, 2] = float("nan")
    if target.shape[3] > W:
        target[0, 1, 0, W] = float("nan")              # and the column to the right
    got = _hip.eval_moments(pred.cuda(), target.cuda(), lat.cuda(), clim.cuda()).cpu()
    hit = got[1, 0]
    assert bool(torch.isnan(hit[NAN_SUMS]).all()), hit
    assert bool(torch.isfinite(hit[FINITE_SUMS]).all()), hit
    e = err(got, *want[True])
    e[1, 0, NAN_SUMS] = 0.0
    print("eval_moments %s with NaN: worst finite error %.3g (bound %.3g)" % (shapes[0], np.nanmax(e), BOUND))
    assert np.isfinite(e).all() and e.max() <= BOUND


@pytest.mark.parametrize("shapes", (SCALAR, VEC), ids=("scalar", "float4"))
def test_masked_family_all_valid(shapes):
    from climate_learn import _hip
    pred, target, lat, clim, want = case(shapes)
    H, W = pred.shape[2:]
    p, t, lw, cl = pred.cuda(), target.cuda(), lat.cuda(), clim.cuda()
    plain, masked = _hip.eval_moments(p, t, lw, cl), _hip.masked_moments(p, t, lw, cl, mask=None)
    assert masked.shape == pred.shape[:2] + (13,)
    assert bool((masked[..., 12] == float(H * W)).all())
    e = np.abs(masked[..., :12].cpu().numpy() - plain.cpu().numpy()) / want[True][1]
    print("masked_moments(mask=None) against eval_moments %s: %.3g (bound %.3g)" % (shapes[0], e.max(), BOUND))
    assert e.max() <= BOUND


def test_eval_moments_checks_its_operands():
    """a target of another [B,C] or a smaller one used to be launched and read out of bounds"""
    from climate_learn import _hip
    pred, target, lat, clim, _ = case(SCALAR)
    p, t, lw, cl = pred.cuda(), target.cuda(), lat.cuda(), clim.cuda()
    bad = {"wrong [B,C]": dict(target=t[:, :2].contiguous()), "smaller target": dict(target=t[:, :, :10].contiguous()),
           "short lat_w": dict(lat_w=lw[:4].contiguous()), "mis-sized clim": dict(clim=cl[:, :, :30].contiguous())}
    for what, kw in bad.items():
        args = dict(target=t, lat_w=lw, clim=cl)
        args.update(kw)
        with pytest.raises(_hip.HipBackendError) as ei:
            _hip.eval_moments(p, **args)
        assert "failed with code" not in str(ei.value), (what, str(ei.value))      # refused in Python: nothing was launched
