"""The bodies that tests/test_resample_gpu.py (plain modes) and tests/test_resample_aa_gpu.py (antialiased modes) share: the
forward and the moments check of one pair of sizes.  A caller hands over what differs: its input per offset, its float64 replica,
its bounds, its modes and the antialias flag.  Channels, affine pair, offsets and the target are resample_ref's for both."""
import numpy as np
import torch

from tests import resample_ref as R

GUARD = 64


def case_ids(cases):
    return ["%dx%d-%dx%d" % (hw + HW) for hw, HW in cases]


def affine(on):
    return (R.GPU_SCALE, R.GPU_SHIFT) if on else (None, None)


def dev(v):
    return None if v is None else torch.as_tensor(np.asarray(v, np.float32)).cuda()


def run_into_guards(x, HW, mode, scale, shift, lead, antialias):
    """_hip.resample into the middle of a NaN-filled buffer; returns the field and checks that nothing else was written"""
    from climate_learn import _hip
    n = x.shape[0] * len(R.GPU_CHANNELS) * HW[0] * HW[1]
    buf = torch.full((lead + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[lead:lead + n].view(x.shape[0], len(R.GPU_CHANNELS), *HW)
    got = _hip.resample(x, HW, mode, channels=R.GPU_CHANNELS, scale=dev(scale), shift=dev(shift), out=out, antialias=antialias)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[:lead]).all() and np.isnan(host[lead + n:]).all(), "wrote outside the output"
    field = host[lead:lead + n].reshape(out.shape)
    assert not np.isnan(field).any(), "left pixels unwritten"
    return field


def check_fwd(hw, HW, input_at, replica, field_tol, modes, antialias, bitwise=None):
    """every mode, both offsets, affine off and on, the output on a 16-byte boundary and off it.  field_tol(mode) bounds
    |kernel - replica| / max|x| and is 0 where the result must be exact; bitwise(got, xh, mode, off) holds a caller's own
    bit-for-bit assertions on an unscaled field"""
    worst = dict.fromkeys(modes, 0.0)
    for off in R.OFFSETS:
        xh = input_at(off)
        x = torch.from_numpy(xh).cuda()
        xmax = float(np.abs(xh[:, list(R.GPU_CHANNELS)]).max())
        for mode in modes:
            for aff in (False, True):
                scale, shift = affine(aff)
                rep = replica(xh, HW, mode, R.GPU_CHANNELS, scale, shift)
                for lead in (GUARD, GUARD - 3):              # the output on a 16-byte boundary, and off it
                    got = run_into_guards(x, HW, mode, scale, shift, lead, antialias)
                    err = np.abs(got.astype(np.float64) - rep)
                    tol = field_tol(mode) * xmax
                    if aff:
                        bound = np.abs(np.asarray(scale))[None, :, None, None] * tol + 2.0 ** -23 * np.abs(rep)
                    else:
                        bound = np.full_like(rep, tol)
                        worst[mode] = max(worst[mode], float(err.max()) / xmax)
                    print("%s %s offset %d affine %d lead %d: worst %.4g = %.3g ulp(max|x|), bound %.4g"
                          % (R.case_key(hw, HW), mode, off, aff, lead, err.max(), err.max() / xmax / R.ULP, bound.max()))
                    assert (err <= bound).all()
                    if not aff:
                        if tol == 0.0:
                            assert np.array_equal(got.astype(np.float64), rep)
                        if bitwise is not None:
                            bitwise(got, xh, mode, off)
    print("worst |kernel - replica| / max|x| in ulp:", {m: round(v / R.ULP, 3) for m, v in worst.items()})


def check_moments(hw, HW, input_at, replica, rtol, modes, antialias):
    """the twelve sums against the float64 sums of the replica field and against _hip.eval_moments(_hip.resample(...)): every
    mode, both offsets (the affine at offset 0), latitude weights and climatology off and on.  rtol(mode, off) bounds both"""
    from climate_learn import _hip
    worst = 0.0
    for off in R.OFFSETS:
        xh = input_at(off)
        th, lat, clim = R.gpu_target(HW, off)                 # a target larger than the field, NaN outside the crop
        x, t = torch.from_numpy(xh).cuda(), torch.from_numpy(th).cuda()
        for mode in modes:
            tol = rtol(mode, off)
            for aff in ((False, True) if off == 0 else (False,)):
                scale, shift = affine(aff)
                sc, sh = dev(scale), dev(shift)
                rep = replica(xh, HW, mode, R.GPU_CHANNELS, scale, shift)
                field = _hip.resample(x, HW, mode, channels=R.GPU_CHANNELS, scale=sc, shift=sh, antialias=antialias)
                for lw in (None, lat):
                    for cl in (None, clim):
                        got = _hip.resample_moments(x, HW, mode, t, channels=R.GPU_CHANNELS, scale=sc, shift=sh, lat_w=dev(lw),
                                                    clim=dev(cl), antialias=antialias).cpu().numpy()
                        two = _hip.eval_moments(field, t, dev(lw), dev(cl)).cpu().numpy()
                        want, mag = R.moments64(rep, th, lw, cl)
                        assert got.shape == want.shape == (2, 3, 12) and np.isfinite(got).all()
                        e1, e2 = float((np.abs(got - want) / mag).max()), float((np.abs(got - two) / mag).max())
                        worst = max(worst, e1 / tol)
                        print("%s %s offset %d affine %d lat %d clim %d: against float64 %.3g, against the two-step path %.3g "
                              "(bound %.3g)" % (R.case_key(hw, HW), mode, off, aff, lw is not None, cl is not None, e1, e2, tol))
                        assert e1 <= tol and e2 <= tol
    print("worst error of the twelve sums as a fraction of its bound: %.3g" % worst)
