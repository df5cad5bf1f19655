"""SSIM / PSNR on the device (orbit2_ssim, _hip.ssim_sums, metrics.functional.ssim / psnr, utils.visualize.stitched_scores)
against a float64 oracle: a direct window-by-window evaluation of the published definition with scikit-image's defaults, the
restatement tests/test_inference_cpu.py checks psnr_ssim with (here over numpy's sliding windows instead of two Python loops).

Tolerances: the fp32 emulation of the kernel's own summation order (tests/test_ssim_cpu.py) is off from float64
by at most 2.05e-6 per pixel and 3.3e-8 in an image's mean over the fields of this file at offsets 0 and 280; a factor 4 for the
GPU's fused multiply-adds and its reduction order gives MAP_TOL and MEAN_TOL.  An uncentred fp32 kernel is off by 4.8e-1 per
pixel at offset 280 and cannot pass."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-5          # per pixel of the map, absolute: 4 x 2.05e-6 = 8.2e-6, rounded up
MEAN_TOL = 1.4e-7       # per-image mean, absolute: 4 x 3.3e-8 = 1.32e-7, rounded up (images of more than one window)
# sum of (pred - target)^2, relative: the difference is rounded once (its square carries 2 x 2^-24), a thread adds at most 11
# terms by fma, the wave tree 6 levels, then doubles -- fewer than 21 roundings of 2^-24 on a sum of non-negative terms
SE_RTOL = 21 * 2.0 ** -24


def make_fields(shape, target_shape=None, offset=0.0, seed=0):
    """fp32 (pred, target): the target a smooth field of range about 5 plus noise, at `offset`; the prediction is the target's
    crop plus noise of another size in every image"""
    target_shape = target_shape or shape
    rng = np.random.default_rng(seed)
    B, C, Ht, Wt = target_shape
    yy, xx = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    target = np.empty(target_shape)
    for i in range(B * C):
        ph = rng.uniform(0, 2 * np.pi, 3)
        smooth = 1.5 * np.sin(yy / 7.0 + ph[0]) + np.cos(xx / 11.0 + ph[1]) + 0.5 * np.sin((xx + yy) / 5.0 + ph[2])
        target[i // C, i % C] = smooth + 0.05 * rng.standard_normal((Ht, Wt))
    target = (target + offset).astype(np.float32)
    noise = rng.standard_normal(shape) * (0.05 + 0.1 * np.arange(B * C).reshape(B, C, 1, 1))
    pred = (target[:, :, : shape[2], : shape[3]].astype(np.float64) + noise).astype(np.float32)
    return pred, target


def ssim_oracle(pred, target, lat_w=None, data_range=None):
    """float64: (sums [B,C,6], map [B,C,H-6,W-6]) of include/orbit2_hip.h:orbit2_ssim; `target` may be larger (top-left crop)"""
    from numpy.lib.stride_tricks import sliding_window_view
    pred = np.asarray(pred, dtype=np.float64)
    B, C, H, W = pred.shape
    target = np.asarray(target, dtype=np.float64)[:, :, :H, :W]
    w = np.ones(H) if lat_w is None else np.asarray(lat_w, dtype=np.float64)[:H]
    sums, smap = np.zeros((B, C, 6)), np.zeros((B, C, H - 6, W - 6))
    for b in range(B):
        for c in range(C):
            x, y = pred[b, c], target[b, c]
            R = float(y.max() - y.min()) if data_range is None else float(np.broadcast_to(data_range, (B, C))[b, c])
            c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
            wx = sliding_window_view(x, (7, 7)).reshape(H - 6, W - 6, 49)
            wy = sliding_window_view(y, (7, 7)).reshape(H - 6, W - 6, 49)
            mx, my = wx.mean(-1), wy.mean(-1)
            dx, dy = wx - mx[..., None], wy - my[..., None]
            vx, vy, vxy = (dx * dx).sum(-1) / 48, (dy * dy).sum(-1) / 48, (dx * dy).sum(-1) / 48
            with np.errstate(invalid="ignore", divide="ignore"):
                s = (2 * mx * my + c1) * (2 * vxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
            smap[b, c] = s
            sums[b, c] = (s.sum(), (w[3:H - 3, None] * s).sum(), ((x - y) ** 2).sum(), y.min(), y.max(), R)
    return sums, smap


LAT = np.cos(np.deg2rad(np.linspace(-80, 75, 39))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch_case(offset):
    """the (2,3,39,71) prediction against a (2,3,41,72) target, its oracle with a non-trivial lat_w: computed once"""
    pred, target = make_fields((2, 3, 39, 71), (2, 3, 41, 72), offset, seed=11)
    return pred, target, ssim_oracle(pred, target, LAT)


def _run(pred, target, lat_w=None, data_range=None):
    from climate_learn import _hip
    lw = None if lat_w is None else torch.from_numpy(np.asarray(lat_w, dtype=np.float32)).cuda()
    sums, smap = _hip.ssim_sums(torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda(), lw, data_range, ssim_map=True)
    return sums.cpu().numpy(), smap.cpu().numpy().astype(np.float64)


def _check(got, want, n_centres, what, lat=None, mean_tol=MEAN_TOL):
    """sums and map of a call against the oracle's; prints each figure before it asserts"""
    (gs, gm), (ws, wm) = got, want
    e_map = float(np.abs(gm - wm).max())
    e_mean = float(np.abs(gs[..., :2] - ws[..., :2]).max() / n_centres)
    e_se = float((np.abs(gs[..., 2] - ws[..., 2]) / np.maximum(ws[..., 2], 1e-300)).max())
    print("%s: map %.3g (tol %.3g), sums 0..1 per centre %.3g (tol %.3g), squared error rel %.3g (tol %.3g)"
          % (what, e_map, MAP_TOL, e_mean, mean_tol, e_se, SE_RTOL))
    assert gm.shape == wm.shape
    assert e_map <= MAP_TOL, what
    assert e_mean <= mean_tol * (1.0 if lat is None else max(1.0, float(np.abs(lat).max()))), what          # sum 1 carries the weights
    assert e_se <= SE_RTOL, what
    assert np.array_equal(gs[..., 3:], ws[..., 3:]), what          # min and max are selections, the range their difference


def test_exactly_one_window():
    pred, target = make_fields((1, 1, 7, 7), offset=280.0, seed=1)
    got, want = _run(pred, target), ssim_oracle(pred, target)
    assert got[1].shape == (1, 1, 1, 1)
    _check(got, want, 1, "7 x 7", mean_tol=MAP_TOL)                  # the mean of one pixel is that pixel
    assert abs(got[0][0, 0, 0] - got[1][0, 0, 0, 0]) < 1e-7          # the one value is the sum


@pytest.mark.parametrize("shape", [(1, 1, 9, 150), (1, 1, 150, 9)])
def test_thin_bands_many_tiles_along_one_axis(shape):
    pred, target = make_fields(shape, offset=280.0, seed=2)
    lat = np.linspace(0.5, 1.5, shape[2]).astype(np.float32)
    _check(_run(pred, target, lat), ssim_oracle(pred, target, lat), (shape[2] - 6) * (shape[3] - 6), str(shape), lat)


@pytest.mark.parametrize("offset", [0.0, 280.0])
def test_batch_with_cropped_target_per_pixel(offset):
    """several tiles in both directions with ragged tails, the target a top-left crop with its own pitch, B * C > 1, a
    non-trivial lat_w; at offset 280 an uncentred fp32 kernel is off by 1e-1 per pixel (tests/test_ssim_cpu.py)"""
    pred, target, want = _batch_case(offset)
    _check(_run(pred, target, LAT), want, 33 * 65, "batch at offset %g" % offset)


def test_tile_seams():
    """the tile edge on the image edge (one tile exactly, 2 x 2 tiles exactly) and one centre more than that in each direction"""
    from climate_learn import _hip
    th, tw = _hip.SSIM_TILE
    assert (th, tw) == (32, 64)
    for ny, nx, extra in ((1, 1, 0), (1, 1, 1), (2, 2, 0), (2, 2, 1)):
        shape = (1, 1, ny * th + 6 + extra, nx * tw + 6 + extra)
        pred, target = make_fields(shape, offset=280.0, seed=3 + extra)
        lat = np.linspace(0.5, 1.5, shape[2]).astype(np.float32)
        _check(_run(pred, target, lat), ssim_oracle(pred, target, lat), (shape[2] - 6) * (shape[3] - 6), str(shape), lat)


def test_given_data_range_is_used_and_echoed():
    pred, target, _ = _batch_case(280.0)
    got = _run(pred, target, LAT, 8.0)
    want = ssim_oracle(pred, target, LAT, 8.0)
    _check(got, want, 33 * 65, "data_range 8")
    assert np.all(got[0][..., 5] == 8.0)
    per_image = np.linspace(4.0, 9.0, 6).astype(np.float32).reshape(2, 3)
    got = _run(pred, target, LAT, torch.from_numpy(per_image))
    _check(got, ssim_oracle(pred, target, LAT, per_image), 33 * 65, "data_range per image")


def test_constant_target_image_scores_nan_and_leaves_the_others_alone():
    """range 0 is not special-cased: image (1, 0), constant in target and prediction, is 0 / 0 at every window"""
    pred, target, want = _batch_case(280.0)
    pred, target = pred.copy(), target.copy()
    pred[1, 0], target[1, 0] = 280.0, 280.0
    (gs, gm), (ws, wm) = _run(pred, target, LAT), ssim_oracle(pred, target, LAT)
    assert np.isnan(ws[1, 0, :2]).all() and np.isnan(gs[1, 0, :2]).all() and np.isnan(gm[1, 0]).all()
    assert gs[1, 0, 2] == 0.0 and tuple(gs[1, 0, 3:]) == (280.0, 280.0, 0.0)
    keep = np.ones((2, 3), dtype=bool)
    keep[1, 0] = False
    _check((gs[keep][None], gm[keep][None]), (want[0][keep][None], want[1][keep][None]), 33 * 65, "beside a constant image")


def test_identical_fields_score_one_and_infinite_psnr():
    from climate_learn.metrics import functional as fn
    _, target, _ = _batch_case(280.0)
    t = torch.from_numpy(target).cuda()
    s = fn.ssim(t, t).cpu().numpy()
    assert s.shape == (4,) and np.abs(s - 1.0).max() <= MEAN_TOL + 2.0 ** -23          # (the metric is returned in fp32)
    assert torch.isinf(fn.psnr(t, t)).all() and (fn.psnr(t, t) > 0).all()


def _raw(pred, target, lat, rng, sums, smap, B, C, H, W, Ht=None, Wt=None):
    from climate_learn import _hip
    p = lambda t: None if t is None else t.data_ptr()
    return _hip.lib().orbit2_ssim(p(pred), p(target), H if Ht is None else Ht, W if Wt is None else Wt, p(lat), p(rng), p(sums),
                                  p(smap), B, C, H, W, torch.cuda.current_stream().cuda_stream)


def test_outputs_stay_inside_their_buffers():
    pred, target, want = _batch_case(280.0)
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    n_s, n_m, guard = 2 * 3 * 6, 2 * 3 * 33 * 65, 1024
    sums = torch.full((guard + n_s + guard,), -7.0, dtype=torch.float64, device="cuda")
    smap = torch.full((guard + n_m + guard,), -7.0, dtype=torch.float32, device="cuda")
    assert _raw(p, t, None, None, sums[guard:], smap[guard:], 2, 3, 39, 71, 41, 72) == 0
    torch.cuda.synchronize()
    for buf, n in ((sums, n_s), (smap, n_m)):
        assert (buf[:guard] == -7.0).all() and (buf[guard + n:] == -7.0).all()
    assert np.abs(smap[guard:guard + n_m].cpu().numpy().reshape(2, 3, 33, 65) - want[1]).max() <= MAP_TOL


def test_refusals():
    from climate_learn import _hip
    a = torch.zeros(1, 2, 8, 8, device="cuda")
    sums = torch.full((2, 6), -7.0, dtype=torch.float64, device="cuda")
    smap = torch.full((2, 2, 2), -7.0, device="cuda")
    for args in ((None, a, None, None, sums, smap, 1, 2, 8, 8), (a, None, None, None, sums, smap, 1, 2, 8, 8),
                 (a, a, None, None, None, smap, 1, 2, 8, 8), (a, a, None, None, sums, smap, 0, 2, 8, 8),
                 (a, a, None, None, sums, smap, 1, 0, 8, 8), (a, a, None, None, sums, smap, 1, 2, 6, 8),
                 (a, a, None, None, sums, smap, 1, 2, 8, 6), (a, a, None, None, sums, smap, 1, 2, 8, 8, 7, 8),
                 (a, a, None, None, sums, smap, 1, 2, 8, 8, 8, 7), (a, a, None, None, sums, smap, 256, 256, 8, 8)):
        assert _raw(*args) == -1
    torch.cuda.synchronize()
    assert (sums == -7.0).all() and (smap == -7.0).all()             # nothing was written
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.ssim_sums(a.cpu(), a)
    with pytest.raises(_hip.HipBackendError, match="must be torch.float32"):
        _hip.ssim_sums(a.double(), a)
    with pytest.raises(_hip.HipBackendError, match="smaller than the prediction"):
        _hip.ssim_sums(a, a[:, :, :7].contiguous())
    with pytest.raises(_hip.HipBackendError, match="lat_w has 4 entries"):
        _hip.ssim_sums(a, a, torch.ones(4, device="cuda"))
    with pytest.raises(_hip.HipBackendError, match="at least 7 x 7"):
        _hip.ssim_sums(a[:, :, :6].contiguous(), a)


def test_metric_agrees_with_the_host_psnr_ssim():
    """ties the device path to the restatement the project already pins (tests/test_inference_cpu.py)"""
    from climate_learn.metrics import functional as fn
    from climate_learn.utils.visualize import psnr_ssim
    pred, target = make_fields((1, 1, 40, 56), offset=280.0, seed=5)
    psnr, ssim = psnr_ssim(target[0, 0], pred[0, 0])
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
    s = _run(pred, target)[0]
    print("ssim %.9f host %.9f, psnr %.6f host %.6f" % (s[0, 0, 0] / (34 * 50), ssim, float(fn.psnr(p, t, True)), psnr))
    assert abs(s[0, 0, 0] / (34 * 50) - ssim) <= 1e-6
    assert abs(float(fn.ssim(p, t, aggregate_only=True)) - ssim) <= 1e-6
    assert abs(float(fn.psnr(p, t, aggregate_only=True)) - psnr) <= 1e-3
    assert fn.ssim(p, t).shape == (2,) and fn.psnr(p, t).shape == (2,)
    # a Normal is taken by its loc
    normal = torch.distributions.Normal(p, torch.ones_like(p))
    assert torch.equal(fn.ssim(normal, t), fn.ssim(p, t)) and torch.equal(fn.psnr(normal, t), fn.psnr(p, t))


def test_stitched_scores_equal_the_metrics_on_the_stitched_tensor():
    from oracle.harness import build_pair
    from climate_learn.metrics import functional as fn
    from climate_learn.utils.visualize import stitched_scores, tiled_predict
    model, sd, cfg, O, x, y, in_vars, out_vars = build_pair(D=128, depth=1, heads=2, grid=(16, 32), B=1, seed=7)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(2)
    X = torch.randn(1, len(in_vars), 32, 64, generator=g).cuda()
    Y = torch.randn(1, len(out_vars), 130, 260, generator=g).cuda()            # larger than the prediction: top-left crop
    st = tiled_predict(model, X, Y, in_vars, out_vars, 2, 4)
    lat = torch.linspace(0.5, 1.5, 128)
    got = stitched_scores(st, Y, out_vars, lat)
    want = {"psnr": fn.psnr(st, Y), "ssim": fn.ssim(st, Y), "lat_ssim": fn.ssim(st, Y, lat_weights=lat)}
    assert list(got) == list(out_vars)
    for c, v in enumerate(out_vars):
        assert set(got[v]) == {"psnr", "ssim", "lat_ssim"}
        for k in want:
            a, b = got[v][k], float(want[k][c])
            assert a == b or (np.isnan(a) and np.isnan(b)), (v, k, a, b)
    assert set(stitched_scores(st, Y, out_vars)[out_vars[0]]) == {"psnr", "ssim"}
