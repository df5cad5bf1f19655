"""Extreme-value scores on the device (csrc/extremes.hip through orbit2_masked_loss_fwd at ORBIT2_MASKED_QUANTILES / _TAIL;
metrics.functional.field_quantiles, quantile_bias, tail_rmse / tail_mae / tail_bias, exceedance_scores; the tail_rmse,
lat_tail_rmse and quantile_bias registry names; utils.visualize.extreme_scores; the inference driver) against
tests/extremes_ref.py, the numpy yardstick.

Order statistics are compared exactly (as floats: the sign of a zero is free), counts exactly, the linear quantile to 1 fp32 ulp
of float32(np.quantile(float64)) -- the brackets are exact and the interpolation is done in double, so only the last rounding can
differ -- and the tail sums to rtol 2e-5 / atol 2e-6, the tolerance the project's score reductions are held to
(tests/test_masked_gpu.py).  Shapes are the smallest that reach each path: one pixel; one partial four-pixel item; a cropped
target on the float4 path; an odd width in a view offset by one element (scalar lanes, nothing aligned); a plane of more than 64
workgroups' worth of pixels (the grid-stride second trip)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import extremes_ref as R
from tests._child import free_port
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-6
LEVELS = R.LEVELS
SHAPES = {                                            # name: (pred shape, target spatial size, offset view)
    "one": ((1, 1, 1, 1), (1, 1), False),
    "seven": ((1, 1, 1, 7), (1, 7), False),
    "crop_vec": ((2, 3, 24, 40), (26, 44), False),
    "odd_view": ((1, 2, 37, 131), (37, 131), True),
    "two_trips": ((1, 1, 300, 512), (300, 512), False),
}


def _dev(a, offset_view=False):
    """a contiguous fp32 device tensor of the array; offset_view: a view one element into a larger buffer (4-byte aligned only)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset_view:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def make_pair(shape_name, value_set, seed=0):
    """numpy (pred, target, crop of the target): both fields of the named value set; outside the crop the target holds huge
    finite values that would show in every quantile if they were read"""
    shape, (Ht, Wt), _ = SHAPES[shape_name]
    B, C, H, W = shape
    n = B * C * H * W
    pred = R.values(value_set, n, seed + 1).reshape(shape)
    crop = R.values(value_set, n, seed + 2).reshape(shape)
    target = np.full((B, C, Ht, Wt), 3e38, dtype=np.float32)
    target[:, :, :H, :W] = crop
    return pred, target, crop


def levels_dev(levels=LEVELS):
    return torch.tensor(levels, dtype=torch.float32, device="cuda")


def check_quantiles(got, cnt, want, want_cnt, tag):
    got, cnt = got.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(cnt, want_cnt), tag
    w32 = want.astype(np.float32)
    np.testing.assert_array_equal(got[..., 1:], w32[..., 1:], err_msg=str(tag))          # the brackets: data values (NaN = NaN)
    fin = np.isfinite(w32[..., 0])
    assert np.array_equal(np.isnan(got[..., 0]), np.isnan(w32[..., 0])), tag
    worst = int(R.ulp_distance(got[..., 0][fin], w32[..., 0][fin]).max()) if fin.any() else 0
    assert worst <= 1, (tag, worst)
    # q = 0 / q = 1 (the first and last of LEVELS): the minimum in the value and the lower bracket, the maximum in all three
    # slots, bit for bit up to the sign of a zero
    for j, col, slots in ((0, 1, (0, 1)), (-1, 2, (0, 1, 2))):
        ext = w32[:, :, j, col]
        for slot in slots:
            g = got[:, :, j, slot]
            np.testing.assert_array_equal(g, ext, err_msg=str(tag))
            nz = np.isfinite(ext) & (ext != 0)
            assert np.array_equal(g.view(np.uint32)[nz], ext.view(np.uint32)[nz]), tag


# ---- quantiles: every shape x every value set, pooled and per image ------------------------------------------------------------
@pytest.mark.parametrize("per_image", [False, True], ids=["pooled", "per_image"])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_quantiles_equal_sorted_order_statistics(shape_name, per_image):
    from climate_learn import _hip
    view = SHAPES[shape_name][2]
    lv = levels_dev()
    for k, value_set in enumerate(R.VALUE_SETS):
        pred, target, crop = make_pair(shape_name, value_set, seed=10 * k)
        want, want_cnt = R.grouped_quantiles(pred, crop, LEVELS, per_image=per_image)
        p, t = _dev(pred, view), _dev(target, view)
        got, cnt = _hip.masked_quantiles(p, t, lv, per_image=per_image)
        check_quantiles(got, cnt, want, want_cnt, (shape_name, value_set, per_image))
        again, cnt2 = _hip.masked_quantiles(p, t, lv, per_image=per_image)              # integers only: the same bits
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(cnt, cnt2)


@pytest.mark.parametrize("per_image", [False, True], ids=["pooled", "per_image"])
@pytest.mark.parametrize("shape_name", ["crop_vec", "odd_view"])
def test_quantiles_over_holes_and_a_broadcast_mask(shape_name, per_image):
    """NaN / Inf holes in the target, a broadcast [H,W] mask, a NaN in a valid pred pixel's neighbourhood that must not be read,
    and one channel wholly invalid: NaN rows and a count of 0 for it"""
    from climate_learn import _hip
    from climate_learn.metrics.functional import _mask_operand
    view = SHAPES[shape_name][2]
    pred, target, crop = make_pair(shape_name, "gauss280", seed=7)
    B, C, H, W = pred.shape
    r = np.random.default_rng(11)
    for arr in (target, crop):
        arr[0, 0, 2:7, 2:9] = np.nan
        arr[0, 0, 3, 5], arr[0, 0, 4, 6] = np.inf, -np.inf
        arr[B - 1, 0, H - 1, W - 6:W] = np.inf
        arr[:, C - 1, :H, :W] = np.nan                                  # a channel without data, in every image
    pred[0, 0, 2:7, 2:9] = np.nan                                       # invalid pixels: never read
    mask = (r.random((H, W)) < 0.75)
    mask[0, 0] = mask[H - 1, W - 1] = False
    want, want_cnt = R.grouped_quantiles(pred, crop, LEVELS, mask=mask, per_image=per_image)
    p, t = _dev(pred, view), _dev(target, view)
    m, pitch, sb, sc = _mask_operand(torch.from_numpy(mask).cuda(), p, t)
    assert (pitch, sb, sc) == (W, 0, 0)
    got, cnt = _hip.masked_quantiles(p, t, levels_dev(), m, (pitch, sb, sc), per_image=per_image)
    check_quantiles(got, cnt, want, want_cnt, (shape_name, per_image))
    dead = [g for g in range(len(want_cnt)) if want_cnt[g] == 0]
    assert dead and all(torch.isnan(got[:, g]).all() and int(cnt[g]) == 0 for g in dead)
    assert want_cnt.sum() > 0 and torch.isfinite(got[0, 0]).all()


def test_one_field_twice_and_a_single_level():
    from climate_learn import _hip
    pred, target, crop = make_pair("crop_vec", "zero_inflated", seed=3)
    t = _dev(crop)
    got, cnt = _hip.masked_quantiles(t, t, levels_dev())
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))             # pred is target: identical rows
    want, want_cnt = R.grouped_quantiles(crop, crop, LEVELS)
    check_quantiles(got, cnt, want, want_cnt, "pred is target")
    one, _ = _hip.masked_quantiles(t, t, levels_dev((0.9772,)))                        # Q = 1; eight levels above are Q = 7
    assert torch.equal(one[:, :, 0].view(torch.int32), got[:, :, LEVELS.index(0.9772)].view(torch.int32))
    eight, _ = _hip.masked_quantiles(t, t, levels_dev(LEVELS + (0.25,)))               # Q = 8
    assert torch.equal(eight[:, :, :7].view(torch.int32), got.view(torch.int32))


def test_plain_kinds_keep_their_bits_around_a_quantile_call():
    from climate_learn import _hip
    pred, target, _ = make_pair("crop_vec", "gauss0", seed=5)
    target[0, 1, 3:9, 5:11] = np.nan
    p, t = _dev(pred), _dev(target)
    lat = torch.linspace(0.5, 1.5, pred.shape[2], device="cuda")
    cw = torch.tensor([1.0, 10.0, 10.0], device="cuda")
    before = [_hip.masked_loss_fwd(p, t, lat, cw, kind) for kind in (0, 1)]
    _hip.masked_quantiles(p, t, levels_dev())
    _hip.masked_tail(p, t, torch.zeros(3, 2, device="cuda"))
    after = [_hip.masked_loss_fwd(p, t, lat, cw, kind) for kind in (0, 1)]
    for (o0, c0), (o1, c1) in zip(before, after):
        assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)) and torch.equal(c0, c1)
        assert int(c0[-1]) == pred.size - 36 and torch.isfinite(o0).all()


# ---- the tail --------------------------------------------------------------------------------------------------------------------
def lat_weights(H):
    w = np.cos(np.deg2rad(np.linspace(-80.0, 80.0, H)))
    return (w / w.mean()).astype(np.float32)


def tail_pair(shape_name, value_set, seed=0):
    """as make_pair, with the prediction the target plus a bias and noise: every sum is well conditioned"""
    pred, target, crop = make_pair(shape_name, value_set, seed)
    r = np.random.default_rng(seed + 40)
    pred = (crop + 0.3 + 0.5 * r.standard_normal(crop.shape)).astype(np.float32)
    if value_set in ("two_valued", "zero_inflated"):                    # keep ties between the fields: a third of pred is target
        keep = r.random(crop.shape) < 0.33
        pred[keep] = crop[keep]
    return pred, target, crop


def thresholds_of(crop, T, per_image, lower):
    """[G,T] float32: data values of each group (ties with the threshold exist); with T > 1 the last one lies beyond every value"""
    B, C = crop.shape[:2]
    groups = [crop[b, c] for b in range(B) for c in range(C)] if per_image else [crop[:, c] for c in range(C)]
    thr = np.empty((len(groups), T), dtype=np.float32)
    for g, x in enumerate(groups):
        s = np.sort(x.ravel())
        picks = s[np.linspace(0, s.size - 1, T).astype(int)] if T > 1 else s[[s.size // 2]]
        if T > 1:
            picks[-1] = -np.inf if lower else np.inf                    # an empty tail
        thr[g] = picks
    return thr


def check_tail(got_s, got_n, want_s, want_n, tag):
    assert np.array_equal(got_n.cpu().numpy(), want_n), tag
    np.testing.assert_allclose(got_s.cpu().numpy().astype(np.float64), want_s, rtol=RTOL, atol=ATOL, err_msg=str(tag))


@pytest.mark.parametrize("lower", [False, True], ids=["upper", "lower"])
@pytest.mark.parametrize("shape_name,value_set,T,per_image,with_lat", [
    ("crop_vec", "gauss280", 8, False, True), ("crop_vec", "zero_inflated", 8, True, False), ("crop_vec", "two_valued", 1, False, False),
    ("odd_view", "gauss0", 8, True, True), ("odd_view", "zero_inflated", 3, False, False),
    ("two_trips", "gauss280", 8, False, True), ("seven", "sign_mix", 2, False, False), ("one", "constant", 1, True, True)])
def test_tail_sums_and_counts(shape_name, value_set, T, per_image, with_lat, lower):
    from climate_learn import _hip
    view = SHAPES[shape_name][2]
    pred, target, crop = tail_pair(shape_name, value_set, seed=T)
    H = pred.shape[2]
    thr = thresholds_of(crop, T, per_image, lower)
    lat = lat_weights(H) if with_lat else None
    want_s, want_n = R.tail(pred, crop, thr, lat, None, lower, per_image)
    p, t = _dev(pred, view), _dev(target, view)
    args = (p, t, torch.from_numpy(thr).cuda(), None if lat is None else torch.from_numpy(lat).cuda())
    got_s, got_n = _hip.masked_tail(*args, lower=lower, per_image=per_image)
    tag = (shape_name, value_set, T, per_image, with_lat, lower)
    check_tail(got_s, got_n, want_s, want_n, tag)
    first = want_n[:, :, 0, 0] if per_image else want_n[:, :, 0, 0].sum(0)            # a data value of the group as threshold:
    assert (first > 0).all(), tag                                                     # its ties are in the tail
    if T > 1:                                                                         # beyond every value: nothing
        assert not want_n[:, :, -1, :3].any() and not want_s[:, :, -1].any() and not got_s[:, :, -1].any()
    assert (got_n[..., 3] == int(want_n[0, 0, 0, 3])).all()
    s2, n2 = _hip.masked_tail(*args, lower=lower, per_image=per_image)                # fixed-order sums: the same bits
    assert torch.equal(got_s.view(torch.int32), s2.view(torch.int32)) and torch.equal(got_n, n2)


def test_tail_over_holes_and_a_mask():
    from climate_learn import _hip
    from climate_learn.metrics.functional import _mask_operand
    pred, target, crop = tail_pair("crop_vec", "gauss280", seed=9)
    B, C, H, W = pred.shape
    for arr in (target, crop):
        arr[0, 0, 2:7, 2:9] = np.nan
        arr[1, 1, :H, :W] = np.nan
    pred[0, 0, 2:7, 2:9] = np.nan
    mask = np.random.default_rng(2).random((B, 1, H, W)) < 0.8
    thr = thresholds_of(np.where(np.isfinite(crop), crop, 280.0).astype(np.float32), 4, False, False)
    want_s, want_n = R.tail(pred, crop, thr, lat_weights(H), mask, False, False)
    p, t = _dev(pred), _dev(target)
    m, pitch, sb, sc = _mask_operand(torch.from_numpy(mask).cuda(), p, t)
    got_s, got_n = _hip.masked_tail(p, t, torch.from_numpy(thr).cuda(), torch.from_numpy(lat_weights(H)).cuda(), m, (pitch, sb, sc))
    check_tail(got_s, got_n, want_s, want_n, "holes")
    assert not got_n[1, 1].any() and not got_s[1, 1].any() and torch.isfinite(got_s).all()


# ---- functionals, registry names, extreme_scores ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored():
    """the (2,3,24,40) case against its (26,44) target with a few NaN targets, and its yardstick pieces, computed once"""
    pred, target, crop = tail_pair("crop_vec", "gauss280", seed=21)
    for arr in (target, crop):
        arr[1, 2, 5:8, 10:20] = np.nan
    return dict(pred=pred, target=target, crop=crop, p=_dev(pred), t=_dev(target), lat=lat_weights(pred.shape[2]))


def _want_tail(s, q, lower, lat=None, thr=None):
    """per channel (sums [C,4], counts [C,4]) over the batch beyond the float32 pooled target quantile at q, from the yardstick"""
    if thr is None:
        thr = R.grouped_quantiles(s["crop"], s["crop"], (q,))[0][0, :, :, 0].astype(np.float32)
    ws, wn = R.tail(s["pred"], s["crop"], thr, lat, None, lower, False)
    return ws.sum(0)[:, 0], wn.sum(0)[:, 0]


def _ulp(x):
    """one fp32 unit in the last place at the largest magnitude of x"""
    return float(np.spacing(np.float32(np.nanmax(np.abs(x)))))


def _close(got, want):
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), want, rtol=RTOL, atol=ATOL)


def test_functionals_against_the_yardstick(scored):
    from climate_learn.metrics import functional as fn
    s = scored
    q3 = fn.SIGMA_LEVELS
    want_q, _ = R.grouped_quantiles(s["pred"], s["crop"], q3)
    got = fn.field_quantiles(s["p"], q3)                                 # the prediction's own quantiles: every pixel is finite
    full, _ = R.grouped_quantiles(s["pred"], s["pred"], q3)
    assert tuple(got.shape) == (3, 3) and int(R.ulp_distance(got.cpu().numpy(), full[1, :, :, 0].astype(np.float32)).max()) <= 1
    img = fn.field_quantiles(s["t"][:, :, :24, :40], (0.5,), per_image=True)
    want_img, _ = R.grouped_quantiles(s["crop"], s["crop"], (0.5,), per_image=True)
    assert tuple(img.shape) == (6, 1) and int(R.ulp_distance(img.cpu().numpy(), want_img[0, :, :, 0].astype(np.float32)).max()) <= 1
    qb = fn.quantile_bias(s["p"], s["t"], q3)
    per = want_q[1, :, :, 0] - want_q[0, :, :, 0]
    np.testing.assert_allclose(qb.cpu().numpy().astype(np.float64), np.concatenate((per, per.mean(0, keepdims=True))), rtol=0,
                               atol=2 * _ulp(want_q[..., 0]))             # the difference of two fp32 quantiles, each to 1 ulp
    for lower, q in ((False, 0.9772), (True, 0.05)):
        ws, wn = _want_tail(s, q, lower, s["lat"])
        per = np.sqrt(ws[:, 1] / ws[:, 0])
        _close(fn.tail_rmse(s["p"], s["t"], q, lower, lat_weights=torch.from_numpy(s["lat"])), np.append(per, per.mean()))
        ws, wn = _want_tail(s, q, lower)
        per = ws[:, 2] / ws[:, 0]
        _close(fn.tail_mae(s["p"], s["t"], q, lower), np.append(per, per.mean()))
        per = ws[:, 3] / wn[:, 0]
        _close(fn.tail_bias(s["p"], s["t"], q, lower), np.append(per, per.mean()))
        h, f, ms = wn[:, 1].astype(float), wn[:, 2].astype(float), (wn[:, 0] - wn[:, 1]).astype(float)
        ex = fn.exceedance_scores(s["p"], s["t"], q, lower)
        for k, want in (("csi", h / (h + ms + f)), ("pod", h / (h + ms)), ("far", f / (h + f)), ("frequency_bias", (h + f) / (h + ms))):
            _close(ex[k], want)
    # explicit thresholds; one beyond every value: zero counts, zero sums, NaN from the functional
    thr = np.array([[279.0], [283.5], [1e6]], dtype=np.float32)
    ws, wn = _want_tail(s, None, False, thr=thr)
    got = fn.tail_rmse(s["p"], s["t"], thresholds=torch.from_numpy(thr[:, 0]))
    _close(got[:2], np.sqrt(ws[:2, 1] / ws[:2, 0]))
    assert wn[2, 0] == 0 and torch.isnan(got[2]) and torch.isnan(got[3])
    assert torch.isnan(fn.exceedance_scores(s["p"], s["t"], thresholds=torch.from_numpy(thr[:, 0]))["pod"][2])
    # q = 0 is the whole field: the masked mean squared error of the channel over the valid pixels
    ws, wn = _want_tail(s, 0.0, False)
    v = np.isfinite(s["crop"])
    d2 = np.where(v, (s["pred"].astype(np.float64) - s["crop"]) ** 2, 0.0)
    np.testing.assert_allclose(ws[:, 1] / ws[:, 0], d2.sum((0, 2, 3)) / v.sum((0, 2, 3)), rtol=1e-12)
    _close(fn.tail_rmse(s["p"], s["t"], 0.0)[:3], np.sqrt(d2.sum((0, 2, 3)) / v.sum((0, 2, 3))))


def test_registered_metrics_and_extreme_scores(scored):
    import climate_learn as cl
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.utils import MetricsMetaInfo
    from climate_learn.utils.visualize import extreme_scores
    s = scored
    lat_deg = np.linspace(-80.0, 80.0, 24)
    meta = MetricsMetaInfo(["a", "b", "c"], ["a", "b", "c"], lat_deg, np.arange(40), None)
    ws, _ = _want_tail(s, 0.9772, False)
    per = np.sqrt(ws[:, 1] / ws[:, 0])
    _close(cl.load_loss("cuda", None, "tail_rmse", False, meta)(s["p"], s["t"]), np.append(per, per.mean()))
    ws, _ = _want_tail(s, 0.9772, False, s["lat"])
    per = np.sqrt(ws[:, 1] / ws[:, 0])
    _close(cl.load_loss("cuda", None, "lat_tail_rmse", False, meta)(s["p"], s["t"]), np.append(per, per.mean()))
    want_q, _ = R.grouped_quantiles(s["pred"], s["crop"], (0.8413,))
    per = want_q[1, :, 0, 0] - want_q[0, :, 0, 0]
    got = cl.load_loss("cuda", None, "quantile_bias", False, meta).set_level(0.8413)(s["p"], s["t"])
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), np.append(per, per.mean()), rtol=0, atol=2 * _ulp(want_q[..., 0]))
    res = extreme_scores(s["p"], s["t"], ["a", "b", "c"], lat_weights=torch.from_numpy(s["lat"]))
    for side, lower in (("upper", False), ("lower", True)):
        for j, q0 in enumerate(fn.SIGMA_LEVELS):
            q = float(np.float32(1.0 - q0)) if lower else q0
            wq, _ = R.grouped_quantiles(s["pred"], s["crop"], (q,))
            ws, wn = _want_tail(s, q, lower, s["lat"])
            h, f, ms = wn[:, 1].astype(float), wn[:, 2].astype(float), (wn[:, 0] - wn[:, 1]).astype(float)
            for c, v in enumerate("abc"):
                row = res[v][side][j]
                want = {"target_quantile": wq[0, c, 0, 0], "pred_quantile": wq[1, c, 0, 0], "quantile_bias": wq[1, c, 0, 0] - wq[0, c, 0, 0],
                        "tail_rmse": np.sqrt(ws[c, 1] / ws[c, 0]), "tail_bias": ws[c, 3] / wn[c, 0], "csi": h[c] / (h[c] + ms[c] + f[c]),
                        "frequency_bias": (h[c] + f[c]) / (h[c] + ms[c])}
                assert row["level"] == pytest.approx(q, abs=1e-7)
                ulp = _ulp(wq[..., 0])                                   # a quantile to 1 fp32 ulp, their difference to 2
                for k, w in want.items():
                    tol = dict(rtol=0, atol=(2 if k == "quantile_bias" else 1) * ulp) if "quantile" in k else dict(rtol=RTOL, atol=ATOL)
                    np.testing.assert_allclose(row[k], w, err_msg="%s %s %d %s" % (v, side, j, k), **tol)


# ---- the inference driver --------------------------------------------------------------------------------------------------------
def test_inference_driver_extreme_scores(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_extremes.yaml")))
    conf["extreme_scores"] = {"levels": [0.0, 0.9772]}
    conf["model"].update(embed_dim=256, depth=2, decoder_depth=1, num_heads=4)
    conf["data"]["synthetic"]["ERA5_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256])
    cfg = os.path.join(tmp_path, "inf.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    env = dict(os.environ, MASTER_PORT=str(free_port()))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "visualize.py"), cfg],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    out_vars = conf["data"]["dict_out_variables"]["ERA5_1"]
    got = [ln for ln in lines if ln.startswith("extreme_scores ")]
    assert [ln.split()[1] for ln in got] == out_vars
    rmse = [ln for ln in lines if ln.startswith("rmse [")]
    assert len(rmse) == 1
    rmse = [float(v) for v in re.findall(r"[-+.\dinfae]+", rmse[0][len("rmse ["):])]
    num = r"([-+.\dinfae]+)"
    for c, ln in enumerate(got):
        body = ln.split(" ", 2)[2]
        assert body.startswith("{'upper': [{") and "'lower': [{" in body
        rows = re.findall(r"\{'level': %s, 'target_quantile': %s, 'pred_quantile': %s, 'quantile_bias': %s, 'tail_rmse': %s, "
                          r"'tail_bias': %s, 'csi': %s, 'frequency_bias': %s\}" % ((num,) * 8), body)
        assert len(rows) == 4                                                       # two levels, upper and lower
        assert [float(row[0]) for row in rows] == pytest.approx([0.0, 0.9772, 1.0, 0.0228], abs=1e-6)
        # level 0, upper tail (and level 1, lower): the whole field -- the driver's own rmse of that variable
        for row in (rows[0], rows[2]):
            np.testing.assert_allclose(float(row[4]), rmse[c], rtol=RTOL, atol=ATOL)
