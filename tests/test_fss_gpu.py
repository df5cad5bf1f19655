"""The fractions skill score on the device (csrc/fss.hip through orbit2_masked_loss_fwd at ORBIT2_FSS_KIND;
metrics.functional.fss / fss_profile; the fss registry name; utils.visualize.neighbourhood_scores; the inference driver) against
tests/fss_ref.py, the numpy yardstick.

The four integer sums are compared exactly.  The score is held to 1 fp32 ulp of float32(1 - c3 / (c1 + c2)) computed in double
from the yardstick's integers: the kernel does the same three double operations and rounds once, so only that last rounding can
differ; NaN where the yardstick is NaN.  Shapes are the smallest that reach each path: fewer columns than a word, one short of a
word, a whole word, one more; several words with a partial last one; and one plane of more than one strip and more than one band
of the window pass, its size taken from the partition the binding mirrors (_hip.fss_partition), never from a copied number."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import extremes_ref as E
from tests import fss_ref as R
from tests._child import free_port
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

B, C = 2, 3
VALUE_SETS = ("gauss0", "gauss280", "zero_inflated", "two_valued", "constant")
LEVEL_COUNTS = (1, 5, 8)


def partition_plane():
    """(H, W) of a plane that spans more than one band and more than one strip at every threshold count of the tests"""
    from climate_learn import _hip
    W = _hip.FSS_STRIP + 37
    H = _hip.FSS_BANDS[0] + 5
    for T in LEVEL_COUNTS:
        strip, band = _hip.fss_partition(B, C, H, W, T)
        assert W > strip and H > band
    return H, W


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


def make_pair(H, W, value_set, seed=0):
    """numpy (pred, target) [B,C,H,W]: the target of the named value set, the prediction the target moved by (1, 2) pixels plus
    noise -- events near the target's, rarely on them"""
    n = B * C * H * W
    target = E.values(value_set, n, seed + 1).reshape(B, C, H, W)
    noise = E.values("gauss0", n, seed + 2).reshape(B, C, H, W)
    pred = (np.roll(target, (1, 2), (2, 3)) + np.float32(0.3) * noise).astype(np.float32)
    return pred, target


def thresholds_of(target, T, per_image, lower):
    """[G,T] float32: data values of each group between its 20th and 90th percentile (ties with the threshold exist), none beyond
    the largest value of any image of the group (lower: the smallest), so that the target has the event in every image"""
    groups = [target[b:b + 1, c] for b in range(B) for c in range(C)] if per_image else [target[:, c] for c in range(C)]
    thr = np.empty((len(groups), T), dtype=np.float32)
    for g, x in enumerate(groups):
        s = np.sort(x[np.isfinite(x)].ravel())
        lo, hi = (0.1, 0.8) if lower else (0.2, 0.9)
        picks = s[(np.linspace(lo, hi, T) * (s.size - 1)).astype(int)] if T > 1 else s[[s.size // 2]]
        ends = [img[np.isfinite(img)] for img in x]
        thr[g] = np.maximum(picks, max(e.min() for e in ends)) if lower else np.minimum(picks, min(e.max() for e in ends))
    return thr


def check(out, cnt, want_cnt, want, tag, nonzero=True):
    got_cnt, got = cnt.cpu().numpy(), out.cpu().numpy()
    if nonzero:                                         # nothing hides behind NaN == NaN
        assert (want_cnt[..., 1] + want_cnt[..., 2] > 0).all() and np.isfinite(want).all(), tag
    print(tag, "cnt equal:", np.array_equal(got_cnt, want_cnt))
    assert got_cnt.dtype == np.int64 and np.array_equal(got_cnt, want_cnt), tag
    w32 = want.astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(w32)), tag
    fin = np.isfinite(w32)
    worst = int(E.ulp_distance(got[fin], w32[fin]).max()) if fin.any() else 0
    print(tag, "worst ulp:", worst)
    assert worst <= 1, (tag, worst)


# ---- main parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", list(R.PLANES) + ["partition"], ids=lambda p: p if isinstance(p, str) else "%dx%d" % p)
def test_sums_equal_the_yardstick(plane):
    from climate_learn import _hip
    H, W = partition_plane() if plane == "partition" else plane
    k = 0
    for T in LEVEL_COUNTS:
        for per_image in (False, True):
            for lower in (False, True):
                pred, target = make_pair(H, W, VALUE_SETS[k % len(VALUE_SETS)], seed=7 * k)
                k += 1
                thr = thresholds_of(target, T, per_image, lower)
                p, t, th = _dev(pred), _dev(target), torch.from_numpy(thr).cuda()
                for n in R.WINDOWS:
                    want_cnt, want = R.grouped(pred, target, thr, n, None, lower, per_image)
                    out, cnt = _hip.masked_fss(p, t, th, n, lower=lower, per_image=per_image)
                    check(out, cnt, want_cnt, want, (plane, T, per_image, lower, n))
                    assert (cnt[..., 0] == H * W).all()


# ---- operand forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [False, True], ids=["aligned", "odd_view"])
def test_crop_holes_mask_and_a_nan_prediction(view):
    """a target larger than the prediction (huge finite values outside the crop that would be events if they were read), NaN and
    Inf holes in the target, a broadcast [H,W] mask, NaN predictions at valid and at invalid pixels, in a view offset by one
    element, and one image without any valid pixel"""
    from climate_learn import _hip
    from climate_learn.metrics.functional import _mask_operand
    H, W = (33, 71) if view else (32, 72)
    pred, crop = make_pair(H, W, "gauss280", seed=5)
    crop[0, 0, 2:7, 2:9] = np.nan
    crop[0, 0, 3, 5], crop[0, 0, 4, 6] = np.inf, -np.inf
    crop[1, 2] = np.nan                                                 # an image without data
    pred[0, 0, 2:7, 2:9] = np.nan                                       # at invalid pixels: never compared
    pred[1, 1, 10, 10:14] = np.nan                                      # at valid pixels: in no indicator
    target = np.full((B, C, H + 2, W + 5), 3e38, dtype=np.float32)
    target[:, :, :H, :W] = crop
    mask = np.random.default_rng(11).random((H, W)) < 0.8
    mask[0, 0] = mask[H - 1, W - 1] = False
    thr = thresholds_of(np.where(np.isfinite(crop), crop, np.float32(280.0)), 5, False, False)
    p, t = _dev(pred, view), _dev(target, view)
    m, pitch, sb, sc = _mask_operand(torch.from_numpy(mask).cuda(), p, t)
    assert (pitch, sb, sc) == (W, 0, 0)
    for n, lower in ((7, False), (65, True)):
        want_cnt, want = R.grouped(pred, crop, thr, n, mask, lower)
        out, cnt = _hip.masked_fss(p, t, torch.from_numpy(thr).cuda(), n, m, (pitch, sb, sc), lower=lower)
        check(out, cnt, want_cnt, want, (view, n, lower), nonzero=False)
        assert not cnt[1, 2].any() and torch.isnan(out[1, 2]).all() and torch.isfinite(out[0]).all()
        assert int(cnt[0, 0, 0, 0]) == int((mask & np.isfinite(crop[0, 0])).sum())


# ---- degenerate cases --------------------------------------------------------------------------------------------------------------
def test_no_event_every_pixel_an_event_and_one_field_twice():
    from climate_learn import _hip
    H, W = 9, 65
    pred, target = make_pair(H, W, "gauss0", seed=3)
    p, t = _dev(pred), _dev(target)
    above = torch.full((C, 1), 1e6, device="cuda")
    out, cnt = _hip.masked_fss(p, t, above, 7)
    assert torch.isnan(out).all() and not cnt[..., 1:].any() and (cnt[..., 0] == H * W).all()
    out, cnt = _hip.masked_fss(p, t, -above, 7)                         # every pixel an event in both fields: the window's area
    area = int((R.box_counts(np.ones((H, W), bool), 7) ** 2).sum())
    assert (out == 1.0).all() and (cnt[..., 1] == area).all() and (cnt[..., 2] == area).all() and not cnt[..., 3].any()
    thr = torch.from_numpy(thresholds_of(target, 5, False, False)).cuda()
    out, cnt = _hip.masked_fss(t, t, thr, 33)                           # pred is target
    assert (out == 1.0).all() and not cnt[..., 3].any() and torch.equal(cnt[..., 1], cnt[..., 2]) and (cnt[..., 1] > 0).all()


# ---- side effects ------------------------------------------------------------------------------------------------------------------
def test_guard_words_plain_kinds_and_two_calls():
    """nothing is written around out, cnt or beyond the macro's workspace words; kinds 0 / 1 give the same bits before and after
    an FSS call on the same workspace; two FSS calls give the same bits"""
    from climate_learn import _hip
    H, W, T, n = 33, 71, 5, 33
    pred, target = make_pair(H, W, "zero_inflated", seed=9)
    target[0, 1, 3:9, 5:11] = np.nan
    p, t = _dev(pred), _dev(target)
    thr = torch.from_numpy(thresholds_of(target, T, False, False)).cuda()
    G = 8                                                                # guard words at each end
    words = _hip.fss_ws_words(B, C, H, W, T)
    assert words >= 2 * B * C * _hip.LOSS_BLOCKS
    ws = torch.full((words // 2 + G,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    out = torch.full((B * C * T + 2 * G,), -7.5, device="cuda")
    cnt = torch.full((B * C * T * 4 + 2 * G,), -77, dtype=torch.int64, device="cuda")
    lat = torch.linspace(0.5, 1.5, H, device="cuda")
    cw = torch.tensor([1.0, 10.0, 10.0], device="cuda")

    def plain(kind):
        o, c = torch.empty(C + 1, device="cuda"), torch.empty(C + 1, dtype=torch.int64, device="cuda")
        _hip._call("orbit2_masked_loss_fwd", p, t, H, W, None, 0, 0, 0, lat, cw, o, c, ws, B, C, H, W, kind)
        return o, c

    def fss():
        kind = _hip.FSS_KIND | (T << 8) | (n << 16)
        _hip._call("orbit2_masked_loss_fwd", p, t, H, W, None, 0, 0, 0, None, thr, out[G:-G], cnt[G:-G], ws, B, C, H, W, kind)
        return out[G:-G].clone().view(B, C, T), cnt[G:-G].clone().view(B, C, T, 4)

    before = [plain(kind) for kind in (0, 1)]
    ws.fill_(0x5a5a5a5a5a5a5a5a)
    o1, c1 = fss()
    assert (ws[words // 2:] == 0x5a5a5a5a5a5a5a5a).all()
    assert (out[:G] == -7.5).all() and (out[-G:] == -7.5).all() and (cnt[:G] == -77).all() and (cnt[-G:] == -77).all()
    want_cnt, want = R.grouped(pred, target, thr.cpu().numpy(), n)
    check(o1, c1, want_cnt, want, "guarded")
    after = [plain(kind) for kind in (0, 1)]
    for (a0, n0), (a1, n1) in zip(before, after):
        assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and torch.equal(n0, n1)
        assert int(n0[-1]) == pred.size - 36 and torch.isfinite(a0).all()
    o2, c2 = fss()                                                      # on a workspace the plain kinds have written to
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(c1, c2)
    o3, c3 = _hip.masked_fss(p, t, thr, n)
    assert torch.equal(o1.view(torch.int32), o3.view(torch.int32)) and torch.equal(c1, c3)


# ---- functionals, the registry name, neighbourhood_scores --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored():
    """a (2,3,24,40) prediction against its (26,44) target with a few NaN targets, computed once"""
    H, W = 24, 40
    pred, crop = make_pair(H, W, "zero_inflated", seed=21)
    crop[1, 2, 5:8, 10:20] = np.nan
    target = np.full((B, C, H + 2, W + 4), 3e38, dtype=np.float32)
    target[:, :, :H, :W] = crop
    return dict(pred=pred, crop=crop, p=_dev(pred), t=_dev(target))


def _device_quantiles(s, q):
    """[C,Q] float32: the pooled target quantiles as the device finds them (tests/test_extremes_gpu.py holds them to numpy's)"""
    from climate_learn.metrics import functional as fn
    return fn._quantiles(s["p"], s["t"], q)[0][0, :, :, 0].cpu().numpy()


def _ulps(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float64).astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    return int(E.ulp_distance(got[fin], want[fin]).max()) if fin.any() else 0


def test_functionals_and_the_registered_metric(scored):
    import climate_learn as cl
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.utils import MetricsMetaInfo
    s = scored
    thr = _device_quantiles(s, (0.9772,))
    per = R.pooled(R.grouped(s["pred"], s["crop"], thr, 9)[0])[:, 0]
    assert np.isfinite(per).all() and (per > 0).all() and (per < 1).all()
    want = np.append(per.astype(np.float32), per.astype(np.float32).mean(dtype=np.float32))
    got = fn.fss(s["p"], s["t"])
    assert tuple(got.shape) == (C + 1,) and _ulps(got[:C].cpu().numpy(), per) <= 1 and _ulps(got[C:].cpu().numpy(), want[C:]) <= 2
    meta = MetricsMetaInfo(["a", "b", "c"], ["a", "b", "c"], np.linspace(-80.0, 80.0, 24), np.arange(40), None)
    assert torch.equal(cl.load_loss("cuda", None, "fss", False, meta)(s["p"], s["t"]), got)
    metric = cl.load_loss("cuda", None, "fss", False, meta).set_window(5).set_level(0.8413)
    thr5 = _device_quantiles(s, (0.8413,))
    assert _ulps(metric(s["p"], s["t"])[:C].cpu().numpy(), R.pooled(R.grouped(s["pred"], s["crop"], thr5, 5)[0])[:, 0]) <= 1
    # explicit thresholds, the lower side, and a threshold beyond every value: NaN
    low = np.array([[0.0], [0.5], [-10.0]], dtype=np.float32)
    got = fn.fss(s["p"], s["t"], 3, lower=True, thresholds=torch.from_numpy(low[:, 0]))
    per = R.pooled(R.grouped(s["pred"], s["crop"], low, 3, None, True)[0])[:, 0]
    assert np.isnan(per[2]) and np.isfinite(per[:2]).all() and _ulps(got[:C].cpu().numpy(), per) <= 1 and torch.isnan(got[C])
    # the profile
    windows = (1, 3, 9, 33)
    thr3 = _device_quantiles(s, fn.SIGMA_LEVELS)
    prof = fn.fss_profile(s["p"], s["t"], windows)
    cnts = {n: R.grouped(s["pred"], s["crop"], thr3, n)[0].sum(0) for n in windows}
    for j, n in enumerate(windows):
        assert _ulps(prof["fss"][:, :, j].cpu().numpy(), R.pooled(cnts[n][None])) <= 1
    base = cnts[1][..., 1] / cnts[1][..., 0]
    v = np.isfinite(s["crop"])
    with np.errstate(invalid="ignore"):
        events = np.stack([[(v[:, c] & (s["crop"][:, c] >= thr3[c, k])).sum() for k in range(3)] for c in range(C)])
    assert np.array_equal(cnts[1][..., 1], events) and np.array_equal(cnts[1][..., 0], np.broadcast_to(v.sum((0, 2, 3))[:, None], (C, 3)))
    assert _ulps(prof["base_rate"].cpu().numpy(), base) <= 1 and _ulps(prof["uniform"].cpu().numpy(), 0.5 + 0.5 * base) <= 1
    score = np.stack([R.pooled(cnts[n][None]) for n in windows], -1)
    reach = score >= (0.5 + 0.5 * base)[..., None]
    want_w = np.where(reach.any(-1), np.asarray(windows)[reach.argmax(-1)], 0)
    margin = np.abs(score - (0.5 + 0.5 * base)[..., None]).min()
    assert margin > 1e-6                                                 # no score sits on its bar: the comparison is decided
    assert np.array_equal(prof["skilful_window"].cpu().numpy(), want_w)


def test_neighbourhood_scores_against_the_yardstick(scored):
    from climate_learn.metrics import functional as fn
    from climate_learn.utils.visualize import neighbourhood_scores
    s = scored
    windows = (1, 5, 17)
    res = neighbourhood_scores(s["p"], s["t"], ["a", "b", "c"], windows=windows)
    thr3 = _device_quantiles(s, fn.SIGMA_LEVELS)
    cnts = {n: R.grouped(s["pred"], s["crop"], thr3, n)[0].sum(0) for n in windows}
    for c, v in enumerate("abc"):
        assert len(res[v]) == 3
        for j, row in enumerate(res[v]):
            assert row["level"] == fn.SIGMA_LEVELS[j] and row["threshold"] == float(thr3[c, j])
            base = cnts[1][c, j, 1] / cnts[1][c, j, 0]
            assert _ulps([row["base_rate"]], [base]) <= 1 and _ulps([row["uniform"]], [0.5 + 0.5 * base]) <= 1
            for n in windows:
                assert _ulps([row["fss"][n]], [R.score(tuple(int(x) for x in cnts[n][c, j]))]) <= 1
            reach = [n for n in windows if row["fss"][n] >= row["uniform"]]
            assert row["skilful_window"] == (reach[0] if reach else 0)


# ---- the inference driver ----------------------------------------------------------------------------------------------------------
def test_inference_driver_neighbourhood_scores(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_fss.yaml")))
    conf["neighbourhood_scores"] = {"levels": [0.5, 0.9772], "windows": [1, 9, 255]}
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
    got = [ln for ln in lines if ln.startswith("neighbourhood_scores ")]
    assert [ln.split()[1] for ln in got] == out_vars and not [ln for ln in lines if ln.startswith("extreme_scores ")]
    num = r"([-+.\dinfae]+)"
    for ln in got:
        rows = re.findall(r"\{'level': %s, 'threshold': %s, 'base_rate': %s, 'uniform': %s, 'skilful_window': (\d+), "
                          r"'fss': \{1: %s, 9: %s, 255: %s\}\}" % ((num,) * 7), ln.split(" ", 2)[2])
        assert len(rows) == 2 and [float(row[0]) for row in rows] == pytest.approx([0.5, 0.9772], abs=1e-6)
        for row in rows:
            base, uniform, skilful = float(row[2]), float(row[3]), int(row[4])
            scores = [float(v) for v in row[5:8]]
            assert 0.0 < base <= 1.0 and uniform == pytest.approx(0.5 + base / 2, abs=2e-6) and skilful in (0, 1, 9, 255)
            assert all(0.0 <= v <= 1.0 for v in scores)
            # the event is "at or beyond the target's quantile at q": at least the fraction 1 - q of the pixels, more only by ties
            assert base >= 1.0 - float(row[0]) - 1e-3
