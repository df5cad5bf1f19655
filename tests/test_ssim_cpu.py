"""CPU checks of the device SSIM / PSNR: the ABI entry and its binding, the refusals that need no GPU, the metric registry, the
host algebra of metrics.functional.ssim / psnr on fabricated sums, and an fp32 numpy emulation of the kernel's own summation
order (csrc/ssim.hip: tile pivot, 7-tap row pass, 7-tap column pass oldest row first) against float64 -- the measurement the
tolerances of tests/test_ssim_gpu.py are derived from."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_ssim_gpu import LAT, MAP_TOL, MEAN_TOL, make_fields, ssim_oracle


def test_abi_entry_and_binding():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    assert re.search(r"\bint orbit2_ssim\(const float\* pred, const float\* target, int Ht, int Wt, const float\* lat_w, "
                     r"const float\* data_range,\s+double\* sums, float\* ssim_map, int B, int C, int H, int W, void\* stream\);",
                     hdr)
    assert "#define ORBIT2_ABI_VERSION 8" in hdr and _hip.ABI_VERSION == 8
    I, P = ctypes.c_int, ctypes.c_void_p
    assert _hip.PROTOTYPES["orbit2_ssim"] == (I, (P, P, I, I, P, P, P, P, I, I, I, I, P))
    assert hasattr(_hip.lib(), "orbit2_ssim") and _hip.lib().orbit2_abi_version() == 8
    tile = tuple(int(re.search(r"#define ORBIT2_SSIM_TILE_%s (\d+)" % a, hdr).group(1)) for a in "HW")
    assert _hip.SSIM_TILE == tile and _hip.SSIM_WIN == int(re.search(r"#define ORBIT2_SSIM_WIN (\d+)", hdr).group(1)) == 7


def test_entry_and_binding_refuse_without_a_gpu():
    from climate_learn import _hip
    f = _hip.lib().orbit2_ssim
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    assert f(None, a, 8, 8, None, None, a, None, 1, 1, 8, 8, None) == -1
    assert f(a, None, 8, 8, None, None, a, None, 1, 1, 8, 8, None) == -1
    assert f(a, a, 8, 8, None, None, None, None, 1, 1, 8, 8, None) == -1
    assert f(a, a, 8, 8, None, None, a, None, 0, 1, 8, 8, None) == -1
    assert f(a, a, 8, 8, None, None, a, None, 1, 1, 6, 8, None) == -1          # smaller than the window
    assert f(a, a, 8, 8, None, None, a, None, 1, 1, 8, 6, None) == -1
    assert f(a, a, 7, 8, None, None, a, None, 1, 1, 8, 8, None) == -1          # target smaller than the prediction
    assert f(a, a, 8, 8, None, None, a, None, 256, 256, 8, 8, None) == -1      # B * C > 65535
    assert not any(buf)
    x = torch.zeros(1, 1, 8, 40)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.ssim_sums(x, x)
    with pytest.raises(_hip.HipBackendError, match="at least 7 x 7"):
        _hip.ssim_sums(x[:, :, :6], x)


def test_names_resolve_in_the_registry():
    from climate_learn.metrics.metrics import LatitudeWeightedMetric, Metric
    from climate_learn.metrics.utils import METRICS_REGISTRY, MetricsMetaInfo
    for name in ("ssim", "lat_ssim", "psnr"):
        assert name in METRICS_REGISTRY and issubclass(METRICS_REGISTRY[name], Metric) and METRICS_REGISTRY[name].name == name
    assert issubclass(METRICS_REGISTRY["lat_ssim"], LatitudeWeightedMetric)
    meta = MetricsMetaInfo(["a"], ["a"], np.linspace(-60, 60, 13), np.arange(8), None)
    assert METRICS_REGISTRY["lat_ssim"](metainfo=meta).lat_weights.shape == (1, 1, 13, 1)


def test_host_algebra_on_fabricated_sums(monkeypatch):
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.utils import METRICS_REGISTRY, MetricsMetaInfo
    B, C, H, W = 2, 3, 13, 20
    rng = np.random.default_rng(0)
    sums = rng.uniform(1.0, 50.0, (B, C, 6))
    sums[..., 5] = rng.uniform(2.0, 6.0, (B, C))
    sums[1, 2, 2] = 0.0                                 # one image without error: psnr = inf
    seen = {}

    def fake(pred, target, lat_w=None, data_range=None, ssim_map=False):
        seen.update(lat_w=lat_w, data_range=data_range, shape=tuple(pred.shape))
        return torch.from_numpy(sums)
    monkeypatch.setattr(_hip, "ssim_sums", fake)
    pred, target = torch.zeros(B, C, H, W), torch.zeros(B, C, H + 2, W + 1)
    per_channel = (sums[..., 0] / ((H - 6) * (W - 6))).mean(0)
    got = fn.ssim(pred, target).numpy()
    assert got.shape == (C + 1,) and seen["lat_w"] is None and seen["data_range"] is None
    assert np.allclose(got[:C], per_channel, rtol=1e-6) and np.isclose(got[C], per_channel.mean(), rtol=1e-6)
    assert np.isclose(float(fn.ssim(pred, target, aggregate_only=True, data_range=3.0)), per_channel.mean(), rtol=1e-6)
    assert seen["data_range"] == 3.0
    # the weights are normalised over the valid rows 3 .. H - 4 only
    lat = torch.linspace(0.2, 1.7, H + 2).view(1, 1, -1, 1)                    # longer than the prediction: its first H are used
    w = lat.reshape(-1)[:H].double().numpy()
    want = (sums[..., 1] / ((W - 6) * w[3:H - 3].sum())).mean(0)
    got = fn.ssim(pred, target, lat_weights=lat).numpy()
    assert seen["lat_w"].shape == (H,) and np.allclose(got[:C], want, rtol=1e-6) and np.isclose(got[C], want.mean(), rtol=1e-6)
    assert not np.allclose(want, (sums[..., 1] / ((W - 6) * w.sum())).mean(0), rtol=1e-3)
    # psnr: batch mean of the per-image dB, inf where an image has no error
    db = 10 * np.log10(sums[..., 5] ** 2 / np.where(sums[..., 2] == 0, np.nan, sums[..., 2] / (H * W)))
    db[1, 2] = np.inf
    got = fn.psnr(pred, target).numpy()
    assert got.shape == (C + 1,) and np.allclose(got[:2], db.mean(0)[:2], rtol=1e-6) and got[2] == np.inf and got[3] == np.inf
    # a Normal is taken by its loc; the registered objects go the same way
    normal = torch.distributions.Normal(pred, torch.ones_like(pred))
    assert torch.equal(fn.ssim(normal, target), fn.ssim(pred, target)) and seen["shape"] == (B, C, H, W)
    meta = MetricsMetaInfo(["a"], ["a"], np.linspace(-60, 60, H), np.arange(W), None)
    assert torch.equal(METRICS_REGISTRY["ssim"](metainfo=meta)(pred, target), fn.ssim(pred, target))
    assert torch.equal(METRICS_REGISTRY["psnr"](aggregate_only=True, metainfo=meta)(pred, target), fn.psnr(pred, target, True))
    obj = METRICS_REGISTRY["lat_ssim"](metainfo=meta)
    assert torch.equal(obj(pred, target), fn.ssim(pred, target, lat_weights=obj.lat_weights))
    assert seen["lat_w"].shape == (H,)


# ---- the kernel's summation order in fp32 numpy ----------------------------------------------------------------------------------
F = np.float32


def emulate_map(pred, target, data_range, centred=True, tile=(32, 64), strip=8):
    """fp32 S map of one [H,W] image the way csrc/ssim.hip sums it: per tile of centres both fields minus the target's value at
    the tile's first pixel, then per strip of 8 centre rows and per column minus the (tile-centred) target under the middle of
    the strip's windows (centred=False: minus nothing); 7-tap row sums added left to right, seven row sums added oldest first,
    the formula of the kernel operation by operation; and the image's sum of S in the kernel's reduction order.  (numpy has no fused multiply-add: the products are rounded once more
    than on the device -- part of what the factor 4 of the tolerance covers.)"""
    H, W = pred.shape
    out, total = np.zeros((H - 6, W - 6), dtype=F), 0.0
    lanes = np.arange(64)
    R = F(data_range)
    c1, c2 = (F(0.01) * R) * (F(0.01) * R), (F(0.03) * R) * (F(0.03) * R)
    inv_n, inv_n1 = F(1) / F(49), F(1) / F(48)
    for y0 in range(0, H - 6, tile[0]):
        for x0 in range(0, W - 6, tile[1]):
            x1 = min(x0 + tile[1], W - 6)
            n = x1 - x0
            pivot = target[y0, x0] if centred else F(0)
            ta, tb = pred[y0:y0 + tile[0] + 6, x0:x1 + 6] - pivot, target[y0:y0 + tile[0] + 6, x0:x1 + 6] - pivot
            for r0 in range(0, min(tile[0], H - 6 - y0), strip):
                m = min(strip, H - 6 - y0 - r0)
                local = tb[min(r0 + 3 + strip // 2, ta.shape[0] - 1), 3:3 + n] if centred else np.zeros(n, dtype=F)
                a, b = ta[r0:r0 + m + 6], tb[r0:r0 + m + 6]
                rows = [np.zeros((m + 6, n), dtype=F) for _ in range(5)]
                for k in range(7):
                    ak, bk = a[:, k:k + n] - local, b[:, k:k + n] - local
                    for q, term in enumerate((ak, bk, ak * ak, bk * bk, ak * bk)):
                        rows[q] = rows[q] + term
                w = []
                for q in range(5):
                    v = rows[q][0:m]
                    for k in range(1, 7):
                        v = v + rows[q][k:k + m]
                    w.append(v)
                ma, mb = w[0] * inv_n, w[1] * inv_n
                va, vb, vab = (w[2] - w[0] * ma) * inv_n1, (w[3] - w[1] * mb) * inv_n1, (w[4] - w[0] * mb) * inv_n1
                shift = local + pivot
                ux, uy = ma + shift, mb + shift
                num = (F(2) * ux * uy + c1) * (F(2) * vab + c2)
                den = (ux * ux + uy * uy + c1) * (va + vb + c2)
                assert num.dtype == F and den.dtype == F
                out[y0 + r0:y0 + r0 + m, x0:x1] = num / den
                # the sum of the image: a lane adds its strip's centres top to bottom, the wave's butterfly adds the lanes,
                # everything from there on is double
                lane = np.zeros(64, dtype=F)
                for r in range(m):
                    lane[:n] = lane[:n] + out[y0 + r0 + r, x0:x1]
                for o in (32, 16, 8, 4, 2, 1):
                    lane = lane + lane[lanes ^ o]
                assert lane.dtype == F
                total += float(lane[0])
    return out, total


def _emulation_errors(pred, target, centred):
    """(worst per-pixel error, worst error of an image's mean) of the emulation against float64 over the images of a case"""
    _, want = ssim_oracle(pred, target)
    worst_px = worst_mean = 0.0
    for b in range(pred.shape[0]):
        for c in range(pred.shape[1]):
            t = target[b, c, : pred.shape[2], : pred.shape[3]]
            got, total = emulate_map(pred[b, c], t, F(np.float64(t.max()) - np.float64(t.min())), centred)
            worst_px = max(worst_px, float(np.abs(got.astype(np.float64) - want[b, c]).max()))
            worst_mean = max(worst_mean, abs(total / got.size - float(want[b, c].mean())))
    return worst_px, worst_mean


# the issue's 39 x 71 field and every field of tests/test_ssim_gpu.py
CASES = [((1, 1, 39, 71), None, 21), ((2, 3, 39, 71), (2, 3, 41, 72), 11), ((1, 1, 7, 7), None, 1), ((1, 1, 9, 150), None, 2),
         ((1, 1, 150, 9), None, 2), ((1, 1, 38, 70), None, 3), ((1, 1, 39, 71), None, 4), ((1, 1, 70, 134), None, 3),
         ((1, 1, 71, 135), None, 4), ((1, 1, 40, 56), None, 5)]


def test_emulated_summation_order_centred_against_raw():
    """the centred form stays inside the GPU tests' tolerances at both offsets with the factor 4 to spare; the raw form exceeds
    the per-pixel tolerance at offset 280 -- the tolerance tells the two apart"""
    worst = {}
    for offset in (0.0, 280.0):
        for shape, tshape, seed in CASES:
            pred, target = make_fields(shape, tshape, offset, seed)
            px, mean = _emulation_errors(pred, target, True)
            if shape[2:] == (7, 7):
                mean = 0.0                              # one window: the image's mean is that pixel, held to MAP_TOL
            worst[offset] = tuple(max(u, v) for u, v in zip(worst.get(offset, (0.0, 0.0)), (px, mean)))
            print("offset %5.1f %-18s centred: per pixel %.3g, image mean %.3g" % (offset, shape, px, mean))
    for offset, (px, mean) in worst.items():
        print("offset %5.1f worst: per pixel %.3g, image mean %.3g" % (offset, px, mean))
        assert 4 * px <= MAP_TOL and 4 * mean <= MEAN_TOL, (offset, px, mean)
    pred, target = make_fields((1, 1, 39, 71), None, 280.0, 21)
    raw_px, raw_mean = _emulation_errors(pred, target, False)
    print("offset 280.0 (1, 1, 39, 71) raw: per pixel %.3g, image mean %.3g" % (raw_px, raw_mean))
    assert raw_px > 100 * MAP_TOL
    assert LAT.shape == (39,) and math.isclose(float(LAT.max()), 1.0, abs_tol=0.05)
