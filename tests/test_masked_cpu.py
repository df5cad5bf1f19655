"""CPU checks of the missing-data masks: tests/masked_ref.py -- the float64 restatement the GPU tests compare
against -- reproduces the reference's own numbers (tests/golden/masked.npz) and the unmasked oracle; the registry names, the
ABI entries and their bindings exist; the mask helper accepts and refuses what it says; nothing runs on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import masked_ref as ref
from tests.conftest import GOLDEN, ROOT

NAMES = ("masked_mse", "masked_lat_mse", "masked_bayesian_tv", "masked_rmse", "masked_lat_rmse", "masked_mae",
         "masked_pearson", "masked_mean_bias")
ENTRIES = ("orbit2_masked_loss_fwd", "orbit2_masked_loss_bwd", "orbit2_masked_moments")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "masked.npz")))


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_ref_reproduces_the_reference_masked_rmse(gold):
    pred, target = _t(gold["pred"]), _t(gold["target"]).clone()
    target[_t(gold["nan_where"])] = float("nan")                   # the reference saw a zero there and a zero in its mask
    for tag in ("b1", "bc"):
        mask = _t(gold["mask_" + tag])
        np.testing.assert_allclose(ref.rmse(pred, target, None, mask).numpy(), gold["rmse." + tag], rtol=1e-12)
        np.testing.assert_allclose(ref.rmse(pred, target, _t(gold["lat_w"]), mask).numpy(), gold["lat_rmse." + tag], rtol=1e-12)
    # all ones: the reference's masked form differs from its plain rmse by the +1e-9 only (7e-10 relative)
    ones = ref.rmse(pred, _t(gold["target"]), None, torch.ones(pred.shape[2:])).numpy()
    np.testing.assert_allclose(ones, gold["rmse.ones"], rtol=1e-12)
    rel = np.abs(gold["rmse.ones"] / gold["rmse.plain"] - 1)
    assert rel.max() < 7e-10 and rel.min() > 1e-10


@pytest.mark.parametrize("kind", ["mse", "bayesian_tv"])
def test_ref_rectangle_identity_against_the_reference(gold, kind):
    """valid region = one top-left rectangle: the reference's loss on the cropped fields, TV terms included"""
    pred, target = _t(gold["pred"]), _t(gold["target"])
    h0, w0 = (int(v) for v in gold["rect_hw"])
    rect = torch.zeros(pred.shape[2:], dtype=torch.bool)
    rect[:h0, :w0] = True
    nan_t = target.clone()
    nan_t[:, :, h0:, :] = float("nan")                             # the same rectangle, half by NaN, half by the mask
    k = 0 if kind == "mse" else 1
    for lat in (False, True):
        for var in (False, True):
            key = "rect." + kind + (".lat" if lat else "") + (".var" if var else "")
            lw = _t(gold["lat_w"]) if lat else None
            cw = _t(gold["var_weights"]) if var else None
            for tgt in (target, nan_t):
                out, cnt = ref.loss(pred, tgt, k, lw, cw, rect)
                np.testing.assert_allclose(out.numpy(), gold[key], rtol=1e-12)
                assert cnt.tolist() == [2 * h0 * w0] * 3 + [6 * h0 * w0]


@pytest.mark.parametrize("kind", ["mse", "bayesian_tv"])
def test_ref_all_valid_is_the_unmasked_oracle(gold, kind):
    from oracle.orbit2_oracle import LOSSES
    pred, target = _t(gold["pred"]).double(), _t(gold["target"]).double()
    names, weights = ["a", "b", "c"], dict(zip("abc", gold["var_weights"].tolist()))
    lw = _t(gold["lat_w"]).double()
    for mask in (None, torch.ones(pred.shape[2:])):
        out, _, g = ref.loss(pred, target, 0 if kind == "mse" else 1, lw, _t(gold["var_weights"]), mask, grad=True)
        p = pred.clone().requires_grad_(True)
        want = LOSSES[kind](p, target, names, weights, False, lw.view(1, 1, -1, 1))
        np.testing.assert_allclose(out.numpy(), want.detach().numpy(), rtol=1e-13)
        (gw,) = torch.autograd.grad(want[-1], p)
        np.testing.assert_allclose(g.numpy(), gw.numpy(), rtol=1e-12, atol=1e-18)


def test_ref_ignores_what_is_invalid(gold):
    """NaN / Inf in pred and target at invalid pixels change nothing, and the gradient is 0 there"""
    pred, target = _t(gold["pred"]).clone(), _t(gold["target"]).clone()
    mask = _t(gold["mask_bc"])
    base = ref.loss(pred, target, 1, None, None, mask, grad=True)
    bad = mask == 0
    pred[bad], target[bad] = float("nan"), float("inf")
    out, cnt, g = ref.loss(pred, target, 1, None, None, mask, grad=True)
    assert torch.equal(out, base[0]) and torch.equal(cnt, base[1]) and torch.equal(g, base[2])
    assert torch.isfinite(out).all() and torch.isfinite(g).all() and bool((g[bad] == 0).all())
    m = ref.moments(pred, target, None, None, mask)
    assert torch.isfinite(m).all() and torch.equal(m[..., 12].long(), (~bad).sum((2, 3)))
    # a channel without data: NaN, and the aggregate is the mean of the others
    target[:, 1] = float("nan")
    for got in (ref.mae(pred, target, None, mask), ref.mean_bias(pred, target, mask), ref.pearson(pred, target, mask)):
        assert torch.isnan(got[1]) and torch.isfinite(got[[0, 2, 3]]).all()
        assert torch.isclose(got[3], (got[0] + got[2]) / 2, rtol=1e-14)


def test_registry_names_resolve_through_the_loader():
    import climate_learn as cl
    from climate_learn.metrics.metrics import LatitudeWeightedMetric
    from climate_learn.metrics.utils import METRICS_REGISTRY, MetricsMetaInfo
    meta = MetricsMetaInfo(["a"], ["a"], np.linspace(-60, 60, 13), np.arange(8), None)
    for name in NAMES:
        obj = cl.load_loss("cpu", None, name, True, meta)
        assert type(obj) is METRICS_REGISTRY[name] and obj.name == name and obj.aggregate_only
        assert getattr(obj, "graph_capturable", False) is True
        assert obj.set_mask(np.ones((13, 8))) is obj and obj._static_mask.dtype == torch.bool
        assert isinstance(obj, LatitudeWeightedMetric) == ("lat" in name)


def test_abi_entries_and_bindings():
    from climate_learn import _hip
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "orbit2_hip.h")).read(), flags=re.S)
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    mask = (P, I, L, L)
    want = {"orbit2_masked_loss_fwd": (P, P, I, I) + mask + (P, P, P, P, P, I, I, I, I, I, P),
            "orbit2_masked_loss_bwd": (P, P, I, I) + mask + (P, P, P, P, P, I, I, I, I, I, P),
            "orbit2_masked_moments": (P, P, I, I) + mask + (P, P, P, I, I, I, I, P)}
    for name in ENTRIES:
        assert re.search(r"\bint %s\(const float\* pred, const float\* target, int Ht, int Wt, const uint8_t\* mask, "
                         r"int mask_pitch,\s+int64_t mask_sb, int64_t mask_sc," % name, hdr), name
        assert _hip.PROTOTYPES[name] == (I, want[name]) and hasattr(_hip.lib(), name)
    assert "#define ORBIT2_ABI_VERSION 8" in hdr and _hip.ABI_VERSION == 8 and _hip.lib().orbit2_abi_version() == 8
    for name in ("masked_loss_fwd", "masked_loss_bwd", "masked_moments"):
        assert callable(getattr(_hip, name))


def test_entries_refuse_bad_arguments_without_a_gpu():
    """every refusal returns before anything is launched"""
    from climate_learn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    fwd = lambda **k: lib.orbit2_masked_loss_fwd(*[{**dict(pred=a, target=a, Ht=8, Wt=8, mask=None, pitch=0, sb=0, sc=0, lat=None,
                                                          cw=None, out=a, cnt=a, ws=a, B=1, C=1, H=8, W=8, kind=0, s=None),
                                                   **k}[n] for n in ("pred", "target", "Ht", "Wt", "mask", "pitch", "sb", "sc",
                                                                     "lat", "cw", "out", "cnt", "ws", "B", "C", "H", "W", "kind",
                                                                     "s")])
    for bad in (dict(pred=None), dict(target=None), dict(out=None), dict(cnt=None), dict(ws=None), dict(B=0), dict(Ht=7),
                dict(Wt=7), dict(kind=2), dict(kind=-1), dict(mask=a, pitch=7), dict(mask=a, pitch=8, sb=-1)):
        assert fwd(**bad) == -1, bad
    assert lib.orbit2_masked_loss_bwd(a, a, 8, 8, None, 0, 0, 0, None, None, a, a, a, 1, 1, 8, 8, 2, None) == -1      # kind 2
    assert lib.orbit2_masked_loss_bwd(a, a, 8, 8, None, 0, 0, 0, None, None, a, None, a, 1, 1, 8, 8, 0, None) == -1   # no counts
    assert lib.orbit2_masked_moments(a, a, 8, 8, None, 0, 0, 0, None, None, None, 1, 1, 8, 8, None) == -1
    assert lib.orbit2_masked_moments(a, a, 8, 8, a, 4, 0, 0, None, None, a, 1, 1, 8, 8, None) == -1                   # pitch < W
    assert not any(buf)


def test_mask_helper_accepts_and_refuses():
    from climate_learn.metrics.functional import _mask_operand
    from climate_learn.models.hub.interpolation import Resampled
    B, C, H, W, Ht, Wt = 2, 3, 5, 8, 7, 12
    pred, target = torch.zeros(B, C, H, W), torch.zeros(B, C, Ht, Wt)
    assert _mask_operand(None, pred, target) == (None, 0, 0, 0)
    for hh, ww in ((H, W), (Ht, Wt)):
        for shape, sb, sc in (((hh, ww), 0, 0), ((1, 1, hh, ww), 0, 0), ((B, 1, hh, ww), hh * ww, 0),
                              ((B, C, hh, ww), C * hh * ww, hh * ww)):
            for dtype in (torch.bool, torch.uint8, torch.int64, torch.float32):
                src = (torch.arange(int(np.prod(shape))).reshape(shape) % 3).to(dtype)         # 0, 1, 2, ...: 2 is "keep" too
                m, pitch, gb, gc = _mask_operand(src, pred, target)
                assert m.dtype == torch.uint8 and m.is_contiguous() and tuple(m.shape) == shape       # never expanded
                assert (pitch, gb, gc) == (ww, sb, sc)
                assert torch.equal(m != 0, src != 0)
    bool_mask = torch.ones(H, W, dtype=torch.bool)
    assert _mask_operand(bool_mask, pred, target)[0].data_ptr() == bool_mask.data_ptr()        # used in place
    for shape in ((C, H, W), (B + 1, 1, H, W), (1, C, H, W), (B, C - 1, H, W), (H, W + 1), (B, C, H + 1, W), (B, C, Ht, W), (W,)):
        with pytest.raises(ValueError, match=r"a mask is \[H,W\], \[1,1,H,W\], \[B,1,H,W\] or \[B,C,H,W\]"):
            _mask_operand(torch.ones(shape), pred, target)
    lazy = Resampled(torch.zeros(B, C, 2, 4), (H, W))
    for mask in (None, bool_mask):
        with pytest.raises(TypeError, match="Resampled"):
            _mask_operand(mask, lazy, target)


def test_cpu_tensors_are_refused():
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.utils import METRICS_REGISTRY, MetricsMetaInfo
    pred, target = torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8)
    mask = torch.ones(8, 8, dtype=torch.bool)
    cnt = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.masked_loss_fwd(pred, target, None, None, 0)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.masked_loss_bwd(pred, target, None, None, torch.ones(1), cnt, 0)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.masked_moments(pred, target)
    meta = MetricsMetaInfo(["a", "b"], ["a", "b"], np.linspace(-60, 60, 8), np.arange(8), None)
    for name in NAMES:
        with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
            METRICS_REGISTRY[name](metainfo=meta)(pred, target)
    for f in (fn.masked_mse, fn.masked_bayesian_tv):
        with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
            f(pred, target, mask=mask)
    for f in (fn.rmse, fn.mae, fn.pearson, fn.mean_bias):
        with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
            f(pred, target, mask=mask)
