"""CPU-side checks of the all-member ensemble scores: the float64 yardstick (tests/ensemble_ref.py) is what it claims to be,
the tie rule fills every bin, the library exports the entry and refuses bad arguments before any launch, and the host
reductions of metrics.functional follow their formulae."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_ref as ref
from tests.hashmask import o2_hash64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _crps_integral(x, y):
    """the integral of (F_ens(t) - 1{t >= y})^2 dt, exact for a step function: summed over the intervals between breakpoints"""
    pts = np.sort(np.concatenate((x, [y])))
    total = 0.0
    for a, b in zip(pts[:-1], pts[1:]):
        F = np.count_nonzero(x <= a) / len(x)
        total += (F - (1.0 if a >= y else 0.0)) ** 2 * (b - a)
    return total


@pytest.mark.parametrize("x,y", [
    ([0.3, -1.2], 0.1), ([1.0, 2.0, 4.0], 2.5), ([280.5, 279.1, 281.7, 280.0, 279.9], 283.0),
    ([0.0, 0.0, 0.0, 1.5], 0.0), (list(np.random.default_rng(5).standard_normal(64)), -0.35),
    (list(np.random.default_rng(6).standard_normal(33)), -4.0)])
def test_brute_force_crps_is_the_defining_integral(x, y):
    x = np.asarray(x, dtype=np.float64)
    emp, _ = ref.crps_fields(x.reshape(-1, 1, 1, 1, 1), np.full((1, 1, 1, 1), y))
    emp, want = float(emp.reshape(-1)[0]), _crps_integral(x, y)
    assert abs(emp - want) <= 1e-6 * want, (emp, want)


@pytest.mark.parametrize("n", [2, 3, 8, 33, 64])
def test_sorted_identity_of_the_pair_term(n):
    x = np.random.default_rng(n).standard_normal((n, 1, 1, 3, 5)) + 280.0
    s = np.sort(x, axis=0)
    k = np.arange(1, n + 1).reshape(n, 1, 1, 1, 1)
    lhs = 2 * ((2 * k - n - 1) * s).sum(0)
    rhs = np.abs(x[:, None] - x[None]).sum((0, 1))
    assert np.allclose(lhs, rhs, rtol=1e-9, atol=1e-9)
    assert np.allclose(ref.pair_sum(x), rhs / 2, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,lo,hi", [(2, 599, 684), (8, 188, 247), (64, 13, 47)])
def test_tie_rule_fills_every_bin(n, lo, hi):
    """an all-ties channel (every member equals the target) of 1920 pixels: the replica's ranks reach each of the n + 1 bins,
    sum to the pixel count, lie in the per-bin range recorded for these two seeds, and differ between the seeds"""
    shape = (1, 1, 40, 48)
    target = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
    members = np.broadcast_to(target, (n,) + shape)
    hists = []
    for seed in (0, 0x1234567800000005):
        h = ref.rank_histogram(members, target, seed)[0, 0]
        assert h.shape == (n + 1,) and h.sum() == 1920 and h.min() > 0
        assert lo <= h.min() and h.max() <= hi, (n, seed, h.min(), h.max())
        want = (o2_hash64(seed, np.arange(1920, dtype=np.uint64)) * np.uint64(n + 1)) >> np.uint64(32)
        assert np.array_equal(h, np.bincount(want.astype(np.int64), minlength=n + 1))
        hists.append(h)
    assert not np.array_equal(hists[0], hists[1])


def test_entry_is_declared_in_header_binding_and_library():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    assert re.search(r"\bint orbit2_ensemble_scores\(", hdr)
    assert int(re.search(r"^#define\s+ORBIT2_ENSEMBLE_MAX_MEMBERS\s+(\d+)", hdr, flags=re.M).group(1)) == _hip.ENSEMBLE_MAX_MEMBERS == 64
    assert "orbit2_ensemble_scores" in _hip.PROTOTYPES and hasattr(_hip.lib(), "orbit2_ensemble_scores")
    I, I64, U64, P = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
    assert _hip.PROTOTYPES["orbit2_ensemble_scores"] == (I, (P, I64, I, P, I, I, P, P, P, I, P, U64, P, P, I, I, I, I, I, P))
    assert _hip.ABI_VERSION == 8                                   # additive within the version


def test_entry_refuses_bad_arguments_before_any_launch():
    """host-side argument checks only (no device is touched: every call returns before a launch or a memset)"""
    from climate_learn import _hip
    f = _hip.lib().orbit2_ensemble_scores
    m, t, s, cf, h, q, lv = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000      # never dereferenced
    B, C, H, W = 2, 3, 8, 8
    field = B * C * H * W

    def call(members=m, stride=field, n=4, target=t, Ht=H, Wt=W, sums=s, crps=cf, hist=h, quant=q, levels=lv, Q=3, B=B, C=C,
             H=H, W=W):
        return f(members, stride, n, target, Ht, Wt, None, sums, crps, 0, hist, 0, quant, levels, Q, B, C, H, W, None)

    assert call(members=None) == -1 and call(target=None) == -1
    assert call(sums=None, crps=None, hist=None, quant=None) == -1
    assert call(n=1) == -1 and call(n=0) == -1 and call(n=65) == -1 and call(n=-3) == -1
    assert call(stride=field - 1) == -1 and call(stride=0) == -1
    for name in ("B", "C", "H", "W"):
        assert call(**{name: 0}) == -1 and call(**{name: -1}) == -1
    assert call(Ht=H - 1) == -1 and call(Wt=W - 1) == -1
    assert call(B=256, C=256, stride=256 * 256 * H * W) == -1       # B * C > 65535
    assert call(levels=None) == -1 and call(Q=0) == -1 and call(Q=17) == -1
    x = torch.zeros(4, 1, 1, 4, 4)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.ensemble_scores(x, x[0])
    with pytest.raises(_hip.HipBackendError, match=r"\[N,B,C,H,W\]"):
        _hip.ensemble_scores(x[0], x[0])


def test_functions_refuse_a_wrong_prediction_by_name():
    from climate_learn.metrics import functional as fn
    y = torch.zeros(1, 1, 4, 4)
    normal = torch.distributions.Normal(y, y + 1)
    for bad in (y, normal, [y, y], None):
        for call in (lambda p: fn.ensemble_crps(p, y), lambda p: fn.ensemble_spread_skill_ratio(p, y),
                     lambda p: fn.ensemble_crps_field(p, y), lambda p: fn.ensemble_rank_histogram(p, y),
                     lambda p: fn.ensemble_quantiles(p, [0.5])):
            with pytest.raises(TypeError, match=r"EnsembleMembers or an \[N, B, C, H, W\] fp32 device tensor"):
                call(bad)


def test_reductions_from_fabricated_sums(monkeypatch):
    """_hip.ensemble_scores replaced by fabricated outputs: the host algebra of every ensemble_* function against its formula"""
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    from climate_learn.utils import EnsembleMembers
    N, B, C, H, W = 5, 2, 3, 4, 6
    rng = np.random.default_rng(2)
    sums = torch.from_numpy(rng.random((B, C, 4)) * 50 + 1)
    hist = torch.from_numpy(rng.integers(0, 9, (B, C, N + 1)))
    seen = []

    def fake(members, target, lat_w=None, **kw):
        seen.append((tuple(members.shape), None if lat_w is None else tuple(lat_w.shape), kw))
        return {"sums": sums, "hist": hist, "crps_field": "field", "quantiles": "quant"}

    monkeypatch.setattr(_hip, "ensemble_scores", fake)
    stack, y = torch.zeros(N, B, C, H, W), torch.zeros(B, C, H + 2, W + 1)
    s, n = sums.numpy(), H * W * B
    for pred in (stack, EnsembleMembers(stack)):
        for fair, pairs in ((False, N * N), (True, N * (N - 1))):
            want = (s[..., 0] - s[..., 1] / pairs).sum(0) / n
            got = fn.ensemble_crps(pred, y, fair=fair)
            assert got.dtype == torch.float32 and got.shape == (C + 1,)
            assert np.allclose(got.numpy(), np.append(want, want.mean()), rtol=1e-6)
            assert np.allclose(float(fn.ensemble_crps(pred, y, True, None, fair)), want.mean(), rtol=1e-6)
        var, err = s[..., 3].sum(0), s[..., 2].sum(0)
        want = np.append(np.sqrt(var / n) / np.sqrt(err / n), np.sqrt(var.sum() / (n * C)) / np.sqrt(err.sum() / (n * C)))
        assert np.allclose(fn.ensemble_spread_skill_ratio(pred, y).numpy(), want, rtol=1e-6)
        assert np.allclose(float(fn.ensemble_spread_skill_ratio(pred, y, True)), want[-1], rtol=1e-6)
        h = fn.ensemble_rank_histogram(pred, y, seed=9)
        assert h.dtype == torch.int64 and h.shape == (C + 1, N + 1)
        assert np.array_equal(h[:-1].numpy(), hist.numpy().sum(0)) and np.array_equal(h[-1].numpy(), hist.numpy().sum((0, 1)))
        assert seen[-1][2] == dict(sums=False, hist=True, seed=9)
        assert fn.ensemble_crps_field(pred, y, fair=True) == "field" and seen[-1][2] == dict(sums=False, crps_field="fair")
        assert fn.ensemble_crps_field(pred, y) == "field" and seen[-1][2] == dict(sums=False, crps_field="empirical")
        assert fn.ensemble_quantiles(pred, [0.1, 0.9]) == "quant" and seen[-1][2] == dict(sums=False, quantiles=[0.1, 0.9])
    # latitude weights reach the kernel cropped to the prediction's rows
    fn.ensemble_crps(stack, y, lat_weights=torch.ones(1, 1, H + 2, 1))
    assert seen[-1][1] == (H,)
