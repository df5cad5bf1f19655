"""What can be checked without a device of the parts the scores share: the operand checks of a scored pair (_hip._scored_pair:
every wrapper refuses with the wording the wrappers' own tests pin) and the metric algebra that is stated once for the masked
and the unmasked sums (metrics.functional.pearson / mean_bias / mae)."""
import pytest
import torch


def test_every_scoring_wrapper_refuses_cpu_tensors():
    from climate_learn import _hip
    x = torch.zeros(2, 3, 8, 40)
    lat, cnt = torch.ones(8), torch.zeros(4, dtype=torch.int64)
    calls = {"eval_moments": lambda: _hip.eval_moments(x, x, lat, x[0]),
             "masked_loss_fwd": lambda: _hip.masked_loss_fwd(x, x, lat, None, 0),
             "masked_loss_bwd": lambda: _hip.masked_loss_bwd(x, x, lat, None, torch.ones(1), cnt, 0),
             "masked_moments": lambda: _hip.masked_moments(x, x, lat),
             "gaussian_scores": lambda: _hip.gaussian_scores(x, x, x, lat),
             "ensemble_scores": lambda: _hip.ensemble_scores(torch.stack((x, x)), x, lat),
             "ssim_sums": lambda: _hip.ssim_sums(x, x, lat),
             "resample_moments": lambda: _hip.resample_moments(x[:, :, :4, :20].contiguous(), (8, 40), "bilinear", x, lat_w=lat)}
    for name, call in calls.items():
        with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
            call()
    with pytest.raises(_hip.HipBackendError, match="at least 7 x 7"):          # a property of the call: before the device check
        _hip.ssim_sums(x[:, :, :6], x)


def test_scored_pair_wording(monkeypatch):
    """the shape checks behind the device check, with the fragments tests/test_*_gpu.py expect of the wrappers"""
    from climate_learn import _hip
    E = _hip.HipBackendError
    with pytest.raises(E, match="must be torch.float32"):
        _hip._dev(_FakeCuda(torch.float64), _hip.F32, "pred")
    monkeypatch.setattr(_hip, "_dev", lambda t, dtype, name: t)
    p, t = torch.zeros(2, 3, 8, 9), torch.zeros(2, 3, 10, 9)
    assert _hip._scored_pair("f", p, t, torch.ones(8), torch.zeros(3, 8, 9)) == (2, 3, 8, 9)
    assert _hip._scored_pair("f", (2, 3, 8, 9), t, torch.ones(9), torch.zeros(1, 3, 8, 9)) == (2, 3, 8, 9)
    for bad in (t[0], torch.zeros(8, 9)):
        with pytest.raises(E, match=r"f takes \[B,C,H,W\] fields"):
            _hip._scored_pair("f", p, bad)
    for bad in (t[:, :2], t[:1]):
        with pytest.raises(E, match=r"does not match the prediction's \[B,C\]"):
            _hip._scored_pair("f", p, bad)
    for bad in (t[:, :, :7], t[:, :, :, :8]):
        with pytest.raises(E, match="smaller than the prediction"):
            _hip._scored_pair("f", p, bad)
    with pytest.raises(E, match="lat_w has 4 entries"):
        _hip._scored_pair("f", p, t, torch.ones(4))
    for bad in (torch.zeros(3, 8, 8), torch.zeros(2, 8, 9), torch.zeros(2, 3, 8, 9)):
        with pytest.raises(E, match=r"climatology must be \[C,H,W\]"):
            _hip._scored_pair("f", p, t, None, bad)


class _FakeCuda:
    """what _dev looks at, of a device tensor of another dtype"""
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype


def test_masked_and_unmasked_forms_share_their_algebra(monkeypatch):
    """everything valid (s[..., 12] = H W): pearson, mean_bias and mae of the masked sums are those of the unmasked ones"""
    from climate_learn.metrics import functional as fn
    B, C, H, W = 3, 4, 5, 7
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(B, C, H, W, generator=g, dtype=torch.float64), torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.rand(H, generator=g, dtype=torch.float64).view(1, 1, H, 1) + 0.5
    d = a - b
    terms = (a, b, a * a, b * b, a * b, w * d * d, w * d.abs(), w * a, w * b, w * a * b, w * a * a, w * b * b)
    m12 = torch.stack([t.sum((2, 3)) for t in terms], -1)                       # [B,C,12]
    m13 = torch.cat((m12, torch.full((B, C, 1), float(H * W), dtype=torch.float64)), -1)
    monkeypatch.setattr(fn, "_moments", lambda pred, target, lat_weights=None, climatology=None: (m12, H * W))
    monkeypatch.setattr(fn, "_masked_sums", lambda pred, target, lat_weights=None, mask=None: m13)
    pred = torch.empty(B, C, H, W)
    want = {fn.pearson: [torch.corrcoef(torch.stack((a[:, c].flatten(), b[:, c].flatten())))[0, 1] for c in range(C)],
            fn.mean_bias: [(b[:, c] - a[:, c]).mean() for c in range(C)],
            fn.mae: [(w * d.abs())[:, c].mean() for c in range(C)]}
    for f, ref in want.items():
        plain, masked = f(pred, pred), f(pred, pred, mask=fn.TARGET_FINITE)
        assert plain.shape == (C + 1,) and plain.dtype == torch.float32
        assert torch.equal(plain, masked)                                        # same expression, same operands
        assert torch.allclose(plain[:C].double(), torch.stack(ref), rtol=1e-6, atol=1e-7)
        assert torch.equal(f(pred, pred, aggregate_only=True), plain[C])
    # the aggregate rules differ: a channel without data is skipped by the masked form and poisons the unmasked one
    m13[:, 1] = 0.0
    m12[:, 1] = float("nan")
    for f in want:
        masked, plain = f(pred, pred, mask=fn.TARGET_FINITE), f(pred, pred)
        assert torch.isnan(masked[1]) and torch.isfinite(masked[C]) and torch.isnan(plain[C])
