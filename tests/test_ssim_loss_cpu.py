"""CPU checks of the SSIM training loss: the header's closed form against float64 autograd; the fp32 emulation of
the kernel against float64, which is where the GPU tests' field tolerance comes from; the C entry's refusals before any launch;
the binding against the stub library of tests/test_binding_cpu.py; the registry names, the driver's `trainer.ssim` block and the
config."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import ssim_loss_ref as S
from tests import test_binding_cpu as TB
from tests.conftest import ROOT

hip = TB.hip                                        # the stub-library fixture of the binding tests


def test_constants_match_the_header():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+ORBIT2_SSIM_VJP_(\w+)\s+(\d+)", hdr, flags=re.M)}
    assert d == {"TILE_H": S.TILE_H, "TILE_W": S.TILE_W}
    assert _hip.SSIM_VJP_TILE == (S.TILE_H, S.TILE_W) and _hip.SSIM_WIN == S.WIN
    assert int(re.search(r"^#define\s+ORBIT2_LOSS_SSIM_VJP\s+(\d+)", hdr, flags=re.M).group(1)) == S.LOSS_SSIM_VJP == _hip.LOSS_SSIM_VJP
    assert "the kind\n * value 3 of orbit2_loss_bwd" in hdr                 # the ABI-8 comment's list of additions
    assert int(re.search(r"^#define\s+ORBIT2_ABI_VERSION\s+(\d+)", hdr, flags=re.M).group(1)) == 8 == _hip.ABI_VERSION


def _pair(hw, offset):
    return S.make_pair(hw, (hw[0] + 2, hw[1] + 4), offset)


@pytest.fixture(scope="module")
def refs():
    """(pred, target, lat_w, vjp64) per (shape, offset, with lat_w): computed once, read by the tests below"""
    out = {}
    for hw in S.TOL_SHAPES:
        for off in S.OFFSETS:
            pred, target = _pair(hw, off)
            for lat in (False, True):
                lw = S.lat_weights(hw[0]) if lat else None
                out[hw, off, lat] = (pred, target, lw, S.vjp64(pred, target, lw, S.GPU_COEF, S.GPU_RANGE))
    return out


def test_closed_form_against_float64_autograd(refs):
    """the header's formula, five box sums and a pivot, is the gradient: to 1e-10 of max|d|, at offset 280 too, for two pivots"""
    for (hw, off, lat), (pred, target, lw, want) in refs.items():
        if off != 280.0:
            continue
        for b in range(S.GPU_B):
            for c in range(S.GPU_C):
                y = target[b, c, :hw[0], :hw[1]]
                for pivot in (None, float(y.mean()) + 1.0):
                    got = S.closed_form64(pred[b, c], y, S.GPU_RANGE[b][c], lw, S.GPU_COEF[b][c], pivot)
                    e = np.abs(got - want[b, c]).max() / np.abs(want[b, c]).max()
                    assert e <= 1e-10, (hw, lat, b, c, pivot, e)


def test_emulation_against_float64(refs):
    """the kernel's fp32 order against float64, relative to max|d| of the image, over TOL_SHAPES at offsets 0 and 280 with and
    without lat_w: the worst is what ssim_loss_ref.EMUL_WORST records, and the GPU bound is 4 x that.  Offset 280 is no worse
    than offset 0 by more than the bracket: the centring holds."""
    worst = {off: 0.0 for off in S.OFFSETS}
    for (hw, off, lat), (pred, target, lw, want) in refs.items():
        emu = S.emulate(pred, target, lw, S.GPU_COEF, S.GPU_RANGE)
        assert emu.dtype == np.float32 and np.isfinite(emu).all()
        worst[off] = max(worst[off], S.worst_error(emu, want))
    print("emulation worst / max|d|:", worst)
    assert 0.5 * S.EMUL_WORST <= max(worst.values()) <= S.EMUL_WORST
    assert min(worst.values()) >= 0.5 * max(worst.values())
    assert S.FIELD_TOL == 4 * S.EMUL_WORST


def test_emulation_skips_an_image_of_coefficient_zero():
    pred, target = _pair((13, 9), 0.0)
    pred[0, 1, 4, 4] = np.nan
    target[0, 1] = 3.0
    coef = ((0.75, 0.0, 2.0), (0.03125, 1.0, -0.5))
    rng = ((5.0, 0.0, 6.5), (3.5, 8.0, 5.5))
    emu = S.emulate(pred, target, None, coef, rng)
    assert not emu[0, 1].any() and np.isfinite(emu).all()
    assert S.worst_error(emu, S.vjp64(pred, target, None, coef, rng)) <= S.EMUL_WORST


def test_design_records_the_tolerance():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%.1e" % S.EMUL_WORST in text and "%.2e" % S.FIELD_TOL in text


# ---- the C entry refuses before any launch: addresses that are never dereferenced ----------------------------------------------
def test_entry_refuses_bad_arguments_without_a_gpu():
    from climate_learn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    names = ("pred", "target", "Ht", "Wt", "lat", "cw", "gscale", "dpred", "B", "C", "H", "W", "kind", "s")
    valid = dict(pred=a, target=a, Ht=8, Wt=8, lat=None, cw=None, gscale=a, dpred=a, B=1, C=1, H=8, W=8, kind=S.LOSS_SSIM_VJP, s=None)
    bwd = lambda **k: lib.orbit2_loss_bwd(*[{**valid, **k}[n] for n in names])
    for bad in (dict(cw=a), dict(H=6), dict(W=6), dict(H=6, W=6), dict(B=256, C=256), dict(B=65536), dict(pred=None),
                dict(target=None), dict(gscale=None), dict(dpred=None), dict(B=0), dict(C=0), dict(Ht=7), dict(Wt=7),
                dict(kind=4), dict(kind=-1), dict(kind=4, cw=a), dict(cw=a, lat=a)):
        assert bwd(**bad) == -1, bad
    # the forward of this loss is orbit2_ssim: orbit2_loss_fwd has no kind 3
    for kind in (3, 4, -1):
        assert lib.orbit2_loss_fwd(a, a, 8, 8, None, None, a, a, 1, 1, 8, 8, kind, None) == -1
    assert not any(buf)


# ---- the binding, against the stub library of tests/test_binding_cpu.py ------------------------------------------------------
def _operands(B=2, C=3, H=9, W=12):
    return (TB.t(TB.F32, B, C, H, W), TB.t(TB.F32, B, C, H + 1, W + 2), TB.t(TB.F32, H), torch.ones(B, C), torch.full((B, C), 5.0))


def test_ssim_vjp_reaches_loss_bwd_with_kind_3(hip, monkeypatch):
    pred, target, lat_w, coef, rng = _operands()
    coef[1, 2], rng[0, 1] = -2.0, 7.0
    seen = []
    call = hip._call
    monkeypatch.setattr(hip, "_call", lambda name, *args: (seen.append(args), call(name, *args))[1])
    for lw in (lat_w, None):
        del hip.stub.calls[:], seen[:]
        out = hip.ssim_vjp(pred, target, lw, coef, rng)
        assert tuple(out.shape) == (2, 3, 9, 12) and out.dtype == torch.float32
        (entry, args), = hip.stub.calls
        assert entry == "orbit2_loss_bwd" and args[-1] == TB.STREAM and args[-2] == 3
        gscale = seen[0][6]
        assert args[:12] == (pred.data_ptr(), target.data_ptr(), 10, 14, None if lw is None else lw.data_ptr(), None,
                             gscale.data_ptr(), out.data_ptr(), 2, 3, 9, 12)
        assert gscale.dtype == torch.float32 and gscale.is_contiguous() and gscale.numel() == 2 * 2 * 3
        assert torch.equal(gscale.reshape(2, -1)[0], coef.reshape(-1)) and torch.equal(gscale.reshape(2, -1)[1], rng.reshape(-1))


def test_ssim_vjp_operand_refusals(hip):
    pred, target, lat_w, coef, rng = _operands()
    for i in range(5):
        ops = [pred, target, lat_w, coef, rng]
        ops[i] = ops[i].clone()
        ops[i].flagged_host = True
        with pytest.raises(hip.HipBackendError, match="GPU tensor"):
            hip.ssim_vjp(*ops)
        ops[i] = ops[i].double()
        with pytest.raises(hip.HipBackendError, match="float32"):
            hip.ssim_vjp(*ops)
    with pytest.raises(hip.HipBackendError, match="contiguous"):
        hip.ssim_vjp(TB.t(TB.F32, 2, 3, 12, 9).transpose(2, 3), target, lat_w, coef, rng)
    with pytest.raises(hip.HipBackendError, match="smaller than the prediction"):
        hip.ssim_vjp(pred, target[..., :8, :].contiguous(), lat_w, coef, rng)
    with pytest.raises(hip.HipBackendError, match="lat_w has 8 entries"):
        hip.ssim_vjp(pred, target, lat_w[:8].clone(), coef, rng)
    with pytest.raises(hip.HipBackendError, match="at least 7 x 7"):
        hip.ssim_vjp(pred[..., :6, :].contiguous(), target, None, coef, rng)
    for bad in (coef[0], torch.ones(3, 2), 1.0):
        with pytest.raises(hip.HipBackendError, match=r"\[B,C\]"):
            hip.ssim_vjp(pred, target, lat_w, bad, rng)
        with pytest.raises(hip.HipBackendError, match=r"\[B,C\]"):
            hip.ssim_vjp(pred, target, lat_w, coef, bad)
    assert hip.stub.calls == []
    # what stays as it was: the signatures of the two loss wrappers
    hip.loss_bwd(pred, target, None, None, torch.ones(1), 1)
    hip.loss_fwd(pred, target, None, None, 0)
    assert [(n, a[-2]) for n, a in hip.stub.calls] == [("orbit2_loss_bwd", 1), ("orbit2_loss_fwd", 0)]


@pytest.mark.parametrize("lat", [False, True])
def test_ssim_fn_calls_the_two_kernels(hip, lat):
    """forward: orbit2_ssim at the given range; backward: orbit2_loss_bwd at kind 3 with the saved operands"""
    from climate_learn import _ops
    pred, target, lat_w, _, rng = _operands()
    pred.requires_grad_(True)
    s = _ops.SSIMFn.apply(pred * 1.0, target, lat_w if lat else None, rng)
    assert tuple(s.shape) == (2, 3) and s.dtype == torch.float32 and s.requires_grad
    s.backward(torch.ones_like(s))
    (n0, a0), (n1, a1) = hip.stub.calls
    assert n0 == "orbit2_ssim" and a0[5] == rng.data_ptr() and a0[7] is None and a0[8:12] == (2, 3, 9, 12)
    assert n1 == "orbit2_loss_bwd" and a1[-2] == 3 and a1[5] is None and a1[8:12] == (2, 3, 9, 12)
    assert (a1[4] is None) == (not lat) and a1[:4] == a0[:4]
    assert tuple(pred.grad.shape) == (2, 3, 9, 12)


# ---- the loss objects, the driver, the config --------------------------------------------------------------------------------------
OUT_VARS = ["total_precipitation_24hr", "2m_temperature_min", "land_sea_mask"]


def _meta():
    from climate_learn.metrics.utils import MetricsMetaInfo
    return MetricsMetaInfo(OUT_VARS, OUT_VARS, np.linspace(-60, 60, 16), np.arange(24), None)


@pytest.mark.parametrize("name,base", [("ssim_loss", None), ("mse_ssim", "mse"), ("bayesian_tv_ssim", "bayesian_tv")])
def test_registered_losses(name, base):
    import climate_learn as cl
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.metrics import Metric
    from climate_learn.metrics.utils import METRICS_REGISTRY
    obj = cl.load_loss("cpu", None, name, True, _meta())
    assert type(obj) is METRICS_REGISTRY[name] and isinstance(obj, Metric) and obj.name == name and obj.aggregate_only
    assert obj.weight == 1.0 and obj.data_range == "target" and obj.graph_capturable is True
    assert not getattr(obj, "takes_source", False)
    assert type(obj)._base is (None if base is None else getattr(fn, base))
    for plain in ("mse", "bayesian_tv", "ssim", "lat_ssim"):
        assert not hasattr(METRICS_REGISTRY[plain], "data_range")
    assert cl.metrics.ssim_loss is fn.ssim_loss


def test_loss_calls_the_functional(hip, monkeypatch):
    """base + weight x ssim_loss, the term's operands, weight 0 = the base alone"""
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.utils import METRICS_REGISTRY
    calls = []

    def term(pred, target, var_names, var_weights, aggregate_only, lat_weights, data_range):
        calls.append((var_names, var_weights, aggregate_only, lat_weights, data_range))
        return torch.tensor([1.0, 2.0, 3.0, 2.0])

    monkeypatch.setattr(fn, "ssim_loss", term)
    pred, target = TB.t(TB.F32, 2, 3, 9, 12), TB.t(TB.F32, 2, 3, 9, 12)
    obj = METRICS_REGISTRY["ssim_loss"](metainfo=_meta())
    obj.weight, obj.data_range = 0.5, 4.0
    assert obj(pred, target, OUT_VARS, {"2m_temperature_min": 10}).tolist() == [0.5, 1.0, 1.5, 1.0]
    assert calls == [(OUT_VARS, {"2m_temperature_min": 10}, False, None, 4.0)]
    both = METRICS_REGISTRY["mse_ssim"](True, _meta())
    monkeypatch.setattr(type(both), "_base", staticmethod(lambda *a: torch.tensor([10.0, 20.0, 30.0, 20.0])))
    assert float(both(pred, target, OUT_VARS, None)) == 22.0
    both.weight = 0
    del calls[:]
    assert float(both(pred, target, OUT_VARS, None)) == 20.0 and calls == []


def test_ssim_loss_arguments():
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    pred, target = torch.zeros(2, 3, 9, 12), torch.zeros(2, 3, 9, 12)
    for bad in ("image", "Target", ""):
        with pytest.raises(ValueError, match="data_range is a number, a dict per variable or 'target'"):
            fn.ssim_loss(pred, target, OUT_VARS, None, False, None, bad)
    with pytest.raises(ValueError, match="needs var_names"):
        fn.ssim_loss(pred, target, None, None, False, None, {"a": 1.0})
    with pytest.raises(ValueError, match="missing: \\['land_sea_mask'\\]"):
        fn.ssim_loss(pred, target, OUT_VARS, None, False, None, {"total_precipitation_24hr": 1.0, "2m_temperature_min": 2.0})
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        fn.ssim_loss(pred[0], target[0])
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):          # no CPU path
        fn.ssim_loss(pred, target, OUT_VARS)
    rng = fn._ssim_loss_range({"total_precipitation_24hr": 1.0, "2m_temperature_min": 2.0, "land_sea_mask": 3.0}, OUT_VARS, pred)
    assert rng.tolist() == [[1.0, 2.0, 3.0]] * 2 and rng.is_contiguous()
    assert fn._ssim_loss_range(4, None, pred).tolist() == [[4.0] * 3] * 2
    assert fn._ssim_loss_range(4, None, pred) is fn._ssim_loss_range(4.0, OUT_VARS, pred)        # cached: one upload
    assert fn._ssim_loss_range("target", None, pred) is None


def _driver():
    spec = importlib.util.spec_from_file_location("intermediate_downscaling", os.path.join(ROOT, "examples", "intermediate_downscaling.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_reads_and_refuses_the_ssim_block():
    drv = _driver()
    from climate_learn.metrics.utils import METRICS_REGISTRY
    assert set(drv.SSIM_LOSSES) == {n for n, k in METRICS_REGISTRY.items() if hasattr(k, "data_range")}
    block = {"weight": 0.25, "data_range": 6.0}
    for name in drv.SSIM_LOSSES:
        assert drv.ssim_settings({"train_loss": name, "ssim": block}) == block
        assert drv.ssim_settings({"train_loss": name}) == {} and drv.ssim_settings({"train_loss": name, "ssim": None}) == {}
    for name in ("bayesian_tv", "mse", "bayesian_tv_consistency", "ssim"):
        assert drv.ssim_settings({"train_loss": name}) == {}
        with pytest.raises(ValueError, match="trainer.ssim goes with an SSIM loss .*not with train_loss '%s'" % name):
            drv.ssim_settings({"train_loss": name, "ssim": block})
    with pytest.raises(ValueError, match="trainer.ssim.data_range is a number, a dict per variable or 'target', got 'image'"):
        drv.ssim_settings({"train_loss": "mse_ssim", "ssim": {"data_range": "image"}})
    assert drv.ssim_settings({"train_loss": "mse_ssim", "ssim": {"data_range": "target"}}) == {"data_range": "target"}


def test_config_names_the_loss():
    import yaml
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m_ssim.yaml")))
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    assert conf["trainer"]["train_loss"] == "bayesian_tv_ssim"
    assert conf["trainer"].pop("ssim") == {"weight": 1.0, "data_range": "target"}
    conf["trainer"]["train_loss"] = base["trainer"]["train_loss"]
    assert conf == base
