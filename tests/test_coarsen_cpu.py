"""CPU checks of the consistency training loss: the window facts the adjoint kernel of the antialiased resample
is built on, its dense numpy statement against CPU autograd of F.interpolate(antialias=True), the fp32 emulation of the stated
order against float64 (where the GPU test's bound comes from), the refusals of the C entry at the transposed mode codes, the
binding against the stub library, and the loss objects with their wiring into training_step.

Bound the GPU test uses (tests/coarsen_ref.py): |kernel - adjoint64| <= min(4 x the emulation's worst, the ceiling) * max|g|, the
emulation's worst being 0.34 / 0.53 ulp (bilinear / bicubic) and the ceiling (3 + 3) S^2 u / (5 + 5) S^2 u with S = 1."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import coarsen_ref as C
from tests import resample_aa_ref as A
from tests import resample_ref as R
from tests import test_binding_cpu as TB
from tests import test_resample_cpu as TR
from tests.conftest import ROOT

hip = TB.hip                                        # the stub-library fixture of the binding tests


def test_constants_match_the_header():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+ORBIT2_AT_(\w+)\s+(\d+)", hdr, flags=re.M)}
    assert d == {"TILE_H": C.TILE_H, "TILE_W": C.TILE_W, "COVER": C.COVER}
    assert _hip.RESAMPLE_ADJOINT_TILE == (C.TILE_H, C.TILE_W)
    assert int(re.search(r"^#define\s+ORBIT2_TRANSPOSE\s+(\d+)", hdr, flags=re.M).group(1)) == C.TRANSPOSE == _hip.TRANSPOSE == 16
    assert "the mode values 21 and 22" in hdr                             # the ABI-8 comment's list of additions
    assert int(re.search(r"^#define\s+ORBIT2_ABI_VERSION\s+(\d+)", hdr, flags=re.M).group(1)) == 8
    assert max(C.MAX_COVER.values()) == C.COVER


def test_window_facts():
    """what the adjoint kernel rests on, for every n_out <= n_in <= 160 and the named pairs: a fine coordinate lies in at most 3
    (bilinear) / 5 (bicubic) windows and in at least one, and lo and lo + n do not decrease with o"""
    pairs = [(i, o) for i in range(1, 161) for o in range(1, i + 1)] + list(C.NAMED_PAIRS)
    for mode in C.MODES:
        most, least = 0, 1 << 30
        for n_in, n_out in pairs:
            lo, n, _, _ = A.windows(mode, n_in, n_out)
            assert (np.diff(lo) >= 0).all() and (np.diff(lo + n) >= 0).all(), (mode, n_in, n_out)
            c = C.cover(mode, n_in, n_out)
            most, least = max(most, int(c.max())), min(least, int(c.min()))
        print("%s: a fine coordinate lies in %d .. %d windows" % (mode, least, most))
        assert least == 1 and most == C.MAX_COVER[mode]
    # cover() counts what member() states
    assert np.array_equal(C.cover("bicubic", 23, 10), C.member("bicubic", 23, 10).sum(0))


COARSENING = [(hw, HW) for hw, HW in A.SHAPES if HW[0] <= hw[0] and HW[1] <= hw[1]]      # resample_aa_ref: source, then result


@pytest.mark.parametrize("fine,coarse", COARSENING, ids=lambda v: "x".join(map(str, v)))
def test_dense_adjoint_against_autograd(fine, coarse):
    """the dense adjoint in float32 against CPU autograd of F.interpolate(antialias=True): PyTorch's definition of the backward"""
    pair = R.case_key(fine, coarse)
    g = R.make_input(coarse, 1, 2, seed=coarse[0] * 1000 + coarse[1] + 17)
    for mode in C.MODES:
        x = torch.zeros(1, 2, *fine, requires_grad=True)
        Fn.interpolate(x, coarse, mode=mode, align_corners=False, antialias=True).backward(torch.from_numpy(g))
        d = C.dense(mode, fine[0], coarse[0]).T[None, None] @ g @ C.dense(mode, fine[1], coarse[1])[None, None]
        assert d.dtype == np.float32
        e = float(np.abs(d - x.grad.numpy()).max() / np.abs(g).max())
        print("%s %s: |dense adjoint - autograd| / max|g| = %.4g" % (pair, mode, e))
        if fine == coarse:
            assert np.array_equal(d, g) and np.array_equal(x.grad.numpy(), g)           # the identity is exact
        else:
            assert e <= 4 * C.AUTOGRAD_MEASURED[(pair, mode)]
        # and the float64 statement is the same operator
        assert np.abs(C.adjoint64(g, fine, mode) - d).max() <= 16 * R.ULP * np.abs(g).max()


def test_adjoint_is_the_transpose_of_the_replica():
    """<A p, g> = <p, A^T g> in float64 with resample_aa_ref.replica_aa as A: the dense matrices state the forward's windows"""
    for fine, coarse in (((40, 56), (5, 7)), ((17, 23), (6, 10)), ((33, 65), (13, 27))):
        p = R.make_input(fine, 2, 3, seed=3)
        g = C.gpu_input(coarse, 0.0)
        for mode in C.MODES:
            lhs = float((A.replica_aa(p, coarse, mode) * g).sum())
            rhs = float((p.astype(np.float64) * C.adjoint64(g, fine, mode)).sum())
            assert abs(lhs - rhs) <= 1e-12 * float(np.abs(p).sum() * np.abs(g).max())


def test_emulation_against_adjoint64():
    """the stated fp32 order against float64, in units of max|g|, over the GPU cases at offsets 0 and 280: the worst per mode is
    under the derivable ceiling and is what coarsen_ref.ADJ_EMUL_WORST records for the GPU bound; the identity is exact; the
    largest column sum of |weight| is what the ceiling assumes"""
    worst, colsum = dict.fromkeys(C.MODES, 0.0), dict.fromkeys(C.MODES, 0.0)
    for fine, coarse in C.GPU_CASES:
        for mode in C.MODES:
            for ax in (0, 1):
                s = float(np.abs(C.dense(mode, fine[ax], coarse[ax]).astype(np.float64)).sum(0).max())
                colsum[mode] = max(colsum[mode], s)
            for off in C.OFFSETS:
                g = C.gpu_input(coarse, off)
                emu = C.emulate_adjoint(g, fine, mode)
                if fine == coarse:
                    assert np.array_equal(emu, g)
                e = float(np.abs(emu.astype(np.float64) - C.adjoint64(g, fine, mode)).max() / np.abs(g).max())
                assert e <= C.ceiling(mode), (fine, coarse, mode, off)
                worst[mode] = max(worst[mode], e)
    print("emulation worst / ulp(max|g|):", {k: round(v / C.ULP, 3) for k, v in worst.items()}, "column sums:", colsum)
    for mode in C.MODES:
        assert 0.5 * C.ADJ_EMUL_WORST[mode] <= worst[mode] <= C.ADJ_EMUL_WORST[mode]
        assert colsum[mode] <= C.COLSUM[mode]
        assert C.field_tol(mode) == min(4 * C.ADJ_EMUL_WORST[mode], C.ceiling(mode))
    assert C.ceiling("bilinear") == 6 * C.ULP and C.ceiling("bicubic") == 10 * C.ULP


# ---- the C entry refuses before any launch: addresses that are never dereferenced ----------------------------------------------
def _adj(**kw):
    """a valid adjoint call of tests/test_resample_cpu._fwd's shapes (x the 5 x 7 gradient, out the 40 x 56 result) but for `kw`"""
    return TR._fwd(**dict(dict(idx=None, ctot=3, sc=None, sh=None), **kw))


@pytest.mark.parametrize("mode", [16, 17, 18, 20, 23, 21 | 8, 22 | 8, 21 | 32, 16 | 6 | 64])
def test_entry_refuses_transpose_with_another_base(mode):
    assert _adj(mode=mode) == -1
    assert TR._fwd(mode=mode) == -1 and TR._mom(mode=mode) == -1


@pytest.mark.parametrize("mode", [21, 22])
def test_entry_refuses_bad_arguments_at_the_transposed_modes(mode):
    assert _adj(mode=mode, h=41) == -1 and _adj(mode=mode, w=57) == -1                   # an upsampling pair
    assert _adj(mode=mode, h=41, w=57) == -1
    assert _adj(mode=mode, idx=TR.IDX) == -1 and _adj(mode=mode, idx=TR.IDX, ctot=5) == -1
    assert _adj(mode=mode, ctot=5) == -1 and _adj(mode=mode, ctot=2) == -1
    assert _adj(mode=mode, sc=TR.SC, sh=TR.SH) == -1 and _adj(mode=mode, sc=TR.SC) == -1 and _adj(mode=mode, sh=TR.SH) == -1
    for bad in (b for b in TR.BAD if "mode" not in b):
        assert TR._fwd(**dict(bad, mode=mode)) == -1, bad
        if bad not in (dict(sc=None), dict(sh=None), dict(idx=None)):     # (what the valid adjoint call passes already)
            assert _adj(**dict(bad, mode=mode)) == -1, bad
    # the moments entry has no transposed form
    assert TR._mom(mode=mode) == -1 and TR._mom(mode=mode, idx=None, ctot=3, sc=None, sh=None) == -1


# ---- the binding, against the stub library of tests/test_binding_cpu.py ------------------------------------------------------
@pytest.mark.parametrize("mode,code", [("bilinear", 21), ("bicubic", 22)])
def test_resample_adjoint_reaches_the_entry_with_its_mode_code(hip, mode, code):
    g = TB.t(TB.F32, 2, 3, 4, 6)
    out = hip.resample_adjoint(g, (16, 24), mode)
    assert tuple(out.shape) == (2, 3, 16, 24) and out.dtype == torch.float32
    (entry, args), = hip.stub.calls
    assert entry == "orbit2_resample_fwd"
    assert args[-1] == TB.STREAM and args[-2] == code
    # x, chan_idx, in_ctotal, scale, shift, out, B, C, h, w, H, W
    assert args[:12] == (g.data_ptr(), None, 3, None, None, out.data_ptr(), 2, 3, 4, 6, 16, 24)


def test_resample_adjoint_operand_refusals(hip):
    g = TB.t(TB.F32, 2, 3, 4, 6)
    host = g.clone()
    host.flagged_host = True
    with pytest.raises(hip.HipBackendError, match="GPU tensor"):
        hip.resample_adjoint(host, (16, 24))
    with pytest.raises(hip.HipBackendError, match="float32"):
        hip.resample_adjoint(g.double(), (16, 24))
    with pytest.raises(hip.HipBackendError, match="contiguous"):
        hip.resample_adjoint(TB.t(TB.F32, 2, 3, 6, 4).transpose(2, 3), (16, 24))
    for size in ((3, 24), (16, 5), (3, 5)):
        with pytest.raises(hip.HipBackendError, match="coarsening"):
            hip.resample_adjoint(g, size)
    for mode in ("nearest", "area", 1):
        with pytest.raises(hip.HipBackendError, match="bilinear or bicubic"):
            hip.resample_adjoint(g, (16, 24), mode)
    with pytest.raises(hip.HipBackendError):
        hip.resample_adjoint(g[0], (16, 24))
    with pytest.raises(hip.HipBackendError, match="size"):
        hip.resample_adjoint(g, 16)
    assert hip.stub.calls == []
    hip.resample_adjoint(g, (4, 6))                                       # the identity is a coarsening
    assert hip.stub.calls[0][1][-2] == 21
    # what stays as it was
    assert hip.RESAMPLE_MODES == {"nearest": 0, "bilinear": 1, "bicubic": 2} and hip.ANTIALIAS == 4


def test_coarsen_fn_calls_the_two_kernels(hip):
    """forward: the antialiased resample of the detached prediction; backward: the adjoint at the prediction's size"""
    from climate_learn import _ops
    pred = torch.zeros(2, 3, 16, 24, requires_grad=True)
    out = _ops.CoarsenFn.apply(pred * 1.0, (4, 6), "bicubic")
    assert tuple(out.shape) == (2, 3, 4, 6) and out.requires_grad
    out.backward(torch.ones_like(out))
    assert [(n, a[-2], a[6:12]) for n, a in hip.stub.calls] == [("orbit2_resample_fwd", 6, (2, 3, 16, 24, 4, 6)),
                                                                 ("orbit2_resample_fwd", 22, (2, 3, 4, 6, 16, 24))]
    assert tuple(pred.grad.shape) == (2, 3, 16, 24)
    # _hip.resample itself still refuses a field that requires grad
    with pytest.raises(hip.HipBackendError, match="requires grad"):
        hip.resample(pred, (4, 6), "bilinear", antialias=True)


# ---- the loss objects -----------------------------------------------------------------------------------------------------------
IN_VARS = ["land_sea_mask", "2m_temperature", "total_precipitation_24hr", "2m_temperature_min"]
OUT_VARS = ["total_precipitation_24hr", "2m_temperature_min", "land_sea_mask"]


def _meta(out_vars=OUT_VARS):
    from climate_learn.metrics.utils import MetricsMetaInfo
    return MetricsMetaInfo(IN_VARS, out_vars, np.linspace(-60, 60, 16), np.arange(24), None)


@pytest.mark.parametrize("name,base", [("mse_consistency", "mse"), ("bayesian_tv_consistency", "bayesian_tv")])
def test_registered_losses(name, base):
    import climate_learn as cl
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.metrics import Metric
    from climate_learn.metrics.utils import METRICS_REGISTRY
    obj = cl.load_loss("cpu", None, name, True, _meta())
    assert type(obj) is METRICS_REGISTRY[name] and isinstance(obj, Metric) and obj.name == name and obj.aggregate_only
    assert obj.takes_source is True and obj.graph_capturable is True
    assert obj.weight == 1.0 and obj.mode == "bilinear"
    assert type(obj)._base is getattr(fn, base)
    for plain in ("mse", "bayesian_tv", "lat_mse", "masked_mse"):
        assert not getattr(METRICS_REGISTRY[plain], "takes_source", False)
    # set_rescale keeps the pair as plain numbers (uploaded once, cached); None clears it
    assert obj.set_rescale([2.0, 1.0, 1.0], [0.5, 0.0, 0.0]) is obj and obj._rescale == ((2.0, 1.0, 1.0), (0.5, 0.0, 0.0))
    assert obj.set_rescale(None, None)._rescale is None
    x = torch.zeros(2, 4, 4, 6)
    assert obj.set_source(x, tuple(IN_VARS)) is obj and obj._source is x and obj._in_variables == IN_VARS
    # a second instance does not see the first one's source
    assert cl.load_loss("cpu", None, name, True, _meta())._source is None


def test_loss_calls_and_messages(monkeypatch):
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics import metrics as M
    from climate_learn.models.hub import Resampled
    pred, target, x = torch.zeros(2, 3, 16, 24), torch.zeros(2, 3, 16, 24), torch.zeros(2, 4, 4, 6)
    obj = M.MSEConsistency(metainfo=_meta())
    with pytest.raises(RuntimeError, match="set_source"):
        obj(pred, target, var_names=OUT_VARS)
    obj.set_source(x, IN_VARS)
    with pytest.raises(RuntimeError, match="consistency_scores requires the output variables to be among the input variables."):
        obj(pred, target, var_names=["orography"] + OUT_VARS[1:])
    # what reaches the functionals: the base loss as it is, the term with the gathered channels, the constant's weight 0
    seen = {}

    def base(p, t, names, weights, agg):
        seen["base"] = (names, weights, agg)
        return torch.tensor([1.0, 2.0, 3.0, 4.0])

    def term(p, s, names, weights, agg, lat, mode, channels, rescale):
        seen["term"] = (s, names, weights, agg, lat, mode, channels, rescale)
        return torch.tensor([10.0, 20.0, 30.0, 40.0])

    monkeypatch.setattr(M.MSEConsistency, "_base", staticmethod(base))
    monkeypatch.setattr(fn, "consistency_mse", term)
    obj.weight, obj.mode = 0.5, "bicubic"
    obj.set_rescale([1.0, 2.0, 1.0], [0.0, 3.0, 0.0])
    vw = {"2m_temperature_min": 10, "land_sea_mask": 7}
    assert obj(pred, target, var_names=OUT_VARS, var_weights=vw).tolist() == [6.0, 12.0, 18.0, 24.0]
    assert seen["base"] == (OUT_VARS, vw, False)
    assert seen["term"] == (x, OUT_VARS, {"total_precipitation_24hr": 1.0, "2m_temperature_min": 10.0, "land_sea_mask": 0.0},
                            False, None, "bicubic", [2, 3, 0], ((1.0, 2.0, 1.0), (0.0, 3.0, 0.0)))
    obj.aggregate_only = True
    assert float(obj(pred, target, var_names=OUT_VARS)) == 24.0
    # the functional's own refusals, by name, before any kernel
    monkeypatch.undo()
    with pytest.raises(ValueError, match="does not coarsen onto"):
        fn.consistency_mse(torch.zeros(2, 3, 3, 24), x, channels=[0, 1, 2])              # 3 // 4 = 0: finer than the prediction
    with pytest.raises(ValueError, match="does not coarsen onto"):
        fn.consistency_mse(torch.zeros(2, 3, 16, 32), x, channels=[0, 1, 2])             # 32 // 4 = 8 columns onto 6
    with pytest.raises(TypeError, match="Resampled"):
        fn.consistency_mse(Resampled(torch.zeros(2, 3, 4, 6), (16, 24)), x)
    with pytest.raises(ValueError, match="channels"):
        fn.consistency_mse(pred, x, channels=[0, 1, 4])
    with pytest.raises(ValueError, match="name them with `channels`"):
        fn.consistency_mse(pred, x)


class _Recorder:
    """a loss as training_step sees one: records its calls"""

    def __init__(self):
        self.calls = []

    def __call__(self, pred, target, var_names=None, var_weights=None):
        self.calls.append(("call", var_names, var_weights))
        return pred.sum().reshape(1)


class _SourceRecorder(_Recorder):
    takes_source = True

    def set_source(self, x, in_variables):
        self.calls.append(("set_source", x, in_variables))


def test_training_step_hands_the_source_to_a_loss_that_takes_it(monkeypatch):
    from climate_learn import trainer
    monkeypatch.setattr(trainer, "clip_replace_constant", lambda y, yhat, out_variables: yhat)
    net = SimpleNamespace(forward=lambda x, iv, ov: x[:, :1] * 2.0)
    x, y = torch.ones(2, 4, 4, 6), torch.zeros(2, 1, 4, 6)
    batch = (x, y, IN_VARS, OUT_VARS[:1])
    plain = _Recorder()
    assert float(trainer.training_step(batch, 0, net, "cpu", {"a": 1.0}, plain)) == 96.0
    assert plain.calls == [("call", OUT_VARS[:1], {"a": 1.0})] and not hasattr(plain, "_source")
    taking = _SourceRecorder()
    assert float(trainer.training_step(batch, 0, net, "cpu", None, taking)) == 96.0
    assert [c[0] for c in taking.calls] == ["set_source", "call"]
    assert taking.calls[0][1].data_ptr() == x.data_ptr() and taking.calls[0][2] == IN_VARS


def test_loader_sets_the_rescale(monkeypatch):
    from climate_learn.utils import loaders
    norm = lambda m, s: SimpleNamespace(mean=m, std=s)                    # noqa: E731
    tin = {"2m_temperature_min": norm(280.0, 20.0), "land_sea_mask": norm(0.3, 0.4), "total_precipitation_24hr": object()}
    tout = {"2m_temperature_min": norm(270.0, 10.0), "land_sea_mask": norm(0.3, 0.4), "total_precipitation_24hr": object()}

    def dm(out_vars):
        return SimpleNamespace(get_data_variables=lambda: (IN_VARS, out_vars), get_lat_lon=lambda: (np.arange(4.0), np.arange(6.0)),
                               get_climatology=lambda split: torch.zeros(len(out_vars), 4, 6), transforms=tin,
                               output_transforms=tout)

    model = torch.nn.Identity()
    out = loaders.load_model_module("cpu", dm(OUT_VARS), "downscaling", model=model, train_loss="bayesian_tv_consistency")
    assert out[1].takes_source and out[1]._rescale == ((1.0, 2.0, 1.0), (0.0, 1.0, 0.0))
    plain = loaders.load_model_module("cpu", dm(OUT_VARS), "downscaling", model=model, train_loss="bayesian_tv")[1]
    assert not hasattr(plain, "_rescale")
    with pytest.raises(RuntimeError, match="consistency_scores requires the output variables to be among the input variables."):
        loaders.load_model_module("cpu", dm(["orography"]), "downscaling", model=model, train_loss="mse_consistency")


def test_config_names_the_loss():
    import yaml
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m_consistency.yaml")))
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    assert conf["trainer"]["train_loss"] == "bayesian_tv_consistency"
    assert conf["trainer"].pop("consistency") == {"weight": 1.0, "mode": "bilinear"}
    conf["trainer"]["train_loss"] = base["trainer"]["train_loss"]
    assert conf == base
