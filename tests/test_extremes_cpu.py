"""CPU checks of the extreme-value scores: the numpy replica of the digit-pass select against np.sort on the value
sets the GPU tests use; csrc/quantile_select.h through a stand-alone host program, plainly and under host sanitizers; the header's
constants and workspace macros against the binding's; the entry's refusals before any launch; the two wrappers against the stub
library of tests/test_binding_cpu.py; the host algebra of every functional from fabricated kernel outputs."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import extremes_ref as R
from tests import test_binding_cpu as TB
from tests.conftest import ROOT

hip = TB.hip                                        # the stub-library fixture of the binding tests
CSRC = os.path.join(ROOT, "orbit-2_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "orbit2_hip.h")


# ---- the select replica ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.VALUE_SETS)
def test_replica_equals_sorted_order_statistics(name):
    for n in (1, 7, 960, 5000):
        x = R.values(name, n, seed=n)
        s = np.sort(x, kind="stable")
        ranks = sorted({0, n - 1, n // 2, (n - 1) // 3} | {R.position(q, n)[k] for q in R.LEVELS for k in (0, 1)})
        got = R.select(x, ranks)
        assert got.dtype == np.float32 and np.array_equal(got, s[ranks]), (name, n)       # == : the sign of a zero is ignored
        both = s[ranks] != 0
        assert np.array_equal(got.view(np.uint32)[both], s[ranks].view(np.uint32)[both])  # data values bit for bit


def test_replica_on_hand_made_edges():
    one = np.array([-0.0], dtype=np.float32)
    assert R.select(one, [0]).view(np.uint32)[0] == 0x80000000                            # m = 1
    x = np.array([0.0, -0.0, 1e-45, -1e-45, R.FLT_MAX, -R.FLT_MAX], dtype=np.float32)
    got = R.select(x, range(6))
    assert got.view(np.uint32).tolist() == [0xff7fffff, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x7f7fffff]
    ulps = (np.float32(1.0).view(np.uint32) + np.arange(5, dtype=np.uint32)).view(np.float32)[::-1].copy()
    assert np.array_equal(R.select(ulps, range(5)), ulps[::-1])                           # 1 ulp apart
    assert np.array_equal(R.key(R.unkey(np.arange(0, 2 ** 32, 65521, dtype=np.uint64).astype(np.uint32))),
                          np.arange(0, 2 ** 32, 65521, dtype=np.uint64).astype(np.uint32))


def test_yardstick_brackets_and_linear_value():
    x = R.values("gauss280", 1001, seed=3)
    out, m = R.quantiles(x, np.ones(x.shape, bool), R.LEVELS)
    assert m == 1001 and out[0, 1] == x.min() == out[0, 0] and out[-1, 2] == x.max() == out[-1, 0]
    for j, q in enumerate(np.asarray(R.LEVELS, dtype=np.float32).astype(np.float64)):
        lo, hi, frac = R.position(q, m)
        s = np.sort(x).astype(np.float64)
        assert abs(out[j, 0] - (s[lo] + frac * (s[hi] - s[lo]))) <= 1e-12 * abs(out[j, 0])
    assert np.isnan(R.quantiles(x, np.zeros(x.shape, bool), R.LEVELS)[0]).all()


# ---- csrc/quantile_select.h on the host -----------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_program_of_the_select_header(tmp_path, sanitize):
    """key map, scan step and position arithmetic (tests/quantile_select_host.cpp): a program of its own, never Python code"""
    exe = str(tmp_path / "quantile_select_host")
    flags = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-w", "-I", CSRC] + flags +
                   [os.path.join(ROOT, "tests", "quantile_select_host.cpp"), "-o", exe], check=True, capture_output=True)
    if sanitize:
        assert b"__asan_init" in open(exe, "rb").read()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "quantile_select ok", r.stdout[-2000:] + r.stderr[-2000:]


# ---- header and binding -----------------------------------------------------------------------------------------------------------
def _macro(hdr, name):
    """(parameter names, body) of a function-like macro of the header"""
    m = re.search(r"^#define\s+%s\(([^)]*)\)\s+(.+)$" % name, hdr, flags=re.M)
    return [p.strip() for p in m.group(1).split(",")], m.group(2)


def _eval_macro(hdr, name, *args):
    params, body = _macro(hdr, name)
    body = body.replace("(long long)", "").replace("ORBIT2_LOSS_BLOCKS", "64")
    assert re.fullmatch(r"[\w\s()*+]+", body), body
    return eval(body, {"__builtins__": {}}, dict(zip(params, args)))


def test_header_constants_and_workspace_macros_match_the_binding():
    from climate_learn import _hip
    hdr = open(HEADER).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+ORBIT2_MASKED_(\w+)\s+(\d+)", hdr, flags=re.M)}
    assert d == {"QUANTILES": _hip.MASKED_QUANTILES, "TAIL": _hip.MASKED_TAIL, "PER_IMAGE": _hip.MASKED_PER_IMAGE,
                 "LOWER": _hip.MASKED_LOWER, "MAX_LEVELS": _hip.MASKED_MAX_LEVELS}
    assert (d["QUANTILES"], d["TAIL"], d["PER_IMAGE"], d["LOWER"], d["MAX_LEVELS"]) == (3, 4, 16, 32, 8)
    assert int(re.search(r"^#define\s+ORBIT2_LOSS_BLOCKS\s+(\d+)", hdr, flags=re.M).group(1)) == 64 == _hip.LOSS_BLOCKS
    for G, Q in ((1, 1), (3, 6), (48, 8), (5, 3)):
        assert _eval_macro(hdr, "ORBIT2_QUANTILE_WS_WORDS", G, Q) == _hip.quantile_ws_words(G, Q) > 0
    for B, C, T in ((1, 1, 1), (16, 3, 6), (2, 5, 8)):
        assert _eval_macro(hdr, "ORBIT2_TAIL_WS_WORDS", B, C, T) == _hip.tail_ws_words(B, C, T) > 0
    params, body = _macro(hdr, "ORBIT2_MASKED_KIND")
    assert params == ["kind", "flags", "n"] and body.replace(" ", "") == "((kind)|(flags)|((n)<<8))"
    # the ABI: version 8, the entry's prototype as it was, no new export and no query function for the workspaces
    assert int(re.search(r"^#define\s+ORBIT2_ABI_VERSION\s+(\d+)", hdr, flags=re.M).group(1)) == 8 == _hip.ABI_VERSION
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _hip.PROTOTYPES["orbit2_masked_loss_fwd"] == (I, (P, P, I, I, P, I, L, L, P, P, P, P, P, I, I, I, I, I, P))
    assert not [n for n in _hip.PROTOTYPES if "quantile" in n or "tail" in n or "extreme" in n]
    stripped = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert not re.search(r"\borbit2_\w*(quantile|tail_ws|extreme)\w*\s*\(", stripped)


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_kind_words_without_a_gpu():
    """every refusal returns before anything is launched or written; the addresses are never dereferenced"""
    from climate_learn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    names = ("pred", "target", "Ht", "Wt", "mask", "pitch", "sb", "sc", "lat", "cw", "out", "cnt", "ws", "B", "C", "H", "W", "kind", "s")
    base = dict(pred=a, target=a, Ht=8, Wt=8, mask=None, pitch=0, sb=0, sc=0, lat=None, cw=a, out=a, cnt=a, ws=a, B=1, C=1, H=8,
                W=8, kind=0, s=None)
    fwd = lambda **k: lib.orbit2_masked_loss_fwd(*[{**base, **k}[n] for n in names])
    kq = lambda n, flags=0: _hip.MASKED_QUANTILES | flags | (n << 8)
    kt = lambda n, flags=0: _hip.MASKED_TAIL | flags | (n << 8)
    bad = [dict(kind=kq(0)), dict(kind=kq(9)), dict(kind=kq(4), cw=None), dict(kind=kq(4), lat=a),
           dict(kind=kq(4, _hip.MASKED_LOWER)),
           dict(kind=kt(0)), dict(kind=kt(9)), dict(kind=kt(4), cw=None),
           dict(kind=kq(4) | 64), dict(kind=kq(4) | 128), dict(kind=kq(4) | (1 << 16)), dict(kind=kt(4) | (1 << 30)),
           dict(kind=_hip.MASKED_PER_IMAGE), dict(kind=_hip.MASKED_LOWER), dict(kind=1 | _hip.MASKED_PER_IMAGE),
           dict(kind=1 << 8), dict(kind=1 | (3 << 8)), dict(kind=2), dict(kind=-1),
           # a pooled group of 2^31 pixels; per image the same planes pass the size check and fail on nothing else -- not called
           dict(kind=kq(4), B=1 << 15, H=256, W=256, Ht=256, Wt=256), dict(kind=kt(4), B=1 << 15, H=256, W=256, Ht=256, Wt=256),
           # what kinds 0 / 1 refuse
           dict(kind=kq(4), pred=None), dict(kind=kq(4), target=None), dict(kind=kt(4), out=None), dict(kind=kt(4), cnt=None),
           dict(kind=kq(4), ws=None), dict(kind=kt(4), B=0), dict(kind=kq(4), Ht=7), dict(kind=kt(4), mask=a, pitch=7)]
    bad += [dict(kind=k | (4 << 8)) for k in range(5, 16)]
    for case in bad:
        assert fwd(**case) == -1, case
    assert not any(buf)


# ---- the wrappers against the stub library -------------------------------------------------------------------------------------------
def _operands():
    B, C, H, W = 2, 3, 8, 12
    return dict(pred=TB.t(TB.F32, B, C, H, W), target=TB.t(TB.F32, B, C, H + 1, W + 4), lat_w=TB.t(TB.F32, H),
                mask=TB.t(torch.uint8, B * C * H * W), levels=TB.t(TB.F32, 6), thr=TB.t(TB.F32, C, 5), thr_img=TB.t(TB.F32, B * C, 5))


def test_wrappers_reach_the_entry_with_the_kind_word(hip):
    o = _operands()
    B, C, H, W = o["pred"].shape
    ms = (W, C * H * W, H * W)
    out, cnt = hip.masked_quantiles(o["pred"], o["target"], o["levels"], o["mask"], ms, per_image=True)
    assert tuple(out.shape) == (2, B * C, 6, 3) and out.dtype == torch.float32 and tuple(cnt.shape) == (B * C,) and cnt.dtype == torch.int64
    out, cnt = hip.masked_quantiles(o["pred"], o["pred"], o["levels"])
    assert tuple(out.shape) == (2, C, 6, 3) and tuple(cnt.shape) == (C,)
    s, n = hip.masked_tail(o["pred"], o["target"], o["thr"], o["lat_w"], o["mask"], ms, lower=True)
    assert tuple(s.shape) == tuple(n.shape) == (B, C, 5, 4) and s.dtype == torch.float32 and n.dtype == torch.int64
    hip.masked_tail(o["pred"], o["target"], o["thr_img"], per_image=True)
    calls = hip.stub.calls
    assert [c[0] for c in calls] == ["orbit2_masked_loss_fwd"] * 4
    kinds = [c[1][17] for c in calls]
    assert kinds == [3 | 16 | (6 << 8), 3 | (6 << 8), 4 | 32 | (5 << 8), 4 | 16 | (5 << 8)]
    for name, args in calls:
        assert args[-1] == TB.STREAM and args[13:17] == (B, C, H, W)
    a = calls[0][1]
    assert a[0] == o["pred"].data_ptr() and a[1] == o["target"].data_ptr() and a[2:4] == (H + 1, W + 4)
    assert a[4] == o["mask"].data_ptr() and a[5:8] == ms and a[8] is None and a[9] == o["levels"].data_ptr()
    assert calls[1][1][0] == calls[1][1][1] == o["pred"].data_ptr() and calls[1][1][4] is None
    t = calls[2][1]
    assert t[8] == o["lat_w"].data_ptr() and t[9] == o["thr"].data_ptr() and t[4] == o["mask"].data_ptr()
    assert calls[3][1][9] == o["thr_img"].data_ptr() and calls[3][1][8] is None


@pytest.mark.parametrize("which", ["pred", "target", "levels", "mask", "thr", "lat_w"])
def test_wrappers_refuse_host_and_wrong_dtype_before_the_entry(hip, which):
    def run(o):
        W, C, H = o["pred"].shape[3], o["pred"].shape[1], o["pred"].shape[2]
        ms = (W, C * H * W, H * W)
        if which in ("pred", "target", "levels", "mask"):
            hip.masked_quantiles(o["pred"], o["target"], o["levels"], o["mask"], ms)
        if which in ("pred", "target", "thr", "mask", "lat_w"):
            hip.masked_tail(o["pred"], o["target"], o["thr"], o["lat_w"], o["mask"], ms)

    o = _operands()
    o[which] = o[which].clone()
    o[which].flagged_host = True
    with pytest.raises(hip.HipBackendError, match="GPU tensor"):
        run(o)
    o = _operands()
    o[which] = o[which].to(torch.float64)
    with pytest.raises(hip.HipBackendError, match="must be"):
        run(o)
    assert hip.stub.calls == []


def test_wrappers_refuse_bad_level_counts_and_shapes(hip):
    o = _operands()
    for levels in (TB.t(TB.F32, 0), TB.t(TB.F32, 9), TB.t(TB.F32, 2, 3)):
        with pytest.raises(hip.HipBackendError, match="levels"):
            hip.masked_quantiles(o["pred"], o["target"], levels)
    for thr in (TB.t(TB.F32, 3, 9), TB.t(TB.F32, 2, 4), TB.t(TB.F32, 4), TB.t(TB.F32, 6, 4)):
        with pytest.raises(hip.HipBackendError, match="thresholds"):
            hip.masked_tail(o["pred"], o["target"], thr)
    with pytest.raises(hip.HipBackendError, match="smaller than the prediction"):
        hip.masked_quantiles(o["target"], o["pred"], o["levels"])
    big = torch.empty(0).new_empty((1 << 15, 1, 256, 256), device="meta")
    with pytest.raises(hip.HipBackendError, match=r"2\^31"):
        hip._groups("masked_quantiles", *big.shape, False)
    assert hip._groups("masked_quantiles", *big.shape, True) == 1 << 15
    assert hip.stub.calls == []


# ---- the host algebra of the functionals -----------------------------------------------------------------------------------------
@pytest.fixture
def fabricated(monkeypatch):
    """_hip.masked_quantiles / masked_tail replaced by functions that answer fabricated outputs and record their arguments"""
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    monkeypatch.setattr(fn, "_mask_operand", lambda mask, pred, target: (mask, 0, 0, 0))
    rec = dict(calls=[])
    r = np.random.default_rng(5)
    B, C = 2, 3

    def quantiles(pred, target, levels, mask=None, mask_strides=(0, 0, 0), per_image=False):
        G, Q = (B * C if per_image else C), levels.numel()
        out = torch.from_numpy(r.standard_normal((2, G, Q, 3)).astype(np.float32))
        rec["calls"].append(("q", pred, target, levels.clone(), per_image))
        rec["quant"] = out
        return out, torch.full((G,), 7, dtype=torch.int64)

    def tail(pred, target, thr, lat_w=None, mask=None, mask_strides=(0, 0, 0), lower=False, per_image=False):
        T = thr.shape[1]
        s = torch.from_numpy(r.uniform(0.5, 2.0, (B, C, T, 4)).astype(np.float32))
        n = torch.from_numpy(r.integers(1, 50, (B, C, T, 4)))
        n[..., 1] = torch.minimum(n[..., 1], n[..., 0])
        s[:, 1], n[:, 1] = 0.0, 0                                  # channel 1: an empty tail in every image
        rec["calls"].append(("t", pred, target, thr.clone(), lat_w, lower))
        rec["s"], rec["n"] = s, n
        return s, n

    monkeypatch.setattr(_hip, "masked_quantiles", quantiles)
    monkeypatch.setattr(_hip, "masked_tail", tail)
    rec["pred"], rec["target"] = torch.zeros(B, C, 4, 6), torch.zeros(B, C, 4, 6)
    return rec


def test_quantile_functionals_from_fabricated_outputs(fabricated):
    from climate_learn.metrics import functional as fn
    rec, pred, target = fabricated, fabricated["pred"], fabricated["target"]
    assert fn.SIGMA_LEVELS == (0.8413, 0.9772, 0.9987)
    got = fn.field_quantiles(pred, fn.SIGMA_LEVELS, per_image=True)
    kind, p, t, levels, per_image = rec["calls"][-1]
    assert p.data_ptr() == t.data_ptr() and per_image and levels.tolist() == [np.float32(q) for q in fn.SIGMA_LEVELS]
    assert torch.equal(got, rec["quant"][0, :, :, 0]) and tuple(got.shape) == (6, 3)
    got = fn.quantile_bias(pred, target, (0.05, 0.95))
    q = rec["quant"][..., 0]
    assert tuple(got.shape) == (4, 2) and torch.equal(got[:3], q[1] - q[0])
    assert torch.allclose(got[3], (q[1] - q[0]).mean(0))
    agg = fn.quantile_bias(pred, target, 0.5, aggregate_only=True)
    assert tuple(agg.shape) == (1,) and torch.allclose(agg, (rec["quant"][1, :, 0, 0] - rec["quant"][0, :, 0, 0]).mean())


def test_tail_functionals_from_fabricated_outputs(fabricated):
    from climate_learn.metrics import functional as fn
    rec, pred, target = fabricated, fabricated["pred"], fabricated["target"]
    lat = torch.linspace(0.5, 1.5, 4)
    got = fn.tail_rmse(pred, target, 0.9, lat_weights=lat)
    assert [c[0] for c in rec["calls"]] == ["q", "t"]
    assert rec["calls"][0][1].data_ptr() == pred.data_ptr() and rec["calls"][0][2].data_ptr() == target.data_ptr()
    # the threshold is field 0 of that call: the target's own quantile over the prediction's crop
    assert torch.equal(rec["calls"][1][3], rec["quant"][0, :, :, 0]) and torch.equal(rec["calls"][1][4], lat)
    s, n = rec["s"].double().sum(0), rec["n"].sum(0).double()
    want = (s[:, 0, 1] / s[:, 0, 0]).sqrt().float()
    assert tuple(got.shape) == (4,) and torch.isnan(got[1]) and torch.isnan(got[3])   # an empty tail is NaN, and so the plain mean
    assert torch.equal(got[[0, 2]], want[[0, 2]])
    thr = torch.tensor([1.0, 2.0, 3.0])
    got = fn.tail_mae(pred, target, thresholds=thr, lower=True)
    assert [c[0] for c in rec["calls"][2:]] == ["t"] and rec["calls"][2][3].tolist() == [[1.0], [2.0], [3.0]] and rec["calls"][2][5]
    s = rec["s"].double().sum(0)
    assert torch.equal(got[[0, 2]], (s[:, 0, 2] / s[:, 0, 0]).float()[[0, 2]])
    got = fn.tail_bias(pred, target, thresholds=thr, aggregate_only=True)
    s, n = rec["s"].double().sum(0), rec["n"].sum(0).double()
    assert got.dim() == 0 and torch.isnan(got)
    per = fn.tail_bias(pred, target, thresholds=thr)
    s, n = rec["s"].double().sum(0), rec["n"].sum(0).double()
    assert torch.equal(per[[0, 2]], (s[:, 0, 3] / n[:, 0, 0]).float()[[0, 2]]) and rec["calls"][-1][4] is None
    ex = fn.exceedance_scores(pred, target, 0.95)
    n = rec["n"].sum(0).double()[:, 0]
    h, f, ms = n[:, 1], n[:, 2], n[:, 0] - n[:, 1]
    assert set(ex) == {"csi", "pod", "far", "frequency_bias"} and all(tuple(v.shape) == (3,) for v in ex.values())
    for k, want in (("csi", h / (h + ms + f)), ("pod", h / (h + ms)), ("far", f / (h + f)), ("frequency_bias", (h + f) / (h + ms))):
        assert torch.equal(ex[k][[0, 2]], want.float()[[0, 2]]), k
    assert torch.isnan(ex["pod"][1]) and torch.isnan(ex["frequency_bias"][1])


def test_registry_names_and_levels(fabricated):
    import climate_learn as cl
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.metrics import LatitudeWeightedMetric
    from climate_learn.metrics.utils import METRICS_REGISTRY, MetricsMetaInfo
    rec, pred, target = fabricated, fabricated["pred"], fabricated["target"]
    meta = MetricsMetaInfo(["a", "b", "c"], ["a", "b", "c"], np.linspace(-60, 60, 4), np.arange(6), None)
    for name in ("tail_rmse", "lat_tail_rmse", "quantile_bias"):
        obj = cl.load_loss("cpu", None, name, False, meta)
        assert type(obj) is METRICS_REGISTRY[name] and obj.name == name and obj.level == 0.9772
        assert isinstance(obj, LatitudeWeightedMetric) == (name == "lat_tail_rmse")
        assert obj.set_level(0.95) is obj and obj.level == 0.95
        got = obj(pred, target)
        assert tuple(got.shape) == (4,)
        q_call = [c for c in rec["calls"] if c[0] == "q"][-1]
        assert q_call[3].tolist() == [np.float32(0.95)]
        if name == "lat_tail_rmse":
            assert rec["calls"][-1][4] is not None and rec["calls"][-1][4].numel() == 4
        assert cl.load_loss("cpu", None, name, True, meta)(pred, target).dim() == 0


def test_extreme_scores_layout_from_fabricated_outputs(fabricated):
    from climate_learn.utils.visualize import extreme_scores
    rec = fabricated
    res = extreme_scores(rec["pred"], rec["target"], ["a", "b", "c"], levels=(0.9, 0.99))
    assert set(res) == {"a", "b", "c"}
    kinds = [c[0] for c in rec["calls"]]
    assert kinds == ["q", "t", "q", "t"] and [c[5] for c in rec["calls"] if c[0] == "t"] == [False, True]
    up, low = [c[3].tolist() for c in rec["calls"] if c[0] == "q"]
    assert up == [np.float32(0.9), np.float32(0.99)] and np.allclose(low, [0.1, 0.01], atol=1e-7)
    keys = {"level", "target_quantile", "pred_quantile", "quantile_bias", "tail_rmse", "tail_bias", "csi", "frequency_bias"}
    for v in res:
        assert set(res[v]) == {"upper", "lower"} and all(len(res[v][s]) == 2 and set(res[v][s][0]) == keys for s in res[v])
    s, n, q = rec["s"].double().sum(0), rec["n"].sum(0).double(), rec["quant"][..., 0].double()       # the lower call's
    row = res["c"]["lower"][1]
    h, f, ms = n[2, 1, 1], n[2, 1, 2], n[2, 1, 0] - n[2, 1, 1]
    assert row["level"] == pytest.approx(0.01) and row["target_quantile"] == float(q[0, 2, 1])
    assert row["quantile_bias"] == float(q[1, 2, 1] - q[0, 2, 1]) and row["tail_rmse"] == float((s[2, 1, 1] / s[2, 1, 0]).sqrt())
    assert row["tail_bias"] == float(s[2, 1, 3] / n[2, 1, 0]) and row["csi"] == float(h / (h + ms + f))
    assert row["frequency_bias"] == float((h + f) / (h + ms)) and np.isnan(res["b"]["lower"][0]["tail_rmse"])


def test_config_and_driver_block():
    import yaml
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_extremes.yaml")))
    plain = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference.yaml")))
    assert conf.pop("extreme_scores") is True and conf == plain                  # the key is the only difference
    src = open(os.path.join(ROOT, "examples", "visualize.py")).read()
    assert 'conf.get("extreme_scores")' in src and 'print("extreme_scores", var' in src
