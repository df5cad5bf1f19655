"""CPU checks of the fractions skill score: the numpy yardstick against scipy's zero-padded box filter and against
the replica of the kernel's word / prefix / running-sum order; csrc/fss_window.h through a stand-alone host program, plainly and
under host sanitizers; the header's constants and workspace macro against the binding's; the entry's refusals before any launch;
the wrapper against the stub library of tests/test_binding_cpu.py; the host algebra of the functionals, the registered metric
and neighbourhood_scores from fabricated kernel outputs; the config and the driver block."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import extremes_ref as E
from tests import fss_ref as R
from tests import test_binding_cpu as TB
from tests.conftest import ROOT

hip = TB.hip                                        # the stub-library fixture of the binding tests
CSRC = os.path.join(ROOT, "orbit-2_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADER = os.path.join(ROOT, "include", "orbit2_hip.h")


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
def _plane(shape, seed):
    H, W = shape
    target = E.values("zero_inflated", H * W, seed).reshape(H, W)
    pred = np.roll(target, (1, 2), (0, 1)) + np.float32(0.25) * E.values("gauss0", H * W, seed + 1).reshape(H, W)
    return pred.astype(np.float32), target


@pytest.mark.parametrize("shape", R.CPU_PLANES, ids=lambda s: "%dx%d" % s)
def test_yardstick_equals_the_zero_padded_box_filter(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    pred, target = _plane(shape, 3)
    ind = target >= np.float32(1.0)
    for n in R.WINDOWS:
        want = ndimage.uniform_filter(ind.astype(np.float64), size=n, mode="constant", cval=0.0) * n * n
        got = R.box_counts(ind, n)
        assert got.dtype == np.int64 and np.abs(got - want).max() < 1e-6, (shape, n)


@pytest.mark.parametrize("shape", R.CPU_PLANES, ids=lambda s: "%dx%d" % s)
def test_replica_of_the_kernel_order_equals_the_yardstick(shape):
    pred, target = _plane(shape, 5)
    target[shape[0] // 2, shape[1] // 3] = np.nan                           # an invalid pixel
    pred[0, 0] = np.nan                                                     # a NaN prediction at a valid one: compares false
    mask = np.random.default_rng(1).random(shape) < 0.9
    for k, n in enumerate(R.WINDOWS):
        lower, m = bool(k & 1), (mask if k % 3 == 0 else None)
        want = R.sums(pred, target, 1.0, n, m, lower)
        assert all(type(v) is int for v in want) and want[1] + want[2] > 0, (shape, n)
        assert R.popcount_replica(pred, target, 1.0, n, m, lower, band=32) == want, (shape, n)
    assert R.popcount_replica(pred, target, 1.0, 7, band=4) == R.sums(pred, target, 1.0, 7)      # many bands


def test_yardstick_on_hand_made_cases():
    t = np.zeros((5, 5), dtype=np.float32)
    t[2, 2] = 1.0
    p = np.roll(t, 1, 1)                                                    # the event one pixel aside
    assert R.sums(p, t, 0.5, 1) == (25, 1, 1, 2) and R.score(R.sums(p, t, 0.5, 1)) == 0.0         # grid scale: the double penalty
    assert R.sums(t, t, 0.5, 3) == (25, 9, 9, 0) and R.score(R.sums(t, t, 0.5, 3)) == 1.0
    c = R.sums(p, t, 0.5, 255)                                              # larger than the plane: clamped, every count is 1
    assert c == (25, 25, 25, 0)
    assert np.isnan(R.score(R.sums(p, t, 2.0, 3))) and R.sums(p, t, 2.0, 3) == (25, 0, 0, 0)
    assert R.sums(p, t, 0.5, 3, lower=True)[1] == sum(int(v) ** 2 for v in R.box_counts(t <= 0.5, 3).ravel())
    t[0, 0] = np.nan                                                        # invalid: in no indicator, no centre
    assert R.sums(t, t, -1.0, 1) == (24, 24, 24, 0)
    assert 255 ** 4 < 2 ** 32 and (2 ** 63 - 1) // 255 ** 4 == 2181368337 > 2 ** 31


# ---- csrc/fss_window.h on the host ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_program_of_the_window_header(tmp_path, sanitize):
    """span, prefix popcount, strip table, bands and workspace layout (tests/fss_window_host.cpp): a program of its own, never
    Python code"""
    exe = str(tmp_path / "fss_window_host")
    flags = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-w", "-I", CSRC] + flags +
                   [os.path.join(ROOT, "tests", "fss_window_host.cpp"), "-o", exe], check=True, capture_output=True)
    if sanitize:
        assert b"__asan_init" in open(exe, "rb").read()
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "fss_window ok", r.stdout[-2000:] + r.stderr[-2000:]


# ---- header and binding -----------------------------------------------------------------------------------------------------------
def _macro(hdr, name):
    m = re.search(r"^#define\s+%s\(([^)]*)\)\s+(.+)$" % name, hdr, flags=re.M)
    return [p.strip() for p in m.group(1).split(",")], m.group(2)


def test_header_constants_and_workspace_macro_match_the_binding():
    from climate_learn import _hip
    hdr = open(HEADER).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+ORBIT2_FSS_(\w+)\s+(\d+)", hdr, flags=re.M)}
    assert d == {"KIND": _hip.FSS_KIND, "MAX_WINDOW": _hip.FSS_MAX_WINDOW} == {"KIND": 5, "MAX_WINDOW": 255}
    params, body = _macro(hdr, "ORBIT2_FSS_WS_WORDS")
    assert params == ["B", "C", "H", "W", "T"]
    expr = body.replace("(long long)", "").replace("/", "//")
    assert re.fullmatch(r"[\w\s()*+/]+", expr), expr
    for B, C, H, W, T in ((1, 1, 1, 1, 1), (2, 3, 9, 63, 5), (2, 3, 9, 64, 8), (16, 3, 512, 1024, 3), (1, 2, 7, 129, 1)):
        got = eval(expr, {"__builtins__": {}}, dict(B=B, C=C, H=H, W=W, T=T))
        assert got == _hip.fss_ws_words(B, C, H, W, T) == 2 * B * C * (2 * T + 1) * H * ((W + 63) // 64) and got % 2 == 0
    params, body = _macro(hdr, "ORBIT2_FSS_WORD")
    assert params == ["flags", "T", "n"] and body.replace(" ", "") == "(ORBIT2_FSS_KIND|(flags)|((T)<<8)|((n)<<16))"
    # the window header's constants are the binding's: the partition a test derives its shapes from
    win = open(os.path.join(CSRC, "fss_window.h")).read()
    c = {k: int(v) for k, v in re.findall(r"^constexpr int FSS_(\w+) = (\d+);", win, flags=re.M)}
    assert c["MAX_WINDOW"] == _hip.FSS_MAX_WINDOW and c["STRIP"] == _hip.FSS_STRIP and c["MAX_LEVELS"] == _hip.MASKED_MAX_LEVELS
    assert (c["MAX_BAND"], c["MIN_BAND"], c["FILL"]) == _hip.FSS_BANDS
    assert _hip.fss_partition(16, 3, 512, 1024, 3) == (256, 128) and _hip.fss_partition(2, 3, 70, 300, 1) == (256, 32)
    assert _hip.fss_partition(1, 1, 4096, 256, 1) == (256, 32) and _hip.fss_partition(16, 1, 4096, 256, 1) == (256, 64)
    # the ABI: version 8, the entry's prototype as it was, no new export
    assert int(re.search(r"^#define\s+ORBIT2_ABI_VERSION\s+(\d+)", hdr, flags=re.M).group(1)) == 8 == _hip.ABI_VERSION
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _hip.PROTOTYPES["orbit2_masked_loss_fwd"] == (I, (P, P, I, I, P, I, L, L, P, P, P, P, P, I, I, I, I, I, P))
    assert not [n for n in _hip.PROTOTYPES if "fss" in n]
    stripped = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert not re.search(r"\borbit2_\w*fss\w*\s*\(", stripped)


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_fss_words_without_a_gpu():
    """every refusal returns before anything is launched or written; the addresses are never dereferenced"""
    from climate_learn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    names = ("pred", "target", "Ht", "Wt", "mask", "pitch", "sb", "sc", "lat", "cw", "out", "cnt", "ws", "B", "C", "H", "W", "kind", "s")
    base = dict(pred=a, target=a, Ht=8, Wt=8, mask=None, pitch=0, sb=0, sc=0, lat=None, cw=a, out=a, cnt=a, ws=a, B=1, C=1, H=8,
                W=8, kind=0, s=None)
    fwd = lambda **k: lib.orbit2_masked_loss_fwd(*[{**base, **k}[n] for n in names])
    kf = lambda T, n, flags=0: _hip.FSS_KIND | flags | (T << 8) | (n << 16)
    good = kf(3, 9)
    bad = [dict(kind=kf(0, 9)), dict(kind=kf(9, 9)), dict(kind=kf(3, 0)), dict(kind=kf(3, 2)), dict(kind=kf(3, 254)),
           dict(kind=kf(3, 256)), dict(kind=kf(3, 1) | (1 << 24)), dict(kind=good | 64), dict(kind=good | 128),
           dict(kind=good | (1 << 24)), dict(kind=good | (1 << 30)), dict(kind=-good),
           dict(kind=good, lat=a), dict(kind=good, cw=None), dict(kind=good, ws=None), dict(kind=good, ws=a + 4),
           # a pooled group of 2^31 pixels; per image the same planes pass the size check and fail on nothing else -- not called
           dict(kind=good, B=1 << 15, H=256, W=256, Ht=256, Wt=256),
           # what kinds 0 / 1 refuse
           dict(kind=good, pred=None), dict(kind=good, target=None), dict(kind=good, out=None), dict(kind=good, cnt=None),
           dict(kind=good, B=0), dict(kind=good, Ht=7), dict(kind=good, mask=a, pitch=7)]
    # bits 16 and up stay refused on every other kind
    bad += [dict(kind=k | (9 << 16)) for k in (0, 1)]
    bad += [dict(kind=k | (4 << 8) | (9 << 16)) for k in (_hip.MASKED_QUANTILES, _hip.MASKED_TAIL)]
    for case in bad:
        assert fwd(**case) == -1, case
    assert not any(buf)


# ---- the wrapper against the stub library -------------------------------------------------------------------------------------------
def _operands():
    B, C, H, W = 2, 3, 8, 12
    return dict(pred=TB.t(TB.F32, B, C, H, W), target=TB.t(TB.F32, B, C, H + 1, W + 4), mask=TB.t(torch.uint8, B * C * H * W),
                thr=TB.t(TB.F32, C, 5), thr_img=TB.t(TB.F32, B * C, 2))


def test_wrapper_reaches_the_entry_with_the_kind_word(hip):
    o = _operands()
    B, C, H, W = o["pred"].shape
    ms = (W, C * H * W, H * W)
    out, cnt = hip.masked_fss(o["pred"], o["target"], o["thr"], 9, o["mask"], ms, lower=True)
    assert tuple(out.shape) == (B, C, 5) and out.dtype == torch.float32
    assert tuple(cnt.shape) == (B, C, 5, 4) and cnt.dtype == torch.int64
    out, cnt = hip.masked_fss(o["pred"], o["pred"], o["thr_img"], 255, per_image=True)
    assert tuple(out.shape) == (B, C, 2) and tuple(cnt.shape) == (B, C, 2, 4)
    hip.masked_fss(o["pred"], o["target"], o["thr"], 1)
    calls = hip.stub.calls
    assert [c[0] for c in calls] == ["orbit2_masked_loss_fwd"] * 3
    assert [c[1][17] for c in calls] == [5 | 32 | (5 << 8) | (9 << 16), 5 | 16 | (2 << 8) | (255 << 16), 5 | (5 << 8) | (1 << 16)]
    for name, args in calls:
        assert args[-1] == TB.STREAM and args[13:17] == (B, C, H, W) and args[8] is None           # lat_w is always NULL
        assert isinstance(args[12], int) and args[12] % 8 == 0 and args[10] and args[11]
    a = calls[0][1]
    assert a[0] == o["pred"].data_ptr() and a[1] == o["target"].data_ptr() and a[2:4] == (H + 1, W + 4)
    assert a[4] == o["mask"].data_ptr() and a[5:8] == ms and a[9] == o["thr"].data_ptr()
    b = calls[1][1]
    assert b[0] == b[1] == o["pred"].data_ptr() and b[2:4] == (H, W) and b[4] is None and b[9] == o["thr_img"].data_ptr()


@pytest.mark.parametrize("which", ["pred", "target", "thr", "mask"])
def test_wrapper_refuses_host_and_wrong_dtype_before_the_entry(hip, which):
    def run(o):
        B, C, H, W = o["pred"].shape
        hip.masked_fss(o["pred"], o["target"], o["thr"], 9, o["mask"], (W, C * H * W, H * W))

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


def test_wrapper_refuses_bad_windows_and_shapes(hip):
    o = _operands()
    for window in (0, 2, 8, 256, 257, -3, 9.0, True, None, "9"):
        with pytest.raises(hip.HipBackendError, match="window"):
            hip.masked_fss(o["pred"], o["target"], o["thr"], window)
    for thr in (TB.t(TB.F32, 3, 9), TB.t(TB.F32, 2, 4), TB.t(TB.F32, 4), TB.t(TB.F32, 6, 4), TB.t(TB.F32, 3, 0)):
        with pytest.raises(hip.HipBackendError, match="thresholds"):
            hip.masked_fss(o["pred"], o["target"], thr, 9)
    with pytest.raises(hip.HipBackendError, match="thresholds"):
        hip.masked_fss(o["pred"], o["target"], o["thr"], 9, per_image=True)                       # [C, T] where [B*C, T] is read
    with pytest.raises(hip.HipBackendError, match="smaller than the prediction"):
        hip.masked_fss(o["target"], o["pred"], o["thr"], 9)
    with pytest.raises(hip.HipBackendError, match=r"2\^31"):
        hip._groups("masked_fss", 1 << 15, 1, 256, 256, False)
    assert hip.stub.calls == []


# ---- the host algebra of the functionals -----------------------------------------------------------------------------------------
B_, C_ = 2, 3


def _fabricate(window, T):
    """cnt [B,C,T,4] of one fabricated call: channel 0 scores rise with the window, channel 1 has no event at all (0 / 0),
    channel 2 is perfect"""
    n = torch.zeros(B_, C_, T, 4, dtype=torch.int64)
    n[..., 0] = 1000
    for k in range(T):
        ev = 100 // (k + 1)                                                 # target events per image at window 1
        w2 = window * window
        n[:, 0, k, 1] = ev * w2 if window > 1 else ev
        n[:, 0, k, 2] = ev * w2 if window > 1 else ev
        n[:, 0, k, 3] = (2 * ev * w2) // (window + k) if window > 1 else 2 * ev
        n[:, 2, k, 1] = n[:, 2, k, 2] = ev * w2 if window > 1 else ev
    return n


@pytest.fixture
def fabricated(monkeypatch):
    """_hip.masked_quantiles / masked_fss replaced by functions that answer fabricated outputs and record their arguments"""
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    monkeypatch.setattr(fn, "_mask_operand", lambda mask, pred, target: (mask, 0, 0, 0))
    rec = dict(calls=[])

    def quantiles(pred, target, levels, mask=None, mask_strides=(0, 0, 0), per_image=False):
        Q = levels.numel()
        out = torch.arange(2 * C_ * Q * 3, dtype=torch.float32).reshape(2, C_, Q, 3) / 7
        rec["calls"].append(("q", pred, target, levels.clone(), per_image))
        rec["quant"] = out
        return out, torch.full((C_,), 7, dtype=torch.int64)

    def masked_fss(pred, target, thr, window, mask=None, mask_strides=(0, 0, 0), lower=False, per_image=False):
        assert type(window) is int
        n = _fabricate(window, thr.shape[1])
        rec["calls"].append(("f", pred, target, thr.clone(), window, lower, per_image))
        return torch.zeros(B_, C_, thr.shape[1]), n

    monkeypatch.setattr(_hip, "masked_quantiles", quantiles)
    monkeypatch.setattr(_hip, "masked_fss", masked_fss)
    rec["pred"], rec["target"] = torch.zeros(B_, C_, 4, 6), torch.zeros(B_, C_, 4, 6)
    return rec


def _want(window, k=0):
    """[C] double: the pooled score of every channel from the fabricated integers summed over the batch"""
    n = _fabricate(window, k + 1).sum(0)[:, k].double()
    return 1.0 - n[:, 3] / (n[:, 1] + n[:, 2])


def test_fss_functional_from_fabricated_outputs(fabricated):
    from climate_learn.metrics import functional as fn
    rec, pred, target = fabricated, fabricated["pred"], fabricated["target"]
    got = fn.fss(pred, target)
    assert [c[0] for c in rec["calls"]] == ["q", "f"]
    q, f = rec["calls"]
    assert q[1].data_ptr() == pred.data_ptr() and q[2].data_ptr() == target.data_ptr() and q[3].tolist() == [np.float32(0.9772)]
    assert torch.equal(f[3], rec["quant"][0, :, :, 0]) and f[4:] == (9, False, False)     # the target's own quantile, window 9
    want = _want(9).float()
    assert tuple(got.shape) == (4,) and got.dtype == torch.float32
    assert torch.equal(got[[0, 2]], want[[0, 2]]) and got[2] == 1.0 and 0.0 < got[0] < 1.0
    assert torch.isnan(got[1]) and torch.isnan(got[3])                                    # 0 / 0 is NaN, and so the plain mean
    thr = torch.tensor([1.0, 2.0, 3.0])
    got = fn.fss(pred, target, window=33, lower=True, thresholds=thr)
    assert [c[0] for c in rec["calls"][2:]] == ["f"] and rec["calls"][2][3].tolist() == [[1.0], [2.0], [3.0]]
    assert rec["calls"][2][4:] == (33, True, False) and torch.equal(got[[0, 2]], _want(33).float()[[0, 2]])
    assert fn.fss(pred, target, 3, thresholds=thr, aggregate_only=True).dim() == 0


def test_fss_profile_from_fabricated_outputs(fabricated):
    from climate_learn.metrics import functional as fn
    rec, pred, target = fabricated, fabricated["pred"], fabricated["target"]
    windows = (3, 9, 1, 33)
    prof = fn.fss_profile(pred, target, windows)
    assert [c[0] for c in rec["calls"]] == ["q", "f", "f", "f", "f"]                       # window 1 once, then one call per other window
    assert [c[4] for c in rec["calls"][1:]] == [1, 3, 9, 33]
    assert rec["calls"][0][3].tolist() == [np.float32(q) for q in fn.SIGMA_LEVELS]
    assert set(prof) == {"fss", "base_rate", "uniform", "skilful_window"}
    assert tuple(prof["fss"].shape) == (3, 3, 4) and tuple(prof["base_rate"].shape) == tuple(prof["uniform"].shape) == (3, 3)
    assert prof["skilful_window"].dtype == torch.int64 and tuple(prof["skilful_window"].shape) == (3, 3)
    for k in range(3):
        for j, w in enumerate(windows):
            want = _want(w, k).float()
            assert torch.equal(prof["fss"][[0, 2], k, j], want[[0, 2]]) and torch.isnan(prof["fss"][1, k, j])
        ev = 100 // (k + 1)
        assert prof["base_rate"][0, k] == np.float32(ev / 1000) and prof["uniform"][0, k] == np.float32(0.5 + ev / 2000)
        assert prof["base_rate"][1, k] == 0 and prof["uniform"][1, k] == 0.5
        # channel 0 at level k: fss = 1 - 1 / (w + k) for w > 1 and 0 at w = 1; uniform = 0.5 + ev / 2000
        reach = [w for w in sorted(windows) if (1.0 - 1.0 / (w + k) if w > 1 else 0.0) >= 0.5 + ev / 2000]
        assert int(prof["skilful_window"][0, k]) == reach[0] == 3
        assert int(prof["skilful_window"][1, k]) == 0                                        # NaN reaches nothing
        assert int(prof["skilful_window"][2, k]) == 1                                        # perfect at the grid scale
    none = fn.fss_profile(pred, target, (1,), q=(0.5,))
    assert tuple(none["fss"].shape) == (3, 1, 1) and none["skilful_window"][:, 0].tolist() == [0, 0, 1]


def test_registry_name_level_and_window(fabricated):
    import climate_learn as cl
    from climate_learn.metrics.utils import METRICS_REGISTRY, MetricsMetaInfo
    rec, pred, target = fabricated, fabricated["pred"], fabricated["target"]
    meta = MetricsMetaInfo(["a", "b", "c"], ["a", "b", "c"], np.linspace(-60, 60, 4), np.arange(6), None)
    obj = cl.load_loss("cpu", None, "fss", False, meta)
    assert type(obj) is METRICS_REGISTRY["fss"] and obj.name == "fss" and obj.level == 0.9772 and obj.window == 9
    assert obj.set_window(17) is obj and obj.window == 17 and obj.set_level(0.95) is obj
    got = obj(pred, target)
    assert tuple(got.shape) == (4,) and torch.equal(got[[0, 2]], _want(17).float()[[0, 2]])
    assert rec["calls"][-2][3].tolist() == [np.float32(0.95)] and rec["calls"][-1][4] == 17
    assert type(obj).window == 9                                                           # set_window touches the object alone
    assert cl.load_loss("cpu", None, "fss", True, meta)(pred, target).dim() == 0


def test_neighbourhood_scores_layout_from_fabricated_outputs(fabricated):
    from climate_learn.utils.visualize import neighbourhood_scores
    rec = fabricated
    res = neighbourhood_scores(rec["pred"], rec["target"], ["a", "b", "c"], levels=(0.9, 0.99), windows=(1, 3, 9))
    assert set(res) == {"a", "b", "c"} and [c[0] for c in rec["calls"]] == ["q", "f", "f", "f"]
    assert rec["calls"][0][3].tolist() == [np.float32(0.9), np.float32(0.99)]
    assert all(torch.equal(c[3], rec["quant"][0, :, :, 0]) for c in rec["calls"][1:])
    keys = {"level", "threshold", "base_rate", "uniform", "skilful_window", "fss"}
    for c, v in enumerate("abc"):
        assert len(res[v]) == 2 and all(set(row) == keys and list(row["fss"]) == [1, 3, 9] for row in res[v])
        for j, row in enumerate(res[v]):
            assert row["level"] == (0.9, 0.99)[j] and row["threshold"] == float(rec["quant"][0, c, j, 0])
            assert type(row["skilful_window"]) is int and type(row["fss"][3]) is float
    row = res["a"][1]
    assert row["base_rate"] == pytest.approx(0.05) and row["uniform"] == pytest.approx(0.525) and row["skilful_window"] == 3
    assert row["fss"][1] == 0.0 and row["fss"][9] == pytest.approx(float(_want(9, 1)[0]))
    assert np.isnan(res["b"][0]["fss"][3]) and res["b"][0]["skilful_window"] == 0 and res["c"][0]["skilful_window"] == 1
    assert len(neighbourhood_scores(rec["pred"], rec["target"], ["a", "b", "c"])["a"]) == 3
    assert [c[4] for c in rec["calls"][-7:]] == [1, 3, 5, 9, 17, 33, 65]


def test_config_and_driver_block():
    import yaml
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_fss.yaml")))
    ext = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_extremes.yaml")))
    assert conf.pop("neighbourhood_scores") is True and ext.pop("extreme_scores") is True and conf == ext
    src = open(os.path.join(ROOT, "examples", "visualize.py")).read()
    assert 'conf.get("neighbourhood_scores")' in src and 'print("neighbourhood_scores", var' in src
    assert src.index('print("extreme_scores", var') < src.index('print("neighbourhood_scores", var')
    assert "neighbourhood_scores" in src.split('"""')[1]                                   # the docstring names the block
