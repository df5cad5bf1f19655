"""The all-member ensemble scores on the device (orbit2_ensemble_scores, metrics.functional.ensemble_*, utils.mc_dropout_members,
the inference driver's `scores: members`) against the float64 brute force of tests/ensemble_ref.py.

Tolerance against float64 for the sums, the derived scores, the CRPS field and the quantiles: rtol 2e-5, atol 2e-6, the one the
project's score reductions are held to (tests/test_mc_dropout_gpu.py).  The histogram, q = 0 / q = 1 and repeated calls are
compared bit for bit."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import ensemble_ref as ref
from tests._child import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(rtol=2e-5, atol=2e-6)
SHAPE, TARGET_HW = (2, 3, 24, 40), (26, 44)
LEVELS = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]
HI_SEED = (0x12345678 << 32) | 5


@functools.lru_cache(maxsize=None)
def _case(n, offset, shape=SHAPE, target_hw=TARGET_HW):
    """inputs and float64 references of one case, computed once and shared (never written to)"""
    members, target = ref.make_inputs(n, shape, target_hw, offset)
    lat = ref.lat_weights(shape[2])
    emp, fair = ref.crps_fields(members, target)
    out = dict(members=members, target=target, lat=lat, emp=emp, fair=fair, sums=ref.sums(members, target),
               sums_lat=ref.sums(members, target, lat), quant=ref.quantiles(members, LEVELS))
    for v in out.values():
        v.setflags(write=False)
    return out


def _close(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err - (KW["atol"] + KW["rtol"] * np.abs(want))).max())
    print("[ensemble %s] max abs err %.3e, worst margin to the bound %.3e" % (what, float(err.max()), worst), flush=True)
    assert np.allclose(got, want, **KW), what


def _channel_means(s, n):
    """[C + 1] from float64 sums [B, C]: per channel the mean over (b, h, w), then the mean of those"""
    per = s.sum(0) / n
    return np.append(per, per.mean())


@pytest.mark.parametrize("offset", [0.0, 280.0])
@pytest.mark.parametrize("n", [2, 3, 5, 8, 16, 33, 64])
def test_scores_against_float64(n, offset):
    """every padded network size, padded and unpadded; cropped target; latitude weights on and off; both CRPS forms.  At
    offset 280 the per-pixel field is the check that a pair sum on raw values fails (up to 4e-5 absolute there)"""
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    c = _case(n, offset)
    members, target = torch.tensor(c["members"], device="cuda"), torch.tensor(c["target"], device="cuda")
    lat = torch.tensor(c["lat"], device="cuda")
    B, C, H, W = SHAPE
    tag = "N=%d offset=%g" % (n, offset)
    out = _hip.ensemble_scores(members, target, crps_field="empirical", quantiles=LEVELS)
    _close(out["sums"], c["sums"], tag + " sums")
    _close(out["crps_field"], c["emp"], tag + " crps_field empirical")
    _close(out["quantiles"], c["quant"], tag + " quantiles")
    assert torch.equal(out["quantiles"][0], members.amin(0)) and torch.equal(out["quantiles"][-1], members.amax(0))
    out = _hip.ensemble_scores(members, target, lat, crps_field="fair")
    _close(out["sums"], c["sums_lat"], tag + " sums lat")
    _close(out["crps_field"], c["fair"], tag + " crps_field fair")
    _close(fn.ensemble_crps_field(members, target, fair=True), c["fair"], tag + " fn crps_field fair")
    _close(fn.ensemble_quantiles(members, LEVELS), c["quant"], tag + " fn quantiles")
    wl = lat.view(1, 1, -1, 1)
    for lw, s in ((None, c["sums"]), (wl, c["sums_lat"])):
        which = tag + (" lat" if lw is not None else "")
        px = H * W
        _close(fn.ensemble_crps(members, target, False, lw), _channel_means(s[..., 0] - s[..., 1] / (n * n), px * B),
               which + " ensemble_crps")
        _close(fn.ensemble_crps(members, target, False, lw, fair=True),
               _channel_means(s[..., 0] - s[..., 1] / (n * (n - 1)), px * B), which + " ensemble_crps fair")
        var, err = s[..., 3].sum(0), s[..., 2].sum(0)
        _close(fn.ensemble_spread_skill_ratio(members, target, False, lw),
               np.append(np.sqrt(var / err), np.sqrt(var.sum() / err.sum())), which + " spread/skill")
        agg = fn.ensemble_crps(members, target, True, lw)
        assert agg.dim() == 0 and torch.equal(agg, fn.ensemble_crps(members, target, False, lw)[-1])


@pytest.mark.parametrize("n,shape", [(5, (2, 3, 7, 13)),            # odd, no multiple of 4 or 64
                                     (3, (1, 1, 520, 512)),          # > 1024 workgroups x 256 pixels: a second grid-stride trip
                                     (2, (2, 8, 130, 128))])         # >= 16 images: > 64 workgroups x 256 pixels per image
def test_odd_and_multi_trip_shapes(n, shape):
    from climate_learn import _hip
    c = _case(n, 0.0, shape, None)
    members, target = torch.tensor(c["members"], device="cuda"), torch.tensor(c["target"], device="cuda")
    out = _hip.ensemble_scores(members, target, torch.tensor(c["lat"], device="cuda"), hist=True, seed=5, crps_field="empirical",
                               quantiles=LEVELS)
    tag = "N=%d %s" % (n, "x".join(map(str, shape)))
    _close(out["sums"], c["sums_lat"], tag + " sums lat")
    _close(out["crps_field"], c["emp"], tag + " crps_field")
    _close(out["quantiles"], c["quant"], tag + " quantiles")
    assert np.array_equal(out["hist"].cpu().numpy(), ref.rank_histogram(c["members"], c["target"], 5))


def _raw_call(members, stride, n, target, outs, levels, shape, fair=0, seed=0, lat=None):
    from climate_learn import _hip
    B, C, H, W = shape
    p = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
    return _hip.lib().orbit2_ensemble_scores(p(members), stride, n, p(target), target.shape[2], target.shape[3], p(lat),
                                             p(outs.get("sums")), p(outs.get("crps")), fair, p(outs.get("hist")), seed,
                                             p(outs.get("quant")), p(levels), 0 if levels is None else levels.numel(), B, C, H,
                                             W, torch.cuda.current_stream().cuda_stream)


GUARD = 64


def _guarded(numel, dtype, sentinel):
    """(buffer, view): `numel` elements with GUARD sentinel elements on either side"""
    buf = torch.full((numel + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[GUARD: GUARD + numel]


def test_member_stride_sentinels_and_output_selection():
    """members a field + 37 elements apart with sentinels in the gaps (1e30: reading one would wreck every score); every
    output inside guard bands; each output alone and all together give the same bits (240 pixels per image: one workgroup
    per image, so the double sums have one summation order too)"""
    n, shape = 5, (2, 3, 12, 20)
    B, C, H, W = shape
    field, gap = B * C * H * W, 37
    c = _case(n, 0.0, shape, (13, 23))
    stack = torch.full((n, field + gap), 1e30, device="cuda")
    stack[:, :field] = torch.tensor(c["members"], device="cuda").reshape(n, field)
    pristine = stack.clone()
    target = torch.tensor(c["target"], device="cuda")
    levels = torch.tensor(LEVELS, device="cuda")
    spec = {"sums": (B * C * 4, torch.float64, -7.0), "crps": (field, torch.float32, -7.0),
            "hist": (B * C * (n + 1), torch.int64, -7), "quant": (len(LEVELS) * field, torch.float32, -7.0)}
    results = {}
    for chosen in (["sums"], ["crps"], ["hist"], ["quant"], list(spec)):
        bufs = {k: _guarded(*spec[k]) for k in chosen}
        rc = _raw_call(stack, field + gap, n, target, {k: v[1] for k, v in bufs.items()}, levels if "quant" in chosen else None,
                       shape, seed=5)
        torch.cuda.synchronize()
        assert rc == 0, (chosen, rc)
        for k, (buf, view) in bufs.items():
            assert bool((buf[:GUARD] == spec[k][2]).all()) and bool((buf[-GUARD:] == spec[k][2]).all()), (chosen, k)
            results.setdefault(k, []).append(view.clone())
    assert torch.equal(stack, pristine)
    for k, (alone, together) in results.items():
        assert torch.equal(alone, together), k
    _close(results["sums"][0].view(B, C, 4), c["sums"], "strided sums")
    _close(results["crps"][0].view(shape), c["emp"], "strided crps_field")
    _close(results["quant"][0].view((len(LEVELS),) + shape), c["quant"], "strided quantiles")
    assert np.array_equal(results["hist"][0].view(B, C, n + 1).cpu().numpy(), ref.rank_histogram(c["members"], c["target"], 5))
    # the wrapper takes the same view
    from climate_learn import _hip
    view = stack[:, :field].view((n,) + shape)
    assert view.stride(0) == field + gap
    out = _hip.ensemble_scores(view, target, hist=True, seed=5)
    assert torch.equal(out["sums"].view(-1), results["sums"][0]) and torch.equal(out["hist"].view(-1), results["hist"][0])


@pytest.mark.parametrize("n", [2, 8, 33, 64])
def test_rank_histogram_equals_the_replica(n):
    """channel 0 tie-free, channel 1 every member equal to the target, channel 2 quantised to multiples of 0.25 (partial ties)"""
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    B, C, H, W = SHAPE
    c = _case(n, 0.0)
    members, target = c["members"].copy(), c["target"].copy()
    members[:, :, 1] = target[None, :, 1, :H, :W]
    members[:, :, 2] = np.round(members[:, :, 2] * 4) / 4
    target[:, 2] = np.round(target[:, 2] * 4) / 4
    eq = (members == target[None, :, :, :H, :W]).sum(0)
    assert eq[:, 0].max() == 0 and eq[:, 1].min() == n and 0 < (eq[:, 2] > 0).mean() < 1
    m, t = torch.from_numpy(members).cuda(), torch.from_numpy(target).cuda()
    hists = {}
    for seed in (0, 5, HI_SEED):
        got = _hip.ensemble_scores(m, t, sums=False, hist=True, seed=seed)["hist"]
        assert got.dtype == torch.int64 and got.shape == (B, C, n + 1)
        hists[seed] = got.cpu().numpy()
        assert np.array_equal(hists[seed], ref.rank_histogram(members, target, seed)), seed
        assert (hists[seed].sum(-1) == H * W).all()
        rows = fn.ensemble_rank_histogram(m, t, seed=seed).cpu().numpy()
        assert rows.shape == (C + 1, n + 1) and (rows[:C].sum(-1) == H * W * B).all()
        assert np.array_equal(rows[:C], hists[seed].sum(0)) and np.array_equal(rows[C], hists[seed].sum((0, 1)))
    # the seed's high word moves the tie channels; no seed moves the tie-free channel.  (Seeds 0 and 5 are each held to the
    # replica above, not to differ from each other: o2_hash64 xors the seed's low word into the index, so a low word below 8
    # only permutes the pixels of an image whose first index is a multiple of 8 -- an all-ties channel counts the same.)
    assert np.array_equal(hists[5][:, 0], hists[HI_SEED][:, 0]) and np.array_equal(hists[0][:, 0], hists[5][:, 0])
    for ch in (1, 2):
        assert not np.array_equal(hists[5][:, ch], hists[HI_SEED][:, ch]), ch
    # ... and the seed salt does not: a score is a pure function of its arguments
    _hip.seed_salt(12345)
    try:
        salted = _hip.ensemble_scores(m, t, sums=False, hist=True, seed=5)["hist"].cpu().numpy()
    finally:
        _hip.seed_salt(0)
    assert np.array_equal(salted, hists[5])
    a = _hip.ensemble_scores(m, t, hist=True, seed=5, crps_field="fair", quantiles=LEVELS)
    b = _hip.ensemble_scores(m, t, hist=True, seed=5, crps_field="fair", quantiles=LEVELS)
    for k in ("hist", "crps_field", "quantiles"):
        assert torch.equal(a[k], b[k]), k


def test_moments_agree_with_the_gaussian_scores_at_offset_0():
    """sums 2 and 3 against orbit2_gaussian_scores' sums 2 and 1 on the Welford mean / std of the same stack (offset 0 only:
    at 280 the fp32 Welford mean itself carries 3e-5)"""
    from climate_learn import _hip
    from climate_learn.utils import EnsembleMembers
    n = 16
    c = _case(n, 0.0)
    members, target = torch.tensor(c["members"], device="cuda"), torch.tensor(c["target"], device="cuda")
    st = EnsembleMembers(members).statistics()
    assert st.n == n
    for lat in (None, torch.tensor(c["lat"], device="cuda")):
        g = _hip.gaussian_scores(st.mean, st.std, target, lat).cpu().numpy()
        s = _hip.ensemble_scores(members, target, lat)["sums"]
        _close(s[..., 2], g[..., 2], "error of the mean against gaussian_scores")
        _close(s[..., 3], g[..., 1], "variance against gaussian_scores")


def test_refusals_with_a_device():
    from climate_learn import _hip
    n, shape = 4, (1, 2, 8, 8)
    field = 2 * 64
    members, target = torch.ones(n, *shape, device="cuda"), torch.ones(shape, device="cuda")
    levels = torch.tensor([0.5], device="cuda")
    outs = {"sums": torch.full((1, 2, 4), -7.0, dtype=torch.float64, device="cuda"), "crps": torch.full(shape, -7.0, device="cuda"),
            "hist": torch.full((1, 2, n + 1), -7, dtype=torch.int64, device="cuda"),
            "quant": torch.full((1,) + shape, -7.0, device="cuda")}
    call = lambda **kw: _raw_call(**{**dict(members=members, stride=field, n=n, target=target, outs=outs, levels=levels,   # noqa: E731
                                            shape=shape), **kw})
    assert call(members=None) == -1
    assert call(outs={}) == -1
    assert call(n=1) == -1 and call(n=65) == -1
    assert call(stride=field - 1) == -1
    assert call(shape=(1, 2, 0, 8)) == -1 and call(shape=(0, 2, 8, 8)) == -1
    assert call(shape=(1, 2, 9, 8)) == -1 and call(shape=(1, 2, 8, 9)) == -1             # target smaller than the prediction
    assert call(levels=None) == -1
    assert call(levels=torch.zeros(17, device="cuda")) == -1
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert float(v.min()) == -7.0 == float(v.max()), k                               # refused before anything was written
    assert call() == 0
    torch.cuda.synchronize()
    assert float(outs["quant"].min()) == 1.0 and int(outs["hist"].sum()) == 2 * 64
    # non-finite members: the scores are unspecified, but every pixel is still counted in one of the N + 1 bins
    bad = members.clone()
    bad[0, 0, 0, :4], bad[1, 0, 1, :4], bad[2, 0, 0, 2:6] = float("nan"), float("inf"), float("-inf")
    got = _hip.ensemble_scores(bad, torch.full_like(target, float("inf")), hist=True, crps_field="fair", quantiles=[0.0, 0.3, 1.0])
    assert got["hist"].shape == (1, 2, n + 1) and bool((got["hist"].sum(-1) == 64).all()) and int(got["hist"].min()) >= 0
    E = _hip.HipBackendError
    with pytest.raises(E, match="2 to 64 are served"):
        _hip.ensemble_scores(members[:1], target)
    with pytest.raises(E, match="members must be torch.float32"):
        _hip.ensemble_scores(members.double(), target)
    with pytest.raises(E, match="at least one field apart"):
        _hip.ensemble_scores(members.permute(0, 1, 2, 4, 3), target)
    with pytest.raises(E, match="does not match the prediction's"):
        _hip.ensemble_scores(members, target[:, :1].contiguous())
    with pytest.raises(E, match="smaller than the prediction"):
        _hip.ensemble_scores(members, target[:, :, :4].contiguous())
    with pytest.raises(E, match="lat_w has 4 entries"):
        _hip.ensemble_scores(members, target, torch.ones(4, device="cuda"))
    with pytest.raises(E, match="'empirical' or 'fair'"):
        _hip.ensemble_scores(members, target, crps_field="both")
    with pytest.raises(E, match="1 to 16 are served"):
        _hip.ensemble_scores(members, target, quantiles=[0.5] * 17)
    with pytest.raises(E, match=r"lie in \[0, 1\]"):
        _hip.ensemble_scores(members, target, quantiles=[0.5, 1.5])
    with pytest.raises(E, match="no output was asked for"):
        _hip.ensemble_scores(members, target, sums=False)


# ----------------------------------------------------------------------------------------------------------------- model level
def _model_batch():
    from tests.test_mc_dropout_gpu import _pair
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.1)
    return model, (x.cuda(), y.cuda(), in_vars, out_vars)


@pytest.mark.parametrize("div,overlap", [(1, 0), (2, 4)])
def test_members_equal_stacking_and_statistics_agree(div, overlap):
    import climate_learn as cl
    from climate_learn.utils import (EnsembleMembers, enable_dropout, get_monte_carlo_predictions, mc_dropout_members,
                                     mc_dropout_statistics, tiled_predict)
    from tests.test_mc_dropout_gpu import GRID, _welford_bound
    model, batch = _model_batch()
    n = 6
    cl.manual_seed(9)
    ens = mc_dropout_members(batch, model, n, div=div, overlap=overlap)
    assert isinstance(ens, EnsembleMembers) and ens.n == n and ens.members.shape[0] == n
    assert ens.members.dtype == torch.float32 and ens.members.is_cuda and ens.members.is_contiguous()
    assert model.mc_dropout and not model.training                        # the mode mc_dropout_statistics leaves
    assert tuple(model.img_size) == GRID
    cl.manual_seed(9)
    if div == 1:
        stack = get_monte_carlo_predictions(batch, model, n)
    else:
        model.eval()
        enable_dropout(model)
        stack = torch.stack([tiled_predict(model, *batch, div, overlap) for _ in range(n)])
    assert torch.equal(ens.members, stack) and not torch.equal(stack[0], stack[1])
    cl.manual_seed(9)
    assert torch.equal(mc_dropout_members(batch, model, n, div=div, overlap=overlap).members, ens.members)
    cl.manual_seed(9)
    streamed = mc_dropout_statistics(batch, model, n, div=div, overlap=overlap)
    st = ens.statistics()
    assert st.n == n and torch.equal(st.mean, streamed.mean) and torch.equal(st.m2, streamed.m2)      # the same Welford steps
    bound = _welford_bound(stack)
    assert float((st.mean.double() - stack.double().mean(0)).abs().max()) <= bound
    assert float((st.std.double() - stack.double().std(0)).abs().max()) <= bound
    model.eval()
    assert not model.mc_dropout
    with pytest.raises(ValueError, match="2 to 64 ensemble members"):
        mc_dropout_members(batch, model, 1)


def test_member_stack_peak_memory_grows_by_n_fields_not_2n():
    """N = 12 against N = 4: the peak grows by the 8 more fields of the stack (plus allocator rounding, bounded here by one
    field); a torch.stack of a list would hold 2 N at its peak and grow by 16"""
    from climate_learn.utils import mc_dropout_members
    model, batch = _model_batch()
    mc_dropout_members(batch, model, 2)                                   # warm-up: caches, compute copies
    peaks = {}
    for n in (4, 12):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ens = mc_dropout_members(batch, model, n)
        torch.cuda.synchronize()
        peaks[n] = torch.cuda.max_memory_allocated()
        one = ens.members[0].numel() * 4
        del ens
    print("[member stack memory] peak at N=4 %d B, at N=12 %d B, one prediction %d B" % (peaks[4], peaks[12], one), flush=True)
    assert 8 * one <= peaks[12] - peaks[4] <= 9 * one


# ---------------------------------------------------------------------------------------------------------------------- driver
_NUM = re.compile(r"[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?|\binf\b|\bnan\b")


def _run_driver(cfg, cwd):
    env = dict(os.environ, MASTER_PORT=str(free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "visualize.py"), cfg], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def test_inference_driver_member_scores(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_mc_members.yaml")))
    mc_conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_mc.yaml")))
    assert conf["mc_dropout"] == {"members": 16, "seed": 0, "scores": "members"}
    assert {k: v for k, v in conf.items() if k != "mc_dropout"} == {k: v for k, v in mc_conf.items() if k != "mc_dropout"}
    for c in (conf, mc_conf):
        c["model"].update(embed_dim=256, depth=2, decoder_depth=1, num_heads=4)
        c["data"]["synthetic"]["ERA5_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256])
    conf["mc_dropout"] = {"members": 4, "seed": 3, "scores": "members"}
    mc_conf["mc_dropout"] = {"members": 4, "seed": 3}
    out_vars = conf["data"]["dict_out_variables"]["ERA5_1"]
    lines = {}
    for name, c in (("members", conf), ("mc", mc_conf)):
        d = os.path.join(tmp_path, name)
        os.makedirs(d)
        cfg = os.path.join(d, "inf.yaml")
        yaml.safe_dump(c, open(cfg, "w"))
        lines[name] = _run_driver(cfg, d)
    mc, mem = lines["mc"], lines["members"]
    # without the key: exactly the six MC lines of today, nothing of the new report
    start = mc.index("mc_dropout members 4 seed 3")
    assert len(mc) == start + 6 and mc[-1].startswith("mc_dropout saved")
    assert not any("ensemble_" in ln or "rank_histogram" in ln for ln in mc)
    assert not os.path.exists(os.path.join(tmp_path, "mc", "0_mc_rank_hist.npy"))
    # with it: the same lines first (numbers masked: unseeded random weights differ between two processes), then the new ones
    assert len(mem) == len(mc) + 3 + len(out_vars)
    for a, b in zip(mc, mem):
        assert _NUM.sub("#", a) == _NUM.sub("#", b), (a, b)
    tail = mem[len(mc):]
    for ln, name in zip(tail[:3], ("ensemble_crps", "ensemble_crps_fair", "ensemble_spread_skill_ratio")):
        m = re.match(name + r" \[([^\]]+)\]$", ln)
        assert m, ln
        vals = [float(v) for v in m.group(1).split(",")]
        assert len(vals) == len(out_vars) + 1 and all(np.isfinite(v) and v >= 0 for v in vals), ln
    pixels = 128 * 256
    for ln, var in zip(tail[3:], out_vars):
        m = re.match(r"rank_histogram %s \[([^\]]+)\]$" % re.escape(var), ln)
        assert m, ln
        counts = [int(v) for v in m.group(1).split(",")]
        assert len(counts) == 5 and min(counts) >= 0 and sum(counts) == pixels, ln
    d = os.path.join(tmp_path, "members")
    hist = np.load(os.path.join(d, "0_mc_rank_hist.npy"))
    assert hist.shape == (len(out_vars) + 1, 5) and hist.dtype == np.int64 and (hist[:-1].sum(-1) == pixels).all()
    p05, p50, p95 = (np.load(os.path.join(d, "0_mc_p%s.npy" % q)) for q in ("05", "50", "95"))
    assert p05.shape == p50.shape == p95.shape == (1, len(out_vars), 128, 256)           # the stitched size
    assert np.isfinite(p05).all() and np.isfinite(p95).all()
    assert (p05 <= p50).all() and (p50 <= p95).all() and (p05 < p95).any()
