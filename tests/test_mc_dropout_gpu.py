"""MC-dropout mode on the device: the fused Block and the whole model against the CPU oracle fed the kernels' own masks
(tests/hashmask.py), the bitwise properties a tolerance cannot tell, the streaming ensemble statistics against fp64, the
Gaussian scores against the reference's recorded values / the closed form, and the inference driver's optional block."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests._child import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, DEPTH, HEADS, GRID, B = 128, 3, 2, (16, 32), 2
L, M, HID = (GRID[0] // 2) * (GRID[1] // 2), B * (GRID[0] // 2) * (GRID[1] // 2), 4 * D
TOL = 2e-2                                           # the contract's normalised max error


def _pair(p, drop_path=0.5, attn=None, backend=None):
    """the issue's case with probability p on the element sites, `attn` (default p) on the attention probabilities"""
    from climate_learn.utils.fused_attn import FusedAttn
    from oracle.harness import build_pair
    model, sd, cfg, O, x, y, in_vars, out_vars = build_pair(D=D, depth=DEPTH, heads=HEADS, grid=GRID, B=B, seed=31)
    for blk in model.blocks:
        blk.attn.attn_drop_p = p if attn is None else attn
        blk.attn.proj_drop_p = blk.mlp.drop = p
        blk.drop_path = drop_path
        if backend is not None:
            blk.attn.fused_attn = FusedAttn[backend]
    model.pos_drop_p = p
    return model.cuda().eval(), sd, cfg, O, x, y, in_vars, out_vars


def _flat(seed, n_cols, p):
    from tests.hashmask import keep_mask
    m, sc = keep_mask(seed, M * n_cols, p)
    return (torch.from_numpy(m) * sc).view(B, L, n_cols)


def _block_masks(ss, p):
    """the four masks of one Block in MC-dropout mode, in the order BlockFn draws its seeds: attn, proj, fc1, fc2 -- and NO
    DropPath seed (the mode leaves DropPath off, so none is drawn)"""
    from tests.hashmask import attn_keep_mask
    sa, sp, s1, s2 = ss.next(), ss.next(), ss.next(), ss.next()
    am, asc = attn_keep_mask(sa, B * HEADS, L, p)
    return {"attn": (torch.from_numpy(am) * asc).view(B, HEADS, L, L), "proj": _flat(sp, D, p), "fc1": _flat(s1, HID, p),
            "fc2": _flat(s2, D, p)}


def _bf16(o):
    if torch.is_tensor(o):
        return o.to(torch.bfloat16) if o.is_floating_point() else o
    return {k: _bf16(v) for k, v in o.items()}


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_block_in_mc_mode_matches_oracle_with_replicated_masks(p):
    """model.blocks[1] in MC-dropout mode against the oracle's block with the kernels' attn / proj / fc1 / fc2 masks and no
    DropPath (drop_path is 0.5: a DropPath that wrongly fired would zero or double a sample's branch).  Bound: the contract's
    2e-2, or oracle.harness.grad_tolerance of what plain bf16 moves the masked oracle's output, if that is more (printed)."""
    import climate_learn as cl
    from climate_learn import _ops
    from climate_learn.utils import enable_dropout
    from oracle.harness import grad_tolerance, nerr
    model, sd, cfg, O, *_ = _pair(p)
    g = torch.Generator().manual_seed(7)
    t = torch.randn(B, L, D, generator=g).to(torch.bfloat16)              # bf16-rounded N(0, 1) tokens
    enable_dropout(model)
    blk = model.blocks[1]
    assert blk.dropout_probs() == dict(attn_drop=p, proj_drop=p, mlp_drop=p, drop_path=0.0)
    cl.manual_seed(123)
    with torch.no_grad():
        got = blk(t.cuda()).float().cpu()
    ss = _ops._SeedStream()
    ss.manual_seed(123)
    masks = _block_masks(ss, p)
    assert _ops.seeds.mark() == ss.mark() == 4                           # four seeds drawn, none for DropPath
    ref = O.block(t.float(), sd, "blocks.1.", HEADS, masks)
    spread = nerr(O.block(t, _bf16(sd), "blocks.1.", HEADS, _bf16(masks)).float(), ref)
    tol = grad_tolerance(spread, "blocks.1 output in MC mode, p=%g" % p)
    gap = nerr(O.block(t.float(), sd, "blocks.1.", HEADS), ref)
    err = nerr(got, ref)
    print("[mc block p=%g] err %.3e  bf16 spread of the masked oracle %.3e  bound %.3e  unmasked oracle is %.3e away"
          % (p, err, spread, tol, gap), flush=True)
    assert gap > 2 * TOL                                                  # the case discriminates: twice the tolerance
    assert err <= tol, (err, tol)


def test_whole_model_in_mc_mode_matches_masked_oracle():
    """p = 0.5 everywhere, DropPath 0.5 configured: the MC-mode prediction against the oracle's forward with the `pos` mask and
    the per-block masks, no DropPath, within 2e-2 -- and closer to it than to the unmasked oracle"""
    import climate_learn as cl
    from climate_learn import _ops
    from climate_learn.utils import enable_dropout
    from oracle.harness import nerr
    p = 0.5
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(p)
    enable_dropout(model)
    cl.manual_seed(77)
    with torch.no_grad():
        got = model(x.cuda(), in_vars, out_vars).float().cpu()
    ss = _ops._SeedStream()
    ss.manual_seed(77)
    masks = {"pos": _flat(ss.next(), D, p)}
    for i in range(DEPTH):
        masks["blocks.%d" % i] = _block_masks(ss, p)
    assert _ops.seeds.mark() == ss.mark() == 1 + 4 * DEPTH
    ref = O.forward(sd, cfg, x, in_vars, out_vars, masks)
    plain = O.forward(sd, cfg, x, in_vars, out_vars)
    err, gap, err_plain = nerr(got, ref), nerr(plain, ref), nerr(got, plain)
    print("[mc model p=0.5] err to the masked oracle %.3e, to the unmasked oracle %.3e; the two oracles are %.3e apart"
          % (err, err_plain, gap), flush=True)
    assert err <= TOL, err
    assert err < err_plain


def _predict(model, x, in_vars, out_vars):
    with torch.no_grad():
        return model(x, in_vars, out_vars).clone()


def test_droppath_alone_leaves_mc_mode_bitwise_at_eval():
    from climate_learn.utils import enable_dropout
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.0, drop_path=0.5)
    x = x.cuda()
    base = _predict(model, x, in_vars, out_vars)
    enable_dropout(model)
    assert torch.equal(_predict(model, x, in_vars, out_vars), base)
    model.train()                                                         # ... while train mode does apply it
    assert not torch.equal(_predict(model, x, in_vars, out_vars), base)


@pytest.mark.parametrize("backend,moves", [("DEFAULT", False), ("HIP", True), ("NONE", True)])
def test_attention_probability_dropout_per_backend(backend, moves):
    """only attn_drop = 0.5 is non-zero: it moves this prediction by a few 1e-3, far inside any tolerance, so the check is
    bitwise -- off under DEFAULT (the reference hands SDPA the Attention module's own training flag), on under HIP and NONE"""
    from climate_learn.utils import enable_dropout
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.0, drop_path=0.0, attn=0.5, backend=backend)
    x = x.cuda()
    base = _predict(model, x, in_vars, out_vars)
    enable_dropout(model)
    got = _predict(model, x, in_vars, out_vars)
    assert torch.equal(got, base) == (not moves)
    assert torch.isfinite(got).all()


def test_ensemble_is_reproducible_members_differ_and_eval_restores():
    import climate_learn as cl
    from climate_learn.utils import get_monte_carlo_predictions
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.1)
    batch = (x, y, in_vars, out_vars)
    before = _predict(model, x.cuda(), in_vars, out_vars)
    cl.manual_seed(5)
    a = get_monte_carlo_predictions(batch, model, 3)
    assert a.shape == (3, B, 1, 4 * GRID[0], 4 * GRID[1]) and a.dtype == torch.float32 and a.is_cuda
    assert model.mc_dropout and not model.training
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])
    cl.manual_seed(5)
    assert torch.equal(get_monte_carlo_predictions(batch, model, 3), a)
    cl.manual_seed(6)
    assert not torch.equal(get_monte_carlo_predictions(batch, model, 3), a)
    model.eval()
    assert not model.mc_dropout
    assert torch.equal(_predict(model, x.cuda(), in_vars, out_vars), before)


def _welford_bound(members):
    n = members.shape[0]
    return 2 * n * 2.0 ** -24 * float(members.abs().max())


@pytest.mark.parametrize("offset", [0.0, 280.0])
def test_ensemble_update_against_fp64(offset):
    """N = 32 members of [2, 3, 64, 128], centred at 0 and at 280 (a field in kelvin): mean and std within
    2 N 2^-24 max|member| of the fp64 statistics of the stack (each step rounds the running mean, no larger than the largest
    member, to half an ulp, and feeds the difference into m2 once more)"""
    from climate_learn import _hip
    from climate_learn.utils.mc_dropout import EnsembleStatistics
    n = 32
    g = torch.Generator().manual_seed(11)
    members = (torch.randn(n, 2, 3, 64, 128, generator=g) + offset).cuda()
    mean, m2 = torch.full_like(members[0], float("nan")), torch.full_like(members[0], float("nan"))    # k = 1 must not read them
    for k in range(n):
        _hip.ensemble_update(members[k], mean, m2, k + 1)
    st = EnsembleStatistics(mean, m2, n)
    ref = members.double()
    e_mean = float((st.mean.double() - ref.mean(0)).abs().max())
    e_std = float((st.std.double() - ref.std(0)).abs().max())
    bound = _welford_bound(members)
    print("[ensemble_update offset %g] max |mean err| %.3e  max |std err| %.3e  bound %.3e" % (offset, e_mean, e_std, bound),
          flush=True)
    assert e_mean <= bound and e_std <= bound
    assert isinstance(st.as_normal(), torch.distributions.Normal) and st.n == n


def test_ensemble_update_scalar_path_and_refusals():
    """a length that is not a multiple of 4 on bases that are not 16-byte aligned takes the scalar lanes: same numbers"""
    from climate_learn import _hip
    n, length = 5, 4099
    g = torch.Generator().manual_seed(12)
    buf = torch.randn(n, length + 1, generator=g).cuda()
    mean_b, m2_b = torch.empty(length + 1, device="cuda"), torch.empty(length + 1, device="cuda")
    mean, m2 = mean_b[1:], m2_b[1:]
    assert mean.data_ptr() % 16 == 4
    for k in range(n):
        _hip.ensemble_update(buf[k, 1:], mean, m2, k + 1)
    ref = buf[:, 1:].double()
    bound = _welford_bound(buf)
    assert float((mean.double() - ref.mean(0)).abs().max()) <= bound
    assert float(((m2 / (n - 1)).sqrt().double() - ref.std(0)).abs().max()) <= bound
    with pytest.raises(_hip.HipBackendError, match="one shape"):
        _hip.ensemble_update(buf[0], mean, m2, 1)
    with pytest.raises(_hip.HipBackendError, match="code -1"):
        _hip.ensemble_update(buf[0, 1:], mean, m2, 0)
    with pytest.raises(_hip.HipBackendError, match="code -1"):
        _hip.ensemble_update(buf[0, 1:], mean, mean, 2)


@pytest.mark.parametrize("div,overlap", [(1, 0), (2, 4)])
def test_streaming_statistics_equal_stacking(div, overlap):
    import climate_learn as cl
    from climate_learn.utils import enable_dropout, get_monte_carlo_predictions, mc_dropout_statistics, tiled_predict
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.1)
    x, y = x.cuda(), y.cuda()
    batch = (x, y, in_vars, out_vars)
    n = 8
    cl.manual_seed(9)
    st = mc_dropout_statistics(batch, model, n, div=div, overlap=overlap)
    assert tuple(model.img_size) == GRID                                   # the tiled run gave the model its grid back
    cl.manual_seed(9)
    if div == 1:
        stack = get_monte_carlo_predictions(batch, model, n)
    else:
        model.eval()
        enable_dropout(model)
        stack = torch.stack([tiled_predict(model, x, y, in_vars, out_vars, div, overlap) for _ in range(n)])
    assert st.mean.shape == stack.shape[1:] and st.n == n
    assert not torch.equal(stack[0], stack[1])
    bound = _welford_bound(stack)
    e_mean = float((st.mean.double() - stack.double().mean(0)).abs().max())
    e_std = float((st.std.double() - stack.double().std(0)).abs().max())
    print("[streaming div %d] max |mean err| %.3e  max |std err| %.3e  bound %.3e" % (div, e_mean, e_std, bound), flush=True)
    assert e_mean <= bound and e_std <= bound
    assert float(st.std.max()) > 0


def test_streaming_peak_memory_does_not_grow_with_members():
    from climate_learn.utils import mc_dropout_statistics
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.1)
    batch = (x.cuda(), y.cuda(), in_vars, out_vars)
    mc_dropout_statistics(batch, model, 2)                                # warm-up: caches, compute copies
    peaks = {}
    for n in (4, 16):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        st = mc_dropout_statistics(batch, model, n)
        torch.cuda.synchronize()
        peaks[n] = torch.cuda.max_memory_allocated()
        one = st.mean.numel() * 4
        del st
    print("[streaming memory] peak at N=4 %d B, at N=16 %d B, one prediction %d B" % (peaks[4], peaks[16], one), flush=True)
    assert peaks[16] - peaks[4] < one


def test_mc_mode_through_the_data_parallel_wrapper():
    import torch.nn as nn
    import climate_learn as cl
    from climate_learn.models.hub.components.vit_blocks import Block
    from climate_learn.utils import enable_dropout, mc_dropout_statistics
    from oracle.harness import nerr
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.1)
    batch = (x.cuda(), y.cuda(), in_vars, out_vars)
    cl.manual_seed(4)
    plain = mc_dropout_statistics(batch, model, 4)
    model.eval()
    eng = cl.HipDataParallel(model, unit_types=(Block, nn.Sequential)).eval()
    enable_dropout(eng)
    assert model.mc_dropout and model.blocks[2].mlp.mc_dropout
    eng.eval()
    assert not model.mc_dropout
    cl.manual_seed(4)
    wrapped = mc_dropout_statistics(batch, eng, 4)
    assert model.mc_dropout and float(wrapped.std.max()) > 0
    assert nerr(wrapped.mean, plain.mean) <= TOL


# ---------------------------------------------------------------------------------------------------------------- scores
def _crps_closed_form(mean, std, target):
    """the closed form of the Gaussian CRPS in the tensors' own precision (fp64 on the host)"""
    z = (target - mean) / std
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    return std * (z * (2 * cdf - 1) + 2 * pdf - 1 / math.sqrt(math.pi))


def _lat_w(lat):
    w = np.cos(np.deg2rad(lat))
    return torch.from_numpy(w / w.mean()).float().view(1, 1, -1, 1)


def test_gaussian_spread_and_ratio_match_reference_golden(golden_dir):
    from climate_learn.metrics import functional as fn
    z = np.load(os.path.join(golden_dir, "probabilistic.npz"))
    mean, std, target = (torch.from_numpy(z[k]).cuda() for k in ("mean", "std", "target"))
    pred = torch.distributions.Normal(mean, std)
    wl = _lat_w(z["lat"])
    kw = dict(rtol=2e-5, atol=2e-6)
    assert np.allclose(fn.gaussian_spread(pred).cpu().numpy(), z["spread"], **kw)
    assert np.allclose(float(fn.gaussian_spread(pred, True)), z["spread.agg"], **kw)
    assert np.allclose(fn.gaussian_spread(pred, False, wl).cpu().numpy(), z["lat_spread"], **kw)
    assert np.allclose(float(fn.gaussian_spread(pred, True, wl)), z["lat_spread.agg"], **kw)
    assert np.allclose(fn.gaussian_spread_skill_ratio(pred, target).cpu().numpy(), z["ratio"], **kw)
    assert np.allclose(float(fn.gaussian_spread_skill_ratio(pred, target, True)), z["ratio.agg"], **kw)
    assert np.allclose(fn.gaussian_spread_skill_ratio(pred, target, False, wl).cpu().numpy(), z["lat_ratio"], **kw)
    assert np.allclose(float(fn.gaussian_spread_skill_ratio(pred, target, True, wl)), z["lat_ratio.agg"], **kw)
    assert float(z["reference_crps_callable"]) == 0.0                       # why the CRPS has no recorded reference value


def test_gaussian_crps_matches_the_closed_form(golden_dir):
    from climate_learn.metrics import functional as fn
    z = np.load(os.path.join(golden_dir, "probabilistic.npz"))
    mean, std, target = (torch.from_numpy(z[k]) for k in ("mean", "std", "target"))
    pred = torch.distributions.Normal(mean.cuda(), std.cuda())
    kw = dict(rtol=2e-5, atol=2e-6)
    for wl in (None, _lat_w(z["lat"])):
        c = _crps_closed_form(mean.double(), std.double(), target.double())
        if wl is not None:
            c = c * wl.double()
        want = torch.cat((c.mean([0, 2, 3]), c.mean().unsqueeze(0))).numpy()
        got = fn.gaussian_crps(pred, target.cuda(), False, wl)
        assert got.dtype == torch.float32 and np.allclose(got.cpu().numpy(), want, **kw), (got, want)
        assert np.allclose(float(fn.gaussian_crps(pred, target.cuda(), True, wl)), want[-1], **kw)
    # a target larger than the prediction is consumed through its top-left crop
    big = torch.zeros(3, 3, 30, 47)
    big[:, :, :24, :40] = target
    assert torch.equal(fn.gaussian_crps(pred, big.cuda()), fn.gaussian_crps(pred, target.cuda()))


def test_gaussian_crps_closed_form_is_the_defining_integral():
    """three points against scipy's quadrature of the integral of (F(x) - 1{x >= y})^2: this pins the 1 / sqrt(pi) term (the
    reference's text has 1 / pi: 0.96275550 where the integral is 0.54476001 at the first point)"""
    from scipy.integrate import quad
    from scipy.stats import norm
    from climate_learn import _hip
    pts = [(0.3, 1.7, 1.1), (-2.0, 0.4, -1.7), (280.0, 3.0, 271.5)]
    for mu, sg, yv in pts:
        lo = quad(lambda t: norm.cdf(t, mu, sg) ** 2, mu - 40 * sg, yv, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        hi = quad(lambda t: (norm.cdf(t, mu, sg) - 1) ** 2, yv, mu + 40 * sg, epsabs=1e-13, epsrel=1e-13, limit=400)[0]
        closed = float(_crps_closed_form(torch.tensor(mu, dtype=torch.float64), torch.tensor(sg, dtype=torch.float64),
                                         torch.tensor(yv, dtype=torch.float64)))
        assert abs(closed - (lo + hi)) <= 1e-6 * (lo + hi), (mu, sg, yv, closed, lo + hi)
    assert abs(float(_crps_closed_form(*(torch.tensor(v, dtype=torch.float64) for v in pts[0]))) - 0.54476001) < 1e-8
    mu, sg, yv = (torch.tensor([p[i] for p in pts], dtype=torch.float32).view(1, 3, 1, 1).cuda() for i in range(3))
    got = _hip.gaussian_scores(mu, sg, yv)[0, :, 0].cpu()
    want = _crps_closed_form(mu.double(), sg.double(), yv.double()).view(3).cpu()
    assert torch.allclose(got, want, rtol=2e-5, atol=2e-6), (got, want)


def test_zero_spread_is_a_normal_case():
    """a channel whose std is exactly 0 (constant output channels are copied from the target into every member): crps is
    mean |target - mean| there, every output finite, a point covered only where target == mean"""
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    g = torch.Generator().manual_seed(3)
    mean = torch.randn(2, 3, 16, 24, generator=g)
    std = torch.rand(2, 3, 16, 24, generator=g) + 0.1
    target = mean + torch.randn(2, 3, 16, 24, generator=g)
    std[:, 1] = 0.0
    target[:, 1, :4] = mean[:, 1, :4]                                     # a quarter of that channel hits exactly
    std[0, 2, 0, 0] = 1e-42                                               # a denormal spread: z overflows, the score must not
    pred = torch.distributions.Normal(mean.cuda(), std.cuda(), validate_args=False)
    crps = fn.gaussian_crps(pred, target.cuda())
    spread = fn.gaussian_spread(pred)
    ratio = fn.gaussian_spread_skill_ratio(pred, target.cuda())
    cover = fn.gaussian_coverage(pred, target.cuda())
    for t in (crps, spread, ratio, cover):
        assert torch.isfinite(t).all(), t
    want = float((target[:, 1] - mean[:, 1]).abs().double().mean())
    assert abs(float(crps[1]) - want) <= 2e-5 * want + 2e-6
    assert float(spread[1]) == 0.0 and float(ratio[1]) == 0.0
    assert abs(float(cover[1]) - 0.25) < 1e-6
    raw = _hip.gaussian_scores(mean.cuda(), std.cuda(), target.cuda())
    assert raw.shape == (2, 3, 4) and raw.dtype == torch.float64 and torch.isfinite(raw).all()
    assert float(raw[:, 1, 3].sum()) == 2 * 4 * 24


def test_gaussian_scores_refuse_bad_arguments():
    from climate_learn import _hip
    lib = _hip.lib()
    a = torch.ones(1, 2, 8, 8, device="cuda")
    out = torch.full((1, 2, 4), -7.0, dtype=torch.float64, device="cuda")
    p, st = a.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert lib.orbit2_gaussian_scores(None, p, p, 8, 8, None, out.data_ptr(), 1, 2, 8, 8, st) == -1
    assert lib.orbit2_gaussian_scores(p, p, p, 8, 8, None, None, 1, 2, 8, 8, st) == -1
    assert lib.orbit2_gaussian_scores(p, p, p, 7, 8, None, out.data_ptr(), 1, 2, 8, 8, st) == -1       # target smaller
    assert lib.orbit2_gaussian_scores(p, p, p, 8, 6, None, out.data_ptr(), 1, 2, 8, 8, st) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == -7.0 == float(out.max())                    # refused before anything was launched
    with pytest.raises(_hip.HipBackendError, match="differ in shape"):
        _hip.gaussian_scores(a, a[:, :, :4].contiguous(), a)
    with pytest.raises(_hip.HipBackendError, match="code -1"):
        _hip.gaussian_scores(a, a, a[:, :, :4].contiguous())
    with pytest.raises(_hip.HipBackendError, match="lat_w"):
        _hip.gaussian_scores(a, a, a, torch.ones(4, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- driver
def _run_driver(cfg, cwd):
    env = dict(os.environ, MASTER_PORT=str(free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "visualize.py"), cfg], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


_NUM = re.compile(r"[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?|\binf\b|\bnan\b")


def test_inference_driver_mc_dropout_block(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_mc.yaml")))
    plain_conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference.yaml")))
    assert conf["mc_dropout"] == {"members": 16, "seed": 0}
    assert {k: v for k, v in conf.items() if k != "mc_dropout"} == plain_conf          # the example = inference.yaml + the block
    for c in (conf, plain_conf):
        c["model"].update(embed_dim=256, depth=2, decoder_depth=1, num_heads=4)
        c["data"]["synthetic"]["ERA5_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256])
    conf["mc_dropout"] = {"members": 4, "seed": 3}
    mc_dir, plain_dir = os.path.join(tmp_path, "mc"), os.path.join(tmp_path, "plain")
    outs = {}
    for d, c in ((mc_dir, conf), (plain_dir, plain_conf)):
        os.makedirs(d)
        cfg = os.path.join(d, "inf.yaml")
        yaml.safe_dump(c, open(cfg, "w"))
        outs[d] = _run_driver(cfg, d).splitlines()
    mc, plain = outs[mc_dir], outs[plain_dir]
    # without the block: today's output, line for line -- and the run with the block starts with exactly those lines.  The
    # lines are compared with their numbers masked: the driver builds the model from unseeded random weights when no
    # `trainer.pretrain` is given, so two processes print different metric values (12.04 against 11.75 dB PSNR seen)
    assert not any("mc_dropout" in ln or "gaussian" in ln for ln in plain)
    assert plain[-1].startswith("mean_bias [") and len(mc) == len(plain) + 6
    for a, b in zip(plain, mc):
        assert _NUM.sub("#", a) == _NUM.sub("#", b), (a, b)
        assert len(_NUM.findall(a)) == len(_NUM.findall(b)), (a, b)
    assert not os.path.exists(os.path.join(plain_dir, "0_mc_mean.npy"))
    tail = mc[len(plain):]
    assert tail[0] == "mc_dropout members 4 seed 3"
    for ln, name in zip(tail[1:5], ("gaussian_crps", "gaussian_spread", "gaussian_spread_skill_ratio", "coverage_1sigma")):
        m = re.match(name + r" \[([^\]]+)\]$", ln)
        assert m, ln
        vals = [float(v) for v in m.group(1).split(",")]
        assert len(vals) == 4 and all(v == v and abs(v) != float("inf") for v in vals), ln     # 3 channels + aggregate, finite
        assert all(v >= 0 for v in vals)
    assert tail[5].startswith("mc_dropout saved")
    mean, spread = np.load(os.path.join(mc_dir, "0_mc_mean.npy")), np.load(os.path.join(mc_dir, "0_mc_spread.npy"))
    assert mean.shape == spread.shape == (1, 3, 128, 256)                   # the stitched size
    assert np.isfinite(mean).all() and np.isfinite(spread).all() and (spread >= 0).all() and spread.max() > 0


def test_driver_report_scales_the_spread_without_shifting_it(tmp_path, monkeypatch, capsys):
    """the driver's report with a denormalisation of scale 2 and shift 270 (the synthetic data module's is the identity): the
    mean is scaled and shifted, the spread scaled only"""
    import importlib.util
    import climate_learn as cl
    from climate_learn.utils import mc_dropout_statistics
    spec = importlib.util.spec_from_file_location("orbit2_visualize_driver", os.path.join(ROOT, "examples", "visualize.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    monkeypatch.chdir(tmp_path)
    model, sd, cfg, O, x, y, in_vars, out_vars = _pair(0.1)
    batch = (x.cuda(), y.cuda(), in_vars, out_vars)
    denorm = lambda t: t * 2.0 + 270.0                                     # noqa: E731
    gt = denorm(y.cuda()[:, :, : 4 * GRID[0], : 4 * GRID[1]].float())
    res = drv.mc_dropout_report(model, batch, gt, denorm, 3, 21, 1, 0, 0)
    assert not model.mc_dropout                                            # the report leaves the mode
    cl.manual_seed(21)
    st = mc_dropout_statistics(batch, model, 3)
    assert np.array_equal(res["mean"], (st.mean * 2.0 + 270.0).cpu().numpy())
    assert np.allclose(res["spread"], (st.std * 2.0).cpu().numpy(), rtol=1e-6, atol=1e-4) and res["spread"].max() < 100.0
    assert np.array_equal(np.load(os.path.join(tmp_path, "0_mc_spread.npy")), res["spread"])
    out = capsys.readouterr().out
    assert "gaussian_crps [" in out and "coverage_1sigma [" in out
