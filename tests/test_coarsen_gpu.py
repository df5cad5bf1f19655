"""The adjoint of the antialiased resample on the device (_hip.resample_adjoint: orbit2_resample_fwd at mode codes 21 and 22)
against its float64 statement (tests/coarsen_ref.py), then through _ops.CoarsenFn, metrics.functional.consistency_mse, the
registered losses and training_step.

Cases (coarsen_ref.GPU_CASES, fine -> coarse), each in both modes at offsets 0 and 280, B = 2, C = 3: integer 8x, 10x, 4x over
several 32 x 64 tiles, a non-integer pair with an odd width, 300x7 -> 1x1 and 7x300 -> 1x1, the identity (bit-exact), and fine
sizes one past a tile and one short of it near ratios 4 and 2.5.  The output is written into a NaN-filled buffer with guards on
both sides, on a 16-byte boundary and off it.

Bound (derived in tests/test_coarsen_cpu.py): |kernel - adjoint64| <= coarsen_ref.field_tol(mode) * max|g| = min(4 x the
emulation's worst, the ceiling): 1.36 ulp (bilinear) and 2.12 ulp (bicubic) of max|g|; 0 for the identity."""
import numpy as np
import pytest
import torch

from tests import coarsen_ref as C
from tests import resample_aa_ref as A
from tests import resample_ref as R
from tests._child import run_child

pytestmark = pytest.mark.gpu
GUARD = 64
CASE_IDS = ["%dx%d_%dx%d" % (f + c) for f, c in C.GPU_CASES]
LOSS_TOL = 2e-5                                      # tests/test_hip_ops.py::test_loss: the fused mse against the oracle's


def nerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def _code(mode):
    from climate_learn import _hip
    return _hip.RESAMPLE_MODES[mode] | _hip.ANTIALIAS | _hip.TRANSPOSE


def _adjoint_into_guards(g, fine, mode, lead):
    """the entry itself, writing into the middle of a NaN-filled buffer; returns the field and checks nothing else was written"""
    from climate_learn import _hip
    B, Cc, h, w = g.shape
    n = B * Cc * fine[0] * fine[1]
    buf = torch.full((lead + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[lead:lead + n]
    rc = _hip.lib().orbit2_resample_fwd(g.data_ptr(), None, Cc, None, None, out.data_ptr(), B, Cc, h, w, fine[0], fine[1],
                                        _code(mode), None)
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[:lead]).all() and np.isnan(host[lead + n:]).all(), "wrote outside the output"
    field = host[lead:lead + n].reshape(B, Cc, *fine)
    assert not np.isnan(field).any(), "left pixels unwritten"
    return field


@pytest.mark.parametrize("fine,coarse", C.GPU_CASES, ids=CASE_IDS)
def test_adjoint_against_float64(fine, coarse):
    from climate_learn import _hip
    worst = dict.fromkeys(C.MODES, 0.0)
    for off in C.OFFSETS:
        gh = C.gpu_input(coarse, off)
        g = torch.from_numpy(gh).cuda()
        gmax = float(np.abs(gh).max())
        for mode in C.MODES:
            want = C.adjoint64(gh, fine, mode)
            tol = 0.0 if fine == coarse else C.field_tol(mode) * gmax
            for lead in (GUARD, GUARD - 3):                # the output on a 16-byte boundary, and off it
                got = _adjoint_into_guards(g, fine, mode, lead)
                err = float(np.abs(got.astype(np.float64) - want).max())
                worst[mode] = max(worst[mode], err / gmax)
                print("%s %s offset %d lead %d: worst %.4g = %.3g ulp(max|g|), bound %.4g"
                      % (R.case_key(fine, coarse), mode, off, lead, err, err / gmax / C.ULP, tol))
                assert err <= tol
                if fine == coarse:
                    assert np.array_equal(got, gh), "the identity is not exact"
            # the wrapper is that call, and two calls give the same bits
            a, b = _hip.resample_adjoint(g, fine, mode), _hip.resample_adjoint(g, fine, mode)
            assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), got)
    print("worst |kernel - adjoint64| / max|g| in ulp:", {m: round(v / C.ULP, 3) for m, v in worst.items()})


@pytest.mark.parametrize("fine,coarse", C.GPU_CASES[:4] + C.GPU_CASES[7:], ids=CASE_IDS[:4] + CASE_IDS[7:])
def test_dot_product_identity(fine, coarse):
    """<A p, g> = <p, A^T g> with both kernels on the device and both sums in float64 on the host: they share their fp32 weights
    bit for bit, so what is left is the two kernels' summation error, bounded by their field bounds times sum|p| max|g|"""
    from climate_learn import _hip
    ph = R.make_input(fine, 2, 3, seed=fine[0] * 7 + fine[1])
    gh = C.gpu_input(coarse, 0.0)
    p, g = torch.from_numpy(ph).cuda(), torch.from_numpy(gh).cuda()
    for mode in C.MODES:
        lhs = float((_hip.resample(p, coarse, mode, antialias=True).cpu().double() * g.cpu().double()).sum())
        rhs = float((p.cpu().double() * _hip.resample_adjoint(g, fine, mode).cpu().double()).sum())
        bound = (A.field_tol(mode, fine, coarse) + C.field_tol(mode)) * float(np.abs(ph).sum()) * float(np.abs(gh).max())
        print("%s %s: <Ap, g> %.9g, <p, A^T g> %.9g, difference %.3g, bound %.3g"
              % (R.case_key(fine, coarse), mode, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound


def test_entry_refusals_on_real_buffers():
    from climate_learn import _hip
    g = torch.randn(2, 3, 4, 5, device="cuda")
    out = torch.full((2, 3, 9, 13), float("nan"), device="cuda")
    small = torch.full((2, 3, 2, 3), float("nan"), device="cuda")
    call = lambda m, o, H, W: _hip.lib().orbit2_resample_fwd(g.data_ptr(), None, 3, None, None, o.data_ptr(), 2, 3, 4, 5, H, W, m,  # noqa: E731
                                                             None)
    assert [call(m, out, 9, 13) for m in (21, 22)] == [0, 0]
    assert [call(m, small, 2, 3) for m in (21, 22)] == [-1, -1]               # an upsampling pair
    assert [call(m, out, 9, 13) for m in (16, 17, 20, 18, 23, 29)] == [-1] * 6
    assert [call(m, out, 3, 13) for m in (21, 22)] == [-1, -1] and [call(m, out, 9, 4) for m in (21, 22)] == [-1, -1]
    torch.cuda.synchronize()
    assert torch.isnan(small).all() and torch.isfinite(out).all()
    with pytest.raises(_hip.HipBackendError, match="coarsening"):
        _hip.resample_adjoint(g, (2, 3))
    # the forward wrappers still refuse a field that requires grad
    with pytest.raises(_hip.HipBackendError, match="requires grad"):
        _hip.resample(out.requires_grad_(), (4, 5), "bilinear", antialias=True)


# ---- consistency_mse ----------------------------------------------------------------------------------------------------------
IN_VARS = ["land_sea_mask", "orography", "2m_temperature", "total_precipitation_24hr", "10m_u_component_of_wind"]
OUT_VARS = ["total_precipitation_24hr", "2m_temperature", "orography"]
CHANNELS = [3, 2, 1]
VW = {"2m_temperature": 10.0, "total_precipitation_24hr": 1.0}


def _restate(pred, source, mode, channels, rescale, lat, chan_w):
    """consistency_mse in float64 torch on the CPU from the dense axis matrices: ([C + 1] value, its gradient in pred, the
    gradient of the aggregate in the coarsened field)"""
    B, Cc, H, W = pred.shape
    s = H // source.shape[2]
    hc, wc = H // s, W // s
    ay, ax = (torch.from_numpy(C.dense(mode, n, m).astype(np.float64)) for n, m in ((H, hc), (W, wc)))
    p = pred.detach().cpu().double().requires_grad_()
    coarse = torch.einsum("oY,bcYX,pX->bcop", ay, p, ax)
    coarse.retain_grad()
    given = source.cpu().double()[:, channels][:, :, :hc, :wc]
    if rescale is not None:
        given = given * torch.tensor(rescale[0], dtype=torch.float64).view(1, -1, 1, 1) \
            + torch.tensor(rescale[1], dtype=torch.float64).view(1, -1, 1, 1)
    err = (coarse - given).square()
    if lat is not None:
        err = err * lat.double()[:hc].view(1, 1, -1, 1)
    if chan_w is not None:
        err = err * torch.tensor(chan_w, dtype=torch.float64).view(1, -1, 1, 1)
    out = torch.cat((err.mean([0, 2, 3]), err.mean().unsqueeze(0)))
    out[-1].backward()
    return out.detach(), p.grad, coarse.grad


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("lat,weights,rescale", [(False, False, False), (True, True, True), (True, False, False),
                                                 (False, True, True)])
def test_consistency_mse_value_and_gradient(mode, lat, weights, rescale):
    """pred [2,3,32,48] against source [2,5,8,14], of which the prediction covers the first 12 columns (with s = H // h, as
    utils.visualize.consistency_scores has it, the rows of a source always equal H // s: only its columns can exceed the
    prediction's; a source of 9 rows gives s = 3 and is refused as one the prediction does not coarsen onto).  The value within the
    fused mse's own tolerance of the float64 restatement.  The gradient: the adjoint of the kernel's own upstream gradient
    within the adjoint bound times that gradient's magnitude; and against the restatement, that plus what the fused mse's
    backward may differ by (LOSS_TOL of the upstream magnitude, passed through weights whose column sums are at most 1)."""
    from climate_learn import _hip
    from climate_learn.metrics import functional as fn
    gen = torch.Generator().manual_seed(11)
    pred = torch.randn(2, 3, 32, 48, generator=gen).cuda().requires_grad_()
    source = torch.randn(2, 5, 8, 12 + 2, generator=gen).cuda()
    lw = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-70, 70, 8)))).float() if lat else None
    names, vw = (OUT_VARS, VW) if weights else (None, None)
    rs = ([1.25, 0.5, 1.0], [0.1, -0.2, 0.0]) if rescale else None
    out = fn.consistency_mse(pred, source, names, vw, False, lw, mode, CHANNELS, rs)
    assert tuple(out.shape) == (4,) and out.dtype == torch.float32
    out[-1].backward()
    agg = fn.consistency_mse(pred.detach(), source, names, vw, True, lw, mode, CHANNELS, rs)
    assert agg.dim() == 0 and torch.equal(agg, out[-1])
    want, wgrad, wup = _restate(pred, source, mode, CHANNELS, rs, lw, [1.0, 10.0, 1.0] if weights else None)
    print("%s lat %d weights %d rescale %d: value %s, restated %s" % (mode, lat, weights, rescale, out.tolist(), want.tolist()))
    assert nerr(out, want) < LOSS_TOL
    # the upstream gradient the backward saw, recomputed by the same two calls
    coarse = _hip.resample(pred.detach(), (8, 12), mode, antialias=True)
    given = fn._consistency_given(source, CHANNELS, rs, pred.device)
    up = _hip.loss_bwd(coarse, given, fn._lat(lw, coarse), fn._chan_weights(coarse, names, vw), torch.ones(1, device="cuda"), 0)
    upmax = float(up.abs().max())
    assert nerr(up, wup) < LOSS_TOL
    own = C.adjoint64(up.cpu().numpy(), (32, 48), mode)
    e_own = float(np.abs(pred.grad.cpu().numpy().astype(np.float64) - own).max())
    e_all = float((pred.grad.cpu().double() - wgrad).abs().max())
    print("    gradient: against the adjoint of its own upstream %.3g (bound %.3g), against the restatement %.3g (bound %.3g)"
          % (e_own, C.field_tol(mode) * upmax, e_all, (C.field_tol(mode) + LOSS_TOL) * upmax))
    assert e_own <= C.field_tol(mode) * upmax
    assert e_all <= (C.field_tol(mode) + LOSS_TOL) * upmax


def test_consistency_mse_refusals():
    from climate_learn.metrics import functional as fn
    from climate_learn.models.hub import Interpolation
    pred = torch.randn(2, 3, 32, 48, device="cuda")
    source = torch.randn(2, 5, 8, 14, device="cuda")
    with pytest.raises(ValueError, match="does not coarsen onto"):
        fn.consistency_mse(pred, source[:, :, :, :11], channels=CHANNELS)
    with pytest.raises(TypeError, match="Resampled"):
        fn.consistency_mse(Interpolation(size=(32, 48)).lazy(source, IN_VARS, OUT_VARS), source, channels=CHANNELS)
    # a bf16 prediction is taken as the fused losses take one
    out = fn.consistency_mse(pred.bfloat16().requires_grad_(), source, channels=CHANNELS)
    assert out.dtype == torch.float32 and torch.isfinite(out).all()


# ---- the registered losses through training_step ------------------------------------------------------------------------------------
# the model wants its four constant fields among the inputs; no constant among the outputs (clip_replace_constant writes one
# into the clamped prediction in place, which the clamp's backward refuses)
MODEL_IN = ["land_sea_mask", "orography", "lattitude", "landcover", "2m_temperature", "total_precipitation_24hr"]
MODEL_CHANNELS = [5, 4]
MODEL_OUT = ["total_precipitation_24hr", "2m_temperature"]


def test_training_step_with_the_consistency_loss():
    """a one-block Res_Slim_ViT on a 16 x 32 grid takes one step of bayesian_tv_consistency: the loss is bayesian_tv + weight x
    consistency_mse of the same prediction, and every parameter gets a finite gradient"""
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.metrics import BayesianTVConsistency
    from climate_learn.metrics.utils import MetricsMetaInfo
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.trainer import clip_replace_constant, training_step
    torch.manual_seed(3)
    grid = (16, 32)
    model = Res_Slim_ViT(MODEL_IN, grid, len(MODEL_IN), len(MODEL_OUT), 1, patch_size=2, embed_dim=128, depth=1, decoder_depth=1,
                         num_heads=2, drop_path=0.0, drop_rate=0.0, learn_pos_emb=True).cuda().eval()
    model.data_config(156.0, grid, len(MODEL_IN), len(MODEL_OUT))
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, len(MODEL_IN), *grid, generator=gen).cuda()
    y = torch.randn(2, len(MODEL_OUT), 4 * grid[0], 4 * grid[1], generator=gen).cuda()
    loss_obj = BayesianTVConsistency(aggregate_only=True, metainfo=MetricsMetaInfo(MODEL_IN, MODEL_OUT, None, None, None))
    loss_obj.weight, loss_obj.mode = 0.5, "bicubic"
    rescale = ([1.25, 0.5], [0.1, -0.2])
    loss_obj.set_rescale(*rescale)
    dev = torch.device("cuda:0")
    loss = training_step((x, y, MODEL_IN, MODEL_OUT), 0, model, dev, VW, loss_obj)
    assert loss.dim() == 0 and loss_obj._source.data_ptr() == x.data_ptr()
    loss.backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        pred = clip_replace_constant(y, model(x, MODEL_IN, MODEL_OUT), MODEL_OUT)
    base = fn.bayesian_tv(pred, y, MODEL_OUT, VW, True)
    term = fn.consistency_mse(pred, x, MODEL_OUT, {"total_precipitation_24hr": 1.0, "2m_temperature": 10.0},
                              True, None, "bicubic", MODEL_CHANNELS, rescale)
    print("loss %.7g = bayesian_tv %.7g + 0.5 x consistency %.7g" % (float(loss.detach()), float(base), float(term)))
    assert float(term) > 0 and abs(float(loss) - float(base + 0.5 * term)) <= 1e-6 * abs(float(loss))
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert len(grads) > 25 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()), \
        [n for n, g in grads.items() if g is None or not bool(torch.isfinite(g).all())]
    assert any(float(g.abs().max()) > 0 for g in grads.values())
    # an output variable that is not among the step's inputs is named
    loss_obj.set_source(x, MODEL_IN[:4] + ["geopotential_500", "total_precipitation_24hr"])
    with pytest.raises(RuntimeError, match="among the input variables"):
        loss_obj(pred, y, var_names=MODEL_OUT, var_weights=VW)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def child_graph_capture_of_the_consistency_loss():
    """forward + backward of consistency_mse captured once (one stream) on static tensors, replayed on new contents: loss and
    gradient equal an eager call on the new data bit for bit -- no host read, no host-to-device copy in the step"""
    from climate_learn.metrics import functional as fn
    gen = torch.Generator().manual_seed(21)
    sp = torch.randn(2, 3, 32, 48, generator=gen).cuda().requires_grad_()
    ss = torch.randn(2, 5, 8, 14, generator=gen).cuda()
    lw = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-70, 70, 8)))).float().cuda()
    rs = ([1.25, 0.5, 1.0], [0.1, -0.2, 0.0])
    f = lambda p, s: fn.consistency_mse(p, s, OUT_VARS, VW, True, lw, "bicubic", CHANNELS, rs)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up outside the capture: the cached index and weights upload here
        f(sp, ss).backward()
    torch.cuda.current_stream().wait_stream(side)
    sp.grad = None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        lv = f(sp, ss)
        lv.backward()
    newp, news = torch.randn(2, 3, 32, 48, generator=gen).cuda(), torch.randn(2, 5, 8, 14, generator=gen).cuda()
    with torch.no_grad():
        sp.copy_(newp)
    ss.copy_(news)
    gr.replay()
    torch.cuda.synchronize()
    ep = newp.clone().requires_grad_()
    ev = f(ep, news)
    ev.backward()
    assert float(ev) > 0 and torch.equal(lv, ev) and torch.equal(sp.grad, ep.grad)


def test_graph_capture_of_the_consistency_loss():
    run_child(__file__, "child_graph_capture_of_the_consistency_loss", timeout=300)


# ---- the training driver ---------------------------------------------------------------------------------------------------------------
def test_training_driver_runs_the_consistency_config(tmp_path):
    """configs/interm_8m_consistency.yaml through examples/intermediate_downscaling.py at one Block and batch 2: the loader sets
    the rescale, the graphed step hands its static input to the loss, `trainer.consistency` reaches the loss object"""
    import os
    import re
    import subprocess
    import sys
    import yaml
    from tests._child import free_port
    from tests.conftest import ROOT
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m_consistency.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2, consistency={"weight": 0.5, "mode": "bicubic"})
    conf["model"].update(depth=1, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)

    cfg = os.path.join(tmp_path, "c.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "intermediate_downscaling.py"), cfg],
                       cwd=tmp_path, env=dict(os.environ, MASTER_PORT=str(free_port())), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", r.stdout)]
    assert len(losses) == 4 and all(v == v and 0 < v < 1e4 for v in losses)
