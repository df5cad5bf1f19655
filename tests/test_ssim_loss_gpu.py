"""The SSIM training loss on the device: the vector-Jacobian kernel (orbit2_loss_bwd at kind 3) against the float64
autograd reference of tests/ssim_loss_ref.py within the field tolerance derived in tests/test_ssim_loss_cpu.py; containment of an
image of coefficient 0; repeatable bits; kinds 0..2 as they were; _ops.SSIMFn and metrics.functional.ssim_loss; one model step."""
import numpy as np
import pytest
import torch

from tests import rowimage_ref as R
from tests import ssim_loss_ref as S
from tests._child import run_child

pytestmark = pytest.mark.gpu
GUARD = 64
CASE_IDS = ["%dx%d_%dx%d" % (hw + thw) for hw, thw, _ in S.GPU_CASES]


def _vjp_into_guards(pred, target, lat_w, coef, rng, lead):
    """the entry itself, writing into the middle of a NaN-filled buffer; returns the field and checks nothing else was written
    and nothing was left unwritten"""
    from climate_learn import _hip
    B, Cc, H, W = pred.shape
    n = B * Cc * H * W
    buf = torch.full((lead + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[lead:lead + n]
    gscale = torch.stack((coef, rng)).contiguous()
    rc = _hip.lib().orbit2_loss_bwd(pred.data_ptr(), target.data_ptr(), target.shape[2], target.shape[3],
                                    None if lat_w is None else lat_w.data_ptr(), None, gscale.data_ptr(), out.data_ptr(), B, Cc,
                                    H, W, _hip.LOSS_SSIM_VJP, None)
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[:lead]).all() and np.isnan(host[lead + n:]).all(), "wrote outside the output"
    field = host[lead:lead + n].reshape(B, Cc, H, W)
    assert not np.isnan(field).any(), "left pixels unwritten"
    return field


def _dev(a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float32)).cuda()


@pytest.mark.parametrize("hw,thw,offsets", S.GPU_CASES, ids=CASE_IDS)
def test_vjp_against_float64(hw, thw, offsets):
    """B x C = 2 x 3 with distinct coefficients and given ranges, with and without lat_w, the output on a 16-byte boundary and
    off it: within the field tolerance of the float64 reference, relative to max|d| of the image"""
    from climate_learn import _hip
    coef, rng = _dev(S.GPU_COEF), _dev(S.GPU_RANGE)
    worst = 0.0
    for off in offsets:
        ph, th = S.make_pair(hw, thw, off)
        pred, target = _dev(ph), _dev(th)
        for lw in (None, S.lat_weights(hw[0])):
            want = S.vjp64(ph, th, lw, S.GPU_COEF, S.GPU_RANGE)
            for lead in (GUARD, GUARD - 3):
                got = _vjp_into_guards(pred, target, _dev(lw), coef, rng, lead)
                err = S.worst_error(got, want)
                worst = max(worst, err)
                print("%dx%d offset %d lat_w %d lead %d: worst %.4g of max|d|, bound %.4g"
                      % (hw + (off, lw is not None, lead, err, S.FIELD_TOL)))
                assert err <= S.FIELD_TOL
            # the wrapper is that call, and two calls give the same bits
            a = _hip.ssim_vjp(pred, target, _dev(lw), coef, rng)
            b = _hip.ssim_vjp(pred, target, _dev(lw), coef, rng)
            assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), got)
    print("worst |kernel - vjp64| / max|d|: %.4g = %.2f x the emulation's" % (worst, worst / S.EMUL_WORST))


def test_coefficient_zero_contains_its_image():
    """an image of coefficient 0 with a constant target (R = 0: S = 0 / 0) and NaN in its prediction: exactly 0, and the other
    images as without it; both guards untouched"""
    hw, thw = (39, 71), (41, 75)
    ph, th = S.make_pair(hw, thw, 280.0)
    th[0, 1] = 277.0
    ph[0, 1, 5, 9] = ph[0, 1, 38, 70] = np.nan
    th[1, 2, 0, 0] = np.inf                                     # the pivot of a skipped image's first tile
    coef = [list(r) for r in S.GPU_COEF]
    rng = [list(r) for r in S.GPU_RANGE]
    coef[0][1], rng[0][1] = 0.0, 0.0
    coef[1][2] = -0.0
    lw = S.lat_weights(hw[0])
    want = S.vjp64(ph, th, lw, coef, rng)                       # (the reference skips an image of coefficient 0 as well)
    for lead in (GUARD, GUARD - 3):
        got = _vjp_into_guards(_dev(ph), _dev(th), _dev(lw), _dev(coef), _dev(rng), lead)
        assert not got[0, 1].any() and not got[1, 2].any() and np.isfinite(got).all()
        err = S.worst_error(got, want)
        print("containment lead %d: worst %.4g of max|d|, bound %.4g" % (lead, err, S.FIELD_TOL))
        assert err <= S.FIELD_TOL


def test_entry_refusals_on_real_buffers():
    """the refusals of tests/test_ssim_loss_cpu.py with device addresses: nothing is written"""
    from climate_learn import _hip
    lib = _hip.lib()
    pred, target = torch.zeros(1, 1, 8, 8, device="cuda"), torch.zeros(1, 1, 8, 8, device="cuda")
    gs = torch.ones(2, device="cuda")
    out = torch.full((64,), float("nan"), device="cuda")
    p, t, g, o = pred.data_ptr(), target.data_ptr(), gs.data_ptr(), out.data_ptr()
    assert lib.orbit2_loss_bwd(p, t, 8, 8, None, g, g, o, 1, 1, 8, 8, 3, None) == -1            # chan_w
    assert lib.orbit2_loss_bwd(p, t, 8, 8, None, None, g, o, 1, 1, 6, 8, 3, None) == -1
    assert lib.orbit2_loss_bwd(p, t, 8, 8, None, None, g, o, 1, 1, 8, 6, 3, None) == -1
    assert lib.orbit2_loss_bwd(p, t, 8, 8, None, None, g, o, 256, 256, 8, 8, 3, None) == -1
    assert lib.orbit2_loss_bwd(p, t, 8, 8, None, None, g, o, 1, 1, 8, 8, 4, None) == -1
    assert lib.orbit2_loss_bwd(p, t, 8, 8, None, None, g, o, 1, 1, 8, 8, -1, None) == -1
    assert lib.orbit2_loss_fwd(p, t, 8, 8, None, None, o, o, 1, 1, 8, 8, 3, None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_kinds_0_to_2_are_as_they_were(kind):
    """orbit2_loss_bwd at kinds 0..2 through _hip.loss_bwd: the bound of tests/test_image_tail_edges_gpu.py against
    tests/rowimage_ref.py at 24 x 40, and the same bits twice"""
    from climate_learn import _hip
    gs = torch.tensor([R.LOSS_GSCALE])
    pred, tgt = R.loss_inputs(24, 40, True)
    latw = R.loss_latw(24, tgt.shape[2])
    cwd = torch.tensor(R.LOSS_CHANW).cuda()
    grad, G, _ = R.loss_bwd(pred, tgt, latw, R.LOSS_CHANW, float(gs), kind)
    a = _hip.loss_bwd(pred.cuda(), tgt.cuda(), latw.cuda(), cwd, gs.cuda(), kind)
    b = _hip.loss_bwd(pred.cuda(), tgt.cuda(), latw.cuda(), cwd, gs.cuda(), kind)
    assert torch.equal(a, b)
    assert R.excess(a, grad, 8 * R.EPS24 * G) <= 1.0


# ---- _ops.SSIMFn and metrics.functional.ssim_loss ------------------------------------------------------------------------------------
NAMES = ["2m_temperature", "land_sea_mask", "total_precipitation_24hr"]          # land_sea_mask is in CONSTANTS: coefficient 0
VW = {"2m_temperature": 10.0, "total_precipitation_24hr": 0.5}
# on the way into the kernel the coefficient -cw_c / (B C divisor) passes at most four fp32 roundings beyond the kernel's own
COEF_SLACK = 8 * 2.0 ** -24


@pytest.mark.parametrize("data_range", ["target", 5.0])
@pytest.mark.parametrize("lat", [False, True])
def test_ssim_loss_gradient_and_value(data_range, lat):
    from climate_learn.metrics import functional as fn
    hw, thw = (39, 71), (41, 75)
    ph, th = S.make_pair(hw, thw, 280.0)
    th[:, 1] = 1.0                                              # the constant variable: range 0, SSIM 0 / 0
    B, C = ph.shape[:2]
    lw = S.lat_weights(thw[0]) if lat else None
    pred = _dev(ph).requires_grad_(True)
    lat_t = None if lw is None else _dev(lw).view(1, 1, -1, 1)
    out = fn.ssim_loss(pred, _dev(th), NAMES, VW, False, lat_t, data_range)
    assert tuple(out.shape) == (C + 1,) and bool(torch.isfinite(out).all()) and float(out[1].detach()) == 0.0
    (g,) = torch.autograd.grad(out[-1], pred)
    crop = th[..., :hw[0], :hw[1]]
    rng = (crop.max((2, 3)).astype(np.float64) - crop.min((2, 3))).astype(np.float32) if data_range == "target" \
        else np.full((B, C), data_range, np.float32)
    div = (hw[0] - 6) * (hw[1] - 6) if lw is None else (hw[1] - 6) * float(lw[3:hw[0] - 3].astype(np.float64).sum())
    cw = [10.0, 0.0, 0.5]
    coef = [[-cw[c] / (B * C * div) for c in range(C)] for _ in range(B)]
    want = S.vjp64(ph, th, None if lw is None else lw[:hw[0]], coef, rng)
    err = S.worst_error(g.cpu().numpy(), want)
    print("ssim_loss gradient, data_range %r lat_w %d: worst %.4g of max|d|, bound %.4g" % (data_range, lat, err, S.FIELD_TOL + COEF_SLACK))
    assert err <= S.FIELD_TOL + COEF_SLACK and not bool(g[:, 1].any())
    # the value is 1 - ssim per channel
    plain = fn.ssim_loss(pred.detach(), _dev(th), None, None, False, lat_t, data_range)
    score = fn.ssim(pred.detach(), _dev(th), False, lat_t, None if data_range == "target" else data_range)
    for c in (0, 2):
        assert abs(float(plain[c]) - (1.0 - float(score[c]))) <= 1e-6
        assert abs(float(out[c]) - cw[c] * float(plain[c])) <= 1e-6 * cw[c]
    assert abs(float(out[-1]) - float(out[:C].mean())) <= 1e-6


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------
def child_graph_capture_of_the_ssim_loss():
    """forward + backward of ssim_loss captured once (one stream) on static tensors, replayed on a second batch: the gradient equals
    an eager call on the new data bit for bit (the kernel has no atomics, its coefficient and range are formed on the device), the
    value to fp32 rounding (the forward's sums are added across workgroups by double atomics, in any order)"""
    from climate_learn.metrics import functional as fn
    hw, thw = (39, 71), (41, 75)
    ph, th = S.make_pair(hw, thw, 280.0, seed=5)
    th[:, 1] = 1.0
    sp, st = _dev(ph).requires_grad_(), _dev(th)
    lw = _dev(S.lat_weights(thw[0])).view(1, 1, -1, 1)
    f = lambda p, t: fn.ssim_loss(p, t, NAMES, VW, True, lw, "target")      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up outside the capture: the cached weights upload here
        f(sp, st).backward()
    torch.cuda.current_stream().wait_stream(side)
    sp.grad = None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        lv = f(sp, st)
        lv.backward()
    nph, nth = S.make_pair(hw, thw, 270.0, seed=6)
    nth[:, 1] = 2.0
    newp, newt = _dev(nph), _dev(nth)
    with torch.no_grad():
        sp.copy_(newp)
    st.copy_(newt)
    gr.replay()
    torch.cuda.synchronize()
    ep = newp.clone().requires_grad_()
    ev = f(ep, newt)
    ev.backward()
    assert 0 < float(ev) < 2 and abs(float(lv) - float(ev)) <= 1e-6 * float(ev)
    assert torch.equal(sp.grad, ep.grad) and bool(sp.grad[:, 0].any()) and not bool(sp.grad[:, 1].any())


def test_graph_capture_of_the_ssim_loss():
    from climate_learn.metrics.utils import METRICS_REGISTRY
    assert all(METRICS_REGISTRY[n].graph_capturable is True for n in ("ssim_loss", "mse_ssim", "bayesian_tv_ssim"))
    run_child(__file__, "child_graph_capture_of_the_ssim_loss", timeout=300)


# ---- one step of a model --------------------------------------------------------------------------------------------------------------
MODEL_IN = ["land_sea_mask", "orography", "lattitude", "landcover", "2m_temperature", "total_precipitation_24hr"]
MODEL_OUT = ["total_precipitation_24hr", "2m_temperature"]
MODEL_VW = {"2m_temperature": 10.0, "total_precipitation_24hr": 1.0}


def _step(loss_name, weight=None):
    """one SGD step of an interm_8m-sized Res_Slim_ViT on a 16 x 32 -> 64 x 128 grid from a fixed seed: (loss, gradients,
    parameters after the step)"""
    from climate_learn.metrics.utils import METRICS_REGISTRY, MetricsMetaInfo
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.trainer import training_step
    torch.manual_seed(3)
    grid = (16, 32)
    model = Res_Slim_ViT(MODEL_IN, grid, len(MODEL_IN), len(MODEL_OUT), 1, patch_size=2, embed_dim=256, depth=6, decoder_depth=4,
                         num_heads=4, drop_path=0.0, drop_rate=0.0, learn_pos_emb=True).cuda().eval()
    model.data_config(156.0, grid, len(MODEL_IN), len(MODEL_OUT))
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, len(MODEL_IN), *grid, generator=gen).cuda()
    y = torch.randn(2, len(MODEL_OUT), 4 * grid[0], 4 * grid[1], generator=gen).cuda()
    loss_obj = METRICS_REGISTRY[loss_name](aggregate_only=True, metainfo=MetricsMetaInfo(MODEL_IN, MODEL_OUT, None, None, None))
    if weight is not None:
        loss_obj.weight = weight
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    loss = training_step((x, y, MODEL_IN, MODEL_OUT), 0, model, torch.device("cuda:0"), MODEL_VW, loss_obj)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    return float(loss.detach()), grads, {n: p.detach().clone() for n, p in model.named_parameters()}


def test_training_step_with_the_ssim_loss():
    base_loss, base_grads, base_params = _step("bayesian_tv")
    loss, grads, _ = _step("bayesian_tv_ssim")
    print("loss %.7g with the SSIM term, %.7g without" % (loss, base_loss))
    assert np.isfinite(loss) and loss != base_loss
    assert len(grads) > 25 and all(bool(torch.isfinite(g).all()) for g in grads.values()), \
        [n for n, g in grads.items() if not bool(torch.isfinite(g).all())]
    assert any(not torch.equal(grads[n], base_grads[n]) for n in grads)
    zero_loss, _, zero_params = _step("bayesian_tv_ssim", weight=0)
    assert zero_loss == base_loss
    assert all(torch.equal(zero_params[n], base_params[n]) for n in base_params)


# ---- the training driver ---------------------------------------------------------------------------------------------------------------
def test_training_driver_runs_the_ssim_config(tmp_path):
    """configs/interm_8m_ssim.yaml through examples/intermediate_downscaling.py at one Block and batch 2: `trainer.ssim` reaches the
    loss object, and the graphed step (hipgraph: auto at this size) captures the loss with the model"""
    import os
    import re
    import subprocess
    import sys
    import yaml
    from tests._child import free_port
    from tests.conftest import ROOT
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m_ssim.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2, ssim={"weight": 0.5, "data_range": 6.0})
    conf["model"].update(depth=1, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)
    cfg = os.path.join(tmp_path, "c.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "intermediate_downscaling.py"), cfg],
                       cwd=tmp_path, env=dict(os.environ, MASTER_PORT=str(free_port())), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", r.stdout)]
    assert len(losses) == 4 and all(v == v and 0 < v < 1e4 for v in losses)
    # the block with another loss is refused by name before anything is built
    conf["trainer"]["train_loss"] = "bayesian_tv"
    yaml.safe_dump(conf, open(cfg, "w"))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "intermediate_downscaling.py"), cfg],
                       cwd=tmp_path, env=dict(os.environ, MASTER_PORT=str(free_port())), capture_output=True, text=True)
    assert r.returncode != 0 and "trainer.ssim goes with an SSIM loss" in r.stderr and "'bayesian_tv'" in r.stderr
