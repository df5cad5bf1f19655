"""Missing-data masks on the device (csrc/loss.hip: orbit2_masked_loss_fwd / _bwd / _moments; metrics.functional.masked_mse,
masked_bayesian_tv, rmse / mae / pearson / mean_bias with a mask; the masked_* registry names) against tests/masked_ref.py, the
float64 restatement that tests/test_masked_cpu.py ties to the reference's own numbers.

Tolerances are the project's own for the same arithmetic: nerr < 2e-5 for a loss and its gradient (tests/test_hip_ops.py::
test_loss: fp32 per-lane sums of a few terms, a fixed tree, one division), rtol 2e-5 / atol 2e-6 for the metrics
(tests/test_inference_gpu.py).  Shapes are the smallest that reach each hazard: nothing 16-byte aligned (scalar lanes), everything
aligned (float4 / dword groups), invalid pixels that cut through a 4-wide group and sit on the first and last row and column
(every stencil term meets an invalid and an outside neighbour), planes larger than one sweep of the forward's grid."""
import os

import numpy as np
import pytest
import torch

from tests import masked_ref as ref
from tests._child import run_child
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

LOSS_TOL = 2e-5
RTOL, ATOL = 2e-5, 2e-6
KINDS = {"mse": 0, "bayesian_tv": 1}
UNALIGNED = ((2, 3, 19, 37), (2, 3, 23, 41))          # cropped, odd widths: every row starts off a 16-byte boundary
ALIGNED = ((2, 2, 16, 64), (2, 2, 20, 64))            # the vector path
CW = (1.0, 10.0, 10.0)


def nerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def lat_weights(H):
    w = np.cos(np.deg2rad(np.linspace(-80.0, 80.0, H)))
    return torch.from_numpy(w / w.mean()).float()


def make_case(shape, tshape, seed=0, holes=True):
    """fp32 CPU (pred, target, masks): the target's top-left crop = 0.6 pred + noise, everything outside it is large noise and NaN
    that must never be read.  holes: NaN, +Inf and -Inf in a block that cuts through 4-wide groups, on the first and last row and
    column, and one whole (b, c) plane NaN.  masks: the three forms, each with about a quarter invalid, corners included"""
    B, C, H, W = shape
    Ht, Wt = tshape[2:]
    g = torch.Generator().manual_seed(100 + seed)
    pred = torch.randn(shape, generator=g) * 1.7 + 0.3
    target = 1e3 * torch.randn(tshape, generator=g)
    target[:, :, H:, :] = float("nan")
    target[:, :, :H, :W] = 0.6 * pred + torch.randn(shape, generator=g)
    if holes:
        target[0, 0, 2:7, 2:9] = float("nan")
        target[0, 0, 3, 5] = float("inf")
        target[0, 0, 4, 6] = float("-inf")
        target[B - 1, 0, 0, 1:6] = float("nan")                     # first row
        target[B - 1, 0, H - 1, W - 6:W] = float("inf")             # last row, last column
        target[0, C - 1, 3:H - 2, 0] = float("nan")               # first column
        target[0, C - 1, 1:5, W - 1] = float("-inf")              # last column
        target[B - 1, 1] = float("nan")                           # a plane without data
    masks = {"none": None,
             "hw": torch.rand(H, W, generator=g) > 0.25,                                       # bool, the prediction's size
             "b1": (torch.rand(B, 1, Ht, Wt, generator=g) > 0.25).float() * 2.5,               # float, the target's size
             "bc": (torch.rand(B, C, H, W, generator=g) > 0.25).to(torch.uint8) * 255}          # uint8
    masks["hw"][0, 0] = masks["hw"][H - 1, W - 1] = False
    masks["hw"][0, W - 1] = True
    return pred, target, masks


def poison(pred, target, mask):
    """NaN / Inf in pred at every third invalid pixel: it must not enter any arithmetic"""
    v = ref.validity(pred, target, mask)
    bad = (~v).flatten().nonzero().flatten()[::3]
    out = pred.clone()
    out.view(-1)[bad[0::2]] = float("nan")
    out.view(-1)[bad[1::2]] = float("inf")
    return out, v


def dev(t):
    return None if t is None else t.cuda()


def run_loss(pred, target, kind, lat_w, chan_w, mask):
    """(out, cnt, dpred) of the functional entry on the device; mask in its caller's dtype and shape"""
    from climate_learn import _hip
    from climate_learn.metrics.functional import _mask_operand
    p, t = pred.cuda(), target.cuda()
    m, pitch, sb, sc = _mask_operand(dev(mask), p, t)
    out, cnt = _hip.masked_loss_fwd(p, t, dev(lat_w), dev(chan_w), kind, m, (pitch, sb, sc))
    dp = _hip.masked_loss_bwd(p, t, dev(lat_w), dev(chan_w), torch.ones(1, device="cuda"), cnt, kind, m, (pitch, sb, sc))
    return out, cnt, dp


def check_loss(pred, target, kind, lat_w, chan_w, mask):
    pred, v = poison(pred, target, mask)
    want, wcnt, wgrad = ref.loss(pred, target, kind, lat_w, chan_w, mask, grad=True)
    out, cnt, dp = run_loss(pred, target, kind, lat_w, chan_w, mask)
    print("kind %d out nerr %.3g dpred nerr %.3g valid %d of %d"
          % (kind, nerr(out, want), nerr(dp, wgrad), int(wcnt[-1]), v.numel()))
    assert torch.equal(cnt.cpu(), wcnt)
    assert torch.isfinite(out).all() and torch.isfinite(dp).all()
    assert bool((dp.cpu()[~v] == 0).all())                          # exactly 0.0 where invalid
    assert nerr(out, want) < LOSS_TOL and nerr(dp, wgrad) < LOSS_TOL
    return out, cnt, dp


# ---- 1. loss and gradient against masked_ref ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [UNALIGNED, ALIGNED], ids=["scalar", "vector"])
@pytest.mark.parametrize("form", ["none", "hw", "b1", "bc"])
@pytest.mark.parametrize("lat", [False, True], ids=["nolat", "lat"])
@pytest.mark.parametrize("kind", ["mse", "bayesian_tv"])
def test_loss_and_gradient(kind, lat, form, shapes):
    pred, target, masks = make_case(*shapes)
    H, C = shapes[0][2], shapes[0][1]
    check_loss(pred, target, KINDS[kind], lat_weights(H) if lat else None, torch.tensor(CW[:C]), masks[form])


def test_functional_entries_and_autograd():
    """metrics.functional.masked_mse / masked_bayesian_tv: variable weights by name, aggregate_only, a Normal prediction, and the
    gradient through the aggregate entry scaled by what comes from upstream"""
    from climate_learn.metrics import functional as fn
    pred, target, masks = make_case(*UNALIGNED)
    names, vw = ["a", "b", "c"], {"b": 10.0, "c": 10.0}
    lw = lat_weights(UNALIGNED[1][2]).view(1, 1, -1, 1)             # the target's rows: cropped to the prediction's
    for name, f in (("mse", fn.masked_mse), ("bayesian_tv", fn.masked_bayesian_tv)):
        want, _, wgrad = ref.loss(pred, target, KINDS[name], lw.reshape(-1), torch.tensor(CW), masks["b1"], grad=True)
        p = pred.cuda().requires_grad_()
        out = f(p, target.cuda(), names, vw, False, lw, masks["b1"].cuda())
        (3.0 * out[-1] + 0.0 * out[0]).backward()
        assert nerr(out, want) < LOSS_TOL and nerr(p.grad, 3.0 * wgrad) < LOSS_TOL
        agg = f(torch.distributions.Normal(pred.cuda(), torch.ones_like(pred).cuda()), target.cuda(), names, vw, True, lw,
                masks["b1"].cuda())
        assert agg.dim() == 0 and float(agg) == float(out[-1].detach())


# ---- 2. a plane larger than one sweep of the forward's grid ----------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [((1, 2, 130, 515), (1, 2, 131, 517)), ((1, 2, 130, 516), (1, 2, 131, 516))],
                         ids=["scalar", "vector"])
def test_plane_larger_than_one_sweep(shapes):
    """the forward (and the moments) launch 64 workgroups of 256 threads per (b, c) plane, one item = 4 pixels of a row: one sweep
    is 16384 items, and 130 rows x 129 groups are 16770"""
    assert shapes[0][2] * ((shapes[0][3] + 3) // 4) > 64 * 256
    pred, target, masks = make_case(*shapes)
    check_loss(pred, target, 1, lat_weights(130), torch.tensor(CW[:2]), masks["hw"])
    from climate_learn.metrics import functional as fn          # the moments kernel sweeps its plane the same way
    p, t, m, lw = pred.cuda(), target.cuda(), masks["hw"].cuda(), lat_weights(130)
    for got, want in ((fn.mae(p, t, False, lw, m), ref.mae(pred, target, lw, masks["hw"])),
                      (fn.rmse(p, t, False, lw, m), ref.rmse(pred, target, lw, masks["hw"])),
                      (fn.pearson(p, t, mask=m), ref.pearson(pred, target, masks["hw"])),
                      (fn.mean_bias(p, t, mask=m), ref.mean_bias(pred, target, masks["hw"]))):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=RTOL, atol=ATOL, equal_nan=True)


# ---- 3. the reference's own numbers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "masked.npz")))


def test_rectangle_identity_against_the_reference(gold):
    """valid region = the top-left 11 x 23 rectangle (rows by NaN, columns by the mask): the reference's mse / bayesian_tv on
    the cropped fields and latitude weights, TV terms included"""
    from climate_learn.metrics import functional as fn
    pred, target = torch.from_numpy(gold["pred"]), torch.from_numpy(gold["target"]).clone()
    h0, w0 = (int(v) for v in gold["rect_hw"])
    target[:, :, h0:, :] = float("nan")
    mask = torch.zeros(pred.shape[2:], dtype=torch.bool)
    mask[:, :w0] = True
    names, vw = ["a", "b", "c"], dict(zip("abc", gold["var_weights"].tolist()))
    lw = torch.from_numpy(gold["lat_w"])
    for name, f in (("mse", fn.masked_mse), ("bayesian_tv", fn.masked_bayesian_tv)):
        for lat in (False, True):
            for var in (False, True):
                key = "rect." + name + (".lat" if lat else "") + (".var" if var else "")
                out = f(pred.cuda(), target.cuda(), names if var else None, vw if var else None, False,
                        lw.view(1, 1, -1, 1) if lat else None, mask.cuda())
                print(key, nerr(out, torch.from_numpy(gold[key])))
                assert nerr(out, torch.from_numpy(gold[key])) < LOSS_TOL


def test_masked_rmse_against_the_reference(gold):
    from climate_learn.metrics import functional as fn
    pred, target = torch.from_numpy(gold["pred"]).cuda(), torch.from_numpy(gold["target"]).clone()
    target[torch.from_numpy(gold["nan_where"])] = float("nan")
    target = target.cuda()
    lw = torch.from_numpy(gold["lat_w"]).view(1, 1, -1, 1)
    for tag in ("b1", "bc"):
        mask = torch.from_numpy(gold["mask_" + tag]).cuda()
        np.testing.assert_allclose(fn.rmse(pred, target, mask=mask).cpu().numpy(), gold["rmse." + tag], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(fn.rmse(pred, target, False, lw, mask).cpu().numpy(), gold["lat_rmse." + tag], rtol=RTOL,
                                   atol=ATOL)
        agg = fn.rmse(pred, target, True, lw, mask)
        assert agg.dim() == 0 and abs(float(agg) - gold["lat_rmse." + tag][-1]) <= ATOL + RTOL * gold["lat_rmse." + tag][-1]
    ones = fn.rmse(pred, torch.from_numpy(gold["target"]).cuda(), mask=torch.ones(pred.shape[2:], device="cuda"))
    np.testing.assert_allclose(ones.cpu().numpy(), gold["rmse.ones"], rtol=RTOL, atol=ATOL)


# ---- 4. all valid: the unmasked kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [UNALIGNED, ALIGNED], ids=["scalar", "vector"])
@pytest.mark.parametrize("kind", ["mse", "bayesian_tv"])
def test_all_valid_agrees_with_the_unmasked_loss(kind, shapes):
    from climate_learn import _hip
    pred, target, _ = make_case(*shapes, holes=False)
    target = torch.nan_to_num(target, nan=7.0)                      # the unmasked entry's crop is finite anyway; keep it so
    H, C = shapes[0][2], shapes[0][1]
    lw, cw = lat_weights(H).cuda(), torch.tensor(CW[:C]).cuda()
    k = KINDS[kind]
    plain = _hip.loss_fwd(pred.cuda(), target.cuda(), lw, cw, k)
    dplain = _hip.loss_bwd(pred.cuda(), target.cuda(), lw, cw, torch.ones(1, device="cuda"), k)
    for mask in (None, torch.ones(shapes[0][2:], dtype=torch.bool)):
        out, cnt, dp = run_loss(pred, target, k, lw, cw, mask)
        assert nerr(out, plain) < LOSS_TOL and nerr(dp, dplain) < LOSS_TOL
        n = pred.numel() // C
        assert cnt.tolist() == [n] * C + [n * C]


# ---- 5. degenerate inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "bayesian_tv"])
def test_nothing_valid_and_a_channel_without_data(kind):
    pred, target, masks = make_case(*UNALIGNED)
    k = KINDS[kind]
    for mask, tgt in ((torch.zeros(UNALIGNED[0][2:]), target), (None, torch.full_like(target, float("nan")))):
        out, cnt, dp = run_loss(pred, tgt, k, None, torch.tensor(CW), mask)
        assert torch.equal(out.cpu(), torch.zeros(4)) and torch.equal(dp.cpu(), torch.zeros_like(pred)) and cnt.tolist() == [0] * 4
    base, bcnt, _ = run_loss(pred, target, k, None, torch.tensor(CW), masks["bc"])
    gone = target.clone()
    gone[:, 1] = float("nan")
    out, cnt, dp = run_loss(pred, gone, k, None, torch.tensor(CW), masks["bc"])
    assert float(out[1]) == 0.0 and int(cnt[1]) == 0 and bool((dp[:, 1] == 0).all())
    assert torch.equal(out[[0, 2]], base[[0, 2]]) and torch.equal(cnt[[0, 2]], bcnt[[0, 2]])
    want, _ = ref.loss(pred, gone, k, None, torch.tensor(CW), masks["bc"])
    assert nerr(out, want) < LOSS_TOL


# ---- 6. reproducibility, exact counts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [UNALIGNED, ALIGNED], ids=["scalar", "vector"])
def test_two_calls_give_the_same_bits(shapes):
    pred, target, masks = make_case(*shapes)
    C = shapes[0][1]
    a = run_loss(pred, target, 1, lat_weights(shapes[0][2]), torch.tensor(CW[:C]), masks["b1"])
    b = run_loss(pred, target, 1, lat_weights(shapes[0][2]), torch.tensor(CW[:C]), masks["b1"])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    v = ref.validity(pred, target, masks["b1"])
    assert a[1].tolist() == v.sum((0, 2, 3)).tolist() + [int(v.sum())]


def test_counts_are_exact_beyond_2_24():
    """one channel of 17 x 1024 x 1024 pixels: fp32 stops counting at 2^24 = 16.8 M"""
    from climate_learn import _hip
    g = torch.Generator(device="cuda").manual_seed(3)
    target = torch.randn(17, 1, 1024, 1024, device="cuda", generator=g)
    target[target > 2.0] = float("nan")                             # 2.3 % missing
    pred = torch.zeros_like(target)
    n = int(torch.isfinite(target).sum())
    assert n > 2 ** 24
    out, cnt = _hip.masked_loss_fwd(pred, target, None, None, 0)
    assert cnt.tolist() == [n, n]
    m = _hip.masked_moments(pred, target)
    assert int(m[..., 12].sum()) == n and torch.equal(m[..., 12].long(), torch.isfinite(target).sum((2, 3)))


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------
def child_graph_capture_follows_the_missing_pixels():
    """forward + backward of masked_bayesian_tv captured on static tensors; then the NaN pattern of the static target moves and
    the graph is replayed: loss and dpred equal an eager call on the new data -- the divisor is read on the device"""
    from climate_learn.metrics import functional as fn
    pred, target, masks = make_case(*UNALIGNED)
    names, vw = ["a", "b", "c"], {"b": 10.0, "c": 10.0}
    sp, st, sm = pred.cuda().requires_grad_(), target.cuda().clone(), masks["hw"].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up outside the capture
        fn.masked_bayesian_tv(sp, st, names, vw, True, None, sm).backward()
    torch.cuda.current_stream().wait_stream(side)
    sp.grad = None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        lv = fn.masked_bayesian_tv(sp, st, names, vw, True, None, sm)
        lv.backward()
    moved = target.clone()
    moved[:, :, :19, :37] = torch.nan_to_num(moved[:, :, :19, :37], nan=0.25, posinf=0.5, neginf=-0.5)
    moved[0, 2, 5:16, 10:30] = float("nan")               # far more missing than before: another divisor
    moved[1, 1, ::2, :] = float("inf")
    st.copy_(moved.cuda())
    gr.replay()
    torch.cuda.synchronize()
    ep = pred.cuda().requires_grad_()
    ev = fn.masked_bayesian_tv(ep, moved.cuda(), names, vw, True, None, sm)
    ev.backward()
    assert torch.equal(lv, ev) and torch.equal(sp.grad, ep.grad)
    want, cnt, wgrad = ref.loss(pred, moved, 1, None, torch.tensor(CW), masks["hw"], grad=True)
    old_cnt = ref.loss(pred, target, 1, None, torch.tensor(CW), masks["hw"])[1]
    assert int(cnt[-1]) != int(old_cnt[-1])
    assert nerr(lv.reshape(1), want[-1:]) < LOSS_TOL and nerr(sp.grad, wgrad) < LOSS_TOL


def test_graph_capture_follows_the_missing_pixels():
    run_child(__file__, "child_graph_capture_follows_the_missing_pixels")


# ---- 8. metrics ---------------------------------------------------------------------------------------------------------------------
def _meta(H, W, C):
    from climate_learn.metrics.utils import MetricsMetaInfo
    names = ["v%d" % c for c in range(C)]
    return MetricsMetaInfo(names, names, np.linspace(-80.0, 80.0, H), np.arange(W), None)


@pytest.mark.parametrize("shapes", [UNALIGNED, ALIGNED], ids=["scalar", "vector"])
def test_metrics_against_masked_ref(shapes):
    from climate_learn.metrics import functional as fn
    from climate_learn.metrics.utils import METRICS_REGISTRY
    pred, target, masks = make_case(*shapes)
    (B, C, H, W), (Ht, Wt) = shapes[0], shapes[1][2:]
    lw = lat_weights(Ht)
    p, t = pred.cuda(), target.cuda()
    for form in ("hw", "b1", "bc"):
        mask = masks[form]
        pp, _ = poison(pred, target, mask)
        p = pp.cuda()
        want = {"mae": ref.mae(pp, target, None, mask), "lat_mae": ref.mae(pp, target, lw, mask),
                "pearson": ref.pearson(pp, target, mask), "mean_bias": ref.mean_bias(pp, target, mask),
                "rmse": ref.rmse(pp, target, None, mask), "lat_rmse": ref.rmse(pp, target, lw, mask)}
        got = {"mae": fn.mae(p, t, mask=mask.cuda()), "lat_mae": fn.mae(p, t, False, lw.view(1, 1, -1, 1), mask.cuda()),
               "pearson": fn.pearson(p, t, mask=mask.cuda()), "mean_bias": fn.mean_bias(p, t, mask=mask.cuda()),
               "rmse": fn.rmse(p, t, mask=mask.cuda()), "lat_rmse": fn.rmse(p, t, False, lw.view(1, 1, -1, 1), mask.cuda())}
        for k in want:
            print(form, k, got[k].tolist(), want[k].tolist())
            np.testing.assert_allclose(got[k].cpu().numpy(), want[k].numpy(), rtol=RTOL, atol=ATOL, equal_nan=True)
        assert torch.isnan(want["mae"][1]) == torch.isnan(got["mae"][1].cpu())
    # the channel without data in every batch entry: NaN, and the aggregate is the mean of the others
    gone = target.clone()
    gone[:, 1] = float("nan")
    got = fn.mae(pred.cuda(), gone.cuda(), mask=masks["hw"].cuda()).cpu()
    assert torch.isnan(got[1]) and torch.isfinite(got[-1])
    np.testing.assert_allclose(got.numpy(), ref.mae(pred, gone, None, masks["hw"]).numpy(), rtol=RTOL, atol=ATOL, equal_nan=True)
    # the registry objects, called as evaluate_func calls them: NaN targets alone are missing data; set_mask = mask=
    meta = _meta(Ht, Wt, C)
    for name, key in (("masked_mae", "mae"), ("masked_pearson", "pearson"), ("masked_mean_bias", "mean_bias"),
                      ("masked_rmse", "rmse"), ("masked_lat_rmse", "lat_rmse")):
        obj = METRICS_REGISTRY[name](metainfo=meta)
        f = getattr(ref, key.replace("lat_", ""))
        args = (lw,) if key == "lat_rmse" else ((None,) if key in ("mae", "rmse") else ())
        np.testing.assert_allclose(obj(pred.cuda(), t).cpu().numpy(), f(pred, target, *args, None).numpy(), rtol=RTOL, atol=ATOL,
                                   equal_nan=True)
        with_arg = obj(pred.cuda(), t, mask=masks["b1"].cuda())
        assert obj.set_mask(masks["b1"]) is obj
        assert torch.equal(obj(pred.cuda(), t), with_arg) and obj._static_mask.is_cuda         # uploaded once, kept there
        np.testing.assert_allclose(with_arg.cpu().numpy(), f(pred, target, *args, masks["b1"]).numpy(), rtol=RTOL, atol=ATOL,
                                   equal_nan=True)
        assert torch.equal(obj(pred.cuda(), t, mask=masks["bc"].cuda()),
                           METRICS_REGISTRY[name](metainfo=meta)(pred.cuda(), t, mask=masks["bc"].cuda()))   # mask= overrides
    # ... and the losses, as training_step calls them
    names = meta.out_vars
    vw = dict(zip(names, CW))
    for name, k, lat in (("masked_mse", 0, False), ("masked_lat_mse", 0, True), ("masked_bayesian_tv", 1, False)):
        obj = METRICS_REGISTRY[name](aggregate_only=True, metainfo=meta)
        want = ref.loss(pred, target, k, lw if lat else None, torch.tensor(CW[:C]), None)[0][-1]
        got = obj(pred.cuda(), t, var_names=names, var_weights=vw)
        assert got.dim() == 0 and abs(float(got) - float(want)) < LOSS_TOL * abs(float(want))
        want = ref.loss(pred, target, k, lw if lat else None, torch.tensor(CW[:C]), masks["hw"])[0][-1]
        obj.set_mask(masks["hw"].numpy())
        got = obj(pred.cuda(), t, var_names=names, var_weights=vw)
        assert abs(float(got) - float(want)) < LOSS_TOL * abs(float(want))
    # mask=None on the unmasked functions runs what it always ran: NaN targets give NaN there
    assert torch.isnan(fn.mae(pred.cuda(), t)[-1]) and torch.isnan(fn.rmse(pred.cuda(), t)[-1])


# ---- 9. through the product ---------------------------------------------------------------------------------------------------------
def _write_npz_tree(root, hw, variables, rng, nan_box=None):
    """reference on-disk format: <root>/{train,val,test}/<year>_<shard>.npz var -> [T,1,H,W], lat.npy, lon.npy,
    normalize_{mean,std}.npz, <split>/climatology.npz; nan_box (i0, i1, j0, j1): no data there, in every field"""
    H, W = hw
    for split in ("train", "val", "test"):
        os.makedirs(os.path.join(root, split))
        for sh in range(2):
            d = {v: (np.abs(rng.normal(size=(3, 1, H, W))) * 1e-3 if "precip" in v else rng.normal(size=(3, 1, H, W)) + 270.0)
                 for v in variables}
            if nan_box:
                for a in d.values():
                    a[:, :, nan_box[0]:nan_box[1], nan_box[2]:nan_box[3]] = np.nan
            np.savez(os.path.join(root, split, "2000_%d.npz" % sh), **d)
        np.savez(os.path.join(root, split, "climatology.npz"), **{v: np.zeros((1, H, W)) for v in variables})
    np.save(os.path.join(root, "lat.npy"), np.linspace(-80, 80, H))
    np.save(os.path.join(root, "lon.npy"), np.linspace(0, 350, W))
    np.savez(os.path.join(root, "normalize_mean.npz"), **{v: np.array([0.5e-3 if "precip" in v else 270.0]) for v in variables})
    np.savez(os.path.join(root, "normalize_std.npz"), **{v: np.array([1e-3 if "precip" in v else 1.0]) for v in variables})


def test_training_step_on_a_tree_with_missing_data(tmp_path):
    """a reference-format npz tree whose high-resolution fields are NaN in a box (an ocean): the loader names alone make it
    trainable -- masked_bayesian_tv gives a finite loss and finite parameter gradients where bayesian_tv gives NaN"""
    import climate_learn as cl
    from climate_learn import trainer
    rng = np.random.default_rng(0)
    consts = ["land_sea_mask", "orography", "lattitude", "landcover"]
    outs = ["total_precipitation_24hr", "2m_temperature_min"]
    lo, hi = os.path.join(tmp_path, "lo"), os.path.join(tmp_path, "hi")
    _write_npz_tree(lo, (16, 32), consts + outs, rng)
    _write_npz_tree(hi, (64, 128), outs, rng, nan_box=(9, 31, 50, 101))
    dm = cl.data.IterDataModule("downscaling", lo, hi, consts + outs, outs, batch_size=2, buffer_size=4, subsample=1)
    dm.setup()
    device = torch.device("cuda")
    kwargs = {"default_vars": consts + outs, "embed_dim": 128, "depth": 1, "decoder_depth": 1, "num_heads": 2}
    batch = next(iter(dm.train_dataloader()))
    assert torch.isnan(batch[1][:, :, 9:31, 50:101]).all() and torch.isfinite(batch[1][:, :, :9]).all()
    cl.manual_seed(0)
    torch.manual_seed(0)
    out = cl.load_downscaling_module(device, data_module=dm, architecture="res_slimvit", train_loss="masked_bayesian_tv",
                                     model_kwargs=kwargs, val_loss=["masked_rmse", "masked_pearson", "masked_mean_bias"],
                                     val_target_transform=[None, None, None])
    net, loss_fn, val_losses = out[0].to(device), out[1], out[2]
    assert loss_fn.name == "masked_bayesian_tv" and loss_fn.aggregate_only
    vw = {"total_precipitation_24hr": 1.0, "2m_temperature_min": 10.0}
    loss = trainer.training_step(batch, 0, net, device, vw, loss_fn)
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert torch.isfinite(loss) and float(loss) > 0 and len(grads) > 10 and all(torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    with torch.no_grad():
        scores = trainer.validation_step(next(iter(dm.val_dataloader())), 0, net.eval(), device, val_losses, [None, None, None])
    assert len(scores) == 3 * (len(outs) + 1) and all(torch.isfinite(v) for v in scores.values()), scores
    plain = cl.load_loss(device, net, "bayesian_tv", True, None)
    assert torch.isnan(trainer.training_step(batch, 0, net.train(), device, vw, plain))        # the need, shown
