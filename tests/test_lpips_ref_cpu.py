"""tests/lpips_ref.py against torch autograd or F.* in float64 at one tiny shape each, the float64 chain of the references against
the oracle's `perceptual`, and the fp32 baselines (the same formulas in fp32 on the CPU against float64) at the shapes of
tests/test_lpips_edges_gpu.py: the measurements its tolerances are taken from (profiles/lpips_edge_tests.md records them; run
with -s to print them)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import orbit2_oracle as O
from tests import lpips_ref as L

F64, F32 = torch.float64, torch.float32


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_im2col_and_col2im_equal_unfold_and_its_autograd():
    N, H, W, C = 2, 3, 4, 8
    x, dcol, act, tapg = L.col_inputs(N, H, W, C, False)
    xr = L.nchw(x.double(), N, H, W).requires_grad_()
    unf = F.unfold(xr, 3, padding=1).view(N, C, 9, H * W).permute(0, 3, 2, 1).reshape(N * H * W, 9 * C)     # tap-major, channel-minor
    assert torch.equal(L.im2col(x.double(), N, H, W, C), unf.detach())
    unf.backward(dcol.double())
    g, A = L.col2im(dcol, N, H, W, C)
    assert close(g, L.nhwc(xr.grad)) and bool((A >= g.abs() - 1e-12).all())
    gm, Am = L.col2im(dcol, N, H, W, C, act=act)
    assert close(gm, L.nhwc(xr.grad) * (act > 0))
    gt, At = L.col2im(dcol, N, H, W, C, act=act, tapg=tapg)
    assert close(gt, (L.nhwc(xr.grad) + tapg.double()) * (act > 0)) and bool((At >= gt.abs() - 1e-12).all())
    assert int((act > 0).sum()) and int((act == 0).sum()) and int((act < 0).sum())


@pytest.mark.parametrize("ties", [False, True])
def test_maxpool_equals_max_pool2d_of_relu_and_its_autograd(ties):
    """with forced ties torch's max_pool2d routes the gradient to the first maximum in row-major order too (its CPU kernel scans
    the window with `>`); where the maximum is 0 the ReLU mask leaves nothing to route"""
    N, H, W, C = 2, 4, 6, 8
    x, gy, tapg = L.pool_inputs(N, H, W, C)
    if not ties:
        x = L.rt(torch.randn(N * H * W, C, generator=torch.Generator().manual_seed(2)))
    am, tied = L.first_argmax(F.relu(x), N, H, W, C)
    xr = L.nchw(x.double(), N, H, W).requires_grad_()
    y = F.max_pool2d(F.relu(xr), 2, 2)
    assert torch.equal(L.maxpool_fwd(F.relu(x), N, H, W, C).double(), L.nhwc(y.detach()))
    y.backward(L.nchw(gy.double(), N, H // 2, W // 2))
    dz = L.maxpool_bwd(gy, F.relu(x), N, H, W, C)                     # the kernel sees the post-ReLU activation
    assert torch.equal(dz.double(), L.nhwc(xr.grad))
    dzt = L.maxpool_bwd(gy, F.relu(x), N, H, W, C, tapg=tapg)
    want = ((L.nhwc(xr.grad).float() + tapg) * (x > 0)).to(L.BF)
    assert torch.equal(dzt, want)
    if ties:
        for j in range(3):                                           # positions 0, 1, 2 each win a tie somewhere
            assert bool(((am == j) & tied & (L.maxpool_fwd(F.relu(x), N, H, W, C).reshape(am.shape) > 0)).any()), j


def test_conv1_equals_conv2d_of_the_scaled_image_and_its_autograd():
    N, H, W = 2, 4, 5
    img, pred, target, tie, dz = L.conv1_inputs(N, H, W)
    w1, b1 = L.conv1_weights()
    shift = torch.tensor(O.LPIPS_SHIFT, dtype=F64).view(1, 3, 1, 1)
    scale = torch.tensor(O.LPIPS_SCALE, dtype=F64).view(1, 3, 1, 1)
    w = w1.double().reshape(3, 3, 3, 64).permute(3, 2, 0, 1)
    pr = pred.double().requires_grad_()
    pre = F.conv2d((pr - shift) / scale, w, b1.double(), padding=1)
    out, A = L.conv1_fwd(pred, w1, b1)
    assert close(out, L.nhwc(F.relu(pre).detach())) and bool((A >= out - 1e-12).all())
    l1c, gs = 0.0234375, 0.375
    (gs * l1c * (pr - target.double()).abs().sum() + (pre * L.nchw(dz.double(), N, H, W)).sum()).backward()
    dimg, G = L.conv1_bwd(dz, w1, pred, target, l1c, gs)
    assert close(dimg, pr.grad) and bool((G >= dimg.abs() - 1e-12).all())      # autograd's |x|' is 0 at 0 as well
    assert int(tie.sum()) >= 1 and bool((pred == target)[tie].all()) and not bool((pred == target)[~tie].any())
    lp, _ = L.conv1_bwd(dz, w1, pred, target, 0.0)
    assert torch.equal((dimg - lp)[tie], torch.zeros(int(tie.sum()), dtype=F64))


@pytest.mark.parametrize("C", [64, 512])
def test_tap_head_equals_the_oracle_formula_under_autograd(C):
    B, HW = 2, 5
    f, lin = L.tap_inputs(C, HW, B)
    f0 = f[:B].double().requires_grad_()
    n0 = f0 / (f0.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    n1 = f[B:].double() / (f[B:].double().pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    val = (((n0 - n1) ** 2) * lin.double()).sum(-1).mean(-1)
    ref, A = L.tap_fwd(f, lin, B)
    assert close(ref, val.detach()) and bool((A >= ref - 1e-15).all())
    (val.sum() * HW * L.TAP_COEF * L.GSCALE).backward()
    g, G = L.tap_bwd(f, lin, L.TAP_COEF, B, L.GSCALE)
    live = (f[:B].abs().sum(-1, keepdim=True) > 0).double()               # autograd gives NaN at the all-zero pixel
    assert close(g * live, torch.nan_to_num(f0.grad) * (f[:B] > 0) * live, 1e-12)
    assert bool((g[0, 0] == 0).all()) and bool(torch.isfinite(g).all()) and bool((G >= g.abs() - 1e-15).all())


def chain(pred, target, sd, dtype=F64):
    """`perceptual` and its gradient with respect to pred through the references of this module, stage by stage"""
    B, _, H, W = pred.shape
    N = 2 * B
    w1 = sd["conv0.weight"].permute(2, 3, 1, 0).reshape(27, 64)
    h, _ = L.conv1_fwd(torch.cat([pred, target]), w1, sd["conv0.bias"], dtype)
    acts, ci = [("conv", h, H, W, 64)], 1
    for c in O.VGG16_CFG[1:]:
        _, x, ph, pw, pc = acts[-1][:5]
        if c == "M":
            acts.append(("pool", L.maxpool_fwd(x, N, ph, pw, pc), ph // 2, pw // 2, pc))
            continue
        wg = sd["conv%d.weight" % ci].to(dtype).permute(0, 2, 3, 1).reshape(c, 9 * pc)
        acts.append(("conv", F.relu(L.im2col(x, N, ph, pw, pc) @ wg.t() + sd["conv%d.bias" % ci].to(dtype)), ph, pw, c, wg))
        ci += 1
    conv_seen, taps = -1, {}
    for j, a in enumerate(acts):
        if a[0] == "conv":
            conv_seen += 1
            if conv_seen in O.VGG16_TAPS:
                taps[j] = O.VGG16_TAPS.index(conv_seen)
    val = torch.zeros(B, dtype=dtype)
    for j, k in taps.items():
        val = val + L.tap_fwd(acts[j][1].reshape(N, -1, acts[j][4]), sd["lin%d.weight" % k], B, dtype)[0]
    loss = L.l1_mean(pred, target, dtype) + 0.5 * val.mean()

    def tap(j):
        if j not in taps:
            return None
        _, f, h, w, c = acts[j][:5]
        return L.tap_bwd(f.reshape(N, h * w, c), sd["lin%d.weight" % taps[j]], 0.5 / (B * h * w), B, None, dtype)[0].reshape(-1, c)

    j = len(acts) - 1
    gz = tap(j)
    while j > 0:
        _, _, h, w, _, wg = acts[j]
        dcol = gz @ wg
        cin = wg.shape[1] // 9
        if acts[j - 1][0] == "conv":
            gz = L.col2im(dcol, B, h, w, cin, act=acts[j - 1][1][: B * h * w], tapg=tap(j - 1), dtype=dtype)[0]
            j -= 1
        else:
            gp = L.col2im(dcol, B, h, w, cin, dtype=dtype)[0]
            _, x, sh, sw, sc = acts[j - 2][:5]
            x = x[: B * sh * sw]
            am, _ = L.first_argmax(x, B, sh, sw, sc)                      # maxpool_bwd rounds to bf16: route in `dtype` here
            v = torch.where(am.unsqueeze(3) == torch.arange(4).view(1, 1, 1, 4, 1), gp.reshape(B, sh // 2, sw // 2, 1, sc), torch.zeros((), dtype=dtype))
            gz = (L._unwindows(v, B, sh, sw, sc) + tap(j - 2)) * (x > 0)
            j -= 2
    dimg, _ = L.conv1_bwd(gz, w1, pred, target, 1.0 / pred.numel(), None, dtype)
    return loss, dimg


def test_chain_of_the_references_reproduces_the_oracle_perceptual():
    B, H, W = 1, 16, 16
    sd = {k: v.double() for k, v in O.init_lpips_weights(5).items()}
    g = torch.Generator().manual_seed(9)
    pred = torch.randn(B, 3, H, W, generator=g).double() * 0.6
    target = pred * 0.7 + 0.5 * torch.randn(B, 3, H, W, generator=g).double()
    pr = pred.clone().requires_grad_()
    ref = O.perceptual(pr, target, sd)
    ref.backward()
    ref = ref.detach()
    loss, dimg = chain(pred, target, sd)
    # l1_coef goes through a C float in conv1_bwd: 1/768 rounded to fp32 moves the L1 part by 2^-24 of itself
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref))
    assert float((dimg - pr.grad).abs().max()) <= 2.0 ** -23 / pred.numel() + 1e-12 * float(pr.grad.abs().max())


# ---- fp32 baselines ----------------------------------------------------------------------------------------------------------
def units(base, ref, A):
    """the baseline's largest error in units of 2^-24 A"""
    A = A.double()
    e = (base.double() - ref).abs()
    return float(torch.where(A > 0, e / (L.EPS24 * A).clamp_min(1e-300), torch.zeros_like(e)).max())


def test_col2im_fp32_baselines():
    """nine terms and tapg: at most 10 roundings of A; on the 1/4 grid the fp32 sums are exact"""
    for (H, W), N, C in itertools.product(L.COL_SIZES, L.BATCHES, L.CHANNELS):
        x, dcol, act, tapg = L.col_inputs(N, H, W, C, False)
        for form, kw in (("plain", {}), ("act", dict(act=act)), ("act+tapg", dict(act=act, tapg=tapg))):
            ref, A = L.col2im(dcol, N, H, W, C, **kw)
            u = units(L.col2im(dcol, N, H, W, C, dtype=F32, **kw)[0], ref, A)
            print("col2im %dx%d N=%d C=%d %-8s baseline %.2f x 2^-24 A" % (H, W, N, C, form, u))
            assert u <= 10.0
        x, dcol, act, tapg = L.col_inputs(N, H, W, C, True)
        ref, _ = L.col2im(dcol, N, H, W, C, act=act, tapg=tapg)
        assert torch.equal(L.col2im(dcol, N, H, W, C, act=act, tapg=tapg, dtype=F32)[0].double(), ref)
        assert torch.equal(L.rt(ref.float()).double(), ref)               # and exact in bf16


def test_conv1_fp32_baselines():
    """27 terms + bias, the scaling's subtraction and division: at most 27 + 8 roundings of A; bwd: 576 terms, division, L1 term"""
    w1, b1 = L.conv1_weights()
    for (H, W), N in itertools.product(L.CONV1_SIZES + ((64, 65),), L.BATCHES):
        img, pred, target, tie, dz = L.conv1_inputs(N, H, W)
        ref, A = L.conv1_fwd(img, w1, b1)
        u = units(L.conv1_fwd(img, w1, b1, dtype=F32)[0], ref, A)
        gref, G = L.conv1_bwd(dz, w1, pred, target, 0.0234375, L.GSCALE)
        ug = units(L.conv1_bwd(dz, w1, pred, target, 0.0234375, L.GSCALE, dtype=F32)[0], gref, G)
        print("conv1 %dx%d N=%d fwd baseline %.2f x 2^-24 A, bwd baseline %.2f x 2^-24 G" % (H, W, N, u, ug))
        assert u <= 35.0 and ug <= 584.0


def tap_cases():
    cases = [(C, HW, B) for C in L.TAP_CHANNELS for HW in L.tap_hws(C) for B in L.BATCHES]
    return cases + [(C, HW, 1) for C, HW in L.TAP_SWITCH + L.TAP_TRIP]


def test_tap_fp32_baselines():
    """the per-pixel sum of C terms and the mean over HW pixels; the gradient per element"""
    for C, HW, B in tap_cases():
        f, lin = L.tap_inputs(C, HW, B)
        ref, A = L.tap_fwd(f, lin, B)
        u = units(L.tap_fwd(f, lin, B, dtype=F32)[0], ref, A)
        g, G = L.tap_bwd(f, lin, L.TAP_COEF, B, L.GSCALE)
        ug = units(L.tap_bwd(f, lin, L.TAP_COEF, B, L.GSCALE, dtype=F32)[0], g, G)
        print("tap C=%d HW=%d B=%d val baseline %.2f x 2^-24 A, gradient baseline %.2f x 2^-24 G" % (C, HW, B, u, ug))
        assert u <= 16.0 and ug <= 16.0


def test_l1_mean_fp32_baselines():
    """inputs on the 2^-6 grid: differences exact, and up to 16385 terms the fp32 sum too (below 2^18): the division alone rounds"""
    for n in L.L1_SIZES + (L.TRIP + 1000,):
        a, b = L.l1_inputs(n)
        ref = L.l1_mean(a, b)
        u = float((L.l1_mean(a, b, dtype=F32).double() - ref).abs() / (L.EPS24 * ref).clamp_min(1e-300))
        print("l1_mean n=%d baseline %.2f x 2^-24 |ref|, %d ties" % (n, u, int((a == b).sum())))
        assert u <= (1.0 if n <= 16385 else 16.0)
