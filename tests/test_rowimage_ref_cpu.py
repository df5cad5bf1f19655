"""tests/rowimage_ref.py against torch autograd at one tiny shape each, and the fp32 baselines (the same formulas in fp32 on the
CPU against float64) at the shapes of the GPU edge tests: the measurements their fp32 tolerances are taken from
(profiles/row_image_edge_tests.md records them; run with -s to print them)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import orbit2_oracle as O
from tests import rowimage_ref as R

F64, F32 = torch.float64, torch.float32


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_layernorm_reference_equals_autograd():
    x, gam, bet, dy, dres = R.ln_inputs(24, 5)
    xr, gr, br = (t.double().requires_grad_() for t in (x, gam, bet))
    yr = F.layer_norm(xr, (24,), gr, br, 1e-5)
    yr.backward(dy.double())
    y, mean, rstd = R.ln_fwd(x, gam, bet)
    assert close(y, yr.detach()) and close(mean, x.double().mean(-1))
    assert close(rstd, 1.0 / torch.sqrt(x.double().var(-1, unbiased=False) + 1e-5))
    dx, dg, db = R.ln_bwd(dy, x, gam, dres)
    assert close(dx, xr.grad + dres.double()) and close(dg, gr.grad) and close(db, br.grad)
    dx0, _, _ = R.ln_bwd(dy, x, gam, None)
    assert close(dx0, xr.grad)
    sinks = (torch.arange(24.0), -torch.arange(24.0))
    _, dg1, db1 = R.ln_bwd(dy, x, gam, None, sinks, 1.0)
    assert close(dg1, gr.grad + sinks[0].double()) and close(db1, br.grad + sinks[1].double())
    _, dg2, db2 = R.ln_bwd(dy, x, gam, None, sinks, 0.0)
    assert close(dg2, gr.grad) and close(db2, br.grad)


@pytest.mark.parametrize("mode,r,Cout", [(0, 1, 3), (1, 2, 8)])
def test_conv_reference_equals_autograd(mode, r, Cout):
    x, idx, w, b, add, dout = R.conv_inputs(2, 5, 6, mode, 3, Cout, r, 5, "larger" if mode == 0 else None)
    xs = x[:, idx.long()].double().requires_grad_()
    wr, br = w.double().requires_grad_(), b.double().requires_grad_()
    pre = F.conv2d(xs, wr, br, padding=1)
    yr = pre + add.double()[:, :, :5, :6] if mode == 0 else F.pixel_shuffle(F.gelu(pre), r)
    yr.backward(dout.double())
    out, pre_ref, A = R.conv_fwd(xs.detach(), w, b, mode, r, add)
    assert close(out, yr.detach()) and close(pre_ref, pre.detach())
    assert bool((A >= pre_ref.abs() - 1e-12).all())                       # the companion dominates every element
    din, dw, db, Adin, Adw, Adb = R.conv_bwd(dout, xs.detach(), w, pre_ref, mode, r)
    assert close(din, xs.grad) and close(dw, wr.grad) and close(db, br.grad)
    assert bool((Adin >= din.abs() - 1e-12).all()) and bool((Adw >= dw.abs() - 1e-12).all()) and bool((Adb >= db.abs() - 1e-12).all())


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("lat,chan", [(False, False), (True, True)])
def test_loss_reference_equals_autograd(kind, lat, chan):
    pred, tgt = R.loss_inputs(11, 10, True)
    latw = R.loss_latw(11, tgt.shape[2]) if lat else None
    chanw = R.LOSS_CHANW if chan else None
    pr = pred.double().requires_grad_()
    out = R.loss_fwd(pr, tgt, latw, chanw, kind)
    (out[-1] * R.LOSS_GSCALE).backward()
    grad, G, ties = R.loss_bwd(pred, tgt, latw, chanw, R.LOSS_GSCALE, kind)
    assert close(grad, pr.grad, 1e-13)
    assert bool((G >= grad.abs() - 1e-15).all())
    if kind:
        assert ties >= 20
    if kind == 2 and not lat:           # the composition equals the oracle's image_gradient
        names = ["c0", "c1"] if chan else None
        vw = dict(zip(names, R.LOSS_CHANW)) if chan else None
        t = O.crop_target(tgt.double(), pred).contiguous()
        assert close(out[-1].detach(), O.image_gradient(pred.double(), t, names, vw), 1e-13)


def test_adamw_reference_equals_torch_optimizer():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(37, generator=g).double()
    grads = [torch.randn(37, generator=g).double() for _ in range(3)]
    q = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([q], lr=R.ADAMW["lr"], betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-5)
    p, m, v = p0.clone(), torch.zeros(37, dtype=F64), torch.zeros(37, dtype=F64)
    po, mo, vo = p0.clone(), torch.zeros(37, dtype=F64), torch.zeros(37, dtype=F64)
    pk, mk, vk = p, m, v
    for step, gr in enumerate(grads, 1):
        q.grad = gr.clone()
        opt.step()
        p, m, v = R.adamw_step(p, gr * 4.0, m, v, step, grad_scale=0.25, as_kernel_args=False)
        pk, mk, vk = R.adamw_step(pk, gr * 4.0, mk, vk, step, grad_scale=0.25)
        O.adamw_step(po, gr, mo, vo, step, **R.ADAMW)
    assert close(p, q.detach(), 1e-13)
    assert close(p, po, 1e-13) and close(m, mo, 1e-13) and close(v, vo, 1e-13)
    # the scalars as the C entry receives them (fp32) move the step by the roundings of the scalars, no more
    assert close(pk, p, 1e-6) and close(vk, v, 2e-6) and not torch.equal(vk, v)


# ---- fp32 baselines ----------------------------------------------------------------------------------------------------------
def ln_baselines(D, rows):
    """largest fp32-baseline error of every LayerNorm output at one shape, relative to 2^-24 of the output's magnitude"""
    x, gam, bet, dy, dres = R.ln_inputs(D, rows)
    ref = R.ln_fwd(x, gam, bet) + R.ln_bwd(dy, x, gam, dres)
    base = R.ln_fwd(x, gam, bet, dtype=F32) + R.ln_bwd(dy, x, gam, dres, dtype=F32)
    return {n: (float(R.base_err(b, r)), float(r.abs().max())) for n, b, r in zip(("y", "mean", "rstd", "dx", "dgamma", "dbeta"), base, ref)}


@pytest.mark.parametrize("D,rows", [(D, 130) for D in R.LN_WIDTHS] + list(R.LN_SWITCH))
def test_layernorm_fp32_baselines(D, rows):
    """an fp32 evaluation of a row of D terms and a column of `rows` terms stays within (terms + 8) roundings of the magnitude:
    the baselines are measures of fp32 arithmetic, not of a mistake in the formulas"""
    for name, (b, scale) in ln_baselines(D, rows).items():
        terms = rows if name in ("dgamma", "dbeta") else D
        print("ln D=%d rows=%d %-6s baseline %.3e = %.2f x 2^-24 max|ref|" % (D, rows, name, b, b / (R.EPS24 * scale)))
        assert b <= (terms + 8) * R.EPS24 * scale, name


@pytest.mark.parametrize("cfg", R.CONV_CHANNELS, ids=lambda c: "m%d_%dto%d_r%d" % c[:4])
def test_conv_fp32_baselines_within_the_dot_product_bound(cfg):
    """the fp32 baseline of every conv output obeys the bound the GPU test asks of the kernel (n 2^-24 A per element; GELU
    outputs: 1e-5 of the maximum), at every size and batch of that test"""
    mode, Cin, Cout, r, ctot, addend = cfg
    worst = {}
    for (H, W), B in itertools.product(R.CONV_SIZES, (1, 3)):
        x, idx, w, b, add, dout = R.conv_inputs(B, H, W, mode, Cin, Cout, r, ctot, addend)
        xs = x if idx is None else x[:, idx.long()]
        out, pre, A = R.conv_fwd(xs, w, b, mode, r, add)
        din, dw, db, Adin, Adw, Adb = R.conv_bwd(dout, xs, w, pre, mode, r)
        o32, p32, _ = R.conv_fwd(xs, w, b, mode, r, add, dtype=F32)
        g32 = R.conv_bwd(dout, xs, w, p32, mode, r, dtype=F32)
        nparts = B * ((H + 15) // 16) * ((W + 15) // 16)
        checks = [("pre", p32, pre, (9 * Cin + 2) * R.EPS24 * A)]
        if mode == 0:
            checks += [("out", o32, out, (9 * Cin + 2) * R.EPS24 * A), ("din", g32[0], din, 9 * Cout * R.EPS24 * Adin),
                       ("dweight", g32[1], dw, (256 + nparts + 2) * R.EPS24 * Adw), ("dbias", g32[2], db, (256 + nparts + 2) * R.EPS24 * Adb)]
        else:
            checks += [(n, a, b_, 1e-5 * b_.abs().max() * torch.ones_like(b_)) for n, a, b_ in
                       (("out", o32, out), ("din", g32[0], din), ("dweight", g32[1], dw), ("dbias", g32[2], db))]
        for name, a, ref, bound in checks:
            worst[name] = max(worst.get(name, 0.0), R.excess(a, ref, bound))
    for name, e in worst.items():
        print("conv %s %-7s fp32 baseline uses %.3f of the bound" % (str(cfg[:4]), name, e))
        assert e <= 1.0, name


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_loss_fp32_baselines(kind):
    """the fp32 baseline of each of the C + 1 outputs, in units of one rounding of the output: a few roundings at most"""
    for (H, W), larger, lat, chan in itertools.product(R.LOSS_SHAPES, (False, True), (False, True), (False, True)):
        pred, tgt = R.loss_inputs(H, W, larger)
        latw = R.loss_latw(H, tgt.shape[2]) if lat else None
        chanw = R.LOSS_CHANW if chan else None
        ref = R.loss_fwd(pred, tgt, latw, chanw, kind)
        base = R.loss_fwd(pred, tgt, latw, chanw, kind, dtype=F32)
        units = ((base.double() - ref).abs() / (R.EPS24 * ref.abs()).clamp_min(1e-300)).max()
        print("loss kind %d %dx%d larger=%d lat=%d chan=%d baseline %.2f x 2^-24 |ref|" % (kind, H, W, larger, lat, chan, units))
        assert float(units) <= 16.0
