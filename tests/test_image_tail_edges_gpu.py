"""The image-tail kernels (csrc/image.hip; the losses: csrc/loss.hip) at their partition edges, against the float64 references of tests/rowimage_ref.py.

conv3x3, fp32 against float64 with derived bounds (A = the same sum over absolute values, u = 2^-24):
  mode-0 out, pre (both modes), mode-0 din: per element n u A, n = 9 Cin + 2 (forward), 9 Cout (din)
  dweight / dbias in mode 0:               (256 + nparts + 2) u A, A over all pixels: the 256-term chain of a tile + the sum of parts
  GELU output and the mode-1 gradients:    1e-5 of the maximum (gelu_f's own error is not derived here), and exact placement: out is
                                           pixel_shuffle(gelu(the kernel's own pre)) in float64 to 1e-6 of the maximum
losses: every input a multiple of 2^-6 (differences exact, sgn(0) ties occur, the signs of kernel and reference cannot differ):
  forward: each of the C + 1 outputs within 4 x the fp32 baseline (the oracle's function in fp32 on the CPU), the baseline never
           taken below one fp32 rounding of the output (rowimage_ref.fp32_floor: one sample of a rounding error may be 0)
  gradient: per element 8 u G, G = the sum of the absolute values of the gradient's terms at that element
unpatchify and clamp_channel move or select values: exact.
Each test prints the share of its bound that every output used ("[edge] ...")."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import orbit2_oracle as O
from tests import rowimage_ref as R

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = R.EPS24
TRIP = 8192 * 256                         # items of one trip of this file's grid-stride loops (img_grid)
BIG_H, BIG_W = 1449, 1448                 # 2 098 152 pixels: 1000 items in the second trip


@pytest.fixture(scope="module")
def hip():
    from climate_learn import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip


def check(tag, items):
    """items: (name, got, ref, bound tensor); every element within its bound"""
    worst = {name: R.excess(got, ref, bound) for name, got, ref, bound in items}
    print("[edge] %s " % tag + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert not [n for n, e in worst.items() if not e <= 1.0], (tag, worst)


def of_max(ref, frac):
    return frac * ref.abs().max() * torch.ones_like(ref)


def cuda(t):
    return None if t is None else t.cuda()


def bits(t):
    return t.view(torch.int32)


def conv_items(hip, B, H, W, cfg, tag):
    """forward and backward of one case; returns the check items and the kernel's (din, dw, db)"""
    mode, Cin, Cout, r, ctot, addend = cfg
    x, idx, w, b, add, dout = R.conv_inputs(B, H, W, mode, Cin, Cout, r, ctot, addend)
    xs = x if idx is None else x[:, idx.long()]
    out_r, pre_r, A = R.conv_fwd(xs, w, b, mode, r, add)
    din_r, dw_r, db_r, Adin, Adw, Adb = R.conv_bwd(dout, xs, w, pre_r, mode, r)
    out, pre = hip.conv3x3_fwd(x.cuda(), cuda(idx), w.cuda(), b.cuda(), mode, r, cuda(add))
    din, dw, db = hip.conv3x3_bwd(dout.cuda(), x.cuda(), cuda(idx), w.cuda(), pre, True, mode, r)
    nparts = B * ((H + 15) // 16) * ((W + 15) // 16)
    nf, nw = 9 * Cin + 2, 256 + nparts + 2
    if mode == 0:
        assert pre is None
        items = [("out", out, out_r, nf * U * A), ("din", din, din_r, 9 * Cout * U * Adin),
                 ("dweight", dw, dw_r, nw * U * Adw), ("dbias", db, db_r, nw * U * Adb)]
    else:
        placed = F.pixel_shuffle(F.gelu(pre.cpu().double()), r)
        items = [("pre", pre, pre_r, nf * U * A), ("out", out, out_r, of_max(out_r, 1e-5)), ("placement", out, placed, of_max(placed, 1e-6)),
                 ("din", din, din_r, of_max(din_r, 1e-5)), ("dweight", dw, dw_r, of_max(dw_r, 1e-5)), ("dbias", db, db_r, of_max(db_r, 1e-5))]
    # no data gradient asked for: none returned, the same weight gradients; and the same bits from call to call (no atomics)
    none, dw2, db2 = hip.conv3x3_bwd(dout.cuda(), x.cuda(), cuda(idx), w.cuda(), pre, False, mode, r)
    assert none is None and torch.equal(bits(dw), bits(dw2)) and torch.equal(bits(db), bits(db2)), tag
    return items


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cfg", R.CONV_CHANNELS, ids=lambda c: "m%d_%dto%d_r%d_%s_%s" % c)
def test_conv3x3_sizes_and_channels(hip, cfg, B):
    """images smaller than 3 pixels on a side, one exact 16 x 16 tile, one pixel short of and past a tile in each direction, a
    second and a third tile row; Cin 1 and 8 (the maximum); a Cout that is neither <= 16 nor a multiple of 16 (17, 18, 36);
    r 1, 2, 3; chan_idx NULL and a selection out of 11 channels; the addend with the pitch of out and with a larger one"""
    for H, W in R.CONV_SIZES:
        tag = "conv %dx%d B=%d" % (H, W, B)
        check(tag, conv_items(hip, B, H, W, cfg, tag))


@pytest.mark.parametrize("B,H,W,nparts", [(8, 32, 64, 64), (13, 16, 65, 65)])
def test_conv3x3_sum_of_parts_form_switch(hip, B, H, W, nparts):
    """64 parts: the last case of the one-thread-per-element form; 65: the first of the 32-lane form"""
    assert B * ((H + 15) // 16) * ((W + 15) // 16) == nparts
    tag = "conv parts=%d" % nparts
    check(tag, conv_items(hip, B, H, W, (0, 2, 3, 1, None, None), tag))


@pytest.mark.parametrize("mode,Cin,Cout,r", [(0, 8, 17, 1), (1, 2, 18, 3)])
def test_conv3x3_bwd_adds_to_what_dweight_and_dbias_hold(hip, mode, Cin, Cout, r):
    B, H, W = 3, 17, 33
    x, idx, w, b, add, dout = R.conv_inputs(B, H, W, mode, Cin, Cout, r, None, None)
    _, pre_r, _ = R.conv_fwd(x, w, b, mode, r)
    _, dw_r, db_r, _, Adw, Adb = R.conv_bwd(dout, x, w, pre_r, mode, r)
    g = torch.Generator().manual_seed(5)
    dw0, db0 = torch.randn(dw_r.shape, generator=g) * 10, torch.randn(db_r.shape, generator=g) * 10
    _, pre = hip.conv3x3_fwd(x.cuda(), None, w.cuda(), b.cuda(), mode, r, None)
    lib = hip.lib()
    xd, wd, dd, dw, db = x.cuda(), w.cuda(), dout.cuda(), dw0.cuda(), db0.cuda()
    ws = torch.empty(lib.orbit2_conv3x3_bwd_ws_floats(B, Cin, Cout, H, W), device="cuda")
    rc = lib.orbit2_conv3x3_bwd(dd.data_ptr(), xd.data_ptr(), None, Cin, wd.data_ptr(), None if pre is None else pre.data_ptr(), None,
                                dw.data_ptr(), db.data_ptr(), B, Cin, Cout, H, W, mode, r, ws.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    n = 256 + B * 2 * 3 + 2
    if mode == 0:
        bw, bb = n * U * (Adw + dw0.double().abs()), n * U * (Adb + db0.double().abs())
    else:
        bw, bb = of_max(dw_r, 1e-5) + U * dw0.double().abs(), of_max(db_r, 1e-5) + U * db0.double().abs()
    check("conv += mode %d" % mode, [("dweight", dw, dw0.double() + dw_r, bw), ("dbias", db, db0.double() + db_r, bb)])


# ---- the second trip of the grid-stride loops ----------------------------------------------------------------------------------
def check_with_tail(tag, items):
    """the bound on everything, and on the elements past the first trip on their own"""
    check(tag, items)
    check(tag + " past %d" % TRIP, [(n, g.reshape(-1)[TRIP:], r.reshape(-1)[TRIP:], b.reshape(-1)[TRIP:]) for n, g, r, b in items])


def test_second_trip_conv3x3(hip):
    B, H, W = 1, BIG_H, BIG_W
    assert B * H * W > TRIP
    cfg = (0, 1, 1, 1, None, None)
    x, idx, w, b, add, dout = R.conv_inputs(B, H, W, *cfg)
    out_r, pre_r, A = R.conv_fwd(x, w, b)
    din_r, dw_r, db_r, Adin, Adw, Adb = R.conv_bwd(dout, x, w, pre_r)
    out, _ = hip.conv3x3_fwd(x.cuda(), None, w.cuda(), b.cuda(), 0, 1, None)
    din, dw, db = hip.conv3x3_bwd(dout.cuda(), x.cuda(), None, w.cuda(), None, True, 0, 1)
    check_with_tail("trip2 conv", [("out", out, out_r, 11 * U * A), ("din", din, din_r, 9 * U * Adin)])
    nparts = ((H + 15) // 16) * ((W + 15) // 16)
    check("trip2 conv weights", [("dweight", dw, dw_r, (256 + nparts + 2) * U * Adw), ("dbias", db, db_r, (256 + nparts + 2) * U * Adb)])


def test_second_trip_unpatchify(hip):
    B, C, h, w, p, s = 1, 1, BIG_H, BIG_W, 1, 1
    g = torch.Generator().manual_seed(21)
    t = R.rt(torch.randn(B, h * w, C, generator=g))
    ref = O.unpatchify(t, (h, w), p, s, C)
    img = hip.unpatchify_fwd(t.to(BF).cuda(), B, C, h, w, p, s).cpu()
    assert torch.equal(img, ref) and torch.equal(img.reshape(-1)[TRIP:], ref.reshape(-1)[TRIP:])
    dimg = torch.randn(ref.shape, generator=g)
    dt = hip.unpatchify_bwd(dimg.cuda(), B, C, h, w, p, s).cpu()
    want = dimg.reshape(B, h * w, C).to(BF)                      # p = s = 1, C = 1: the permutation is the identity
    assert torch.equal(dt, want) and torch.equal(dt.reshape(-1)[TRIP:], want.reshape(-1)[TRIP:])


def test_second_trip_clamp_channel(hip):
    g = torch.Generator().manual_seed(22)
    x = torch.randn(1, 2, BIG_H, BIG_W, generator=g)
    y = hip.clamp_channel_(x.clone().cuda(), 1).cpu()
    assert torch.equal(bits(y[:, 0]), bits(x[:, 0]))
    want = x[:, 1].clamp(min=0)
    assert torch.equal(y[:, 1], want) and torch.equal(y[:, 1].reshape(-1)[TRIP:], want.reshape(-1)[TRIP:])
    gr = torch.randn(x.shape, generator=g)
    d = hip.clamp_channel_bwd_(y.cuda(), gr.clone().cuda(), 1).cpu()
    wantd = torch.where(y[:, 1] > 0, gr[:, 1], torch.zeros(()))
    assert torch.equal(bits(d[:, 0]), bits(gr[:, 0]))
    assert torch.equal(d[:, 1], wantd) and torch.equal(d[:, 1].reshape(-1)[TRIP:], wantd.reshape(-1)[TRIP:])


def test_second_trip_loss_bwd(hip):
    pred, tgt = R.loss_inputs(BIG_H, BIG_W, False, B=1, C=1)
    latw = R.loss_latw(BIG_H, BIG_H)
    gs = torch.tensor([R.LOSS_GSCALE])
    grad, G, _ = R.loss_bwd(pred, tgt, latw, None, float(gs), 1)
    dp = hip.loss_bwd(pred.cuda(), tgt.cuda(), latw.cuda(), None, gs.cuda(), 1)
    check_with_tail("trip2 loss_bwd", [("dpred", dp, grad, 8 * U * G)])


# ---- unpatchify ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("p", [1, 2, 4])
def test_unpatchify_patch_and_scale(hip, p, s):
    B = 2
    g = torch.Generator().manual_seed(10 * p + s)
    for C, (h, w) in itertools.product((1, 3), ((4, 8), (8, 12))):
        t32 = torch.randn(B, h * w // (p * p), C * (s * p) ** 2, generator=g)
        t = R.rt(t32)
        ref = O.unpatchify(t, (h, w), p, s, C)
        assert torch.equal(hip.unpatchify_fwd(t.to(BF).cuda(), B, C, h, w, p, s).cpu(), ref), (C, h, w)
        assert torch.equal(hip.unpatchify_fwd_f32(t32.cuda(), B, C, h, w, p, s).cpu(), O.unpatchify(t32, (h, w), p, s, C)), (C, h, w)
        dimg = torch.randn(ref.shape, generator=g)
        tr = t32.clone().requires_grad_()
        O.unpatchify(tr, (h, w), p, s, C).backward(dimg)
        assert torch.equal(hip.unpatchify_bwd(dimg.cuda(), B, C, h, w, p, s).cpu(), tr.grad.to(BF)), (C, h, w)


# ---- clamp_channel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,chan", [(3, 0), (3, 2), (1, 0)])
def test_clamp_channel_first_and_last(hip, C, chan):
    g = torch.Generator().manual_seed(8 + chan)
    x = torch.randn(2, C, 7, 9, generator=g)
    x[:, :, 0, :4] = torch.tensor([0.0, -0.0, 0.0, -0.0])               # exact zero and minus zero
    y = hip.clamp_channel_(x.clone().cuda(), chan).cpu()
    others = [c for c in range(C) if c != chan]
    assert torch.equal(bits(y[:, others]), bits(x[:, others]))            # -0.0 elsewhere keeps its sign bit
    assert torch.equal(y[:, chan], x[:, chan].clamp(min=0)) and not bool((y[:, chan] < 0).any())
    gr = torch.randn(x.shape, generator=g)
    d = hip.clamp_channel_bwd_(y.cuda(), gr.clone().cuda(), chan).cpu()
    assert torch.equal(bits(d[:, others]), bits(gr[:, others]))
    keep = y[:, chan] > 0
    assert torch.equal(d[:, chan][keep], gr[:, chan][keep]) and bool((d[:, chan][~keep] == 0).all())
    assert int((~keep).sum()) >= 6 and int(keep.sum()) >= 6


# ---- losses --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", R.LOSS_SHAPES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_loss_edges(hip, kind, H, W):
    """H = 1, W = 1 (no neighbour in one direction), 24 x 40, and 129 x 128 = 16512 pixels: the second trip of loss_fwd_kernel's
    64 x 256 loop; with and without latitude and channel weights, the target as large as pred and larger, gscale = 0.37"""
    gs = torch.tensor([R.LOSS_GSCALE])
    for larger, lat, chan in itertools.product((False, True), repeat=3):
        pred, tgt = R.loss_inputs(H, W, larger)
        latw = R.loss_latw(H, tgt.shape[2]) if lat else None
        chanw = R.LOSS_CHANW if chan else None
        cwd = torch.tensor(chanw).cuda() if chan else None
        ref = R.loss_fwd(pred, tgt, latw, chanw, kind)
        base = R.loss_fwd(pred, tgt, latw, chanw, kind, dtype=F32)
        b = R.fp32_floor((base.double() - ref).abs(), ref.abs())
        out = hip.loss_fwd(pred.cuda(), tgt.cuda(), cuda(latw), cwd, kind)
        grad, G, ties = R.loss_bwd(pred, tgt, latw, chanw, float(gs), kind)
        if kind and H >= 9 and W >= 9:
            assert ties >= 20
        dp = hip.loss_bwd(pred.cuda(), tgt.cuda(), cuda(latw), cwd, gs.cuda(), kind)
        check("loss kind %d %dx%d larger=%d lat=%d chan=%d ties=%d" % (kind, H, W, larger, lat, chan, ties),
              [("out", out, ref, 4.0 * b), ("dpred", dp, grad, 8 * U * G)])
