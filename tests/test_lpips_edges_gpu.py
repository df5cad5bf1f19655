"""The nine kernels of csrc/lpips.hip (the `perceptual` losses), each alone and at its edges, against the float64 references of
tests/lpips_ref.py.

Bounds (u = 2^-24, b = the fp32 baseline: the reference's formulas in fp32 on the CPU against float64, its largest error over the
tensor in units of the companion A / G, per element times A / G, never below u A: lpips_ref.baseline):
  im2col, maxpool fwd, maxpool bwd:     move or select values: torch.equal.  maxpool bwd with tapg too: the reference forms g + tapg
                                        in fp32 and rounds once to bf16, as the kernel does
  col2im, conv1 fwd, GEMM stages, tap bwd (bf16 outputs of fp32 arithmetic): per element 2^-8 |ref| + 4 b
  conv1 bwd dimg, tap fwd val, l1 mean (fp32 outputs): 4 b; a prefilled destination counts as one more term of A
Exact grids: pred / target / l1 inputs are multiples of 2^-6 (pred == target ties occur and every difference is exact); col2im
also runs on dcol and tapg that are multiples of 1/4 in [-1, 1], where every sum is exact in bf16 and the output is compared bit
for bit; the 2 M-pixel conv1 bwd case has dz in {-2..2} and w1 on multiples of 1/16, so the 576-term sums are exact in fp32.
Each test prints the share of its bound that every output used ("[edge] ...")."""
import itertools

import pytest
import torch

from oracle import orbit2_oracle as O
from tests import lpips_ref as L

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
TRIP = L.TRIP
SENTINEL = 7.0


@pytest.fixture(scope="module")
def hip():
    from climate_learn import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip


def check(tag, items):
    """items: (name, got, ref, bound tensor); every element within its bound"""
    worst = {name: L.excess(got.float() if torch.is_tensor(got) and got.dtype == BF else got, ref, bound) for name, got, ref, bound in items}
    print("[edge] %s " % tag + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert not [n for n, e in worst.items() if not e <= 1.0], (tag, worst)


def check_with_tail(tag, items, start):
    """the bound on everything, and on the elements past the first trip (flat index >= start) on their own"""
    check(tag, items)
    check(tag + " past the first trip", [(n, g.reshape(-1)[start:], r.reshape(-1)[start:], b.reshape(-1)[start:]) for n, g, r, b in items])


def dev(t):
    """a bf16-exact fp32 CPU tensor as the bf16 device tensor a kernel reads"""
    return None if t is None else t.to(BF).cuda()


def bits(t):
    return t.view(torch.int32)


def cuda_gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def levels(shape, lo, hi, step, seed):
    """bf16 device tensor of multiples of `step` in [lo*step, hi*step): drawn on the device, the big cases only (the reference is
    computed from the copy read back, so nothing depends on the device's generator)"""
    return (torch.randint(lo, hi, shape, device="cuda", dtype=torch.int8, generator=cuda_gen(seed)).to(F32) * step).to(BF)


# ---- im2col / col2im -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", L.CHANNELS)
@pytest.mark.parametrize("N", L.BATCHES)
def test_im2col_small_images_and_seam(hip, N, C):
    """images under 3 pixels wide or high (every tap but the centre leaves the image somewhere), one lane group per pixel (C = 8)
    to 64; N = 3 with W = 1 or 2: a tap that leaks across a row end or an image seam copies a neighbour's nonzero value"""
    for H, W in L.COL_SIZES:
        x = L.col_inputs(N, H, W, C, False)[0]
        assert bool((x != 0).all())
        col = hip.im2col3x3(dev(x), N, H, W, C)
        assert torch.equal(col.float().cpu(), L.im2col(x, N, H, W, C)), (H, W)


@pytest.mark.parametrize("C", L.CHANNELS)
@pytest.mark.parametrize("N", L.BATCHES)
def test_col2im_three_forms(hip, N, C):
    """plain, act, act + tapg.  On the 1/4 grid the output is compared bit for bit; with bf16 normals: 2^-8 |ref| + 4 b"""
    for H, W in L.COL_SIZES:
        _, dcol, act, tapg = L.col_inputs(N, H, W, C, True)
        items = []
        for form, kw in (("plain", {}), ("act", dict(act=act)), ("act+tapg", dict(act=act, tapg=tapg))):
            ref, _ = L.col2im(dcol, N, H, W, C, **kw)
            out = hip.col2im3x3(dev(dcol), N, H, W, C, **{k: dev(v) for k, v in kw.items()})
            assert torch.equal(out.float().cpu().double(), ref), (form, H, W)
        _, dcol, act, tapg = L.col_inputs(N, H, W, C, False)
        for form, kw in (("plain", {}), ("act", dict(act=act)), ("act+tapg", dict(act=act, tapg=tapg))):
            ref, A = L.col2im(dcol, N, H, W, C, **kw)
            base, _ = L.col2im(dcol, N, H, W, C, dtype=F32, **kw)
            out = hip.col2im3x3(dev(dcol), N, H, W, C, **{k: dev(v) for k, v in kw.items()})
            items.append((form, out, ref, L.bound_bf16(base, ref, A)))
        check("col2im %dx%d N=%d C=%d" % (H, W, N, C), items)


# ---- 2x2 max-pool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", L.CHANNELS)
@pytest.mark.parametrize("N", L.BATCHES)
def test_maxpool_ties_zeros_and_tapg(hip, N, C):
    """x on five levels with zeros and negative values: most windows hold their maximum more than once, and the gradient goes to
    the first such position in row-major order only; all three outputs bit for bit"""
    for H, W in L.POOL_SIZES:
        x, gy, tapg = L.pool_inputs(N, H, W, C)
        assert bool((x < 0).any()) and bool((x == 0).any())
        y = hip.maxpool2_fwd(dev(x), N, H, W, C)
        assert torch.equal(y.float().cpu(), L.maxpool_fwd(x, N, H, W, C)), (H, W)
        dz = hip.maxpool2_bwd(dev(gy), dev(x), N, H, W, C)
        assert torch.equal(dz.cpu(), L.maxpool_bwd(gy, x, N, H, W, C)), (H, W)
        dzt = hip.maxpool2_bwd(dev(gy), dev(x), N, H, W, C, tapg=dev(tapg))
        want = L.maxpool_bwd(gy, x, N, H, W, C, tapg=tapg)
        assert torch.equal(dzt.cpu(), want), (H, W)
        assert not torch.equal(want, L.maxpool_bwd(gy, x, N, H, W, C))
    am, tied = L.first_argmax(x, N, H, W, C)                     # the 4 x 8 case: every position wins, 0 to 2 win ties
    pos = L.maxpool_fwd(x, N, H, W, C).reshape(am.shape) > 0
    assert all(bool(((am == j) & pos).any()) for j in range(4)) and all(bool(((am == j) & tied & pos).any()) for j in range(3))


# ---- first convolution ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", L.BATCHES)
def test_conv1_fwd_sizes(hip, N):
    """nonzero bias, channel 2 of the image offset by 3: a swapped shift, scale or channel moves every output"""
    w1, b1 = L.conv1_weights()
    for H, W in L.CONV1_SIZES:
        img = L.conv1_inputs(N, H, W)[0]
        ref, A = L.conv1_fwd(img, w1, b1)
        base, _ = L.conv1_fwd(img, w1, b1, dtype=F32)
        out = hip.lpips_conv1_fwd(img.cuda(), w1.cuda(), b1.cuda())
        assert int((ref > 0).sum()) and (H * W < 4 or int((ref == 0).sum()))
        check("conv1 fwd %dx%d N=%d" % (H, W, N), [("out", out, ref, L.bound_bf16(base, ref, A))])


@pytest.mark.parametrize("N", L.BATCHES)
def test_conv1_bwd_sizes_ties_and_gscale(hip, N):
    """pred == target wherever the flat index is a multiple of 3: the L1 term is 0 there, so there the result is the LPIPS part
    alone and the same bits with and without gscale; gscale as a device scalar equals gscale = None with l1_coef scaled (the
    product 3/128 x 3/8 is exact in fp32: the same bits); each channel on its own"""
    w1, _ = L.conv1_weights()
    l1c, gs = 0.0234375, L.GSCALE
    for H, W in L.CONV1_SIZES:
        img, pred, target, tie, dz = L.conv1_inputs(N, H, W)
        args = (dev(dz), w1.cuda(), pred.cuda(), target.cuda())
        plain = hip.lpips_conv1_bwd(*args, l1c)
        scaled = hip.lpips_conv1_bwd(*args, l1c, gscale=torch.tensor([gs]).cuda())
        folded = hip.lpips_conv1_bwd(*args, l1c * gs)
        assert torch.equal(bits(scaled), bits(folded))
        assert torch.equal(bits(scaled.cpu())[tie], bits(plain.cpu())[tie]) and not torch.equal(scaled, plain)
        items = []
        for name, got, g in (("none", plain, None), ("gscale", scaled, gs)):
            ref, G = L.conv1_bwd(dz, w1, pred, target, l1c, g)
            base, _ = L.conv1_bwd(dz, w1, pred, target, l1c, g, dtype=F32)
            bound = L.bound_f32(base, ref, G)
            items += [("%s ch%d" % (name, c), got[:, c], ref[:, c], bound[:, c]) for c in range(3)]
        lp, G0 = L.conv1_bwd(dz, w1, pred, target, 0.0)
        b0 = L.bound_f32(L.conv1_bwd(dz, w1, pred, target, 0.0, dtype=F32)[0], lp, G0)
        items.append(("lpips part at ties", plain.cpu()[tie], lp[tie], b0[tie]))
        check("conv1 bwd %dx%d N=%d" % (H, W, N), items)


# ---- LPIPS head ----------------------------------------------------------------------------------------------------------------
def tap_case(hip, C, HW, B, tag, tail_from=None):
    """forward into a prefilled val (twice: the same bits), backward with gscale None and a device scalar; returns the items.
    tail_from: the first pixel of the second trip; those pixels' gradients are the tail of check_with_tail"""
    f, lin = L.tap_inputs(C, HW, B)
    fd, lind = dev(f), lin.cuda()
    ref, A = L.tap_fwd(f, lin, B)
    base, _ = L.tap_fwd(f, lin, B, dtype=F32)
    val0 = torch.full((B,), L.L1_PREFILL)
    val, val2 = val0.clone().cuda(), val0.clone().cuda()
    hip.lpips_tap_fwd(fd, lind, val, B, HW, C)
    hip.lpips_tap_fwd(fd, lind, val2, B, HW, C)
    assert torch.equal(bits(val), bits(val2)), tag
    items = [("val", val, val0.double() + ref, L.bound_f32(val0 + base, val0.double() + ref, A + val0.double()))]
    for name, g in (("g", None), ("g*gscale", L.GSCALE)):
        gref, G = L.tap_bwd(f, lin, L.TAP_COEF, B, g)
        gbase, _ = L.tap_bwd(f, lin, L.TAP_COEF, B, g, dtype=F32)
        got = hip.lpips_tap_bwd(fd, lind, L.TAP_COEF, B, HW, C, gscale=None if g is None else torch.tensor([g]).cuda())
        got = got.float().cpu().view(B, HW, C)
        assert bool(torch.isfinite(got).all()), tag
        assert bool((got[0, 0] == 0).all()), tag                                  # the all-zero prediction pixel
        items.append((name, got, gref, L.bound_bf16(gbase, gref, G)))
    if tail_from is not None:
        items = items[:1] + [(n, g_[:, tail_from:], r[:, tail_from:], b[:, tail_from:]) for n, g_, r, b in items[1:]] + items[1:]
    return items


@pytest.mark.parametrize("C", L.TAP_CHANNELS)
def test_tap_head_group_geometry(hip, C):
    """G = C / 8 lanes per pixel, 256 / G pixels per block: HW = 1, 3, one short of and one past a block's pixels (the pixel loop
    then ends at different trips in the groups of one wave); an all-zero prediction pixel, an all-zero target pixel, a pixel with
    one nonzero channel; val prefilled (the entry adds); finite everywhere"""
    for HW, B in itertools.product(L.tap_hws(C), L.BATCHES):
        tag = "tap C=%d HW=%d B=%d" % (C, HW, B)
        check(tag, tap_case(hip, C, HW, B, tag))


@pytest.mark.parametrize("C,HW", L.TAP_SWITCH + L.TAP_TRIP)
def test_tap_head_combine_switch_and_second_trip(hip, C, HW):
    """64 | 65 partials: the last case of the one-thread combine, the first of the 32-lane one; 1025 blocks' worth of pixels: the
    1024-block cap, a second trip of the pixel loop.  There the gradients of the pixels past the first trip are checked on their
    own too, and so is their share of val: a second forward with every first-trip pixel zeroed in both images (a zero pixel pair
    adds nothing)"""
    blocks = (HW * (C // 8) + 255) // 256
    assert blocks in (64, 65) or blocks > 1024
    tag = "tap C=%d HW=%d (%d blocks)" % (C, HW, blocks)
    first = 1024 * L.tap_ppb(C) if blocks > 1024 else None
    check(tag, tap_case(hip, C, HW, 1, tag, first))
    if first is not None:
        f, lin = L.tap_inputs(C, HW, 1)
        f[:, :first] = 0.0
        ref, A = L.tap_fwd(f, lin, 1)
        base, _ = L.tap_fwd(f, lin, 1, dtype=F32)
        val = torch.zeros(1).cuda()
        hip.lpips_tap_fwd(dev(f), lin.cuda(), val, 1, HW, C)
        assert float(ref) > 0
        check(tag + " val of the second trip", [("val", val, ref, L.bound_f32(base, ref, A))])


# ---- l1 mean -------------------------------------------------------------------------------------------------------------------
def l1_case(hip, a, b, tag):
    ref = L.l1_mean(a, b).view(1)
    base = L.l1_mean(a, b, dtype=F32).view(1)
    out0 = torch.tensor([L.L1_PREFILL])
    out, out2 = out0.clone().cuda(), out0.clone().cuda()
    hip.l1_mean(a.cuda(), b.cuda(), out)
    hip.l1_mean(a.cuda(), b.cuda(), out2)
    assert torch.equal(bits(out), bits(out2)), tag
    return ("out", out, out0.double() + ref, L.bound_f32(out0 + base, out0.double() + ref, out0.double() + ref))


def test_l1_mean_sizes(hip):
    """one element, one short of / exactly / one past a block, 64 | 65 partials; out prefilled (the entry adds); inputs on the
    2^-6 grid with a fifth of them equal; two calls: the same bits"""
    for n in L.L1_SIZES:
        a, b = L.l1_inputs(n)
        check("l1_mean n=%d" % n, [l1_case(hip, a, b, n)])


# ---- the second trip of every grid-stride loop -----------------------------------------------------------------------------------
def test_second_trip_im2col(hip):
    N, H, W, C = 1, 360, 648, 8
    assert TRIP < N * H * W * 9 * (C // 8) < TRIP + 4096
    x = levels((N * H * W, C), 1, 100, 1.0, 1)                      # nonzero everywhere
    col, ref = hip.im2col3x3(x, N, H, W, C).cpu(), L.im2col(x.cpu(), N, H, W, C)
    assert torch.equal(col, ref) and torch.equal(col.reshape(-1)[TRIP * 8:], ref.reshape(-1)[TRIP * 8:])


def test_second_trip_col2im(hip):
    """act + tapg form on the 1/4 grid: every sum is exact in fp32 and in bf16, the fp32 reference is the exact result and the
    whole output is compared bit for bit"""
    N, H, W, C = 1, 128, 257, 512
    assert TRIP < N * H * W * (C // 8) < TRIP + 16384
    dcol, tapg = levels((N * H * W, 9 * C), -4, 5, 0.25, 2), levels((N * H * W, C), -4, 5, 0.25, 3)
    act = levels((N * H * W, C), -1, 3, 0.5, 4)
    out = hip.col2im3x3(dcol, N, H, W, C, act=act, tapg=tapg).cpu()
    ref = L.col2im(dcol.cpu(), N, H, W, C, act=act.cpu(), tapg=tapg.cpu(), dtype=F32)[0].to(BF)
    assert bool((ref.float().abs() <= 10).all()) and int((ref != 0).sum()) > ref.numel() // 4
    assert torch.equal(out, ref) and torch.equal(out.reshape(-1)[TRIP * 8:], ref.reshape(-1)[TRIP * 8:])


BIG_POOL = (1, 256, 514, 512)


def test_second_trip_maxpool_fwd(hip):
    N, H, W, C = BIG_POOL
    assert TRIP < N * (H // 2) * (W // 2) * (C // 8) < TRIP + 16384
    x = levels((N * H * W, C), -2, 3, 0.5, 5)
    y, ref = hip.maxpool2_fwd(x, N, H, W, C).cpu(), L.maxpool_fwd(x.cpu(), N, H, W, C)
    assert torch.equal(y, ref) and torch.equal(y.reshape(-1)[TRIP * 8:], ref.reshape(-1)[TRIP * 8:])


def test_second_trip_maxpool_bwd(hip):
    """with tapg; the windows past the first trip (whole windows: 64 lane groups each) on their own as well"""
    N, H, W, C = BIG_POOL
    x = levels((N * H * W, C), -2, 3, 0.5, 5)
    gy = levels((N * (H // 2) * (W // 2), C), -100, 101, 0.03125, 6)
    tapg = levels((N * H * W, C), -100, 101, 0.0078125, 7)
    dz = hip.maxpool2_bwd(gy, x, N, H, W, C, tapg=tapg).cpu()
    ref = L.maxpool_bwd(gy.cpu(), x.cpu(), N, H, W, C, tapg=tapg.cpu())
    assert torch.equal(dz, ref)
    w0 = TRIP // (C // 8)
    assert torch.equal(L._windows(dz, N, H, W, C).reshape(-1, 4, C)[w0:], L._windows(ref, N, H, W, C).reshape(-1, 4, C)[w0:])


def test_second_trip_conv1_fwd(hip):
    N, H, W = 1, 512, 513
    assert TRIP < N * H * W * 8 < TRIP + 8192
    w1, b1 = L.conv1_weights()
    img = L.conv1_inputs(N, H, W)[0]
    ref, A = L.conv1_fwd(img, w1, b1)
    base, _ = L.conv1_fwd(img, w1, b1, dtype=F32)
    out = hip.lpips_conv1_fwd(img.cuda(), w1.cuda(), b1.cuda())
    check_with_tail("trip2 conv1 fwd", [("out", out.float().cpu(), ref, L.bound_bf16(base, ref, A))], TRIP * 8)


def test_second_trip_conv1_bwd(hip):
    """dz in {-2..2}, w1 multiples of 1/16 in [-1, 1]: every product is a multiple of 1/16 and every 576-term sum stays below
    2^11, so the transposed convolution is exact in fp32 in any order and the fp32 reference of that part is the exact result;
    the division by the scale and the L1 term are then taken in float64"""
    N, H, W = 1, 1449, 1448
    assert TRIP < N * H * W < TRIP + 1024
    g = torch.Generator().manual_seed(8)
    w1 = torch.randint(-16, 17, (27, 64), generator=g).float() / 16
    pred = levels((N, 3, H, W), -100, 101, 0.015625, 9).float()
    target = torch.where(levels((N, 3, H, W), 0, 3, 1.0, 10) == 0, pred, levels((N, 3, H, W), -100, 101, 0.015625, 11).float())
    dz = levels((N * H * W, 64), -2, 3, 1.0, 12)
    l1c = 1.0 / pred.numel()
    gs = torch.tensor([L.GSCALE])
    dimg = hip.lpips_conv1_bwd(dz, w1.cuda(), pred, target, l1c, gscale=gs.cuda()).cpu()
    pc, tc = pred.cpu(), target.cpu()
    assert int((pc == tc).sum()) > pc.numel() // 4
    parts = L.conv1_bwd_parts(dz.cpu(), w1, N, H, W, dtype=F32)
    assert float(parts[1].max()) < 2048
    ref, G = L.conv1_bwd(None, w1, pc, tc, l1c, L.GSCALE, parts=parts)
    base, _ = L.conv1_bwd(None, w1, pc, tc, l1c, L.GSCALE, dtype=F32, parts=parts)
    bound = L.bound_f32(base, ref, G)
    check("trip2 conv1 bwd", [("dimg", dimg, ref, bound)])
    check("trip2 conv1 bwd past the first trip", [("dimg", dimg.reshape(3, -1)[:, TRIP:], ref.reshape(3, -1)[:, TRIP:], bound.reshape(3, -1)[:, TRIP:])])


def test_second_trip_l1_mean(hip):
    """and the elements past the first trip on their own: a second call with the first trip's elements equal in a and b"""
    n = TRIP + 1000
    a, b = L.l1_inputs(n)
    check("trip2 l1_mean", [l1_case(hip, a, b, n)])
    b[:TRIP] = a[:TRIP]
    assert float(L.l1_mean(a, b)) > 0
    check("trip2 l1_mean past the first trip", [l1_case(hip, a, b, n)])


# ---- every stage of the network on its own -----------------------------------------------------------------------------------------
def gemm_items(name, out, x, w, bias, relu):
    """out [M, N] (bf16, device) against x [M, K] @ w [N, K]^T (+ bias, ReLU) of the kernel's own bf16 operands"""
    x, w = x.float().cpu(), w.float().cpu()
    b = None if bias is None else bias.float().cpu()

    def f(dtype):
        pre = x.to(dtype) @ w.to(dtype).t()
        if b is not None:
            pre = pre + b.to(dtype)
        return torch.relu(pre) if relu else pre
    A = x.double().abs() @ w.double().abs().t() + (0 if b is None else b.double().abs())
    ref = f(F64)
    return (name, out, ref, L.bound_bf16(f(F32), ref, A))


def test_every_stage_of_the_network_on_its_own(hip):
    """B = 1, 32 x 32, two images through LPIPSVGG16._features: each of the 13 convolutions (im2col + GEMM with bias + ReLU:
    K = 27 to 4608, N = 64 to 512, M = 2048 down to 8) and of the 4 pools against the float64 reference of that stage applied to the
    kernel's own bf16 input; then every kernel of the backward stage loop against the float64 reference of that step applied to the
    operands the kernel read (its own upstream gradient): 5 tap gradients, 12 GEMMs, 12 col2im, 4 pool routings, conv1 bwd"""
    from climate_learn.metrics import lpips_hip as LH
    sd = {k: (v if "lin" in k else L.rt(v)) for k, v in O.init_lpips_weights(5).items()}
    net = LH.LPIPSVGG16("cuda", sd)
    B, H, W = 1, 32, 32
    g = torch.Generator().manual_seed(132)
    pred = torch.randn(B, 3, H, W, generator=g) * 0.6
    target = pred * 0.7 + 0.5 * torch.randn(B, 3, H, W, generator=g)
    img = torch.cat([pred, target])
    N = 2 * B
    acts = net._features(img.cuda())
    w1, b1 = net.w1.cpu(), net.b1.cpu()
    ref, A = L.conv1_fwd(img, w1, b1)
    items = [("conv0", acts[0][1], ref, L.bound_bf16(L.conv1_fwd(img, w1, b1, dtype=F32)[0], ref, A))]
    li = 0
    for j in range(1, len(acts)):
        kind, out, h, w, c = acts[j]
        _, x, ph, pw, pc = acts[j - 1]
        if kind == "pool":
            assert torch.equal(out.cpu(), L.maxpool_fwd(x.cpu(), N, ph, pw, pc)), j
            continue
        lay = net.layers[li]
        li += 1
        items.append(gemm_items("conv%d" % li, out, L.im2col(x.cpu(), N, ph, pw, pc), lay["w"], lay["b"], True))
    assert li == 12 and len(acts) == 17
    check("stages fwd", items)

    gs = 3.0
    recs = []
    dimg = LH._input_gradient(net, acts, LH._tap_positions(acts), (B, H, W), pred.cuda(), target.cuda(), torch.tensor([gs]).cuda(),
                              record=lambda kind, j, out, **kw: recs.append((kind, j, out, kw)))
    items, count = [], {}
    for kind, j, out, kw in recs:
        count[kind] = count.get(kind, 0) + 1
        name = "dimg" if kind == "conv1" else "%s%d" % (kind, j)
        if kind == "tap":
            c = kw["feats"].shape[1]
            f, lin = kw["feats"].float().cpu().view(N, -1, c), kw["lin"].cpu()
            ref, G = L.tap_bwd(f, lin, kw["coef"], B, gs)
            items.append((name, out.float().cpu().view(ref.shape), ref, L.bound_bf16(L.tap_bwd(f, lin, kw["coef"], B, gs, dtype=F32)[0], ref, G)))
        elif kind == "gemm":
            items.append(gemm_items(name, out, kw["gz"], kw["wt"], None, False))
        elif kind == "col2im":
            a = [kw["dcol"].float().cpu()] + list(kw["dims"])
            k = dict(act=None if kw["act"] is None else kw["act"].float().cpu(), tapg=None if kw["tapg"] is None else kw["tapg"].float().cpu())
            ref, A = L.col2im(*a, **k)
            items.append((name, out, ref, L.bound_bf16(L.col2im(*a, dtype=F32, **k)[0], ref, A)))
        elif kind == "pool":
            assert torch.equal(out.cpu(), L.maxpool_bwd(kw["g"].cpu(), kw["x"].cpu(), *kw["dims"], tapg=kw["tapg"].cpu())), name
        else:
            dz = kw["dz"].float().cpu()
            ref, G = L.conv1_bwd(dz, w1, pred, target, 1.0 / pred.numel(), gs)
            items.append((name, out, ref, L.bound_f32(L.conv1_bwd(dz, w1, pred, target, 1.0 / pred.numel(), gs, dtype=F32)[0], ref, G)))
    assert count == dict(tap=5, gemm=12, col2im=12, pool=4, conv1=1) and dimg is recs[-1][2]
    check("stages bwd", items)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_on_real_buffers(hip):
    """the C entries refuse, with an error code and without a launch, what they cannot serve: C not a multiple of 8, a tap C
    outside {64, 128, 256, 512}, odd H or W for the pools, tapg without act, non-positive sizes; the wrappers refuse, with
    HipBackendError and before the call, sizes that do not match the tensors handed over.  Every destination keeps its sentinel."""
    lib, s = hip.lib(), torch.cuda.current_stream().cuda_stream
    src = torch.ones(1 << 16, dtype=BF).cuda()
    f32 = torch.ones(1 << 14).cuda()
    dst, dstf = torch.full((1 << 16,), SENTINEL, dtype=BF).cuda(), torch.full((1 << 14,), SENTINEL).cuda()
    p, q, pf, qf = src.data_ptr(), dst.data_ptr(), f32.data_ptr(), dstf.data_ptr()
    bad_dims = [(2, 4, 4, 12), (2, 4, 4, 4), (0, 4, 4, 8), (2, 0, 4, 8), (2, 4, -1, 8), (2, 4, 4, 0), (-2, 4, 4, 8)]
    rcs = {}
    for d in bad_dims:
        rcs["im2col", d] = lib.orbit2_im2col3x3(p, q, *d, s)
        rcs["col2im", d] = lib.orbit2_col2im3x3(p, p, p, q, *d, s)
        rcs["pool fwd", d] = lib.orbit2_maxpool2_fwd(p, q, *d, s)
        rcs["pool bwd", d] = lib.orbit2_maxpool2_bwd(p, p, p, q, *d, s)
    for d in ((2, 3, 4, 8), (2, 4, 5, 8), (1, 1, 1, 8)):
        rcs["pool fwd", d] = lib.orbit2_maxpool2_fwd(p, q, *d, s)
        rcs["pool bwd", d] = lib.orbit2_maxpool2_bwd(p, p, None, q, *d, s)
    rcs["col2im tapg without act"] = lib.orbit2_col2im3x3(p, None, p, q, 2, 4, 4, 8, s)
    for d in ((0, 4, 4), (1, 0, 4), (1, 4, -3)):
        rcs["conv1 fwd", d] = lib.orbit2_lpips_conv1_fwd(pf, pf, pf, q, *d, s)
        rcs["conv1 bwd", d] = lib.orbit2_lpips_conv1_bwd(p, pf, pf, pf, 0.5, None, qf, *d, s)
    for d in ((2, 8, 96), (2, 8, 8), (2, 8, 1024), (2, 8, 0), (0, 8, 64), (2, 0, 64), (-1, 8, 64)):
        rcs["tap fwd", d] = lib.orbit2_lpips_tap_fwd(p, pf, qf, *d, qf + 4096, s)
        rcs["tap bwd", d] = lib.orbit2_lpips_tap_bwd(p, pf, q, 0.5, None, *d, s)
    for n in (0, -5):
        rcs["l1", n] = lib.orbit2_l1_mean(pf, pf, qf, n, qf + 4096, s)
    torch.cuda.synchronize()
    assert not [k for k, rc in rcs.items() if rc == 0], rcs
    assert bool((dst == SENTINEL).all()) and bool((dstf == SENTINEL).all())

    E = hip.HipBackendError
    x = torch.ones(2 * 4 * 4, 8, dtype=BF).cuda()
    col = torch.ones(2 * 4 * 4, 72, dtype=BF).cuda()
    gy = torch.ones(2 * 2 * 2, 8, dtype=BF).cuda()
    img, w1, b1 = torch.ones(2, 3, 4, 4).cuda(), torch.ones(27, 64).cuda(), torch.ones(64).cuda()
    dz = torch.ones(2 * 4 * 4, 64, dtype=BF).cuda()
    feats, lin, one = torch.ones(2 * 2 * 8, 64, dtype=BF).cuda(), torch.ones(64).cuda(), torch.ones(1).cuda()
    val, out = torch.full((2,), SENTINEL).cuda(), torch.full((1,), SENTINEL).cuda()
    calls = [
        lambda: hip.im2col3x3(x, 3, 4, 4, 8), lambda: hip.im2col3x3(x, 2, 4, 5, 8), lambda: hip.im2col3x3(x, 2, 4, 4, 16),
        lambda: hip.im2col3x3(x[:, :4].contiguous(), 2, 4, 4, 4), lambda: hip.im2col3x3(x, 0, 4, 4, 8),
        lambda: hip.col2im3x3(col, 3, 4, 4, 8), lambda: hip.col2im3x3(x, 2, 4, 4, 8), lambda: hip.col2im3x3(col, 2, 4, 4, 8, tapg=x),
        lambda: hip.col2im3x3(col, 2, 4, 4, 8, act=x[:-1]), lambda: hip.col2im3x3(col, 2, 4, 4, 8, act=x, tapg=gy),
        lambda: hip.maxpool2_fwd(x, 2, 4, 8, 8), lambda: hip.maxpool2_fwd(x[:30], 2, 3, 5, 8), lambda: hip.maxpool2_fwd(x, 4, 4, 4, 8),
        lambda: hip.maxpool2_bwd(gy, x, 2, 4, 8, 8), lambda: hip.maxpool2_bwd(x, x, 2, 4, 4, 8), lambda: hip.maxpool2_bwd(gy, x, 2, 4, 4, 8, tapg=gy),
        lambda: hip.maxpool2_bwd(gy[:6], x[:30], 2, 3, 5, 8),
        lambda: hip.lpips_conv1_fwd(img[:, :2].contiguous(), w1, b1), lambda: hip.lpips_conv1_fwd(img[0], w1, b1),
        lambda: hip.lpips_conv1_fwd(torch.ones(2, 4, 4, 4).cuda(), w1, b1), lambda: hip.lpips_conv1_fwd(img, w1[:26], b1),
        lambda: hip.lpips_conv1_fwd(img, w1, b1[:63]), lambda: hip.lpips_conv1_fwd(img[:0], w1, b1),
        lambda: hip.lpips_conv1_bwd(dz, w1, img, img[:1], 0.5), lambda: hip.lpips_conv1_bwd(dz[:-1], w1, img, img, 0.5),
        lambda: hip.lpips_conv1_bwd(dz, w1[:26], img, img, 0.5), lambda: hip.lpips_conv1_bwd(dz, w1, img, img, 0.5, gscale=one[:0]),
        lambda: hip.lpips_conv1_bwd(dz, w1, torch.ones(2, 4, 4, 3).cuda(), torch.ones(2, 4, 4, 3).cuda(), 0.5),
        lambda: hip.lpips_tap_fwd(feats, lin, val, 3, 8, 64), lambda: hip.lpips_tap_fwd(feats, lin, val, 2, 4, 128),
        lambda: hip.lpips_tap_fwd(feats, lin[:32], val, 2, 8, 64), lambda: hip.lpips_tap_fwd(feats, lin, val[:1], 2, 8, 64),
        lambda: hip.lpips_tap_fwd(feats.view(-1, 32), lin[:32], val, 2, 16, 32), lambda: hip.lpips_tap_fwd(feats, lin, val, 2, 0, 64),
        lambda: hip.lpips_tap_bwd(feats, lin, 0.5, 3, 8, 64), lambda: hip.lpips_tap_bwd(feats, lin[:32], 0.5, 2, 8, 64),
        lambda: hip.lpips_tap_bwd(feats.view(-1, 32), lin[:32], 0.5, 2, 16, 32), lambda: hip.lpips_tap_bwd(feats, lin, 0.5, 2, 8, 64, gscale=one[:0]),
        lambda: hip.l1_mean(img, img[:1], out), lambda: hip.l1_mean(img, img, out[:0]), lambda: hip.l1_mean(img[:0], img[:0], out),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(E):
            call()
            pytest.fail("wrapper call %d was not refused" % i)
    torch.cuda.synchronize()
    assert bool((val == SENTINEL).all()) and bool((out == SENTINEL).all())
    # and the same operands with the right sizes are served
    hip.lpips_tap_fwd(feats, lin, val, 2, 8, 64)
    hip.l1_mean(img, img, out)
    assert hip.im2col3x3(x, 2, 4, 4, 8).shape == (32, 72) and hip.maxpool2_bwd(gy, x, 2, 4, 4, 8, tapg=x).shape == (32, 8)
    assert float(out) == SENTINEL and bool((val == SENTINEL).all())           # identical images, identical features: + 0
