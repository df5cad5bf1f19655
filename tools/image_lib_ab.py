"""Same-box, same-process A/B of two builds of the image-tail, loss and score kernels (csrc/image.hip, csrc/loss.hip,
csrc/ensemble.hip):
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/image_lib_ab.py orbit-2_amd/lib/alt/<name>.so [other.so]
tools/lib_ab.py loads the two builds, keeps the guarded buffers, times and sums up; this file calls every entry of the three files
in both.  Cases, all taken from the test modules:
  conv3x3 fwd / bwd / ws query  tests/rowimage_ref's CONV_CHANNELS x CONV_SIZES at B = 1 and 3 (both modes, chan_idx, addend, Cout
                                17 / 18 / 36), dweight and dbias prefilled;
  unpatchify, its three forms   tests/test_image_tail_edges_gpu.py::test_unpatchify_patch_and_scale's p, s, C and grids;
  clamp fwd / bwd               the first and the last channel of a [2, 3, 7, 9] image with signed zeros;
  loss fwd / bwd                kinds 0, 1, 2 on rowimage_ref.LOSS_SHAPES, target larger or not, lat_w and chan_w off and on, the
                                block partials of the workspace included;
  the three masked entries      tests/test_masked_gpu.py's UNALIGNED, ALIGNED and larger-than-one-sweep cases (NaN and Inf targets),
                                no mask, [H,W], [B,C,H,W] and a mask with nothing valid, kinds 0 and 1;
  eval_moments                  the same fields without holes, lat_w and climatology off and on;
  ensemble_update               k = 1 and 3, n = 4099 (n % 4 != 0), bases aligned and 3 floats off;
  gaussian_scores               tests/test_ensemble_scores_gpu.py's SHAPE with std == 0 in one channel;
  ensemble_scores               that module's member counts and one for the padded size 32, every output;
  posembed fwd / bwd            tests/test_hip_ops.py::test_posembed_table_forward_backward's six (oh, nh, D).
Rules: every output is bitwise equal inside its NaN-filled guarded buffer.  The sums that end in double atomics in no fixed order
(eval_moments, masked_moments, gaussian_scores, ensemble_scores' sums) are bitwise equal where an image has one workgroup; with
k > 1 workgroups the builds agree within (k - 1) 2^-52 of the sum of the summands' magnitudes (tools/resample_lib_ab.py's rule,
tests/resample_ref.moments64; the summands of the two score entries are not negative, so their sums are their magnitudes).
Then every leg is timed, both builds interleaved: the losses, masked losses and both moments at tools/masked_bench.py's two shapes,
the three convolutions of the interm_1b tail (bench.py's default step) forward and backward, ensemble_update and gaussian_scores at
tools/mc_dropout_bench.py's field, posembed 16 -> 64 at D = 1024.  Exit status 1 if a rule is broken."""
import itertools
import numpy as np
import torch
from lib_ab import BITS, GUARD, P, S, count, guarded, libs, ok, summary, tally
from climate_learn.metrics.functional import _mask_operand
from tests import ensemble_ref as E, resample_ref as RS, rowimage_ref as R
from tests import test_ensemble_scores_gpu as TE, test_hip_ops, test_image_tail_edges_gpu as TI, test_masked_gpu as TM

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
BLOCKS = 64                                                                   # ORBIT2_LOSS_BLOCKS
cuda = lambda v: None if v is None else v.cuda()
marks = lambda f: {m.args[0]: m.args[1] for m in f.pytestmark if m.name == "parametrize"}
multi_equal = 0


def compare(kind, tag, call, dests, timing=False, lead=GUARD):
    """call(lib, one address per destination) in both builds.  dests: (elements, dtype, prefill or None, must be written); every
    buffer whole, bit for bit (int64 outputs live in float64 buffers).  Returns the tree build's destinations."""
    G = [guarded(n, dt, lead, pre) for n, dt, pre, _ in dests]
    run = lambda lib, key: ok(call(lib, *[g[key].data_ptr() + lead * g[key].element_size() for g in G]))
    for key, lib in libs.items(): run(lib, key)
    torch.cuda.synchronize()
    eq = all(torch.equal(g["tree"].view(BITS[d[1]]), g["alt"].view(BITS[d[1]])) for g, d in zip(G, dests)) \
        and not any(d[3] and bool(torch.isnan(g["tree"][lead:lead + d[0]]).any()) for g, d in zip(G, dests))
    tally(kind, "%-16s %s: bitwise equal %s" % (kind, tag, eq), eq, run if timing else None, {key: key for key in libs})
    return [g["tree"][lead:lead + d[0]] for g, d in zip(G, dests)]


def sums(kind, tag, call, shape, k, mags, extra=(), timing=False):
    """an entry whose float64 [shape] sums end in double atomics (extra: its fixed-order destinations).  mags: () -> magnitudes"""
    global multi_equal
    G = [guarded(int(np.prod(shape)), F64)] + [guarded(n, dt, prefill=pre) for n, dt, pre, _ in extra]
    run = lambda lib, key: ok(call(lib, *[g[key].data_ptr() + GUARD * g[key].element_size() for g in G]))
    for key, lib in libs.items(): run(lib, key)
    torch.cuda.synchronize()
    a, b = (G[0][key].cpu().numpy() for key in ("tree", "alt"))
    body = np.zeros(a.shape, bool)
    body[GUARD:GUARD + int(np.prod(shape))] = True
    fixed = np.array_equal(a.view(np.int64)[~body], b.view(np.int64)[~body]) and bool(np.isfinite(a[body]).all()) \
        and all(torch.equal(g["tree"].view(BITS[d[1]]), g["alt"].view(BITS[d[1]])) for g, d in zip(G[1:], extra)) \
        and not any(d[3] and bool(torch.isnan(g["tree"][GUARD:GUARD + d[0]]).any()) for g, d in zip(G[1:], extra))
    a, b = a[body].reshape(shape), b[body].reshape(shape)
    eq = bool(np.array_equal(a, b))
    line = "%-16s %s k=%d: sums bitwise equal %s, the rest and the guards %s" % (kind, tag, k, eq, fixed)
    if k == 1:
        passed = fixed and eq
    else:
        bound = (k - 1) * 2.0 ** -52 * np.broadcast_to(mags(a), shape)
        within = bool((np.abs(a - b) <= bound).all())
        worst = int(np.argmax(np.abs(a - b) / np.maximum(bound, 1e-300)))
        passed, kind = fixed and within, kind + ", k > 1"
        multi_equal += eq
        line += ", largest difference %.3g (bound there %.3g): within %s" % (np.abs(a - b).flat[worst], bound.flat[worst], within)
    tally(kind, line, passed, run if timing else None, {key: key for key in libs})


def agree(what, args):
    n = {k: getattr(lib, what)(*args) for k, lib in libs.items()}
    count.setdefault("queries", [0, 0])
    count["queries"][0] += 1; count["queries"][1] += n["tree"] == n["alt"] > 0
    if not n["tree"] == n["alt"] > 0: print("%s%r: tree %d, alt %d" % (what, args, n["tree"], n["alt"]), flush=True)
    return n["tree"]


image_blocks = lambda pixels: min(64, -(-pixels // 2048))                     # score_sums.h: o2_image_blocks


def mag12(pred, target, lat, clim, valid=None):
    """the magnitudes of the twelve moments' summands: tests/resample_ref.moments64 on the host; on the device in float64 for the
    timed fields, which the host would take minutes over.  valid: the masked entry adds nothing at the other pixels"""
    H, W = pred.shape[2:]
    if pred.numel() <= 1 << 21:
        p, t = pred.cpu().numpy().astype(np.float64), target[:, :, :H, :W].cpu().numpy().astype(np.float64)
        if valid is not None:
            v = valid.cpu().numpy()
            c = 0.0 if clim is None else clim.cpu().numpy()[None]
            p, t = np.where(v, p, c), np.where(v, t, c)
        return RS.moments64(p, t, None if lat is None else lat[:H].cpu().numpy(), None if clim is None else clim.cpu().numpy())[1]
    c = 0.0 if clim is None else clim.double()
    a, b = pred.double() - c, target[:, :, :H, :W].double() - c
    if valid is not None: a, b = torch.where(valid, a, 0.0), torch.where(valid, b, 0.0)
    w = 1.0 if lat is None else lat[:H].double().view(1, 1, H, 1)
    d = a - b
    terms = (a, b, a * a, b * b, a * b, w * d * d, w * d, w * a, w * b, w * a * b, w * a * a, w * b * b)
    return torch.stack([x.abs().sum((2, 3)) for x in terms], -1).cpu().numpy()


# ---- csrc/image.hip ------------------------------------------------------------------------------------------------------------
def conv_case(B, H, W, cfg, tag, timing=False):
    mode, Cin, Cout, r, ctot, addend = cfg
    x, idx, w, b, add, dout = (cuda(v) for v in R.conv_inputs(B, H, W, mode, Cin, Cout, r, ctot, addend))
    Ha, Wa = (add.shape[2], add.shape[3]) if add is not None else (0, 0)
    n_out, n_pre = dout.numel(), B * Cout * H * W
    if mode == 0:
        pre = None
        compare("conv fwd", tag, lambda lib, o: lib.orbit2_conv3x3_fwd(P(x), P(idx), x.shape[1], P(w), P(b), o, None, P(add), Ha, Wa,
                                                                       B, Cin, Cout, H, W, 0, r, S()), [(n_out, F32, None, True)], timing)
    else:
        _, pre = compare("conv fwd", tag, lambda lib, o, p: lib.orbit2_conv3x3_fwd(P(x), P(idx), x.shape[1], P(w), P(b), o, p, None, 0, 0,
                                                                                   B, Cin, Cout, H, W, 1, r, S()),
                         [(n_out, F32, None, True), (n_pre, F32, None, True)], timing)
        pre = pre.clone()
    nws = agree("orbit2_conv3x3_bwd_ws_floats", (B, Cin, Cout, H, W))
    compare("conv bwd", tag, lambda lib, di, dw, db, ws: lib.orbit2_conv3x3_bwd(P(dout), P(x), P(idx), x.shape[1], P(w), P(pre), di, dw, db,
                                                                                B, Cin, Cout, H, W, mode, r, ws, S()),
            [(B * Cin * H * W, F32, None, True), (w.numel(), F32, 0.5, True), (Cout, F32, 0.5, True), (nws, F32, None, True)],
            timing)


def image_cases():
    for cfg, B, (H, W) in itertools.product(R.CONV_CHANNELS, (1, 3), R.CONV_SIZES):
        conv_case(B, H, W, cfg, "m%d %d->%d r%d idx %s add %s" % cfg + " %dx%d B=%d" % (H, W, B))
    m = marks(TI.test_unpatchify_patch_and_scale)
    for p, s, C, (h, w) in itertools.product(m["p"], m["s"], (1, 3), ((4, 8), (8, 12))):
        B, g = 2, torch.Generator().manual_seed(10 * p + s)
        t32 = torch.randn(B, h * w // (p * p), C * (s * p) ** 2, generator=g).cuda()
        t16, dimg = t32.to(BF), torch.randn(B, C, h * s, w * s, generator=g).cuda()
        tag, a = "p=%d s=%d C=%d %dx%d" % (p, s, C, h, w), (B, C, h, w, p, s)
        compare("unpatchify fwd", tag, lambda lib, o: lib.orbit2_unpatchify_fwd(P(t16), o, *a, S()), [(dimg.numel(), F32, None, True)])
        compare("unpatchify f32", tag, lambda lib, o: lib.orbit2_unpatchify_fwd_f32(P(t32), o, *a, S()), [(dimg.numel(), F32, None, True)])
        compare("unpatchify bwd", tag, lambda lib, o: lib.orbit2_unpatchify_bwd(P(dimg), o, *a, S()), [(t32.numel(), BF, None, True)])
    for C, chan in marks(TI.test_clamp_channel_first_and_last)["C,chan"]:
        g = torch.Generator().manual_seed(8 + chan)
        x = torch.randn(2, C, 7, 9, generator=g)
        x[:, :, 0, :4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
        gr = torch.randn(x.shape, generator=g).cuda()
        y, = compare("clamp fwd", "C=%d chan %d" % (C, chan), lambda lib, o: lib.orbit2_clamp_channel(o, 2, C, 63, chan, S()),
                     [(x.numel(), F32, x.cuda().flatten(), True)])
        y = y.clone()
        compare("clamp bwd", "C=%d chan %d" % (C, chan), lambda lib, o: lib.orbit2_clamp_channel_bwd(P(y), o, 2, C, 63, chan, S()),
                [(x.numel(), F32, gr.flatten(), True)])
    for oh, nh, D in marks(test_hip_ops.test_posembed_table_forward_backward)["oh,nh,D"]:
        posembed_case(oh, nh, D)


def posembed_case(oh, nh, D, timing=False):
    ow, nw = 2 * oh, 2 * nh
    g = torch.Generator().manual_seed(oh * 131 + nh)
    pe, sw, sb, go = (torch.randn(*s, generator=g).cuda() for s in ((oh * ow, D), (D,), (D,), (nh * nw, D)))
    tag = "%dx%d -> %dx%d D=%d" % (oh, ow, nh, nw, D)
    for on in (True,) if timing else (True, False):
        compare("posembed fwd", tag + " res %d" % on, lambda lib, o: lib.orbit2_posembed_fwd(
            P(pe), P(sw) if on else None, P(sb) if on else None, 0.703, o, oh, ow, nh, nw, D, S()), [(nh * nw * D, F32, None, True)], timing)
    compare("posembed bwd", tag, lambda lib, o: lib.orbit2_posembed_bwd(P(go), o, oh, ow, nh, nw, D, S()), [(oh * ow * D, F32, None, True)],
            timing)


# ---- csrc/loss.hip -------------------------------------------------------------------------------------------------------------
def loss_case(pred, tgt, lat, cw, kind, tag, timing=False):
    B, C, H, W = pred.shape
    Ht, Wt = tgt.shape[2:]
    gs = torch.tensor([R.LOSS_GSCALE]).cuda()
    compare("loss fwd", tag, lambda lib, o, ws: lib.orbit2_loss_fwd(P(pred), P(tgt), Ht, Wt, P(lat), P(cw), o, ws, B, C, H, W, kind, S()),
            [(C + 1, F32, None, True), (2 * B * C * BLOCKS, F32, None, True)], timing)
    compare("loss bwd", tag, lambda lib, o: lib.orbit2_loss_bwd(P(pred), P(tgt), Ht, Wt, P(lat), P(cw), P(gs), o, B, C, H, W, kind, S()),
            [(pred.numel(), F32, None, True)], timing)


def masked_case(pred, tgt, mask, lat, cw, kind, tag, timing=False):
    B, C, H, W = pred.shape
    Ht, Wt = tgt.shape[2:]
    mk = _mask_operand(mask, pred, tgt)
    gs = torch.ones(1, device="cuda")
    _, cnt, _ = compare("masked loss fwd", tag, lambda lib, o, c, ws: lib.orbit2_masked_loss_fwd(
        P(pred), P(tgt), Ht, Wt, P(mk[0]), *mk[1:], P(lat), P(cw), o, c, ws, B, C, H, W, kind, S()),
        [(C + 1, F32, None, True), (C + 1, F64, None, True), (2 * B * C * BLOCKS, F32, None, True)], timing)
    cnt = cnt.clone()
    compare("masked loss bwd", tag, lambda lib, o: lib.orbit2_masked_loss_bwd(
        P(pred), P(tgt), Ht, Wt, P(mk[0]), *mk[1:], P(lat), P(cw), P(gs), P(cnt), o, B, C, H, W, kind, S()), [(pred.numel(), F32, None, True)],
        timing)


def moments_cases(pred, tgt, mask, lat, clim, tag, plain, timing=False):
    """orbit2_masked_moments, and orbit2_eval_moments where the target's crop is finite (plain)"""
    B, C, H, W = pred.shape
    Ht, Wt = tgt.shape[2:]
    mk = _mask_operand(mask, pred, tgt)
    if plain:
        sums("eval_moments", tag, lambda lib, o: lib.orbit2_eval_moments(P(pred), P(tgt), Ht, Wt, P(lat), P(clim), o, B, C, H, W, S()),
             (B, C, 12), image_blocks(H * W), lambda a: mag12(pred, tgt, lat, clim), timing=timing)
    valid = TM.ref.validity(pred.cpu(), tgt.cpu(), None if mask is None else mask.cpu()).cuda()
    mags = lambda a: np.concatenate([mag12(pred, tgt, lat, clim, valid), a[..., 12:]], -1)          # the count: integers, exact
    sums("masked_moments", tag, lambda lib, o: lib.orbit2_masked_moments(P(pred), P(tgt), Ht, Wt, P(mk[0]), *mk[1:], P(lat), P(clim), o,
                                                                          B, C, H, W, S()),
         (B, C, 13), image_blocks(H * (-(-W // 4)) * 4), mags, timing=timing)


def loss_cases():
    for (H, W), kind, larger, lat, chan in itertools.product(R.LOSS_SHAPES, (0, 1, 2), (False, True), (False, True), (False, True)):
        pred, tgt = R.loss_inputs(H, W, larger)
        latw = R.loss_latw(H, tgt.shape[2]).float().cuda() if lat else None
        loss_case(pred.cuda(), tgt.cuda(), latw, torch.tensor(R.LOSS_CHANW).cuda() if chan else None, kind,
                  "kind %d %dx%d larger %d lat %d chan %d" % (kind, H, W, larger, lat, chan))
    big = marks(TM.test_plane_larger_than_one_sweep)["shapes"]
    for shapes in (TM.UNALIGNED, TM.ALIGNED) + tuple(big):
        (B, C, H, W), holes = shapes[0], TM.make_case(*shapes)
        pred, tgt = TM.poison(holes[0], holes[1], None)[0].cuda(), holes[1].cuda()
        lat, cw = TM.lat_weights(H).cuda(), torch.tensor(TM.CW[:C]).cuda()
        forms = {"none": None, "hw": holes[2]["hw"].cuda(), "bc": holes[2]["bc"].cuda(), "nothing": torch.zeros(H, W, dtype=torch.uint8).cuda()}
        for (name, mask), kind, lat_on in itertools.product(forms.items(), (0, 1), (False, True)):
            tag = "%dx%dx%dx%d mask %s kind %d lat %d" % (B, C, H, W, name, kind, lat_on)
            masked_case(pred, tgt, mask, lat if lat_on else None, cw, kind, tag)
        finite = [v.cuda() for v in TM.make_case(*shapes, holes=False)[:2]]
        clim = torch.randn(C, H, W, generator=torch.Generator().manual_seed(H)).cuda()
        for (name, mask), lat_on, clim_on in itertools.product(forms.items(), (False, True), (False, True)):
            tag = "%dx%dx%dx%d mask %s lat %d clim %d" % (B, C, H, W, name, lat_on, clim_on)
            moments_cases(finite[0] if name == "none" else pred, finite[1] if name == "none" else tgt, mask, lat if lat_on else None,
                          clim if clim_on else None, tag, plain=name == "none")


# ---- csrc/ensemble.hip ---------------------------------------------------------------------------------------------------------
def update_case(n, k, lead, timing=False):
    g = torch.Generator(device="cuda").manual_seed(n + k)
    x, mean, m2 = (torch.randn(n, device="cuda", generator=g) for _ in range(3))
    compare("ensemble_update", "n=%d k=%d lead %d" % (n, k, lead), lambda lib, m, s: lib.orbit2_ensemble_update(P(x), m, s, n, k, S()),
            [(n, F32, None if k == 1 else mean, True), (n, F32, None if k == 1 else m2.abs(), True)], timing, lead)


def gaussian_case(mean, std, tgt, lat, tag, timing=False):
    B, C, H, W = mean.shape
    sums("gaussian_scores", tag, lambda lib, o: lib.orbit2_gaussian_scores(P(mean), P(std), P(tgt), tgt.shape[2], tgt.shape[3], P(lat), o,
                                                                            B, C, H, W, S()),
         (B, C, 4), image_blocks(H * W), np.abs, timing=timing)


def ensemble_cases():
    for n, k, lead in itertools.product((4099,), (1, 3), (GUARD, GUARD - 3)):
        update_case(n, k, lead)
    B, C, H, W = TE.SHAPE
    lat = torch.tensor(E.lat_weights(H)).cuda()
    members, target = (torch.tensor(v).cuda() for v in E.make_inputs(8, TE.SHAPE, TE.TARGET_HW, 0.0))
    std = members.std(0)
    std[:, 1] = 0.0                                                           # a constant channel: crps = |d|, no NaN
    for lat_on in (False, True):
        gaussian_case(members.mean(0), std, target, lat if lat_on else None, "%dx%dx%dx%d std == 0 in channel 1 lat %d" % (B, C, H, W, lat_on))
    levels = torch.tensor(TE.LEVELS).cuda()
    field, nblk = B * C * H * W, -(-H * W // 256)
    k = min(nblk, 64 if B * C >= 16 else 1024 // (B * C))                     # score_sums.h: o2_image_block_cap
    for n in sorted(set(marks(TE.test_scores_against_float64)["n"]) | {24}):   # 24: the padded size 32, which no test's N reaches
        members, target = (torch.tensor(v).cuda() for v in E.make_inputs(n, TE.SHAPE, TE.TARGET_HW, 280.0))
        for fair in (0, 1):
            sums("ensemble_scores", "N=%d fair %d" % (n, fair), lambda lib, s, cf, hs, q: lib.orbit2_ensemble_scores(
                P(members), field, n, P(target), target.shape[2], target.shape[3], P(lat), s, cf, fair, hs, TE.HI_SEED, q, P(levels),
                len(TE.LEVELS), B, C, H, W, S()), (B, C, 4), k, np.abs,
                [(field, F32, None, True), (B * C * (n + 1), F64, None, True), (len(TE.LEVELS) * field, F32, None, True)])


# ---- every leg alone, timed ----------------------------------------------------------------------------------------------------
def timed_cases():
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    for (B, C, H, W), (Ht, Wt) in (((16, 3, 512, 1024), (721, 1440)), ((16, 3, 512, 1022), (721, 1439))):    # tools/masked_bench.py
        pred, tgt = rand(B, C, H, W), rand(B, C, Ht, Wt)
        tgt[:, :, :H, :W] += 0.6 * pred
        lat, cw = torch.rand(H, device="cuda", generator=g) + 0.5, torch.tensor([1.0, 10.0, 10.0], device="cuda")
        mask = (rand(H, W) > -0.25).to(torch.uint8)
        for kind in (0, 1, 2):
            loss_case(pred, tgt, lat, cw, kind, "timed kind %d W=%d" % (kind, W), True)
        for kind, (name, m) in itertools.product((0, 1), (("none", None), ("hw", mask))):
            masked_case(pred, tgt, m, lat, cw, kind, "timed kind %d mask %s W=%d" % (kind, name, W), True)
        moments_cases(pred, tgt, None, lat, None, "timed W=%d" % W, True, True)
        del pred, tgt
    B, h, w, V, C, s, ratio = 16, 128, 256, 23, 3, 4, 4                       # interm_1b: bench.py's default step (res_slimvit.py)
    for cfg, (H, W) in (((1, C + 4, ratio * s * s, s, V, None), (h, w)), ((0, ratio, C, 1, None, None), (h * s, w * s)),
                        ((0, C, C, 1, None, "same"), (h * s, w * s))):
        conv_case(B, H, W, cfg, "timed m%d %d->%d r%d idx %s add %s" % cfg + " %dx%d B=%d" % (H, W, B), True)
    n = 16 * 3 * 512 * 1024                                                   # tools/mc_dropout_bench.py
    update_case(n, 3, GUARD, True)
    mean, std, tgt = rand(16, 3, 512, 1024), rand(16, 3, 512, 1024).abs(), rand(16, 3, 512, 1024)
    gaussian_case(mean, std, tgt, torch.rand(512, device="cuda", generator=g) + 0.5, "timed 16x3x512x1024", True)
    del mean, std, tgt
    posembed_case(16, 64, 1024, True)


def main():
    image_cases()
    loss_cases()
    ensemble_cases()
    timed_cases()
    summary("%d of the k > 1 lines also bitwise equal" % multi_equal)


main()
