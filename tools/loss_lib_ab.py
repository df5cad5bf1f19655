"""Same-box, same-process A/B of two builds of the loss kernels (csrc/ssim.hip, csrc/lpips.hip):
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/loss_lib_ab.py orbit-2_amd/lib/alt/<name>.so [other.so]
loads the working-tree library (or other.so in its place: an A/A run of two builds of one revision) and the other build (of the
same ABI version: _hip.load) side by side (tools/lib_ab.py: the loading, the guarded buffers, the timing and the summary), calls every entry of the two files in both and prints one line per case, then a summary.
Cases, all taken from the test modules:
  orbit2_ssim (sums and map)   tests/test_ssim_gpu.py's 7 x 7, the two thin bands, 39 x 71 against a 41 x 72 target and the four seam
                               shapes, at offsets 0 and 280, lat_w off and on, the range found and given;
  the SSIM VJP                 tests/ssim_loss_ref.GPU_CASES with GPU_COEF and GPU_RANGE, lat_w off and on, as they are and with one
                               coefficient 0, the output on a 16-byte boundary and 3 floats off it;
  the nine entries of lpips.hip  on tests/lpips_ref's COL_SIZES, POOL_SIZES, CONV1_SIZES, BATCHES, CHANNELS, TAP_CHANNELS, TAP_SWITCH,
                               L1_SIZES and one TAP_TRIP pair, act / tapg off and on, gscale None and a device scalar, inputs from
                               lpips_ref's generators; both workspace queries.
Rules: every destination lies inside a NaN-filled buffer with a guard band on either side and the whole buffer is compared.  Every
output of lpips.hip, the SSIM map, the VJP field and sums[3..5] are bitwise equal; so are sums[0..2] of an image of one tile.  An
image of k > 1 tiles adds its workgroups' partials with double atomics in no fixed order, so two runs of ONE build may differ:
there the builds agree within (k - 1) 2^-52 of the sum of the summands' magnitudes (from the float64 oracle
test_ssim_gpu.ssim_oracle: sum |s|, sum |w s|, sum d^2), the most a reordering of k double additions moves a sum; the line shows
k, the difference and the bound.
Then the kernels are timed one by one, both builds interleaved, the median of 5 rounds of 4 launches per build and the relative
gap of the medians: orbit2_ssim (sums; sums + map) and the VJP at tools/ssim_bench.py's [16, 3, 512, 1024]; every kernel of
lpips.hip at the largest VGG stage it serves for sixteen [3, 128, 256] images (8 predictions + 8 targets).  The timed lines are compared by the same rules (at [16, 3, 512, 1024], where the float64 oracle
would take minutes, the magnitudes come from the working-tree build's own sums and map).  Exit status 1 if a rule is broken."""
import itertools
import numpy as np
import torch
from lib_ab import GUARD, P, S, _hip, bitwise, count, guarded, libs, ok, summary, tally
from tests import lpips_ref as L, ssim_loss_ref as V, test_ssim_gpu as TS

dev = lambda v, dtype=np.float32: None if v is None else torch.as_tensor(np.asarray(v, dtype)).cuda()
bf = lambda t: None if t is None else t.to(torch.bfloat16).cuda()
multi_equal = 0


# ---- csrc/ssim.hip ---------------------------------------------------------------------------------------------------------------
def ssim_case(tag, pred, target, lat, rng, oracle, timing=False, with_map=True):
    """pred, target: device tensors; lat, rng: device tensors or None; oracle: () -> (sums64, map64), asked only at k > 1"""
    global multi_equal
    B, C, H, W = pred.shape
    th, tw = _hip.SSIM_TILE
    k, nm = -(-(H - 6) // th) * -(-(W - 6) // tw), B * C * (H - 6) * (W - 6) if with_map else 0
    sums, maps = guarded(B * C * 6, torch.float64), guarded(nm, torch.float32)

    def run(lib, key):
        ok(lib.orbit2_ssim(P(pred), P(target), target.shape[2], target.shape[3], P(lat), P(rng), sums[key].data_ptr() + 8 * GUARD,
                           maps[key].data_ptr() + 4 * GUARD if with_map else None, B, C, H, W, S()))
    for key, lib in libs.items(): run(lib, key)
    torch.cuda.synchronize()
    a, b = sums["tree"].cpu().numpy(), sums["alt"].cpu().numpy()
    body = np.zeros(a.shape, bool)
    body[GUARD:GUARD + B * C * 6] = (np.arange(B * C * 6) % 6) < 3                       # sums[0..2] of every image
    fixed = np.array_equal(a.view(np.int64)[~body], b.view(np.int64)[~body]) and bool(np.isfinite(a[GUARD:GUARD + B * C * 6]).all()) \
        and torch.equal(maps["tree"].view(torch.int32), maps["alt"].view(torch.int32)) \
        and not bool(torch.isnan(maps["tree"][GUARD:GUARD + nm]).any())
    a3, b3 = a[body].reshape(B, C, 3), b[body].reshape(B, C, 3)
    eq = bool(np.array_equal(a3, b3))
    line = "ssim      %s k=%d: map, sums[3..5] and guards bitwise equal %s, sums[0..2] bitwise equal %s" % (tag, k, fixed, eq)
    if k == 1:
        kind, passed = "ssim, one tile", fixed and eq
    else:
        s64, m64 = oracle()
        w = np.ones(H) if lat is None else lat.cpu().numpy().astype(np.float64)[:H]
        mag = np.stack([np.abs(m64).sum((2, 3)), (w[3:H - 3, None] * np.abs(m64)).sum((2, 3)), s64[..., 2]], -1)
        bound = (k - 1) * 2.0 ** -52 * mag
        within = bool((np.abs(a3 - b3) <= bound).all())
        worst = int(np.argmax(np.abs(a3 - b3) / bound))
        kind, passed = "ssim, several tiles", fixed and within
        multi_equal += eq
        line += ", largest difference %.3g (bound there %.3g): within %s" % (np.abs(a3 - b3).flat[worst], bound.flat[worst], within)
    tally(kind, line, passed, run if timing else None, {key: key for key in libs})


def ssim_cases():
    shapes = [((1, 1, 7, 7), None), ((1, 1, 9, 150), None), ((1, 1, 150, 9), None), ((2, 3, 39, 71), (2, 3, 41, 72))]
    th, tw = _hip.SSIM_TILE
    shapes += [((1, 1, ny * th + 6 + e, nx * tw + 6 + e), None) for ny, nx, e in ((1, 1, 0), (1, 1, 1), (2, 2, 0), (2, 2, 1))]
    for (shape, tshape), off, lat_on, rng_on in itertools.product(shapes, (0.0, 280.0), (False, True), (False, True)):
        pred, target = TS.make_fields(shape, tshape, off, seed=3)
        lat = np.linspace(0.5, 1.5, shape[2]).astype(np.float32) if lat_on else None
        rng = np.linspace(4.0, 9.0, shape[0] * shape[1]).astype(np.float32) if rng_on else None
        oracle = lambda: TS.ssim_oracle(pred, target, lat, None if rng is None else rng.reshape(shape[:2]))
        tag = "%dx%dx%dx%d offset %d lat_w %d range given %d" % (shape + (off, lat_on, rng_on))
        ssim_case(tag, dev(pred), dev(target), dev(lat), dev(rng), oracle)


def vjp_call(pred, target, lat, gscale):
    B, C, H, W = pred.shape
    return lambda lib, out: lib.orbit2_loss_bwd(P(pred), P(target), target.shape[2], target.shape[3], P(lat), None, P(gscale), out,
                                                B, C, H, W, _hip.LOSS_SSIM_VJP, S())


def vjp_cases():
    zero = [list(r) for r in V.GPU_COEF]
    zero[0][1] = 0.0
    for hw, thw, offsets in V.GPU_CASES:
        for off, lat_on, (cname, coef), lead in itertools.product(offsets, (False, True), (("as given", V.GPU_COEF), ("one zero", zero)),
                                                                  (GUARD, GUARD - 3)):
            ph, th = V.make_pair(hw, thw, off)
            gscale = torch.stack((dev(coef), dev(V.GPU_RANGE))).contiguous()
            tag = "%dx%d offset %d lat_w %d coef %s lead %d" % (hw + (off, lat_on, cname, lead))
            bitwise("ssim vjp", tag, vjp_call(dev(ph), dev(th), dev(V.lat_weights(hw[0])) if lat_on else None, gscale),
                    ph.size, torch.float32, lead)


# ---- csrc/lpips.hip ----------------------------------------------------------------------------------------------------------------
BFT, F32 = torch.bfloat16, torch.float32


def col_case(N, H, W, C, x, dcol, act, tapg, timing=False):
    """im2col, and col2im plain / act / act + tapg, on device tensors"""
    tag = "N=%d %dx%d C=%d" % (N, H, W, C)
    bitwise("im2col", tag, lambda lib, o: lib.orbit2_im2col3x3(P(x), o, N, H, W, C, S()), N * H * W * 9 * C, BFT, timing=timing)
    for form, a, g in (("plain", None, None), ("act", act, None), ("act+tapg", act, tapg))[2 if timing else 0:]:
        bitwise("col2im", tag + " " + form, lambda lib, o: lib.orbit2_col2im3x3(P(dcol), P(a), P(g), o, N, H, W, C, S()),
                N * H * W * C, BFT, timing=timing)


def pool_case(N, H, W, C, x, gy, tapg, timing=False):
    tag = "N=%d %dx%d C=%d" % (N, H, W, C)
    bitwise("pool fwd", tag, lambda lib, o: lib.orbit2_maxpool2_fwd(P(x), o, N, H, W, C, S()), N * (H // 2) * (W // 2) * C, BFT,
            timing=timing)
    for g in (None, tapg)[1 if timing else 0:]:
        bitwise("pool bwd", tag + " tapg %d" % (g is not None), lambda lib, o: lib.orbit2_maxpool2_bwd(P(gy), P(x), P(g), o, N, H, W, C, S()),
                N * H * W * C, BFT, timing=timing)


def conv1_case(N, H, W, img, pred, target, dz, w1, b1, gs, timing=False):
    tag = "N=%d %dx%d" % (N, H, W)
    bitwise("conv1 fwd", tag, lambda lib, o: lib.orbit2_lpips_conv1_fwd(P(img), P(w1), P(b1), o, N, H, W, S()), N * H * W * 64, BFT,
            timing=timing)
    for g in (None, gs)[1 if timing else 0:]:
        bitwise("conv1 bwd", tag + " gscale %d" % (g is not None),
                lambda lib, o: lib.orbit2_lpips_conv1_bwd(P(dz), P(w1), P(pred), P(target), 0.0234375, P(g), o, N, H, W, S()),
                N * 3 * H * W, F32, timing=timing)


def ws_of(kind, query, *args):
    """the workspace of a two-stage sum: the query of both builds agrees (part of the rules), one buffer per build"""
    n = {k: getattr(lib, query)(*args) for k, lib in libs.items()}
    count.setdefault(kind, [0, 0])
    count[kind][0] += 1; count[kind][1] += n["tree"] == n["alt"] > 0
    if not n["tree"] == n["alt"] > 0: print("%s%r: tree %d, alt %d" % (query, args, n["tree"], n["alt"]), flush=True)
    return {id(lib): torch.empty(max(n[k], 1), device="cuda") for k, lib in libs.items()}


def tap_case(C, HW, B, f, lin, gs, timing=False):
    tag = "C=%d HW=%d B=%d" % (C, HW, B)
    ws = ws_of("workspace queries", "orbit2_lpips_tap_ws_floats", B, HW, C)
    bitwise("tap fwd", tag, lambda lib, o: lib.orbit2_lpips_tap_fwd(P(f), P(lin), o, B, HW, C, P(ws[id(lib)]), S()), B, F32,
            prefill=0.0 if timing else L.L1_PREFILL, timing=timing)             # (timed: val is added to on every launch)
    for g in (None, gs)[1 if timing else 0:]:
        bitwise("tap bwd", tag + " gscale %d" % (g is not None),
                lambda lib, o: lib.orbit2_lpips_tap_bwd(P(f), P(lin), o, L.TAP_COEF, P(g), B, HW, C, S()), B * HW * C, BFT, timing=timing)


def l1_case(n, a, b, timing=False):
    ws = ws_of("workspace queries", "orbit2_l1_mean_ws_floats", n)
    bitwise("l1 mean", "n=%d" % n, lambda lib, o: lib.orbit2_l1_mean(P(a), P(b), o, n, P(ws[id(lib)]), S()), 1, F32,
            prefill=0.0 if timing else L.L1_PREFILL, timing=timing)


def lpips_cases():
    gs = torch.tensor([L.GSCALE]).cuda()
    for N, C in itertools.product(L.BATCHES, L.CHANNELS):
        for H, W in L.COL_SIZES:
            col_case(N, H, W, C, *(bf(v) for v in L.col_inputs(N, H, W, C, False)))
        for H, W in L.POOL_SIZES:
            pool_case(N, H, W, C, *(bf(v) for v in L.pool_inputs(N, H, W, C)))
    w1, b1 = (v.cuda() for v in L.conv1_weights())
    for N, (H, W) in itertools.product(L.BATCHES, L.CONV1_SIZES):
        img, pred, target, _, dz = L.conv1_inputs(N, H, W)
        conv1_case(N, H, W, img.cuda(), pred.cuda(), target.cuda(), bf(dz), w1, b1, gs)
    taps = [(C, HW, B) for C in L.TAP_CHANNELS for HW in L.tap_hws(C) for B in L.BATCHES] + [(C, HW, 1) for C, HW in L.TAP_SWITCH + L.TAP_TRIP[:1]]
    for C, HW, B in taps:
        f, lin = L.tap_inputs(C, HW, B)
        tap_case(C, HW, B, bf(f), lin.cuda(), gs)
    for n in L.L1_SIZES:
        l1_case(n, *(v.cuda() for v in L.l1_inputs(n)))


# ---- every kernel alone, timed ---------------------------------------------------------------------------------------------------------
def timed_cases():
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    B, C, H, W = 16, 3, 512, 1024                                                # tools/ssim_bench.py
    yy, xx = torch.arange(H, device="cuda").view(1, 1, H, 1) / 37.0, torch.arange(W, device="cuda").view(1, 1, 1, W) / 53.0
    phase = torch.rand(B, C, 1, 1, device="cuda", generator=g) * 6.28
    target = 280.0 + 2.0 * torch.sin(yy + phase) + 1.5 * torch.cos(xx - phase) + 0.1 * rand(B, C, H, W)
    pred = target + 0.3 * rand(B, C, H, W)
    lat = torch.rand(H, device="cuda", generator=g) + 0.5
    def oracle(memo=[]):
        """at this size the float64 oracle takes minutes: the magnitudes come from the working-tree build's own sums and map, which
        the tests hold within 1e-5 of the oracle per pixel"""
        if not memo:
            s, m = _hip.ssim_sums(pred, target, lat, ssim_map=True)
            memo.append((s.cpu().numpy(), m.double().cpu().numpy()))
        return memo[0]
    ssim_case("16x3x512x1024 sums", pred, target, lat, None, oracle, timing=True, with_map=False)
    ssim_case("16x3x512x1024 sums + map", pred, target, lat, None, oracle, timing=True)
    gscale = torch.stack((torch.rand(B, C, device="cuda", generator=g) + 0.5, torch.full((B, C), 7.0, device="cuda"))).contiguous()
    bitwise("ssim vjp", "16x3x512x1024", vjp_call(pred, target, lat, gscale), pred.numel(), torch.float32, timing=True)
    del pred, target
    N, H, W = 16, 128, 256                                                       # 8 predictions + 8 targets of [3, 128, 256]
    gs = torch.tensor([L.GSCALE]).cuda()
    act = lambda *shape: torch.relu(rand(*shape)).to(BFT)
    col_case(N, H, W, 64, act(N * H * W, 64), rand(N * H * W, 9 * 64).to(BFT), act(N * H * W, 64), rand(N * H * W, 64).to(BFT), True)
    pool_case(N, H, W, 64, act(N * H * W, 64), rand(N * (H // 2) * (W // 2), 64).to(BFT), rand(N * H * W, 64).to(BFT), True)
    w1, b1 = (v.cuda() for v in L.conv1_weights())
    img = rand(N, 3, H, W) * 0.6
    conv1_case(N, H, W, img, img[:8].repeat(2, 1, 1, 1), img[8:].repeat(2, 1, 1, 1), rand(N * H * W, 64).to(BFT), w1, b1, gs, True)
    for Ct, HW in ((64, H * W), (512, (H // 8) * (W // 8))):                     # relu1_2 and relu4_3
        tap_case(Ct, HW, N // 2, act(N, HW, Ct), torch.rand(Ct, device="cuda", generator=g) * (2.0 / Ct), gs, True)
    l1_case(8 * 3 * H * W, rand(8 * 3 * H * W), rand(8 * 3 * H * W), True)


def main():
    ssim_cases()
    vjp_cases()
    lpips_cases()
    timed_cases()
    summary("%d of the several-tile lines also bitwise equal" % multi_equal)


main()
