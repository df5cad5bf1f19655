"""Same-box, same-process A/B of two builds of the resample kernels (csrc/resample.hip):
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/resample_lib_ab.py orbit-2_amd/lib/alt/<name>.so [other.so]
loads the working-tree library (or other.so in its place: an A/A run of two builds of one revision) and the other build (of the
same ABI version: _hip.load) side by side, calls orbit2_resample_fwd and orbit2_resample_moments of both and prints one line per
case, then a summary.  Cases: the size pairs of tests/resample_ref.GPU_CASES in the three plain modes and of
tests/resample_aa_ref.GPU_CASES in the two antialiased ones, their inputs at offsets 0 and 280, channels (4, 0, 2), affine off
and on; the forward output on a 16-byte boundary and 3 floats off it (the whole NaN-guarded buffer is compared), the moments
with latitude weights and climatology off and on against resample_ref.gpu_target.
Rules: a forward is bitwise equal; so are the twelve sums of an image of one tile.  An image of k > 1 tiles adds its workgroups'
partials with double atomics in no fixed order, so two runs of ONE build may differ: there the builds agree within
(k - 1) 2^-52 of the sum of the summands' magnitudes (resample_ref.moments64), the most a reordering of k double additions moves
a sum; the line shows k, the difference and the bound.
Then the shapes of tools/resample_bench.py are compared in the same way and timed, fwd and moments, both builds interleaved: the
median of 5 rounds of 4 launches per build and the relative gap of the medians.  Exit status 1 if a rule is broken."""
import itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]
import numpy as np
import torch
from climate_learn import _hip
from tests import resample_aa_ref as A, resample_ref as R

libs = {"alt": _hip.load(os.path.abspath(sys.argv[1])),
        "tree": _hip.load(os.path.abspath(sys.argv[2])) if len(sys.argv) > 2 else _hip.lib()}
P = lambda t: None if t is None else t.data_ptr()
S = lambda: torch.cuda.current_stream().cuda_stream
dev = lambda v, dtype=np.float32: None if v is None else torch.as_tensor(np.asarray(v, dtype)).cuda()
ok = lambda rc: rc == 0 or sys.exit("rc = %d" % rc)
GUARD = 64
count = {"fwd": [0, 0], "moments, one tile": [0, 0], "moments, several tiles": [0, 0]}        # [lines, lines that pass]
multi_equal = 0


def t(f, n=4):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
med = lambda v: sorted(v)[len(v) // 2]


def timed(run, outs):
    ms = {k: [] for k in libs}
    for _ in range(5):
        for k, lib in libs.items(): ms[k].append(t(lambda: run(lib, outs[k])))
    gap = med(ms["tree"]) / med(ms["alt"]) - 1
    return gap, "   alt %8.4f ms | tree %8.4f ms (%+.1f %%)" % (med(ms["alt"]), med(ms["tree"]), 100 * gap)


def compare(tag, x, idx, HW, code, tiles, scale, shift, target, lat, clim, timing):
    """the lines of one operand set: fwd at two alignments, moments at lat / clim off and on (timing: one of each, timed).
    target, lat, clim: host arrays.  Returns the timed gaps"""
    global multi_equal
    B, Cin, h, w = x.shape
    C, (H, W) = (len(idx) if idx is not None else Cin), HW
    n, k = B * C * H * W, -(-H // tiles[0]) * -(-W // tiles[1])
    sc, sh, ix, tg = dev(scale), dev(shift), dev(idx, np.int32), dev(target)
    gaps = []
    for lead in ((GUARD,) if timing else (GUARD, GUARD - 3)):
        def fwd(lib, o):
            ok(lib.orbit2_resample_fwd(P(x), P(ix), Cin, P(sc), P(sh), o.data_ptr() + 4 * lead, B, C, h, w, H, W, code, S()))
        outs = {name: torch.full((lead + n + GUARD,), float("nan"), device="cuda") for name in libs}
        for name, lib in libs.items(): fwd(lib, outs[name])
        torch.cuda.synchronize()
        eq = torch.equal(outs["tree"].view(torch.int32), outs["alt"].view(torch.int32)) \
            and not bool(torch.isnan(outs["tree"][lead:lead + n]).any())                     # (and the field was written)
        count["fwd"][0] += 1; count["fwd"][1] += eq
        line = "fwd     %s lead %d: bitwise equal %s" % (tag, lead, eq)
        if timing:
            gap, text = timed(fwd, outs); gaps.append((gap, "fwd " + tag)); line += text
        print(line, flush=True)
    field = outs["tree"][lead:lead + n].view(B, C, H, W).cpu().numpy()
    for lw, cl in ([(lat, None)] if timing else itertools.product((None, lat), (None, clim))):
        lwd, cld = dev(lw), dev(cl)
        def mom(lib, o):
            ok(lib.orbit2_resample_moments(P(x), P(ix), Cin, P(sc), P(sh), P(tg), tg.shape[2], tg.shape[3], P(lwd), P(cld), P(o),
                                           B, C, h, w, H, W, code, S()))
        outs = {name: torch.full((B, C, 12), float("nan"), dtype=torch.float64, device="cuda") for name in libs}
        for name, lib in libs.items(): mom(lib, outs[name])
        torch.cuda.synchronize()
        a, b = outs["tree"].cpu().numpy(), outs["alt"].cpu().numpy()
        eq = bool(np.array_equal(a, b)) and bool(np.isfinite(a).all())
        line = "moments %s lat %d clim %d k=%d: bitwise equal %s" % (tag, lw is not None, cl is not None, k, eq)
        if k == 1:
            count["moments, one tile"][0] += 1; count["moments, one tile"][1] += eq
        else:
            bound = (k - 1) * 2.0 ** -52 * R.moments64(field, target, lw, cl)[1]
            within = bool((np.abs(a - b) <= bound).all())
            worst = int(np.argmax(np.abs(a - b) / bound))
            count["moments, several tiles"][0] += 1; count["moments, several tiles"][1] += within; multi_equal += eq
            line += ", largest difference %.3g (bound there %.3g): within %s" % (np.abs(a - b).flat[worst], bound.flat[worst],
                                                                                 within)
        if timing:
            gap, text = timed(mom, outs); gaps.append((gap, "moments " + tag)); line += text
        print(line, flush=True)
    return gaps


def main():
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "resample.npz")))
    plain = [(hw, HW, m, _hip.RESAMPLE_MODES[m], _hip.RESAMPLE_TILE, R.gpu_input(hw, HW, 0.0, golden))
             for hw, HW in R.GPU_CASES for m in R.MODES]
    anti = [(hw, HW, m + "+aa", _hip.RESAMPLE_MODES[m] | _hip.ANTIALIAS, (A.TILE_H, A.TILE_W), A.gpu_input(hw, 0.0))
            for hw, HW in A.GPU_CASES for m in A.MODES]
    for hw, HW, name, code, tiles, x0 in plain + anti:
        for off, aff in itertools.product(R.OFFSETS, (False, True)):
            target, lat, clim = R.gpu_target(HW, off)
            tag = "%-11s %s offset %d affine %d" % (name, R.case_key(hw, HW), off, aff)
            compare(tag, dev(x0 + np.float32(off)), R.GPU_CHANNELS, HW, code, tiles, R.GPU_SCALE if aff else None,
                    R.GPU_SHIFT if aff else None, target, lat, clim, False)
    # the shapes of tools/resample_bench.py
    g = torch.Generator(device="cuda").manual_seed(0)
    gaps = []
    up = torch.randn(16, 23, 128, 256, device="cuda", generator=g)
    down = torch.randn(16, 3, 512, 1024, device="cuda", generator=g)
    for x, idx, HW, modes, aa in [(up, (21, 6, 5), (512, 1024), R.MODES, 0), (down, None, (128, 256), A.MODES, _hip.ANTIALIAS),
                                  (down, None, (64, 128), A.MODES, _hip.ANTIALIAS)]:
        target = torch.randn(16, 3, *HW, device="cuda", generator=g).cpu().numpy()
        lat = (torch.rand(HW[0], device="cuda", generator=g) + 0.5).cpu().numpy()
        for m in modes:
            tag = "%-11s %dx%d-%dx%d" % ((m + "+aa" if aa else m,) + tuple(x.shape[2:]) + HW)
            gaps += compare(tag, x, idx, HW, _hip.RESAMPLE_MODES[m] | aa, (A.TILE_H, A.TILE_W) if aa else _hip.RESAMPLE_TILE,
                            None, None, target, lat, None, True)
    worst = max(gaps, key=lambda v: abs(v[0]))
    print("%d lines; %s; %d of the several-tile lines also bitwise equal; gaps of the medians in percent %s; largest %+.1f %% (%s)"
          % (sum(v[0] for v in count.values()), "; ".join("%s: %d of %d" % (k, v[1], v[0]) for k, v in count.items()),
             multi_equal, " ".join("%+.1f" % (100 * v[0]) for v in gaps), 100 * worst[0], worst[1]))
    sys.exit(any(v[0] != v[1] for v in count.values()))


main()
