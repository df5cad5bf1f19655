"""Same-box, same-process A/B of two builds of the LayerNorm / element kernels (csrc/norm_elem.hip):
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/elem_lib_ab.py orbit-2_amd/lib/alt/<name>.so [other.so]
loads the working-tree library (or other.so in its place: an A/A run of two builds of one revision) and the other build (of the
same ABI version: _hip.load) side by side, runs layernorm_fwd_ld, layernorm_bwd, dropout_bwd, dropout_bwd_colsum, post_reduce,
colsum and batch_sum through both and prints, per case, whether every output is bitwise equal.  The small shapes (no timing) are
the (D, rows) pairs of tests/test_hip_ops.py::test_layernorm crossed with p in {0, 0.1}, row scale on / off, beta in {0, 1} and
fp32 / bf16 sinks: every form and partition of the LayerNorm backward, both column-sum partitions.  The rows x D of the four
configurations of tests/test_dispatch_cpu.py:CONFIGS (hidden width 4 D for the colsum / dropout legs) are also timed,
interleaved: the median of 5 rounds of 4 launches per build and their relative gap.  The last line sums up."""
import itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]
import torch
from climate_learn import _hip

libs = {"alt": _hip.load(os.path.abspath(sys.argv[1])),
        "tree": _hip.load(os.path.abspath(sys.argv[2])) if len(sys.argv) > 2 else _hip.lib()}
BF, F32 = torch.bfloat16, torch.float32
P = lambda t: None if t is None else t.data_ptr()
S = lambda: torch.cuda.current_stream().cuda_stream
rnd = lambda *shape, dtype=BF: torch.randn(*shape, device="cuda", dtype=dtype)
empty = lambda *shape, dtype=BF: torch.empty(*shape, device="cuda", dtype=dtype)
SEED = (1 << 40) + 12345


def t(f, n=4):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
med = lambda v: sorted(v)[len(v) // 2]


def cases(rows, D, wide, p, scaled, beta, fp32):
    """(name, run(lib, outs), fresh outs) for one shape and one setting; wide: the hidden width of the colsum / dropout legs.
    A sink that is accumulated into (beta = 1) starts from the same values for both builds; a workspace, always the last of the
    outs and written only in part, is not compared."""
    sink = F32 if fp32 else BF
    rps = (rows + 7) // 8
    scale = (torch.rand(8, device="cuda") * 2).float() if scaled else None
    x, dy, g, b = rnd(rows, D), rnd(rows, D), rnd(D), rnd(D)
    mean, rstd = x.float().mean(1), (x.float().var(1, unbiased=False) + 1e-5).rsqrt()
    dres = rnd(rows, D) if scaled else None                   # (the residual-stream gradient rides on the same switch)
    sink0 = {n: rnd(n, dtype=sink) for n in (D, wide, rows // 8 * D)}
    xw, add = rnd(rows, wide), rnd(rps, D)
    xw32 = xw.float() if fp32 else None
    ok = lambda rc: rc == 0 or sys.exit("rc = %d" % rc)

    def ln_fwd(lib, o):
        ok(lib.orbit2_layernorm_fwd_ld(P(x), P(g), P(b), P(o[0]), P(o[1]), P(o[2]), rows, D, D, 1e-5, S()))
    yield "layernorm_fwd_ld", ln_fwd, lambda: [empty(rows, D), empty(rows, dtype=F32), empty(rows, dtype=F32)]
    nws = libs["tree"].orbit2_layernorm_bwd_ws_floats(rows, D)

    def ln_bwd(lib, o):
        ok(lib.orbit2_layernorm_bwd(P(dy), P(x), P(g), P(mean), P(rstd), P(dres), P(o[0]), P(o[1]), P(o[2]), int(fp32), beta,
                                    P(o[3]), nws, rows, D, S()))
    yield "layernorm_bwd", ln_bwd, lambda: [empty(rows, D), sink0[D].clone(), sink0[D].flip(0).clone(), empty(nws, dtype=F32)]

    def drop(lib, o):
        ok(lib.orbit2_dropout_bwd(P(xw), P(o[0]), rows, wide, p, SEED, P(scale), rps, S()))
    yield "dropout_bwd", drop, lambda: [empty(rows, wide)]
    cws = libs["tree"].orbit2_colsum_ws_floats(rows, wide)

    def drop_cs(lib, o):
        ok(lib.orbit2_dropout_bwd_colsum(P(xw), P(o[0]), rows, wide, p, SEED, P(scale), rps, P(o[1]), int(fp32), beta, P(o[2]), cws, S()))
    yield "dropout_bwd_colsum", drop_cs, lambda: [empty(rows, wide), sink0[wide].clone(), empty(cws, dtype=F32)]

    def post(lib, o):
        ok(lib.orbit2_post_reduce(P(x), P(add), rps, P(dy), P(o[0]), rows, D, p, SEED, P(scale), rps, S()))
    yield "post_reduce", post, lambda: [empty(rows, D)]

    def colsum(lib, o):                                       # (the fp32 sink setting also sums the fp32 input)
        src = xw32 if fp32 else xw
        ok(lib.orbit2_colsum(P(src), int(fp32), rows, wide, wide, P(o[0]), int(fp32), beta, P(o[1]), cws, S()))
    yield "colsum", colsum, lambda: [sink0[wide].clone(), empty(cws, dtype=F32)]
    if rows >= 8:
        def bsum(lib, o):
            ok(lib.orbit2_batch_sum(P(x), P(o[0]), 8, rows // 8, D, int(fp32), beta, S()))
        yield "batch_sum", bsum, lambda: [sink0[rows // 8 * D].clone()]


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_dispatch_cpu import CONFIGS
    timed = [(B * (h // 2) * (w // 2), D) for D, _, B, (h, w) in CONFIGS.values()]
    small = [(200, D) for D in (64, 256, 1024, 3072, 5120, 8192)] + [(33000, D) for D in (256, 1024, 3072, 2048)]
    settings = list(itertools.product((0.0, 0.1), (False, True), (0.0, 1.0), (False, True)))
    lines = unequal = 0
    worst = (0.0, "")
    for (rows, D), timing in [(s, False) for s in small] + [(s, True) for s in timed]:
        wide = 4 * D if timing else D                        # (the small shapes keep the test's widths on every leg)
        for p, scaled, beta, fp32 in (settings if not timing else [(0.1, True, 0.0, True), (0.0, False, 1.0, False)]):
            for name, run, fresh in cases(rows, D, wide, p, scaled, beta, fp32):
                outs = {k: fresh() for k in libs}
                for k, lib in libs.items(): run(lib, outs[k])
                torch.cuda.synchronize()
                n = len(outs["tree"]) - (name in ("layernorm_bwd", "dropout_bwd_colsum", "colsum"))      # without the workspace
                eq = [torch.equal(a, b) for a, b in zip(outs["tree"][:n], outs["alt"][:n])]
                lines += 1; unequal += not all(eq)
                line = "%-19s rows=%d D=%d wide=%d p=%.1f scale/dres=%d beta=%g fp32=%d: bitwise equal %s" % (
                    name, rows, D, wide, p, scaled, beta, fp32, eq)
                if timing:
                    ms = {k: [] for k in libs}
                    for _ in range(5):
                        for k, lib in libs.items(): ms[k].append(t(lambda: run(lib, outs[k])))
                    gap = med(ms["tree"]) / med(ms["alt"]) - 1
                    if abs(gap) > abs(worst[0]): worst = (gap, "%s rows=%d D=%d" % (name, rows, D))
                    line += "   alt %8.4f ms | tree %8.4f ms (%+.1f %%)" % (med(ms["alt"]), med(ms["tree"]), 100 * gap)
                print(line, flush=True)
                del outs
    print("%d lines, %d not bitwise equal; largest gap of the medians %+.1f %% (%s)" % (lines, unequal, 100 * worst[0], worst[1]))


main()
