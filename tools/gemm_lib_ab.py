"""Same-box, same-process A/B of two builds of the GEMM kernels (csrc/gemm.hip):
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/gemm_lib_ab.py orbit-2_amd/lib/alt/<name>.so [other.so]
tools/lib_ab.py loads the two builds, keeps the guarded buffers, times and sums up; this file calls orbit2_gemm_bf16, its grouped
entry and orbit2_sgemm_f32_ws in both so that every kernel instantiation of the file runs, at the smallest shapes that reach it:
  single launches, all four operand forms: the 128-tile kernel (hint 128) on ragged M, N and K, its 64-row form (hint 64, A
    K-contiguous), the 8-phase kernel (hint 256) on ragged M and N, the 4-wave kernel (hint 260) on whole tiles: plain, fp32
    output, beta = 1, the three compile-time epilogue kinds in their forms (kind 3 with colsum_ws), the same options under the
    runtime epilogue (hint 262), the path gate with some entries 0.0 (zeros; the residual rows), and the tail-queue twin of each;
  grouped launches, all four forms: hint 128 and hint 256 on the first problem (ragged tiles, a beta = 1 member), whole tiles on
    the 4-wave kernel, its weight-gradient form with a K gate, and the tail-queue twin of each 4-wave group;
  the three fp32 kernels with the split-K combine, and a dropout epilogue under a seed salt.
Every output and every side output (save_pre, save_dact, colsum_ws) must be bitwise equal, guard bands included.
Then the Block's GEMMs at the interm_1b size (M = 65536 tokens, D = 3072) are timed, both builds interleaved: the forward GEMMs
with their epilogues, the input gradients, the grouped weight gradients (4-wave kernels), and one line per other family: the
128-tile kernel, its 64-row form, the 8-phase kernel single and grouped, the 128-tile group.  Exit status 1 if a line differs."""
import ctypes as C
import torch
from lib_ab import BITS, GUARD, P, S, guarded, libs, ok, summary, tally
from climate_learn import _hip

BF, F32, I16 = torch.bfloat16, torch.float32, torch.int16
gen = torch.Generator(device="cuda").manual_seed(1)
rnd = lambda *s: (torch.randn(*s, device="cuda", generator=gen) * 0.5).to(BF)
FORMS = ("nt", "nn", "tn", "tt")
kc = lambda form: (form[0] == "n", form[1] == "t")


def compare(kind, tag, call, dests, timing=False):
    """call(lib, one tensor per destination) in both builds.  dests: (elements, dtype, prefill or None, must be written); every
    buffer whole, bit for bit"""
    G = [guarded(n, dtype, prefill=pre) for n, dtype, pre, _ in dests]
    run = lambda lib, key: call(lib, *[g[key][GUARD:GUARD + d[0]] for g, d in zip(G, dests)])
    for key, lib in libs.items(): run(lib, key)
    torch.cuda.synchronize()
    eq = all(torch.equal(g["tree"].view(BITS[d[1]]), g["alt"].view(BITS[d[1]])) for g, d in zip(G, dests)) \
        and not any(d[3] and bool(torch.isnan(g["tree"][GUARD:GUARD + d[0]]).any()) for g, d in zip(G, dests))
    tally(kind, "%-14s %s: bitwise equal %s" % (kind, tag, eq), eq, run if timing else None, {key: key for key in libs})


def operands(form, M, N, K):
    a_kc, b_kc = kc(form)
    return rnd(M, K) if a_kc else rnd(K, M), rnd(N, K) if b_kc else rnd(K, N)


def single(kind, form, M, N, K, tile, out=BF, timing=False, tail=-1, gate=None, opts=(), **kw):
    """one orbit2_gemm_bf16 call.  opts: names of the operands the epilogue takes (bias, residual, rowscale, mul: inputs made here;
    save_pre, save_dact, colsum: side outputs, compared); gate: the path gate's entries, one per 256 rows (with a residual the row
    scale is the gate); tail: tiles by ticket"""
    a_kc, b_kc = kc(form)
    A, B = operands(form, M, N, K)
    bias = rnd(N) if "bias" in opts else None
    res = rnd(M, N) if "residual" in opts else None
    mul = torch.randint(-16384, 16384, (M, N), dtype=I16, device="cuda", generator=gen) if "mul" in opts else None
    gate_t = None if gate is None else torch.tensor(gate, dtype=F32, device="cuda")
    rows = (torch.rand(M // 256, device="cuda", generator=gen) + 0.5) if "rowscale" in opts else None
    rows = gate_t if gate is not None and res is not None else rows
    sides = [o for o in ("save_pre", "save_dact", "colsum") if o in opts]
    dests = [(M * N, out, 0.5 if kw.get("beta") else None, True)]
    dests += [((M // 256) * N, F32, None, True) if o == "colsum" else (M * N, BF, None, o == "save_pre") for o in sides]
    sched = _hip._sched_word(torch.device("cuda", torch.cuda.current_device())) if tail >= 0 else None

    def call(lib, c, *side):
        side = dict(zip(sides, side))
        a = _hip.GemmArgs()
        _hip._gemm_fill(a, A, B, c.view(M, N), M, N, K, A.shape[1], B.shape[1], N, a_kc=a_kc, b_kc=b_kc, bias=bias, residual=res,
                        ldr=N if res is not None else 0, rowscale=rows, rows_per_scale=256 if rows is not None else 0, mul=mul,
                        save_pre=side["save_pre"].view(M, N) if "save_pre" in side else None,
                        save_dact=side["save_dact"].view(I16).view(M, N) if "save_dact" in side else None, tile=tile, seed=5, **kw)
        if "colsum" in side:
            assert lib.orbit2_gemm_bf16_colsum_rows(C.byref(a)) == M // 256
            a.colsum_ws = P(side["colsum"])
        ok(lib.orbit2_gemm_bf16(C.byref(a), P(gate_t), 256 if gate is not None else 0, sched, tail, S()))
    tag = "%s hint %3d %5d x %5d x %5d%s%s%s%s" % (form, tile, M, N, K, " fp32" if out is F32 else "", " tail %d" % tail if tail >= 0 else "",
                                                " gate" if gate is not None else "", "".join(" " + o for o in opts) + "".join(
                                                    " %s=%s" % kv for kv in sorted(kw.items())))
    compare(kind, tag, call, dests, timing)


def grouped(kind, form, shapes, hint=0, timing=False, tail=-1, beta_member=None, kgate=None):
    """one orbit2_gemm_bf16_grouped call over shapes = [(M, N, K)]; the hint goes on the first problem (258: a group too small
    to fill the chip still takes the 256-tile kernels, the 4-wave one when all tiles are whole); kgate: entries of the K
    gate of every problem, one per K / len(kgate) rows of the contraction, the dropped ranges of A zeroed as the entry asks"""
    a_kc, b_kc = kc(form)
    ops = [operands(form, *s) for s in shapes]
    n = len(shapes)
    kg = None if kgate is None else torch.tensor(kgate, dtype=F32, device="cuda")
    if kg is not None:
        for (A, _), (M, N, K) in zip(ops, shapes):
            A.view(len(kgate), K // len(kgate), M)[kg == 0.0] = 0
    sched = _hip._sched_word(torch.device("cuda", torch.cuda.current_device())) if tail >= 0 else None

    def call(lib, *outs):
        arr = (_hip.GemmArgs * n)()
        for i, ((A, B), (M, N, K), c) in enumerate(zip(ops, shapes, outs)):
            _hip._gemm_fill(arr[i], A, B, c.view(M, N), M, N, K, A.shape[1], B.shape[1], N, a_kc=a_kc, b_kc=b_kc,
                            beta=1.0 if i == beta_member else 0.0, tile=hint if i == 0 else 0)
        kgs = (C.c_void_p * n)(*([P(kg)] * n)) if kg is not None else None
        kper = (C.c_int * n)(*[K // len(kgate) for _, _, K in shapes]) if kg is not None else None
        ok(lib.orbit2_gemm_bf16_grouped(arr, n, kgs, kper, sched, tail, S()))
    tag = "%s hint %3d %s%s%s%s" % (form, hint, " ".join("%dx%dx%d" % s for s in shapes), " tail %d" % tail if tail >= 0 else "",
                                  " beta=1 on %d" % beta_member if beta_member is not None else "", " K gate" if kgate else "")
    compare(kind, tag, call, [(M * N, BF, 0.5 if i == beta_member else None, True) for i, (M, N, _) in enumerate(shapes)], timing)


def sgemm(M, N, K):
    A, B = torch.randn(M, K, device="cuda", generator=gen), torch.randn(K, N, device="cuda", generator=gen)
    n = libs["tree"].orbit2_sgemm_f32_ws_floats(M, N, K)
    assert n == libs["alt"].orbit2_sgemm_f32_ws_floats(M, N, K)
    dests = [(M * N, F32, 0.5, True)] + ([(n, F32, None, True)] if n else [])
    compare("fp32", "%d x %d x %d, %d workspace floats" % (M, N, K, n), lambda lib, c, ws=None: ok(lib.orbit2_sgemm_f32_ws(
        P(A), P(B), P(c), M, N, K, K, N, N, 0, 0, 0.75, 1.0, P(ws), n, S())), dests)


FC1 = dict(opts=("bias", "save_dact"), act=1, drop_p=0.1)                            # compile-time kind 1 in the forward form
PROJ = dict(opts=("bias", "residual", "rowscale"), drop_p=0.1)                       # kind 2
DX_FC2 = dict(opts=("mul", "colsum"))                                                # kind 3 in the input-gradient form
W4_GROUP = [(256, 512, 192), (768, 256, 128), (256, 256, 320), (512, 1024, 128)]
RAGGED_GROUP = [(264, 520, 128), (256, 256, 192), (520, 264, 128), (256, 512, 320)]


def equality():
    for form in FORMS:
        single("128-tile", form, 136, 200, 72, 128, opts=("bias", "residual"), act=1)
        single("128-tile", form, 520, 776, 192, 128, out=F32)
        single("8-phase", form, 520, 776, 192, 256, opts=("bias", "save_pre"), act=1, drop_p=0.1)
        single("8-phase", form, 264, 520, 128, 256, out=F32, beta=1.0)
        for tail in (-1, 2):
            single("4-wave", form, 512, 768, 192, 260, tail=tail)
        grouped("128 group", form, [(200, 136, 128), (384, 520, 192), (128, 128, 64), (72, 1032, 256)], beta_member=1)
        grouped("128 group", form, W4_GROUP, hint=128)
        grouped("8-phase group", form, RAGGED_GROUP, hint=256, beta_member=2)
        for tail in (-1, 3):
            grouped("4-wave group", form, W4_GROUP, hint=258, tail=tail, beta_member=1)
    for form, M, N, K in (("nt", 72, 136, 200), ("nn", 1000, 384, 200)):
        single("64-row", form, M, N, K, 64, opts=("residual",), act=1)
    single("4-wave", "nt", 512, 768, 192, 260, out=F32, opts=("bias",))
    single("4-wave", "tn", 512, 768, 192, 260, beta=1.0)
    single("4-wave", "nt", 512, 768, 192, 260, opts=("bias",), colscale=(256, 0.125))          # the lean epilogue with both options
    for tail in (-1, 2):
        for tile in (260, 262):                                                              # compiled kinds, then the runtime form
            single("4-wave kinds", "nt", 512, 768, 192, tile, tail=tail, **FC1)
            single("4-wave kinds", "nt", 512, 768, 192, tile, tail=tail, **PROJ)
        single("4-wave kinds", "nn", 512, 768, 192, 260, tail=tail, **DX_FC2)
        single("4-wave kinds", "nn", 512, 768, 192, 262, tail=tail, opts=("mul",))
        single("path gate", "nt", 768, 512, 128, 260, tail=tail, gate=[1.0, 0.0, 1.0], opts=("bias", "save_dact"), act=1)
        single("path gate", "nt", 768, 512, 128, 260, tail=tail, gate=[0.0, 1.5, 0.0], opts=("bias", "residual"), drop_p=0.1)
        grouped("4-wave group", "tn", [(256, 512, 512), (512, 256, 512)], hint=258, tail=tail, kgate=[1.0, 0.0, 0.0, 1.0])
    for M, N, K in ((2048, 1024, 64), (115, 256, 1024), (16, 256, 1024)):
        sgemm(M, N, K)
    for lib in libs.values(): ok(lib.orbit2_seed_salt(0x9E3779B97F4A7C15, 0, S()))
    single("seed salt", "nt", 136, 200, 72, 128, opts=("bias",), drop_p=0.25)
    for lib in libs.values(): ok(lib.orbit2_seed_salt(0, 0, S()))


def timing():
    M, D = 65536, 3072
    for N, K, kw in ((3 * D, D, dict(opts=("bias",))), (D, D, PROJ), (4 * D, D, dict(opts=("bias", "save_pre"), act=1, drop_p=0.1)),
                     (4 * D, D, FC1), (D, 4 * D, PROJ)):
        single("timed fwd", "nt", M, N, K, 0, timing=True, **kw)
    for N, K in ((D, 3 * D), (D, 4 * D), (4 * D, D)):
        single("timed dX", "nn", M, N, K, 0, timing=True)
    DW = [(3 * D, D, M), (D, D, M), (4 * D, D, M), (D, 4 * D, M)]
    grouped("timed dW", "tn", DW, timing=True)
    for form in ("nt", "tn"):
        single("timed 128", form, *((M, D, D) if form == "nt" else (D, D, M)), 128, timing=True)
        single("timed 8-phase", form, *((M, D, D) if form == "nt" else (D, D, M)), 256, timing=True)
    for form in ("nt", "nn"):
        single("timed 64-row", form, M, D, D, 64, timing=True)
    grouped("timed 8-ph grp", "tn", DW, hint=256, timing=True)
    grouped("timed 128 grp", "tn", DW, hint=128, timing=True)


if __name__ == "__main__":
    equality()
    timing()
    summary()
