"""Same-box, same-process A/B of two builds of the attention kernels:
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/attn_lib_ab.py orbit-2_amd/lib/alt/<name>.so [B]
loads the working-tree library and the other build (of the same ABI version: _hip.load) side by side, checks that forward and backward agree and times
them interleaved (median of 5 rounds of 4 launches) at the interm_1b shape and at d = 64 / d = 256.  The small shapes (no timing)
are the ones of tests/test_hip_ops.py::test_attention_fwd_bwd, each with flags 0, ATTN_4WAVES and ATTN_SPLIT_DKV: together they
reach every instantiation family of the compiler-scheduled kernels (d, waves per workgroup, ragged or not, dropout or not, the
fused and the split dK + dV passes)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]
import torch
from climate_learn import _hip

alt = _hip.load(os.path.abspath(sys.argv[1]))
B = int(sys.argv[2]) if len(sys.argv) > 2 else 4
BF, F32 = torch.bfloat16, torch.float32
P = lambda t: t.data_ptr()
S = lambda: torch.cuda.current_stream().cuda_stream

def fwd(lib, qkv, out, lse, Bx, L, H, d, p, fl=0):
    assert lib.orbit2_attn_fwd_ld(P(qkv), P(out), P(lse), Bx, L, H, d, p, 11, fl, 3 * H * d, H * d, None, None, -1, S()) == 0
def bwd(lib, qkv, out, do, lse, delta, dqkv, Bx, L, H, d, p, fl=0):
    assert lib.orbit2_attn_bwd_ld(P(qkv), P(out), P(do), P(lse), P(delta), P(dqkv), Bx, L, H, d, p, 11, fl, 3 * H * d, H * d, None, None, -1, S()) == 0
def t(f, n=4):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
med = lambda v: sorted(v)[len(v) // 2]
libs = {"tree": _hip.lib(), "alt": alt}
LONG = [(24, 8192, 128, B, 0), (16, 4096, 64, B, 0), (32, 4096, 256, max(1, B // 2), 0), (2, 1024 + 32, 128, 1, 0)]
SMALL = [(2, L, d, 2, fl) for d, Ls in ((64, (128, 512, 578)), (128, (70, 200, 256, 300)), (256, (128, 161))) for L in Ls
         for fl in (0, _hip.ATTN_4WAVES, _hip.ATTN_SPLIT_DKV)]
for (H, L, d, Bx, flg) in LONG + SMALL:
    qkv = (torch.randn(Bx, L, 3 * H * d, device="cuda") * 0.7).to(BF)
    do = torch.randn(Bx, L, H * d, device="cuda").to(BF)
    for p in (0.0, 0.1):
        r = {}
        for k, lib in libs.items():
            out = torch.empty(Bx, L, H * d, dtype=BF, device="cuda"); lse = torch.empty(Bx, H, L, dtype=F32, device="cuda")
            delta = torch.empty(2 * Bx * H * ((L + 63) // 64 * 64 + 64), dtype=F32, device="cuda"); dqkv = torch.empty_like(qkv)   # >= orbit2_attn_bwd_ws_floats
            fwd(lib, qkv, out, lse, Bx, L, H, d, p, flg); bwd(lib, qkv, out, do, lse, delta, dqkv, Bx, L, H, d, p, flg)
            r[k] = (out, lse, delta, dqkv)
        torch.cuda.synchronize()
        eq = [torch.equal(a, b) for a, b in zip(r["tree"], r["alt"])]
        dev = max((a.float() - b.float()).abs().max().item() for a, b in zip(r["tree"], r["alt"]))
        line = "H=%d L=%d d=%d flags=%d p=%.1f: out/lse/delta/dqkv bitwise equal %s, max |diff| %.2e" % (H, L, d, flg, p, eq, dev)
        if L >= 4096:
            tf, tb = {k: [] for k in libs}, {k: [] for k in libs}
            for rnd in range(5):
                for k, lib in libs.items():
                    o, l, dl, dq = r[k]
                    tf[k].append(t(lambda: fwd(lib, qkv, o, l, Bx, L, H, d, p)))
                    tb[k].append(t(lambda: bwd(lib, qkv, o, do, l, dl, dq, Bx, L, H, d, p)))
            gf = 4.0 * Bx * H * L * L * d / 1e9
            line += "\n   fwd: alt %7.3f ms %5.0f TF | tree %7.3f ms %5.0f TF (%+.1f %%)   bwd: alt %7.3f ms %5.0f TF | tree %7.3f ms %5.0f TF (%+.1f %%)" % (
                med(tf["alt"]), gf / med(tf["alt"]), med(tf["tree"]), gf / med(tf["tree"]), 100 * (med(tf["alt"]) / med(tf["tree"]) - 1),
                med(tb["alt"]), 2 * gf / med(tb["alt"]), med(tb["tree"]), 2 * gf / med(tb["tree"]), 100 * (med(tb["alt"]) / med(tb["tree"]) - 1))
        print(line, flush=True)
