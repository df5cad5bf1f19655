"""Tail-queue diagnostic (-DO2_TQ_TRACE build: tools/mkvar_tq_trace.sh): what does a static launch of the one-workgroup-per-CU kernels
lose at its end, and what does the tail queue get back?  At the bench shapes (interm_1b, batch 16, 128 x 256), per kernel family,
static and queued: per XCD (the XCC id register, checked against b & 7) the time its last workgroup ends before the kernel's end, the
idle share of the chip at the launch's end (mean of those over the kernel's span), the span, and how many tail tiles each XCD drew.

    python tools/tail_idle.py [--quick] [--tails=0,1024,...]     # --quick: a quarter of the tokens; --tails: tail sizes in tiles"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]
import torch
from climate_learn import _hip
_hip.LIB_PATH = os.environ.get("ORBIT2_TRACE_LIB", os.path.join(ROOT, "orbit-2_amd", "lib", "alt", "tqtrace.so"))
from climate_learn import _ops

BF, F32 = torch.bfloat16, torch.float32
QUICK = "--quick" in sys.argv
D, H, d, B, L = 3072, 24, 128, (4 if QUICK else 16), 8192
T = B * L
WGS = 65536
g = torch.Generator(device="cuda").manual_seed(1)
r = lambda *s: (torch.randn(*s, device="cuda", generator=g) * 0.5).to(BF)


def read(reader, base, n):
    buf = (C.c_ulonglong * (3 * WGS))()
    assert getattr(_hip.lib(), reader)(buf, 3 * WGS) == 0
    return [(buf[3 * (base + b)], buf[3 * (base + b) + 1], buf[3 * (base + b) + 2] & 15) for b in range(n)]


def report(name, mode, rec, S):
    """rec: (start, end, xcc) per workgroup of the grid; S: workgroups that walked statically (the rest drew tickets)"""
    n = len(rec)
    t0, t1 = min(s for s, _, _ in rec), max(e for _, e, _ in rec)
    by_res = [sorted({rec[b][2] for b in range(x, n, 8)}) for x in range(8)]
    fixed = all(len(v) == 1 for v in by_res) and len({v[0] for v in by_res}) == 8
    ends = [max(rec[b][1] for b in range(x, n, 8)) for x in range(8)]
    idle = 100.0 * sum(t1 - e for e in ends) / 8 / (t1 - t0)
    # a ticket holder that got a tile ran for far longer than one that returned at once
    drew = [sum(1 for b in range(S + ((x - S) % 8), n, 8) if rec[b][1] - rec[b][0] > 300) for x in range(8)] if S < n else None
    print("%-22s %-6s %6d wgs  span %9.1f us  idle at end %5.2f %%  XCD last end before kernel end [us]: %s%s%s"
          % (name, mode, n, (t1 - t0) / 100.0, idle, " ".join("%6.1f" % ((t1 - e) / 100.0) for e in ends),
             "  | tail tiles per XCD: " + " ".join("%3d" % v for v in drew) if drew else "",
             "" if fixed else "  !! XCC ids per b & 7: %s" % by_res), flush=True)
    return (t1 - t0) / 100.0, idle


TAILS = [int(v) for v in next((a.split("=")[1] for a in sys.argv if a.startswith("--tails=")), "0").split(",")]   # 0: the library's own


def both(name, reader, base, tiles, launch, reps=6):
    """launch(tail_queue) -> runs the family.  Static, then queued with each tail of --tails (tiles; 0 = sized by the library): the
    mean time of `reps` launches by events, and the trace of the last one"""
    out = []
    for tail in [None] + TAILS:
        tq = None if tail is None else (True if tail == 0 else tail)
        launch(tq)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch(tq)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / reps
        t = 0 if tail is None else (512 if tail == 0 else tail)
        if t > tiles or (tail == 0 and tiles < 6 * 256):
            t = 0
        mode = "static" if tail is None else "q%d" % t
        span, idle = report(name, mode, read(reader, base, tiles + t), tiles - t)
        out.append((mode, us, idle))
    print("%-22s mean of %d launches [us]: %s" % (name, reps, "  ".join(
        "%s %.1f (%+.2f %%, idle %.2f %%)" % (m, us, 100.0 * (us / out[0][1] - 1.0), idle) for m, us, idle in out)), flush=True)


gate = torch.ones(B, device="cuda", dtype=F32)
gate[B // 2] = 0.0
gate[B - 3] = 0.0
GK = dict(gate=gate, rows_per_gate=L)
ldD, ldq, ldh = _ops._ld_pad(D), _ops._ld_pad(3 * D), _ops._ld_pad(4 * D)
print("# tokens %d; pitches %d %d %d; device %s" % (T, ldD, ldq, ldh, torch.cuda.get_device_name()), flush=True)


def rows(M, N, ld):
    buf = torch.empty(M, ld, dtype=BF, device="cuda")
    buf.copy_(r(M, ld))
    return buf[:, :N]


def gemm_family(name, N, K, b_kc, lda, ldc, gated, **kw):
    A = rows(T, K, lda)
    W = r(N, K) if b_kc else r(K, N)
    o = torch.empty(T, ldc, dtype=BF, device="cuda")[:, :N]
    extra = {}
    if "save_dact" in kw:
        kw = dict(kw)
        kw.pop("save_dact")
        extra["save_dact"] = torch.empty(T, ldc, dtype=torch.int16, device="cuda")[:, :N]
    if "mul" in kw:
        kw = dict(kw)
        kw.pop("mul")
        extra["mul"] = torch.randint(-16384, 16384, (T, ldc), device="cuda", dtype=torch.int16)[:, :N]
    if "residual" in kw:
        kw = dict(kw, residual=r(T, N), ldr=N)
        if gated:
            kw.update(rowscale=gate, rows_per_scale=L)
    tiles = (T // 256) * (N // 256)
    both(name + (" gated" if gated else ""), "orbit2_debug_read_tq_trace_gemm", 0, tiles,
         lambda tq: _hip.gemm(A, W, o, T, N, K, lda, K if b_kc else N, ldc, a_kc=True, b_kc=b_kc, tail_queue=tq,
                              **(GK if gated else {}), **extra, **kw))
    del A, W, o, extra
    torch.cuda.empty_cache()


bias3, bias12, bias9 = r(D), r(4 * D), r(3 * D)
for gated in (False, True):
    gemm_family("NT kind0 qkv", 3 * D, D, True, ldD, ldq, gated, bias=bias9, colscale=(D, 0.1275))
    gemm_family("NT kind1 fc1", 4 * D, D, True, ldD, ldh, gated, bias=bias12, act=1, drop_p=0.1, seed=7, save_dact=True)
    gemm_family("NT kind2 fc2", D, 4 * D, True, ldh, D, gated, bias=bias3, drop_p=0.1, seed=7, residual=True)
    gemm_family("NN kind3 dpre", 4 * D, D, False, D, ldh, gated, mul=True, want_colsum=True)
    gemm_family("NN kind0 dh2", D, 4 * D, False, ldh, D, gated)

# the Block's grouped weight-gradient launch, balanced as _ops._DwBatch.flush does it
shapes = [(D, 4 * D, D, ldh), (4 * D, D, ldh, ldD), (D, D, D, ldD), (3 * D, D, ldq, ldD)]       # (N, K, pitch of dy, pitch of x)
for gated in (False, True):
    probs, keep = [], []
    for N, K, lda, ldb in shapes:
        dy, x = rows(T, N, lda), rows(T, K, ldb)
        if gated:
            dy[(gate == 0).repeat_interleave(L)] = 0
        kw = dict(a_kc=False, b_kc=False)
        if gated:
            kw["kgate"] = (gate, L)
        probs.append((dy, x, torch.empty(N, K, dtype=BF, device="cuda"), N, K, T, lda, ldb, K, kw))
    probs, sums = _ops._dw_balance(probs)
    tiles = sum((p[3] // 256) * (p[4] // 256) for p in probs)
    both("TN grouped dW" + (" gated" if gated else ""), "orbit2_debug_read_tq_trace_gemm", 0, tiles,
         lambda tq: _hip.gemm_grouped(probs, tail_queue=tq))
    del probs, sums
    torch.cuda.empty_cache()

# attention d = 128
qkv = rows(T, 3 * D, ldq)
dout = r(T, D)
for gated in (False, True):
    gt = gate if gated else None
    out = torch.empty(T, ldD, dtype=BF, device="cuda")[:, :D]
    res = {}

    def fwd(tq):
        res["o"], res["lse"] = _hip.attn_fwd(qkv, B, L, H, d, 0.1, 11, flags=_hip.ATTN_Q_PRESCALED, out=out, gate=gt, tail_queue=tq)

    def bwd(tq):
        _hip.attn_bwd(qkv, res["o"], dout, res["lse"], B, L, H, d, 0.1, 11, flags=_hip.ATTN_Q_PRESCALED, gate=gt, tail_queue=tq)

    sfx = " gated" if gated else ""
    both("attn fwd" + sfx, "orbit2_debug_read_tq_trace_attn", 0, (L // 256) * H * B, fwd)
    # (one call runs the statistics pass, dQ and dK + dV: the mean time is the whole backward's in both rows)
    for name, base, tiles in (("attn dQ", 0, (L // 256) * H * B), ("attn dK+dV", WGS // 2, (L // 128) * H * B)):
        both(name + sfx, "orbit2_debug_read_tq_trace_attn", base, tiles, bwd, reps=3)
