"""Which kernel runs: the selection in csrc/gemm.hip and csrc/attn.hip for the product's own calls, pinned on the CPU.

tests/dispatch_recorder.hip includes both sources with hipLaunchKernelGGL redefined to print the kernel instantiation, grid, block
and launch arguments (host-only build, no GPU).  Pinned are the calls the product makes under default settings -- with a counter
word and a library-sized tail, the Block's calls with their path gate or K gate -- on the recorder's own device
shape (256 CUs on 8 XCCs), so the lines say which twin of a kernel runs, on which grid, with which gate and which tail.  The
expected lines in tests/dispatch_expected.txt were recorded from the sources of the commit named in that file's header, never from
the code under test: a product shape that falls from the 4-wave kernel to the 128-tile kernel, or from a generated attention kernel
to a compiler-scheduled one, a mis-sized tail or an ignored gate passes every parity test and fails here.

Run as a script, the module is also the A/B driver for a change of the dispatch code itself:
    python tests/test_dispatch_cpu.py CSRC_DIR [LOG]      # product calls + the sweep below against CSRC_DIR; prints count, sha256
Two source trees select identically when the two digests agree (return codes are part of the log)."""
import difflib
import hashlib
import itertools
import math
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orbit-2_amd", "csrc")
EXPECTED = os.path.join(ROOT, "tests", "dispatch_expected.txt")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (embed_dim, heads, per-GPU batch, low-res grid) of the configurations the benchmark runs (configs/*.yaml, bench.py)
CONFIGS = {
    "interm_117m": (1024, 16, 8, (32, 64)),
    "interm_1b": (3072, 24, 16, (128, 256)),
    "interm_1b_daymet": (3072, 24, 4, (96, 192)),
    "interm_10b": (8192, 32, 2, (128, 256)),
}
ATTN_Q_PRESCALED = 4
P = dict(bias="0x1000", residual="0x2000", rowscale="0x3000", save_dact="0x4000", mul="0x5000", save_pre="0x6000",
         dgelu_pre="0x7000")      # fake addresses, 16-byte aligned; never dereferenced
SCHED = "0x9000"                  # the counter word of a tail-queue call
OTHER_GATE = "0x3100"             # a gate that is no call's row scale
TQ = dict(sched=SCHED, tail=0)    # _ops._TQ: the library sizes the tail
OTHER_DEVICE = {"ORBIT2_RECORDER_DEVICE": "304x8"}      # not the part the tail queue is sized for: auto tails stay static


def build_recorder(csrc, out):
    subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O0", "-w", "-I", csrc,
                    os.path.join(ROOT, "tests", "dispatch_recorder.hip"), "-o", out], check=True, capture_output=True)
    return out


def record(exe, lines, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("ORBIT2_W4_PACE", "ORBIT2_RECORDER_DEVICE")}
    e.update(env or {})
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=e, check=True)
    return r.stdout


def call(cmd, **kw):
    return cmd + " " + " ".join("%s=%s" % (k, v) for k, v in kw.items())


def gemm(M, N, K, lda, ldb, ldc, **kw):
    return call("gemm", M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, **kw)


def group(problems, n=None, **kw):
    """problems: keyword dicts of the members"""
    return [call("group", n=len(problems) if n is None else n, lines=len(problems), **kw)] + [call("g", **p) for p in problems]


# ---- the product's calls (climate_learn/_ops.py: BlockFn, ChainFn under res_slimvit's head, EmbedFn) ------------------------
def _dw_group(problems, kgate=None):
    """the grouped weight-gradient launch of _ops._DwBatch.flush for problems (N, K, M, lda, ldb) = dW[N, K] over M tokens: the
    units of _ops._dw_balance_units as recorder lines.  kgate = (address, tokens per entry): the K gate of every problem; a unit
    that takes the gate from entry g0 on gets the address of that entry (fp32: 4 bytes each)"""
    from climate_learn import _ops
    units = _ops._dw_balance_units([p[:3] for p in problems], _ops._DW_BALANCE, kgate and kgate[1])
    probs = []
    for i, n0, n1, m0, m1, g0 in units:
        n, k, m, lda, ldb = problems[i]
        kg = {} if g0 is None else dict(kgate=hex(int(kgate[0], 16) + 4 * g0), k_per_gate=kgate[1])
        probs.append(dict(M=n1 - n0, N=k, K=m1 - m0, lda=lda, ldb=ldb, ldc=k, a_kc=0, b_kc=0, **kg))
    return group(probs, **TQ)


def _dw_single(N, K, M, lda, ldb):
    """_ops._dw: a lone weight gradient, split over the tokens when its output is too few tiles"""
    from climate_learn import _ops
    if _ops._dw_split_ok(M, N, K):
        S = _ops._DW_SPLIT
        return group([dict(M=N, N=K, K=M // S, lda=lda, ldb=ldb, ldc=K, a_kc=0, b_kc=0)] * S, **TQ)
    return [gemm(N, K, M, lda, ldb, K, a_kc=0, b_kc=0)]                 # (the one call _ops makes without the tail queue)


def product_calls(name, drop):
    """what _ops passes under default settings: every call but a lone unsplit weight gradient with the tail queue, and in
    the dropout configurations (DropPath on) the Block's GEMMs and attention calls with the branch's scales as their gate"""
    from climate_learn import _ops
    D, heads, B, (h, w) = CONFIGS[name]
    L, d, hid = (h // 2) * (w // 2), D // heads, 4 * D
    M = B * L
    p = 0.1 if drop else 0.0
    ldD, ldq, ldh = _ops._ld_pad(D), _ops._ld_pad(3 * D), _ops._ld_pad(hid)
    dp = dict(drop_p=p, seed=7) if drop else {}
    path = dict(rowscale=P["rowscale"], rows_per_scale=L) if drop else {}
    gate = dict(gate=P["rowscale"], rows_per_gate=L) if drop else {}      # _ops._gate_kw
    agate = dict(gate=P["rowscale"]) if drop else {}
    kgate = (P["rowscale"], L) if drop else None
    gelu = dict(act=1, save_dact=P["save_dact"], **dp)
    out = ["# %s %s dropout: embedding" % (name, "with" if drop else "without")]
    out.append(gemm(M, D, D, D, D, D, bias=P["bias"], residual=P["residual"], ldr=D, res_mod=L, res_first=1, **dp, **TQ))
    out += _dw_single(D, D, M, D, D)
    out.append(gemm(M, D, D, D, D, D, b_kc=0, **TQ))
    out.append("# Block forward: qkv, attention, proj, fc1, fc2")
    out.append(gemm(M, 3 * D, D, ldD, D, ldq, bias=P["bias"], colscale_n=D, colscale=math.log2(math.e) / math.sqrt(d), **gate, **TQ))
    attn = dict(B=B, L=L, H=heads, d=d, drop_p=p, seed=7, flags=ATTN_Q_PRESCALED, ldq=ldq, ldo=ldD, **agate, **TQ)
    out.append(call("afwd", **attn))
    out.append(gemm(M, D, D, ldD, D, D, bias=P["bias"], residual=P["residual"], ldr=D, **dp, **path, **gate, **TQ))
    out.append(gemm(M, hid, D, ldD, D, ldh, bias=P["bias"], **gelu, **gate, **TQ))
    out.append(gemm(M, D, hid, ldh, hid, D, bias=P["bias"], residual=P["residual"], ldr=D, **dp, **path, **gate, **TQ))
    out.append("# Block backward: fc2 dx (fused column sums), fc1 dx, proj dx, attention, qkv dx, the grouped weight gradients")
    out.append(gemm(M, hid, D, D, hid, ldh, b_kc=0, mul=P["mul"], want_colsum=1, **gate, **TQ))
    out.append(gemm(M, D, hid, ldh, D, D, b_kc=0, **gate, **TQ))
    out.append(gemm(M, D, D, D, D, D, b_kc=0, **gate, **TQ))
    out.append(call("abwd", **attn))
    out.append(gemm(M, D, 3 * D, ldq, D, D, b_kc=0, **gate, **TQ))
    out += _dw_group([(D, hid, M, D, ldh), (hid, D, M, ldh, ldD), (D, D, M, D, ldD), (3 * D, D, M, ldq, ldD)], kgate)
    out.append("# head chain: 4 x (Linear + GELU), Linear to 192; backward")
    out += [gemm(M, D, D, D, D, D, bias=P["bias"], act=1, save_dact=P["save_dact"], **TQ)] * 4
    out.append(gemm(M, 192, D, D, D, 192, bias=P["bias"], **TQ))
    out += _dw_single(192, D, M, 192, D)
    out.append(gemm(M, D, 192, 192, D, D, b_kc=0, mul=P["mul"], **TQ))
    out += [gemm(M, D, D, D, D, D, b_kc=0, mul=P["mul"], **TQ)] * 3
    out.append(gemm(M, D, D, D, D, D, b_kc=0, **TQ))
    out += _dw_group([(D, D, M, D, D)] * 4)
    return out


def all_product_calls():
    return [ln for name in CONFIGS for drop in (True, False) for ln in product_calls(name, drop)]


# ---- the sweep (script mode): every rule of the selection from both sides ----------------------------------------------------
def sweep_gemm():
    shapes = [(131072, 12288, 3072), (3072, 4096, 1024), (2560, 4864, 1024), (512, 45824, 512), (256, 91904, 512),
              (4608, 5120, 512), (131000, 12288, 3072), (4096, 12296, 3072), (4096, 4096, 3104), (4096, 4096, 3076),
              (4096, 4096, 64), (4096, 4096, 96), (4096, 4096, 128), (4096, 1024, 1024), (64, 1024, 1024), (48, 1024, 1024),
              (72, 1024, 1024), (768, 512, 192), (4096, 8192, 8192), (18432, 3072, 3072)]
    hints = [0, 64, 128, 256, 257, 258, 260, 261, 262, 7]
    drop = dict(drop_p=0.1, seed=3)
    k1 = dict(bias=P["bias"], act=1, save_dact=P["save_dact"])
    k2 = dict(bias=P["bias"], residual=P["residual"], ldr=4096)
    k3 = dict(mul=P["mul"])
    epis = [{}, k1, dict(k1, **drop), k2, dict(k2, **drop), dict(k2, rowscale=P["rowscale"], rows_per_scale=8192),
            dict(k2, rowscale=P["rowscale"], rows_per_scale=100), k3,
            # near-misses of w4_epi_kind: first clause
            dict(k2, out_fp32=1), dict(k2, save_pre=P["save_pre"]), dict(dgelu_pre=P["dgelu_pre"]), dict(k2, beta=1.0),
            dict(k2, colscale_n=8, colscale=0.5), dict(k2, res_first=1), dict(k2, res_mod=512), dict(bias=P["bias"], act=2),
            # kind 1
            dict(k1, bias=0), dict(k1, act=0), dict(k1, residual=P["residual"], ldr=4096),
            dict(k1, rowscale=P["rowscale"], rows_per_scale=256), dict(k1, mul=P["mul"]),
            # kind 2
            dict(k2, mul=P["mul"]), dict(k2, ldr=4100), dict(k2, residual="0x2008"), dict(k2, act=1),
            # kind 3
            dict(k3, bias=P["bias"]), dict(k3, **drop), dict(k3, rowscale=P["rowscale"], rows_per_scale=256),
            dict(k3, save_dact=P["save_dact"]), dict(k3, dgelu_pre=P["dgelu_pre"]),
            # heavy epilogues outside the compile-time kinds
            dict(bias=P["bias"], act=1), drop, dict(dgelu_pre=P["dgelu_pre"], **drop), dict(save_dact=P["save_dact"], act=1, drop_p=0.45)]
    out = []
    for (M, N, K), (akc, bkc), hint, epi, ws in itertools.product(shapes, itertools.product((1, 0), (1, 0)), hints, epis, (0, 1)):
        kw = dict(a_kc=akc, b_kc=bkc, tile_hint=hint, **epi)
        if ws:
            kw["colsum_ws"] = "0x8000"
        out.append(gemm(M, N, K, K if akc else M, K if bkc else N, N, **kw))
    # pitches (the "camped rows" rule is about them), misaligned pointers and strides, broken argument blocks
    for lda, ldb, hint in itertools.product((8192, 8256, 12288), (8192, 8256), (0, 260)):
        out.append(gemm(4096, 8192, 8192, lda, ldb, 8192, tile_hint=hint))
    out.append(gemm(4096, 8192, 4096, 4096, 4096, 8192))
    for bad in (dict(A="0x10008"), dict(B="0x20004"), dict(C="0x30002"), dict(lda=4100), dict(ldb=4100), dict(ldc=4098),
                dict(A=0), dict(M=0), dict(K=-64), dict(drop_p=1.0), dict(drop_p=-0.5), dict(rowscale=P["rowscale"]),
                dict(colscale_n=12), dict(save_dact="0x4008", act=1), dict(mul=P["mul"], dgelu_pre=P["dgelu_pre"]), dict(null=1)):
        out.append(call("gemm", **dict(dict(M=4096, N=4096, K=4096, lda=4096, ldb=4096, ldc=4096), **bad)))
    return out


FORMS = tuple(itertools.product((1, 0), (1, 0)))
TAILS = ({}, dict(sched=SCHED, tail=0), dict(sched=SCHED, tail=-1), dict(sched=SCHED, tail=64))


def sweep_gemm_gate_queue():
    """the path gate and the tail queue of the single GEMM: a reduced cross of shapes x forms x epilogues at hints 0 / 260 / 262"""
    big, small = (131072, 12288, 3072), (3072, 4096, 1024)          # 24576 tiles of 256 x 256; 192
    out = []

    def add(shape, form, **kw):
        (M, N, K), (akc, bkc) = shape, form
        out.append(gemm(M, N, K, K if akc else M, K if bkc else N, N, a_kc=akc, b_kc=bkc, **kw))

    # every clause of the gate rule, honoured and as a near-miss
    G, rows = P["rowscale"], 8192
    res = dict(bias=P["bias"], residual=P["residual"], ldr=12288, rowscale=G, rows_per_scale=rows)
    epis = [{}, dict(bias=P["bias"]), res, dict(out_fp32=1), dict(res, out_fp32=1), dict(beta=1.0), dict(res, beta=1.0),
            dict(res, res_first=1), dict(res, res_mod=4096), dict(res, rowscale=OTHER_GATE), dict(res, rows_per_scale=4096),
            dict(res, save_pre=P["save_pre"]), dict(res, act=1, save_dact=P["save_dact"]), dict(res, colsum_ws="0x8000"),
            dict(res, ldr=12292), dict(res, residual="0x2008"), dict(rowscale=G, rows_per_scale=rows),
            dict(res, drop_p=0.1, seed=3), dict(mul=P["mul"]), dict(mul=P["mul"], colsum_ws="0x8000")]
    for form, hint, epi, tq in itertools.product(FORMS, (0, 260, 262), epis, TAILS):
        add(big, form, tile_hint=hint, gate=G, rows_per_gate=rows, **epi, **tq)
    for form, tq, bad in itertools.product(((1, 1), (1, 0)), TAILS[:2], (dict(rows_per_gate=0), dict(rows_per_gate=-8),
                                                                       dict(gate=0, rows_per_gate=rows), dict(gate=0, rows_per_gate=0))):
        add(big, form, **dict(dict(res, gate=G), **bad), **tq)
    # the tail of every (form, kind) pair, auto and forced (1, 64, T, T + 1 tiles), gated or not
    k1 = dict(bias=P["bias"], act=1, save_dact=P["save_dact"])
    k2 = dict(bias=P["bias"], residual=P["residual"], ldr=12288)
    drop = dict(drop_p=0.1, seed=3)
    for shape, form, hint, epi, gate in itertools.product((big, small), FORMS, (0, 260, 262),
                                                          ({}, k1, dict(k1, **drop), k2, dict(k2, **drop), dict(mul=P["mul"])),
                                                          ({}, dict(gate=G, rows_per_gate=rows))):
        T = (shape[0] // 256) * (shape[1] // 256)
        for tail in (0, -1, 1, 64, T, T + 1):
            add(shape, form, tile_hint=hint, sched=SCHED, tail=tail, **epi, **gate)
    # O2_TQ_MIN_STATIC_ROUNDS: a two-round family asks for its tail from 6 rounds of 256 tiles on
    for shape, (form, epi), hint in itertools.product(((1280, 78592, 1024), (1536, 65536, 1024), (1536, 65792, 1024)),
                                                      (((1, 0), {}), ((1, 1), k2), ((1, 1), {}), ((0, 0), {})), (0, 260)):
        add(shape, form, tile_hint=hint, sched=SCHED, tail=0, **epi)
    # the other families and the stamped form stay static with a counter; a counter the entry refuses
    for shape, form, hint, tail in itertools.product((big, small, (131000, 12288, 3072)), FORMS, (0, 64, 128, 256, 261), (0, 64)):
        add(shape, form, tile_hint=hint, sched=SCHED, tail=tail)
    for sched, gate, hint in itertools.product((0, "0x9002", "0x9001"), ({}, dict(gate=G, rows_per_gate=rows)), (0, 128)):
        add(big, (1, 0), tile_hint=hint, sched=sched, tail=0, **gate)
    out.append(call("gemm", null=1, sched=SCHED, tail=0))
    out.append(call("gemm", null=1, gate=G, rows_per_gate=rows))
    return out


def sweep_grouped():
    def prob(M, N, K, akc=0, bkc=0, **kw):
        return dict(M=M, N=N, K=K, lda=K if akc else M, ldb=K if bkc else N, ldc=N, a_kc=akc, b_kc=bkc, **kw)
    out = []
    for n in range(0, 14):
        for (M, N), K, hint, (akc, bkc) in itertools.product(((3072, 3072), (256, 256), (256, 5120), (1000, 3072)),
                                                            (32768, 32704, 64, 96), (0, 128, 256, 7),
                                                            ((0, 0), (1, 1), (1, 0), (0, 1))):
            members = [prob(M, N, K, akc, bkc, **({"tile_hint": hint} if i == 0 else {})) for i in range(min(n, 12))]
            out += group(members, n=n)
    base = [prob(3072, 3072, 32768) for _ in range(4)]
    out += group(base[:3] + [prob(3072, 3072, 32768, 1, 1)])                      # mixed forms
    out += group(base[:3] + [prob(3072, 3000, 32768)])                            # one ragged member
    out += group(base[:3] + [prob(3072, 3072, 32768, colsum_ws="0x8000")])        # column sums: single launches only
    out += group(base[:3] + [prob(3072, 3072, 32768, A="0x10008")])               # a member the epilogue check refuses
    out += group([prob(256, 256 * t, 32768) for t in (100, 100, 56)])             # 256 tiles in all: not more than a round
    out += group([prob(256, 256 * t, 32768) for t in (100, 100, 57)])             # 257
    out += group([prob(256, 256 * t, 65536) for t in (100, 91)])                  # 191 tiles: under the grouped fill rule
    out += group([prob(256, 256 * t, 65536) for t in (100, 92)])                  # 192
    out += group(base, null=1)
    # ---- the K gates and the tail queue (576 tiles; the pacing start barrier is on: K = 512 K-tiles, more than a round)
    G = P["rowscale"]
    ok = dict(kgate=G, k_per_gate=4096)
    tails = ({}, dict(sched=SCHED, tail=0), dict(sched=SCHED, tail=-1), dict(sched=SCHED, tail=64))
    for tq in tails:
        out += group([dict(p, **ok) for p in base], **tq)
        out += group([dict(p, kgate=G, k_per_gate=4000) for p in base], **tq)          # not whole K-tiles
        out += group([dict(p, kgate=G, k_per_gate=5120) for p in base], **tq)          # K is not whole entries
        out += group([dict(p, kgate=G, k_per_gate=0) for p in base], **tq)
        out += group([dict(p, **(ok if i % 2 else {})) for i, p in enumerate(base)], **tq)      # NULL entries among the gates
        out += group([dict(p, **(ok if i % 2 else dict(kgate=0, k_per_gate=4096))) for i, p in enumerate(base)], **tq)
        for akc, bkc in ((1, 1), (1, 0), (0, 1)):                                      # a form other than TN
            out += group([dict(prob(3072, 3072, 32768, akc, bkc), **ok) for _ in range(4)], **tq)
        for hint in (128, 256):                                                        # a family other than the 4-wave one
            out += group([dict(p, **ok, **({"tile_hint": hint} if i == 0 else {})) for i, p in enumerate(base)], **tq)
        out += group([dict(p, **ok) for p in base[:3]] + [dict(prob(3072, 3000, 32768), **ok)], **tq)
        out += group([dict(base[0], **ok)], **tq)                                      # n = 1: the single launch, with the counter
        out += group([dict(prob(131072, 12288, 3072, 1, 0), **ok)], **tq)              # ... on a shape whose single launch has a tail
        out += group(base, **tq)
    for tail in (1, 64, 319, 320, 321, 575, 576, 577):      # 320 leaves S = 256 static workgroups (no start barrier), 319 S = 257
        out += group(base, sched=SCHED, tail=tail)
        out += group([dict(p, **ok) for p in base], sched=SCHED, tail=tail)
    # O2_TQ_MIN_STATIC_ROUNDS: the four-round grouped family asks for its tail from 8 rounds of 256 tiles on
    for last in (47, 48, 49):
        out += group([prob(256, 256 * t, 32768) for t in (1000, 1000, last)], sched=SCHED, tail=0)
    for sched in (0, "0x9002"):
        out += group(base, sched=sched, tail=0)
        out += group(base[:1], sched=sched, tail=0)
    out += group(base, null=1, sched=SCHED, tail=0)
    out += group(base, n=0, sched=SCHED, tail=0)
    out += group(base, n=13, sched=SCHED, tail=0)
    return out


def sweep_attn():
    out = []
    for d, L, flags, p, pad, cmd in itertools.product((64, 96, 128, 256), (128, 256, 512, 8192, 8200, 16384, 16640), range(16),
                                                      (0.0, 0.1), (0, 64), ("afwd", "abwd")):
        H = 4
        out.append(call(cmd, B=2, L=L, H=H, d=d, drop_p=p, seed=5, flags=flags, ldq=3 * H * d + pad, ldo=H * d + pad))
    for cmd, flags in itertools.product(("afwd", "abwd"), (4, 6, 12)):
        out.append(call(cmd, B=1, L=16384, H=171, d=128, flags=flags, ldq=3 * 171 * 128, ldo=171 * 128))      # past 32-bit byte offsets
        out.append(call(cmd, B=1, L=16384, H=24, d=128, flags=flags, ldq=3 * 24 * 128, ldo=65664))
        out.append(call(cmd, B=10923, L=16384, H=24, d=128, flags=flags, ldq=9216, ldo=3072))                # B * H * L >= 2^32
        out.append(call(cmd, B=10922, L=16384, H=24, d=128, flags=flags, ldq=9216, ldo=3072))
        ok = dict(B=2, L=512, H=4, d=128, flags=flags, ldq=1536, ldo=512)
        for bad in (dict(qkv=0), dict(out=0), dict(lse=0), dict(dout=0), dict(delta=0), dict(dqkv=0), dict(B=0), dict(L=0),
                    dict(H=-1), dict(d=32), dict(drop_p=1.0), dict(drop_p=-0.1), dict(ldo=504), dict(ldo=516), dict(ldq=1528),
                    dict(ldq=1540)):
            out.append(call(cmd, **dict(ok, **bad)))
    return out


def sweep_attn_gate_queue():
    """the gate and the tail queue of the attention entries: the generated kernels (d = 128, flags 4) against the
    compiler-scheduled ones (other d, NO_W4, q not pre-scaled), the split dK + dV pass, launches large and small"""
    out = []
    G = P["rowscale"]
    for (B, H, L), d, flags, p, cmd, gate in itertools.product(((16, 24, 8192), (2, 4, 512)), (64, 128, 256), (0, 4, 6, 12),
                                                               (0.0, 0.1), ("afwd", "abwd"), ({}, dict(gate=G))):
        base = dict(B=B, L=L, H=H, d=d, drop_p=p, seed=5, flags=flags, ldq=3 * H * d, ldo=H * d, **gate)
        out.append(call(cmd, **base))
        T = (L // 256) * H * B                  # 256-row workgroups of the forward and of dQ; dK + dV has twice as many
        for tail in (0, -1, 1, 64, T, T + 1, 2 * T, 2 * T + 1):
            out.append(call(cmd, sched=SCHED, tail=tail, **base))
    for cmd, flags, tail, gate in itertools.product(("afwd", "abwd"), (4, 6), (0, 64), ({}, dict(gate=G))):
        for B in (10923, 10922):                # B * H * L >= 2^32: dQ stays on the generated kernel, dK + dV leaves it
            out.append(call(cmd, B=B, L=16384, H=24, d=128, flags=flags, ldq=9216, ldo=3072, sched=SCHED, tail=tail, **gate))
    for cmd, sched in itertools.product(("afwd", "abwd"), (0, "0x9002")):
        out.append(call(cmd, B=2, L=512, H=4, d=128, flags=4, ldq=1536, ldo=512, sched=sched, tail=0))
        out.append(call(cmd, B=2, L=512, H=4, d=64, flags=0, ldq=768, ldo=256, sched=sched, tail=0, gate=G))
    return out


def sweep_log(exe):
    """(number of calls, the whole log): the product's calls and the sweeps; the grouped sweep once per ORBIT2_W4_PACE setting
    (the library reads it once per process), the gate / tail-queue sweeps also on a device the tail queue is not sized for"""
    queue = sweep_gemm_gate_queue() + sweep_attn_gate_queue()
    fixed = all_product_calls() + sweep_gemm() + sweep_attn() + queue
    grouped = sweep_grouped() + [ln for name in CONFIGS for ln in product_calls(name, True) if ln.startswith(("group", "g "))]
    log = record(exe, fixed)
    for pace in (None, "0", "2"):
        log += "== ORBIT2_W4_PACE %s\n" % pace + record(exe, grouped, {} if pace is None else {"ORBIT2_W4_PACE": pace})
    log += "== ORBIT2_RECORDER_DEVICE %s\n" % OTHER_DEVICE["ORBIT2_RECORDER_DEVICE"]
    log += record(exe, all_product_calls() + queue + grouped, OTHER_DEVICE)
    return log.count("\nrc=") + log.startswith("rc="), log


# ---- the test ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_product_calls_select_the_pinned_kernels(tmp_path):
    exe = build_recorder(CSRC, str(tmp_path / "dispatch_recorder"))
    got = record(exe, all_product_calls()).splitlines()
    want = [ln for ln in open(EXPECTED).read().splitlines() if not ln.startswith("#")]
    assert len(want) > 300                                   # 8 runs of ~30 calls, two or more lines each
    assert got == want, "\n".join(itertools.islice(difflib.unified_diff(want, got, "pinned", "this tree", lineterm="", n=2), 80))


# ---- the gate and the queue do not move the selection ---------------------------------------------------
OWN = ("gate", "rows_per_gate", "sched", "tail", "kgate", "k_per_gate")     # the keys of the gate and the queue


def _blocks(lines):
    """the calls of a list of lines, each with its "g" lines and without the gate / queue keys and the comments"""
    out = []
    for ln in lines:
        if ln.startswith("#"):
            continue
        ln = " ".join(t for t in ln.split() if t.split("=")[0] not in OWN)
        if ln.startswith("g "):
            out[-1].append(ln)
        else:
            out.append([ln])
    return out


def _with(block, head=None, member=None):
    return [block[0] + (" " + head if head else "")] + [g + (" " + member if member else "") for g in block[1:]]


def _parse(log):
    """per call: (return code, [(kernel name, grid, block, the rest of the launch line)])"""
    out = []
    for rec in ("\n" + log).split("\n> ")[1:]:
        lines = rec.splitlines()
        launches = [ln.split(" ", 3) for ln in lines[1:] if " grid=" in ln]
        out.append((lines[-1], [(k, g, b, rest) for k, g, b, rest in launches]))
    return out


def _untwinned(kernel):
    """the name of the plain kernel a gated or tail-queue twin stands for"""
    name, args = kernel.rstrip(">").split("<") if "<" in kernel else (kernel, "")
    a = [x.strip() for x in args.split(",")]
    if name == "gemm256w_tq_kernel":
        return "gemm256w_kernel<%s, false, %s>" % (a[0], a[1])
    if name == "gemm256w_grouped_tq_kernel":
        return "gemm256w_grouped_kernel<%s>" % a[0]
    for twin in ("_w4_gated_kernel", "_w4_tq_kernel"):
        if name.endswith(twin):
            return "%s_w4_kernel<%s>" % (name[:-len(twin)], a[0])
    return kernel


def no_move_inputs():
    """every product call, and sweep lines that reach the four GEMM families (single and grouped) and both attention classes"""
    shapes = ((131072, 12288, 3072), (3072, 4096, 1024), (131000, 12288, 3072), (768, 512, 192))
    k2 = dict(bias=P["bias"], residual=P["residual"], ldr=12288, rowscale=P["rowscale"], rows_per_scale=8192)
    lines = all_product_calls()
    for (M, N, K), (akc, bkc), epi in itertools.product(shapes, ((1, 1), (1, 0), (0, 0)), ({}, k2)):
        lines.append(gemm(M, N, K, K if akc else M, K if bkc else N, N, a_kc=akc, b_kc=bkc, **epi))
    lines.append(gemm(768, 512, 192, 192, 192, 512, tile_hint=128))
    for hint, K in itertools.product((0, 128, 256), (32768, 32704)):
        lines += group([dict(M=3072, N=3072, K=K, lda=3072, ldb=3072, ldc=3072, a_kc=0, b_kc=0,
                             **({"tile_hint": hint} if i == 0 else {})) for i in range(4)])
    for d, flags, p, cmd in itertools.product((64, 128, 256), (4, 6, 12), (0.0, 0.1), ("afwd", "abwd")):
        lines.append(call(cmd, B=16, L=8192, H=24, d=d, drop_p=p, seed=5, flags=flags, ldq=3 * 24 * d, ldo=24 * d))
    return _blocks(lines)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_gate_and_the_queue_do_not_move_the_selection(tmp_path):
    """Each call plain, gated, queued with tail < 0 and queued with an auto tail on a device the queue is not sized for: the same
    return code, grid and block, the same kernel up to its documented twin (gemm256w_kernel<F, false, E> / gemm256w_tq_kernel<F, E>,
    ..._w4_kernel<D> / ..._w4_gated_kernel<D> / ..._w4_tq_kernel<D, G>); a queued call whose plan has no tail launches exactly what
    the unqueued call launches; so does a gated call whose gate the rule of DESIGN 4.11 ignores (a residual behind a row scale
    that is not the gate).  A grouped launch whose tail leaves no more than one round of static workgroups has no start barrier."""
    exe = build_recorder(CSRC, str(tmp_path / "dispatch_recorder"))
    blocks = no_move_inputs()
    kv = lambda ln: dict(t.split("=") for t in ln.split()[1:])

    def gated(b):
        if b[0].startswith("a"):
            return _with(b, "gate=" + OTHER_GATE)
        if b[0].startswith("gemm"):
            return _with(b, "gate=%s rows_per_gate=%s" % (OTHER_GATE, kv(b[0]).get("rows_per_scale", 256)))
        return _with(b, member="kgate=%s k_per_gate=64" % OTHER_GATE)

    flat = lambda bs: [ln for b in bs for ln in b]
    plain = _parse(record(exe, flat(blocks)))
    gate = _parse(record(exe, flat(gated(b) for b in blocks)))
    static = _parse(record(exe, flat(_with(b, "sched=%s tail=-1" % SCHED) for b in blocks)))
    other = _parse(record(exe, flat(_with(b, "sched=%s tail=0" % SCHED) for b in blocks), OTHER_DEVICE))
    assert len(plain) == len(gate) == len(static) == len(other) == len(blocks) > 150
    kernels = set()
    for b, p, g, s, o in zip(blocks, plain, gate, static, other):
        assert s == p and o == p, b                              # no tail: the unqueued launch, argument by argument
        assert g[0] == p[0] and [(_untwinned(k), gr, bl) for k, gr, bl, _ in g[1]] == [(k, gr, bl) for k, gr, bl, _ in p[1]], b
        a = kv(b[0])
        if b[0].startswith("gemm") and "residual" in a and "rowscale" in a:
            assert g == p, b                                     # the row scale is not the gate: the gate is ignored
        kernels.update(k.split("<")[0] for k, _, _, _ in p[1])
    assert {"gemm128_kernel", "gemm256t_kernel", "gemm256w_kernel", "gemm128_grouped_kernel", "gemm256t_grouped_kernel",
            "gemm256w_grouped_kernel", "attn_fwd_w4_kernel", "attn_bwd_dq_w4_kernel", "attn_bwd_dkv_w4_kernel", "attn_fwd_kernel",
            "attn_fwd_lazy_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"} <= kernels
    assert any(_untwinned(k) != k for _, ls in gate for k, _, _, _ in ls)      # some gated twin did run
    # grouped launches with a forced tail: T + tail workgroups of the twin; the start barrier only with more than a round static
    groups = [(b, p) for b, p in zip(blocks, plain) if b[0].startswith("group") and p[1] and
              p[1][0][0].startswith("gemm256w_grouped_kernel") and int(p[1][0][1].split("=")[1]) > 257]
    assert any(" pace=1 " in p[1][0][3] for _, p in groups)
    for static_wgs in (256, 257):
        tails = [int(p[1][0][1].split("=")[1]) - static_wgs for _, p in groups]
        queued = _parse(record(exe, flat(_with(b, "sched=%s tail=%d" % (SCHED, t)) for (b, _), t in zip(groups, tails))))
        for (b, p), t, q in zip(groups, tails, queued):
            (k, gr, bl, rest), (pk, pgr, pbl, prest) = q[1][0], p[1][0]
            assert q[0] == p[0] and _untwinned(k) == pk and k != pk and bl == pbl and gr == "grid=%d" % (static_wgs + 2 * t), b
            want = prest.replace(" pace=1 ", " pace=0 ").replace(" pace=2 ", " pace=0 ") if static_wgs == 256 else prest
            assert rest == "%s 0x%x %d %d" % (want, int(SCHED, 16), static_wgs, t), b


# ---- a counter and a tail go together --------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_a_tail_without_a_counter_and_a_misaligned_counter_are_refused(tmp_path):
    """every folded entry: tail >= 0 with a NULL counter, and a counter that is not 4-byte aligned at any tail (static included),
    return O2_ERR_ARG (-1) before any launch"""
    exe = build_recorder(CSRC, str(tmp_path / "dispatch_recorder"))
    member = dict(M=3072, N=3072, K=32768, lda=3072, ldb=3072, ldc=3072, a_kc=0, b_kc=0)
    attn = dict(B=2, L=512, H=4, d=128, flags=ATTN_Q_PRESCALED, ldq=1536, ldo=512)
    for bad in (dict(sched=0, tail=0), dict(sched="0x9002", tail=-1)):
        lines = [gemm(131072, 12288, 3072, 3072, 12288, 12288, b_kc=0, **bad)] + group([member] * 4, **bad) + \
            [call("afwd", **attn, **bad), call("abwd", **attn, **bad)]
        calls = _parse(record(exe, lines))
        assert len(calls) == 4
        assert all(rc == "rc=-1" and not launches for rc, launches in calls), bad
    plain = [ln for b in _blocks(lines) for ln in b]             # the same four calls without the queue's keys do launch
    assert all(rc == "rc=0" and launches for rc, launches in _parse(record(exe, plain)))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "orbit-2_amd"))
    csrc = sys.argv[1] if len(sys.argv) > 1 else CSRC
    exe = build_recorder(csrc, os.path.join(os.environ.get("TMPDIR", "/tmp"), "dispatch_recorder_%d" % os.getpid()))
    try:
        if "--product" in sys.argv:                          # the text of tests/dispatch_expected.txt (below its header)
            sys.stdout.write(record(exe, all_product_calls()))
        else:
            calls, log = sweep_log(exe)
            if len(sys.argv) > 2:
                open(sys.argv[2], "w").write(log)
            print("%d calls, sha256 %s" % (calls, hashlib.sha256(log.encode()).hexdigest()))
    finally:
        os.remove(exe)
