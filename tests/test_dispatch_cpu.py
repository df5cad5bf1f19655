"""Which kernel runs: the selection in csrc/gemm.hip and csrc/attn.hip for the product's own calls, pinned on the CPU.

tests/dispatch_recorder.hip includes both sources with hipLaunchKernelGGL redefined to print the kernel instantiation, grid, block
and launch arguments (host-only build, no GPU).  The expected lines in tests/dispatch_expected.txt were recorded from the sources of
the commit named in that file's header, never from the code under test: a product shape that falls from the 4-wave kernel to the
128-tile kernel, or from a generated attention kernel to a compiler-scheduled one, passes every parity test and fails here.

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


def build_recorder(csrc, out):
    subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O0", "-w", "-I", csrc,
                    os.path.join(ROOT, "tests", "dispatch_recorder.hip"), "-o", out], check=True, capture_output=True)
    return out


def record(exe, lines, env=None):
    e = {k: v for k, v in os.environ.items() if k != "ORBIT2_W4_PACE"}
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
def _dw_group(problems):
    """the grouped weight-gradient launch of _ops._DwBatch.flush for problems (N, K, M, lda, ldb) = dW[N, K] over M tokens:
    _ops._dw_balance's slicing on shapes alone"""
    from climate_learn import _ops
    S = _ops._DW_BALANCE
    M = problems[0][2]
    full = [dict(M=n, N=k, K=m, lda=lda, ldb=ldb, ldc=k, a_kc=0, b_kc=0) for n, k, m, lda, ldb in problems]
    ok = len(problems) >= 2 and all(p[2] == M and p[0] % 256 == 0 and p[1] % 256 == 0 for p in problems) and \
        M % (S * 64) == 0 and M // S >= 32768
    plan = _ops._dw_balance_plan([(p[0] // 256, p[1] // 256) for p in problems], S) if ok else None
    if plan is None:
        return group(full)
    cut = {i: (r0, r) for i, r0, r in plan}
    keep, split = [], [[] for _ in range(S)]
    for i, (n, k, m, lda, ldb) in enumerate(problems):
        if i not in cut:
            keep.append(full[i])
            continue
        r0, r = cut[i]
        if r0 > 0:
            keep.append(dict(full[i], M=256 * r0))
        for q in range(S):
            split[q].append(dict(M=256 * r, N=k, K=M // S, lda=lda, ldb=ldb, ldc=k, a_kc=0, b_kc=0))
    probs = keep + [u for q in range(S) for u in split[q]]
    return group(probs) if len(probs) <= 12 else group(full)


def _dw_single(N, K, M, lda, ldb):
    """_ops._dw: a lone weight gradient, split over the tokens when its output is too few tiles"""
    from climate_learn import _ops
    if _ops._dw_split_ok(M, N, K):
        S = _ops._DW_SPLIT
        return group([dict(M=N, N=K, K=M // S, lda=lda, ldb=ldb, ldc=K, a_kc=0, b_kc=0)] * S)
    return [gemm(N, K, M, lda, ldb, K, a_kc=0, b_kc=0)]


def product_calls(name, drop):
    from climate_learn import _ops
    D, heads, B, (h, w) = CONFIGS[name]
    L, d, hid = (h // 2) * (w // 2), D // heads, 4 * D
    M = B * L
    p = 0.1 if drop else 0.0
    ldD, ldq, ldh = _ops._ld_pad(D), _ops._ld_pad(3 * D), _ops._ld_pad(hid)
    dp = dict(drop_p=p, seed=7) if drop else {}
    path = dict(rowscale=P["rowscale"], rows_per_scale=L) if drop else {}
    gelu = dict(act=1, save_dact=P["save_dact"], **dp)
    out = ["# %s %s dropout: embedding" % (name, "with" if drop else "without")]
    out.append(gemm(M, D, D, D, D, D, bias=P["bias"], residual=P["residual"], ldr=D, res_mod=L, res_first=1, **dp))
    out += _dw_single(D, D, M, D, D)
    out.append(gemm(M, D, D, D, D, D, b_kc=0))
    out.append("# Block forward: qkv, attention, proj, fc1, fc2")
    out.append(gemm(M, 3 * D, D, ldD, D, ldq, bias=P["bias"], colscale_n=D, colscale=math.log2(math.e) / math.sqrt(d)))
    attn = dict(B=B, L=L, H=heads, d=d, drop_p=p, seed=7, flags=ATTN_Q_PRESCALED, ldq=ldq, ldo=ldD)
    out.append(call("afwd", **attn))
    out.append(gemm(M, D, D, ldD, D, D, bias=P["bias"], residual=P["residual"], ldr=D, **dp, **path))
    out.append(gemm(M, hid, D, ldD, D, ldh, bias=P["bias"], **gelu))
    out.append(gemm(M, D, hid, ldh, hid, D, bias=P["bias"], residual=P["residual"], ldr=D, **dp, **path))
    out.append("# Block backward: fc2 dx (fused column sums), fc1 dx, proj dx, attention, qkv dx, the grouped weight gradients")
    out.append(gemm(M, hid, D, D, hid, ldh, b_kc=0, mul=P["mul"], want_colsum=1))
    out.append(gemm(M, D, hid, ldh, D, D, b_kc=0))
    out.append(gemm(M, D, D, D, D, D, b_kc=0))
    out.append(call("abwd", **attn))
    out.append(gemm(M, D, 3 * D, ldq, D, D, b_kc=0))
    out += _dw_group([(D, hid, M, D, ldh), (hid, D, M, ldh, ldD), (D, D, M, D, ldD), (3 * D, D, M, ldq, ldD)])
    out.append("# head chain: 4 x (Linear + GELU), Linear to 192; backward")
    out += [gemm(M, D, D, D, D, D, bias=P["bias"], act=1, save_dact=P["save_dact"])] * 4
    out.append(gemm(M, 192, D, D, D, 192, bias=P["bias"]))
    out += _dw_single(192, D, M, 192, D)
    out.append(gemm(M, D, 192, 192, D, D, b_kc=0, mul=P["mul"]))
    out += [gemm(M, D, D, D, D, D, b_kc=0, mul=P["mul"])] * 3
    out.append(gemm(M, D, D, D, D, D, b_kc=0))
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


def sweep_log(exe):
    """(number of calls, the whole log): the product's calls and the three sweeps; the grouped sweep once per ORBIT2_W4_PACE setting
    (the library reads it once per process)"""
    fixed = all_product_calls() + sweep_gemm() + sweep_attn()
    grouped = sweep_grouped() + [ln for name in CONFIGS for ln in product_calls(name, True) if ln.startswith(("group", "g "))]
    log = record(exe, fixed)
    for pace in (None, "0", "2"):
        log += "== ORBIT2_W4_PACE %s\n" % pace + record(exe, grouped, {} if pace is None else {"ORBIT2_W4_PACE": pace})
    return log.count("\nrc=") + log.startswith("rc="), log


# ---- the test ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_product_calls_select_the_pinned_kernels(tmp_path):
    exe = build_recorder(CSRC, str(tmp_path / "dispatch_recorder"))
    got = record(exe, all_product_calls()).splitlines()
    want = [ln for ln in open(EXPECTED).read().splitlines() if not ln.startswith("#")]
    assert len(want) > 300                                   # 8 runs of ~30 calls, two or more lines each
    assert got == want, "\n".join(itertools.islice(difflib.unified_diff(want, got, "pinned", "this tree", lineterm="", n=2), 80))


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
