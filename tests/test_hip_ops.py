"""GPU parity tests: every C-ABI entry point against the CPU oracle (oracle/orbit2_oracle.py, plain
PyTorch fp32) on the same seeded inputs.  bf16 kernels are compared against the fp32 oracle evaluated on
the bf16-rounded inputs; tolerance = normalised max error (max|a-b| / max|b|), stated per test."""
import os
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import orbit2_oracle as O
from tests.hashmask import attn_keep_mask, keep_mask


@pytest.fixture(scope="module")
def hip():
    from climate_learn import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip


def nerr(a, b):
    a = a.detach().float().cpu().double()
    b = b.detach().float().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def bf(t):
    return t.to(torch.bfloat16)


def rt(t):
    """round-trip through bf16 (what the kernel sees), back to fp32 on CPU"""
    return t.to(torch.bfloat16).float()


def test_selftest_layout_maps(hip):
    assert hip.selftest() == 0


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 192), (136, 200, 128), (1024, 1024, 512), (520, 776, 192)])
@pytest.mark.parametrize("form", ["nt", "nn", "tn", "tt"])
@pytest.mark.parametrize("tile", [128, 256])
def test_gemm_forms(hip, M, N, K, form, tile):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = rt(torch.randn(M, K, generator=g))
    B = rt(torch.randn(N, K, generator=g))
    ref = A @ B.t()
    a_kc = form[0] == "n"
    b_kc = form[1] == "t"
    Ad = bf(A if a_kc else A.t().contiguous()).cuda()
    Bd = bf(B if b_kc else B.t().contiguous()).cuda()
    out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    hip.gemm(Ad, Bd, out, M, N, K, K if a_kc else M, K if b_kc else N, N, a_kc=a_kc, b_kc=b_kc, tile=tile)
    torch.cuda.synchronize()
    assert nerr(out, ref) < 2e-5   # fp32 out: only accumulation-order differences
    outb = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(Ad, Bd, outb, M, N, K, K if a_kc else M, K if b_kc else N, N, a_kc=a_kc, b_kc=b_kc, tile=tile)
    assert nerr(outb, ref) < 6e-3  # one bf16 rounding of the result (2^-8 relative)


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (256, 512, 128), (512, 768, 192), (1024, 1024, 512), (768, 256, 1088)])
@pytest.mark.parametrize("form", ["nt", "nn", "tn", "tt"])
def test_gemm_forms_4wave_kernel(hip, M, N, K, form):
    """the 4-wave 256x256x64 kernel (tile hint 260; whole tiles, hand-placed main loop, csrc/gemm_w4_asm.h): every operand
    form against the fp32 product, K-tiles 1, 2 and 3 (pipeline prologue / dead-slot loads), an odd count (17), and bit-equality
    with the 8-phase kernel (same k order per accumulator) for fp32, bf16 and beta-accumulating outputs"""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = rt(torch.randn(M, K, generator=g))
    B = rt(torch.randn(N, K, generator=g))
    ref = A @ B.t()
    a_kc, b_kc = form[0] == "n", form[1] == "t"
    Ad = bf(A if a_kc else A.t().contiguous()).cuda()
    Bd = bf(B if b_kc else B.t().contiguous()).cuda()
    lda, ldb = (K if a_kc else M), (K if b_kc else N)
    outs = {}
    for tile in (260, 256):
        out = torch.empty(M, N, dtype=torch.float32, device="cuda")
        hip.gemm(Ad, Bd, out, M, N, K, lda, ldb, N, a_kc=a_kc, b_kc=b_kc, tile=tile)
        outb = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        hip.gemm(Ad, Bd, outb, M, N, K, lda, ldb, N, a_kc=a_kc, b_kc=b_kc, tile=tile)
        acc = torch.full((M, N), 0.5, dtype=torch.bfloat16, device="cuda")
        hip.gemm(Ad, Bd, acc, M, N, K, lda, ldb, N, a_kc=a_kc, b_kc=b_kc, beta=1.0, tile=tile)
        outs[tile] = (out, outb, acc)
    torch.cuda.synchronize()
    assert nerr(outs[260][0], ref) < 2e-5
    assert nerr(outs[260][1], ref) < 6e-3
    assert nerr(outs[260][2], ref + 0.5) < 6e-3
    for x, y in zip(outs[260], outs[256]):
        assert torch.equal(x, y)


def test_gemm_4wave_kernel_operands_beyond_2GiB(hip):
    """weight-gradient form at the size of the interm_1b batch-16 step: 131072 tokens x a 9216-wide K-strided operand = 2.4 GB, so
    the last third of the contraction lies past 2^31 bytes from the operand's base -- the range of a buffer descriptor; the
    kernel advances the descriptors' 48-bit bases along K (a 32-bit per-lane offset read zeros there: found in round 3 by
    comparing with the 8-phase kernel at this size)"""
    K, M, N = 131072, 256, 256
    g = torch.Generator().manual_seed(9)
    A = bf(torch.randn(K, 9216, generator=g) * 0.5).cuda()
    B = bf(torch.randn(K, 256, generator=g) * 0.5).cuda()
    outs = []
    for tile in (260, 256):
        o = torch.empty(M, N, dtype=torch.float32, device="cuda")
        hip.gemm(A[:, 9216 - M:], B, o, M, N, K, 9216, 256, N, a_kc=False, b_kc=False, tile=tile)   # the operand's LAST columns
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref = A[K - 4096:, 9216 - M:].float().t() @ B[K - 4096:].float()                                  # the tail alone is non-zero
    tail = torch.empty(M, N, dtype=torch.float32, device="cuda")
    hip.gemm(A[K - 4096:, 9216 - M:], B[K - 4096:], tail, M, N, 4096, 9216, 256, N, a_kc=False, b_kc=False, tile=260)
    assert nerr(tail, ref.cpu()) < 2e-5


@pytest.mark.parametrize("name,M,N,K,a_kc,b_kc", [
    ("fwd qkv", 131072, 9216, 3072, True, True), ("fwd fc2", 131072, 3072, 12288, True, True),
    ("dX qkv", 131072, 3072, 9216, True, False), ("dX fc1", 131072, 3072, 12288, True, False),
    ("dW qkv", 9216, 3072, 131072, False, False), ("dW fc1", 12288, 3072, 131072, False, False),
    ("dW fc2", 3072, 12288, 131072, False, False)])
def test_gemm_4wave_equals_8phase_at_the_bench_shapes(hip, name, M, N, K, a_kc, b_kc):
    """the GEMM shapes of the interm_1b step at per-GPU batch 16 (131072 tokens; the hidden tensors with their padded row pitch):
    two independently written kernels -- 64-bit global addresses in the 8-phase kernel, buffer descriptors in the 4-wave kernel --
    must agree bit for bit at FULL size (operands of 2-3 GB; address arithmetic that only small shapes exercise is how the
    round-3 descriptor-range defect got past the other tests)"""
    pad = lambda n: n + 64 if (2 * n) % 8192 == 0 else n
    g = torch.Generator(device="cuda").manual_seed(len(name) + M)
    rnd = lambda r, c, ld: (torch.randn(r, ld, device="cuda", generator=g) * 0.5).to(torch.bfloat16)[:, :c]
    A = rnd(M, K, pad(K)) if a_kc else rnd(K, M, pad(M))
    B = rnd(N, K, K) if b_kc else rnd(K, N, pad(N))
    outs = []
    for tile in (260, 256):
        o = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        hip.gemm(A, B, o, M, N, K, A.stride(0), B.stride(0), N, a_kc=a_kc, b_kc=b_kc, tile=tile)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    rows = torch.tensor([0, M // 2 + 3, M - 1], device="cuda")           # and a few rows against fp32 arithmetic
    a = (A[rows].float() if a_kc else A[:, rows].float().t())
    ref = a @ (B.float().t() if b_kc else B.float())
    assert nerr(outs[0][rows], ref.cpu()) < 6e-3


def test_gemm_grouped_dw_4wave_equals_8phase_at_the_bench_size(hip):
    """the weight-gradient group of one interm_1b Block at per-GPU batch 16 (131072 tokens; dY / X of the MLP with the padded row
    pitch, 2.4-3.2 GB operands read K-strided): the grouped launch on the 4-wave kernel and on the 8-phase kernel, bit for bit"""
    T, D = 131072, 3072
    pad = lambda n: n + 64 if (2 * n) % 8192 == 0 else n
    g = torch.Generator(device="cuda").manual_seed(21)
    rnd = lambda c: (torch.randn(T, pad(c), device="cuda", generator=g) * 0.5).to(torch.bfloat16)[:, :c]
    res = {}
    shapes = ((3 * D, D), (D, D), (4 * D, D), (D, 4 * D))
    ops = [(rnd(no), rnd(ni)) for no, ni in shapes]
    for hint in (258, 256):
        probs = []
        for (dy, x), (no, ni) in zip(ops, shapes):
            out = torch.empty(no, ni, dtype=torch.bfloat16, device="cuda")
            probs.append((dy, x, out, no, ni, T, dy.stride(0), x.stride(0), ni, dict(a_kc=False, b_kc=False, tile=hint)))
        hip.gemm_grouped(probs)
        torch.cuda.synchronize()
        res[hint] = [p[2] for p in probs]
    for a, b in zip(res[258], res[256]):
        assert torch.equal(a, b)
    dy, x = ops[2]                                                        # a few entries of dW fc1 against fp32 dot products
    ref = dy[:, :4].float().t() @ x[:, :8].float()
    assert nerr(res[258][2][:4, :8], ref.cpu()) < 6e-3


def child_gemm_grouped_dw_with_cohort_pacing():
    """body of the next test (ORBIT2_W4_PACE is read once per process): the same comparison under pacing mode 2"""
    from climate_learn import _hip
    assert os.environ.get("ORBIT2_W4_PACE") == "2"
    test_gemm_grouped_dw_4wave_equals_8phase_at_the_bench_size(_hip)
    # mixed-length cohorts: problems of 2048 and 512 K-tiles in one launch (the balanced launch's shape) -- a workgroup that
    # leaves its sweep credits the cohort's counter, nobody waits out the poll budget; results = the single launches', bit for bit
    T, D = 131072, 3072
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda r, c: (torch.randn(r, c, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    dy, x = rnd(T, 1024), rnd(T, D)
    outs = [torch.empty(1024, D, dtype=torch.bfloat16, device="cuda") for _ in range(10)]
    q = T // 4
    probs = []
    for rep in range(2):                               # 10 problems = 480 tiles: two rounds, full and quarter sweeps in one cohort
        probs.append((dy, x, outs[5 * rep], 1024, D, T, 1024, D, D, dict(a_kc=False, b_kc=False)))
        probs += [(dy[i * q:(i + 1) * q], x[i * q:(i + 1) * q], outs[5 * rep + 1 + i], 1024, D, q, 1024, D, D, dict(a_kc=False, b_kc=False))
                  for i in range(4)]
    _hip.gemm_grouped(probs)
    torch.cuda.synchronize()
    ref = [torch.empty(1024, D, dtype=torch.bfloat16, device="cuda") for _ in range(10)]
    for (a, b, _, M, N, K, lda, ldb, ldc, kw), o in zip(probs, ref):
        _hip.gemm(a, b, o, M, N, K, lda, ldb, ldc, tile=256, **kw)
    torch.cuda.synchronize()
    for a, b in zip(outs, ref):
        assert torch.equal(a, b)


def test_gemm_grouped_dw_with_cohort_pacing():
    """ORBIT2_W4_PACE=2 (check points inside the sweep: generated code in the TN loop that the default mode jumps over): the
    bench-size weight-gradient group still equals the 8-phase kernel bit for bit, also with sweeps of different lengths in one
    cohort (the exit credit), and the launch ends (bounded polls)"""
    from tests._child import run_child
    run_child(__file__, "child_gemm_grouped_dw_with_cohort_pacing", timeout=600, env={"ORBIT2_W4_PACE": "2"})


def test_gemm_4wave_kernel_takes_whole_tiles_only(hip):
    A, B = bf(torch.randn(264, 128)).cuda(), bf(torch.randn(256, 128)).cuda()
    out = torch.empty(264, 256, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(Exception):
        hip.gemm(A, B, out, 264, 256, 128, 128, 128, 256, tile=260)
    hip.gemm(A, B, out, 264, 256, 128, 128, 128, 256)          # auto: the 8-phase / 128-tile kernels take it
    assert nerr(out, A.float().cpu() @ B.float().cpu().t()) < 6e-3


def test_gemm_grouped_4wave_matches_single_launches(hip):
    """a grouped launch of whole-tile problems runs on the 4-wave kernel: equal, bit for bit, to the same problems launched
    one by one on it, in every operand form, with a beta-accumulating member.  (Every member has two K-tiles or more: with a
    one-K-tile member the plan gives the whole group to the 128-tile kernel.)"""
    g = torch.Generator().manual_seed(78)
    for a_kc, b_kc in ((False, False), (True, True), (True, False), (False, True)):
        probs, refs = [], []
        for i, (M, N, K) in enumerate([(256, 512, 192), (768, 256, 128), (256, 256, 320), (512, 1024, 128)]):
            A = bf(torch.randn((M, K) if a_kc else (K, M), generator=g)).cuda()
            B = bf(torch.randn((N, K) if b_kc else (K, N), generator=g)).cuda()
            beta = 1.0 if i == 1 else 0.0
            c0 = bf(torch.randn(M, N, generator=g)).cuda()
            single = c0.clone()
            hip.gemm(A, B, single, M, N, K, A.shape[1], B.shape[1], N, a_kc=a_kc, b_kc=b_kc, beta=beta, tile=260)
            out = c0.clone()
            probs.append((A, B, out, M, N, K, A.shape[1], B.shape[1], N, dict(a_kc=a_kc, b_kc=b_kc, beta=beta, tile=258)))
            refs.append(single)
            ref32 = (A.float().cpu() if a_kc else A.float().cpu().t()) @ (B.float().cpu().t() if b_kc else B.float().cpu())
            assert nerr(single, ref32 + beta * c0.float().cpu()) < 8e-3
        hip.gemm_grouped(probs)
        torch.cuda.synchronize()
        for pr, ref in zip(probs, refs):
            assert torch.equal(pr[2], ref)


@pytest.mark.parametrize("form", ["tn", "nt", "nn", "tt"])
def test_gemm_grouped_8phase_matches_single_launches(hip, form):
    """hint 256 on the first problem gives the group to the 8-phase kernel: ragged M and N, two to five K-tiles, a
    beta-accumulating member; equal, bit for bit, to the same problems launched one by one under hint 256, the single launches
    within one bf16 rounding (plus that of the accumulated C) of the fp32 product, and the rows behind every output untouched"""
    g = torch.Generator().manual_seed(79)
    a_kc, b_kc = form[0] == "n", form[1] == "t"
    probs, refs = [], []
    for i, (M, N, K) in enumerate([(264, 520, 128), (256, 256, 192), (520, 264, 128), (256, 512, 64 * 5)]):
        A = bf(torch.randn((M, K) if a_kc else (K, M), generator=g)).cuda()
        B = bf(torch.randn((N, K) if b_kc else (K, N), generator=g)).cuda()
        beta = 1.0 if i == 2 else 0.0
        c0 = torch.full((M + 8, N), 7.0, dtype=torch.bfloat16, device="cuda")        # 8 guard rows
        c0[:M] = bf(torch.randn(M, N, generator=g)).cuda()
        single = c0.clone()
        hip.gemm(A, B, single, M, N, K, A.shape[1], B.shape[1], N, a_kc=a_kc, b_kc=b_kc, beta=beta, tile=256)
        out = c0.clone()
        probs.append((A, B, out, M, N, K, A.shape[1], B.shape[1], N, dict(a_kc=a_kc, b_kc=b_kc, beta=beta, tile=256)))
        refs.append(single)
        ref32 = (A.float().cpu() if a_kc else A.float().cpu().t()) @ (B.float().cpu().t() if b_kc else B.float().cpu())
        assert nerr(single[:M], ref32 + beta * c0[:M].float().cpu()) < 8e-3
    hip.gemm_grouped(probs)
    torch.cuda.synchronize()
    for pr, ref in zip(probs, refs):
        assert torch.equal(pr[2], ref)
        assert torch.all(pr[2][pr[3]:] == 7.0) and torch.all(ref[pr[3]:] == 7.0)


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("M", [12, 100, 301])
def test_gemm_any_row_count_when_a_is_k_contiguous(hip, M, tile):
    """M need not be a multiple of 8 when A is K-contiguous (rows are clamped at staging, masked at the store)"""
    N, K = 136, 128
    g = torch.Generator().manual_seed(M)
    A, B = rt(torch.randn(M, K, generator=g)), rt(torch.randn(N, K, generator=g))
    bias = rt(torch.randn(N, generator=g))
    guard = torch.full((M + 8, N), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.gemm(bf(A).cuda(), bf(B).cuda(), guard, M, N, K, K, K, N, bias=bf(bias).cuda(), act=2, tile=tile)
    assert nerr(guard[:M], torch.relu(A @ B.t() + bias)) < 6e-3
    assert torch.all(guard[M:] == 7.0)                      # nothing written past row M-1
    with pytest.raises(Exception):                          # still required for the K-strided A form
        hip.gemm(bf(A.t().contiguous()).cuda(), bf(B).cuda(), guard, M, N, K, M + (-M) % 8, K, N, a_kc=False)


@pytest.mark.parametrize("name,N,K,form", [("proj fwd", 1024, 1024, "nt"), ("fc2 fwd", 1024, 4096, "nt"), ("dX qkv", 1024, 3072, "nn"),
                                             ("dX fc1", 1024, 4096, "nn"), ("dX proj", 1024, 1024, "nn"), ("ragged K", 1000, 1000, "nt")])
def test_gemm_single_round_grids(hip, name, N, K, form):
    """the GEMMs of BASELINE configs[1] (interm_117m, 32x64 grid, batch 8: 4096 tokens) whose 128x128 tiles make ONE round of the
    chip (N = 1024: 256 tiles), as dispatched, with a bias + dropout epilogue, against the fp32 product"""
    M = 4096
    g = torch.Generator().manual_seed(N + K)
    A, B = rt(torch.randn(M, K, generator=g)), rt(torch.randn(N, K, generator=g) * 0.1)
    a_kc, b_kc = form[0] == "n", form[1] == "t"
    Ad, Bd = bf(A).cuda(), bf(B if b_kc else B.t().contiguous()).cuda()
    bias = bf(torch.randn(N, generator=g)).cuda()
    o = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(Ad, Bd, o, M, N, K, K, K if b_kc else N, N, a_kc=a_kc, b_kc=b_kc, bias=bias, drop_p=0.1, seed=11)
    torch.cuda.synchronize()
    mask, sc = keep_mask(11, M * N, 0.1)
    want = (A @ B.t() + bias.float().cpu()) * torch.from_numpy(mask).view(M, N) * sc
    assert nerr(o, want) < 6e-3
    # as dispatched these grids run on 64-ROW tiles (two workgroups per CU, round 5): the same bits as the 128 x 128 tiles
    o128, o64 = torch.empty_like(o), torch.empty_like(o)
    hip.gemm(Ad, Bd, o128, M, N, K, K, K if b_kc else N, N, a_kc=a_kc, b_kc=b_kc, bias=bias, drop_p=0.1, seed=11, tile=128)
    hip.gemm(Ad, Bd, o64, M, N, K, K, K if b_kc else N, N, a_kc=a_kc, b_kc=b_kc, bias=bias, drop_p=0.1, seed=11, tile=64)
    assert torch.equal(o, o64) and torch.equal(o64, o128)


@pytest.mark.parametrize("M,N,K,b_kc", [(64, 128, 64, True), (72, 136, 200, True), (1000, 384, 200, False), (130, 128, 128, False)])
def test_gemm_64_row_tiles_ragged(hip, M, N, K, b_kc):
    """tile hint 64 on ragged shapes: rows clamped at M, nothing written past them, bits equal to the 128 x 128 tiles"""
    g = torch.Generator().manual_seed(M + N + K)
    A, B = rt(torch.randn(M, K, generator=g)), rt(torch.randn(N, K, generator=g))
    Ad, Bd = bf(A).cuda(), bf(B if b_kc else B.t().contiguous()).cuda()
    res = bf(torch.randn(M, N, generator=g)).cuda()
    outs = []
    for tile in (128, 64):
        guard = torch.full((M + 70, N), 7.0, dtype=torch.bfloat16, device="cuda")
        hip.gemm(Ad, Bd, guard, M, N, K, K, K if b_kc else N, N, a_kc=True, b_kc=b_kc, act=1, residual=res, ldr=N, tile=tile)
        assert torch.all(guard[M:] == 7.0)
        outs.append(guard[:M].clone())
    assert torch.equal(outs[0], outs[1])
    assert nerr(outs[1], F.gelu(A @ B.t()) + res.float().cpu()) < 8e-3
    with pytest.raises(Exception):                          # the 64-row tile exists for a K-contiguous A only
        hip.gemm(bf(A.t().contiguous()).cuda(), Bd, guard, M, N, K, M + (-M) % 8, K if b_kc else N, N, a_kc=False, b_kc=b_kc, tile=64)


@pytest.mark.parametrize("form,K", [("tn", 70), ("tn", 201), ("tn", 64 + 35), ("nt", 72), ("nn", 136), ("tt", 40)])
def test_gemm_ragged_contraction_length(hip, form, K):
    """K need not be a multiple of the 64-wide k-step: the tail is staged from a zero page (weight-gradient form:
    K = number of tokens, any value; K-contiguous operands: K % 8 == 0)"""
    M, N = 136, 200
    g = torch.Generator().manual_seed(K)
    A, B = rt(torch.randn(M, K, generator=g)), rt(torch.randn(N, K, generator=g))
    a_kc, b_kc = form[0] == "n", form[1] == "t"
    Ad = bf(A if a_kc else A.t().contiguous()).cuda()
    Bd = bf(B if b_kc else B.t().contiguous()).cuda()
    out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    hip.gemm(Ad, Bd, out, M, N, K, K if a_kc else M, K if b_kc else N, N, a_kc=a_kc, b_kc=b_kc)
    assert nerr(out, A @ B.t()) < 2e-5


@pytest.mark.parametrize("form", ["tn", "nt", "nn", "tt"])
def test_gemm_grouped_matches_single_launches(hip, form):
    """one grouped launch == the same problems launched one by one (same kernel, same tile walk: bit-identical),
    with ragged tile counts and a beta-accumulating member"""
    g = torch.Generator().manual_seed(77)
    a_kc, b_kc = form[0] == "n", form[1] == "t"
    shapes = [(200, 136, 128), (384, 520, 192), (128, 128, 64), (72, 1032, 256)]
    probs, refs = [], []
    for i, (M, N, K) in enumerate(shapes):
        A = bf(torch.randn((M, K) if a_kc else (K, M), generator=g)).cuda()
        B = bf(torch.randn((N, K) if b_kc else (K, N), generator=g)).cuda()
        beta = 1.0 if i == 1 else 0.0
        c0 = bf(torch.randn(M, N, generator=g)).cuda()
        single = c0.clone()
        hip.gemm(A, B, single, M, N, K, A.shape[1], B.shape[1], N, a_kc=a_kc, b_kc=b_kc, beta=beta, tile=128)
        out = c0.clone()
        probs.append((A, B, out, M, N, K, A.shape[1], B.shape[1], N, dict(a_kc=a_kc, b_kc=b_kc, beta=beta)))
        refs.append(single)
        ref32 = (A.float().cpu() if a_kc else A.float().cpu().t()) @ (B.float().cpu().t() if b_kc else B.float().cpu())
        assert nerr(single, ref32 + beta * c0.float().cpu()) < 8e-3
    hip.gemm_grouped(probs)
    torch.cuda.synchronize()
    for pr, ref in zip(probs, refs):
        assert torch.equal(pr[2], ref)


@pytest.mark.parametrize("tile,M,N", [(128, 256, 192), (256, 256, 192), (260, 512, 256)])
def test_gemm_epilogue_full(hip, tile, M, N):
    K, L = 128, 64
    g = torch.Generator().manual_seed(5)
    A, W = rt(torch.randn(M, K, generator=g)), rt(torch.randn(N, K, generator=g) * 0.2)
    bias, res = rt(torch.randn(N, generator=g)), rt(torch.randn(L, N, generator=g))
    rs = torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.9, 1.0 / 0.9])
    p, seed = 0.1, 0xDEADBEEF12345
    pre = rt(A @ W.t() + bias)
    mask, sc = keep_mask(seed, M * N, p)
    mask = torch.from_numpy(mask).view(M, N)
    # order: +bias -> save_pre -> GELU -> dropout -> rowscale -> +residual(row % L)
    ref = F.gelu(pre) * mask * sc * rs.repeat_interleave(M // 4).view(M, 1) + res.repeat(M // L, 1)
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    sp = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(bf(A).cuda(), bf(W).cuda(), out, M, N, K, K, K, N, bias=bf(bias).cuda(), act=1, save_pre=sp, drop_p=p,
             seed=seed, rowscale=rs.cuda(), rows_per_scale=M // 4, residual=bf(res).cuda(), ldr=N, res_mod=L, tile=tile)
    assert nerr(sp, pre) < 6e-3
    assert nerr(out, ref) < 8e-3
    # res_first: dropout applied after the residual add (pos-embed path), beta accumulate, fp32 out
    ref2 = (A @ W.t() + bias + res.repeat(M // L, 1)) * mask * sc
    out2 = torch.ones(M, N, dtype=torch.float32, device="cuda")
    hip.gemm(bf(A).cuda(), bf(W).cuda(), out2, M, N, K, K, K, N, bias=bf(bias).cuda(), drop_p=p, seed=seed,
             residual=bf(res).cuda(), ldr=N, res_mod=L, res_first=True, beta=0.5, tile=tile)
    assert nerr(out2, ref2 + 0.5) < 1e-4
    out2b = torch.ones(M, N, dtype=torch.bfloat16, device="cuda")     # same through the bf16-output path
    hip.gemm(bf(A).cuda(), bf(W).cuda(), out2b, M, N, K, K, K, N, bias=bf(bias).cuda(), drop_p=p, seed=seed,
             residual=bf(res).cuda(), ldr=N, res_mod=L, res_first=True, beta=0.5, tile=tile)
    assert nerr(out2b, ref2 + 0.5) < 6e-3
    # dgelu epilogue: out = (A x W) * mask * gelu'(pre)
    dg = torch.empty(M, N, dtype=torch.float32, device="cuda")
    hip.gemm(bf(A).cuda(), bf(W).cuda(), dg, M, N, K, K, K, N, dgelu_pre=sp, drop_p=p, seed=seed, tile=tile)
    prq = sp.float().cpu().requires_grad_()
    F.gelu(prq).sum().backward()
    assert nerr(dg, (A @ W.t()) * mask * sc * prq.grad) < 1e-4
    dgb = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(bf(A).cuda(), bf(W).cuda(), dgb, M, N, K, K, K, N, dgelu_pre=sp, drop_p=p, seed=seed, tile=tile)
    assert nerr(dgb, (A @ W.t()) * mask * sc * prq.grad) < 6e-3
    # the same backward factor computed in the FORWARD (save_dact = GELU'(rounded pre) x dropout factor of the element) and
    # applied by a one-multiply epilogue (mul): the forward output is the save_pre path's bit for bit (GELU of the bf16-rounded
    # pre-activation either way), the product equals the dgelu path's up to the factor's 2^-15
    out_d = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    dact = torch.empty(M, N, dtype=torch.int16, device="cuda")       # the factor tensor is int16 fixed point, 14 fraction bits
    hip.gemm(bf(A).cuda(), bf(W).cuda(), out_d, M, N, K, K, K, N, bias=bf(bias).cuda(), act=1, save_dact=dact, drop_p=p,
             seed=seed, rowscale=rs.cuda(), rows_per_scale=M // 4, residual=bf(res).cuda(), ldr=N, res_mod=L, tile=tile)
    assert torch.equal(out_d, out)
    dact_f = dact.float().cpu() / 16384.0
    with pytest.raises(Exception):                                   # a bf16 tensor is not a factor tensor
        hip.gemm(bf(A).cuda(), bf(W).cuda(), out_d, M, N, K, K, K, N, mul=torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), tile=tile)
    assert nerr(dact_f, prq.grad * mask * sc) < 3e-3
    dm = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(bf(A).cuda(), bf(W).cuda(), dm, M, N, K, K, K, N, mul=dact, tile=tile)
    assert nerr(dm, (A @ W.t()) * dact_f) < 6e-3 and nerr(dm, dgb) < 8e-3
    with pytest.raises(Exception):
        hip.gemm(bf(A).cuda(), bf(W).cuda(), dm, M, N, K, K, K, N, mul=dact, dgelu_pre=sp, tile=tile)     # one or the other
    with pytest.raises(Exception):
        hip.gemm(bf(A).cuda(), bf(W).cuda(), dm, M, N, K, K, K, N, save_dact=dact, tile=tile)              # needs act = GELU


@pytest.mark.parametrize("tile", [128, 256, 260])
def test_gemm_save_dact_range(hip, tile):
    """the q14 factor tensor (save_dact) holds [-2, 2): at drop_p = 0.4 (scale 1.67, factor up to 1.88) it is exact to 2^-15
    and large positive pre-activations keep their sign; drop_p >= 0.434 (1.13 x scale >= 2 would wrap) is refused"""
    M, N, K = 256, 256, 128
    g = torch.Generator().manual_seed(15)
    A, W = rt(torch.randn(M, K, generator=g)), rt(torch.randn(N, K, generator=g) * 0.3)
    bias = rt(torch.randn(N, generator=g) + 1.0)
    p, seed = 0.4, 0x1234567
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    dact = torch.empty(M, N, dtype=torch.int16, device="cuda")
    hip.gemm(bf(A).cuda(), bf(W).cuda(), out, M, N, K, K, K, N, bias=bf(bias).cuda(), act=1, save_dact=dact, drop_p=p, seed=seed,
             tile=tile)
    pre = rt(A @ W.t() + bias).requires_grad_()
    F.gelu(pre).sum().backward()
    mask, sc = keep_mask(seed, M * N, p)
    mask = torch.from_numpy(mask).view(M, N)
    fac = dact.float().cpu() / 16384.0
    want = pre.grad * mask * sc
    assert want.max() > 1.8 and (fac - want).abs().max() < 2e-4          # no wrap: the largest factors keep their sign
    for bad in (0.44, 0.5, 0.9):
        with pytest.raises(Exception):
            hip.gemm(bf(A).cuda(), bf(W).cuda(), out, M, N, K, K, K, N, bias=bf(bias).cuda(), act=1, save_dact=dact, drop_p=bad,
                     seed=seed, tile=tile)


@pytest.mark.parametrize("K", [128, 448])
def test_gemm_4wave_compile_time_epilogues(hip, K):
    """the three hot epilogue combinations of the Block have straight-line (compile-time) epilogues on the 4-wave kernel
    (csrc/gemm.hip w4_epi_kind: 1 = bias + GELU + saved GELU' factor + dropout, 2 = bias + dropout + per-sample row scale +
    residual, 3 = x saved factor on the NN form): each must equal, bit for bit, the same kernel's runtime epilogue (hint 262) and
    the 8-phase kernel (256) -- outputs AND the stored factor tensor; padded row pitches as in the step"""
    M, N, rps = 768, 512, 256
    g = torch.Generator().manual_seed(31 + K)
    A, W = bf(torch.randn(M, K, generator=g)).cuda(), bf(torch.randn(N, K, generator=g) * 0.3).cuda()
    bias = bf(torch.randn(N, generator=g)).cuda()
    res = torch.zeros(M, N + 64, dtype=torch.bfloat16, device="cuda")
    res[:, :N] = bf(torch.randn(M, N, generator=g)).cuda()
    rs = (torch.rand(M // rps, generator=g) + 0.5).cuda()
    ldc = N + 64
    got = {}
    for tile in (260, 262, 256):
        o1 = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
        d1 = torch.zeros(M, ldc, dtype=torch.int16, device="cuda")
        hip.gemm(A, W, o1, M, N, K, K, K, ldc, bias=bias, act=1, save_dact=d1, drop_p=0.1, seed=77, tile=tile)
        o2 = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
        hip.gemm(A, W, o2, M, N, K, K, K, ldc, bias=bias, drop_p=0.1, seed=78, rowscale=rs, rows_per_scale=rps, residual=res,
                 ldr=N + 64, tile=tile)
        # kind 3: dX[M, K2] = dY[M, N] . Wt[N, K2] (the stored weight is the K-strided operand) x factor
        K2 = 256
        Wt = bf(torch.randn(N, K2, generator=torch.Generator().manual_seed(5)) * 0.3).cuda()
        o3 = torch.zeros(M, K2 + 64, dtype=torch.bfloat16, device="cuda")
        fac = torch.zeros(M, K2 + 64, dtype=torch.int16, device="cuda")
        fac[:, :K2] = torch.randint(-2000, 20000, (M, K2), generator=torch.Generator().manual_seed(6), dtype=torch.int16).cuda()
        hip.gemm(o2[:, :N], Wt, o3, M, K2, N, ldc, K2, K2 + 64, a_kc=True, b_kc=False, mul=fac, tile=tile)
        # the same kinds without dropout / without the row scale (layers with drop-path rate 0, the head's MLP)
        o4 = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
        d4 = torch.zeros(M, ldc, dtype=torch.int16, device="cuda")
        hip.gemm(A, W, o4, M, N, K, K, K, ldc, bias=bias, act=1, save_dact=d4, drop_p=0.0, seed=0, tile=tile)
        o5 = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
        hip.gemm(A, W, o5, M, N, K, K, K, ldc, bias=bias, drop_p=0.1, seed=79, residual=res, ldr=N + 64, tile=tile)
        got[tile] = (o1, d1, o2, o3, o4, d4, o5)
    torch.cuda.synchronize()
    for other in (262, 256):
        for x, y in zip(got[260], got[other]):
            assert torch.equal(x, y)
    # and against the fp32 restatement (kind 2; kinds 1 / 3 are covered by test_gemm_epilogue_full / test_gemm_save_dact_range
    # through the same epi8_finish)
    mask, sc = keep_mask(78, M * N, 0.1)
    want = res[:, :N].float().cpu() + rs.cpu().repeat_interleave(rps)[:, None] * \
        (A.float().cpu() @ W.float().cpu().t() + bias.float().cpu()) * torch.from_numpy(mask).view(M, N) * sc
    assert nerr(got[260][2][:, :N], want) < 6e-3


def test_gemm_fused_column_sums(hip):
    """the factor-multiply input gradient on the 4-wave kernel (epilogue kind 3) also leaves, per tile row, the column sums of the
    output it STORED (ABI 5 colsum_ws: fc1's bias gradient without a second pass over dpre): each workspace row against the sum of
    that tile row's 256 bf16 output rows, the output itself bit-identical to the call without the workspace; calls that cannot
    fuse say so (no workspace) and the caller falls back to orbit2_colsum"""
    M, N, K = 768, 512, 192
    g = torch.Generator().manual_seed(41)
    dy = bf(torch.randn(M, K, generator=g)).cuda()
    Wt = bf(torch.randn(K, N, generator=g) * 0.3).cuda()
    ldc = N + 64
    fac = torch.zeros(M, ldc, dtype=torch.int16, device="cuda")
    fac[:, :N] = torch.randint(-2000, 20000, (M, N), generator=g, dtype=torch.int16).cuda()
    plain = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
    hip.gemm(dy, Wt, plain, M, N, K, K, N, ldc, a_kc=True, b_kc=False, mul=fac, tile=260)
    out = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
    o2, parts = hip.gemm(dy, Wt, out, M, N, K, K, N, ldc, a_kc=True, b_kc=False, mul=fac, tile=260, want_colsum=True)
    torch.cuda.synchronize()
    assert parts is not None and parts.shape == (M // 256, N) and torch.equal(out, plain)
    want = out[:, :N].float().view(M // 256, 256, N).sum(1)
    assert (parts - want).abs().max() <= 1e-4 * want.abs().max()
    # not fusable: the 8-phase kernel, a bias, a ragged tile count -> no workspace, same output
    for kw in (dict(tile=256), dict(tile=260, bias=bf(torch.randn(N, generator=g)).cuda())):
        o3 = torch.zeros(M, ldc, dtype=torch.bfloat16, device="cuda")
        _, p3 = hip.gemm(dy, Wt, o3, M, N, K, K, N, ldc, a_kc=True, b_kc=False, mul=fac, want_colsum=True, **kw)
        assert p3 is None and ("bias" in kw or torch.equal(o3, plain))


@pytest.mark.parametrize("tile", [128, 256, 260])
def test_gemm_column_scale(hip, tile):
    """colscale epilogue (the qkv Linear's q third times log2(e)/sqrt(d)): columns n < colscale_n are multiplied in fp32
    right after the bias -- one rounding to bf16 -- the rest are untouched bit for bit; fp32 and bf16 outputs"""
    M, N, K, n0, c = 256, 512, 128, 128, 0.12752041
    g = torch.Generator().manual_seed(6)
    A, W, bias = rt(torch.randn(M, K, generator=g)), rt(torch.randn(N, K, generator=g) * 0.2), rt(torch.randn(N, generator=g))
    ref = A @ W.t() + bias
    ref[:, :n0] *= c
    plain = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(bf(A).cuda(), bf(W).cuda(), plain, M, N, K, K, K, N, bias=bf(bias).cuda(), tile=tile)
    for dt, tol in ((torch.float32, 1e-5), (torch.bfloat16, 6e-3)):
        out = torch.empty(M, N, dtype=dt, device="cuda")
        hip.gemm(bf(A).cuda(), bf(W).cuda(), out, M, N, K, K, K, N, bias=bf(bias).cuda(), tile=tile, colscale=(n0, c))
        assert nerr(out[:, :n0], ref[:, :n0]) < tol and nerr(out[:, n0:], ref[:, n0:]) < tol
        if dt == torch.bfloat16:
            assert torch.equal(out[:, n0:], plain[:, n0:])
            # ONE rounding: bf16(fp32 value * c), not bf16(bf16(value) * c)
            assert torch.equal(out[:, :n0].cpu(), bf((A @ W.t() + bias)[:, :n0] * c)) or nerr(out[:, :n0], ref[:, :n0]) < 4e-3
    with pytest.raises(hip.HipBackendError):
        hip.gemm(bf(A).cuda(), bf(W).cuda(), plain, M, N, K, K, K, N, colscale=(4, c))      # not a multiple of 8


def test_dropout_statistics(hip):
    M, N = 512, 1024
    dy = torch.ones(M, N, dtype=torch.bfloat16, device="cuda")
    out = hip.dropout_bwd(dy, M, N, 0.1, 1234567)
    keep = (out.float() > 0).float().mean().item()
    assert abs(keep - (1 - 26 / 256)) < 3e-3
    mask, sc = keep_mask(1234567, M * N, 0.1)
    assert torch.equal((out.float().cpu() > 0).view(-1), torch.from_numpy(mask) > 0)


def test_sgemm(hip):
    g = torch.Generator().manual_seed(3)
    for (M, N, K, ta, tb) in [(115, 96, 200, 0, 0), (70, 130, 64, 1, 0), (33, 65, 100, 0, 1), (64, 64, 64, 1, 1)]:
        A = torch.randn((K, M) if ta else (M, K), generator=g)
        B = torch.randn((N, K) if tb else (K, N), generator=g)
        ref = (A.t() if ta else A) @ (B.t() if tb else B)
        out = torch.empty(M, N, device="cuda")
        hip.sgemm(A.cuda(), B.cuda(), out, M, N, K, A.shape[1], B.shape[1], N, ta=ta, tb=tb)
        assert nerr(out, ref) < 1e-5
    # skinny products against a wide weight are split over K (workspace slabs + deterministic combine)
    for (M, N, K, ta, tb) in [(24, 3072, 3072, 0, 0), (115, 1536, 3000, 0, 1), (1, 512, 4096, 0, 1), (24, 640, 2048, 1, 0),
                              (115, 96, 8192, 1, 1)]:
        assert hip.lib().orbit2_sgemm_f32_ws_floats(M, N, K) > 0
        A = torch.randn((K, M) if ta else (M, K), generator=g)
        B = torch.randn((N, K) if tb else (K, N), generator=g)
        C0 = torch.randn(M, N, generator=g)
        ref = 0.5 * ((A.t() if ta else A).double() @ (B.t() if tb else B).double()).float() + 2.0 * C0
        out = C0.clone().cuda()
        hip.sgemm(A.cuda(), B.cuda(), out, M, N, K, A.shape[1], B.shape[1], N, ta=ta, tb=tb, alpha=0.5, beta=2.0)
        assert nerr(out, ref) < 1e-5
        again = C0.clone().cuda()
        hip.sgemm(A.cuda(), B.cuda(), again, M, N, K, A.shape[1], B.shape[1], N, ta=ta, tb=tb, alpha=0.5, beta=2.0)
        assert torch.equal(out, again)                     # no atomics: bit-reproducible


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,rows", [(64, 200), (256, 200), (1024, 200), (3072, 200), (5120, 200), (8192, 200),
                                    (256, 33000), (1024, 33000), (3072, 33000), (2048, 33000)])
def test_layernorm(hip, D, rows):
    """the backward has a per-wave and a row-shared form, each with a few-rows (< 32768) and a many-rows partition"""
    g = torch.Generator().manual_seed(D)
    x = rt(torch.randn(rows, D, generator=g) * 2 + 0.5)
    gam, bet = rt(1 + 0.1 * torch.randn(D, generator=g)), rt(0.1 * torch.randn(D, generator=g))
    dy, dres = rt(torch.randn(rows, D, generator=g)), rt(torch.randn(rows, D, generator=g))
    xr, gr, br = x.clone().requires_grad_(), gam.clone().requires_grad_(), bet.clone().requires_grad_()
    yr = F.layer_norm(xr, (D,), gr, br, 1e-5)
    yr.backward(dy)
    y, mean, rstd = hip.layernorm_fwd(bf(x).cuda(), bf(gam).cuda(), bf(bet).cuda())
    assert nerr(y, yr) < 6e-3
    dg = torch.empty(D, device="cuda"); db = torch.empty(D, device="cuda")
    dx = hip.layernorm_bwd(bf(dy).cuda(), bf(x).cuda(), bf(gam).cuda(), mean, rstd, bf(dres).cuda(), dg, db)
    assert nerr(dx, xr.grad + dres) < 8e-3
    assert nerr(dg, gr.grad) < 1e-3 and nerr(db, br.grad) < 1e-3


# ---------------------------------------------------------------------------------------------
def _attn_ref(qkv, B, L, H, d, mask=None, sc=1.0):
    q, k, v = qkv.view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    a = ((q * d ** -0.5) @ k.transpose(-2, -1)).softmax(-1)
    if mask is not None:
        a = a * mask * sc
    return (a @ v).transpose(1, 2).reshape(B, L, H * d)


@pytest.mark.parametrize("d,H,L,B", [(64, 2, 128, 2), (128, 2, 256, 1), (64, 4, 512, 1), (128, 3, 384, 2), (256, 2, 128, 1), (256, 1, 256, 2),
                                       (128, 2, 200, 1), (64, 2, 578, 2), (128, 1, 70, 2), (256, 1, 161, 1), (128, 2, 300, 1)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_fwd_bwd(hip, d, H, L, B, p):
    g = torch.Generator().manual_seed(d + L)
    qkv = rt(torch.randn(B, L, 3 * H * d, generator=g)).requires_grad_()
    do = rt(torch.randn(B, L, H * d, generator=g))
    seed = 99887766
    mask, sc = None, 1.0
    if p > 0:
        m, sc = attn_keep_mask(seed, B * H, L, p)
        mask = torch.from_numpy(m).view(B, H, L, L)
    ref = _attn_ref(qkv, B, L, H, d, mask, sc)
    ref.backward(do)
    qd = bf(qkv.detach()).cuda()
    out, lse = hip.attn_fwd(qd, B, L, H, d, p, seed)
    assert nerr(out, ref) < 1e-2
    q, k, _ = qkv.detach().view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    lse_ref = torch.logsumexp((q * d ** -0.5) @ k.transpose(-2, -1), dim=-1)
    assert nerr(lse, lse_ref) < 1e-3
    dqkv = hip.attn_bwd(qd, out, bf(do).cuda(), lse, B, L, H, d, p, seed)
    gr = qkv.grad.view(B, L, 3, H * d)
    dv = dqkv.view(B, L, 3, H * d)
    for i, nm in enumerate("qkv"):
        assert nerr(dv[:, :, i], gr[:, :, i]) < 2e-2, nm


@pytest.mark.parametrize("d,L", [(128, 256), (128, 257), (128, 300), (128, 320), (128, 511), (128, 513), (128, 1024 + 96), (128, 2048),
                                 (256, 20), (256, 128), (256, 161), (256, 289), (256, 300), (256, 512), (256, 1000)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_dkv_one_pass_equals_two_passes(hip, d, L, p):
    """dK and dV come from ONE pass at d = 128 (>= 256 tokens: V rows in LDS, csrc/attn.hip attn_bwd_dkv128_kernel) and -- round
    3 -- at d = 256 (attn_bwd_dkv256_kernel: 32-row query tiles, one wave per SIMD); the two-pass kernels stay selectable
    (flag ORBIT2_ATTN_SPLIT_DKV of orbit2_attn_bwd_ld) and must give the same bits -- odd tile counts (the pair loop's last
    tile is past the end) and ragged tails included"""
    B, H = 2, (3 if d == 128 else 2)
    g = torch.Generator().manual_seed(L)
    qkv = bf(torch.randn(B, L, 3 * H * d, generator=g) * 0.7).cuda()
    do = bf(torch.randn(B, L, H * d, generator=g)).cuda()
    out, lse = hip.attn_fwd(qkv, B, L, H, d, p, 4242)
    one = hip.attn_bwd(qkv, out, do, lse, B, L, H, d, p, 4242)
    two = hip.attn_bwd(qkv, out, do, lse, B, L, H, d, p, 4242, flags=hip.ATTN_SPLIT_DKV)
    assert torch.equal(one, two)


LOG2E = 1.4426950408889634


def _prescale_q(qkv, B, L, H, d):
    """what the qkv GEMM's colscale epilogue stores: the q third times log2(e)/sqrt(d), rounded to bf16 ONCE; returns
    (stored tensor, the fp32 qkv it represents exactly)"""
    x = qkv.view(B, L, 3, H * d).clone()
    x[:, :, 0] = (x[:, :, 0] * (LOG2E / d ** 0.5)).to(torch.bfloat16).float()
    stored = x.reshape(B, L, 3 * H * d)
    eff = x.clone()
    eff[:, :, 0] = eff[:, :, 0] / (LOG2E / d ** 0.5)
    return bf(stored), eff.reshape(B, L, 3 * H * d)


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("mult,min_jump_bits", [(60.0, 8.0), (1200.0, 45.0), (4000.0, 130.0)])
def test_attention_forced_late_rescale(hip, mult, min_jump_bits, prescaled):
    """The no-dropout forward keeps ONE reference per row (its maximum over the first 64 keys) while the probabilities
    relative to it stay below 2^40 (csrc/attn.hip FAST_LIMIT) and drops to an online-softmax loop with a moving reference
    (RESCALE_THR) once they do not.  Force both: one key far down the sequence matches every query strongly, so the row
    maximum jumps there by ~11 bits (stays on the fixed reference: probabilities up to 2^11), by ~66 bits (the guard trips)
    and by > 128 bits (exp2 overflows to inf in the fast loop before the guard trips).
    prescaled: q stored as q * log2(e)/sqrt(d) (flag ORBIT2_ATTN_Q_PRESCALED, what the model's qkv GEMM writes): exact
    products, tight tolerance.  Raw q: the kernel rounds q * log2(e)/sqrt(d) to bf16 itself, a second rounding whose effect on
    a score grows with the score (~2^-9 |s| / sqrt(d)): at these artificial magnitudes (tens to hundreds of nats) percents."""
    B, L, H, d = 1, 512, 2, 128
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(B, L, 3, H, d, generator=g) * 0.5
    qkv[:, 300, 1] = qkv[:, :, 0].mean(1) * mult + 3.0        # a key aligned with the mean query, scaled up
    qkv[:, 450, 1] *= 12.0
    qkv = rt(qkv.reshape(B, L, 3 * H * d))
    if prescaled:
        stored, qkv = _prescale_q(qkv, B, L, H, d)
        out, lse = hip.attn_fwd(stored.cuda(), B, L, H, d, 0.0, 0, flags=hip.ATTN_Q_PRESCALED)
    else:
        out, lse = hip.attn_fwd(bf(qkv).cuda(), B, L, H, d, 0.0, 0)
    ref = _attn_ref(qkv, B, L, H, d)
    q, k, _ = qkv.view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    sc = (q * d ** -0.5) @ k.transpose(-2, -1)
    jump_bits = float((sc.max(-1).values - sc[..., :64].max(-1).values).max()) * LOG2E
    assert jump_bits > min_jump_bits     # the maximum really jumps that late, by that much (exp2 domain)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert nerr(out, ref) < (1e-2 if prescaled else 8e-2)
    assert nerr(lse, torch.logsumexp(sc, -1)) < (1e-3 if prescaled else 3e-3)


@pytest.mark.parametrize("H,L,B", [(2, 256, 1), (3, 512, 2), (1, 1024, 1), (2, 768, 2)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_fwd_generated_kernel(hip, H, L, B, p):
    """d = 128, q pre-scaled, L % 256 == 0: the forward is the generated one-wave-per-SIMD kernel (csrc/attn_fwd_asm.h).  Against
    the oracle with the kernels' own dropout mask, against the compiler-scheduled kernel (flag ORBIT2_ATTN_NO_W4: same math,
    other summation order), bit-repeatable, and its lse drives the unchanged backward."""
    d = 128
    g = torch.Generator().manual_seed(17 * H + L)
    stored, eff = _prescale_q(rt(torch.randn(B, L, 3 * H * d, generator=g)), B, L, H, d)
    eff.requires_grad_()
    do = rt(torch.randn(B, L, H * d, generator=g))
    seed = 0x5EED0000 + L
    mask, sc = None, 1.0
    if p > 0:
        m, sc = attn_keep_mask(seed, B * H, L, p)
        mask = torch.from_numpy(m).view(B, H, L, L)
    ref = _attn_ref(eff, B, L, H, d, mask, sc)
    ref.backward(do)
    sd = stored.cuda()
    out, lse = hip.attn_fwd(sd, B, L, H, d, p, seed, flags=hip.ATTN_Q_PRESCALED)
    old, lse_old = hip.attn_fwd(sd, B, L, H, d, p, seed, flags=hip.ATTN_Q_PRESCALED | hip.ATTN_NO_W4)
    assert nerr(out, ref) < 1e-2
    q, k, _ = eff.detach().view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    assert nerr(lse, torch.logsumexp((q * d ** -0.5) @ k.transpose(-2, -1), dim=-1)) < 1e-3
    assert nerr(out, old) < 8e-3 and float((lse - lse_old).abs().max()) < 1e-4
    again, lse2 = hip.attn_fwd(sd, B, L, H, d, p, seed, flags=hip.ATTN_Q_PRESCALED)
    assert torch.equal(out, again) and torch.equal(lse, lse2)
    dqkv = hip.attn_bwd(sd, out, bf(do).cuda(), lse, B, L, H, d, p, seed, flags=hip.ATTN_Q_PRESCALED)
    gr = eff.grad.view(B, L, 3, H * d)
    dv = dqkv.view(B, L, 3, H * d)
    for i, nm in enumerate("qkv"):
        assert nerr(dv[:, :, i], gr[:, :, i]) < 2e-2, nm


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mult", [60.0, 1200.0, 4000.0])
def test_attention_fwd_generated_kernel_fixup(hip, mult, p):
    """the generated forward keeps one reference per row (its maximum over the first 64 keys); a tile whose half-row sums leave
    [0, 2^40] branches to the fix-up (reference moved, O / l rescaled, the tile's probabilities redone with the same dropout
    mask).  One late key matches every query strongly: +11 bits (no fix-up), +66 bits, > 128 bits (exp2 gives inf first)."""
    B, L, H, d = 1, 512, 2, 128
    g = torch.Generator().manual_seed(78)
    qkv = torch.randn(B, L, 3, H, d, generator=g) * 0.5
    qkv[:, 300, 1] = qkv[:, :, 0].mean(1) * mult + 3.0
    qkv[:, 450, 1] *= 12.0
    stored, eff = _prescale_q(rt(qkv.reshape(B, L, 3 * H * d)), B, L, H, d)
    seed = 31337
    mask, sc = None, 1.0
    if p > 0:
        m, sc = attn_keep_mask(seed, B * H, L, p)
        mask = torch.from_numpy(m).view(B, H, L, L)
    ref = _attn_ref(eff, B, L, H, d, mask, sc)
    out, lse = hip.attn_fwd(stored.cuda(), B, L, H, d, p, seed, flags=hip.ATTN_Q_PRESCALED)
    q, k, _ = eff.view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    scr = (q * d ** -0.5) @ k.transpose(-2, -1)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert nerr(out, ref) < 1e-2
    assert nerr(lse, torch.logsumexp(scr, -1)) < 1e-3


@pytest.mark.parametrize("d,H,L,B", [(64, 2, 192, 2), (128, 3, 384, 1), (128, 2, 300, 1), (256, 1, 161, 1)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_q_prescaled(hip, d, H, L, B, p):
    """flag ORBIT2_ATTN_Q_PRESCALED: the q third of qkv holds q * log2(e)/sqrt(d) (the qkv GEMM's colscale epilogue);
    out / lse are those of the q it represents, dqkv is the gradient with respect to the UNSCALED q, k, v"""
    g = torch.Generator().manual_seed(3 * d + L)
    stored, eff = _prescale_q(rt(torch.randn(B, L, 3 * H * d, generator=g)), B, L, H, d)
    eff.requires_grad_()
    do = rt(torch.randn(B, L, H * d, generator=g))
    seed = 424242
    mask, sc = None, 1.0
    if p > 0:
        m, sc = attn_keep_mask(seed, B * H, L, p)
        mask = torch.from_numpy(m).view(B, H, L, L)
    ref = _attn_ref(eff, B, L, H, d, mask, sc)
    ref.backward(do)
    out, lse = hip.attn_fwd(stored.cuda(), B, L, H, d, p, seed, flags=hip.ATTN_Q_PRESCALED)
    assert nerr(out, ref) < 1e-2
    q, k, _ = eff.detach().view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    assert nerr(lse, torch.logsumexp((q * d ** -0.5) @ k.transpose(-2, -1), dim=-1)) < 1e-3
    dqkv = hip.attn_bwd(stored.cuda(), out, bf(do).cuda(), lse, B, L, H, d, p, seed, flags=hip.ATTN_Q_PRESCALED)
    gr = eff.grad.view(B, L, 3, H * d)
    dv = dqkv.view(B, L, 3, H * d)
    for i, nm in enumerate("qkv"):
        assert nerr(dv[:, :, i], gr[:, :, i]) < 2e-2, nm
    # both variants of the d = 128 dK+dV pass agree bit for bit with the flag as well
    if d == 128 and L >= 256:
        two = hip.attn_bwd(stored.cuda(), out, bf(do).cuda(), lse, B, L, H, d, p, seed,
                           flags=hip.ATTN_Q_PRESCALED | hip.ATTN_SPLIT_DKV)
        assert torch.equal(dqkv, two)


# ---------------------------------------------------------------------------------------------
def _tables(sd, heads, ids, D):
    """fp32 table algebra of the folded variable aggregation (see csrc/varagg.hip header)."""
    dh = D // heads
    Wq, Wkv = sd["var_agg.q.weight"], sd["var_agg.kv.weight"]
    Wk, Wv = Wkv[:D], Wkv[D:]
    qv = (sd["var_query"].view(1, D) @ Wq.t()).view(D)
    U = torch.stack([(qv[h * dh:(h + 1) * dh, None] * Wk[h * dh:(h + 1) * dh]).sum(0) for h in range(heads)]) * dh ** -0.5
    cm = []
    for v in ids:
        w = sd["token_embeds.%d.proj.weight" % v].view(D, 4)
        c = sd["token_embeds.%d.proj.bias" % v] + sd["var_embed"][0, v]
        cm.append(torch.cat([w.t(), c.view(1, D)], 0))      # [5, D]
    cm = torch.stack(cm)                                     # [V, 5, D]
    stab = torch.einsum("hd,vcd->hvc", U, cm)
    gtab = torch.einsum("vcd,id->vci", cm, Wv)
    return stab.contiguous(), gtab.contiguous()


@pytest.mark.parametrize("D,heads,V,hw", [(64, 4, 5, (8, 16)), (256, 4, 23, (16, 32)), (384, 3, 7, (12, 20)),
                                           (256, 2, 25, (32, 64)), (512, 2, 5, (8, 16)), (256, 4, 30, (8, 16)),
                                           (64, 4, 5, (6, 10)), (256, 4, 30, (6, 10))])    # 30 tokens: a partial workgroup of the scalar backward
def test_varagg_fold_matches_dense_oracle(hip, D, heads, V, hw):
    cfg = O.Config(["v%d" % i for i in range(V + 2)], hw, 1, D, 1, 1, heads)
    sd = O.init_state_dict(cfg, V, seed=1)
    g = torch.Generator().manual_seed(11)
    for k in ("var_embed", "var_query"):
        sd[k] = torch.randn(sd[k].shape, generator=g) * 0.5
    for k in list(sd):
        if k.startswith("var_agg") or k.startswith("token_embeds"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * (0.3 if "token" in k else 0.15)
    ids = list(range(1, V + 1))
    B = 2
    x = torch.randn(B, V, *hw, generator=g)
    leaves = {k: sd[k].clone().requires_grad_() for k in sd if k.startswith(("var_", "token_embeds"))}
    toks = [O.patch_embed(x[:, i:i + 1], leaves["token_embeds.%d.proj.weight" % v],
                          leaves["token_embeds.%d.proj.bias" % v], 2) for i, v in enumerate(ids)]
    t = torch.stack(toks, 1) + leaves["var_embed"][:, ids].unsqueeze(2)
    # dense oracle up to (but excluding) proj: use identity proj to expose z
    eye, zero = torch.eye(D), torch.zeros(D)
    zref = O.variable_aggregation(t, leaves["var_query"], leaves["var_agg.q.weight"], leaves["var_agg.kv.weight"],
                                  eye, zero, heads)
    L = zref.shape[1]
    dz = rt(torch.randn(B * L, D, generator=g))
    zref.reshape(B * L, D).backward(dz)
    # folded path: tables (autograd on CPU for the reference grads of the tables), kernel on GPU
    leaves2 = {k: sd[k].clone().requires_grad_() for k in leaves}
    stab, gtab = _tables(leaves2, heads, ids, D)
    z, attw = hip.varagg_fwd(x.cuda(), stab.detach().cuda(), gtab.detach().cuda(), heads, D)
    assert nerr(z, zref.reshape(B * L, D)) < 6e-3
    dstab, dgtab = hip.varagg_bwd(x.cuda(), gtab.detach().cuda(), attw, bf(dz).cuda(), heads, D)
    torch.autograd.backward([stab, gtab], [dstab.cpu(), dgtab.cpu()])
    for k in leaves:
        if leaves[k].grad is None:
            continue
        # head dims 64/128/256 take the MFMA backward: fp32 operands enter as bf16 hi+lo pairs (fp32-grade result)
        assert nerr(leaves2[k].grad, leaves[k].grad) < 5e-5, k


# ---------------------------------------------------------------------------------------------
def test_unpatchify(hip):
    B, C, h, w, p, s = 2, 3, 8, 16, 2, 4
    g = torch.Generator().manual_seed(2)
    t = rt(torch.randn(B, h * w // 4, C * 64, generator=g))
    ref = O.unpatchify(t, (h, w), p, s, C)
    img = hip.unpatchify_fwd(bf(t).cuda(), B, C, h, w, p, s)
    assert torch.equal(img.cpu(), ref)
    dimg = rt(torch.randn(ref.shape, generator=g))
    tr = t.clone().requires_grad_()
    O.unpatchify(tr, (h, w), p, s, C).backward(dimg)
    dt = hip.unpatchify_bwd(dimg.cuda(), B, C, h, w, p, s)
    assert torch.equal(dt.float().cpu(), tr.grad)


@pytest.mark.parametrize("mode", [0, 1])
def test_conv3x3(hip, mode):
    g = torch.Generator().manual_seed(9 + mode)
    B, ctot, H, W = 2, 9, 12, 20
    Cin, Cout, r = (7, 64, 4) if mode else (4, 3, 1)
    idx = torch.tensor([8, 2, 0, 5, 4, 1, 7][:Cin], dtype=torch.int32)
    x = torch.randn(B, ctot, H, W, generator=g)
    wgt = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2).requires_grad_()
    b = torch.randn(Cout, generator=g).requires_grad_()
    xs = x[:, idx.long()].clone().requires_grad_()
    y = F.conv2d(xs, wgt, b, padding=1)
    add = None
    if mode:
        yr = F.pixel_shuffle(F.gelu(y), r)
    else:
        add = torch.randn(B, Cout, H + 3, W + 2, generator=g)
        yr = y + add[:, :, :H, :W]
    do = torch.randn(yr.shape, generator=g)
    yr.backward(do)
    out, pre = hip.conv3x3_fwd(x.cuda(), idx.cuda(), wgt.detach().cuda(), b.detach().cuda(), mode, r,
                               None if add is None else add.cuda())
    assert nerr(out, yr) < 1e-5
    din, dw, db = hip.conv3x3_bwd(do.cuda(), x.cuda(), idx.cuda(), wgt.detach().cuda(), pre, True, mode, r)
    assert nerr(din, xs.grad) < 1e-5 and nerr(dw, wgt.grad) < 1e-4 and nerr(db, b.grad) < 1e-4


@pytest.mark.parametrize("kind", ["mse", "bayesian_tv"])
@pytest.mark.parametrize("lat", [False, True])
def test_loss(hip, kind, lat):
    g = torch.Generator().manual_seed(4)
    B, C, H, W = 2, 3, 24, 40
    pred = torch.randn(B, C, H, W, generator=g).requires_grad_()
    tgt = torch.randn(B, C, H + 5, W + 7, generator=g)
    names = ["total_precipitation_24hr", "2m_temperature_min", "2m_temperature_max"]
    vw = {"2m_temperature_min": 10.0, "2m_temperature_max": 10.0}
    lw = O.lat_weights(np.linspace(-80, 80, H + 5), H) if lat else None
    full = O.LOSSES[kind](pred, O.crop_target(tgt, pred), names, vw, False, lw)
    full[-1].backward()
    cw = torch.tensor([1.0, 10.0, 10.0])
    out = hip.loss_fwd(pred.detach().cuda(), tgt.cuda(), None if lw is None else lw.view(-1).cuda(), cw.cuda(),
                       int(kind == "bayesian_tv"))
    assert nerr(out, full) < 2e-5
    dp = hip.loss_bwd(pred.detach().cuda(), tgt.cuda(), None if lw is None else lw.view(-1).cuda(), cw.cuda(),
                      torch.ones(1, device="cuda"), int(kind == "bayesian_tv"))
    assert nerr(dp, pred.grad) < 2e-5


def test_loss_image_gradient(hip):
    g = torch.Generator().manual_seed(14)
    B, C, H, W = 2, 3, 20, 36
    pred = torch.randn(B, C, H, W, generator=g).requires_grad_()
    tgt = torch.randn(B, C, H + 2, W + 4, generator=g)
    names = ["total_precipitation_24hr", "2m_temperature_min", "2m_temperature_max"]
    vw = {"2m_temperature_min": 10.0, "2m_temperature_max": 10.0}
    ref = O.image_gradient(pred, O.crop_target(tgt, pred).contiguous(), names, vw)
    ref.backward()
    cw = torch.tensor([1.0, 10.0, 10.0]).cuda()
    out = hip.loss_fwd(pred.detach().cuda(), tgt.cuda(), None, cw, 2)
    assert abs(float(out[-1]) - float(ref)) / float(ref) < 2e-5
    dp = hip.loss_bwd(pred.detach().cuda(), tgt.cuda(), None, cw, torch.ones(1, device="cuda"), 2)
    assert nerr(dp, pred.grad) < 2e-5


def test_clamp_channel(hip):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 8, 8, generator=g)
    y = hip.clamp_channel_(x.clone().cuda(), 1)
    ref = x.clone(); ref[:, 1].clamp_(min=0)
    assert torch.equal(y.cpu(), ref)
    d = hip.clamp_channel_bwd_(y, torch.ones_like(y), 1)
    refd = torch.ones_like(x); refd[:, 1] = (x[:, 1] > 0).float()
    assert torch.equal(d.cpu(), refd)


def test_adamw_and_casts(hip):
    g = torch.Generator().manual_seed(6)
    n = 10007
    p = torch.randn(n + 1, generator=g)[:n].clone()
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    pr, mr, vr = p.clone(), torch.zeros(n), torch.zeros(n)
    pd, md, vd = p.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p16 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    for step, gr in enumerate(grads, 1):
        O.adamw_step(pr, gr, mr, vr, step, 5e-4, 0.9, 0.99, 1e-8, 1e-5)
        hip.adamw(pd, md, vd, (gr * 4.0).cuda(), p16, n, 5e-4, 0.9, 0.99, 1e-8, 1e-5, step, grad_scale=0.25)
    assert nerr(pd, pr) < 1e-6 and nerr(md, mr) < 1e-6 and nerr(vd, vr) < 1e-6
    assert torch.equal(p16.cpu(), pd.cpu().to(torch.bfloat16))
    # bf16 grads + found_inf skip
    fi = torch.zeros(1, device="cuda")
    gb = grads[0].to(torch.bfloat16).cuda()
    gb[17] = float("inf")
    hip.check_finite(gb, n, fi)
    assert fi.item() == 1.0
    before = pd.clone()
    hip.adamw(pd, md, vd, gb, p16, n, 5e-4, 0.9, 0.99, 1e-8, 1e-5, 4, found_inf=fi)
    assert torch.equal(before, pd)
    assert torch.equal(hip.cast_to_bf16(p.cuda()).cpu(), p.to(torch.bfloat16))


def test_colsum_batchsum(hip):
    g = torch.Generator().manual_seed(12)
    x = rt(torch.randn(300, 264, generator=g))
    out = torch.empty(264, device="cuda")
    hip.colsum(bf(x).cuda(), 300, 264, 264, out)
    assert nerr(out, x.sum(0)) < 1e-5
    xb = rt(torch.randn(3, 40, 64, generator=g))
    o2 = torch.empty(40, 64, device="cuda")
    hip.batch_sum(bf(xb).cuda(), 3, 40, 64, o2)
    assert nerr(o2, xb.sum(0)) < 1e-6


@pytest.mark.parametrize("M,N,p,scaled,beta", [(300, 264, 0.1, True, 0.0), (1024, 512, 0.0, True, 1.0), (77, 64, 0.25, False, 0.0)])
def test_dropout_bwd_colsum_equals_the_two_kernels(hip, M, N, p, scaled, beta):
    """the fused pass (mask/DropPath backward + bias gradient) is bit-identical to dropout_bwd followed by colsum"""
    g = torch.Generator().manual_seed(31)
    dy = bf(torch.randn(M, N, generator=g)).cuda()
    rps = 50
    rs = (torch.rand((M + rps - 1) // rps, generator=g) * 2).cuda() if scaled else None
    for dt in (torch.float32, torch.bfloat16):
        base = torch.randn(N, generator=g).to(dt).cuda()
        ref_dym = hip.dropout_bwd(dy, M, N, p, 1234, rs, rps)
        ref_b = base.clone()
        hip.colsum(ref_dym, M, N, N, ref_b, beta=beta)
        got_b = base.clone()
        got_dym = hip.dropout_bwd_colsum(dy, M, N, p, 1234, rs, rps, got_b, beta=beta)
        assert torch.equal(got_dym, ref_dym)
        assert torch.equal(got_b, ref_b)


def test_bad_arguments_are_refused_not_run(hip):
    """the ABI validates shapes on the host and returns an error code (wrapped as HipBackendError); nothing is launched"""
    from climate_learn._hip import HipBackendError
    x = torch.zeros(64, 96, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(HipBackendError):                       # head dim 96 is not built (-3 unsupported)
        hip.attn_fwd(torch.zeros(1, 64, 3 * 2 * 96, dtype=torch.bfloat16, device="cuda"), 1, 64, 2, 96, 0.0, 0)
    with pytest.raises(HipBackendError):                       # dropout probability out of range
        hip.attn_fwd(torch.zeros(1, 64, 3 * 2 * 64, dtype=torch.bfloat16, device="cuda"), 1, 64, 2, 64, 1.0, 0)
    out = torch.zeros(64, 100, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(HipBackendError):                       # N % 8 != 0
        hip.gemm(x, torch.zeros(100, 96, dtype=torch.bfloat16, device="cuda"), out, 64, 100, 96, 96, 96, 100)
    with pytest.raises(HipBackendError):                       # K-contiguous operand with K % 8 != 0
        hip.gemm(torch.zeros(64, 100, dtype=torch.bfloat16, device="cuda"), torch.zeros(64, 100, dtype=torch.bfloat16, device="cuda"),
                 torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda"), 64, 64, 100, 100, 100, 64)
    with pytest.raises(HipBackendError):                       # LayerNorm width not a multiple of 8
        hip.layernorm_fwd(torch.zeros(4, 100, dtype=torch.bfloat16, device="cuda"), torch.zeros(100, dtype=torch.bfloat16, device="cuda"),
                          torch.zeros(100, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(HipBackendError):                       # operands must live on the GPU: there is no CPU path
        hip.layernorm_fwd(torch.zeros(4, 96, dtype=torch.bfloat16), torch.zeros(96, dtype=torch.bfloat16).cuda(),
                          torch.zeros(96, dtype=torch.bfloat16).cuda())
    with pytest.raises(HipBackendError):                       # wrong dtype
        hip.attn_fwd(torch.zeros(1, 64, 3 * 2 * 64, dtype=torch.float32, device="cuda"), 1, 64, 2, 64, 0.0, 0)
    with pytest.raises(HipBackendError):                       # more problems than one grouped launch takes
        hip.gemm_grouped([])
    torch.cuda.synchronize()                                   # nothing faulted


def test_backward_gemm_forms_own_kernel(hip, monkeypatch):
    """the epilogue-free GEMMs of the training step (dX = dY.W in the NT / NN forms, dW = dY^T.X in the TN form, with and
    without accumulation into the gradient bucket) run on orbit2_gemm_bf16 like every other GEMM: correct in every
    form the step uses, and no vendor-library matmul is reachable (torch.matmul / addmm are booby-trapped here)"""
    def boom(*a, **k):
        raise AssertionError("vendor GEMM called from the product path")
    for name in ("matmul", "mm", "addmm", "bmm"):
        monkeypatch.setattr(torch, name, boom)
    g = torch.Generator().manual_seed(21)
    M, N, K = 512, 640, 768
    for a_kc, b_kc, beta in [(True, True, 0.0), (True, False, 0.0), (False, False, 0.0), (False, False, 1.0)]:
        A = bf(torch.randn((M, K) if a_kc else (K, M), generator=g)).cuda()
        B = bf(torch.randn((N, K) if b_kc else (K, N), generator=g)).cuda()
        C0 = bf(torch.randn(M, N, generator=g)).cuda()
        o = C0.clone()
        hip.gemm(A, B, o, M, N, K, K if a_kc else M, K if b_kc else N, N, a_kc=a_kc, b_kc=b_kc, beta=beta)
        Af, Bf = A.float().cpu(), B.float().cpu()
        ref = torch.einsum("mk,nk->mn", Af if a_kc else Af.t(), Bf if b_kc else Bf.t()) + beta * C0.float().cpu()
        assert nerr(o.cpu(), ref) < 1e-2, (a_kc, b_kc, beta)
    assert not hasattr(hip, "plain_gemm") and not hasattr(hip, "PLAIN_GEMM_LIBRARY")


# ---- position-embedding table: bicubic re-grid + resolution embedding -----------------------------------------------
def test_posembed_regrid_matches_reference_golden(hip, golden_dir):
    """orbit2_posembed_fwd against what the REFERENCE's interpolate_pos_embed_on_the_fly returned for the same table
    (tests/golden/components_tiny.npz pos.*, written by make_golden.py from components/pos_embed.py:103-138): up-sampling,
    down-sampling and the same-grid pass-through"""
    from climate_learn.models.hub.components.pos_embed import interpolate_pos_embed_on_the_fly
    z = np.load(os.path.join(golden_dir, "components_tiny.npz"))
    pe = torch.from_numpy(z["pos.in"]).cuda()
    for key, size in (("pos.up_12x24", (24, 48)), ("pos.down_2x4", (4, 8)), ("pos.same", (8, 16))):
        got = interpolate_pos_embed_on_the_fly(pe, 2, size)
        ref = torch.from_numpy(z[key])
        assert got.shape == ref.shape and got.is_cuda
        assert float((got.cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max()) + 1e-6, key


@pytest.mark.parametrize("oh,nh,D", [(8, 16, 128), (16, 8, 64), (16, 64, 1024), (12, 45, 256), (64, 16, 512), (16, 16, 256)])
def test_posembed_table_forward_backward(hip, oh, nh, D):
    """the whole table a step adds to its tokens, out = bicubic(pos_embed) + w * res + b, and its three gradients against torch on
    the CPU (the oracle's pos_embed_for_grid is F.interpolate): fp32, <= 1e-5 of the largest value; the backward is a
    fixed-order gather (two runs agree bit for bit)"""
    from climate_learn import _ops
    import torch.nn.functional as F
    ow, nw = 2 * oh, 2 * nh
    g = torch.Generator().manual_seed(oh * 131 + nh)
    pe = torch.randn(1, oh * ow, D, generator=g)
    sw, sb, res = torch.randn(D, 1, generator=g), torch.randn(D, generator=g), 0.703
    go = torch.randn(nh * nw, D, generator=g)
    pr, wr, br = pe.clone().requires_grad_(), sw.clone().requires_grad_(), sb.clone().requires_grad_()
    grid = pr.reshape(1, oh, ow, D).permute(0, 3, 1, 2)
    if oh != nh:
        grid = F.interpolate(grid, size=(nh, nw), mode="bicubic", align_corners=False)
    ref = grid.permute(0, 2, 3, 1).reshape(nh * nw, D) + (wr[:, 0] * res + br).view(1, -1)
    ref.backward(go)
    pg, wg, bg = pe.cuda().requires_grad_(), sw.cuda().requires_grad_(), sb.cuda().requires_grad_()
    out = _ops.PosResFn.apply(pg, wg, bg, res, oh, ow, nh, nw)
    out.backward(go.cuda())
    err = lambda a, b: float((a.detach().cpu() - b.detach()).abs().max() / b.detach().abs().max())
    assert out.shape == (nh * nw, D) and err(out, ref) < 1e-5
    assert err(pg.grad, pr.grad) < 1e-5 and err(wg.grad, wr.grad) < 1e-5 and err(bg.grad, br.grad) < 1e-5
    first = pg.grad.clone()
    pg.grad = None
    _ops.PosResFn.apply(pg, wg, bg, res, oh, ow, nh, nw).backward(go.cuda())
    assert torch.equal(first, pg.grad)


def test_posembed_argument_checks(hip):
    x = torch.zeros(8 * 16, 6, device="cuda")
    assert hip.lib().orbit2_posembed_fwd(hip._p(x), None, None, 0.0, hip._p(x), 8, 16, 8, 16, 6, None) == -1   # D % 4
    y = torch.zeros(8 * 16, 8, device="cuda")
    assert hip.lib().orbit2_posembed_fwd(hip._p(y), hip._p(y), None, 0.0, hip._p(y), 8, 16, 8, 16, 8, None) == -1  # sw without sb
    assert hip.lib().orbit2_posembed_bwd(hip._p(y), hip._p(y), 8, 16, 8, 12, 8, None) == -1       # same height, other width
