"""GPU tests of the fp32 forward kernels on their own (orbit2_gemm_f32, orbit2_attn_fwd_f32, orbit2_layernorm_fwd_f32 and
the fp32 token entries of the variable aggregation and unpatchify), each against fp64 math on the CPU from the same fp32 inputs.

Bound for ordinary (unit-variance) inputs: normalised max error max|a-b| / max|b| <= 2e-5, the figure tests/test_hip_ops.py
uses for an fp32 GEMM output whose only error is the accumulation order.  Two cases are ill-conditioned on purpose (attention
with q, k scaled by 8; LayerNorm of rows with a common offset of 1e3): plain fp32 PyTorch itself misses 2e-5 there, so the
bound is 4 x the error of the same quantity computed in fp32 PyTorch on the CPU against fp64 on the very same inputs (a
different summation order and exp2 for exp are each worth up to a factor of two; a bf16 rounding or a one-pass variance is
worth a factor of a thousand).  Every test prints the errors it measured."""
import ctypes
import math

import pytest
import torch

from oracle import orbit2_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-5
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def hip():
    from climate_learn import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip


def nerr(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gemm_ref(A, B, bias=None, colscale=None, act=0, residual=None, res_mod=0, beta=0.0, C0=None):
    """the epilogue of include/orbit2_hip.h in fp64 (drop_p = 0)"""
    v = A.double() @ B.double().t()
    if bias is not None:
        v = v + bias.double()
    if colscale is not None:
        v[:, :colscale[0]] = v[:, :colscale[0]] * float(torch.tensor(colscale[1], dtype=torch.float32))
    if act == 1:
        v = gelu64(v)
    if residual is not None:
        rows = torch.arange(v.shape[0]) % res_mod if res_mod > 0 else torch.arange(v.shape[0])
        v = v + residual.double()[rows]
    if beta != 0.0:
        v = v + beta * C0.double()
    return v


def run_gemm(hip, A, B, out=None, **kw):
    M, K = A.shape
    N = B.shape[0]
    Ad, Bd = A.cuda(), B.cuda()
    out = torch.empty(M, N, device="cuda") if out is None else out
    for k in ("bias", "residual"):
        if kw.get(k) is not None:
            kw[k] = kw[k].cuda()
    hip.gemm_f32(Ad, Bd, out, M, N, K, K, K, N, **kw)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 64, 4), (1, 192, 4096), (50, 64, 8), (50, 192, 60), (257, 192, 8), (257, 384, 64), (257, 4096, 1024),
               (4096, 64, 4096), (4096, 384, 1024), (4096, 4096, 64), (50, 4096, 4096)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_f32_shapes(hip, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    ref = gemm_ref(A, B)
    ref_e = gemm_ref(A, B, bias=bias, act=1)
    for tile in (0, 64, 128):
        e = nerr(run_gemm(hip, A, B, tile=tile), ref)
        e2 = nerr(run_gemm(hip, A, B, tile=tile, bias=bias, act=1), ref_e)
        print("[gemm_f32] M=%d N=%d K=%d tile=%d: plain %.2e, bias+GELU %.2e" % (M, N, K, tile, e, e2))
        assert e < TOL and e2 < TOL


def test_gemm_f32_epilogue_pieces(hip):
    M, N, K, L = 257, 384, 64, 50
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, res = torch.randn(N, generator=g), torch.randn(L, N, generator=g)
    resM, C0 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    cs = (N // 3, LOG2E / 8.0)
    plain = run_gemm(hip, A, B)
    cases = {
        "bias": dict(bias=bias),
        "gelu": dict(act=1),
        "colscale": dict(colscale=cs),
        "residual": dict(residual=resM, ldr=N),
        "residual_mod": dict(residual=res, ldr=N, res_mod=L),
        "residual_mod_first": dict(residual=res, ldr=N, res_mod=L, res_first=True),
        "all": dict(bias=bias, colscale=cs, act=1, residual=res, ldr=N, res_mod=L, res_first=True),
    }
    for name, kw in cases.items():
        rkw = {k: v for k, v in kw.items() if k not in ("ldr", "res_first")}
        for tile in (64, 128):
            out = run_gemm(hip, A, B, tile=tile, **dict(kw))
            e = nerr(out, gemm_ref(A, B, **rkw))
            print("[gemm_f32 epilogue] %s tile=%d: %.2e" % (name, tile, e))
            assert e < TOL, name
    # colscale touches the first third only: the other columns keep the bits of a run without it
    out = run_gemm(hip, A, B, colscale=cs)
    assert torch.equal(out[:, cs[0]:], plain[:, cs[0]:]) and not torch.equal(out[:, :cs[0]], plain[:, :cs[0]])
    # beta = 1: accumulation into C, on top of the whole epilogue
    for tile in (64, 128):
        acc = C0.clone().cuda()
        run_gemm(hip, A, B, out=acc, tile=tile, beta=1.0, bias=bias, act=1, residual=res, ldr=N, res_mod=L)
        e = nerr(acc, gemm_ref(A, B, bias=bias, act=1, residual=res, res_mod=L, beta=1.0, C0=C0))
        print("[gemm_f32 epilogue] beta=1 tile=%d: %.2e" % (tile, e))
        assert e < TOL
    # two launches agree bit for bit
    assert torch.equal(run_gemm(hip, A, B, bias=bias, act=1), run_gemm(hip, A, B, bias=bias, act=1))


def test_gemm_f32_padded_leading_dimensions(hip):
    M, N, K = 130, 192, 60
    g = torch.Generator().manual_seed(9)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    res = torch.randn(M, N, generator=g)
    Ap = torch.full((M, K + 12), float("nan"), device="cuda")
    Ap[:, :K] = A.cuda()
    Bp = torch.full((N, K + 4), float("nan"), device="cuda")
    Bp[:, :K] = B.cuda()
    Rp = torch.full((M, N + 16), float("nan"), device="cuda")
    Rp[:, :N] = res.cuda()
    Cp = torch.full((M, N + 8), -7.0, device="cuda")
    hip.gemm_f32(Ap[:, :K], Bp[:, :K], Cp[:, :N], M, N, K, K + 12, K + 4, N + 8, residual=Rp[:, :N], ldr=N + 16)
    torch.cuda.synchronize()
    e = nerr(Cp[:, :N], gemm_ref(A, B, residual=res))
    print("[gemm_f32] padded lda / ldb / ldc / ldr: %.2e" % e)
    assert e < TOL
    assert bool((Cp[:, N:] == -7.0).all())                      # the pad columns of C are not written


@pytest.mark.parametrize("tile", [0, 64, 128])
def test_gemm_f32_exact_integers_asymmetric_b(hip, tile):
    """small integers: every product and partial sum is exact in fp32, so the result is exact whatever the order -- and an
    asymmetric B makes a row / column swap in the C write (or a wrong k pairing of the operand lanes) visible"""
    M, N, K = 200, 160, 72
    m, n, k = torch.arange(M).view(M, 1), torch.arange(N).view(N, 1), torch.arange(K).view(1, K)
    A = ((5 * m + 3 * k) % 9 - 4).float()
    B = ((3 * n + 7 * k + n * k) % 11 - 5).float()
    assert not torch.equal(B[:K, :K], B[:K, :K].t())
    out = run_gemm(hip, A, B, tile=tile)
    assert torch.equal(out.cpu(), (A.double() @ B.double().t()).float())
    eye = torch.eye(K)                                           # A = I: C[m][n] = B[n][m]
    assert torch.equal(run_gemm(hip, eye, B, tile=tile).cpu(), B.t()[:K].contiguous())


def test_gemm_f32_refuses_what_it_does_not_implement(hip):
    M = N = K = 64
    A = torch.randn(M, K, device="cuda")
    B = torch.randn(N, K, device="cuda")
    aux = torch.zeros(M * N, device="cuda")
    lib = hip.lib()

    def args(**kw):
        a = hip.GemmArgs()
        a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), 0
        a.M, a.N, a.K, a.lda, a.ldb, a.ldc = M, N, K, K, K, N
        a.a_kc = a.b_kc = 1
        a.out_fp32 = 1
        a.colscale = 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    p = aux.data_ptr()
    unsupported = [dict(a_kc=0), dict(b_kc=0), dict(a_kc=0, b_kc=0), dict(drop_p=0.1), dict(save_pre=p), dict(save_dact=p),
                   dict(mul=p), dict(dgelu_pre=p), dict(rowscale=p, rows_per_scale=1), dict(colsum_ws=p), dict(act=2),
                   dict(out_fp32=0), dict(tile_hint=256), dict(tile_hint=260), dict(tile_hint=262), dict(tile_hint=32)]
    for kw in unsupported:
        out = torch.full((M, N), 3.0, device="cuda")
        a = args(**kw)
        a.C = out.data_ptr()
        rc = lib.orbit2_gemm_f32(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -3, (kw, rc)
        assert bool((out == 3.0).all()), kw                      # refused before any launch
    out = torch.full((M, N), 3.0, device="cuda")
    a = args()
    a.C = out.data_ptr()
    assert lib.orbit2_gemm_f32(ctypes.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert nerr(out, gemm_ref(A.cpu(), B.cpu())) < TOL
    # the wrapper turns the code into an exception (no fallback)
    with pytest.raises(hip.HipBackendError, match="-3"):
        hip.gemm_f32(A, B, out, M, N, K, K, K, N, tile=256)
    with pytest.raises(hip.HipBackendError):
        hip.gemm_f32(A.to(torch.bfloat16), B, out, M, N, K, K, K, N)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def attn_ref(qkv, d, prescaled, dtype=torch.float64):
    """qkv [B, L, 3, H, d] -> out [B, L, H, d], lse [B, H, L] (natural log) in `dtype` on the CPU"""
    x = qkv.to(dtype)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))              # [B, H, L, d]
    s = q @ k.transpose(-1, -2)
    s = s * (math.log(2.0) if prescaled else 1.0 / math.sqrt(d))                 # a prescaled q carries log2(e) / sqrt(d)
    lse = torch.logsumexp(s, -1)
    out = torch.softmax(s, -1) @ v
    return out.permute(0, 2, 1, 3).contiguous(), lse


def make_qkv(B, L, H, d, seed, qk_scale=1.0, prescaled=False):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 3, H, d, generator=g)
    qkv[:, :, :2] *= qk_scale
    if prescaled:
        qkv[:, :, 0] *= torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32)
    return qkv


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("L", [1, 50, 256, 648, 2048])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_attn_fwd_f32(hip, d, L, prescaled):
    B, H = (2, 3) if L <= 648 else (1, 2)
    qkv = make_qkv(B, L, H, d, 100 * d + L, prescaled=prescaled)
    ref, lse_ref = attn_ref(qkv, d, prescaled)
    flags = hip.ATTN_Q_PRESCALED if prescaled else 0
    out, lse = hip.attn_fwd_f32(qkv.cuda(), B, L, H, d, flags=flags)
    torch.cuda.synchronize()
    e_o, e_l = nerr(out.view(B, L, H, d), ref), nerr(lse, lse_ref)
    print("[attn_fwd_f32] d=%d L=%d prescaled=%d: out %.2e lse %.2e" % (d, L, prescaled, e_o, e_l))
    assert e_o < TOL and e_l < TOL
    assert tuple(out.shape) == (B, L, H * d) and tuple(lse.shape) == (B, H, L)


@pytest.mark.parametrize("d", [64, 128, 256])
def test_attn_fwd_f32_padded_pitches(hip, d):
    B, L, H = 2, 50, 2
    qkv = make_qkv(B, L, H, d, 7 + d)
    ref, lse_ref = attn_ref(qkv, d, False)
    ldq, ldo = 3 * H * d + 12, H * d + 8
    qp = torch.full((B * L, ldq), float("nan"), device="cuda")
    qp[:, :3 * H * d] = qkv.view(B * L, -1).cuda()
    op = torch.full((B * L, ldo), -7.0, device="cuda")
    out, lse = hip.attn_fwd_f32(qp[:, :3 * H * d], B, L, H, d, out=op[:, :H * d])
    torch.cuda.synchronize()
    e_o, e_l = nerr(op[:, :H * d].reshape(B, L, H, d), ref), nerr(lse, lse_ref)
    print("[attn_fwd_f32] d=%d padded ldq / ldo: out %.2e lse %.2e" % (d, e_o, e_l))
    assert e_o < TOL and e_l < TOL
    assert bool((op[:, H * d:] == -7.0).all())


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_attn_fwd_f32_large_scores_relative_bound(hip, d, prescaled):
    """q, k scaled by 8: scores of tens of nats (where the doubly-rounded bf16 path loses ~1e-2).  Ill-conditioned: fp32
    PyTorch itself misses 2e-5 here, so the kernel is allowed 4 x the error of fp32 PyTorch on the CPU on these inputs."""
    B, L, H = 1, 2048, 2
    qkv = make_qkv(B, L, H, d, 31 + d, qk_scale=8.0, prescaled=prescaled)
    ref, lse_ref = attn_ref(qkv, d, prescaled)
    t32, tl32 = attn_ref(qkv, d, prescaled, torch.float32)
    b_o, b_l = nerr(t32, ref), nerr(tl32, lse_ref)
    flags = hip.ATTN_Q_PRESCALED if prescaled else 0
    out, lse = hip.attn_fwd_f32(qkv.cuda(), B, L, H, d, flags=flags)
    torch.cuda.synchronize()
    e_o, e_l = nerr(out.view(B, L, H, d), ref), nerr(lse, lse_ref)
    print("[attn_fwd_f32 q,k x 8] d=%d prescaled=%d: out %.2e (fp32 PyTorch %.2e, bound %.2e) lse %.2e (fp32 PyTorch %.2e, "
          "bound %.2e)" % (d, prescaled, e_o, b_o, 4 * b_o, e_l, b_l, 4 * b_l))
    assert e_o <= 4 * b_o and e_l <= 4 * b_l


def test_attn_fwd_f32_refusals(hip):
    B, L, H, d = 1, 8, 1, 64
    qkv = torch.randn(B, L, 3, H, d, device="cuda")
    out = torch.full((B, L, H * d), 3.0, device="cuda")
    lse = torch.zeros(B, H, L, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    lib = hip.lib()
    assert lib.orbit2_attn_fwd_f32(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, H, d, 0.1, 0, 0, 3 * H * d, H * d, st) == -3
    assert lib.orbit2_attn_fwd_f32(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, H, 32, 0.0, 0, 0, 3 * H * 32, H * 32, st) == -3
    assert lib.orbit2_attn_fwd_f32(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, L, H, d, 0.0, 0, hip.ATTN_4WAVES, 3 * H * d, H * d, st) == -3
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    with pytest.raises(hip.HipBackendError, match="-3"):
        hip.attn_fwd_f32(qkv, B, L, H, d, drop_p=0.1)
    with pytest.raises(hip.HipBackendError):
        hip.attn_fwd_f32(qkv.to(torch.bfloat16), B, L, H, d)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def ln_ref(x, w, b, dtype=torch.float64):
    return torch.nn.functional.layer_norm(x.to(dtype), (x.shape[-1],), w.to(dtype), b.to(dtype), 1e-5)


@pytest.mark.parametrize("rows", [1, 50, 4096])
@pytest.mark.parametrize("D", [128, 1024, 3072, 8192])
def test_layernorm_fwd_f32(hip, D, rows):
    g = torch.Generator().manual_seed(D + rows)
    x = torch.randn(rows, D, generator=g) * 1.7 + 0.3
    w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = ln_ref(x, w, b)
    y, mean, rstd = hip.layernorm_fwd_f32(x.cuda(), w.cuda(), b.cuda(), stats=True)
    yp = torch.full((rows, D + 8), -7.0, device="cuda")
    hip.layernorm_fwd_f32(x.cuda(), w.cuda(), b.cuda(), out=yp[:, :D])          # padded ldy, no statistics (NULL)
    torch.cuda.synchronize()
    x64 = x.double()
    e = nerr(y, ref)
    e_m = nerr(mean, x64.mean(1))
    e_r = nerr(rstd, (x64.var(1, unbiased=False) + 1e-5).rsqrt())
    print("[layernorm_fwd_f32] D=%d rows=%d: y %.2e mean %.2e rstd %.2e" % (D, rows, e, e_m, e_r))
    assert e < TOL and e_m < TOL and e_r < TOL
    assert torch.equal(yp[:, :D], y) and bool((yp[:, D:] == -7.0).all())


@pytest.mark.parametrize("D", [128, 1024, 8192])
def test_layernorm_fwd_f32_large_offset_relative_bound(hip, D):
    """rows with mean 1e3 and spread 1: a one-pass variance (E[x^2] - E[x]^2) loses every digit here.  Ill-conditioned: the bound
    is 4 x the error of fp32 PyTorch on the CPU on the same inputs."""
    rows = 50
    g = torch.Generator().manual_seed(3 * D)
    x = torch.randn(rows, D, generator=g) + 1e3
    w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = ln_ref(x, w, b)
    base = nerr(ln_ref(x, w, b, torch.float32), ref)
    y = hip.layernorm_fwd_f32(x.cuda(), w.cuda(), b.cuda())
    torch.cuda.synchronize()
    e = nerr(y, ref)
    print("[layernorm_fwd_f32 offset 1e3] D=%d: %.2e (fp32 PyTorch %.2e, bound %.2e)" % (D, e, base, 4 * base))
    assert e <= 4 * base


# ---------------------------------------------------------------------------------------------------------------------
# variable aggregation / unpatchify with fp32 tokens
# ---------------------------------------------------------------------------------------------------------------------
def _tables(sd, heads, ids, D):
    """fp32 table algebra of the folded variable aggregation (csrc/varagg.hip header), as in tests/test_hip_ops.py"""
    dh = D // heads
    Wq, Wkv = sd["var_agg.q.weight"], sd["var_agg.kv.weight"]
    Wk, Wv = Wkv[:D], Wkv[D:]
    qv = (sd["var_query"].view(1, D) @ Wq.t()).view(D)
    U = torch.stack([(qv[h * dh:(h + 1) * dh, None] * Wk[h * dh:(h + 1) * dh]).sum(0) for h in range(heads)]) * dh ** -0.5
    cm = []
    for v in ids:
        w = sd["token_embeds.%d.proj.weight" % v].view(D, 4)
        c = sd["token_embeds.%d.proj.bias" % v] + sd["var_embed"][0, v]
        cm.append(torch.cat([w.t(), c.view(1, D)], 0))
    cm = torch.stack(cm)
    return torch.einsum("hd,vcd->hvc", U, cm).contiguous(), torch.einsum("vcd,id->vci", cm, Wv).contiguous()


@pytest.mark.parametrize("D,heads,V,hw", [(64, 4, 5, (8, 16)), (256, 4, 23, (16, 32)), (384, 3, 7, (12, 20)),
                                           (256, 2, 25, (32, 64)), (512, 2, 5, (8, 16)), (256, 4, 30, (8, 16))])
def test_varagg_fwd_f32_matches_dense_oracle(hip, D, heads, V, hw):
    """the cases and the dense oracle of test_hip_ops.py::test_varagg_fold_matches_dense_oracle, evaluated in fp64"""
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
    s64 = {k: v.double() for k, v in sd.items()}
    toks = [O.patch_embed(x[:, i:i + 1].double(), s64["token_embeds.%d.proj.weight" % v], s64["token_embeds.%d.proj.bias" % v], 2)
            for i, v in enumerate(ids)]
    t = torch.stack(toks, 1) + s64["var_embed"][:, ids].unsqueeze(2)
    zref = O.variable_aggregation(t, s64["var_query"], s64["var_agg.q.weight"], s64["var_agg.kv.weight"],
                                  torch.eye(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64), heads)
    L = zref.shape[1]
    stab, gtab = _tables(s64, heads, ids, D)
    st, gt = stab.float().cuda(), gtab.float().cuda()
    z = hip.varagg_fwd_f32(x.cuda(), st, gt, heads, D)                       # attw = NULL
    z2, attw = hip.varagg_fwd_f32(x.cuda(), st, gt, heads, D, want_attw=True)
    zb, attw_b = hip.varagg_fwd(x.cuda(), st, gt, heads, D)                  # the bf16 sibling on the same tables
    torch.cuda.synchronize()
    e = nerr(z, zref.reshape(B * L, D))
    print("[varagg_fwd_f32] D=%d heads=%d V=%d: %.2e" % (D, heads, V, e))
    assert z.dtype == torch.float32 and e < TOL
    assert torch.equal(z, z2)                                               # with and without attw: the same launch otherwise
    assert nerr(attw, attw_b) < 1e-6                                        # the softmax weights of the bf16 sibling
    assert nerr(zb, z) < 6e-3                                               # the sibling's z is this one rounded to bf16 (2^-8)


def test_unpatchify_fwd_f32(hip):
    B, C, h, w, p, s = 2, 3, 8, 16, 2, 4
    g = torch.Generator().manual_seed(2)
    t = torch.randn(B, (h // p) * (w // p), C * (s * p) ** 2, generator=g)
    ref = O.unpatchify(t, (h, w), p, s, C)
    img = hip.unpatchify_fwd_f32(t.cuda(), B, C, h, w, p, s)
    torch.cuda.synchronize()
    assert img.dtype == torch.float32 and torch.equal(img.cpu(), ref)        # a pure index permutation: exact
    with pytest.raises(hip.HipBackendError):
        hip.unpatchify_fwd_f32(t.to(torch.bfloat16).cuda(), B, C, h, w, p, s)
