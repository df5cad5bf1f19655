"""GPU tests of the elementwise / reduction / layout entries (csrc/norm_elem.hip, the table gather / scatter of csrc/varagg.hip),
each against a plain fp32 / fp64 / exact torch statement on the CPU.  Where an output has a pitch or a tail, the buffer carries a
sentinel-filled guard region that must stay untouched.

Bounds (normalised max error max|a-b| / max|b|, as in tests/test_hip_ops.py): exact where the op only moves or rounds data;
6e-3 for one bf16 rounding of an fp32 expression (2^-8 relative); 1e-5 for fp32 sums.  Shapes: odd tails, pitches wider than
the row, and 4100 x 2056 (8.43 M elements: more than the 4096 x 256 chunks of 8 that the capped grid of the elementwise kernels
covers in one trip, so the grid-stride loop runs a second one -- rows from 4080 on)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.hashmask import keep_mask

SEED64 = 0x9F143CDEF6E1B1FA
BIG = (4100, 2056)
SECOND_TRIP_ROW = (4096 * 256 * 8) // BIG[1]          # 4080: the first row the second trip of the 8-wide kernels touches


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
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _mask(M, N, p):
    """fp32 [M, N] dropout factor (0 or 256 / (256 - thr)) of the flat hash at SEED64; computed once per shape, read-only"""
    m, sc = keep_mask(SEED64, M * N, p)
    return torch.from_numpy(m).view(M, N) * np.float32(sc)


# ---- post_reduce ------------------------------------------------------------------------------------------------------------------
def _post_reduce_case(hip, M, N, terms, p, inplace, rps, res_mod, check_rows=None):
    """y = bf16(residual + rowscale[m // rps] * dropout(x + addend[m % res_mod])), every term optional"""
    g = torch.Generator().manual_seed(M + N + len(terms))
    x = rt(torch.randn(M, N, generator=g))
    f = x.clone()
    kw = {}
    if "addend" in terms:
        add = rt(torch.randn(res_mod, N, generator=g))
        f = f + add.repeat((M + res_mod - 1) // res_mod, 1)[:M]
        kw.update(addend=bf(add).cuda(), res_mod=res_mod)
    if p > 0:
        f = f * _mask(M, N, p)
        kw.update(drop_p=p, seed=SEED64)
    if "rowscale" in terms:
        rs = torch.rand((M + rps - 1) // rps, generator=g) * 2
        f = f * rs.repeat_interleave(rps)[:M, None]
        kw.update(rowscale=rs.cuda(), rows_per_scale=rps)
    if "residual" in terms:
        res = rt(torch.randn(M, N, generator=g))
        f = f + res
        kw.update(residual=bf(res).cuda())
    xd = bf(x).cuda()
    if inplace:
        y = hip.post_reduce(xd, M, N, **kw)
        assert y.data_ptr() == xd.data_ptr()
    else:
        buf = torch.full((M * N + 64,), 7.0, dtype=torch.bfloat16, device="cuda")
        y = hip.post_reduce(xd, M, N, out=buf[:M * N].view(M, N), **kw)
        assert torch.equal(xd.cpu(), bf(x)) and bool((buf[M * N:] == 7.0).all())
    torch.cuda.synchronize()
    assert nerr(y, f) < 6e-3
    if p > 0 and "residual" not in terms:                       # dropped elements are exact zeros
        assert torch.equal(y.cpu() == 0, (f == 0))
    if check_rows is not None:
        assert nerr(y[check_rows:], f[check_rows:]) < 6e-3 and float(f[check_rows:].abs().max()) > 1.0


@pytest.mark.parametrize("terms", [("residual", "rowscale"), ("addend",), ("addend", "residual", "rowscale")])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("inplace", [True, False])
def test_post_reduce(hip, terms, p, inplace):
    """the three combinations climate_learn/_ops.py uses (Block: residual + DropPath row scale; embedding: position table addend
    with res_mod + dropout) and all terms together; a row count that no term's period divides"""
    _post_reduce_case(hip, 77, 264, terms, p, inplace, rps=11, res_mod=7)


def test_post_reduce_second_grid_trip(hip):
    M, N = BIG
    _post_reduce_case(hip, M, N, ("addend", "residual", "rowscale"), 0.1, True, rps=11, res_mod=7, check_rows=SECOND_TRIP_ROW)


def test_dropout_bwd_second_grid_trip(hip):
    M, N = BIG
    g = torch.Generator().manual_seed(3)
    dy = rt(torch.randn(M, N, generator=g))
    rs = torch.rand((M + 10) // 11, generator=g) * 2 + 0.5
    want = dy * _mask(M, N, 0.1) * rs.repeat_interleave(11)[:M, None]
    got = hip.dropout_bwd(bf(dy).cuda(), M, N, 0.1, SEED64, rs.cuda(), 11)
    torch.cuda.synchronize()
    assert nerr(got, want) < 6e-3
    assert nerr(got[SECOND_TRIP_ROW:], want[SECOND_TRIP_ROW:]) < 6e-3
    assert torch.equal(got.cpu() == 0, want == 0)


@pytest.mark.parametrize("rows,N", [(5, 72), (3, 7), BIG])
def test_add_rowvec(hip, rows, N):
    g = torch.Generator().manual_seed(rows)
    a, vec = bf(torch.randn(rows, N, generator=g)), bf(torch.randn(N, generator=g))
    got = hip.add_rowvec(a.cuda(), vec.cuda(), rows, N)
    assert torch.equal(got.cpu(), bf(a.float() + vec.float()))


# ---- transpose, casts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(64, 64), (1, 8), (100, 72), (130, 1000), (3072, 1024)])
def test_transpose_bf16(hip, R, C):
    g = torch.Generator().manual_seed(R + C)
    src = bf(torch.randn(R, C, generator=g))
    buf = torch.full((R * C + 64,), 7.0, dtype=torch.bfloat16, device="cuda")
    dst = hip.transpose_bf16(src.cuda(), buf[:R * C].view(C, R))
    assert torch.equal(dst.cpu(), src.t().contiguous())
    assert bool((buf[R * C:] == 7.0).all())


@pytest.mark.parametrize("n", [1, 3, 10007])
def test_cast_bf16_to_f32(hip, n):
    src = bf(torch.randn(n, generator=torch.Generator().manual_seed(n)))
    buf = torch.full((n + 8,), 7.0, device="cuda")
    got = hip.cast_to_f32(src.cuda(), buf[:n])
    assert torch.equal(got.cpu(), src.float()) and bool((buf[n:] == 7.0).all())


def _cast_down(hip, x):
    n = x.numel()
    buf = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device="cuda")
    got = hip.cast_to_bf16(x.cuda(), buf[:n])
    torch.cuda.synchronize()
    assert bool((buf[n:] == 7.0).all())
    return got.cpu()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 10007, 4 * 4096 * 256 + 7])
def test_cast_f32_to_bf16(hip, n):
    """tails of 1, 2 and 3 elements after the 4-wide body (none, one and many body iterations), and 4 * 4096 * 256 + 7: one
    4-wide chunk more than the capped grid covers in one trip, plus a tail of 3"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    assert torch.equal(_cast_down(hip, x), x.to(torch.bfloat16))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_cast_f32_to_bf16_special_values(hip, shift):
    """signed zeros, infinities, NaN (stays NaN), the largest finite fp32 (rounds to inf), fp32 denormals, and exact ties (round
    to even); `shift` rotates the vector so that each value passes through the 4-wide body and through the scalar tail"""
    vals = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38,
            1e-45, -1e-45, 1e-39, 1.1754942e-38, 9.18e-41, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8),
            1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20, 2.0 - 2.0 ** -9, 65280.0 + 128.0]
    x = torch.tensor(vals, dtype=torch.float32).roll(shift)
    assert x.numel() % 4 == 3
    got, want = _cast_down(hip, x), x.to(torch.bfloat16)
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(got.float()), nan)
    # bit patterns, so that -0.0 and +0.0 are told apart
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))


# ---- column sums, batch sums ------------------------------------------------------------------------------------------------------
def _colsum_case(hip, M, N, fp32_in):
    """fp32 / bf16 input with a padded pitch whose padding is NaN; fp32 and bf16 outputs; beta 0, 1, 0.5 on a pre-filled output"""
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, N, generator=g)
    x = x if fp32_in else rt(x)
    ldx = N + 8
    xp = torch.full((M, ldx), float("nan"), dtype=torch.float32 if fp32_in else torch.bfloat16)
    xp[:, :N] = x
    xd = xp.cuda()
    ref = x.double().sum(0)
    for out_dt, tol in ((torch.float32, 1e-5), (torch.bfloat16, 6e-3)):
        for beta in (0.0, 1.0, 0.5):
            base = torch.randn(N, generator=g).to(out_dt)
            buf = torch.full((N + 8,), 7.0, dtype=out_dt, device="cuda")
            buf[:N] = base.cuda()
            hip.colsum(xd, M, N, ldx, buf[:N], beta=beta)
            torch.cuda.synchronize()
            want = ref + beta * base.double()
            assert nerr(buf[:N], want) < tol, (out_dt, beta, nerr(buf[:N], want))
            assert bool((buf[N:] == 7.0).all())


@pytest.mark.parametrize("fp32_in", [True, False])
@pytest.mark.parametrize("M,N", [(1, 264), (7, 264), (32, 72), (33, 72), (300, 264), (32767, 72), (32768, 72)])
def test_colsum(hip, M, N, fp32_in):
    """M = 32 / 33: one and two partial sums of 32 rows; M = 32767 / 32768: either side of the switch from 32 to 128 rows per
    partial sum (csrc/norm_elem.hip cs_rows)"""
    _colsum_case(hip, M, N, fp32_in)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("rows,N", [(40, 64), (37, 50)])
def test_batch_sum(hip, B, rows, N):
    g = torch.Generator().manual_seed(B + rows)
    x = rt(torch.randn(B, rows, N, generator=g))
    xd = bf(x).cuda()
    for out_dt, tol in ((torch.float32, 1e-5), (torch.bfloat16, 6e-3)):
        for beta in (0.0, 1.0):
            base = torch.randn(rows, N, generator=g).to(out_dt)
            buf = torch.full((rows * N + 8,), 7.0, dtype=out_dt, device="cuda")
            buf[:rows * N] = base.reshape(-1).cuda()
            hip.batch_sum(xd, B, rows, N, buf[:rows * N], beta=beta)
            torch.cuda.synchronize()
            want = x.double().sum(0) + beta * base.double()
            assert nerr(buf[:rows * N].view(rows, N), want) < tol, (out_dt, beta)
            assert bool((buf[rows * N:] == 7.0).all())


# ---- per-variable table rows: gather and its transpose -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 200])
def test_tables_gather_scatter(hip, D):
    """V = 5 of 7 variables in a non-monotone order; the parameters live in one flat fp32 buffer at pitches larger than the
    tensors (w_stride, b_stride are real; the padding is NaN for the gather and must be skipped).  Gather == the cm rows of
    tests/test_hip_ops.py _tables, exactly; scatter adds exactly their transpose into pre-filled gradient buffers and leaves the
    rows of unselected variables and all padding untouched"""
    VT, ids = 7, [5, 0, 3, 6, 2]
    V = len(ids)
    ws, bs = 4 * D + 8, D + 3
    g = torch.Generator().manual_seed(D)
    W, Bv, E = torch.randn(VT, D, 4, generator=g), torch.randn(VT, D, generator=g), torch.randn(VT, D, generator=g)
    flat = torch.full((VT * ws + VT * bs,), float("nan"))
    flat[:VT * ws].view(VT, ws)[:, :4 * D] = W.view(VT, 4 * D)
    flat[VT * ws:].view(VT, bs)[:, :D] = Bv
    fd = flat.cuda()
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    Ed = E.cuda()
    cmat = hip.tables_gather(fd[:4 * D], ws, fd[VT * ws:VT * ws + D], bs, Ed, ids_t, V, D)
    torch.cuda.synchronize()

    def rows(W, Bv, E):
        return torch.cat([torch.cat([W[v].t(), (Bv[v] + E[v]).view(1, D)], 0) for v in ids], 0)      # [5 V, D]

    assert cmat.shape == (5 * V, D) and torch.equal(cmat.cpu(), rows(W, Bv, E))
    # scatter: autograd of the same construction
    Wg, Bg, Eg = W.clone().requires_grad_(), Bv.clone().requires_grad_(), E.clone().requires_grad_()
    dc = torch.randn(5 * V, D, generator=g)
    rows(Wg, Bg, Eg).backward(dc)
    gflat0 = torch.randn(VT * ws + VT * bs, generator=g)
    gE0 = torch.randn(VT, D, generator=g)
    gflat, gE = gflat0.cuda(), gE0.cuda()
    hip.tables_scatter(dc.cuda(), gflat[:4 * D], ws, gflat[VT * ws:VT * ws + D], bs, gE, ids_t, V, D)
    torch.cuda.synchronize()
    gflat, gE = gflat.cpu(), gE.cpu()
    gw, gw0 = gflat[:VT * ws].view(VT, ws), gflat0[:VT * ws].view(VT, ws)
    gb, gb0 = gflat[VT * ws:].view(VT, bs), gflat0[VT * ws:].view(VT, bs)
    assert nerr(gw[:, :4 * D] - gw0[:, :4 * D], Wg.grad.view(VT, 4 * D)) < 1e-6
    assert nerr(gb[:, :D] - gb0[:, :D], Bg.grad) < 1e-6
    assert nerr(gE - gE0, Eg.grad) < 1e-6
    assert torch.equal(gw[ids, :4 * D], gw0[ids, :4 * D] + Wg.grad.view(VT, 4 * D)[ids])             # one fp32 addition each
    assert torch.equal(gb[ids, :D], gb0[ids, :D] + Bg.grad[ids]) and torch.equal(gE[ids], gE0[ids] + Eg.grad[ids])
    rest = [v for v in range(VT) if v not in ids]
    assert torch.equal(gw[rest], gw0[rest]) and torch.equal(gb[rest], gb0[rest]) and torch.equal(gE[rest], gE0[rest])
    assert torch.equal(gw[:, 4 * D:], gw0[:, 4 * D:]) and torch.equal(gb[:, D:], gb0[:, D:])


def test_tables_refuse_bad_strides(hip):
    """the weight rows are read 16 bytes at a time: a pitch that is no multiple of 4 floats is refused with -1, nothing runs"""
    D = 64
    f = torch.zeros(4096, device="cuda")
    ids = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(5, D, device="cuda")
    p = hip._p
    assert hip.lib().orbit2_tables_gather(p(f), 4 * D + 2, p(f), D, p(f), p(ids), p(out), 1, D, None) == -1
    assert hip.lib().orbit2_tables_scatter(p(out), p(f), 4 * D + 2, p(f), D, p(f), p(ids), 1, D, None) == -1
    torch.cuda.synchronize()


# ---- LayerNorm forward into a padded destination -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 1024, 3072])
@pytest.mark.parametrize("rows", [1, 5, 203])
def test_layernorm_fwd_padded_destination(hip, D, rows):
    """out= a view of a buffer with row pitch D + 64 (orbit2_layernorm_fwd_ld, ldy > D): the same bits as the contiguous call,
    the padding untouched; row counts that are no multiple of the 4 rows per block; mean / rstd against fp64"""
    g = torch.Generator().manual_seed(D + rows)
    x = rt(torch.randn(rows, D, generator=g) * 2 + 0.5)
    gam, bet = bf(1 + 0.1 * torch.randn(D, generator=g)).cuda(), bf(0.1 * torch.randn(D, generator=g)).cuda()
    xd = bf(x).cuda()
    y, mean, rstd = hip.layernorm_fwd(xd, gam, bet)
    buf = torch.full((rows, D + 64), 7.0, dtype=torch.bfloat16, device="cuda")
    y2, mean2, rstd2 = hip.layernorm_fwd(xd, gam, bet, out=buf[:, :D])
    torch.cuda.synchronize()
    assert torch.equal(y2, y) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    assert bool((buf[:, D:] == 7.0).all())
    x64 = x.double()
    assert nerr(mean, x64.mean(1)) < 1e-5
    assert nerr(rstd, (x64.var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5
    assert nerr(y, F.layer_norm(x64, (D,), gam.cpu().double(), bet.cpu().double(), 1e-5)) < 6e-3


@pytest.mark.parametrize("D", [64, 1024, 3072])
def test_layernorm_fwd_mean_far_from_zero(hip, D):
    """x = bf16(100 + 0.1 * randn): the spread is a thousandth of the mean (and a few bf16 steps wide).  A one-pass variance
    E[x^2] - mean^2 loses it in fp32; the kernel's variance is two-pass over the register-resident row"""
    g = torch.Generator().manual_seed(D)
    x = rt(100 + 0.1 * torch.randn(5, D, generator=g))
    gam, bet = bf(1 + 0.1 * torch.randn(D, generator=g)), bf(0.1 * torch.randn(D, generator=g))
    y, mean, rstd = hip.layernorm_fwd(bf(x).cuda(), gam.cuda(), bet.cuda())
    ref = F.layer_norm(x.double(), (D,), gam.double(), bet.double(), 1e-5)
    e = nerr(y, ref)
    print("[layernorm offset D=%d] y %.2e mean %.2e rstd %.2e" % (
        D, e, nerr(mean, x.double().mean(1)), nerr(rstd, (x.double().var(1, unbiased=False) + 1e-5).rsqrt())))
    assert e < 6e-3
