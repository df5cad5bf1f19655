"""GPU tests of every seeded kernel at the seeds the product feeds them: full 64-bit values (climate_learn/_ops.py _SeedStream is
a splitmix64 stream) with, under a captured graph, a 64-bit device salt xored in (climate_learn/graphs.py SALT_STEP).

A dropout / DropPath decision is a pure function of (seed, element index) that forward and backward recompute independently, in
kernels written in different ways; the other op-level tests use seeds below 2^32, where the fold of the seed's high word
(csrc/common.h o2_hash) is the identity.  Here every kernel family goes against the numpy replica of tests/hashmask.py at
SEED64: attention against the fp32 oracle with the host mask (tests/test_hashmask_cpu.py shows that a dropped or mangled high
word moves that oracle by 30x the tolerances used here), the forward and dK + dV masks read out bit by bit, the flat-hash
kernels (GEMM epilogues, dropout backward, post_reduce) by exact masks, DropPath scales exactly, and the salt module by module:
salt S with seed s == salt 0 with seed s ^ S, `add` included across the 2^64 wrap."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hashmask
from tests.hashmask import attn_keep_mask, keep_mask
from tests.test_hashmask_cpu import SALT64, SEED64, attn_case_inputs, attn_oracle

P = 0.1
SALT_ADD = (1 << 64) - SALT64 + 0x5A5A5A5A00000005          # SALT64 + SALT_ADD wraps past 2^64 to 0x5A5A5A5A00000005
SALT_SUM = (SALT64 + SALT_ADD) % (1 << 64)


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


# ---- 2a. attention, every kernel family, against the fp32 oracle with the host mask at SEED64 ------------------------------------
@functools.lru_cache(maxsize=None)
def _case(d, H, L, B, prescaled, p):
    """inputs and fp32 oracle of one attention case, computed once and shared (read-only) by the tests that use it"""
    stored, eff, do = attn_case_inputs(d, H, L, B, prescaled)
    out, dq, dk, dv = attn_oracle(eff, do, B, L, H, d, SEED64, p)
    q, k, _ = eff.view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    lse = torch.logsumexp((q * d ** -0.5) @ k.transpose(-2, -1), dim=-1)
    return stored, do, out, lse, (dq, dk, dv)


def _run_attn(hip, d, H, L, B, prescaled, p, flags, seed=SEED64, gate=None):
    stored, do = _case(d, H, L, B, prescaled, p)[:2]
    sd = stored.cuda()
    out, lse = hip.attn_fwd(sd, B, L, H, d, p, seed, flags=flags, gate=gate)
    dqkv = hip.attn_bwd(sd, out, bf(do).cuda(), lse, B, L, H, d, p, seed, flags=flags, gate=gate)
    torch.cuda.synchronize()
    return out, lse, dqkv


def _check_attn(tag, got, d, H, L, B, prescaled, p):
    """out, lse and the gradient thirds against the oracle: the bounds of tests/test_hip_ops.py test_attention_fwd_bwd"""
    out, lse, dqkv = got
    _, _, ref, lse_ref, grads = _case(d, H, L, B, prescaled, p)
    dv = dqkv.view(B, L, 3, H * d)
    errs = [nerr(out, ref), nerr(lse, lse_ref)] + [nerr(dv[:, :, i], grads[i]) for i in range(3)]
    print("[seeded attn %s d=%d H=%d L=%d B=%d p=%.1f] out %.2e lse %.2e dq %.2e dk %.2e dv %.2e" % ((tag, d, H, L, B, p) + tuple(errs)))
    assert errs[0] < 1e-2
    assert errs[1] < 1e-3
    for e, nm in zip(errs[2:], "qkv"):
        assert e < 2e-2, nm


def test_attention_generated_kernels_at_a_64_bit_seed(hip):
    """d = 128, q pre-scaled, L % 256 == 0: generated forward, dQ and dK + dV (the dK + dV kernel folds the seed's high word
    into a constant of its own instead of calling o2_hash64); the gated twins with an all-ones gate give the same bits"""
    d, H, L, B = 128, 2, 256, 2
    got = _run_attn(hip, d, H, L, B, True, P, hip.ATTN_Q_PRESCALED)
    _check_attn("generated", got, d, H, L, B, True, P)
    gated = _run_attn(hip, d, H, L, B, True, P, hip.ATTN_Q_PRESCALED, gate=torch.ones(B, device="cuda"))
    for a, b in zip(got, gated):
        assert torch.equal(a, b)


def test_attention_compiler_scheduled_d128_at_a_64_bit_seed(hip):
    """the same call on the 8-wave compiler-scheduled forward / dQ with the one-pass dK + dV (ORBIT2_ATTN_NO_W4), and with the
    two-pass dK, dV kernels (ORBIT2_ATTN_SPLIT_DKV): against the oracle, and one pass == two passes bit for bit"""
    d, H, L, B = 128, 2, 256, 2
    one = _run_attn(hip, d, H, L, B, True, P, hip.ATTN_Q_PRESCALED | hip.ATTN_NO_W4)
    _check_attn("8-wave fused", one, d, H, L, B, True, P)
    two = _run_attn(hip, d, H, L, B, True, P, hip.ATTN_Q_PRESCALED | hip.ATTN_NO_W4 | hip.ATTN_SPLIT_DKV)
    _check_attn("8-wave split", two, d, H, L, B, True, P)
    for a, b in zip(one, two):
        assert torch.equal(a, b)


@pytest.mark.parametrize("d,H,L,B", [(128, 1, 300, 1), (64, 2, 128, 2), (64, 2, 320, 1), (256, 1, 161, 1), (256, 1, 256, 1)])
def test_attention_raw_q_families_at_a_64_bit_seed(hip, d, H, L, B):
    """raw q: ragged d = 128; d = 64 on 4 waves (one-pass dK + dV) and with the 8-wave backward, ragged; d = 256 ragged and on
    whole tiles (one-pass dK + dV at one wave per SIMD)"""
    _check_attn("raw q", _run_attn(hip, d, H, L, B, False, P, 0), d, H, L, B, False, P)


@pytest.mark.parametrize("d,H,L,B", [(128, 2, 256, 2), (64, 2, 320, 1)])
@pytest.mark.parametrize("p", [0.0, P])
def test_attention_4wave_geometry(hip, d, H, L, B, p):
    """ORBIT2_ATTN_4WAVES: 4-wave workgroups at L >= 256 (d = 128: two-pass dK, dV; d = 64: ragged 128-row tiles)"""
    _check_attn("4 waves", _run_attn(hip, d, H, L, B, False, p, hip.ATTN_4WAVES), d, H, L, B, False, p)


# ---- 2b. exact mask read-out through the forward and the dK + dV kernels -------------------------------------------------------
@pytest.mark.parametrize("d,H,L,B,flagnames", [(128, 2, 256, 2, ("ATTN_Q_PRESCALED",)), (128, 2, 256, 2, ("ATTN_Q_PRESCALED", "ATTN_NO_W4")),
                                                (64, 2, 128, 2, ())])
def test_attention_masks_read_out_bit_by_bit(hip, d, H, L, B, flagnames):
    """q = k = 0 makes every probability exactly 1 / L.  Forward: V with one-hot rows V[k][j] = [k == j + d * half] gives
    out[q][j] = sc / L * keep[q][j + d * half]; dV: dO with the same one-hot rows over the queries gives
    dV[k][j] = sc / L * keep[j + d * half][k].  ceil(L / d) launches each assemble the whole [B * H, L, L] keep mask, which must
    be the replica's bit for bit.  (dQ has no such read-out: with constant k the row sums of dS vanish.)"""
    flags = 0
    for nm in flagnames:
        flags |= getattr(hip, nm)
    want, sc = attn_keep_mask(SEED64, B * H, L, P)
    want = want.reshape(B, H, L, L) > 0
    halves = (L + d - 1) // d
    thr = sc / (2.0 * L)
    g = torch.Generator().manual_seed(5)
    fwd_mask = np.zeros((B, H, L, L), dtype=bool)
    dkv_mask = np.zeros((B, H, L, L), dtype=bool)
    j = torch.arange(d)
    # any v for the backward: its out / lse feed the statistics tables, the mask read-out does not depend on them
    qkv_any = torch.zeros(B, L, 3, H, d)
    qkv_any[:, :, 2] = torch.randn(B, L, H, d, generator=g)
    qkv_any = bf(qkv_any.reshape(B, L, 3 * H * d)).cuda()
    out_any, lse_any = hip.attn_fwd(qkv_any, B, L, H, d, P, SEED64, flags=flags)
    assert nerr(lse_any, torch.full((B, H, L), float(np.log(L)))) < 1e-5
    for half in range(halves):
        rows = j + d * half
        ok = rows < L
        hot = torch.zeros(B, L, H, d)
        hot[:, rows[ok], :, j[ok]] = 1.0
        qkv = torch.zeros(B, L, 3, H, d)
        qkv[:, :, 2] = hot
        out, _ = hip.attn_fwd(bf(qkv.reshape(B, L, 3 * H * d)).cuda(), B, L, H, d, P, SEED64, flags=flags)
        o = out.float().cpu().view(B, L, H, d).permute(0, 2, 1, 3)                       # [B, H, q, j]
        assert bool(((o == 0) | ((o - sc / L).abs() < 0.02 * sc / L)).all())             # 0 or bf16(sc / L), nothing between
        fwd_mask[:, :, :, rows[ok].numpy()] = (o > thr).numpy()[:, :, :, ok.numpy()]
        do = bf(hot.reshape(B, L, H * d)).cuda()
        dqkv = hip.attn_bwd(qkv_any, out_any, do, lse_any, B, L, H, d, P, SEED64, flags=flags)
        dv = dqkv.float().cpu().view(B, L, 3, H, d)[:, :, 2].permute(0, 2, 3, 1)          # [B, H, j, k]
        assert bool(((dv == 0) | ((dv - sc / L).abs() < 0.02 * sc / L)).all())
        dkv_mask[:, :, rows[ok].numpy(), :] = (dv > thr).numpy()[:, :, ok.numpy(), :]
    assert np.array_equal(fwd_mask, want)
    assert np.array_equal(dkv_mask, want)


# ---- 2c. flat-hash kernels: exact masks --------------------------------------------------------------------------------------------
FM, FN, FK = 512, 256, 64
FLDC = FN + 64


def _flat_mask(seed=SEED64):
    m, sc = keep_mask(seed, FM * FN, P)
    return torch.from_numpy(m).view(FM, FN) > 0, sc


def _gemm_ones(hip, tile, seed=SEED64, **kw):
    """A = B = 1/8, K = 64: every product is exactly 1.  Output with a padded pitch whose padding holds a sentinel."""
    A = torch.full((FM, FK), 0.125, dtype=torch.bfloat16, device="cuda")
    W = torch.full((FN, FK), 0.125, dtype=torch.bfloat16, device="cuda")
    out = torch.full((FM, FLDC), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.gemm(A, W, out, FM, FN, FK, FK, FK, FLDC, drop_p=P, seed=seed, tile=tile, **kw)
    torch.cuda.synchronize()
    assert bool((out[:, FN:] == 7.0).all())                  # the padding is untouched
    return out[:, :FN].cpu()


def _kept_value(sc):
    return torch.tensor(sc, dtype=torch.float32).to(torch.bfloat16)      # bf16(256 / 230)


@pytest.mark.parametrize("tile", [128, 64, 256, 260, 262])
def test_gemm_dropout_mask_at_a_64_bit_seed(hip, tile):
    mask, sc = _flat_mask()
    out = _gemm_ones(hip, tile)
    assert torch.equal(out > 0, mask)
    assert bool((out[mask] == _kept_value(sc)).all()) and bool((out[~mask] == 0).all())


def test_gemm_4wave_compile_time_epilogues_at_a_64_bit_seed(hip):
    """the 4-wave kernel's compile-time epilogues: kind 1 (bias + GELU + saved GELU' factor + dropout: the factor tensor is zero
    exactly where the element is dropped) and kind 2 (bias + dropout + per-sample row scale + residual)"""
    mask, sc = _flat_mask()
    bias = torch.full((FN,), 0.5, dtype=torch.bfloat16, device="cuda")
    dact = torch.full((FM, FLDC), 1234, dtype=torch.int16, device="cuda")
    out = _gemm_ones(hip, 260, bias=bias, act=1, save_dact=dact)            # GELU(1.5) > 0, GELU'(1.5) > 0
    assert torch.equal(out > 0, mask)
    fac = dact.cpu()
    assert torch.equal(fac[:, :FN] != 0, mask) and bool((fac[:, FN:] == 1234).all())
    zero_bias = torch.zeros(FN, dtype=torch.bfloat16, device="cuda")
    res = torch.zeros(FM, FLDC, dtype=torch.bfloat16, device="cuda")
    rs = torch.ones(FM // 256, device="cuda")
    out = _gemm_ones(hip, 260, bias=zero_bias, residual=res, ldr=FLDC, rowscale=rs, rows_per_scale=256)
    assert torch.equal(out > 0, mask)
    assert bool((out[mask] == _kept_value(sc)).all()) and bool((out[~mask] == 0).all())


def _elem_masks(hip, seed=SEED64):
    """the three elementwise kernels of csrc/norm_elem.hip that draw the flat mask, each on ones"""
    ones = torch.ones(FM, FN, dtype=torch.bfloat16, device="cuda")
    a = hip.dropout_bwd(ones, FM, FN, P, seed)
    cs = torch.empty(FN, device="cuda")
    b = hip.dropout_bwd_colsum(ones, FM, FN, P, seed, None, 0, cs)
    c = hip.post_reduce(ones.clone(), FM, FN, drop_p=P, seed=seed)
    torch.cuda.synchronize()
    return a.cpu(), b.cpu(), c.cpu(), cs.cpu()


def test_elementwise_dropout_masks_at_a_64_bit_seed(hip):
    mask, sc = _flat_mask()
    a, b, c, cs = _elem_masks(hip)
    for out in (a, b, c):
        assert torch.equal(out > 0, mask)
        assert bool((out[mask] == _kept_value(sc)).all()) and bool((out[~mask] == 0).all())
    assert nerr(cs, a.double().sum(0)) < 1e-5


# ---- 2d. DropPath scales --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [SEED64, 7])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_droppath_scales(hip, B, p, seed):
    got = hip.droppath_scales(B, p, seed, "cuda").cpu()
    assert torch.equal(got, torch.from_numpy(hashmask.droppath_scales(seed, B, p)))
    if p == 0.0:
        assert bool((got == 1.0).all())


# ---- 2e. the seed salt, module by module ----------------------------------------------------------------------------------------
def _salted_call(hip, module):
    """one seeded call per translation unit that keeps its own copy of the salt: seed -> tuple of CPU tensors"""
    if module == "gemm":
        return lambda s: (_gemm_ones(hip, 128, seed=s),)
    if module == "attn":
        d, H, L, B = 128, 2, 256, 2
        return lambda s: tuple(t.cpu() for t in _run_attn(hip, d, H, L, B, True, P, hip.ATTN_Q_PRESCALED, seed=s))
    return lambda s: _elem_masks(hip, seed=s)[:3] + (hip.droppath_scales(1000, 0.5, s, "cuda").cpu(),)


@pytest.mark.parametrize("module", ["gemm", "attn", "elem"])
def test_seed_salt_is_an_xor_into_the_seed(hip, module):
    """orbit2_seed_salt sets three per-module device words.  For a call of each module: salt S with seed s == salt 0 with seed
    s ^ S; `add` adds modulo 2^64 (the sum here wraps); and after the reset the salt-0 result is back"""
    call = _salted_call(hip, module)
    same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))
    s = SEED64
    hip.seed_salt(0, add=False)
    r0 = call(s)
    r1 = call(s ^ SALT64)
    r4 = call(s ^ SALT_SUM)
    assert not same(r0, r1) and not same(r1, r4) and not same(r0, r4)
    try:
        hip.seed_salt(SALT64, add=False)
        r2 = call(s)
        hip.seed_salt(SALT_ADD, add=True)
        r3 = call(s)
    finally:
        hip.seed_salt(0, add=False)
    assert same(r1, r2)
    assert same(r3, r4)
    assert same(call(s), r0)
