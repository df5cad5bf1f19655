"""Host-only checks of the numpy mask replicas in tests/hashmask.py at 64-bit seeds.  tests/test_seeded_kernels_gpu.py compares
the kernels with these replicas at a seed whose high word is not zero; that comparison says something only if (a) the replica
itself folds the high word the way csrc/common.h:o2_hash does, (b) the high word changes the masks, and (c) the fp32 attention
oracle under the full seed's mask is far (in units of the GPU test's tolerances) from the oracle under the mask a kernel would
draw if it dropped or mangled the high word.  The attention inputs of the GPU test are generated here, so (c) is checked on
exactly the tensors that test uses."""
import numpy as np
import pytest
import torch

from tests.hashmask import (M32, attn_keep_mask, dkv_w4_hseed, droppath_scales, hash_mix, keep_mask, o2_hash64)

SEED64 = 0x9F143CDEF6E1B1FA          # high word 0x9F143CDE
SALT64 = 0xC3A5C85C97CB3127          # high word 0xC3A5C85C
LO32 = 0xFFFFFFFF
LOG2E = 1.4426950408889634

# (d, H, L, B, q stored pre-scaled) of tests/test_seeded_kernels_gpu.py section "attention, every kernel family"
ATTN_SHAPES = [(128, 2, 256, 2, True), (128, 1, 300, 1, False), (64, 2, 128, 2, False), (64, 2, 320, 1, False),
               (256, 1, 161, 1, False), (256, 1, 256, 1, False)]


def nerr(a, b):
    a = a.detach().float().cpu().double()
    b = b.detach().float().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def _attn_ref(qkv, B, L, H, d, mask=None, sc=1.0):
    q, k, v = qkv.view(B, L, 3, H, d).permute(2, 0, 3, 1, 4)
    a = ((q * d ** -0.5) @ k.transpose(-2, -1)).softmax(-1)
    if mask is not None:
        a = a * mask * sc
    return (a @ v).transpose(1, 2).reshape(B, L, H * d)


def _prescale_q(qkv, B, L, H, d):
    """what the qkv GEMM's colscale epilogue stores: the q third times log2(e)/sqrt(d), rounded to bf16 ONCE; returns
    (stored bf16 tensor, the fp32 qkv it represents exactly)"""
    x = qkv.view(B, L, 3, H * d).clone()
    x[:, :, 0] = (x[:, :, 0] * (LOG2E / d ** 0.5)).to(torch.bfloat16).float()
    stored = x.reshape(B, L, 3 * H * d)
    eff = x.clone()
    eff[:, :, 0] = eff[:, :, 0] / (LOG2E / d ** 0.5)
    return stored.to(torch.bfloat16), eff.reshape(B, L, 3 * H * d)


def attn_case_inputs(d, H, L, B, prescaled):
    """(stored bf16 qkv as the kernel reads it, the fp32 qkv it represents, bf16-rounded fp32 dO) of one attention case"""
    g = torch.Generator().manual_seed(1000 * d + 10 * L + H + B)
    qkv = torch.randn(B, L, 3 * H * d, generator=g).to(torch.bfloat16).float()
    do = torch.randn(B, L, H * d, generator=g).to(torch.bfloat16).float()
    if prescaled:
        stored, eff = _prescale_q(qkv, B, L, H, d)
    else:
        stored, eff = qkv.to(torch.bfloat16), qkv
    return stored, eff, do


def attn_oracle(eff, do, B, L, H, d, seed, p):
    """fp32 (out, dq, dk, dv) of the attention core under the host mask of `seed` (p = 0: no mask)"""
    mask, sc = None, 1.0
    if p > 0:
        m, sc = attn_keep_mask(seed, B * H, L, p)
        mask = torch.from_numpy(m).view(B, H, L, L)
    x = eff.clone().requires_grad_()
    out = _attn_ref(x, B, L, H, d, mask, sc)
    out.backward(do)
    gr = x.grad.view(B, L, 3, H * d)
    return out.detach(), gr[:, :, 0], gr[:, :, 1], gr[:, :, 2]


# ---- the replica folds the high word as o2_hash does ----------------------------------------------------------------------------
def _o2_hash_scalar(seed, idx):
    """csrc/common.h:o2_hash restated with Python integers, one value at a time (independent of the numpy code path)"""
    m = 0xFFFFFFFF
    s_lo, s_hi, lo, hi = seed & m, (seed >> 32) & m, idx & m, (idx >> 32) & m
    t = hi ^ s_hi
    h = lo ^ s_lo ^ (((t << 16) | (t >> 16)) & m) ^ ((t + (t << 3)) & m)
    h ^= h >> 16
    h = (h * 0x7FEB352D) & m
    h ^= h >> 15
    h = (h * 0x846CA68B) & m
    h ^= h >> 16
    return h


@pytest.mark.parametrize("seed", [SEED64, SEED64 ^ SALT64, 0xFFFFFFFF12345678, 7])
def test_numpy_hash_equals_the_scalar_restatement(seed):
    idx = [0, 1, 2, 255, 65535, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 0x9F143CDE00000003, 2 ** 64 - 1]
    got = o2_hash64(seed, np.array(idx, dtype=np.uint64))
    assert [int(x) for x in got] == [_o2_hash_scalar(seed, i) for i in idx]


@pytest.mark.parametrize("seed", [SEED64, SEED64 ^ SALT64, 0xFFFFFFFF12345678])
def test_dkv_w4_seed_constant_is_the_fold(seed):
    """the generated dK + dV kernel's hseed: mix(idx ^ hseed) == o2_hash64(seed, idx) for every 32-bit row index"""
    assert seed >> 32 != 0 and dkv_w4_hseed(seed) != seed & LO32
    idx = np.concatenate([np.arange(1 << 16, dtype=np.uint64),
                          np.array([2 ** 31 - 1, 2 ** 31, 2 ** 32 - 65536, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64)])
    assert np.array_equal(hash_mix(idx ^ np.uint64(dkv_w4_hseed(seed))), o2_hash64(seed, idx))
    # and with a zero high word the constant is the low word: what every seed below 2^32 exercises
    assert dkv_w4_hseed(seed & LO32) == seed & LO32
    assert int(hash_mix(np.array([5], dtype=np.uint64) ^ M32)[0]) == _o2_hash_scalar(LO32, 5)


# ---- the high word matters ------------------------------------------------------------------------------------------------------
def test_flat_mask_depends_on_the_high_word():
    n = 256 * 256
    full, sc = keep_mask(SEED64, n, 0.1)
    low, _ = keep_mask(SEED64 & LO32, n, 0.1)
    assert sc == 256.0 / 230.0
    assert float((full != low).mean()) > 0.10
    for m in (full, low):
        assert abs(float(m.mean()) - 230.0 / 256.0) < 3e-3


def test_attention_mask_depends_on_the_high_word():
    BH, L = 4, 256
    full, _ = attn_keep_mask(SEED64, BH, L, 0.1)
    low, _ = attn_keep_mask(SEED64 & LO32, BH, L, 0.1)
    top, _ = attn_keep_mask(SEED64 ^ (1 << 63), BH, L, 0.1)
    assert float((full != low).mean()) > 0.10 and float((full != top).mean()) > 0.10
    for m in (full, low, top):
        assert abs(float(m.mean()) - 230.0 / 256.0) < 3e-3


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_droppath_scales_depend_on_the_high_word(p):
    B = 4096
    full, low = droppath_scales(SEED64, B, p), droppath_scales(SEED64 & LO32, B, p)
    assert full.dtype == np.float32 and full.shape == (B,)
    assert float(((full > 0) != (low > 0)).mean()) > 0.10
    for s in (full, low):
        assert abs(float((s > 0).mean()) - (1.0 - p)) < 0.02
        assert set(np.unique(s).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}
    assert np.all(droppath_scales(SEED64, 65, 0.0) == 1.0)


# ---- discrimination precondition of the GPU attention tests ---------------------------------------------------------------------
@pytest.mark.parametrize("d,H,L,B,prescaled", ATTN_SHAPES)
def test_oracle_under_the_full_seed_is_far_from_the_truncated_seeds(d, H, L, B, prescaled):
    """a condition on the REFERENCE: out and the three gradients under the mask of SEED64 differ from those under the mask of
    the low word alone (a kernel that drops the high word) and of SEED64 ^ 2^63 (one that loses its top bit) by nerr > 0.1 --
    5x to 10x the tolerances of the GPU test (1e-2 out, 2e-2 per gradient third)"""
    _, eff, do = attn_case_inputs(d, H, L, B, prescaled)
    want = attn_oracle(eff, do, B, L, H, d, SEED64, 0.1)
    for other in (SEED64 & LO32, SEED64 ^ (1 << 63)):
        got = attn_oracle(eff, do, B, L, H, d, other, 0.1)
        for nm, a, b in zip(("out", "dq", "dk", "dv"), got, want):
            e = nerr(a, b)
            print("[precondition d=%d H=%d L=%d B=%d seed=%#x] %s %.3f" % (d, H, L, B, other, nm, e))
            assert e > 0.1, (nm, hex(other), e)
