"""float64 brute-force replica of include/orbit2_hip.h:orbit2_ensemble_scores -- TEST INFRASTRUCTURE.

Deliberately NOT sort-based, so that it shares no identity with the kernel: the pair term is the O(N^2) double sum, the
quantiles are np.quantile, the rank is counted (lt / eq) and its tie-break is tests/hashmask.py:o2_hash64."""
import numpy as np

from tests.hashmask import o2_hash64


def make_inputs(n, shape, target_hw=None, offset=0.0, seed=0):
    """members fp32 [n, B, C, H, W] = mu + sd * randn, target fp32 [B, C, Ht, Wt] = mu + 1.3 sd * randn on the top-left
    H x W (the rest is noise that must not be read), mu = 1.7 randn + offset, sd in [0.05, 0.95]; all rounded to fp32"""
    B, C, H, W = shape
    Ht, Wt = target_hw or (H, W)
    rng = np.random.default_rng(1000 * n + seed)
    mu = 1.7 * rng.standard_normal(shape) + offset
    sd = 0.05 + 0.9 * rng.random(shape)
    members = (mu + sd * rng.standard_normal((n,) + tuple(shape))).astype(np.float32)
    target = (1e3 * rng.standard_normal((B, C, Ht, Wt)) + offset).astype(np.float32)
    target[:, :, :H, :W] = (mu + 1.3 * sd * rng.standard_normal(shape)).astype(np.float32)
    return members, target


def lat_weights(H):
    w = np.cos(np.deg2rad(np.linspace(-80.0, 80.0, H)))
    return (w / w.mean()).astype(np.float32)


def pair_sum(x):
    """sum_{i<j} |x_i - x_j| over axis 0, the double sum itself"""
    acc = np.zeros(x.shape[1:], dtype=np.float64)
    for i in range(x.shape[0]):
        acc += np.abs(x[i][None] - x[i + 1:]).sum(0)
    return acc


def crps_fields(members, target):
    """(empirical, fair) per-pixel CRPS, float64 [B, C, H, W]"""
    x = members.astype(np.float64)
    n, H, W = x.shape[0], x.shape[3], x.shape[4]
    y = target.astype(np.float64)[:, :, :H, :W]
    mabs, pair = np.abs(x - y[None]).mean(0), pair_sum(x)
    return mabs - pair / (n * n), mabs - pair / (n * (n - 1))


def sums(members, target, lat_w=None):
    """float64 [B, C, 4]: sum w mean_i |d_i|, sum w sum_{i<j} |x_i - x_j|, sum w (mean_i d_i)^2, sum w var (unbiased)"""
    x = members.astype(np.float64)
    H, W = x.shape[3], x.shape[4]
    y = target.astype(np.float64)[:, :, :H, :W]
    w = np.ones(H) if lat_w is None else lat_w.astype(np.float64)[:H]
    w = w.reshape(1, 1, H, 1)
    d = x - y[None]
    parts = (np.abs(d).mean(0), pair_sum(x), d.mean(0) ** 2, x.var(0, ddof=1))
    return np.stack([(w * p).sum((2, 3)) for p in parts], axis=-1)


def ranks(members, target, seed):
    """int64 [B, C, H, W]: lt + (h * (eq + 1) >> 32), h = o2_hash64(seed, flat index of the pixel in [B, C, H, W])"""
    H, W = members.shape[3], members.shape[4]
    y = target[:, :, :H, :W]
    lt = (members < y[None]).sum(0).astype(np.uint64)
    eq = (members == y[None]).sum(0).astype(np.uint64)
    h = o2_hash64(seed, np.arange(y.size, dtype=np.uint64)).reshape(y.shape)
    return (lt + ((h * (eq + np.uint64(1))) >> np.uint64(32))).astype(np.int64)


def rank_histogram(members, target, seed):
    """int64 [B, C, N + 1]"""
    n = members.shape[0]
    r = ranks(members, target, seed)
    B, C = r.shape[:2]
    return np.stack([np.stack([np.bincount(r[b, c].ravel(), minlength=n + 1) for c in range(C)]) for b in range(B)]).astype(np.int64)


def quantiles(members, levels):
    """float64 [Q, B, C, H, W] at the fp32-rounded levels"""
    q = np.asarray(levels, dtype=np.float32).astype(np.float64)
    return np.quantile(members.astype(np.float64), q, axis=0)
