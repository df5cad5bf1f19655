"""The float64 / numpy yardstick of the extreme-value scores: order statistics from np.sort, linear quantiles from
np.quantile on float64, tail sums and counts from boolean indexing -- and a numpy replica of the digit-pass radix select on
uint32 keys, which tests/test_extremes_cpu.py holds against np.sort on the value sets the GPU tests use."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
DIGIT_BITS, PASSES = 8, 4                       # csrc/quantile_select.h: QS_DIGIT_BITS, QS_PASSES
LEVELS = (0.0, 0.05, 0.5, 0.8413, 0.9772, 0.9987, 1.0)          # q = 0 / 1, the reference's cuts and its sigma levels


# ---- value sets ----------------------------------------------------------------------------------------------------------------
def values(name, n, seed=0):
    """n float32 values of the named set"""
    r = np.random.default_rng(seed)
    if name == "gauss0":
        v = r.standard_normal(n)
    elif name == "gauss280":
        v = 280.0 + 5.0 * r.standard_normal(n)
    elif name == "constant":
        v = np.full(n, 3.25)
    elif name == "two_valued":
        v = np.where(r.random(n) < 0.3, -1.5, 2.0)
    elif name == "zero_inflated":
        v = np.where(r.random(n) < 0.7, 0.0, r.gamma(0.5, 4.0, n))
    elif name == "ulps":                                       # 1.0 + k ulp: only the lowest digit differs
        v = (np.float32(1.0).view(np.uint32) + r.integers(0, 200, n).astype(np.uint32)).view(np.float32)
    elif name == "sign_mix":                                   # +-0, denormals, +-FLT_MAX, ordinary values of both signs
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, FLT_MAX, -FLT_MAX, 1.0, -1.0, 3.5, -2.25], dtype=np.float32)
        v = pool[r.integers(0, len(pool), n)]
        if n >= len(pool):
            v[:len(pool)] = pool                               # every one of them is there
    else:
        raise KeyError(name)
    return np.asarray(v, dtype=np.float32)


VALUE_SETS = ("gauss0", "gauss280", "constant", "two_valued", "zero_inflated", "ulps", "sign_mix")


# ---- keys and the select replica ------------------------------------------------------------------------------------------------
def key(x):
    """float32 -> the uint32 key of the same order (csrc/quantile_select.h: qs_key)"""
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31, k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def scan_step(hist, rank):
    """(bin, remaining rank): the bin in which the cumulative count first exceeds `rank`"""
    cum = np.cumsum(hist)
    b = min(int(np.searchsorted(cum, rank, side="right")), len(hist) - 1)
    return b, int(rank - (cum[b - 1] if b else 0))


def select(x, ranks):
    """the order statistics x_(r), r in ranks, of the float32 values x by the digit passes of csrc/extremes.hip: one histogram of
    the top digit, then per distinct prefix one histogram of the next digit over the keys that carry it"""
    k = key(x)
    bins, mask = 1 << DIGIT_BITS, (1 << DIGIT_BITS) - 1
    prefix, rem = [0] * len(ranks), [int(r) for r in ranks]
    for p in range(PASSES):
        shift = 32 - DIGIT_BITS * (p + 1)
        hists = {}
        for pre in set(prefix):                                 # equal prefixes share one slot
            sel = k if p == 0 else k[(k >> np.uint32(shift + DIGIT_BITS)) == pre]
            hists[pre] = np.bincount((sel >> np.uint32(shift)) & mask, minlength=bins)
        for i in range(len(ranks)):
            b, rem[i] = scan_step(hists[prefix[i]], rem[i])
            prefix[i] = (prefix[i] << DIGIT_BITS) | b
    return unkey(np.array(prefix, dtype=np.uint32))


def position(q, m):
    """(lo, hi, frac) of level q among m sorted values, as csrc/quantile_select.h: qs_position"""
    pos = float(q) * (m - 1)
    lo = min(int(np.floor(pos)), m - 1)
    return lo, min(lo + 1, m - 1), pos - lo


# ---- the yardstick --------------------------------------------------------------------------------------------------------------
def valid(target, mask=None):
    v = np.isfinite(target)
    return v if mask is None else v & (np.broadcast_to(mask, target.shape) != 0)


def quantiles(x, v, levels):
    """[Q,3] float64 rows (linear quantile of the float64 values, lower bracket, upper bracket) of x[v], and m; NaN rows at m = 0.
    levels are taken as the float32 numbers the kernel reads"""
    s = np.sort(x[v].astype(np.float32), kind="stable")
    m = s.size
    out = np.full((len(levels), 3), np.nan)
    for j, q in enumerate(np.asarray(levels, dtype=np.float32).astype(np.float64)):
        if m:
            lo, hi, _ = position(q, m)
            out[j] = (np.quantile(s.astype(np.float64), q, method="linear"), s[lo], s[hi])
    return out, m


def grouped_quantiles(pred, target, levels, mask=None, per_image=False):
    """(out [2,G,Q,3] float64, cnt [G]) as the entry lays them out; pred and target [B,C,H,W] of one size"""
    B, C = pred.shape[:2]
    v = valid(target, mask)
    groups = [(slice(b, b + 1), c) for b in range(B) for c in range(C)] if per_image else [(slice(None), c) for c in range(C)]
    out = np.empty((2, len(groups), len(levels), 3))
    cnt = np.empty(len(groups), dtype=np.int64)
    for g, (bs, c) in enumerate(groups):
        for f, x in enumerate((target, pred)):
            out[f, g], cnt[g] = quantiles(x[bs, c], v[bs, c], levels)
    return out, cnt


def tail(pred, target, thr, lat_w=None, mask=None, lower=False, per_image=False):
    """(sums [B,C,T,4] float64, cnt [B,C,T,4] int64) of the tail entry; thr float32 [G,T]"""
    B, C, H, W = pred.shape
    v = valid(target, mask)
    thr = np.asarray(thr, dtype=np.float32)
    T = thr.shape[1]
    w = np.ones(H) if lat_w is None else np.asarray(lat_w, dtype=np.float64)[:H]
    w = np.broadcast_to(w[:, None], (H, W))
    sums, cnt = np.zeros((B, C, T, 4)), np.zeros((B, C, T, 4), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            for c in range(C):
                p, t, vv = pred[b, c], target[b, c], v[b, c]
                d = p.astype(np.float64) - t.astype(np.float64)
                for k in range(T):
                    th = thr[b * C + c if per_image else c, k]
                    tin = vv & ((t <= th) if lower else (t >= th))
                    pin = vv & ((p <= th) if lower else (p >= th))
                    sums[b, c, k] = (w[tin].sum(), (w[tin] * d[tin] ** 2).sum(), (w[tin] * np.abs(d[tin])).sum(), d[tin].sum())
                    cnt[b, c, k] = (tin.sum(), (tin & pin).sum(), (~tin & pin).sum(), vv.sum())
    return sums, cnt


def ulp_distance(a, b):
    """the distance of two float32 arrays in units in the last place, through their ordered keys (+-0 one apart)"""
    return np.abs(key(a).astype(np.int64) - key(b).astype(np.int64))
