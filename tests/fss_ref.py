"""The numpy yardstick of the fractions skill score: integer box counts from a 2-D cumulative sum with clamped
corners, the four integer sums as Python ints, the score in double -- and a replica of the kernel's own order (64-pixel words,
per-row word prefixes, prefix popcounts, running sums down a column), which tests/test_fss_cpu.py holds against the yardstick."""
import numpy as np

WINDOWS = (1, 3, 7, 33, 65, 129, 255)
PLANES = ((5, 3), (9, 63), (9, 64), (9, 65), (33, 71), (7, 129))          # the shapes of the issue's parity cases
CPU_PLANES = PLANES + ((40, 200),)


def valid(target, mask=None):
    v = np.isfinite(target)
    return v if mask is None else v & (np.broadcast_to(mask, target.shape) != 0)


def indicator(x, v, thr, lower=False):
    """valid && x >= thr (lower: <=); a NaN compares false"""
    with np.errstate(invalid="ignore"):
        return v & ((x <= np.float32(thr)) if lower else (x >= np.float32(thr)))


def box_counts(ind, n):
    """int64 [H,W]: the set pixels of the boolean plane `ind` in the n x n window around every pixel, zero beyond the plane"""
    H, W = ind.shape
    r = n // 2
    S = np.zeros((H + 1, W + 1), dtype=np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(ind.astype(np.int64), 0), 1)
    i0, i1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    j0, j1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return S[i1][:, j1] - S[i0][:, j1] - S[i1][:, j0] + S[i0][:, j0]


def sums(pred, target, thr, n, mask=None, lower=False):
    """(valid centres, sum cO^2, sum cM^2, sum (cO - cM)^2) of one plane as Python ints"""
    v = valid(target, mask)
    cO = box_counts(indicator(target, v, thr, lower), n)
    cM = box_counts(indicator(pred, v, thr, lower), n)
    return (int(v.sum()), int((cO[v] ** 2).sum()), int((cM[v] ** 2).sum()), int(((cO[v] - cM[v]) ** 2).sum()))


def score(c):
    """the double the entry rounds to fp32: 1 - c[3] / (c[1] + c[2]), NaN at 0 / 0"""
    return float("nan") if c[1] + c[2] == 0 else 1.0 - float(c[3]) / (float(c[1]) + float(c[2]))


def grouped(pred, target, thr, n, mask=None, lower=False, per_image=False):
    """(cnt int64 [B,C,T,4], fss float64 [B,C,T]) as the entry lays them out; pred and target [B,C,H,W] of one size, thr fp32
    [G,T]; mask broadcastable to [B,C,H,W]"""
    B, C = pred.shape[:2]
    thr = np.asarray(thr, dtype=np.float32)
    T = thr.shape[1]
    m = None if mask is None else np.broadcast_to(mask, pred.shape)
    cnt, out = np.zeros((B, C, T, 4), dtype=np.int64), np.zeros((B, C, T))
    for b in range(B):
        for c in range(C):
            for k in range(T):
                s = sums(pred[b, c], target[b, c], thr[b * C + c if per_image else c, k], n, None if m is None else m[b, c], lower)
                cnt[b, c, k], out[b, c, k] = s, score(s)
    return cnt, out


def pooled(cnt):
    """[C,T] float64: the score of a channel from the integers summed over the batch"""
    s = cnt.sum(0)
    return np.array([[score(tuple(int(x) for x in s[c, k])) for k in range(s.shape[1])] for c in range(s.shape[0])])


# ---- the kernel's order ----------------------------------------------------------------------------------------------------------
def pack_words(ind):
    """uint64 [H, ceil(W / 64)]: bit x & 63 of word x >> 6 is column x; bits at or beyond W are 0"""
    H, W = ind.shape
    Wq = (W + 63) // 64
    bits = np.zeros((H, Wq * 64), dtype=np.uint64)
    bits[:, :W] = ind
    return (bits.reshape(H, Wq, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def _popcount(w):
    return bin(int(w)).count("1")


def row_counts(words, W, r):
    """h(x) of one row of words for every column: P(min(x + r + 1, W)) - P(max(x - r, 0)) with P(a) = wordprefix[a >> 6] +
    popcount(word[a >> 6] & lowmask(a & 63)), the word not read at a & 63 == 0"""
    prefix = [0]
    for w in words:
        prefix.append(prefix[-1] + _popcount(w))

    def P(a):
        return prefix[a >> 6] + (_popcount(int(words[a >> 6]) & ((1 << (a & 63)) - 1)) if a & 63 else 0)

    return [P(min(x + r + 1, W)) - P(max(x - r, 0)) for x in range(W)]


def popcount_replica(pred, target, thr, n, mask=None, lower=False, band=32):
    """sums() in the kernel's order: bit words, prefix popcounts along a row, and down every column of a band a running sum that
    row s + r enters and row s - r leaves, warmed up over the rows before the band's first centre"""
    H, W = target.shape
    r = n // 2
    v = valid(target, mask)
    hO = [row_counts(row, W, r) for row in pack_words(indicator(target, v, thr, lower))]
    hM = [row_counts(row, W, r) for row in pack_words(indicator(pred, v, thr, lower))]
    zero = [0] * W
    tot = [0, 0, 0, 0]
    for y0 in range(0, H, band):
        y1 = min(y0 + band, H)
        cO, cM = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
        for s in range(max(y0 - 2 * r, -r), y1):
            e = s + r
            cO += np.array(hO[e] if 0 <= e < H else zero)
            cM += np.array(hM[e] if 0 <= e < H else zero)
            if s >= y0:
                vv = v[s]
                tot[0] += int(vv.sum())
                tot[1] += int((cO[vv] ** 2).sum())
                tot[2] += int((cM[vv] ** 2).sum())
                tot[3] += int(((cO[vv] - cM[vv]) ** 2).sum())
                q = s - r
                cO -= np.array(hO[q] if 0 <= q < H else zero)
                cM -= np.array(hM[q] if 0 <= q < H else zero)
    return tuple(tot)
