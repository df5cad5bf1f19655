"""numpy references of the adjoint of the antialiased resample (orbit2_resample_fwd with mode | ORBIT2_ANTIALIAS |
ORBIT2_TRANSPOSE: codes 21 and 22; include/orbit2_hip.h), in the manner of tests/resample_aa_ref.py, whose
taps_aa() is the one statement of the windows and their fp32 weights.

dense()            the forward operator of one axis as a matrix, fp32 [n_out, n_in]: row o holds window o's weights
member()           bool [n_out, n_in]: whether window o holds fine coordinate i (a tap on the window's edge has weight 0 and is
                   still a member: it takes part in the stated order)
cover()            how many windows hold each fine coordinate
adjoint64()        d = Ay^T g Ax with the fp32 weights, summed in float64: what the kernel approximates
emulate_adjoint()  the same field in the kernel's stated fp32 order: t[o][X] over the windows p that hold X, p ascending, a
                   product then fused multiply-adds, rounded to fp32; d[Y][X] over the windows o that hold Y in the same way
No torch, no GPU."""
import numpy as np

from tests import resample_aa_ref as A
from tests import resample_ref as R

MODES = A.MODES
TRANSPOSE = 16                                      # ORBIT2_TRANSPOSE
TILE_H, TILE_W, COVER = 32, 64, 5                   # ORBIT2_AT_TILE_H, _TILE_W, _COVER (checked against the header)
MAX_COVER = {"bilinear": 3, "bicubic": 5}           # windows that hold one fine coordinate, at every ratio >= 1
F = np.float32
ULP = R.ULP
OFFSETS = R.OFFSETS

# the pairs the window facts are checked on beyond the exhaustive sweep n_out <= n_in <= 160: (n_in, n_out)
NAMED_PAIRS = ((721, 91), (1440, 180), (512, 64), (1024, 128), (4097, 1025), (6500, 3), (300, 1))


def dense(mode, n_in, n_out):
    lo, n, w = A.taps_aa(mode, n_in, n_out)
    m = np.zeros((n_out, n_in), F)
    for o in range(n_out):
        m[o, lo[o]:lo[o] + n[o]] = w[o, :n[o]]
    return m


def member(mode, n_in, n_out):
    lo, n, _, _ = A.windows(mode, n_in, n_out)
    i = np.arange(n_in)[None, :]
    return (lo[:, None] <= i) & (i < (lo + n)[:, None])


def cover(mode, n_in, n_out):
    """int64 [n_in] from the windows alone: +1 at lo, -1 at lo + n"""
    lo, n, _, _ = A.windows(mode, n_in, n_out)
    d = np.zeros(n_in + 1, np.int64)
    np.add.at(d, lo, 1)
    np.add.at(d, lo + n, -1)
    return np.cumsum(d)[:n_in]


def adjoint64(g, size, mode):
    """float64 [B,C,H,W]; g [B,C,h,w], size = (H, W) the fine grid"""
    g = np.asarray(g)
    ay, ax = dense(mode, size[0], g.shape[2]).astype(np.float64), dense(mode, size[1], g.shape[3]).astype(np.float64)
    return ay.T[None, None] @ g.astype(np.float64) @ ax[None, None]


def _pass(g, mat, mem):
    """out[..., i] = sum over the windows p that hold i, ascending, of mat[p, i] * g[..., p]: a product, then fmaf, in fp32"""
    out = np.zeros(g.shape[:-1] + (mat.shape[1],), F)
    started = np.zeros(mat.shape[1], bool)
    for p in range(mat.shape[0]):
        cols = np.flatnonzero(mem[p])
        wgt = np.broadcast_to(mat[p, cols], out[..., cols].shape)
        gp = np.broadcast_to(g[..., p:p + 1], wgt.shape)
        first = (wgt * gp).astype(F)
        later = R._fma(wgt, gp, out[..., cols])
        out[..., cols] = np.where(started[cols], later, first)
        started[cols] = True
    assert started.all()                                             # every fine coordinate lies in a window
    return out


def emulate_adjoint(g, size, mode):
    """fp32 [B,C,H,W] in the built order"""
    g = np.asarray(g, F)
    (H, W), (h, w) = size, g.shape[2:]
    t = _pass(g, dense(mode, W, w), member(mode, W, w))                                  # [B,C,h,W]
    return np.swapaxes(_pass(np.swapaxes(t, 2, 3), dense(mode, H, h), member(mode, H, h)), 2, 3)


# ---- the cases the GPU tests run (tests/test_coarsen_gpu.py), shared with the CPU test that derives their bound: fine (H, W),
# coarse (h, w); B = 2, C = 3 -----------------------------------------------------------------------------------------------------
GPU_CASES = (
    ((40, 56), (5, 7)),                            # integer 8x, one tile
    ((80, 24), (8, 5)),                            # 10x down, 4.8x across, three tiles down
    ((64, 512), (16, 128)),                        # integer 4x, two tiles down and eight across
    ((17, 23), (6, 10)),                           # non-integer, odd width: every second row misaligned
    ((300, 7), (1, 1)),                            # one window holds the whole axis: ten tiles down read one coarse pixel
    ((7, 300), (1, 1)),
    ((8, 8), (8, 8)),                              # the identity: g bit for bit
    # one row and one column past a whole tile, and one short of it: as near to ratio 4 as those sizes come, and near 2.5
    ((TILE_H + 1, TILE_W + 1), (8, 16)),
    ((TILE_H - 1, TILE_W - 1), (7, 15)),
    ((TILE_H + 1, TILE_W + 1), (13, 27)),
    ((TILE_H - 1, TILE_W - 1), (12, 25)),
)


def gpu_input(hw, offset):
    """the gradient g fp32 [2, 3, h, w] of a case at `offset`"""
    return (R.make_input(hw, 2, 3, seed=hw[0] * 1000 + hw[1] + 17) + F(offset)).astype(F)


# ---- bounds (derived in tests/test_coarsen_cpu.py, used by the GPU tests) -----------------------------------------------------------
# the largest column sum of |weight| of a dense axis matrix over GPU_CASES (test_emulation_against_adjoint64 measures and holds
# it): sum_o |Wy[o][Y]| bounds what one fine pixel gathers per unit of max|g|.  The rows of the matrix sum to 1, so its columns
# sum to about 1 / ratio: 1 exactly at the identity, 0.49 (bilinear) and 0.54 (bicubic) at most over the other cases.
COLSUM = {"bilinear": 1.0, "bicubic": 1.0}


def ceiling(mode):
    """a derivable bound on |fp32 in the stated order - adjoint64| / max|g|.  Both use the same fp32 weights, so only the sums
    differ.  With u = 2^-24, S = COLSUM and c = MAX_COVER: each of the at most c operations of t[o][X] rounds a partial sum
    bounded by S max|g|; each of the at most c operations of d[Y][X] rounds a partial sum bounded by S^2 max|g|, and the pass
    carries t's errors times S.  Together (c + c) S^2 u."""
    return 2 * MAX_COVER[mode] * COLSUM[mode] ** 2 * ULP


# the worst the emulation shows, in units of max|g|, over GPU_CASES at offsets 0 and 280, rounded up
# (test_emulation_against_adjoint64 measures and holds these)
ADJ_EMUL_WORST = {"bilinear": 0.34 * ULP, "bicubic": 0.53 * ULP}


def field_tol(mode):
    """GPU bound on |kernel - adjoint64| / max|g|: 4 x the emulation's worst, capped by the ceiling"""
    return min(4 * ADJ_EMUL_WORST[mode], ceiling(mode))


# ---- |dense adjoint - CPU autograd of F.interpolate(antialias=True)| / max|g| in float32, per (fine, coarse, mode), measured on
# the CPU with torch 2.10 (test_dense_adjoint_against_autograd): ATen forms its weights in mixed float / double arithmetic and
# accumulates its backward in fp32, a property of the reference, not of the code under test; the bound is 4 x the measurement
AUTOGRAD_MEASURED = {
    ("40x56_5x7", "bilinear"): 1.741e-09,
    ("40x56_5x7", "bicubic"): 3.483e-09,
    ("128x256_32x64", "bilinear"): 7.72e-09,
    ("128x256_32x64", "bicubic"): 1.544e-08,
    ("17x23_6x10", "bilinear"): 7.228e-09,
    ("17x23_6x10", "bicubic"): 5.783e-08,
    ("721x1440_91x180", "bilinear"): 2.434e-09,
    ("721x1440_91x180", "bicubic"): 6.49e-09,
    ("9x13_1x1", "bilinear"): 1.53e-09,
    ("9x13_1x1", "bicubic"): 1.53e-09,
    ("30x64_8x16", "bilinear"): 5.459e-09,
    ("30x64_8x16", "bicubic"): 3.139e-08,
}
