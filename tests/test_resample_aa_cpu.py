"""CPU checks of the antialiased resample modes (mode | ORBIT2_ANTIALIAS of orbit2_resample_fwd / orbit2_resample_moments,
_hip.resample(..., antialias=True), models.hub.Interpolation / Resampled): the numpy replica of the window contract against
ATen's F.interpolate(antialias=True), the fp32 emulation of the stated order against the replica (where the GPU tests' bounds
come from), the refusals of the two C entries, the binding against a stub library, and the module's arguments.

Bounds the GPU tests use (tests/resample_aa_ref.py): |kernel - replica| <= min(4 x the emulation's worst, the pair's ceiling)
* max|x|, the emulation's worst being 5.1 / 7.8 ulp (bilinear / bicubic) where a tile's windows fit the LDS tables and 28.2 /
73.7 ulp for the windows of hundreds to thousands of taps; the twelve sums within 4 x the emulation's worst of the sum of their
summands' magnitudes (MOMENTS_EMUL_WORST)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import resample_aa_ref as A
from tests import resample_ref as R
from tests import test_binding_cpu as TB
from tests import test_resample_cpu as TR
from tests.conftest import ROOT

hip = TB.hip                                        # the stub-library fixture of the binding tests

# |replica_aa - ATen| per case, measured on the CPU with torch 2.10: ATen forms the window in mixed float / double arithmetic and
# sums in fp32, the replica sums the contract's fp32 weights in float64 -- a property of the reference, not of the code under
# test, hence measured; the bound is 2 x the measurement, as in tests/test_resample_cpu.py.
# (pair, mode, offset): measured                in ulp(max|x|)
MEASURED = {
    ("40x56_5x7", "bilinear", 0): 2.073e-08,          # 0.0892
    ("40x56_5x7", "bicubic", 0): 3.71e-08,            # 0.16
    ("40x56_5x7", "bilinear", 280): 3.484e-05,        # 2.06
    ("40x56_5x7", "bicubic", 280): 8.091e-05,         # 4.78
    ("128x256_32x64", "bilinear", 0): 7.305e-08,      # 0.282
    ("128x256_32x64", "bicubic", 0): 1.072e-07,       # 0.414
    ("128x256_32x64", "bilinear", 280): 5.731e-05,    # 3.38
    ("128x256_32x64", "bicubic", 280): 9.589e-05,     # 5.66
    ("17x23_6x10", "bilinear", 0): 6.896e-08,         # 0.382
    ("17x23_6x10", "bicubic", 0): 3.616e-07,          # 2
    ("17x23_6x10", "bilinear", 280): 3.905e-05,       # 2.32
    ("17x23_6x10", "bicubic", 280): 8.267e-05,        # 4.9
    ("721x1440_91x180", "bilinear", 0): 6.377e-08,    # 0.189
    ("721x1440_91x180", "bicubic", 0): 1.519e-07,     # 0.45
    ("721x1440_91x180", "bilinear", 280): 8.513e-05,  # 5
    ("721x1440_91x180", "bicubic", 280): 0.0001747,   # 10.3
    ("9x13_1x1", "bilinear", 0): 1.192e-08,           # 0.0613
    ("9x13_1x1", "bicubic", 0): 1.403e-08,            # 0.0721
    ("9x13_1x1", "bilinear", 280): 1.214e-05,         # 0.719
    ("9x13_1x1", "bicubic", 280): 1.471e-05,          # 0.871
    ("5x7_40x56", "bilinear", 0): 2.794e-07,          # 1.58
    ("5x7_40x56", "bicubic", 0): 3.613e-07,           # 2.04
    ("5x7_40x56", "bilinear", 280): 4.137e-05,        # 2.46
    ("5x7_40x56", "bicubic", 280): 5.775e-05,         # 3.44
    ("30x64_8x16", "bilinear", 0): 4.105e-08,         # 0.175
    ("30x64_8x16", "bicubic", 0): 1.729e-07,          # 0.739
    ("30x64_8x16", "bilinear", 280): 4.161e-05,       # 2.46
    ("30x64_8x16", "bicubic", 280): 7.433e-05,        # 4.39
    ("24x5_7x19", "bilinear", 0): 8.785e-08,          # 0.543
    ("24x5_7x19", "bicubic", 0): 8.259e-07,           # 5.11
    ("24x5_7x19", "bilinear", 280): 3.986e-05,        # 2.37
    ("24x5_7x19", "bicubic", 280): 6.934e-05,         # 4.12
}


def _input(hw):
    return R.make_input(hw, 1, 2, seed=hw[0] * 1000 + hw[1])


def _at_offset(x, off):
    return (x + np.float32(off)).astype(np.float32)


def test_constants_match_the_header():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+ORBIT2_AA_(\w+)\s+(\d+)", hdr, flags=re.M)}
    assert d == {"TILE_H": A.TILE_H, "TILE_W": A.TILE_W, "CHUNK_ROWS": A.CHUNK_ROWS, "SRC_FLOATS": A.SRC_FLOATS,
                 "WX_FLOATS": A.WX_FLOATS, "WY_FLOATS": A.WY_FLOATS}
    assert int(re.search(r"^#define\s+ORBIT2_ANTIALIAS\s+(\d+)", hdr, flags=re.M).group(1)) == A.ANTIALIAS == _hip.ANTIALIAS == 4
    assert "the mode values 5 and 6" in hdr                               # the ABI-8 comment's list of additions
    # the paths the GPU cases exercise: the long windows form their weights in place, everything else uses the tables
    long_cases = [(hw, HW) for hw, HW in A.GPU_CASES if not A.tile_fits("bicubic", hw, HW)]
    assert long_cases == [((300, 7), (1, 1)), ((7, 300), (1, 1)), ((1, 6500), (2, 3))]
    assert all(A.tile_fits("bilinear", hw, HW) == A.tile_fits("bicubic", hw, HW) for hw, HW in A.GPU_CASES)
    # 80x24 -> 8x5 bicubic: a row window longer than one chunk of rows, still in the tables
    assert int(A.taps_aa("bicubic", 80, 8)[1].max()) > A.CHUNK_ROWS and A.tile_fits("bicubic", (80, 24), (8, 5))


def test_window_rule():
    """what the header states of the windows: inside the grid, monotone (a tile's footprint is first window .. last window), at
    most 2 ceil(support) + 1 taps, 33 for bicubic at 8x and the whole axis when reducing to one pixel, normalised weights, and a
    sum of |weight| within the 1.5 the ceiling assumes"""
    worst_s = 0.0
    for mode in A.MODES:
        for n_in, n_out in ((40, 5), (56, 7), (17, 6), (23, 10), (1440, 180), (721, 91), (9, 1), (300, 1), (8, 8), (5, 40), (7, 56),
                            (6500, 3), (1, 2), (70, 9), (6, 13)):
            lo, n, w = A.taps_aa(mode, n_in, n_out)
            assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= n_in).all()
            assert (np.diff(lo) >= 0).all() and (np.diff(lo + n) >= 0).all()
            assert n.max() <= A.max_taps(mode, n_in, n_out)
            assert np.abs(w.astype(np.float64).sum(1) - 1).max() <= 4 * R.ULP * max(1, n.max() ** 0.5)
            worst_s = max(worst_s, float(np.abs(w.astype(np.float64)).sum(1).max()))
    assert A.max_taps("bicubic", 1440, 180) == 33 and A.taps_aa("bicubic", 1440, 180)[1].max() in (32, 33)
    assert A.taps_aa("bicubic", 721, 1)[1].tolist() == [721]
    assert len({int(v) for v in A.taps_aa("bilinear", 23, 10)[1]}) > 1             # lengths differ between neighbours
    print("largest sum of |weight|: %.4g" % worst_s)
    assert worst_s <= 1.5


@pytest.mark.parametrize("hw,HW", A.SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_replica_against_aten(hw, HW):
    pair = R.case_key(hw, HW)
    for off in A.OFFSETS:
        x = _at_offset(_input(hw), off)
        for mode in A.MODES:
            rep = A.replica_aa(x, HW, mode)
            aten = Fn.interpolate(torch.from_numpy(x), HW, mode=mode, align_corners=False, antialias=True).numpy()
            err = float(np.abs(rep - aten).max())
            print("%s %s offset %d: |replica - ATen| %.4g = %.3g ulp(max|x|)" % (pair, mode, off, err,
                                                                               err / np.abs(x).max() / R.ULP))
            assert err <= 2e-6 * max(1.0, float(np.abs(x).max()))          # the agreement the contract was written to
            if hw == HW:                                                    # the identity is exact
                assert np.array_equal(rep.astype(np.float32), aten) and np.array_equal(rep, x.astype(np.float64))
            else:
                assert err <= 2 * MEASURED[(pair, mode, int(off))]


def test_antialiased_bilinear_upsample_is_the_plain_one():
    """5x7 -> 40x56: a clipped and renormalised window of two taps is the clamped index of the plain mode, so the two bilinear
    fields agree to rounding everywhere; the bicubic ones differ (A = -0.5 against -0.75)"""
    x = _input((5, 7))
    aa, plain = A.replica_aa(x, (40, 56), "bilinear"), R.replica(x, (40, 56), "bilinear")
    assert np.abs(aa - plain).max() <= 4 * R.ULP * np.abs(x).max()
    assert np.abs(A.replica_aa(x, (40, 56), "bicubic") - R.replica(x, (40, 56), "bicubic")).max() > 1e-3


def test_emulation_against_replica():
    """the stated fp32 order against float64, in units of max|x|: the worst per mode and path is under every pair's derivable
    ceiling and is what resample_aa_ref.EMUL_WORST records for the GPU bounds; the identity is exact"""
    worst = dict.fromkeys(A.EMUL_WORST, 0.0)
    cases = [(hw, HW, _input(hw), None) for hw, HW in A.SHAPES]
    cases += [(hw, HW, A.gpu_input(hw, 0.0), A.GPU_CHANNELS) for hw, HW in A.GPU_CASES]
    for hw, HW, x0, ch in cases:
        for off in A.OFFSETS:
            x = _at_offset(x0, off)
            for mode in A.MODES:
                emu = A.emulate_aa(x, HW, mode, ch)
                if hw == HW:
                    assert np.array_equal(emu, R._select(x, ch))
                e = float(np.abs(emu.astype(np.float64) - A.replica_aa(x, HW, mode, ch)).max()) / float(np.abs(x).max())
                assert e <= A.ceiling(mode, hw, HW), (hw, HW, mode, off)
                key = (mode, A.tile_fits(mode, hw, HW))
                worst[key] = max(worst[key], e)
    print("emulation worst / ulp(max|x|):", {k: round(v / R.ULP, 3) for k, v in worst.items()})
    for key in worst:
        assert 0.5 * A.EMUL_WORST[key] <= worst[key] <= A.EMUL_WORST[key]


def test_moments_emulation():
    """the twelve sums of the emulated fp32 field, added with the antialiased kernel's per-lane trip count (4 pixels in fp32, the
    wave's butterfly in fp32, float64 above), against float64 sums of the float64 replica, relative to the sum of the summands'
    magnitudes: the worst per offset and path is what resample_aa_ref.MOMENTS_EMUL_WORST records (the GPU tests allow 4 x)"""
    worst = dict.fromkeys(A.MOMENTS_EMUL_WORST, 0.0)
    for hw, HW in A.GPU_CASES:
        for off in A.OFFSETS:
            x = A.gpu_input(hw, off)
            t, lat, clim = R.gpu_target(HW, off)
            for mode in A.MODES:
                key = (int(off), A.tile_fits(mode, hw, HW))
                for aff in ((None, None), (A.GPU_SCALE, A.GPU_SHIFT)):
                    if aff[0] is not None and off:
                        continue                          # the GPU test runs the affine at offset 0 (its shift moves the field)
                    f = A.emulate_aa(x, HW, mode, A.GPU_CHANNELS, *aff)
                    rep = A.replica_aa(x, HW, mode, A.GPU_CHANNELS, *aff)
                    for lw in (None, lat):
                        for cl in (None, clim):
                            s64, mag = R.moments64(rep, t, lw, cl)
                            e = float((np.abs(A.emulate_moments_aa(f, t, lw, cl) - s64) / mag).max())
                            worst[key] = max(worst[key], e)
    print("moments emulation worst, relative to sum |summand|:", worst)
    for key in worst:
        assert 0.5 * A.MOMENTS_EMUL_WORST[key] <= worst[key] <= A.MOMENTS_EMUL_WORST[key]


# ---- the C entries refuse before any launch: addresses that are never dereferenced ---------------------------------------------
@pytest.mark.parametrize("mode", [4, 7, 8, 13, 3, -1, 4 | 8, 1 << 30])
def test_entries_refuse_other_modes(mode):
    assert TR._fwd(mode=mode) == -1
    assert TR._mom(mode=mode) == -1


@pytest.mark.parametrize("bad", [b for b in TR.BAD if "mode" not in b], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
@pytest.mark.parametrize("mode", [5, 6])
def test_entries_refuse_bad_arguments_at_antialiased_modes(bad, mode):
    assert TR._fwd(**dict(bad, mode=mode)) == -1
    assert TR._mom(**dict(bad, mode=mode)) == -1
    assert TR._mom(tgt=None, mode=mode) == -1 and TR._mom(Ht=39, mode=mode) == -1 and TR._mom(Wt=55, mode=mode) == -1


# ---- the binding, against the stub library of tests/test_binding_cpu.py ------------------------------------------------------
def _aa_cases():
    B, C, Hh, W = 2, 3, 4, 6
    return [
        ("resample", 5, dict(x=TB.t(TB.F32, B, 4, 8, 12), out=TB.t(TB.F32, B, 2, Hh, W)),
         lambda H, o: H.resample(o["x"], (Hh, W), "bilinear", channels=[3, 1], scale=[1.0, 2.0], shift=[0.0, 1.0], out=o["out"],
                                 antialias=True)),
        ("resample", 6, dict(x=TB.t(TB.F32, B, C, 8, 12)), lambda H, o: H.resample(o["x"], (Hh, W), "bicubic", antialias=True)),
        ("resample", 2, dict(x=TB.t(TB.F32, B, C, 8, 12)), lambda H, o: H.resample(o["x"], (Hh, W), "bicubic", antialias=False)),
        ("resample_moments", 6, dict(x=TB.t(TB.F32, B, C, 8, 12), target=TB.t(TB.F32, B, C, Hh + 1, W + 2), lat_w=TB.t(TB.F32, Hh),
                                     clim=TB.t(TB.F32, C, Hh, W)),
         lambda H, o: H.resample_moments(o["x"], (Hh, W), "bicubic", o["target"], lat_w=o["lat_w"], clim=o["clim"],
                                         antialias=True)),
        ("resample_moments", 5, dict(x=TB.t(TB.F32, B, C, 8, 12), target=TB.t(TB.F32, B, C, Hh, W)),
         lambda H, o: H.resample_moments(o["x"], (Hh, W), "bilinear", o["target"], antialias=True)),
    ]


AA_CASES = _aa_cases()
AA_IDS = ["%s-%d" % (c[0], c[1]) for c in AA_CASES]


@pytest.mark.parametrize("case", AA_CASES, ids=AA_IDS)
def test_antialias_reaches_the_entry_with_its_mode_code(hip, case):
    name, code, operands, call = case
    call(hip, operands)
    (entry, args), = hip.stub.calls
    assert entry == {"resample": "orbit2_resample_fwd", "resample_moments": "orbit2_resample_moments"}[name]
    assert args[-1] == TB.STREAM and args[-2] == code
    assert {v.data_ptr() for v in operands.values()} <= {a for a in args[:-1] if isinstance(a, int)}


@pytest.mark.parametrize("case", AA_CASES, ids=AA_IDS)
def test_antialias_operand_refusals(hip, case):
    _, _, operands, call = case
    for key in operands:
        bad = operands[key].clone()
        bad.flagged_host = True
        with pytest.raises(hip.HipBackendError, match="GPU tensor"):
            call(hip, dict(operands, **{key: bad}))
        with pytest.raises(hip.HipBackendError):
            call(hip, dict(operands, **{key: torch.zeros(operands[key].shape, dtype=torch.float64)}))
    assert hip.stub.calls == []


def test_nearest_has_no_antialiased_form(hip):
    x = TB.t(TB.F32, 2, 3, 8, 12)
    with pytest.raises(hip.HipBackendError, match="antialias"):
        hip.resample(x, (4, 6), "nearest", antialias=True)
    with pytest.raises(hip.HipBackendError, match="antialias"):
        hip.resample_moments(x, (4, 6), "nearest", TB.t(TB.F32, 2, 3, 4, 6), antialias=True)
    assert hip.stub.calls == []
    hip.resample(x, (4, 6), "nearest")                                      # the plain mode as before
    assert hip.stub.calls[0][1][-2] == 0
    # the argument is a keyword placed last, and the tables of the plain modes are as they were
    import inspect
    assert list(inspect.signature(hip.resample).parameters)[-1] == "antialias"
    assert list(inspect.signature(hip.resample_moments).parameters)[-1] == "antialias"
    assert hip.RESAMPLE_MODES == {"nearest": 0, "bilinear": 1, "bicubic": 2}


# ---- models.hub.Interpolation / Resampled ------------------------------------------------------------------------------------
def test_interpolation_module_takes_antialias(hip):
    from dataclasses import fields
    from climate_learn.models.hub import Interpolation, Resampled
    assert [f.name for f in fields(Resampled)][-1] == "antialias" and Resampled(torch.zeros(1, 1, 2, 2), (1, 1)).antialias is False
    with pytest.raises(ValueError, match="antialias"):
        Interpolation(size=(4, 6), mode="nearest", antialias=True)
    assert Interpolation(size=(4, 6)).antialias is False and "antialias=False" in Interpolation(size=(4, 6)).extra_repr()
    net = Interpolation(size=(4, 6), mode="bicubic", antialias=True, channels=(2, 0))
    assert "antialias=True" in net.extra_repr() and "antialias=True" in repr(net)
    x = torch.zeros(2, 3, 8, 12)
    lazy = net.lazy(x)
    assert lazy.antialias is True and lazy.mode == "bicubic" and tuple(lazy.shape) == (2, 2, 4, 6)
    a = lazy.affine([2.0, 4.0], [1.0, -1.0]).affine([0.5, 0.25], [10.0, 20.0])
    assert a.antialias is True and a.scale.tolist() == [1.0, 1.0] and a.shift.tolist() == [10.5, 19.75]
    # materialize, moments and forward pass the flag on
    lazy.materialize()
    lazy.moments(torch.zeros(2, 2, 4, 6))
    net.forward(x)
    Interpolation(size=(4, 6), mode="bicubic").forward(x)
    assert [(n, args[-2]) for n, args in hip.stub.calls] == [("orbit2_resample_fwd", 6), ("orbit2_resample_moments", 6),
                                                             ("orbit2_resample_fwd", 6), ("orbit2_resample_fwd", 2)]
