"""CPU checks of the interpolation baselines (orbit2_resample_fwd / orbit2_resample_moments, models.hub.Interpolation, the
loader names): the numpy replica of the coordinate contract against the golden file and ATen, the fp32 emulation of the built
summation order against the replica (where the GPU tests' bounds come from), every argument refusal of the two C entries, and
the loaders.

Bounds the GPU tests use (tests/resample_ref.py): |kernel - replica| <= min(4 x the emulation's worst, ceiling) * max|x| =
8 * 2^-24 (bilinear: the ceiling; the emulation's worst is 3.29 ulp) and 20 * 2^-24 (bicubic: 4 x 5.0; ceiling 64); the twelve
sums within 4 x the emulation's worst of the sum of their summands' magnitudes: 6.4e-7 at offset 0, 1.16e-4 at offset 280."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import resample_ref as R
from tests.conftest import GOLDEN, ROOT

# |replica - ATen| per case, measured on the CPU of the build container: ATen's own fp32 rounding of coordinates, weights and
# sums against float64 sums of the contract's fp32 taps -- a property of the reference, not of the code under test, hence
# measured; the bound is 2 x the measurement (deterministic on one torch build, an ulp or two may move on another).
# (pair, mode, offset): measured           in ulp(max|x|)
MEASURED = {
    ("5x7_40x56", "bilinear", 0): 2.272e-07,          # 1.4
    ("5x7_40x56", "bicubic", 0): 4.961e-07,           # 3.05
    ("5x7_40x56", "bilinear", 280): 4.673e-05,        # 2.77
    ("5x7_40x56", "bicubic", 280): 8.11e-05,          # 4.81
    ("16x32_128x256", "bilinear", 0): 2.643e-07,      # 1.13
    ("16x32_128x256", "bicubic", 0): 5.573e-07,       # 2.38
    ("16x32_128x256", "bilinear", 280): 5.186e-05,    # 3.07
    ("16x32_128x256", "bicubic", 280): 7.811e-05,     # 4.63
    ("6x10_17x23", "bilinear", 0): 1.236e-06,         # 7.72
    ("6x10_17x23", "bicubic", 0): 3.948e-06,          # 24.7
    ("6x10_17x23", "bilinear", 280): 5.863e-05,       # 3.48
    ("6x10_17x23", "bicubic", 280): 0.0005057,        # 30
    ("32x64_180x360", "bilinear", 0): 5.042e-06,      # 23.7
    ("32x64_180x360", "bicubic", 0): 7.473e-06,       # 35.2
    ("32x64_180x360", "bilinear", 280): 4.858e-05,    # 2.88
    ("32x64_180x360", "bicubic", 280): 0.0004415,     # 26.1
    ("91x180_721x1440", "bilinear", 0): 1.424e-05,    # 55.3
    ("91x180_721x1440", "bicubic", 0): 1.754e-05,     # 68.2
    ("91x180_721x1440", "bilinear", 280): 5.344e-05,  # 3.15
    ("91x180_721x1440", "bicubic", 280): 0.0002273,   # 13.4
    ("9x13_4x5", "bilinear", 0): 2.133e-07,           # 0.834
    ("9x13_4x5", "bicubic", 0): 8.222e-07,            # 3.21
    ("9x13_4x5", "bilinear", 280): 4.011e-05,         # 2.37
    ("9x13_4x5", "bicubic", 280): 0.0001598,          # 9.43
    ("1x1_8x8", "bilinear", 0): 2.384e-07,            # 1.7
    ("1x1_8x8", "bicubic", 0): 2.384e-07,             # 1.7
    ("1x1_8x8", "bilinear", 280): 3.052e-05,          # 1.81
    ("1x1_8x8", "bicubic", 280): 6.104e-05,           # 3.63
}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "resample.npz")))


def _at_offset(x, off):
    return (x + np.float32(off)).astype(np.float32)


def test_constants_match_the_header():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    d = {k: int(v) for k, v in re.findall(r"^#define\s+ORBIT2_RESAMPLE_(\w+)\s+(\d+)", hdr, flags=re.M)}
    assert d == {"TILE_H": R.TILE_H, "TILE_W": R.TILE_W, "LDS_FLOATS": R.LDS_FLOATS}
    assert _hip.RESAMPLE_TILE == (R.TILE_H, R.TILE_W) and _hip.RESAMPLE_LDS_FLOATS == R.LDS_FLOATS
    assert tuple(_hip.RESAMPLE_MODES) == R.MODES and list(_hip.RESAMPLE_MODES.values()) == [0, 1, 2]
    for hw, HW in R.SHAPES + R.GPU_CASES:
        assert _hip.resample_staged(*hw, *HW) == R.staged(*hw, *HW)
    # every upsampling pair and the identity stage their window; the downsampling pair reads from global memory
    assert [R.staged(*hw, *HW) for hw, HW in R.GPU_CASES] == [True, True, False, True, True, True]


@pytest.mark.parametrize("hw,HW", R.SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_replica_against_golden_and_aten(golden, hw, HW):
    pair = R.case_key(hw, HW)
    for off in R.OFFSETS:
        x = _at_offset(golden[pair + ".x"], off)
        for mode in R.MODES:
            rep = R.replica(x, HW, mode)
            aten = Fn.interpolate(torch.from_numpy(x), HW, mode=mode).numpy()
            gold = golden[R.case_key(hw, HW, mode, off)]
            sample = golden.get(pair + ".sample")
            rep_g = rep.reshape(*rep.shape[:2], -1)[..., sample] if sample is not None else rep
            errs = float(np.abs(rep - aten).max()), float(np.abs(rep_g - gold).max())
            print("%s %s offset %d: |replica - ATen| %.4g, |replica - golden| %.4g" % (pair, mode, off, *errs))
            if mode == "nearest" or hw == HW:           # a selection, and the identity, are exact
                assert np.array_equal(rep.astype(np.float32), aten) and np.array_equal(rep, rep.astype(np.float32))
                assert np.array_equal(rep_g.astype(np.float32), gold)
            else:
                assert max(errs) <= 2 * MEASURED[(pair, mode, int(off))]


def test_emulation_against_replica(golden):
    """the built fp32 order against float64, in units of max|x|: the worst per mode is under the derivable ceiling, and is what
    resample_ref.EMUL_WORST records for the GPU bounds"""
    worst = dict.fromkeys(R.MODES, 0.0)
    cases = [(hw, HW, golden[R.case_key(hw, HW) + ".x"], None) for hw, HW in R.SHAPES]
    cases += [(hw, HW, R.gpu_input(hw, HW, 0.0, golden), R.GPU_CHANNELS) for hw, HW in R.GPU_CASES]
    for hw, HW, x0, ch in cases:
        for off in R.OFFSETS:
            x = _at_offset(x0, off)
            for mode in R.MODES:
                e = float(np.abs(R.emulate(x, HW, mode, ch).astype(np.float64) - R.replica(x, HW, mode, ch)).max())
                worst[mode] = max(worst[mode], e / float(np.abs(x).max()))
    print("emulation worst / ulp(max|x|):", {m: round(v / R.ULP, 3) for m, v in worst.items()})
    assert worst["nearest"] == 0.0
    for mode in ("bilinear", "bicubic"):
        assert worst[mode] <= R.EMUL_WORST[mode] <= R.CEILING[mode]


def test_moments_emulation(golden):
    """the twelve sums of the emulated fp32 field, added with the built per-lane trip count (16 pixels in fp32, the wave's
    butterfly in fp32, float64 above), against float64 sums of the float64 replica, relative to the sum of the summands'
    magnitudes: the worst per offset is what resample_ref.MOMENTS_EMUL_WORST records (1.6e-7 at 0, 2.9e-5 at 280; the GPU tests
    allow 4 x)"""
    worst = dict.fromkeys((0, 280), 0.0)
    for hw, HW in R.GPU_CASES:
        for off in R.OFFSETS:
            x = R.gpu_input(hw, HW, off, golden)
            t, lat, clim = R.gpu_target(HW, off)
            for mode in R.MODES:
                for aff in ((None, None), (R.GPU_SCALE, R.GPU_SHIFT)):
                    if aff[0] is not None and off:
                        continue                          # the GPU test runs the affine at offset 0 (its shift moves the field)
                    f = R.emulate(x, HW, mode, R.GPU_CHANNELS, *aff)
                    rep = R.replica(x, HW, mode, R.GPU_CHANNELS, *aff)
                    for lw in (None, lat):
                        for cl in (None, clim):
                            s64, mag = R.moments64(rep, t, lw, cl)
                            e = float((np.abs(R.emulate_moments(f, t, lw, cl) - s64) / mag).max())
                            worst[int(off)] = max(worst[int(off)], e)
    print("moments emulation worst, relative to sum |summand|:", worst)
    for off in worst:
        assert worst[off] <= R.MOMENTS_EMUL_WORST[off]


# ---- the C entries refuse before any launch: addresses that are never dereferenced -------------------------------------------
X, IDX, SC, SH, OUT, TGT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def _fwd(x=X, idx=IDX, ctot=5, sc=SC, sh=SH, out=OUT, B=2, C=3, h=5, w=7, H=40, W=56, mode=1):
    from climate_learn import _hip
    return _hip.lib().orbit2_resample_fwd(x, idx, ctot, sc, sh, out, B, C, h, w, H, W, mode, None)


def _mom(x=X, idx=IDX, ctot=5, sc=SC, sh=SH, tgt=TGT, Ht=43, Wt=61, out=OUT, B=2, C=3, h=5, w=7, H=40, W=56, mode=1):
    from climate_learn import _hip
    return _hip.lib().orbit2_resample_moments(x, idx, ctot, sc, sh, tgt, Ht, Wt, None, None, out, B, C, h, w, H, W, mode, None)


BAD = [dict(x=None), dict(out=None), dict(sc=None), dict(sh=None), dict(idx=None), dict(idx=None, ctot=4), dict(mode=-1),
       dict(mode=3), dict(B=0), dict(C=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=0), dict(ctot=0), dict(B=257, C=256)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_entries_refuse_bad_arguments(bad):
    assert _fwd(**bad) == -1
    assert _mom(**bad) == -1


def test_moments_refuses_its_own_arguments():
    assert _mom(tgt=None) == -1
    assert _mom(Ht=39) == -1 and _mom(Wt=55) == -1


def test_binding_refuses_before_the_device():
    """_hip validates the channel list on the host (the C entry trusts its device copy), and the rest of the call's shape"""
    from climate_learn import _hip
    x = torch.zeros(2, 5, 5, 7)
    for ch in ([0, 5], [-1], [4, 0, 7]):
        with pytest.raises(_hip.HipBackendError, match="channels .* outside 0..4"):
            _hip.resample(x, (40, 56), "bilinear", channels=ch)
        with pytest.raises(_hip.HipBackendError, match="channels .* outside 0..4"):
            _hip.resample_moments(x, (40, 56), "bilinear", torch.zeros(2, len(ch), 40, 56), channels=ch)
    with pytest.raises(_hip.HipBackendError, match="mode is one of"):
        _hip.resample(x, (40, 56), "area")
    with pytest.raises(_hip.HipBackendError, match="size is"):
        _hip.resample(x, 40, "bilinear")
    with pytest.raises(_hip.HipBackendError, match="must be positive"):
        _hip.resample(x, (0, 56), "bilinear")
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.resample(x, (40, 56), "bilinear", channels=[4, 0, 2])       # a valid call stops at the device check: no CPU path


# ---- models.hub.Interpolation and the loader names -----------------------------------------------------------------------------
IN_VARS = ["land_sea_mask", "2m_temperature", "total_precipitation_24hr", "10m_u_component_of_wind"]
OUT_VARS = ["total_precipitation_24hr", "2m_temperature"]


def _dm(in_vars=IN_VARS, out_vars=OUT_VARS, transforms=None, output_transforms=None):
    dm = SimpleNamespace(get_data_variables=lambda: (in_vars, out_vars),
                         get_data_dims=lambda: (torch.Size([2, len(in_vars), 8, 16]), torch.Size([2, len(out_vars), 30, 64])))
    if transforms is not None:
        dm.transforms, dm.output_transforms = transforms, output_transforms
    return dm


@pytest.mark.parametrize("mode", R.MODES)
def test_loader_builds_an_interpolation(mode):
    from climate_learn.models.hub import MODEL_REGISTRY, Interpolation
    from climate_learn.utils.loaders import load_architecture, load_optimizer
    assert MODEL_REGISTRY["interpolation"] is Interpolation
    net = load_architecture("downscaling", _dm(), mode + "-interpolation", default_vars=IN_VARS)
    assert isinstance(net, Interpolation)
    assert (net.size, net.mode, net.channels, net.superres_mag) == ((30, 64), mode, (2, 1), None)
    assert net.scale is None and net.shift is None            # no separate statistics: the reference's plain op
    assert list(net.parameters()) == []
    with pytest.warns(UserWarning, match="no trainable parameters"):
        assert load_optimizer(net, "adamw") is None


def test_loader_rescale_and_refusals():
    from climate_learn.utils.loaders import load_architecture
    norm = lambda m, s: SimpleNamespace(mean=m, std=s)                    # noqa: E731
    tin = {"land_sea_mask": norm(0.3, 0.4), "2m_temperature": norm(280.0, 20.0), "total_precipitation_24hr": object(),
           "10m_u_component_of_wind": norm(1.0, 5.0)}
    shared = {v: tin[v] for v in OUT_VARS}
    net = load_architecture("downscaling", _dm(transforms=tin, output_transforms=shared), "bilinear-interpolation",
                            default_vars=IN_VARS)
    assert net.scale is None and net.shift is None            # shared statistics: the identity
    tout = {"total_precipitation_24hr": object(), "2m_temperature": norm(275.0, 16.0)}
    net = load_architecture("downscaling", _dm(transforms=tin, output_transforms=tout), "Bicubic-Interpolation",
                            default_vars=IN_VARS)
    assert net.mode == "bicubic"
    assert net.scale.tolist() == [1.0, 20.0 / 16.0] and net.shift.tolist() == [0.0, (280.0 - 275.0) / 16.0]
    # an output variable that is not among the inputs: the reference's message
    with pytest.raises(RuntimeError, match="Interpolation requires the output variables to match the input variables."):
        load_architecture("downscaling", _dm(out_vars=["2m_temperature", "geopotential_500"]), "nearest-interpolation",
                          default_vars=IN_VARS)
    # every other name as before
    for task, arch in (("downscaling", "vit"), ("downscaling", "trilinear-interpolation"),
                       ("forecasting", "bilinear-interpolation")):
        with pytest.raises(NotImplementedError, match="%s is not an implemented architecture for the %s task" % (arch, task)):
            load_architecture(task, _dm(), arch, default_vars=IN_VARS)


def test_res_slimvit_still_loads():
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.utils.loaders import load_architecture
    net = load_architecture("downscaling", _dm(), "res_slimvit", default_vars=IN_VARS, embed_dim=64, depth=1, num_heads=2)
    assert isinstance(net, Res_Slim_ViT)


def test_interpolation_module_arguments():
    from climate_learn.models.hub import Interpolation, Resampled
    for kw in (dict(), dict(size=(8, 8), superres_mag=2), dict(size=(8, 8), mode="area"), dict(size=(8, 8), scale=[1.0]),
               dict(superres_mag=0)):
        with pytest.raises(ValueError):
            Interpolation(**kw)
    net = Interpolation(superres_mag=4, mode="nearest")
    x = torch.zeros(2, 4, 3, 5)
    lazy = net.lazy(x, IN_VARS, OUT_VARS)
    assert isinstance(lazy, Resampled) and lazy.channels == (2, 1) and tuple(lazy.shape) == (2, 2, 12, 20)
    assert net.lazy(x).channels is None and tuple(net.lazy(x).shape) == (2, 4, 12, 20)
    with pytest.raises(RuntimeError, match="Interpolation requires the output variables to match the input variables."):
        net.lazy(x, IN_VARS, ["geopotential_500"])
    with pytest.raises(RuntimeError, match="requires_grad"):
        net.forward(x.clone().requires_grad_(), IN_VARS, OUT_VARS)
    # a Denormalize folds into the descriptor: (s r + t) std + mean = (s std) r + (t std + mean)
    a = lazy.affine([2.0, 4.0], [1.0, -1.0])
    assert a.scale.tolist() == [2.0, 4.0] and a.shift.tolist() == [1.0, -1.0]
    b = a.affine([0.5, 0.25], [10.0, 20.0])
    assert b.scale.tolist() == [1.0, 1.0] and b.shift.tolist() == [10.5, 19.75]
    assert b.x is lazy.x and b.channels == lazy.channels and lazy.scale is None
