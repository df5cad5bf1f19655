"""The antialiased resample modes on the device (_hip.resample / _hip.resample_moments with antialias=True) against the float64
replica of the window contract (tests/resample_aa_ref.py), then through Resampled, metrics.functional,
utils.visualize.consistency_scores and the inference driver.

Cases (resample_aa_ref.GPU_CASES), each in both modes, at offsets 0 and 280, with and without the affine, five input channels
of which 4, 0, 2 are read, B = 2: integer 8x, 10x (a bicubic row window longer than a chunk of rows) and 4x (two tiles across,
several chunks down), a non-integer pair whose window lengths differ between neighbours, one output row and column past a whole
16 x 64 tile and one short of it (odd W: every second row misaligned), 300x7 -> 1x1, 7x300 -> 1x1 and 1x6500 -> 2x3 (windows
and a footprint row too long for LDS: weights formed in place, taps from global memory), the identity (bit-exact), an upsample
and both mixed directions.  The output is written into a NaN-filled buffer with guards on both sides, on a 16-byte boundary and
off it.

Bounds (derived in tests/test_resample_aa_cpu.py): |kernel - replica| <= field_tol * max|x| = min(4 x the emulation's worst,
the pair's ceiling), 0 for the identity; with the affine that bound times |scale[c]| plus one ulp of the result.  The twelve
sums: within MOMENTS_RTOL (4 x the emulation's worst, per offset and path) of the sum of their summands' magnitudes, against the
float64 sums of the replica field and against _hip.eval_moments(_hip.resample(...)) on the same operands."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import resample_aa_ref as A
from tests import resample_gpu_body as B
from tests import resample_ref as R
from tests._child import free_port
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
CASE_IDS = B.case_ids(A.GPU_CASES)


@pytest.mark.parametrize("hw,HW", A.GPU_CASES, ids=CASE_IDS)
def test_resample_aa_fwd(hw, HW):
    def identity_bits(got, xh, mode, off):
        if hw == HW:
            assert np.array_equal(got, xh[:, list(A.GPU_CHANNELS)]), "the identity is not exact"

    B.check_fwd(hw, HW, lambda off: A.gpu_input(hw, off), A.replica_aa,
                lambda mode: 0.0 if hw == HW else A.field_tol(mode, hw, HW), A.MODES, True, identity_bits)


@pytest.mark.parametrize("hw,HW", A.GPU_CASES, ids=CASE_IDS)
def test_resample_aa_moments(hw, HW):
    B.check_moments(hw, HW, lambda off: A.gpu_input(hw, off), A.replica_aa,
                    lambda mode, off: A.MOMENTS_RTOL[(int(off), A.tile_fits(mode, hw, HW))], A.MODES, True)


def test_plain_modes_are_untouched_and_nearest_is_refused():
    from climate_learn import _hip
    x = torch.randn(2, 3, 9, 13, device="cuda")
    for mode in R.MODES:
        assert torch.equal(_hip.resample(x, (4, 5), mode), _hip.resample(x, (4, 5), mode, antialias=False))
    assert not torch.equal(_hip.resample(x, (4, 5), "bilinear"), _hip.resample(x, (4, 5), "bilinear", antialias=True))
    with pytest.raises(_hip.HipBackendError, match="antialias"):
        _hip.resample(x, (4, 5), "nearest", antialias=True)
    # the C entries themselves: 5 and 6 run, their neighbours are refused before any launch
    out = torch.empty(2, 3, 4, 5, device="cuda")
    call = lambda m: _hip.lib().orbit2_resample_fwd(x.data_ptr(), None, 3, None, None, out.data_ptr(), 2, 3, 9, 13, 4, 5, m, None)
    assert [call(m) for m in (5, 6, 3, 4, 7, 8, 13, -1)] == [0, 0, -1, -1, -1, -1, -1, -1]
    torch.cuda.synchronize()


# ---- Resampled, the metrics and the consistency score ------------------------------------------------------------------------
IN_VARS = ["land_sea_mask", "orography", "2m_temperature", "total_precipitation_24hr", "10m_u_component_of_wind"]
OUT_VARS = ["total_precipitation_24hr", "2m_temperature", "orography"]
CHANNELS = (3, 2, 1)
SCORE_TOL = 1e-5                                     # tests/test_baseline_gpu.py: the metrics of two sets of sums that agree to 1e-6


def test_metrics_take_an_antialiased_resampled():
    from climate_learn.metrics import functional as fn
    from climate_learn.models.hub import Interpolation
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, len(IN_VARS), 36, 56, generator=g).cuda()
    y = torch.randn(2, len(OUT_VARS), 9 + 2, 14 + 3, generator=g).cuda()
    lat = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-80, 80, y.shape[2])))).float()
    clim = 0.3 * torch.randn(3, y.shape[2], y.shape[3], generator=g).cuda()
    base = torch.randn(2, 3, 9, 14, generator=g).cuda()
    for mode in A.MODES:
        lazy = Interpolation(size=(9, 14), mode=mode, antialias=True).lazy(x, IN_VARS, OUT_VARS).affine([2.0, 1.0, 0.5],
                                                                                                        [0.5, 0.0, -1.0])
        assert lazy.antialias and lazy.channels == CHANNELS
        dense = lazy.materialize()
        want = A.replica_aa(x.cpu().numpy(), (9, 14), mode, CHANNELS, [2.0, 1.0, 0.5], [0.5, 0.0, -1.0])
        bound = 2.0 * A.field_tol(mode, (36, 56), (9, 14)) * float(x.abs().max()) + 2.0 ** -23 * np.abs(want)    # as in fwd
        assert (np.abs(dense.cpu().numpy() - want) <= bound).all()
        for name, call in (("rmse", lambda p: fn.rmse(p, y)), ("lat_rmse", lambda p: fn.rmse(p, y, lat_weights=lat)),
                           ("mae", lambda p: fn.mae(p, y)), ("pearson", lambda p: fn.pearson(p, y)),
                           ("mean_bias", lambda p: fn.mean_bias(p, y)), ("acc", lambda p: fn.acc(p, y, clim, lat_weights=lat)),
                           ("mse_skill", lambda p: fn.mse_skill(p, y, base))):
            a, b = call(lazy), call(dense)
            print(mode, name, "lazy", a.tolist(), "materialised", b.tolist())
            assert a.shape == b.shape == (4,) and torch.isfinite(a).all()
            assert (a - b).abs().max() <= SCORE_TOL * max(1.0, float(b.abs().max()))


def test_consistency_scores():
    from climate_learn.models.hub import Interpolation
    from climate_learn.utils.visualize import consistency_scores
    # a smooth input (waves of 21 and 31 pixels) that covers more columns than the prediction
    b, v, i, j = torch.meshgrid(torch.arange(2.0), torch.arange(float(len(IN_VARS))), torch.arange(9.0), torch.arange(16.0),
                                indexing="ij")
    x = (torch.sin(0.3 * i + v) * torch.cos(0.2 * j + b)).cuda()
    core = x[:, :, :, :14].contiguous()
    for mode in A.MODES:
        # a smooth prediction: the materialised upsample of its own input, in the outputs' normalisation
        rescale = ([1.25, 0.5, 1.0], [0.1, -0.2, 0.0])
        up = Interpolation(superres_mag=4, mode=mode, scale=rescale[0], shift=rescale[1]).forward(core, IN_VARS, OUT_VARS)
        assert tuple(up.shape) == (2, 3, 36, 56)
        lat = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-70, 70, 9)))).float()
        got = consistency_scores(x, up, IN_VARS, OUT_VARS, mode=mode, lat_weights=lat, rescale=rescale)
        assert list(got) == OUT_VARS
        assert all(set(v) == {"consistency_rmse", "consistency_bias", "lat_consistency_rmse"} for v in got.values())
        assert set(consistency_scores(x, up, IN_VARS, OUT_VARS, mode=mode)[OUT_VARS[0]]) == {"consistency_rmse", "consistency_bias"}
        # against the numpy replica: coarsen the prediction, compare with the rescaled input channels
        coarse = A.replica_aa(up.cpu().numpy(), (9, 14), mode)
        given = core.cpu().numpy().astype(np.float64)[:, list(CHANNELS)] * np.asarray(rescale[0])[None, :, None, None] \
            + np.asarray(rescale[1])[None, :, None, None]
        d = coarse - given
        w = lat.numpy().astype(np.float64)[None, None, :, None]
        shifted = consistency_scores(x, (up + 0.75).contiguous(), IN_VARS, OUT_VARS, mode=mode, rescale=rescale)
        for c, v in enumerate(OUT_VARS[:2]):
            assert abs(got[v]["consistency_rmse"] - np.sqrt((d[:, c] ** 2).mean((1, 2))).mean()) <= SCORE_TOL
            assert abs(got[v]["lat_consistency_rmse"] - np.sqrt((w[:, 0] * d[:, c] ** 2).mean((1, 2))).mean()) <= SCORE_TOL
            assert abs(got[v]["consistency_bias"] - d[:, c].mean()) <= SCORE_TOL
            # an upsample of the input coarsens back close to it, though not exactly: interpolation and the antialiasing
            # filter both smooth over about a coarse pixel, which takes a few percent off waves this long
            assert got[v]["consistency_rmse"] < 0.1 * given[:, c].std()
            # a constant added to the prediction is its bias, and the rmse is at least that
            assert abs(shifted[v]["consistency_bias"] - got[v]["consistency_bias"] - 0.75) <= SCORE_TOL
            assert shifted[v]["consistency_rmse"] >= 0.75 - abs(got[v]["consistency_bias"]) - SCORE_TOL
        # the constant channel is reported as baseline_scores reports it
        assert got["orography"] == {"consistency_rmse": 0.0, "consistency_bias": 0.0, "lat_consistency_rmse": 0.0}
    with pytest.raises(RuntimeError, match="among the input variables"):
        consistency_scores(x, up, IN_VARS, ["geopotential_500"])


def test_inference_driver_consistency(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_consistency.yaml")))
    plain = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference.yaml")))
    assert conf.pop("consistency") == {"mode": "bilinear"} and conf == plain   # the key is the only difference
    conf["consistency"] = {"mode": "bicubic"}
    conf["baseline"] = {"mode": "bilinear"}                                     # both blocks: the order of their lines
    conf["model"].update(embed_dim=256, depth=2, decoder_depth=1, num_heads=4)
    conf["data"]["synthetic"]["ERA5_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256])
    cfg = os.path.join(tmp_path, "inf.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    env = dict(os.environ, MASTER_PORT=str(free_port()))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "visualize.py"), cfg],
                       cwd=tmp_path, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    out_vars = conf["data"]["dict_out_variables"]["ERA5_1"]
    got = [i for i, ln in enumerate(lines) if ln.startswith("consistency_scores ")]
    base = [i for i, ln in enumerate(lines) if ln.startswith("baseline_scores ")]
    assert [lines[i].split()[1] for i in got] == out_vars and len(base) == len(out_vars)
    assert max(got) < min(base) and [lines[i] for i in base] == lines[-len(out_vars):]
    for i in got:
        vals = dict(re.findall(r"'(\w+)': ([-+.\dinfae]+)", lines[i]))
        assert set(vals) == {"consistency_rmse", "consistency_bias", "lat_consistency_rmse"}
        assert all(np.isfinite(float(v)) for v in vals.values())
        assert float(vals["consistency_rmse"]) > 0 and float(vals["lat_consistency_rmse"]) > 0
