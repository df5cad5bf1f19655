"""The interpolation baseline through the public layers: models.hub.Interpolation (by name, by index, by magnification, lazy),
metrics.functional on a Resampled, mse_skill, the loader names end to end, utils.visualize.baseline_scores and the driver.

The metrics of a Resampled and of its materialised tensor are formed by the same host formulas from two sets of twelve sums
that agree within resample_ref.MOMENTS_RTOL (6.4e-7 of the summands' magnitudes at offset 0, tests/test_resample_cpu.py); the
fields here are randn at offset 0, of magnitude at most about 10 after the affine, so the scores agree within 1e-5 absolute:
rmse and mae are sums of non-negative summands (relative error 6.4e-7 of a score of order 1 to 10); pearson and acc divide an
error of 6.4e-7 sum |a b| by sqrt(sum a^2 sum b^2) >= sum |a b|; mean_bias is off by at most 6.4e-7 mean |field|."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import resample_ref as R
from tests._child import free_port
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
IN_VARS = ["land_sea_mask", "orography", "2m_temperature", "total_precipitation_24hr", "10m_u_component_of_wind"]
OUT_VARS = ["total_precipitation_24hr", "2m_temperature", "orography"]
CHANNELS = (3, 2, 1)
SCORE_TOL = 1e-5


def _fields(seed=0, hw=(9, 14), mag=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, len(IN_VARS), *hw, generator=g).cuda()
    y = torch.randn(2, len(OUT_VARS), hw[0] * mag + 2, hw[1] * mag + 3, generator=g).cuda()
    return x, y


def test_forward_by_name_index_and_magnification():
    from climate_learn.models.hub import Interpolation
    x, _ = _fields()
    for mode in R.MODES:
        want = R.replica(x.cpu().numpy(), (36, 56), mode, CHANNELS)
        by_name = Interpolation(size=(36, 56), mode=mode).forward(x, IN_VARS, OUT_VARS)
        by_index = Interpolation(size=(36, 56), mode=mode, channels=CHANNELS).forward(x)
        by_mag = Interpolation(superres_mag=4, mode=mode).forward(x, IN_VARS, OUT_VARS)
        lazy = Interpolation(superres_mag=4, mode=mode).lazy(x, IN_VARS, OUT_VARS)
        assert tuple(lazy.shape) == tuple(by_name.shape) == (2, 3, 36, 56) and by_name.dtype == torch.float32
        assert torch.equal(by_name, by_index) and torch.equal(by_name, by_mag) and torch.equal(by_name, lazy.materialize())
        err = np.abs(by_name.cpu().numpy() - want).max()
        assert err <= R.FIELD_TOL[mode] * float(x.abs().max())
        # the reference's module: no names, all channels in order
        assert torch.equal(Interpolation(size=(36, 56), mode=mode).forward(x)[:, list(CHANNELS)], by_name)
    with pytest.raises(RuntimeError, match="Interpolation requires the output variables to match the input variables."):
        Interpolation(superres_mag=4).forward(x, IN_VARS, ["geopotential_500"])
    with pytest.raises(RuntimeError, match="requires_grad"):
        Interpolation(superres_mag=4).forward(x.clone().requires_grad_())


def test_metrics_take_a_resampled():
    from climate_learn.metrics import functional as fn
    from climate_learn.models.hub import Interpolation
    x, y = _fields(1)
    lat = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-80, 80, y.shape[2])))).float()
    clim = 0.3 * torch.randn(3, y.shape[2], y.shape[3], generator=torch.Generator().manual_seed(2)).cuda()
    for mode in R.MODES:
        net = Interpolation(superres_mag=4, mode=mode, scale=[1.5, 0.5, 2.0], shift=[0.1, -0.2, 0.0])
        lazy = net.lazy(x, IN_VARS, OUT_VARS).affine([2.0, 1.0, 0.5], [0.5, 0.0, -1.0])
        dense = lazy.materialize()
        # the folded Denormalize is the same field as the transform applied afterwards, to an ulp of the result
        after = net.forward(x, IN_VARS, OUT_VARS) * torch.tensor([2.0, 1.0, 0.5], device="cuda").view(-1, 1, 1) \
            + torch.tensor([0.5, 0.0, -1.0], device="cuda").view(-1, 1, 1)
        assert ((dense - after).abs() <= 2.0 ** -22 * after.abs() + 1e-7).all()
        for name, call in (("rmse", lambda p: fn.rmse(p, y)), ("lat_rmse", lambda p: fn.rmse(p, y, lat_weights=lat)),
                           ("mae", lambda p: fn.mae(p, y)), ("pearson", lambda p: fn.pearson(p, y)),
                           ("mean_bias", lambda p: fn.mean_bias(p, y)), ("acc", lambda p: fn.acc(p, y, clim, lat_weights=lat))):
            a, b = call(lazy), call(dense)
            print(mode, name, "lazy", a.tolist(), "materialised", b.tolist())
            assert a.shape == b.shape == (4,) and torch.isfinite(a).all()
            assert (a - b).abs().max() <= SCORE_TOL


def test_mse_skill():
    from climate_learn.metrics import functional as fn
    from climate_learn.models.hub import Interpolation
    x, y = _fields(3)
    lazy = Interpolation(superres_mag=4).lazy(x, IN_VARS, OUT_VARS)
    dense = lazy.materialize()
    target = y[:, :, :36, :56].contiguous()
    assert fn.mse_skill(target, y, lazy).tolist() == [1.0] * 4                 # a perfect prediction
    assert fn.mse_skill(dense, y, dense).tolist() == [0.0] * 4                 # the baseline itself
    pred = 0.5 * (dense + target)                                              # half the error: a quarter of the MSE
    a, b = fn.mse_skill(pred, y, lazy), fn.mse_skill(pred, y, dense)
    assert (a - b).abs().max() <= SCORE_TOL and (a - 0.75).abs().max() <= 1e-5
    assert fn.mse_skill(pred, y, lazy, aggregate_only=True).dim() == 0
    lat = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-80, 80, y.shape[2])))).float()
    assert (fn.mse_skill(pred, y, lazy, lat_weights=lat) - 0.75).abs().max() <= 1e-5
    assert (fn.mse_skill(lazy, y, pred) + 3.0).abs().max() <= 1e-4             # a Resampled as the prediction: 1 - 4
    from climate_learn.metrics import METRICS_REGISTRY
    assert "mse_skill" not in METRICS_REGISTRY


def test_loader_names_end_to_end():
    import climate_learn as cl
    from climate_learn import trainer
    from climate_learn.models.hub import Interpolation
    dm = cl.data.IterDataModule("downscaling", "synthetic://lo", "synthetic://hi", IN_VARS, out_vars=OUT_VARS, batch_size=2,
                                lowres_hw=(8, 16), highres_hw=(32, 64), steps_per_epoch=1)
    dm.setup()
    device = torch.device("cuda")
    for mode in R.MODES:
        out = cl.load_downscaling_module(device, data_module=dm, architecture=mode + "-interpolation",
                                         model_kwargs={"default_vars": IN_VARS})
        net, test_losses, test_transforms = out[0], out[3], out[6]
        assert isinstance(net, Interpolation) and (net.size, net.mode, net.channels) == ((32, 64), mode, CHANNELS)
        assert net.scale is None                                               # the synthetic module: the reference's plain op
        batch = next(iter(dm.test_dataloader()))
        scores = trainer.test_step(batch, 0, net, device, test_losses, test_transforms)
        assert set(scores) == {"test/%s:%s" % (m, v) for m in ("rmse", "pearson", "mean_bias") for v in OUT_VARS + ["aggregate"]}
        assert all(torch.isfinite(v) for v in scores.values())
        assert float(scores["test/rmse:orography"]) == 0.0                     # a constant channel is the target's own
        x, y = batch[0].cuda(), batch[1].cuda()
        want = R.replica(x.cpu().numpy(), (32, 64), mode, CHANNELS)[:, 1]
        rm = np.sqrt(((want - y[:, 1].cpu().numpy().astype(np.float64)) ** 2).mean((1, 2))).mean()
        assert abs(float(scores["test/rmse:2m_temperature"]) - rm) <= 1e-5 * rm


def test_baseline_scores():
    from climate_learn.metrics import functional as fn
    from climate_learn.models.hub import Interpolation
    from climate_learn.utils.visualize import baseline_scores
    x, y = _fields(4)
    target = y[:, :, :36, :56]
    base = Interpolation(superres_mag=4, mode="bicubic").forward(x, IN_VARS, OUT_VARS)
    pred = (0.5 * (base + target)).contiguous()
    pred[:, 2] = target[:, 2]
    lat = torch.from_numpy(np.cos(np.deg2rad(np.linspace(-80, 80, y.shape[2])))).float()
    denorm = type("D", (), {"std": [1.0, 20.0, 3.0], "mean": [0.0, 280.0, 1.0],
                            "__call__": lambda s, t: t * torch.tensor(s.std, device=t.device).view(-1, 1, 1)
                            + torch.tensor(s.mean, device=t.device).view(-1, 1, 1)})()
    plain = baseline_scores(x, y, IN_VARS, OUT_VARS, pred, mode="bicubic")
    full = baseline_scores(x, y, IN_VARS, OUT_VARS, pred, mode="bicubic", lat_weights=lat, denorm=denorm)
    assert list(plain) == list(full) == OUT_VARS
    assert set(plain[OUT_VARS[0]]) == {"rmse", "rmse_baseline", "mse_skill"}
    assert set(full[OUT_VARS[0]]) == {"rmse", "rmse_baseline", "mse_skill", "lat_rmse", "lat_rmse_baseline", "lat_mse_skill"}
    want = fn.rmse(base, y)
    for c, v in enumerate(OUT_VARS[:2]):
        assert abs(plain[v]["rmse_baseline"] - float(want[c])) <= SCORE_TOL
        assert abs(plain[v]["rmse"] - 0.5 * plain[v]["rmse_baseline"]) <= SCORE_TOL
        for k in ("mse_skill", "lat_mse_skill"):                              # half the error in any unit: skill 3 / 4
            assert abs(full[v][k] - 0.75) <= 1e-4
        assert abs(plain[v]["mse_skill"] - 0.75) <= 1e-5
        # physical units: the error scales with the variable's std (the 280 K offset costs fp32 digits, hence 1e-4 relative)
        assert abs(full[v]["rmse_baseline"] - denorm.std[c] * plain[v]["rmse_baseline"]) <= 1e-4 * full[v]["rmse_baseline"]
    for d in (plain, full):                                                    # the constant channel: no error, no skill
        assert d["orography"]["rmse"] == 0.0 and d["orography"]["rmse_baseline"] == 0.0
        assert np.isnan(d["orography"]["mse_skill"])
    assert np.isnan(full["orography"]["lat_mse_skill"])


def test_inference_driver_baseline(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference_baseline.yaml")))
    plain = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference.yaml")))
    assert conf.pop("baseline") == {"mode": "bilinear"} and conf == plain      # the key is the only difference
    conf["baseline"] = {"mode": "bilinear"}
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
    got = [ln for ln in lines if ln.startswith("baseline_scores ")]
    assert [ln.split()[1] for ln in got] == out_vars and lines[-len(out_vars):] == got
    for ln in got:
        vals = dict(re.findall(r"'(\w+)': ([-+.\dinfae]+)", ln))
        assert set(vals) == {"rmse", "rmse_baseline", "mse_skill", "lat_rmse", "lat_rmse_baseline", "lat_mse_skill"}
        for k in ("rmse", "rmse_baseline", "lat_rmse", "lat_rmse_baseline"):
            assert np.isfinite(float(vals[k])) and float(vals[k]) > 0
