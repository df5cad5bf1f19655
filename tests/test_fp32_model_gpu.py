"""GPU tests of the fp32 forward of Res_Slim_ViT (`set_compute_dtype(torch.float32)`).

Whole model against the reference's own numbers at the project's stated fp32 tolerance: normalised max error
max|a-b| / max|b| <= 1e-4 -- against the reference goldens (tests/golden/model_*_hd64.npz, written by the reference's modules
in fp32) and against the CPU oracle in fp32 on seeded cases.  Measured on the CPU, two independent fp32 evaluations of this
model (the reference's modules and the oracle) agree with each other and with fp64 to 2e-7 ... 3.3e-7, so the bound leaves
more than two orders of magnitude for a different summation order and an exp2-based softmax; nothing that rounds a token tensor
to bf16 meets it (the bf16 path's prediction error is ~4.5e-3).  Every test prints what it measured."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import yaml

from oracle.harness import PINNED_CASES, build_pair, nerr
from tests._child import free_port
from tests.test_model_gpu import CASES, VW, load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
F32, BF = torch.float32, torch.bfloat16


@pytest.mark.parametrize("tag", list(CASES))
def test_fp32_forward_and_losses_vs_reference_golden(golden_dir, tag):
    from climate_learn.metrics import Bayesian_TV, MSE, LatWeightedMSE
    from climate_learn.metrics.utils import MetricsMetaInfo
    from climate_learn.trainer import clip_replace_constant
    c, z, sd, m = load(golden_dir, tag)
    x, y = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["y"]).cuda()
    with torch.no_grad():
        before = m(x, c["in_vars"], c["out_vars"])                       # the default (bf16) path
        assert m.set_compute_dtype(F32) is m
        pred = m(x, c["in_vars"], c["out_vars"])
        m.set_compute_dtype(BF)
        after = m(x, c["in_vars"], c["out_vars"])
    assert pred.dtype == F32 and tuple(pred.shape) == tuple(z["pred"].shape)
    e32, e16 = nerr(pred, torch.from_numpy(z["pred"])), nerr(before, torch.from_numpy(z["pred"]))
    print("[fp32 model] golden %s: pred fp32 %.2e (bf16 path %.2e)" % (tag, e32, e16))
    assert e32 <= TOL
    assert torch.equal(before, after)                                    # switching back restores the default path, bit for bit
    assert e32 < e16                                                     # and fp32 is the closer of the two
    yhat = clip_replace_constant(y, pred, c["out_vars"])
    mi = MetricsMetaInfo(c["in_vars"], c["out_vars"], z["lat"], None, None)
    losses = {"bayesian_tv": Bayesian_TV(aggregate_only=False), "lat_mse": LatWeightedMSE(False, mi), "mse": MSE(False)}
    for name, fn in losses.items():
        e = nerr(fn(yhat, y, var_names=c["out_vars"], var_weights=VW), torch.from_numpy(z["loss." + name]))
        print("[fp32 model] golden %s: loss %s %.2e" % (tag, name, e))
        assert e <= TOL, name


SEEDED = {
    "smoke": PINNED_CASES["smoke"],
    "odd_grid": PINNED_CASES["odd_grid"],                                # 10 x 20 grid, L = 50: ragged attention tail, B = 3
    "interm_117m": PINNED_CASES["interm_117m"],                          # D = 1024, 16 heads, depth 8, L = 512
    "head_dim_128": dict(D=256, depth=2, heads=2, grid=(16, 32), B=2, seed=3),
    "head_dim_256": dict(D=512, depth=1, heads=2, grid=(8, 16), B=1, seed=4),
}


@pytest.mark.parametrize("name", list(SEEDED))
def test_fp32_forward_vs_cpu_oracle(name):
    model, sd, cfg, O, x, y, in_vars, out_vars = build_pair(**SEEDED[name])
    model = model.cuda().eval().set_compute_dtype(F32)
    with torch.no_grad():
        ref = O.forward(sd, cfg, x, in_vars, out_vars)
        bf = model.set_compute_dtype(BF)(x.cuda(), in_vars, out_vars)
        pred = model.set_compute_dtype(F32)(x.cuda(), in_vars, out_vars)
    e32, e16 = nerr(pred, ref), nerr(bf, ref)
    print("[fp32 model] oracle %s: pred fp32 %.2e (bf16 path %.2e)" % (name, e32, e16))
    assert pred.dtype == F32 and e32 <= TOL and e32 < e16


def test_fp32_tiled_predict_vs_oracle_stitch():
    """2 x 2 tiling with overlap (the shape of test_inference_gpu.py::test_tiled_predict_matches_per_tile_forward): the stitched
    fp32 prediction against the oracle's fp32 forward of each tile, placed with the same windows"""
    from climate_learn.utils.visualize import tiled_predict, tile_windows
    model, sd, cfg, O, x, y, in_vars, out_vars = build_pair(D=128, depth=1, heads=2, grid=(16, 32), B=1, seed=7)
    model = model.cuda().eval().set_compute_dtype(F32)
    g = torch.Generator().manual_seed(2)
    X = torch.randn(1, len(in_vars), 32, 64, generator=g)
    Y = torch.randn(1, len(out_vars), 128, 256, generator=g)
    div, ov = 2, 4
    st = tiled_predict(model, X.cuda(), Y.cuda(), in_vars, out_vars, div, ov)
    assert st.dtype == F32 and st.shape == (1, len(out_vars), 128, 256) and model.compute_dtype is F32
    ref = torch.zeros(1, len(out_vars), 128, 256)
    with torch.no_grad():
        for t in tile_windows(32, 64, 128, 256, div, ov):
            (yi1, yi2), (xi1, xi2) = t["inp"]
            (yo1, yo2), (xo1, xo2) = t["out"]
            cfg.img_size = (yi2 - yi1, xi2 - xi1)
            p = O.clip_replace_constant(Y[:, :, yo1:yo2, xo1:xo2], O.forward(sd, cfg, X[:, :, yi1:yi2, xi1:xi2], in_vars, out_vars),
                                        out_vars)
            (ya, yb), (xa, xb) = t["crop_out"]
            (ra, rb), (ca, cb) = t["place_out"]
            ref[:, :, ra:rb, ca:cb] = p[:, :, ya:yb, xa:xb]
    e = nerr(st, ref)
    print("[fp32 model] tiled_predict 2 x 2, overlap 4 vs oracle stitch: %.2e" % e)
    assert e <= TOL


def test_fp32_forward_refusals_and_engines():
    import climate_learn as cl
    from climate_learn.models.hub.components.vit_blocks import Block
    model, sd, cfg, O, x, y, in_vars, out_vars = build_pair()
    model = model.cuda().eval().set_compute_dtype(F32)
    xd = x.cuda()
    with pytest.raises(RuntimeError, match="forward-only.*no_grad"):      # grad mode on, parameters require grad
        model(xd, in_vars, out_vars)
    model.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="training mode"):
        model(xd, in_vars, out_vars)
    model.eval()
    model.tensor_par_size = 2
    with torch.no_grad(), pytest.raises(RuntimeError, match="tensor parallelism"):
        model(xd, in_vars, out_vars)
    model.tensor_par_size = 1
    with torch.no_grad():
        alone = model(xd, in_vars, out_vars)
    # grad mode on is fine once no parameter asks for a gradient
    for p in model.parameters():
        p.requires_grad_(False)
    assert torch.equal(model(xd, in_vars, out_vars), alone)
    for p in model.parameters():
        p.requires_grad_(True)
    # under the replicated (NO_SHARD) engine the fp32 masters are whole: same result
    eng = cl.HipDataParallel(model, unit_types=(Block, nn.Sequential))
    with torch.no_grad():
        assert torch.equal(eng.module(xd, in_vars, out_vars), alone)
    # under the parameter-sharding engine they are 1/N chunks: refused
    m2 = build_pair()[0].cuda().eval().set_compute_dtype(F32)
    fs = cl.HipFullyShardedDataParallel(m2, unit_types=(Block, nn.Sequential))
    with torch.no_grad(), pytest.raises(RuntimeError, match="parameter-sharding engine"):
        fs.module(xd, in_vars, out_vars)


def _run_visualize(cfg, cwd):
    env = dict(os.environ, MASTER_PORT=str(free_port()))
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "visualize.py"), cfg], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=600)


def test_inference_driver_honours_data_type(tmp_path):
    import re
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference.yaml")))
    conf["model"].update(embed_dim=256, depth=2, decoder_depth=1, num_heads=4)
    conf["data"]["synthetic"]["ERA5_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256])
    cfg = os.path.join(tmp_path, "inf.yaml")
    out = {}
    for dt in ("float32", "bfloat16"):
        conf["trainer"]["data_type"] = dt
        yaml.safe_dump(conf, open(cfg, "w"))
        r = _run_visualize(cfg, tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "stitched" in r.stdout and "(128, 256)" in r.stdout
        assert "compute_dtype torch.%s" % dt in r.stdout                  # the flag reached the model
        vals = {}
        for name in ("rmse", "pearson", "mean_bias"):
            m = re.search(name + r" \[([^\]]+)\]", r.stdout)
            assert m, r.stdout[-1500:]
            vals[name] = [float(v) for v in m.group(1).split(",")]
            assert len(vals[name]) == 4 and all(v == v and abs(v) < 1e30 for v in vals[name])      # 3 channels + aggregate, finite
        out[dt] = vals
    print("[fp32 driver] float32 %s | bfloat16 %s" % (out["float32"], out["bfloat16"]))
    conf["trainer"]["data_type"] = "float16"
    yaml.safe_dump(conf, open(cfg, "w"))
    r = _run_visualize(cfg, tmp_path)
    assert r.returncode != 0 and "Data type not supported" in r.stderr
