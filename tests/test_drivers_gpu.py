"""End-to-end runs of the counterpart drivers (examples/*.py) as the user would start them: one process, one GPU,
synthetic ERA5-shaped data.  Checks the reference's observable contract: epoch / batch / loss prints, the checkpoint
dictionary and its path, resume, and the tiled-inference report."""
import os
import re
import subprocess
import sys

import pytest
import torch
import yaml

from tests._child import free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, cfg, cwd):
    env = dict(os.environ, MASTER_PORT=str(free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), cfg], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_training_driver_trains_checkpoints_and_resumes(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=3, batch_size=4)
    conf["model"].update(warmup_epochs=1)
    cfg = os.path.join(tmp_path, "train.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 3 * 4 and all(l == l and l < 1e4 for l in losses)      # 3 epochs x 4 steps, finite
    ck_path = os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_2.ckpt")
    assert os.path.exists(ck_path)
    ck = torch.load(ck_path, map_location="cpu")
    assert {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"} <= set(ck.keys())
    assert ck["epoch"] == 2 and all(v.dtype == torch.float32 for v in ck["model_state_dict"].values())
    # resume from epoch 2's checkpoint for one more epoch
    conf["trainer"].update(max_epochs=4, checkpoint=ck_path)
    yaml.safe_dump(conf, open(cfg, "w"))
    out2 = _run("intermediate_downscaling.py", cfg, tmp_path)
    assert "model resume from checkpoint" in out2
    assert os.path.exists(os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_3.ckpt"))
    assert re.findall(r"epoch:  (\d+) batch_idx 0 ", out2) == ["3"]                 # continues at epoch 3 only


@pytest.mark.parametrize("loss_name", ["mse", "lat_mse", "imagegradient"])
def test_training_driver_other_registered_losses(tmp_path, loss_name):
    """every other training loss the YAML may name runs through the same driver"""
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2, train_loss=loss_name)
    conf["model"].update(depth=1, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)
    cfg = os.path.join(tmp_path, "l.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 4 and all(l == l and 0 < l < 1e4 for l in losses)


def test_training_driver_float32_flag_and_activation_checkpointing(tmp_path):
    """trainer.data_type float32 (no loss scaler; the kernels still compute in bf16 on fp32 masters) together with
    trainer.activation_checkpointing (each Block's forward is replayed in backward with the same dropout seeds)"""
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2, data_type="float32", activation_checkpointing=True)
    conf["model"].update(depth=2, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)
    cfg = os.path.join(tmp_path, "f.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 4 and all(l == l and 0 < l < 1e4 for l in losses)
    bad = dict(conf)
    bad["trainer"] = dict(conf["trainer"], data_type="float16")
    yaml.safe_dump(bad, open(cfg, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "intermediate_downscaling.py"), cfg], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Data type not supported" in r.stderr


def _write_npz_tree(root, hw, variables, rng):
    """reference on-disk format (data/processing/nc2npz.py): <root>/{train,val,test}/<year>_<shard>.npz var -> [T,1,H,W],
    lat.npy, lon.npy, normalize_{mean,std}.npz, <split>/climatology.npz"""
    import numpy as np
    H, W = hw
    for split in ("train", "val", "test"):
        os.makedirs(os.path.join(root, split))
        for sh in range(2):
            np.savez(os.path.join(root, split, "2000_%d.npz" % sh),
                     **{v: (np.abs(rng.normal(size=(3, 1, H, W))) * 1e-3 if "precip" in v else rng.normal(size=(3, 1, H, W)) + 270.0)
                        for v in variables})
        np.savez(os.path.join(root, split, "climatology.npz"), **{v: np.zeros((1, H, W)) for v in variables})
    np.save(os.path.join(root, "lat.npy"), np.linspace(-80, 80, H))
    np.save(os.path.join(root, "lon.npy"), np.linspace(0, 350, W))
    np.savez(os.path.join(root, "normalize_mean.npz"), **{v: np.array([0.5e-3 if "precip" in v else 270.0]) for v in variables})
    np.savez(os.path.join(root, "normalize_std.npz"), **{v: np.array([1e-3 if "precip" in v else 1.0]) for v in variables})


def test_drivers_over_an_on_disk_npz_tree(tmp_path):
    """the npz data plane end to end: both drivers read a reference-format directory tree (file sharding, tiling,
    normalisation, log-precipitation, Denormalize with the stored statistics)"""
    import numpy as np
    rng = np.random.default_rng(0)
    consts = ["land_sea_mask", "orography", "lattitude", "landcover"]
    outs = ["total_precipitation_24hr", "2m_temperature_min", "2m_temperature_max"]
    lo, hi = os.path.join(tmp_path, "lo"), os.path.join(tmp_path, "hi")
    _write_npz_tree(lo, (32, 64), consts + outs, rng)
    _write_npz_tree(hi, (128, 256), outs, rng)
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=3, buffer_size=4)
    conf["model"].update(depth=2, warmup_epochs=1)
    conf["data"].update(low_res_dir={"ERA5_1": lo}, high_res_dir={"ERA5_1": hi}, default_vars=consts + outs,
                        dict_in_variables={"ERA5_1": consts + outs}, dict_out_variables={"ERA5_1": outs})
    conf["data"].pop("synthetic", None)
    cfg = os.path.join(tmp_path, "disk.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 2 * 2 and all(l == l and 0 < l < 1e4 for l in losses)   # 6 samples / batch 3, two epochs
    conf["trainer"].update(pretrain=os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_1.ckpt"), batch_size=1)
    conf["tiling"] = {"do_tiling": True, "div": 2, "overlap": 4}
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("visualize.py", cfg, tmp_path)
    assert "load pretrained model" in out and "(128, 256)" in out
    m = re.search(r"rmse \[([^\]]+)\]", out)
    vals = [float(v) for v in m.group(1).split(",")]
    assert len(vals) == 4 and all(v == v and v > 0 for v in vals)
    assert vals[1] < 50.0                        # temperatures are compared in kelvin (denormalised), errors of a few K


def test_training_driver_with_spatial_tiling(tmp_path):
    """tiling.do_tiling: the data module hands out div x div tiles with an overlap halo (32x64 field, div 2, overlap 2 ->
    18x36 tiles, 162 tokens per sample: ragged attention tiles and odd GEMM row counts in a real run)"""
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=3)
    conf["tiling"] = {"do_tiling": True, "div": 2, "overlap": 2}
    conf["model"].update(depth=2, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)
    cfg = os.path.join(tmp_path, "t.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 4 and all(l == l and 0 < l < 1e4 for l in losses)
    ck = torch.load(os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_1.ckpt"), map_location="cpu")
    assert ck["model_state_dict"]["pos_embed"].shape[1] == 9 * 18


def test_training_driver_daymet_like_perceptual_loss(tmp_path, monkeypatch):
    """configs/interm_1b_daymet.yaml (7 inputs, 3 outputs, hybrid perceptual loss) with a reduced model and grid; the
    seeded stand-in LPIPS weights are an explicit opt-in (without it, and without a weights file, the loss refuses)"""
    monkeypatch.setenv("ORBIT2_LPIPS_SYNTHETIC", "1")
    monkeypatch.delenv("ORBIT2_LPIPS_WEIGHTS", raising=False)
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_1b_daymet.yaml")))
    assert conf["trainer"]["train_loss"] == "perceptual" and len(conf["data"]["dict_in_variables"]["DAYMET_1"]) == 7
    conf["trainer"].update(max_epochs=2, batch_size=2)
    conf["model"].update(embed_dim=256, depth=2, decoder_depth=1, num_heads=4, warmup_epochs=1)
    conf["data"]["synthetic"]["DAYMET_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256], steps_per_epoch=3)
    cfg = os.path.join(tmp_path, "daymet.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 6 and all(l == l and 0 < l < 1e3 for l in losses)
    assert losses[-1] < losses[0]                                   # L1 + LPIPS descends on the fixed synthetic batch set
    assert os.path.exists(os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_1.ckpt"))


def test_inference_driver_reports_stitched_metrics(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference.yaml")))
    conf["model"].update(embed_dim=256, depth=2, decoder_depth=1, num_heads=4)
    conf["data"]["synthetic"]["ERA5_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256])
    cfg = os.path.join(tmp_path, "inf.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("visualize.py", cfg, tmp_path)
    assert "stitched" in out and "(128, 256)" in out
    for name in ("rmse", "pearson", "mean_bias"):
        m = re.search(name + r" \[([^\]]+)\]", out)
        assert m, out[-1500:]
        vals = [float(v) for v in m.group(1).split(",")]
        assert len(vals) == 4 and all(v == v for v in vals)          # 3 channels + aggregate, finite
    assert os.path.exists(os.path.join(tmp_path, "0_prediction.png"))


def test_training_driver_validation_pass(tmp_path):
    """`trainer.validate: true` runs the reference's (switched-off) validation block: rmse / pearson / mean_bias on
    denormalised fields + mse, per output variable and aggregate, in eval mode after every epoch"""
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2, validate=True)
    conf["model"].update(depth=1, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)
    cfg = os.path.join(tmp_path, "v.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    vals = re.findall(r"val epoch:  (\d+) batch_idx (\d+) world_rank 0  losses  (\{.*\})", out)
    assert len(vals) >= 2 and {v[0] for v in vals} == {"0", "1"}
    d = eval(vals[-1][2])
    for metric in ("rmse", "pearson", "mean_bias", "mse"):
        assert "val/%s:aggregate" % metric in d and "val/%s:total_precipitation_24hr" % metric in d, d.keys()
        assert d["val/%s:aggregate" % metric] == d["val/%s:aggregate" % metric]        # not NaN
    assert d["val/rmse:aggregate"] > 0 and -1.0 <= d["val/pearson:aggregate"] <= 1.0


@pytest.mark.parametrize("ddp", [1, 2], ids=["tp2", "dp2xtp2"])
def test_training_driver_tensor_parallel_two_ranks_one_card(tmp_path, ddp):
    """`parallelism.tensor_par: 2` end to end: the ranks of one (or two data-parallel) tensor-parallel group(s) (gloo
    rendezvous, all on the box's single card), reference rank layout, per-rank checkpoint files `<ckpt>_rank_<r>` with the
    reference's split shapes, resume from the per-rank files."""
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2)
    conf["parallelism"].update(tensor_par=2, simple_ddp=ddp, fsdp=1)
    world = 2 * ddp
    conf["model"].update(depth=2, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)
    cfg = os.path.join(tmp_path, "tp.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))

    def run_pair():
        procs, port = [], str(free_port())
        for r in range(world):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE=str(world), RANK=str(r),
                       LOCAL_RANK="0", ORBIT2_DIST_BACKEND="gloo")
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "examples", "intermediate_downscaling.py"), cfg],
                                          cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        outs = [p.communicate(timeout=600) for p in procs]
        for p, (o, e) in zip(procs, outs):
            assert p.returncode == 0, o[-1500:] + e[-3000:]
        return outs[0][0]

    out = run_pair()
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 4 and all(l == l and 0 < l < 1e4 for l in losses)
    D, tp = conf["model"]["embed_dim"], 2
    cks = [torch.load(os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_1.ckpt_rank_%d" % r), map_location="cpu")
           for r in range(2)]
    for ck in cks:
        sd = ck["model_state_dict"]
        assert sd["blocks.0.attn.qkv.weight"].shape == (3 * D // tp, D)
        assert sd["blocks.0.mlp.fc2.weight"].shape == (D, 4 * D // tp)
        assert sd["var_agg.kv.weight"].shape == (2 * D // tp, D)
        assert sd["head.0.weight"].shape == (D, D)
    a, b = cks[0]["model_state_dict"], cks[1]["model_state_dict"]
    assert torch.equal(a["head.0.weight"], b["head.0.weight"]) and torch.equal(a["norm.weight"], b["norm.weight"])
    assert not torch.equal(a["blocks.0.attn.qkv.weight"], b["blocks.0.attn.qkv.weight"])
    # resume both ranks from their own files for one more epoch
    conf["trainer"].update(max_epochs=3, checkpoint=os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_1.ckpt"))
    yaml.safe_dump(conf, open(cfg, "w"))
    out2 = run_pair()
    assert "model resume from checkpoint" in out2
    assert re.findall(r"epoch:  (\d+) batch_idx 0 ", out2) == ["2"]


@pytest.mark.parametrize("mode", ["simple_ddp", "fsdp", "grad_op"])
def test_training_driver_two_data_parallel_ranks_one_card(tmp_path, mode):
    """the multi-rank data-parallel control flow on GPU tensors with two ranks sharing the box's card over gloo (RCCL itself
    needs one GPU per rank and is exercised by the round-end scaling run): NO_SHARD bucket all-reduce (simple_ddp: 2),
    parameter sharding = the reference's FSDP FULL_SHARD (fsdp: 2: per-unit all-gather / reduce-scatter, chunked AdamW,
    full state dict on rank 0), and the gradient / optimizer-state sharding mode (shard_strategy: grad_op)"""
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2)
    key = "fsdp" if mode == "grad_op" else mode
    conf["parallelism"].update(**{"simple_ddp": 1, "fsdp": 1, key: 2})
    if mode == "grad_op":
        conf["parallelism"]["shard_strategy"] = "grad_op"
    conf["model"].update(depth=2, warmup_epochs=1)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=3)
    cfg = os.path.join(tmp_path, "dp.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    procs, port = [], str(free_port())
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0",
                   ORBIT2_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "examples", "intermediate_downscaling.py"), cfg],
                                      cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, o[-1500:] + e[-3000:]
    out = outs[0][0]
    assert ("enter sharded optimizer" in out) == (mode == "grad_op")
    assert ("enter fully sharded FSDP" in out and "per-rank parameter bytes" in out) == (mode == "fsdp")
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 6 and all(l == l and 0 < l < 1e4 for l in losses)
    ck = torch.load(os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_1.ckpt"), map_location="cpu")
    assert all(torch.isfinite(v).all() for v in ck["model_state_dict"].values())


def test_bench_contract_two_ranks_one_card(tmp_path):
    """bench.py's multi-rank path (barrier-bracketed timing, MAX over ranks, ONE JSON line from rank 0, whole-job value)
    rehearsed with two ranks on the box's card over gloo; also with --tensor-par 2"""
    import json

    def run(extra):
        procs, port = [], str(free_port())
        for r in range(2):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK="0",
                       ORBIT2_DIST_BACKEND="gloo")
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                                           "--warmup", "1", "--model", "interm_8m", "--grid", "32x64", "--batch", "2",
                                           "--no-cpu-baseline"] + extra, cwd=tmp_path, env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.PIPE, text=True))
        outs = [p.communicate(timeout=600) for p in procs]
        for p, (o, e) in zip(procs, outs):
            assert p.returncode == 0, o[-1500:] + e[-3000:]
        # file descriptor 1 carries the result line and nothing else: bench.py sends every library banner (gloo's
        # connection chatter here, RCCL's version block on a real multi-GPU run) to stderr
        assert outs[1][0] == ""                                      # only rank 0 prints
        lines = outs[0][0].splitlines()
        assert len(lines) == 1
        return json.loads(lines[0])

    d = run([])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak" and d["unit"] == "samples/s"
    assert d["config"]["global_batch"] == 4 and d["config"]["parallelism"] == "dp2"
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]          # whole-job samples / max-rank time
    assert d["roofline"]["launches"] == 3 and d["roofline_gemm"]["launches"] > 0
    # communication accounting of the timed region: did the bucket collectives hide behind backward?
    c = d["comm"]
    assert d["comm_ms_per_step"] == c["comm_ms_per_step"] > 0 and d["exposed_comm_ms"] == c["exposed_comm_ms_per_step"] >= 0
    assert c["collectives_per_step"] >= 5                       # one or two ranges per unit: 2 Blocks... + path2 + head + root
    nparam = d["config"]["params"]
    assert 2 * nparam <= c["comm_bytes_per_step"] <= 4.5 * nparam      # bf16 buckets + the fp32 ranges of the fp32-compute parameters
    assert d["roofline_attention"]["launches"] > 0 and 0 < d["roofline_attention"]["frac"] < 1
    assert 0 < d["roofline"]["frac"] < 1 and "roofline_step" not in d      # `roofline` IS the step's executed-FLOP figure
    f = run(["--fsdp"])                                          # parameter sharding: + the units' all-gathers (forward and backward)
    assert f["comm"]["collectives_per_step"] > c["collectives_per_step"] and f["comm"]["comm_bytes_per_step"] > c["comm_bytes_per_step"]
    t = run(["--tensor-par", "2"])
    assert t["config"]["parallelism"] == "dp1xtp2" and t["config"]["global_batch"] == 2
    assert abs(t["value"] - 2 * 1e3 / t["ms_per_step"]) < 1e-6 * t["value"]


def test_bench_single_rank_line_with_baselines(tmp_path):
    """one rank, small model, --full: ONE stdout line carrying `roofline`, `cpu_baseline` (oracle on the host) and, with
    --eager-baseline, `gpu_eager_baseline` (the oracle as eager PyTorch on the GPU)"""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--model", "interm_8m",
                        "--batch", "2", "--eager-baseline", "2", "--full"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["vs_baseline"] is None and d["dtype"] == "bf16" and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and rf["unit"] == "TFLOP/s"
    # the step's figure: executed FLOPs per step / step time (one "launch" = one step), the GEMM family beside it
    assert abs(rf["achieved"] * 1e12 - rf["algorithmic_flops_per_launch"] / (rf["avg_launch_ms"] * 1e-3)) < 1e-6 * rf["achieved"] * 1e12
    assert abs(rf["frac"] - d["step_model"]["mfma_frac_of_peak_executed"]) < 1e-12 and 0 < d["roofline_gemm"]["frac"] < 1
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    ge = d["gpu_eager_baseline"]
    assert ge["value"] > 0 and ge["per_gpu_batch"] == 2


def test_bench_other_configs_and_npz_leg(tmp_path):
    """the line carries `other_configs` (each entry = a child run of this script reduced to value /
    ms_per_step / roofline.frac / config) and, with --data npz, `data_npz` (the same step fed through the reference-format data
    plane: samples/s beside the resident figure, loader CPU seconds per sample, workers)"""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--model", "interm_8m",
                        "--grid", "32x64", "--batch", "2", "--no-cpu-baseline", "--other-configs-smoke", "--data", "npz",
                        "--data-workers", "2", "--graph", "off"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    oc = d["other_configs"]
    assert list(oc) == ["interm_8m_32x64_b2"]
    e = oc["interm_8m_32x64_b2"]
    assert "error" not in e and e["value"] > 0 and e["ms_per_step"] > 0 and 0 < e["roofline"]["frac"] < 1
    assert "workload" in e["config"] and e["config"]["per_gpu_batch"] == 2 and e["command"].startswith("python bench.py --model interm_8m")
    n = d["data_npz"]
    assert n["value"] > 0 and n["resident_value"] == d["value"] and abs(n["ratio_to_resident"] - n["value"] / d["value"]) < 1e-9
    assert n["workers"] == 2 and n["loader_cpu_s_per_sample"] > 0 and n["tree"]["low_res"] == [32, 64] and n["tree"]["high_res"] == [128, 256]
    assert "npz" in d["data"]


def test_bench_sharded_engine_with_graph_replay(tmp_path):
    """round 6: `--fsdp --graph on` is no longer refused -- the parameter-sharding engine's step is captured in its single-stream
    form and replayed; the line reports the captured configuration and a finite loss"""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--model", "interm_8m",
                        "--grid", "32x64", "--batch", "2", "--no-cpu-baseline", "--fsdp", "--graph", "on"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.splitlines()[-1])
    assert d["config"]["hipgraph"] is True and d["value"] > 0
    loss = d["step_model"]["final_loss"]
    assert loss == loss and 0 < loss < 1e4


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """without --full the line carries the headline fields and none of the extra runs (`cpu_baseline`, `other_configs`);
    --dump-outputs writes the last timed step's loss and a seeded sample of the updated fp32 parameters as .npy files"""
    import json
    import numpy as np
    out_dir = os.path.join(tmp_path, "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--model", "interm_8m",
                        "--grid", "32x64", "--batch", "2", "--dump-outputs", out_dir],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert "cpu_baseline" not in d and "other_configs" not in d
    files = sorted(os.listdir(out_dir))
    assert "loss.npy" in files and "loss_scale.npy" in files and any(f.startswith("param.") for f in files)
    total = 0
    for f in files:
        a = np.load(os.path.join(out_dir, f))
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(out_dir, "loss.npy"))[0] == d["step_model"]["final_loss"]
