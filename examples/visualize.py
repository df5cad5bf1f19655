#!/usr/bin/env python3
"""Counterpart of the reference's examples/visualize.py (tiled inference + stitching, :340-478).

    python examples/visualize.py configs/inference.yaml

Builds the model from the YAML (same schema as the training configs), optionally loads `trainer.pretrain`
(shape-tolerant, like the reference), cuts test sample 0 into `tiling.div`^2 tiles with an `overlap` halo, runs the
HIP forward on every tile, stitches the interiors, and reports the denormalised rmse / pearson / mean_bias of the
stitched field (the reference's validation metrics, loaders.py:247-255).  Forward only; one process, one GPU.

An optional `mc_dropout: {members: N, seed: S}` block (configs/inference_mc.yaml) adds, after the deterministic run, an
MC-dropout ensemble of N stitched predictions (climate_learn.utils.mc_dropout_statistics: streamed mean and spread, same
tiling), prints gaussian_crps / gaussian_spread / gaussian_spread_skill_ratio and the 1-sigma coverage of the denormalised
field, and saves the mean and the spread as <rank>_mc_mean.npy / <rank>_mc_spread.npy.  With `scores: members` in that block
(configs/inference_mc_members.yaml) the same ensemble is then built as a member stack (climate_learn.utils.mc_dropout_members:
N fields held) and scored without the Gaussian fit: ensemble_crps, ensemble_crps_fair, ensemble_spread_skill_ratio and one
rank_histogram line per output channel are printed, <rank>_mc_rank_hist.npy and the 5 % / 50 % / 95 % quantile fields
<rank>_mc_p05.npy / _p50.npy / _p95.npy saved.

An optional `baseline: {mode: bilinear}` block (configs/inference_baseline.yaml; nearest, bilinear or bicubic) prints one
`baseline_scores` line per output variable: the rmse of the stitched field, the rmse of plain interpolation of the model's own
input, and the mean-squared-error skill of the first against the second (climate_learn.utils.visualize.baseline_scores).

An optional `consistency: {mode: bilinear}` block (configs/inference_consistency.yaml; bilinear or bicubic) prints, before any
`baseline_scores` line, one `consistency_scores` line per output variable: the stitched field coarsened back to the input grid
with antialiasing and read against the field the model was given (climate_learn.utils.visualize.consistency_scores).

An optional `extreme_scores: true` or `extreme_scores: {levels: [...]}` entry (configs/inference_extremes.yaml; default levels
+1 / +2 / +3 sigma) prints one `extreme_scores` line per output variable: for the upper tail at every level and the lower tail at
the mirrored one, the exact quantile of the target and of the stitched field, their difference, and the rmse, bias, critical
success index and frequency bias over the pixels whose target lies in that tail, in physical units
(climate_learn.utils.visualize.extreme_scores).

An optional `neighbourhood_scores: true` or `neighbourhood_scores: {levels: [...], windows: [...]}` entry
(configs/inference_fss.yaml; default levels +1 / +2 / +3 sigma, windows 1 .. 65) prints, after any `extreme_scores` line, one
`neighbourhood_scores` line per output variable: at every level the target's quantile, the base rate of the event "at or beyond
it", the fractions skill score of the stitched field at every window, the score 0.5 + base_rate / 2 that counts as skilful, and the
smallest window that reaches it (climate_learn.utils.visualize.neighbourhood_scores)."""
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]

import climate_learn as cl                                                        # noqa: E402
from climate_learn.utils.fused_attn import FusedAttn                              # noqa: E402
from climate_learn.utils.visualize import (baseline_scores, consistency_scores, extreme_scores, neighbourhood_scores,  # noqa: E402
                                           stitched_scores, tiled_predict, visualize_at_index)


def main():
    conf = yaml.load(open(sys.argv[1]), Loader=yaml.FullLoader)
    tr, mc, dc = conf["trainer"], conf["model"], conf["data"]
    tiling = conf.get("tiling", {}) or {}
    div, overlap = (tiling.get("div", 1), tiling.get("overlap", 0)) if tiling.get("do_tiling", False) else (1, 0)
    local_rank = int(os.environ.get("SLURM_LOCALID", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    data_key = next(iter(dc["low_res_dir"]))
    in_vars, out_vars = dc["dict_in_variables"][data_key], dc["dict_out_variables"][data_key]
    syn = (dc.get("synthetic") or {}).get(data_key, {})
    # the untiled module supplies whole fields (the reference's dm_vis: div=1, overlap=0)
    dm_vis = cl.data.IterDataModule("downscaling", dc["low_res_dir"][data_key], dc["high_res_dir"][data_key], in_vars,
                                    out_vars=out_vars, subsample=1, batch_size=1, div=1, overlap=0,
                                    lowres_hw=tuple(syn.get("lowres_hw", (32, 64))),
                                    highres_hw=tuple(syn["highres_hw"]) if "highres_hw" in syn else None,
                                    steps_per_epoch=syn.get("steps_per_epoch", 1)).to(device)
    dm_vis.setup()
    with torch.device(device):
        out = cl.load_downscaling_module(
            device, data_module=dm_vis, architecture=mc["preset"], train_loss=tr["train_loss"],
            model_kwargs={"default_vars": dc["default_vars"], "superres_mag": mc["superres_mag"],
                          "cnn_ratio": mc["cnn_ratio"], "patch_size": mc["patch_size"], "embed_dim": mc["embed_dim"],
                          "depth": mc["depth"], "decoder_depth": mc["decoder_depth"], "num_heads": mc["num_heads"],
                          "mlp_ratio": mc["mlp_ratio"], "drop_path": mc["drop_path"], "drop_rate": mc["drop_rate"],
                          "tensor_par_size": 1, "tensor_par_group": None, "FusedAttn_option": FusedAttn.CK})
    model, test_losses, test_transforms = out[0], out[3], out[6]
    if tr.get("pretrain"):
        print("load pretrained model", tr["pretrain"], flush=True)
        cl.utils.load_pretrained_weights(model, str(tr["pretrain"]), verbose=True)
    model = model.to(device).eval()
    # trainer.data_type (the reference's examples/intermediate_downscaling.py:593-607): float32 = the fp32 forward kernels,
    # bfloat16 (or absent) = the bf16 ones
    data_type = tr.get("data_type", "bfloat16")
    if data_type == "float32":
        model.set_compute_dtype(torch.float32)
    elif data_type != "bfloat16":
        raise RuntimeError("Data type not supported")
    print("compute_dtype", model.compute_dtype, flush=True)
    model.data_config(dc["spatial_resolution"][data_key], model.img_size, len(in_vars), len(out_vars))
    denorm = test_transforms[0]
    variable = "total_precipitation_24hr" if "total_precipitation_24hr" in out_vars else out_vars[0]
    res = visualize_at_index(model, dm_vis, dm_vis, out_list=out_vars, in_transform=denorm, out_transform=denorm,
                             variable=variable, src=data_key, device=device, div=div, overlap=overlap, index=0)
    print("stitched", {k: (v.shape if hasattr(v, "shape") else v) for k, v in res.items()}, flush=True)
    x, y, iv, ov = next(iter(dm_vis.test_dataloader()))[:4]
    x, y = x.to(device), y.to(device)
    pred_norm = tiled_predict(model, x, y, iv, ov, div, overlap)
    pred = denorm(pred_norm)
    gt = denorm(y[:, :, : pred.shape[2], : pred.shape[3]].float())
    for loss in test_losses:
        print(loss.name, [round(float(v), 6) for v in loss(pred, gt).reshape(-1)], flush=True)
    if conf.get("stitched_scores", False):
        # PSNR / SSIM of every output variable of the whole batch on the device (visualize_at_index scores one variable of one
        # sample on the host); latitude weights as the lat_* metrics build them
        for var, sc in stitched_scores(pred, gt, ov, _lat_weights(dm_vis)).items():
            print("stitched_scores", var, {k: round(v, 6) for k, v in sc.items()}, flush=True)
    extremes = conf.get("extreme_scores")
    if extremes:
        # the tails of the stitched field in physical units: exact quantiles and the scores beyond them, on the device
        # (climate_learn.utils.visualize.extreme_scores); unweighted, so level 0 is the rmse line above
        levels = extremes.get("levels") if isinstance(extremes, dict) else None
        for var, sc in extreme_scores(pred, gt, ov, levels).items():
            print("extreme_scores", var, {side: [{k: round(v, 6) for k, v in row.items()} for row in rows]
                                          for side, rows in sc.items()}, flush=True)
    neighbourhood = conf.get("neighbourhood_scores")
    if neighbourhood:
        # at which scale the stitched field places its events rightly: the fractions skill score across windows, on the device
        # (climate_learn.utils.visualize.neighbourhood_scores)
        opts = {k: neighbourhood[k] for k in ("levels", "windows") if isinstance(neighbourhood, dict) and k in neighbourhood}
        for var, rows in neighbourhood_scores(pred, gt, ov, **opts).items():
            print("neighbourhood_scores", var, [{k: ({w: round(s, 6) for w, s in v.items()} if k == "fss" else round(v, 6))
                                                 for k, v in row.items()} for row in rows], flush=True)
    consistency = conf.get("consistency")
    if consistency:
        # the stitched field coarsened back to the input grid and read against the input, both normalised as the outputs are;
        # the coarsened field is scored without being stored (climate_learn.utils.visualize.consistency_scores)
        from climate_learn.utils.loaders import _interpolation_rescale
        for var, sc in consistency_scores(x, pred_norm, iv, ov, mode=consistency.get("mode", "bilinear"),
                                          lat_weights=_lat_weights(dm_vis, pred_norm.shape[2] // x.shape[2]),
                                          rescale=_interpolation_rescale(dm_vis, ov)).items():
            print("consistency_scores", var, {k: round(v, 6) for k, v in sc.items()}, flush=True)
    baseline = conf.get("baseline")
    if baseline:
        # the same field read against plain interpolation of its own input, in physical units; the baseline is scored without
        # being stored (climate_learn.utils.visualize.baseline_scores)
        from climate_learn.utils.loaders import _interpolation_rescale
        for var, sc in baseline_scores(x, y, iv, ov, pred_norm, mode=baseline.get("mode", "bilinear"),
                                       lat_weights=_lat_weights(dm_vis), denorm=denorm,
                                       rescale=_interpolation_rescale(dm_vis, ov)).items():
            print("baseline_scores", var, {k: round(v, 6) for k, v in sc.items()}, flush=True)
    mcd = conf.get("mc_dropout")
    if mcd:
        scores = mcd.get("scores")
        if scores not in (None, "members"):
            raise RuntimeError("mc_dropout.scores: 'members' or absent, got %r" % (scores,))
        return mc_dropout_report(model, (x, y, iv, ov), gt, denorm, int(mcd["members"]), int(mcd.get("seed", 0)), div, overlap,
                                 local_rank, member_scores=scores == "members")


def _lat_weights(dm, coarsen=1):
    """cos(latitude) / its mean, as the lat_* metrics build them; None without latitudes.  coarsen = s: those of the rows of a
    grid s times coarser, a row's latitude being the mean of the s rows it covers"""
    lat = dm.get_lat_lon()[0]
    if lat is None:
        return None
    import numpy as np
    lat = np.asarray(lat, dtype=np.float64)
    if coarsen > 1:
        lat = lat[: len(lat) // coarsen * coarsen].reshape(-1, coarsen).mean(1)
    w = np.cos(np.deg2rad(lat))
    return torch.from_numpy(w / w.mean()).float()


def mc_dropout_report(model, batch, gt, denorm, members, seed, div, overlap, rank, *, member_scores=False):
    """MC-dropout ensemble of the stitched field: denormalised mean and spread (the spread takes the denormalisation's
    scale only, not its shift), the Gaussian scores against the denormalised ground truth, and the 1-sigma coverage;
    member_scores: then the all-member scores of the same ensemble (member_scores_report)"""
    from climate_learn.metrics import functional as fn
    cl.manual_seed(seed)
    stats = cl.utils.mc_dropout_statistics(batch, model, members, div=div, overlap=overlap)
    model.eval()                                                            # leave MC-dropout mode
    mean = denorm(stats.mean)
    spread = denorm(stats.std) - denorm(torch.zeros_like(stats.mean))
    normal = torch.distributions.Normal(mean, spread, validate_args=False)
    print("mc_dropout members %d seed %d" % (stats.n, seed), flush=True)
    for name, val in (("gaussian_crps", fn.gaussian_crps(normal, gt)), ("gaussian_spread", fn.gaussian_spread(normal)),
                      ("gaussian_spread_skill_ratio", fn.gaussian_spread_skill_ratio(normal, gt)),
                      ("coverage_1sigma", fn.gaussian_coverage(normal, gt))):
        print(name, [round(float(v), 6) for v in val.reshape(-1)], flush=True)
    res = {"mean": mean.detach().cpu().numpy(), "spread": spread.detach().cpu().numpy()}
    import numpy as np
    np.save("%d_mc_mean.npy" % rank, res["mean"])
    np.save("%d_mc_spread.npy" % rank, res["spread"])
    print("mc_dropout saved", {k: v.shape for k, v in res.items()}, flush=True)
    if member_scores:
        res.update(member_scores_report(model, batch, gt, denorm, members, seed, div, overlap, rank))
    return res


def member_scores_report(model, batch, gt, denorm, members, seed, div, overlap, rank):
    """the same ensemble (same seed) as a member stack, every member denormalised in its slice: all-member CRPS (empirical and
    fair), spread / skill, the rank histogram per output channel, and the 5 % / 50 % / 95 % quantile fields"""
    import numpy as np
    from climate_learn.metrics import functional as fn
    cl.manual_seed(seed)
    ens = cl.utils.mc_dropout_members(batch, model, members, div=div, overlap=overlap)
    model.eval()                                                            # leave MC-dropout mode
    for k in range(ens.n):
        ens.members[k].copy_(denorm(ens.members[k]))
    for name, val in (("ensemble_crps", fn.ensemble_crps(ens, gt)), ("ensemble_crps_fair", fn.ensemble_crps(ens, gt, fair=True)),
                      ("ensemble_spread_skill_ratio", fn.ensemble_spread_skill_ratio(ens, gt))):
        print(name, [round(float(v), 6) for v in val.reshape(-1)], flush=True)
    hist = fn.ensemble_rank_histogram(ens, gt, seed=seed).cpu().numpy()
    out_vars = batch[3]
    for c in range(hist.shape[0] - 1):
        print("rank_histogram", out_vars[c] if c < len(out_vars) else c, [int(v) for v in hist[c]], flush=True)
    q = fn.ensemble_quantiles(ens, [0.05, 0.5, 0.95]).cpu().numpy()
    res = {"rank_hist": hist, "p05": q[0], "p50": q[1], "p95": q[2]}
    for k, v in res.items():
        np.save("%d_mc_%s.npy" % (rank, k), v)
    return res


if __name__ == "__main__":
    main()
