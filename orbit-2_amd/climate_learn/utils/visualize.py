"""Tiled inference + stitching (reference: utils/visualize.py:38-330, examples/visualize.py:340-478).

The field is cut into div x div tiles, every tile is enlarged by a halo taken from its neighbours (edge tiles grow
inwards only, so all tiles have the same size), the model runs on each enlarged tile, and only the tile's own
interior is written into the stitched prediction.  Window arithmetic follows the reference line by line, with one
decision: the reference shifts the ground-truth window of non-first tile rows by `top ** vmul` (:211, a typo for
`top * vmul` -- the two agree only for top in {0, 1} x vmul = 1); the halo-consistent product is used here.
Forward only (`torch.no_grad()`), everything stays on the device until the stitched arrays are returned."""
from typing import Dict, List, Tuple

import numpy as np
import torch


def halo(overlap: int) -> Tuple[int, int, int, int]:
    """(top, bottom, left, right) halo in input pixels (reference :62-69; the grid is 2:1, so columns get twice the rows)"""
    if overlap % 2 == 0:
        top = bottom = overlap // 2
        left = right = overlap // 2 * 2
    else:
        left = overlap // 2 * 2
        right = (overlap // 2 + 1) * 2
        top = overlap // 2
        bottom = overlap // 2 + 1
    return top, bottom, left, right


def _axis_windows(n_in: int, n_out: int, div: int, lo: int, hi: int, mul: int):
    """per tile index: (in window, out window, interior inside the in tile, interior inside the out tile, placement in / out)"""
    res = []
    for idx in range(div):
        if div == 1:
            res.append(((0, n_in), (0, n_out), (0, n_in), (0, n_out), (0, n_in), (0, n_out)))
            continue
        i1, i2 = n_in // div * idx, n_in // div * (idx + 1)
        o1, o2 = n_out // div * idx, n_out // div * (idx + 1)
        r_in, r_out = (i1, i2), (o1, o2)
        if idx == 0:
            i2 += lo
            o2 += lo * mul
        else:
            i1 -= lo
            o1 -= lo * mul
        if idx == div - 1:
            i1 -= hi
            o1 -= hi * mul
        else:
            i2 += hi
            o2 += hi * mul
        if idx == 0:
            t_in, t_out = (0, n_in // div), (0, n_out // div)
        elif idx == div - 1:
            t_in = (lo + hi, lo + hi + n_in // div)
            t_out = ((lo + hi) * mul, (lo + hi) * mul + n_out // div)
        else:
            t_in = (lo, lo + n_in // div)
            t_out = (lo * mul, lo * mul + n_out // div)
        res.append(((i1, i2), (o1, o2), t_in, t_out, r_in, r_out))
    return res


def tile_windows(yinp: int, xinp: int, yout: int, xout: int, div: int, overlap: int) -> List[Dict]:
    """the div*div tiles in the reference's (vindex, hindex) order"""
    top, bottom, left, right = halo(overlap)
    vmul, hmul = yout // yinp, xout // xinp
    rows = _axis_windows(yinp, yout, div, top, bottom, vmul)
    cols = _axis_windows(xinp, xout, div, left, right, hmul)
    tiles = []
    for v, (yi, yo, yit, yot, yir, yor) in enumerate(rows):
        for h, (xi, xo, xit, xot, xir, xor_) in enumerate(cols):
            tiles.append(dict(vindex=v, hindex=h, inp=(yi, xi), out=(yo, xo), crop_in=(yit, xit), crop_out=(yot, xot),
                              place_in=(yir, xir), place_out=(yor, xor_)))
    return tiles


def tiled_predict(mm, x, y, in_variables, out_variables, div: int, overlap: int, clip=None):
    """x: [B,V,yinp,xinp], y: [B,C,>=yout,>=xout] (normalised target; constant output channels are copied from it as
    in training).  Returns the stitched prediction [B,C,yout,xout] (fp32, on x's device)."""
    from ..trainer import clip_replace_constant
    clip = clip or clip_replace_constant
    B, _, yinp, xinp = x.shape
    mag = mm.superres_mag
    yout, xout = yinp * mag, xinp * mag
    preds = torch.zeros(B, len(out_variables), yout, xout, dtype=torch.float32, device=x.device)
    # the reference builds the data module with the same (div, overlap), so the model is data_config'd to the tile
    # size before it gets here; do that rebinding (no weights change) when the caller has not
    saved = None
    with torch.no_grad():
        for t in tile_windows(yinp, xinp, yout, xout, div, overlap):
            (yi1, yi2), (xi1, xi2) = t["inp"]
            (yo1, yo2), (xo1, xo2) = t["out"]
            xdiv = x[:, :, yi1:yi2, xi1:xi2].contiguous()
            ydiv = y[:, :, yo1:yo2, xo1:xo2]
            ps = int(getattr(mm, "patch_size", 1))
            if xdiv.shape[2] % ps or xdiv.shape[3] % ps:
                raise ValueError("tiled_predict: the tile %d x %d (div=%d, overlap=%d, halo included) is not a multiple of "
                                 "patch_size=%d" % (xdiv.shape[2], xdiv.shape[3], div, overlap, ps))
            if hasattr(mm, "data_config") and tuple(getattr(mm, "img_size", xdiv.shape[2:])) != tuple(xdiv.shape[2:]):
                if saved is None:
                    saved = (mm.spatial_resolution, mm.img_size, mm.in_channels, mm.out_channels)
                mm.data_config(mm.spatial_resolution, tuple(xdiv.shape[2:]), mm.in_channels, mm.out_channels)
            pred = mm.forward(xdiv, in_variables, out_variables)
            pred = clip(ydiv, pred, out_variables)
            (ya, yb), (xa, xb) = t["crop_out"]
            (ra, rb), (ca, cb) = t["place_out"]
            preds[:, :, ra:rb, ca:cb] = pred[:, :, ya:yb, xa:xb].float()
    if saved is not None:
        mm.data_config(*saved)
    return preds


def psnr_ssim(groundtruth, pred, win: int = 7):
    """Goodness of fit of a stitched field, as the reference prints it (utils/visualize.py:366-372: scikit-image's
    peak_signal_noise_ratio and structural_similarity with data_range = max - min of the ground truth).
    PSNR = 10 log10(range^2 / MSE) (closed form); the squared error sum comes from the evaluation-moment kernel
    (orbit2_eval_moments) when the fields are device tensors.  SSIM is restated from the published definition with
    scikit-image's defaults (7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, mean over the map without its
    3-pixel border); scikit-image is absent from this image, so that part is *parity unpinned* (SURVEY 8c)."""
    from scipy.ndimage import uniform_filter
    if torch.is_tensor(groundtruth) and groundtruth.is_cuda:
        from .. import _hip
        g4, p4 = groundtruth.reshape(1, 1, *groundtruth.shape[-2:]).float().contiguous(), pred.reshape(1, 1, *pred.shape[-2:]).float().contiguous()
        mom = _hip.eval_moments(p4, g4)                         # [1, 1, 12]: index 5 = sum (pred - truth)^2
        mse = float(mom[0, 0, 5]) / g4[0, 0].numel()
        hr, sr = groundtruth.detach().cpu().double().numpy(), pred.detach().cpu().double().numpy()
    else:
        hr, sr = np.asarray(groundtruth, dtype=np.float64), np.asarray(pred, dtype=np.float64)
        mse = float(((hr - sr) ** 2).mean())
    hr, sr = hr.reshape(hr.shape[-2:]), sr.reshape(sr.shape[-2:])
    rng = float(hr.max() - hr.min())
    psnr = float("inf") if mse == 0 else 10.0 * np.log10(rng * rng / mse)
    npx = win * win
    cov_norm = npx / (npx - 1.0)
    ux, uy = uniform_filter(hr, size=win), uniform_filter(sr, size=win)
    uxx, uyy, uxy = uniform_filter(hr * hr, size=win), uniform_filter(sr * sr, size=win), uniform_filter(hr * sr, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    smap = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    pad = (win - 1) // 2
    return psnr, float(smap[pad:-pad, pad:-pad].mean())


def stitched_scores(preds, y, out_variables, lat_weights=None):
    """PSNR and SSIM of a stitched prediction per output variable, on the device: `preds` [B,C,yout,xout] from tiled_predict,
    `y` the normalised target [B,C,>=yout,>=xout] (its top-left crop is scored), data range = max - min of every image's own
    target as the reference passes it to scikit-image (utils/visualize.py:366-372).  One pass of orbit2_ssim over the whole
    batch; only its [B,C,6] sums leave the device.  Returns {variable: {"psnr", "ssim"[, "lat_ssim"]}}, each the mean over the
    batch -- the per-channel entries of metrics.functional.psnr / ssim on the same tensors."""
    from .. import _hip
    from ..metrics import functional as fn
    preds = preds.detach().float().contiguous()
    s = _hip.ssim_sums(preds, y.detach().float().contiguous(), fn._lat(lat_weights, preds))
    cols = {"psnr": fn._psnr_per_image(s, preds).mean(0).float(), "ssim": fn._ssim_per_image(s, preds).mean(0).float().cpu()}
    if lat_weights is not None:
        cols["lat_ssim"] = fn._ssim_per_image(s, preds, lat_weights).mean(0).float().cpu()
    return {v: {k: float(col[c]) for k, col in cols.items()} for c, v in enumerate(out_variables)}


def baseline_scores(x, y, in_variables, out_variables, pred, mode="bilinear", lat_weights=None, denorm=None, rescale=None):
    """A prediction read against the interpolation baseline of its own input: {variable: {"rmse", "rmse_baseline", "mse_skill"}}
    (plus "lat_rmse", "lat_rmse_baseline", "lat_mse_skill" when `lat_weights` is given), rmse as metrics.functional.rmse forms
    it per channel and mse_skill = 1 - MSE(pred) / MSE(baseline) (metrics.functional.mse_skill).
    x [B,V,h,w] the normalised input, y [B,C,>=H,>=W] the normalised target (its top-left crop is scored), pred [B,C,H,W] the
    normalised prediction (e.g. from tiled_predict); the baseline is x's channels named by `out_variables`, resampled to
    (H, W) in `mode`.  It is never stored: a models.hub.Resampled is scored in the pass that resamples it.  `rescale` =
    (scale, shift) per output variable takes the baseline from the inputs' normalisation to the outputs' (utils.loaders builds
    it from the data module); `denorm`, a transforms.Denormalize, moves all three fields to physical units, for the baseline
    folded into the same pass (Resampled.affine).
    Constant output channels (CONSTANTS) are the target's own in the prediction and in the baseline, as clip_replace_constant
    leaves them: both errors are 0 and the skill, 0 / 0, is reported as NaN."""
    from ..data.processing.era5_constants import CONSTANTS
    from ..metrics import functional as fn
    from ..models.hub.interpolation import Interpolation
    scale, shift = rescale if rescale is not None else (None, None)
    pred = pred.detach().float().contiguous()
    H, W = pred.shape[2:]
    base = Interpolation(size=(H, W), mode=mode, scale=scale, shift=shift).lazy(x, in_variables, out_variables)
    y = y.detach().float()
    if denorm is not None:
        pred, y, base = denorm(pred), denorm(y[:, :, :H, :W]), base.affine(denorm.std, denorm.mean)
    const = torch.tensor([v in CONSTANTS for v in out_variables])

    def columns(w, prefix):
        sp, sb = fn._moments(pred, y, w)[0][..., 5].cpu(), fn._moments(base, y, w)[0][..., 5].cpu()    # [B,C] sums of w err^2
        sp, sb = sp.masked_fill(const, 0.0), sb.masked_fill(const, 0.0)
        skill = (1.0 - sp.sum(0) / sb.sum(0)).masked_fill(const, float("nan"))
        return {prefix + "rmse": (sp / (H * W)).sqrt().mean(0), prefix + "rmse_baseline": (sb / (H * W)).sqrt().mean(0),
                prefix + "mse_skill": skill}

    cols = columns(None, "")
    if lat_weights is not None:
        cols.update(columns(lat_weights, "lat_"))
    return {v: {k: float(col[c]) for k, col in cols.items()} for c, v in enumerate(out_variables)}


def consistency_scores(x, pred, in_variables, out_variables, mode="bilinear", lat_weights=None, rescale=None):
    """A prediction read against its own input: {variable: {"consistency_rmse", "consistency_bias"}} (plus
    "lat_consistency_rmse" when `lat_weights`, those of the LOW-resolution rows, is given).  A downscaled field that is sharp
    but does not average back to the field the model was given is wrong in a way no score against the target shows.
    x [B,V,h,w] the normalised input, pred [B,C,H,W] the normalised prediction (e.g. from tiled_predict).  With s = H // h the
    prediction is coarsened to (H // s, W // s) in `mode` (bilinear or bicubic) WITH antialiasing and scored against x's
    channels named by `out_variables`, through their top-left crop where the prediction covers less than x.  Those channels are
    gathered here (the tensor is low-resolution); `rescale` = (scale, shift) per output variable moves them from the inputs'
    normalisation to the outputs', as utils.loaders builds it for the baseline.  The coarsened field is never stored: a
    models.hub.Resampled is scored in the pass that resamples it (one pass, a second one for the latitude-weighted column).
    consistency_rmse is the root mean squared difference per image, averaged over the batch (metrics.functional.rmse);
    consistency_bias is mean(coarsened - input).  Constant output channels (CONSTANTS) are reported as baseline_scores
    reports them: both 0."""
    from ..data.processing.era5_constants import CONSTANTS
    from ..metrics import functional as fn
    from ..models.hub.interpolation import Resampled
    pred = pred.detach().float().contiguous()
    B, C, H, W = pred.shape
    s = H // x.shape[2]
    if s < 1 or H // s > x.shape[2] or W // s > x.shape[3]:
        raise ValueError("consistency_scores: a prediction of %s does not coarsen onto an input of %s"
                         % (tuple(pred.shape), tuple(x.shape)))
    in_variables = list(in_variables)
    if any(v not in in_variables for v in out_variables):
        raise RuntimeError("consistency_scores requires the output variables to be among the input variables.")
    given = x.detach().float()[:, [in_variables.index(v) for v in out_variables]]
    if rescale is not None and rescale[0] is not None:
        scale, shift = (torch.as_tensor(v, dtype=torch.float32, device=given.device).view(1, -1, 1, 1) for v in rescale)
        given = given * scale + shift
    given = given.contiguous()
    coarse = Resampled(pred, (H // s, W // s), mode, antialias=True)
    n = coarse.shape[2] * coarse.shape[3]
    const = torch.tensor([v in CONSTANTS for v in out_variables])
    m = coarse.moments(given, None).cpu()                                                   # [B,C,12] float64
    cols = {"consistency_rmse": (m[..., 5] / n).sqrt().mean(0).masked_fill(const, 0.0),
            "consistency_bias": ((m[..., 0] - m[..., 1]).sum(0) / (B * n)).masked_fill(const, 0.0)}
    if lat_weights is not None:
        m = coarse.moments(given, fn._lat(lat_weights, coarse)).cpu()
        cols["lat_consistency_rmse"] = (m[..., 5] / n).sqrt().mean(0).masked_fill(const, 0.0)
    return {v: {k: float(col[c]) for k, col in cols.items()} for c, v in enumerate(out_variables)}


def extreme_scores(preds, y, out_variables, levels=None, lat_weights=None):
    """What a stitched prediction does in its tails, per output variable: {variable: {"upper": [...], "lower": [...]}}, one entry
    per level q of `levels` (default metrics.functional.SIGMA_LEVELS, at most 8) -- "upper" at q, "lower" at the mirrored 1 - q --
    each {"level", "target_quantile", "pred_quantile", "quantile_bias", "tail_rmse", "tail_bias", "csi", "frequency_bias"}.
    `preds` [B,C,yout,xout] from tiled_predict, `y` the target [B,C,>=yout,>=xout] (its top-left crop; NaN = no data).  The
    quantiles are exact and pooled over the batch per variable (orbit2_masked_loss_fwd at ORBIT2_MASKED_QUANTILES); the tail is
    the pixels whose TARGET is at or beyond its own quantile (upper: >=, lower: <=), scored in one pass for all levels
    (ORBIT2_MASKED_TAIL): tail_rmse = sqrt(sum w d^2 / sum w) with w the latitude weight if given, tail_bias = mean(pred - target),
    csi = hits / (hits + misses + false alarms), frequency_bias = (hits + false alarms) / (hits + misses).  Everything stays on the
    device until the few numbers are read out."""
    from .. import _hip
    from ..metrics import functional as fn
    levels = tuple(float(q) for q in (fn.SIGMA_LEVELS if levels is None else levels))
    preds = preds.detach().float().contiguous()
    y = y.detach().float().contiguous()
    lat = fn._lat(lat_weights, preds)
    res = {v: {} for v in out_variables}
    for side, qs, lower in (("upper", levels, False), ("lower", tuple(1.0 - q for q in levels), True)):
        quant, _ = _hip.masked_quantiles(preds, y, torch.tensor(qs, dtype=torch.float32, device=preds.device))
        s, n = _hip.masked_tail(preds, y, quant[0, :, :, 0].contiguous(), lat, lower=lower)
        s, n, quant = s.double().sum(0).cpu(), n.sum(0).double().cpu(), quant[..., 0].double().cpu()        # [C,L,4] x 2, [2,C,L]
        hits, alarms = n[..., 1], n[..., 2]
        misses = n[..., 0] - hits
        cols = {"target_quantile": quant[0], "pred_quantile": quant[1], "quantile_bias": quant[1] - quant[0],
                "tail_rmse": (s[..., 1] / s[..., 0]).sqrt(), "tail_bias": s[..., 3] / n[..., 0],
                "csi": hits / (hits + misses + alarms), "frequency_bias": (hits + alarms) / (hits + misses)}
        for c, v in enumerate(out_variables):
            res[v][side] = [dict(level=q, **{k: float(col[c, j]) for k, col in cols.items()}) for j, q in enumerate(qs)]
    return res


def neighbourhood_scores(preds, y, out_variables, levels=None, windows=(1, 3, 5, 9, 17, 33, 65)):
    """At which scale a stitched prediction places its events rightly, per output variable: {variable: [row per level q of
    `levels` (default metrics.functional.SIGMA_LEVELS, at most 8)]}, each row {"level", "threshold", "base_rate", "uniform",
    "skilful_window", "fss": {window: value}}.  The event is "at or beyond the variable's exact pooled target quantile at q"
    (`threshold`, orbit2_masked_loss_fwd at ORBIT2_MASKED_QUANTILES); "fss" is the fractions skill score in every window of
    `windows` (odd, 1 .. 255 pixels; ORBIT2_FSS_KIND, one call per window), "base_rate" the fraction of the valid pixels at which
    the target has the event, "uniform" = 0.5 + base_rate / 2 the score that counts as skilful, and "skilful_window" the smallest
    window that reaches it (0: none does).  `preds`, `y` as extreme_scores.  Only these few numbers leave the device."""
    from .. import _hip
    from ..metrics import functional as fn
    levels = tuple(float(q) for q in (fn.SIGMA_LEVELS if levels is None else levels))
    windows = tuple(int(w) for w in windows)
    preds = preds.detach().float().contiguous()
    y = y.detach().float().contiguous()
    quant, _ = _hip.masked_quantiles(preds, y, torch.tensor(levels, dtype=torch.float32, device=preds.device))
    thr = quant[0, :, :, 0].contiguous()
    prof = fn.fss_profile(preds, y, windows, thresholds=thr)
    thr, prof = thr.double().cpu(), {k: v.double().cpu() for k, v in prof.items()}
    return {v: [dict(level=q, threshold=float(thr[c, j]), base_rate=float(prof["base_rate"][c, j]),
                     uniform=float(prof["uniform"][c, j]), skilful_window=int(prof["skilful_window"][c, j]),
                     fss={w: float(prof["fss"][c, j, k]) for k, w in enumerate(windows)})
                for j, q in enumerate(levels)] for c, v in enumerate(out_variables)}


def visualize_at_index(mm, dm, dm_vis, out_list, in_transform, out_transform, variable, src, device, div, overlap, index=0,
                       tensor_par_size=1, tensor_par_group=None, save_png: bool = True, prefix: str = ""):
    """Stitched input / prediction / ground truth of test sample `index` for `variable` (reference :38-490; the PNG
    dumps are optional here).  Returns {'inputs', 'preds', 'groundtruths'} as numpy arrays, north-up for
    ERA5 / PRISM / DAYMET sources like the reference's per-tile flips."""
    out_channel = dm.out_vars.index(variable)
    in_channel = dm.in_vars.index(variable)
    counter, adj_index, batch = 0, None, None
    for batch in dm_vis.test_dataloader():
        bs = batch[0].shape[0]
        if index in range(counter, counter + bs):
            adj_index = index - counter
            break
        counter += bs
    if adj_index is None:
        raise IndexError("test sample %d not found" % index)
    x, y, in_variables, out_variables = batch[:4]
    x, y = x.to(device), y.to(device)
    preds = tiled_predict(mm, x, y, in_variables, out_variables, div, overlap)
    yout, xout = preds.shape[2:]
    inp = in_transform(x[adj_index, in_channel].repeat(len(out_list), 1, 1))[out_channel]
    prd = out_transform(preds[adj_index])[out_channel]
    gt = out_transform(y[adj_index, :, :yout, :xout])[out_channel]
    res = {"inputs": inp.detach().cpu().numpy(), "preds": prd.detach().cpu().numpy(),
           "groundtruths": gt.detach().cpu().numpy()}
    if "ERA5" in src or src == "PRISM" or "DAYMET" in src:
        res = {k: np.flip(v, 0).copy() for k, v in res.items()}
    # evaluation metric of the stitched field (reference :360-372, printed the same way)
    res["psnr"], res["ssim"] = psnr_ssim(gt, prd)
    print("Goodness of fit: PSNR %s , SSIM %s" % (res["psnr"], res["ssim"]), flush=True)
    if save_png:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
            for name, key in (("input", "inputs"), ("prediction", "preds"), ("groundtruth", "groundtruths")):
                img = res[key]
                plt.figure(figsize=(max(img.shape[1] / 100, 2), max(img.shape[0] / 100, 1)))
                plt.imshow(img, cmap="coolwarm", vmin=float(img.min()), vmax=float(img.max()))
                plt.savefig("%s%d_%s.png" % (prefix, rank, name))
                plt.close()
        except ImportError:
            pass
    return res
