#!/usr/bin/env python3
"""Cost of the device SSIM / PSNR: `orbit2_ssim` against a device-to-device copy and the host `psnr_ssim`.

    python tools/ssim_bench.py [--md profiles/ssim.md] [--rounds 5] [--shape 16,3,512,1024] [--host-images 48]

On a [16, 3, 512, 1024] prediction and target (fields in kelvin: smooth, 280 + noise), in one process on one card, the device
legs alternating `--rounds` times after a warm-up of each:
  sums   `_hip.ssim_sums(pred, target, lat_w)`: the range pass reads the target, the SSIM pass reads both fields (each pixel once
         per tile that covers it) and writes 6 doubles per image;
  map    the same with ssim_map=True: one [B,C,H-6,W-6] field written as well;
  copy   `copy_` of one field: two fields' bytes moved, one read and one written;
  host   `utils.visualize.psnr_ssim` looped over the images on CPU copies of the same fields (wall clock, once).
HIP events around the device legs.  GB/s is each leg's time over the bytes it MUST move: two fields read (plus the map written),
not the halo re-reads and not the range pass's second read of the target.  This is a tool beside bench.py, not part of it.

    python tools/ssim_bench.py --backward [--md profiles/ssim_loss.md] [--no-step]

The backward of those sums, the hot path of the SSIM training loss, on the same fields, legs alternating:
  vjp    `_hip.ssim_vjp(pred, target, lat_w, coef, range)`: orbit2_loss_bwd at kind 3, two fields read and one written;
  fwd    `_hip.ssim_sums` at the same given range (the loss's forward);
  copy   `copy_` of one field;
  aten   the autograd backward alone (the graph retained) of an SSIM built from ATen calls -- five depthwise `conv2d` with a
         7 x 7 box, fields centred per image -- on the same card, and `aten fwd` its forward.
Then a whole interm_8m training step (configs/interm_8m_ssim.yaml: batch 32, 32 x 64 -> 128 x 256; training_step + scaled backward
+ AdamW, first eager and then with the forward + backward replayed from a hipGraph) with bayesian_tv and with bayesian_tv_ssim,
alternating, wall clock.  ORBIT2_HIP_LIB
names another build of the library (one compiled with -DORBIT2_SSIM_VJP_TILE_H=32, to compare the two tile heights)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]


def _ev(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(shape, rounds, host_images):
    import torch
    from climate_learn import _hip
    from climate_learn.utils.visualize import psnr_ssim
    B, C, H, W = shape
    field = B * C * H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    yy = torch.arange(H, device="cuda").view(1, 1, H, 1) / 37.0
    xx = torch.arange(W, device="cuda").view(1, 1, 1, W) / 53.0
    phase = torch.rand(B, C, 1, 1, device="cuda", generator=g) * 6.28
    target = 280.0 + 2.0 * torch.sin(yy + phase) + 1.5 * torch.cos(xx - phase) + 0.1 * torch.randn(shape, device="cuda", generator=g)
    pred = target + 0.3 * torch.randn(shape, device="cuda", generator=g)
    lat_w = torch.rand(H, device="cuda", generator=g) + 0.5
    src = torch.randn(field, device="cuda", generator=g)
    dst = torch.empty_like(src)
    map_bytes = B * C * (H - 6) * (W - 6) * 4
    legs = {"sums": (lambda: _hip.ssim_sums(pred, target, lat_w), 20, 2 * field * 4),
            "map": (lambda: _hip.ssim_sums(pred, target, lat_w, ssim_map=True), 20, 2 * field * 4 + map_bytes),
            "copy": (lambda: dst.copy_(src), 20, 2 * field * 4)}
    for fn, _, _ in legs.values():                      # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, reps, _) in legs.items():
            ms[k].append(_ev(fn, reps))
    sums = _hip.ssim_sums(pred, target, lat_w).cpu()
    res = {"shape": list(shape), "rounds": rounds}
    for k, (_, _, nbytes) in legs.items():
        mean = sum(ms[k]) / rounds
        res[k] = {"ms": round(mean, 4), "spread": round((max(ms[k]) - min(ms[k])) / mean, 4), "GBps": round(nbytes / (1e6 * mean), 1)}
    res["sums_over_copy"] = round(res["sums"]["GBps"] / res["copy"]["GBps"], 3)
    res["map_over_copy"] = round(res["map"]["GBps"] / res["copy"]["GBps"], 3)
    # the host path on the same fields: its cost per image, scaled to the batch when fewer images are looped
    n = min(host_images, B * C)
    hp, ht = pred.reshape(B * C, H, W)[:n].cpu(), target.reshape(B * C, H, W)[:n].cpu()
    t0 = time.perf_counter()
    host = [psnr_ssim(ht[i].numpy(), hp[i].numpy()) for i in range(n)]
    dt = time.perf_counter() - t0
    dev_ssim = (sums[..., 0] / ((H - 6) * (W - 6))).reshape(-1)[:n]
    mse = (sums[..., 2] / (H * W)).reshape(-1)[:n]
    dev_psnr = 10 * torch.log10(sums[..., 5].reshape(-1)[:n] ** 2 / mse)
    res["host"] = {"images": n, "ms_per_image": round(1e3 * dt / n, 2), "ms_for_the_batch": round(1e3 * dt / n * B * C, 1)}
    res["max_abs_diff_ssim_vs_host"] = float(max(abs(float(dev_ssim[i]) - host[i][1]) for i in range(n)))
    res["max_abs_diff_psnr_db_vs_host"] = float(max(abs(float(dev_psnr[i]) - host[i][0]) for i in range(n)))
    return res


def _fields(shape):
    import torch
    B, C, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(0)
    yy = torch.arange(H, device="cuda").view(1, 1, H, 1) / 37.0
    xx = torch.arange(W, device="cuda").view(1, 1, 1, W) / 53.0
    phase = torch.rand(B, C, 1, 1, device="cuda", generator=g) * 6.28
    target = 280.0 + 2.0 * torch.sin(yy + phase) + 1.5 * torch.cos(xx - phase) + 0.1 * torch.randn(shape, device="cuda", generator=g)
    pred = target + 0.3 * torch.randn(shape, device="cuda", generator=g)
    return pred, target, torch.rand(H, device="cuda", generator=g) + 0.5, g


def _aten_ssim_sum(pred, target, lat_w, rng):
    """sum over images and valid centres of lat_w S, from ATen calls alone: the fields centred on each image's target mean, five
    depthwise 7 x 7 box convolutions"""
    import torch
    import torch.nn.functional as Fn
    B, C, H, W = pred.shape
    c = target.mean((2, 3), keepdim=True)
    a, b = (pred - c).reshape(1, B * C, H, W), (target - c).reshape(1, B * C, H, W)
    k = torch.full((B * C, 1, 7, 7), 1.0 / 49, device=pred.device)
    box = lambda t: Fn.conv2d(t, k, groups=B * C)
    ma, mb = box(a), box(b)
    va, vb, vab = (box(a * a) - ma * ma) * (49 / 48), (box(b * b) - mb * mb) * (49 / 48), (box(a * b) - ma * mb) * (49 / 48)
    ux, uy = ma + c.reshape(1, B * C, 1, 1), mb + c.reshape(1, B * C, 1, 1)
    r = rng.reshape(1, B * C, 1, 1)
    c1, c2 = (0.01 * r) ** 2, (0.03 * r) ** 2
    S = (2 * ux * uy + c1) * (2 * vab + c2) / ((ux * ux + uy * uy + c1) * (va + vb + c2))
    return (S * lat_w[3:H - 3].view(1, 1, -1, 1)).sum()


def run_backward(shape, rounds, reps=20):
    import torch
    from climate_learn import _hip
    B, C, H, W = shape
    field = B * C * H * W
    pred, target, lat_w, g = _fields(shape)
    coef = torch.rand(B, C, device="cuda", generator=g) + 0.5
    rng = torch.full((B, C), 7.0, device="cuda")
    src = torch.randn(field, device="cuda", generator=g)
    dst = torch.empty_like(src)
    leaf = pred.clone().requires_grad_(True)
    aten_out = _aten_ssim_sum(leaf, target, lat_w, rng)
    legs = {"vjp": (lambda: _hip.ssim_vjp(pred, target, lat_w, coef, rng), reps, 3 * field * 4),
            "fwd": (lambda: _hip.ssim_sums(pred, target, lat_w, rng), reps, 2 * field * 4),
            "copy": (lambda: dst.copy_(src), reps, 2 * field * 4),
            "aten": (lambda: torch.autograd.grad(aten_out, leaf, retain_graph=True), 5, 3 * field * 4),
            "aten fwd": (lambda: _aten_ssim_sum(pred, target, lat_w, rng), 5, 2 * field * 4)}
    for fn, _, _ in legs.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, n, _) in legs.items():
            ms[k].append(_ev(fn, n))
    res = {"shape": list(shape), "rounds": rounds, "lib": os.path.basename(_hip.LIB_PATH)}
    for k, (_, _, nbytes) in legs.items():
        mean = sum(ms[k]) / rounds
        res[k] = {"ms": round(mean, 4), "spread": round((max(ms[k]) - min(ms[k])) / mean, 4), "GBps": round(nbytes / (1e6 * mean), 1)}
    # agreement: ours against the ATen gradient with coef = 1 (fp32 both; ATen's variances cancel at 280 K less well than ours)
    ones = torch.ones(B, C, device="cuda")
    ours = _hip.ssim_vjp(pred, target, lat_w, ones, rng)
    (aten,) = torch.autograd.grad(aten_out, leaf, retain_graph=True)
    res["max_rel_diff_vs_aten"] = float((ours - aten).abs().max() / aten.abs().max())
    return res


def run_step(rounds, steps=10):
    """ms per interm_8m training step with bayesian_tv and with bayesian_tv_ssim, eager and graphed, alternating"""
    import torch
    import torch.nn as nn
    import yaml
    import climate_learn as cl
    from climate_learn.metrics.utils import MetricsMetaInfo
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.models.hub.components.vit_blocks import Block
    from climate_learn.trainer import training_step
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m_ssim.yaml")))
    mc, dc, tr = conf["model"], conf["data"], conf["trainer"]
    in_vars, out_vars = dc["dict_in_variables"]["ERA5_1"], dc["dict_out_variables"]["ERA5_1"]
    (h, w), B = dc["synthetic"]["ERA5_1"]["lowres_hw"], tr["batch_size"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cl.manual_seed(0, 0)
    with torch.device(dev):
        model = Res_Slim_ViT(in_vars, (h, w), len(in_vars), len(out_vars), 1, superres_mag=mc["superres_mag"],
                             cnn_ratio=mc["cnn_ratio"], patch_size=mc["patch_size"], drop_path=mc["drop_path"],
                             drop_rate=mc["drop_rate"], learn_pos_emb=True, embed_dim=mc["embed_dim"], depth=mc["depth"],
                             decoder_depth=mc["decoder_depth"], num_heads=mc["num_heads"], mlp_ratio=mc["mlp_ratio"])
    model.data_config(156.0, (h, w), len(in_vars), len(out_vars))
    eng = cl.HipDataParallel(model, unit_types=(Block, nn.Sequential))
    opt = cl.load_optimizer(eng, "adamw", {"lr": 5e-4, "betas": (0.9, 0.99), "weight_decay": 1e-5})
    scaler = cl.HipGradScaler(init_scale=8192.0, growth_interval=1 << 30, min_scale=128.0)
    meta = MetricsMetaInfo(in_vars, out_vars, None, None, None)
    losses = {k: cl.load_loss(dev, None, k, True, meta) for k in ("bayesian_tv", tr["train_loss"])}
    eng.train()
    g = torch.Generator().manual_seed(1000)
    x = torch.randn(B, len(in_vars), h, w, generator=g)
    y = torch.randn(B, len(out_vars), 4 * h, 4 * w, generator=g)
    batch = (x.to(dev), y.to(dev), in_vars, out_vars)
    vw = dc.get("var_weights", {})

    def eager(loss_fn):
        loss = training_step(batch, 0, eng, dev, vw, loss_fn)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    legs = {"eager " + k: (lambda f=f: eager(f)) for k, f in losses.items()}
    for fn in legs.values():
        for _ in range(3):
            fn()
    for k, f in losses.items():
        gs = cl.GraphedTrainStep(eng, f, batch, vw, scaler=scaler)

        def graphed(gs=gs):
            gs()
            scaler.step(opt)
            scaler.update()

        legs["graphed " + k] = graphed
        for _ in range(3):
            graphed()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
    return {k: {"ms": round(sum(v) / rounds, 4), "min": round(min(v), 4), "max": round(max(v), 4),
                "spread": round((max(v) - min(v)) / (sum(v) / rounds), 4)} for k, v in ms.items()}


def write_backward_md(r, path):
    with open(path, "a") as f:
        f.write("\n## %s, [%s]\n\n" % (r["lib"], ", ".join(map(str, r["shape"]))))
        f.write("| leg | ms per call (spread over %d rounds) | GB/s of the bytes it must move | time over the copy's |\n|---|---|---|---|\n" % r["rounds"])
        for k in ("vjp", "fwd", "copy", "aten", "aten fwd"):
            f.write("| %s | %.4f (%.1f %%) | %.1f | %.2f |\n" % (k, r[k]["ms"], 100 * r[k]["spread"], r[k]["GBps"], r[k]["ms"] / r["copy"]["ms"]))
        f.write("\nOurs against ATen's gradient, fp32 both: %.1e of max|d|.\n" % r["max_rel_diff_vs_aten"])
        if "step" in r:
            f.write("\nAn eager interm_8m training step, wall clock over %d steps per round:\n\n| leg | ms per step (min .. max) |\n|---|---|\n" % r["step_steps"])
            for k, v in r["step"].items():
                f.write("| %s | %.3f (%.3f .. %.3f) |\n" % (k, v["ms"], v["min"], v["max"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backward", action="store_true", help="the SSIM vector-Jacobian kernel and the training step")
    ap.add_argument("--no-step", action="store_true", help="--backward without the training-step legs")
    ap.add_argument("--md")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default="16,3,512,1024")
    ap.add_argument("--host-images", type=int, default=48)
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.shape.split(","))
    if a.backward:
        r = run_backward(shape, a.rounds)
        if not a.no_step:
            r["step"], r["step_steps"] = run_step(a.rounds), 10
        print(json.dumps(r), flush=True)
        if a.md:
            write_backward_md(r, a.md)
        return
    r = run(shape, a.rounds, a.host_images)
    print(json.dumps(r), flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Device SSIM / PSNR: the kernel against a copy and the host path (tools/ssim_bench.py)\n\n")
            f.write("One MI355X, one process, device legs alternating, %d rounds of 20 calls after a warm-up, HIP events; prediction "
                    "and target [%s] fp32, kelvin-like (280 + smooth + noise).\n`sums` = `_hip.ssim_sums` (range pass + SSIM pass, "
                    "6 doubles per image out); `map` = the same with the [B,C,H-6,W-6] map written; `copy` = `copy_` of one field "
                    "(two fields' bytes moved); `host` = `psnr_ssim` looped over %d images on the CPU (wall clock, once).  GB/s "
                    "counts the bytes a leg must move: two fields read (plus the map), not the 1.3 x halo re-reads nor the range "
                    "pass's second read of the target.\n\n"
                    % (r["rounds"], ", ".join(map(str, r["shape"])), r["host"]["images"]))
            f.write("| leg | ms per call (spread) | GB/s of the bytes it must move | rate over the copy's |\n|---|---|---|---|\n")
            f.write("| sums | %.4f (%.1f %%) | %.1f | %.3f |\n" % (r["sums"]["ms"], 100 * r["sums"]["spread"], r["sums"]["GBps"], r["sums_over_copy"]))
            f.write("| map | %.4f (%.1f %%) | %.1f | %.3f |\n" % (r["map"]["ms"], 100 * r["map"]["spread"], r["map"]["GBps"], r["map_over_copy"]))
            f.write("| copy | %.4f (%.1f %%) | %.1f | 1 |\n" % (r["copy"]["ms"], 100 * r["copy"]["spread"], r["copy"]["GBps"]))
            f.write("| host | %.1f for the batch (%.2f per image, %d looped) | | |\n\n"
                    % (r["host"]["ms_for_the_batch"], r["host"]["ms_per_image"], r["host"]["images"]))
            f.write("Agreement with the host path over the looped images: SSIM within %.1e, PSNR within %.1e dB.\n"
                    % (r["max_abs_diff_ssim_vs_host"], r["max_abs_diff_psnr_db_vs_host"]))


if __name__ == "__main__":
    main()
