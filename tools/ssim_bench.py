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
not the halo re-reads and not the range pass's second read of the target.  This is a tool beside bench.py, not part of it."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default="16,3,512,1024")
    ap.add_argument("--host-images", type=int, default=48)
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.shape.split(","))
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
