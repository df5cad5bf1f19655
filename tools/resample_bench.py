#!/usr/bin/env python3
"""Cost of the interpolation baselines: `orbit2_resample_fwd` / `orbit2_resample_moments` against ATen and plain streams.

    python tools/resample_bench.py [--md profiles/resample.md] [--rounds 5] [--x 16,23,128,256] [--size 512,1024]

x [16, 23, 128, 256] -> [16, 3, 512, 1024], the interm_1b pair with the three output variables picked from the 23 inputs by name
(channels 21, 6, 5), in one process on one card, all legs alternating `--rounds` times after a warm-up of each; HIP events.
fwd legs, per mode (nearest, bilinear, bicubic):
  ours      `_hip.resample(x, size, mode, channels)` into a resident output;
  aten      `F.interpolate(x[:, channels], size, mode=mode)` (its gather of the three channels included: 6 MB);
  copy      `copy_` of one output field (a field read and a field written);
  fill      `fill_` of one output field (a field written: what a store-bound kernel can at best do).
moments legs, per mode:
  fused     `_hip.resample_moments(x, size, mode, target, channels, lat_w=lat_w)`: the field is never stored;
  two-step  `_hip.resample` into a resident field, then `_hip.eval_moments` on it;
  aten+     `F.interpolate`, then `_hip.eval_moments`;
  moments   `_hip.eval_moments` alone on a resident field (what reading two fields costs).
GB/s is each leg's time over the bytes it MUST move: the three source channels read plus the field written (ours, aten), plus
the target read (fused), plus the field written, read back and the target read (two-step, aten+).  A tool beside bench.py, not
part of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]
CHANNELS = (21, 6, 5)           # total_precipitation_24hr, 2m_temperature_min, 2m_temperature_max among interm_1b's 23 inputs
MODES = ("nearest", "bilinear", "bicubic")


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


def run(xshape, size, rounds, reps=20):
    import torch
    import torch.nn.functional as F
    from climate_learn import _hip
    B, V, h, w = xshape
    H, W = size
    C = len(CHANNELS)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(xshape, device="cuda", generator=g)
    target = torch.randn(B, C, H, W, device="cuda", generator=g)
    lat_w = torch.rand(H, device="cuda", generator=g) + 0.5
    out = torch.empty(B, C, H, W, device="cuda")
    other = torch.randn(B, C, H, W, device="cuda", generator=g)
    idx = torch.tensor(CHANNELS, device="cuda")
    field, src = B * C * H * W * 4, B * C * h * w * 4
    legs = {}
    for m in MODES:
        legs["ours " + m] = (lambda m=m: _hip.resample(x, size, m, CHANNELS, out=out), src + field)
        legs["aten " + m] = (lambda m=m: F.interpolate(x[:, idx], size, mode=m), src + field)
    legs["copy"] = (lambda: out.copy_(other), 2 * field)
    legs["fill"] = (lambda: out.fill_(1.0), field)
    for m in MODES:
        legs["fused " + m] = (lambda m=m: _hip.resample_moments(x, size, m, target, CHANNELS, lat_w=lat_w), src + field)
        legs["two-step " + m] = (lambda m=m: _hip.eval_moments(_hip.resample(x, size, m, CHANNELS, out=out), target, lat_w),
                                 src + 3 * field)
        legs["aten+ " + m] = (lambda m=m: _hip.eval_moments(F.interpolate(x[:, idx], size, mode=m), target, lat_w),
                              src + 3 * field)
    legs["moments"] = (lambda: _hip.eval_moments(other, target, lat_w), 2 * field)
    for fn, _ in legs.values():                          # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, _) in legs.items():
            ms[k].append(_ev(fn, reps))
    res = {"x": list(xshape), "size": list(size), "rounds": rounds, "reps": reps, "legs": {}}
    for k, (_, nbytes) in legs.items():
        mean = sum(ms[k]) / rounds
        res["legs"][k] = {"ms": round(mean, 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4),
                          "spread": round((max(ms[k]) - min(ms[k])) / mean, 4), "GBps": round(nbytes / (1e6 * mean), 1)}
    # agreement of the two routes to the sums and of ours with ATen, at this shape
    res["agreement"] = {}
    for m in MODES:
        a = _hip.resample(x, size, m, CHANNELS)
        b = F.interpolate(x[:, idx], size, mode=m)
        s1 = _hip.resample_moments(x, size, m, target, CHANNELS, lat_w=lat_w)
        s2 = _hip.eval_moments(a, target, lat_w)
        res["agreement"][m] = {"max_abs_vs_aten": float((a - b).abs().max()),
                               "sums_rel_vs_two_step": float(((s1 - s2).abs() / s2.abs().clamp_min(1e-30))[..., 5].max())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--x", default="16,23,128,256")
    ap.add_argument("--size", default="512,1024")
    a = ap.parse_args()
    r = run(tuple(int(v) for v in a.x.split(",")), tuple(int(v) for v in a.size.split(",")), a.rounds)
    print(json.dumps(r), flush=True)
    if a.md:
        L = r["legs"]
        with open(a.md, "w") as f:
            f.write("# Interpolation baselines: the resample kernels against ATen and plain streams (tools/resample_bench.py)\n\n")
            f.write("One MI355X, one process, all legs alternating, %d rounds of %d calls after a warm-up, HIP events; x [%s] fp32 -> "
                    "[%d, 3, %s], channels %s picked by name.\nGB/s counts the bytes a leg must move (the tool's docstring); the "
                    "spread is (max - min) / mean over the rounds.\n\n"
                    % (r["rounds"], r["reps"], ", ".join(map(str, r["x"])), r["x"][0], ", ".join(map(str, r["size"])),
                       list(CHANNELS)))
            f.write("| leg | ms per call (min .. max, spread) | GB/s of the bytes it must move |\n|---|---|---|\n")
            for k, v in L.items():
                f.write("| %s | %.4f (%.4f .. %.4f, %.1f %%) | %.1f |\n" % (k, v["ms"], v["min"], v["max"], 100 * v["spread"], v["GBps"]))
            f.write("\n| mode | ours / aten | ours / fill | fused / two-step | fused / aten+ | max abs ours - aten | sum 5 fused vs two-step, rel |\n"
                    "|---|---|---|---|---|---|---|\n")
            for m in MODES:
                ag = r["agreement"][m]
                f.write("| %s | %.3f | %.3f | %.3f | %.3f | %.3g | %.3g |\n"
                        % (m, L["ours " + m]["ms"] / L["aten " + m]["ms"], L["ours " + m]["ms"] / L["fill"]["ms"],
                           L["fused " + m]["ms"] / L["two-step " + m]["ms"], L["fused " + m]["ms"] / L["aten+ " + m]["ms"],
                           ag["max_abs_vs_aten"], ag["sums_rel_vs_two_step"]))


if __name__ == "__main__":
    main()
