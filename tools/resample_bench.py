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
the target read (fused), plus the field written, read back and the target read (two-step, aten+).

    python tools/resample_bench.py --antialias [--md profiles/resample_aa.md] [--rounds 5]

measures the antialiased modes instead (the coarsening of a consistency score): x [16, 3, 512, 1024] -> [16, 3, 128, 256] (4x)
and -> [16, 3, 64, 128] (8x), bilinear and bicubic, the same alternation and events.  Legs per size and mode: ours
(`_hip.resample(..., antialias=True)` into a resident output), aten (`F.interpolate(..., antialias=True)`), fused
(`_hip.resample_moments(..., antialias=True)`), two-step (ours, then `_hip.eval_moments`); and once, copy-src: `copy_` of the
source field (the source bytes read and written once: no resampling kernel reads them faster).  GB/s counts the source read plus
the field written (plus the target for fused, plus the field's second trip for two-step).  A tool beside bench.py, not part of
it.

    python tools/resample_bench.py --adjoint [--md profiles/resample_adjoint.md] [--rounds 5]

measures the adjoint of the antialiased coarsening (the backward of the consistency training loss): the gradient
g [16, 3, 128, 256] (4x) and [16, 3, 64, 128] (8x) -> d [16, 3, 512, 1024], bilinear and bicubic.  Legs per size and mode:
adjoint (`_hip.resample_adjoint`) and aten-bwd (the backward of `F.interpolate(..., antialias=True)` alone, by
`torch.autograd.grad` on a kept graph); and once, copy-fine: `copy_` of the fine field, the bandwidth floor of a kernel that
writes it.  GB/s counts g read plus d written.  Then a whole interm_8m training step (batch 32 on a 32 x 64 grid, 23 -> 3
variables, training_step + scaled backward + AdamW, first eager and then with the forward + backward replayed from a hipGraph
as the driver runs this preset) with `bayesian_tv` and with `bayesian_tv_consistency`, alternating on one engine."""
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


def measure(legs, rounds, reps):
    """legs: name -> (call, bytes it must move).  A warm-up of every leg, then all legs alternating `rounds` times; per leg the
    mean, min, max, spread and GB/s of its ms per call"""
    for fn, _ in legs.values():                          # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, _) in legs.items():
            ms[k].append(_ev(fn, reps))
    res = {}
    for k, (_, nbytes) in legs.items():
        mean = sum(ms[k]) / rounds
        res[k] = {"ms": round(mean, 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4),
                  "spread": round((max(ms[k]) - min(ms[k])) / mean, 4), "GBps": round(nbytes / (1e6 * mean), 1)}
    return res


def agreement(ours, aten, fused, two_step):
    """agreement of the two routes to the sums and of ours with ATen, at one shape"""
    return {"max_abs_vs_aten": float((ours - aten).abs().max()),
            "sums_rel_vs_two_step": float(((fused - two_step).abs() / two_step.abs().clamp_min(1e-30))[..., 5].max())}


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
    res = {"x": list(xshape), "size": list(size), "rounds": rounds, "reps": reps, "legs": measure(legs, rounds, reps),
           "agreement": {}}
    for m in MODES:
        a = _hip.resample(x, size, m, CHANNELS)
        res["agreement"][m] = agreement(a, F.interpolate(x[:, idx], size, mode=m),
                                        _hip.resample_moments(x, size, m, target, CHANNELS, lat_w=lat_w),
                                        _hip.eval_moments(a, target, lat_w))
    return res


AA_X, AA_SIZES, AA_MODES = (16, 3, 512, 1024), ((128, 256), (64, 128)), ("bilinear", "bicubic")


def run_antialias(rounds, reps=20):
    import torch
    import torch.nn.functional as F
    from climate_learn import _hip
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(AA_X, device="cuda", generator=g)
    other = torch.empty_like(x)
    B, C, h, w = AA_X
    src = x.numel() * 4
    legs, keep = {"copy-src": (lambda: other.copy_(x), 2 * src)}, []
    for H, W in AA_SIZES:
        out = torch.empty(B, C, H, W, device="cuda")
        target = torch.randn(B, C, H, W, device="cuda", generator=g)
        lat_w = torch.rand(H, device="cuda", generator=g) + 0.5
        keep.append((out, target, lat_w))
        field, tag = out.numel() * 4, "%dx%d" % (H, W)
        for m in AA_MODES:
            k = dict(size=(H, W), m=m, out=out, target=target, lat_w=lat_w)
            legs["ours %s %s" % (m, tag)] = (lambda k=k: _hip.resample(x, k["size"], k["m"], out=k["out"], antialias=True), src + field)
            legs["aten %s %s" % (m, tag)] = (lambda k=k: F.interpolate(x, k["size"], mode=k["m"], align_corners=False,
                                                                     antialias=True), src + field)
            legs["fused %s %s" % (m, tag)] = (lambda k=k: _hip.resample_moments(x, k["size"], k["m"], k["target"], lat_w=k["lat_w"],
                                                                            antialias=True), src + field)
            legs["two-step %s %s" % (m, tag)] = (lambda k=k: _hip.eval_moments(
                _hip.resample(x, k["size"], k["m"], out=k["out"], antialias=True), k["target"], k["lat_w"]), src + 3 * field)
    res = {"x": list(AA_X), "sizes": [list(v) for v in AA_SIZES], "rounds": rounds, "reps": reps,
           "legs": measure(legs, rounds, reps), "agreement": {}}
    for (H, W), (out, target, lat_w) in zip(AA_SIZES, keep):
        for m in AA_MODES:
            a = _hip.resample(x, (H, W), m, antialias=True)
            res["agreement"]["%s %dx%d" % (m, H, W)] = agreement(
                a, F.interpolate(x, (H, W), mode=m, align_corners=False, antialias=True),
                _hip.resample_moments(x, (H, W), m, target, lat_w=lat_w, antialias=True), _hip.eval_moments(a, target, lat_w))
    return res


def run_adjoint(rounds, reps=20):
    import torch
    import torch.nn.functional as F
    from climate_learn import _hip
    g0 = torch.Generator(device="cuda").manual_seed(0)
    B, C, H, W = AA_X
    fine = torch.randn(AA_X, device="cuda", generator=g0)
    other = torch.empty_like(fine)
    nfine = fine.numel() * 4
    legs, keep = {"copy-fine": (lambda: other.copy_(fine), 2 * nfine)}, []
    for h, w in AA_SIZES:
        g = torch.randn(B, C, h, w, device="cuda", generator=g0)
        tag = "%dx%d" % (h, w)
        for m in AA_MODES:
            leaf = fine.clone().requires_grad_()
            coarse = F.interpolate(leaf, (h, w), mode=m, align_corners=False, antialias=True)
            k = dict(g=g, m=m, leaf=leaf, coarse=coarse)
            keep.append(k)
            legs["adjoint %s %s" % (m, tag)] = (lambda k=k: _hip.resample_adjoint(k["g"], (H, W), k["m"]), g.numel() * 4 + nfine)
            legs["aten-bwd %s %s" % (m, tag)] = (lambda k=k: torch.autograd.grad(k["coarse"], k["leaf"], k["g"], retain_graph=True),
                                                 g.numel() * 4 + nfine)
    res = {"x": list(AA_X), "sizes": [list(v) for v in AA_SIZES], "rounds": rounds, "reps": reps,
           "legs": measure(legs, rounds, reps), "agreement": {}}
    for k in keep:
        d = _hip.resample_adjoint(k["g"], (H, W), k["m"])
        ref, = torch.autograd.grad(k["coarse"], k["leaf"], k["g"], retain_graph=True)
        res["agreement"]["%s %dx%d" % (k["m"], k["g"].shape[2], k["g"].shape[3])] = {
            "max_abs_vs_aten": float((d - ref).abs().max()), "repeat_equal": bool(torch.equal(d, _hip.resample_adjoint(k["g"], (H, W), k["m"])))}
    return res


def run_step(rounds, steps=10):
    """ms per interm_8m training step with bayesian_tv and with bayesian_tv_consistency, eager and graphed, alternating"""
    import time
    import torch
    import torch.nn as nn
    import yaml
    import climate_learn as cl
    from climate_learn.metrics.utils import MetricsMetaInfo
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.models.hub.components.vit_blocks import Block
    from climate_learn.trainer import training_step
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m_consistency.yaml")))
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
    scaler = cl.HipGradScaler(init_scale=8192.0, growth_interval=1 << 30, min_scale=128.0)      # a fixed scale: no re-capture
    meta = MetricsMetaInfo(in_vars, out_vars, None, None, None)
    losses = {"bayesian_tv": cl.load_loss(dev, None, "bayesian_tv", True, meta),
              "bayesian_tv_consistency": cl.load_loss(dev, None, "bayesian_tv_consistency", True, meta)}
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


def write_adjoint_md(r, path):
    L = r["legs"]
    with open(path, "w") as f:
        f.write("# The adjoint of the antialiased coarsening and the consistency loss's cost per step (tools/resample_bench.py "
                "--adjoint)\n\n")
        f.write("One MI355X, one process, all legs alternating, %d rounds of %d calls after a warm-up, HIP events; gradient g [%d, %d, "
                "h, w] fp32 -> d [%s] fp32.\nGB/s counts g read plus d written (copy-fine: the fine field read and written); the "
                "spread is (max - min) / mean over the rounds.\n\n"
                % (r["rounds"], r["reps"], r["x"][0], r["x"][1], ", ".join(map(str, r["x"]))))
        f.write("| leg | ms per call (min .. max, spread) | GB/s of the bytes it must move |\n|---|---|---|\n")
        for k, v in L.items():
            f.write("| %s | %.4f (%.4f .. %.4f, %.1f %%) | %.1f |\n" % (k, v["ms"], v["min"], v["max"], 100 * v["spread"], v["GBps"]))
        f.write("\n| mode and size | adjoint / copy-fine | adjoint / aten-bwd | max abs adjoint - aten | two calls equal |\n"
                "|---|---|---|---|---|\n")
        for k, ag in r["agreement"].items():
            f.write("| %s | %.3f | %.3f | %.3g | %s |\n" % (k, L["adjoint " + k]["ms"] / L["copy-fine"]["ms"],
                                                          L["adjoint " + k]["ms"] / L["aten-bwd " + k]["ms"], ag["max_abs_vs_aten"],
                                                          ag["repeat_equal"]))
        if "step" in r:
            S = r["step"]
            f.write("\nA whole interm_8m training step (batch 32, 32 x 64 -> 128 x 256, 23 -> 3 variables; training_step + scaled "
                    "backward + AdamW), wall clock over %d steps per round:\n\n| leg | ms per step (min .. max, spread) |\n|---|---|\n"
                    % r["step_steps"])
            for k, v in S.items():
                f.write("| %s | %.3f (%.3f .. %.3f, %.1f %%) |\n" % (k, v["ms"], v["min"], v["max"], 100 * v["spread"]))
            for how in ("eager", "graphed"):
                a, b = S[how + " bayesian_tv_consistency"]["ms"], S[how + " bayesian_tv"]["ms"]
                f.write("\n%s: the consistency term adds %.3f ms per step (%.1f %%)." % (how, a - b, 100 * (a - b) / b))
            f.write("\n")


# what the two tables differ in: the title, the name of the first column of the second table and its ratios (numerator leg,
# denominator leg; a name that ends in a blank is completed by the row's key)
PLAIN_MD = ("Interpolation baselines: the resample kernels against ATen and plain streams (tools/resample_bench.py)", "mode",
            (("ours ", "aten "), ("ours ", "fill"), ("fused ", "two-step "), ("fused ", "aten+ ")))
AA_MD = ("Antialiased resampling: the antialiased kernel against ATen and a copy of the source (tools/resample_bench.py "
         "--antialias)", "mode and size", (("ours ", "aten "), ("ours ", "copy-src"), ("fused ", "two-step ")))


def write_md(r, path, shapes, title, first, ratios):
    """shapes: the run's `x [...] fp32 -> ...` sentence"""
    L = r["legs"]
    leg = lambda name, k: L[name + k if name.endswith(" ") else name]["ms"]
    with open(path, "w") as f:
        f.write("# %s\n\n" % title)
        f.write("One MI355X, one process, all legs alternating, %d rounds of %d calls after a warm-up, HIP events; %s\nGB/s counts "
                "the bytes a leg must move (the tool's docstring); the spread is (max - min) / mean over the rounds.\n\n"
                % (r["rounds"], r["reps"], shapes))
        f.write("| leg | ms per call (min .. max, spread) | GB/s of the bytes it must move |\n|---|---|---|\n")
        for k, v in L.items():
            f.write("| %s | %.4f (%.4f .. %.4f, %.1f %%) | %.1f |\n" % (k, v["ms"], v["min"], v["max"], 100 * v["spread"], v["GBps"]))
        cols = [first] + ["%s/ %s" % (n, d.strip()) for n, d in ratios] + ["max abs ours - aten", "sum 5 fused vs two-step, rel"]
        f.write("\n| %s |\n%s|\n" % (" | ".join(cols), "|---" * len(cols)))
        for k, ag in r["agreement"].items():
            f.write("| %s | %s | %.3g | %.3g |\n" % (k, " | ".join("%.3f" % (leg(n, k) / leg(d, k)) for n, d in ratios),
                                                    ag["max_abs_vs_aten"], ag["sums_rel_vs_two_step"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--antialias", action="store_true")
    ap.add_argument("--adjoint", action="store_true")
    ap.add_argument("--no-step", action="store_true", help="--adjoint without the training-step legs")
    ap.add_argument("--md")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--x", default="16,23,128,256")
    ap.add_argument("--size", default="512,1024")
    a = ap.parse_args()
    if a.adjoint:
        r = run_adjoint(a.rounds)
        if not a.no_step:
            r["step"], r["step_steps"] = run_step(a.rounds), 10
        print(json.dumps(r), flush=True)
        if a.md:
            write_adjoint_md(r, a.md)
        return
    if a.antialias:
        r = run_antialias(a.rounds)
        shapes = "x [%s] fp32 -> %s." % (", ".join(map(str, r["x"])),
                                         " and ".join("[%d, %d, %d, %d]" % (r["x"][0], r["x"][1], H, W) for H, W in r["sizes"]))
    else:
        r = run(tuple(int(v) for v in a.x.split(",")), tuple(int(v) for v in a.size.split(",")), a.rounds)
        shapes = "x [%s] fp32 -> [%d, 3, %s], channels %s picked by name." % (", ".join(map(str, r["x"])), r["x"][0],
                                                                             ", ".join(map(str, r["size"])), list(CHANNELS))
    print(json.dumps(r), flush=True)
    if a.md:
        write_md(r, a.md, shapes, *(AA_MD if a.antialias else PLAIN_MD))


if __name__ == "__main__":
    main()
