#!/usr/bin/env python3
"""Cost of the missing-data masks: the masked loss and moments kernels against the unmasked ones of the same library.

    python tools/masked_bench.py [--md profiles/masked.md] [--rounds 5] [--shape 16,3,512,1024] [--target-hw 721,1440]

A [16, 3, 512, 1024] prediction against a [16, 3, 721, 1440] target (read through its top-left crop), in one process on one card,
every leg alternating `--rounds` times after a warm-up of each, HIP events around 200 calls (windows of 10 to 60 ms):
  loss <kind>            `_hip.loss_fwd` + `_hip.loss_bwd` (orbit2_loss_fwd / _bwd, csrc/loss.hip: the unmasked kernels)
  masked <kind> <form>   `_hip.masked_loss_fwd` + `_hip.masked_loss_bwd` (the same file) with no mask, an [H,W] mask and a
                         [B,C,H,W] mask; the masks are smooth blobs (coastlines, not salt and pepper) with about 40 % invalid
  moments                `_hip.eval_moments`;  masked moments <form>: `_hip.masked_moments`
for kind in mse, bayesian_tv.  GB/s is each leg's time over its ALGORITHMIC bytes: forward = prediction + target crop (+ mask)
read, backward = the same read + the gradient written; a broadcast mask counts once, the stencil's re-reads of neighbouring
rows do not count.  `x parent` is the leg's time over the unmasked leg's, `bytes x` the same ratio of the algorithmic bytes: what a
kernel that is bound by memory alone would show.  This is a tool beside bench.py, not part of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]

KINDS = (("mse", 0), ("bayesian_tv", 1))
FORMS = ("none", "[H,W]", "[B,C,H,W]")


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


def _blobs(shape, invalid, gen):
    """uint8 mask of `shape` ([..., H, W]): smooth blobs, `invalid` of the pixels zero"""
    import torch
    H, W = shape[-2:]
    lead = tuple(shape[:-2]) + (1, 1)
    yy = torch.arange(H, device="cuda").view(H, 1) / 41.0
    xx = torch.arange(W, device="cuda").view(1, W) / 67.0
    ph = torch.rand(lead + (3,), device="cuda", generator=gen) * 6.28
    f = torch.sin(yy + ph[..., 0]) + torch.cos(xx + ph[..., 1]) + 0.5 * torch.sin(yy * 2.3 + xx * 1.7 + ph[..., 2])
    thr = torch.quantile(f.flatten()[:: max(1, f.numel() // 1000000)].float(), invalid)
    return (f > thr).to(torch.uint8).contiguous()


def run(shape, target_hw, rounds, reps=200):
    import torch
    from climate_learn import _hip
    B, C, H, W = shape
    Ht, Wt = target_hw
    field = B * C * H * W * 4                                       # bytes of one fp32 field of the prediction's size
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.randn(shape, device="cuda", generator=g)
    target = torch.randn(B, C, Ht, Wt, device="cuda", generator=g)
    target[:, :, :H, :W] += 0.6 * pred
    lat_w = torch.rand(H, device="cuda", generator=g) + 0.5
    chan_w = torch.tensor([1.0] + [10.0] * (C - 1), device="cuda")
    gs = torch.ones(1, device="cuda")
    masks = {"none": (None, (0, 0, 0), 0),
             "[H,W]": (_blobs((H, W), 0.4, g), (W, 0, 0), H * W),
             "[B,C,H,W]": (_blobs((B, C, H, W), 0.4, g), (W, C * H * W, H * W), B * C * H * W)}

    def plain(kind):
        _hip.loss_fwd(pred, target, lat_w, chan_w, kind)
        _hip.loss_bwd(pred, target, lat_w, chan_w, gs, kind)

    def masked(kind, form):
        m, strides, _ = masks[form]
        _, cnt = _hip.masked_loss_fwd(pred, target, lat_w, chan_w, kind, m, strides)
        _hip.masked_loss_bwd(pred, target, lat_w, chan_w, gs, cnt, kind, m, strides)

    legs = {}                                                       # name -> (fn, algorithmic bytes, parent leg)
    for name, kind in KINDS:
        legs["loss " + name] = (lambda kind=kind: plain(kind), 5 * field, None)
        for form in FORMS:
            legs["masked %s %s" % (name, form)] = (lambda kind=kind, form=form: masked(kind, form),
                                                   5 * field + 2 * masks[form][2], "loss " + name)
    legs["moments"] = (lambda: _hip.eval_moments(pred, target, lat_w), 2 * field, None)
    for form in FORMS:
        legs["masked moments " + form] = (lambda form=form: _hip.masked_moments(pred, target, lat_w, None, masks[form][0],
                                                                                masks[form][1]),
                                          2 * field + masks[form][2], "moments")
    for fn, _, _ in legs.values():                                  # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, _, _) in legs.items():
            ms[k].append(_ev(fn, reps))
    res = {"shape": list(shape), "target_hw": list(target_hw), "rounds": rounds, "reps": reps, "legs": {}}
    for form in FORMS[1:]:
        res["valid_fraction " + form] = round(float(masks[form][0].float().mean()), 4)
    for k, (_, nbytes, parent) in legs.items():
        mean = sum(ms[k]) / rounds
        res["legs"][k] = {"ms": round(mean, 4), "spread": round((max(ms[k]) - min(ms[k])) / mean, 4),
                          "GBps": round(nbytes / (1e6 * mean), 1), "bytes": nbytes, "parent": parent}
    for k, leg in res["legs"].items():
        if leg["parent"]:
            p = res["legs"][leg["parent"]]
            leg["x_parent"] = round(leg["ms"] / p["ms"], 3)
            leg["x_bytes"] = round(leg["bytes"] / p["bytes"], 4)
    # the two families agree where they must: no mask and a finite target
    a = _hip.loss_fwd(pred, target, lat_w, chan_w, 1)
    b, _ = _hip.masked_loss_fwd(pred, target, lat_w, chan_w, 1)
    res["max_rel_diff_all_valid"] = float(((a - b).abs() / a.abs()).max())
    return res


def write_md(path, r):
    with open(path, "w") as f:
        f.write("# Missing-data masks: the masked kernels against the unmasked ones (tools/masked_bench.py)\n\n")
        f.write("One MI355X, one process, all legs alternating, %d rounds of %d calls after a warm-up, HIP events; prediction [%s] "
                "fp32 against a target [.., %s] read through its top-left crop, latitude and variable weights on.  `loss` / `moments` "
                "are the unmasked kernels of the same library (csrc/loss.hip); a `masked` loss leg is forward + backward.  The "
                "masks are smooth blobs, valid fraction %.2f ([H,W]) and %.2f ([B,C,H,W]).  GB/s counts a leg's algorithmic bytes "
                "(fields and mask once; not the stencil's re-reads of neighbouring rows).  `x parent` is measured time over the "
                "unmasked leg's, `bytes x` the ratio a purely memory-bound kernel would show.\n\n"
                % (r["rounds"], r["reps"], ", ".join(map(str, r["shape"])), ", ".join(map(str, r["target_hw"])),
                   r["valid_fraction [H,W]"], r["valid_fraction [B,C,H,W]"]))
        f.write("| leg | ms per call (spread) | GB/s of its algorithmic bytes | x parent (time) | bytes x (expected) |\n"
                "|---|---|---|---|---|\n")
        for k, leg in r["legs"].items():
            f.write("| %s | %.4f (%.1f %%) | %.1f | %s | %s |\n"
                    % (k, leg["ms"], 100 * leg["spread"], leg["GBps"],
                       "%.3f" % leg["x_parent"] if leg["parent"] else "1 (parent)",
                       "%.4f" % leg["x_bytes"] if leg["parent"] else "1"))
        f.write("\nAll valid (no mask, finite target), bayesian_tv: masked and unmasked forward agree within %.1e (relative).\n"
                % r["max_rel_diff_all_valid"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default="16,3,512,1024")
    ap.add_argument("--target-hw", default="721,1440")
    a = ap.parse_args()
    r = run(tuple(int(v) for v in a.shape.split(",")), tuple(int(v) for v in a.target_hw.split(",")), a.rounds)
    print(json.dumps(r), flush=True)
    if a.md:
        write_md(a.md, r)


if __name__ == "__main__":
    main()
