#!/usr/bin/env python3
"""Cost of the all-member ensemble scores: `orbit2_ensemble_scores` against a device-to-device copy and the eager formulation.

    python tools/ensemble_scores_bench.py [--md profiles/ensemble_scores.md] [--members 8,16,32,64] [--rounds 3]

Per N on a [16, 3, 512, 1024] field, in one process on one card, legs alternating `--rounds` times after a warm-up of each:
  kernel  `_hip.ensemble_scores(stack, target, lat_w, sums=True, quantiles=[0.05, 0.5, 0.95])`: reads N + 1 fields once, writes 3;
  sums    the same call with the sums alone (reads N + 1 fields, writes 96 doubles);
  copy    `copy_` of a buffer of (N + 1) / 2 fields: (N + 1) fields' bytes moved, half read and half written;
  eager   `torch.sort` of the stack over the members, the same four sums from the sorted values, `torch.quantile`.
HIP events around each leg; GB/s of each leg on its own byte count, the kernel's rate over the copy's, and the peak allocated
memory of the kernel and of the eager leg beyond the stack itself.  This is a tool beside bench.py, not part of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]

SHAPE = (16, 3, 512, 1024)
LEVELS = [0.05, 0.5, 0.95]


def _ev(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, torch.cuda.max_memory_allocated() - base


def eager_scores(stack, target, lat_w):
    """the eager formulation: sort over the members, the four sums per (b, c) from the sorted values, torch.quantile"""
    import torch
    n = stack.shape[0]
    d = torch.sort(stack, dim=0).values
    d -= target
    k = torch.arange(1, n + 1, device=stack.device, dtype=stack.dtype).view(n, 1, 1, 1, 1)
    w = lat_w.view(1, 1, -1, 1)
    parts = (d.abs().mean(0), ((2 * k - n - 1) * d).sum(0), d.mean(0) ** 2, d.var(0))
    sums = torch.stack([(w * p).double().sum((2, 3)) for p in parts], dim=-1)
    return sums, torch.quantile(stack, torch.tensor(LEVELS, device=stack.device), dim=0)


def one_size(n, rounds):
    import torch
    from climate_learn import _hip
    B, C, H, W = SHAPE
    field = B * C * H * W
    g = torch.Generator(device="cuda").manual_seed(n)
    stack = torch.empty((n,) + SHAPE, device="cuda")
    for i in range(n):
        stack[i].normal_(generator=g)
    target = torch.randn(SHAPE, device="cuda", generator=g)
    lat_w = torch.rand(H, device="cuda", generator=g) + 0.5
    src = torch.randn((n + 1) * field // 2, device="cuda", generator=g)
    dst = torch.empty_like(src)
    legs = {"kernel": (lambda: _hip.ensemble_scores(stack, target, lat_w, sums=True, quantiles=LEVELS), 10, (n + 1 + 3) * field * 4),
            "sums": (lambda: _hip.ensemble_scores(stack, target, lat_w, sums=True), 10, (n + 1) * field * 4),
            "copy": (lambda: dst.copy_(src), 10, (n + 1) * field * 4),
            "eager": (lambda: eager_scores(stack, target, lat_w), 1, None)}
    with torch.no_grad():
        got, want = legs["kernel"][0](), legs["eager"][0]()
        rel = float(((got["sums"] - want[0]).abs() / want[0].abs().clamp_min(1e-30)).max())
        qerr = float((got["quantiles"] - want[1]).abs().max())
        del got, want
        legs["sums"][0](), legs["copy"][0]()
        ms, peak = {k: [] for k in legs}, {}
        for _ in range(rounds):
            for k, (fn, reps, _) in legs.items():
                t, peak[k] = _ev(fn, reps)
                ms[k].append(t)
    res = {"N": n, "shape": list(SHAPE), "max_rel_diff_sums_vs_eager": rel, "max_abs_diff_quantiles_vs_eager": qerr}
    for k, (_, _, nbytes) in legs.items():
        mean = sum(ms[k]) / rounds
        res[k] = {"ms": round(mean, 3), "spread": round((max(ms[k]) - min(ms[k])) / mean, 4), "peak_MiB": round(peak[k] / 2 ** 20, 1)}
        if nbytes:
            res[k]["GBps"] = round(nbytes / (1e6 * mean), 1)
    res["kernel_over_copy"] = round(res["kernel"]["GBps"] / res["copy"]["GBps"], 3)
    res["sums_over_copy"] = round(res["sums"]["GBps"] / res["copy"]["GBps"], 3)
    del stack, src, dst
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--members", default="8,16,32,64")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    rows = []
    for n in (int(v) for v in a.members.split(",")):
        rows.append(one_size(n, a.rounds))
        print(json.dumps(rows[-1]), flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# All-member ensemble scores: the kernel against a copy and the eager formulation "
                    "(tools/ensemble_scores_bench.py)\n\n")
            f.write("One MI355X, one process, legs alternating, %d rounds, HIP events; field [%s] fp32.\n`kernel` = sums + 3 quantile "
                    "fields in one `orbit2_ensemble_scores` (N + 1 fields read, 3 written); `sums` = the sums alone; `copy` = "
                    "`copy_` moving (N + 1) fields' bytes, half read, half written; `eager` = `torch.sort` + the same sums + "
                    "`torch.quantile`.  Peak MiB is what a leg allocates beyond the stack.\n\n" % (a.rounds, ", ".join(map(str, SHAPE))))
            f.write("| N | kernel ms (spread) | kernel GB/s | sums ms | sums GB/s | copy ms | copy GB/s | kernel / copy | sums / copy | "
                    "eager ms | kernel peak MiB | eager peak MiB | max rel diff of sums | max abs diff of quantiles |\n"
                    "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %d | %.3f (%.1f %%) | %.1f | %.3f | %.1f | %.3f | %.1f | %.3f | %.3f | %.1f | %.1f | %.1f | %.1e | %.1e |\n" % (
                    r["N"], r["kernel"]["ms"], 100 * r["kernel"]["spread"], r["kernel"]["GBps"], r["sums"]["ms"], r["sums"]["GBps"],
                    r["copy"]["ms"], r["copy"]["GBps"], r["kernel_over_copy"], r["sums_over_copy"], r["eager"]["ms"],
                    r["kernel"]["peak_MiB"], r["eager"]["peak_MiB"], r["max_rel_diff_sums_vs_eager"],
                    r["max_abs_diff_quantiles_vs_eager"]))


if __name__ == "__main__":
    main()
