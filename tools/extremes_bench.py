#!/usr/bin/env python3
"""Cost of the extreme-value scores: the radix select against its bandwidth floor and against torch.sort, the tail pass against
masked moments on torch-built masks.

    python tools/extremes_bench.py [--md profiles/extremes.md] [--rounds 5] [--shape 16,3,512,1024] [--target-hw 721,1440]

A [16, 3, 512, 1024] prediction against a [16, 3, 721, 1440] target (read through its top-left crop), one process on one card,
every leg alternating `--rounds` times after a warm-up of each, HIP events around a window of calls.  Three value sets: Gaussian at
offset 280, a constant field, zero-inflated (70 % exact zeros, the rest gamma-distributed).  Per value set:
  select Q=6       `_hip.masked_quantiles` (orbit2_masked_loss_fwd at ORBIT2_MASKED_QUANTILES, csrc/extremes.hip): both fields,
                   G = C pooled groups, six levels -- a memset, four digit passes over prediction + target, four scans
  copy x passes    the floor the design aims at: a device copy of one field (its read + write move the bytes one digit pass
                   reads: prediction + target crop), times the four passes
  sort + gather    what a user would otherwise write: torch.sort of every channel of both fields, then a gather of the 12 ranks
  tail T=6         `_hip.masked_tail` at the six target quantiles, still on the device
  6 x moments      six `_hip.masked_moments` calls on `target >= thr` masks built with torch (the mask building is timed with them)
No ratio is fixed in advance: the file states the measured ones.  This is a tool beside bench.py, not part of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]

LEVELS = (0.0013, 0.0228, 0.1587, 0.8413, 0.9772, 0.9987)         # -3 .. +3 sigma
SETS = ("gaussian at 280", "constant", "zero-inflated")
PASSES = 4


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


def _field(name, shape, gen):
    import torch
    if name == "gaussian at 280":
        return 280.0 + 5.0 * torch.randn(shape, device="cuda", generator=gen)
    if name == "constant":
        return torch.full(shape, 3.25, device="cuda")
    wet = torch.rand(shape, device="cuda", generator=gen) >= 0.7
    return torch.where(wet, torch.randn(shape, device="cuda", generator=gen).square() * 4.0, torch.zeros((), device="cuda"))


def run(shape, target_hw, rounds):
    import torch
    from climate_learn import _hip
    B, C, H, W = shape
    Ht, Wt = target_hw
    field = B * C * H * W * 4
    g = torch.Generator(device="cuda").manual_seed(0)
    levels = torch.tensor(LEVELS, dtype=torch.float32, device="cuda")
    Q = len(LEVELS)
    scratch = torch.empty(shape, device="cuda")
    legs, check = {}, {}
    for name in SETS:
        crop = _field(name, shape, g)
        pred = (crop + 0.5 * torch.randn(shape, device="cuda", generator=g)) if name != "constant" else crop.clone()
        target = torch.zeros(B, C, Ht, Wt, device="cuda")
        target[:, :, :H, :W] = crop
        out, cnt = _hip.masked_quantiles(pred, target, levels)
        thr = out[0, :, :, 0].contiguous()

        def sort_path(pred=pred, crop=crop):
            res = []
            for x in (crop, pred):
                for c in range(C):
                    s, _ = x[:, c].reshape(-1).sort()
                    pos = levels.double() * (s.numel() - 1)
                    lo = pos.floor().long()
                    hi = (lo + 1).clamp_max(s.numel() - 1)
                    a, b = s[lo].double(), s[hi].double()
                    res.append((a + (pos - lo) * (b - a)).float())
            return torch.stack(res).view(2, C, Q)

        def six_moments(pred=pred, target=target, thr=thr):
            return [_hip.masked_moments(pred, target, None, None,
                                        (target[:, :, :H, :W] >= thr[:, k].view(1, C, 1, 1)).view(torch.uint8).contiguous(),
                                        (W, C * H * W, H * W)) for k in range(Q)]

        legs[name] = {
            "select Q=6": (lambda pred=pred, target=target: _hip.masked_quantiles(pred, target, levels), 50),
            "copy x passes": (lambda crop=crop: [scratch.copy_(crop) for _ in range(PASSES)], 50),
            "sort + gather": (sort_path, 3),
            "tail T=6": (lambda pred=pred, target=target, thr=thr: _hip.masked_tail(pred, target, thr), 50),
            "6 x moments": (six_moments, 10),
        }
        ref = sort_path()
        check[name] = {"select_equals_sort": bool(torch.equal(out[:, :, :, 0], ref)),
                       "max_abs_diff": float((out[:, :, :, 0] - ref).abs().max()), "valid": int(cnt.sum())}
        s, n = _hip.masked_tail(pred, target, thr)
        mom = six_moments()
        check[name]["tail_counts_equal_moments"] = bool(all(torch.equal(n[:, :, k, 0], mom[k][..., 12].long()) for k in range(Q)))
    for sets in legs.values():                                       # warm-up: code objects, the allocator's blocks
        for fn, _ in sets.values():
            fn()
            fn()
    ms = {(s, k): [] for s in legs for k in legs[s]}
    for _ in range(rounds):
        for s in legs:
            for k, (fn, reps) in legs[s].items():
                ms[s, k].append(_ev(fn, reps))
    res = {"shape": list(shape), "target_hw": list(target_hw), "rounds": rounds, "levels": list(LEVELS), "field_bytes": field,
           "library": open(_hip.LIB_PATH + ".srchash").read().strip() if os.path.exists(_hip.LIB_PATH + ".srchash") else None,
           "check": check, "sets": {}}
    for s in legs:
        row = {}
        for k in legs[s]:
            mean = sum(ms[s, k]) / rounds
            row[k] = {"ms": round(mean, 4), "spread": round((max(ms[s, k]) - min(ms[s, k])) / mean, 4)}
        row["select / floor"] = round(row["select Q=6"]["ms"] / row["copy x passes"]["ms"], 3)
        row["sort / select"] = round(row["sort + gather"]["ms"] / row["select Q=6"]["ms"], 2)
        row["moments / tail"] = round(row["6 x moments"]["ms"] / row["tail T=6"]["ms"], 2)
        row["select GBps"] = round(PASSES * 2 * field / (1e6 * row["select Q=6"]["ms"]), 1)
        row["tail GBps"] = round(2 * field / (1e6 * row["tail T=6"]["ms"]), 1)
        res["sets"][s] = row
    g280, zi = res["sets"][SETS[0]]["select Q=6"]["ms"], res["sets"][SETS[2]]["select Q=6"]["ms"]
    res["zero_inflated / gaussian"] = round(zi / g280, 3)
    return res


def write_md(path, r):
    with open(path, "w") as f:
        f.write("# Extreme-value scores: the radix select and the tail pass (tools/extremes_bench.py)\n\n")
        f.write("One MI355X, one process, all legs alternating, %d rounds after a warm-up, HIP events; prediction [%s] fp32 against a "
                "target [.., %s] read through its top-left crop; six levels (%s), G = C pooled groups, both fields.  Library source "
                "hash `%s`.\n\n"
                % (r["rounds"], ", ".join(map(str, r["shape"])), ", ".join(map(str, r["target_hw"])),
                   ", ".join(map(str, r["levels"])), r["library"]))
        f.write("The select reads the key in four digits of 8 bits (csrc/quantile_select.h: QS_DIGIT_BITS): a memset, four passes over "
                "prediction + target with 256-bin LDS histograms per tracked prefix (at most 16 per field, 32 KB of LDS), four scans.  "
                "The 11 / 11 / 10 split was not built: 2048 bins x 16 prefixes x 2 fields do not fit the 64 KB of static LDS the "
                "design keeps to, so no measurement chose between the two.  `copy x passes` is a device copy of one field (its "
                "read + write move the bytes one digit pass reads) times four: the floor the design aims at.  `sort + gather` is "
                "torch.sort of every channel of both fields plus a gather of the ranks.  `6 x moments` builds six `target >= thr` "
                "masks with torch and calls masked_moments on each.  GB/s: the select's 4 x 2 fields, the tail's 2 fields, over the "
                "measured time.\n\n")
        f.write("| value set | select Q=6 ms (spread) | copy x passes ms | select / floor | select GB/s | sort + gather ms | sort / select "
                "| tail T=6 ms (spread) | tail GB/s | 6 x moments ms | moments / tail |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for s, row in r["sets"].items():
            f.write("| %s | %.4f (%.1f %%) | %.4f | %.3f | %.1f | %.3f | %.2f | %.4f (%.1f %%) | %.1f | %.4f | %.2f |\n"
                    % (s, row["select Q=6"]["ms"], 100 * row["select Q=6"]["spread"], row["copy x passes"]["ms"], row["select / floor"],
                       row["select GBps"], row["sort + gather"]["ms"], row["sort / select"], row["tail T=6"]["ms"],
                       100 * row["tail T=6"]["spread"], row["tail GBps"], row["6 x moments"]["ms"], row["moments / tail"]))
        f.write("\nZero-inflated over Gaussian, select: %.3f.\n\n" % r["zero_inflated / gaussian"])
        f.write("Agreement on the same tensors: " + "; ".join(
            "%s: select == sort path %s (max |diff| %.1e), tail counts == moments counts %s"
            % (s, c["select_equals_sort"], c["max_abs_diff"], c["tail_counts_equal_moments"]) for s, c in r["check"].items()) + ".\n")


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
