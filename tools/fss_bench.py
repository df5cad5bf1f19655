#!/usr/bin/env python3
"""Cost of the fractions skill score: the entry against its bandwidth floor and against the torch formulation, across windows.

    python tools/fss_bench.py [--md profiles/fss.md] [--rounds 5] [--shape 16,3,512,1024] [--target-hw 721,1440] [--entry-only]

A [16, 3, 512, 1024] prediction against a [16, 3, 721, 1440] target (read through its top-left crop), one process on one card,
every leg alternating `--rounds` times after a warm-up of each, HIP events around a window of calls.  Zero-inflated fields (70 %
exact zeros, the rest gamma-distributed), the prediction the target moved by a few pixels plus noise; T = 3 thresholds, the
channel's pooled target quantiles at +1 / +2 / +3 sigma, still on the device.  Per window n in 3, 9, 33, 129:
  entry            `_hip.masked_fss` (orbit2_masked_loss_fwd at ORBIT2_FSS_KIND, csrc/fss.hip): a memset, the bit-plane pass, the
                   window pass, the final ratio
  bits / window    the two passes apart, from the profiler's kernel records of the same call (null where no profiler is built in)
  torch            what a user would otherwise write: per threshold and field a thresholded float plane,
                   F.avg_pool2d(..., n, 1, n // 2, count_include_pad=True) * n^2 (zero padding), squares and sums over the valid
and once:
  copy             the floor: a device copy of the bytes the entry reads -- the prediction, and the target's crop out of its
                   larger rows -- into a buffer of two fields (400 MB move, more than the last-level cache holds)
--entry-only times the entry legs alone and writes no file: for comparing two builds of the library (ORBIT2_HIP_LIB), as the
ablations of the band height and of the leaving row in profiles/fss.md were.
No ratio is fixed in advance: the file states the measured ones.  This is a tool beside bench.py, not part of it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]

LEVELS = (0.8413, 0.9772, 0.9987)                                   # metrics.functional.SIGMA_LEVELS
WINDOWS = (3, 9, 33, 129)


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


def _kernel_split(fn, reps=5):
    """{kernel name fragment: mean ms} of the two passes from the profiler's kernel records, or None"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for frag in ("fss_bits_kernel", "fss_window_kernel", "fss_final_kernel"):
                if frag in ev.key:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    out[frag] = out.get(frag, 0.0) + total / 1000.0 / reps
        return out if len(out) >= 2 else None
    except Exception:                                                # no profiler in this build: the split stays unmeasured
        return None


def torch_fss(pred, crop, thr, n):
    """[B,C,T] double: the formulation on thresholded floats; crop is the target's top-left crop of the prediction's size"""
    import torch
    import torch.nn.functional as F
    valid = torch.isfinite(crop)
    out = []
    for k in range(thr.shape[1]):
        t = thr[:, k].view(1, -1, 1, 1)
        cO = F.avg_pool2d((valid & (crop >= t)).float(), n, 1, n // 2, count_include_pad=True) * (n * n)
        cM = F.avg_pool2d((valid & (pred >= t)).float(), n, 1, n // 2, count_include_pad=True) * (n * n)
        v = valid.double()
        num = ((cO - cM).double().square() * v).sum((2, 3))
        den = (cO.double().square() * v).sum((2, 3)) + (cM.double().square() * v).sum((2, 3))
        out.append(1.0 - num / den)
    return torch.stack(out, -1)


def run(shape, target_hw, rounds, entry_only=False):
    import torch
    from climate_learn import _hip
    B, C, H, W = shape
    Ht, Wt = target_hw
    field = B * C * H * W * 4
    g = torch.Generator(device="cuda").manual_seed(0)
    wet = torch.rand(shape, device="cuda", generator=g) >= 0.7
    crop = torch.where(wet, torch.randn(shape, device="cuda", generator=g).square() * 4.0, torch.zeros((), device="cuda"))
    crop = torch.nn.functional.avg_pool2d(crop, 5, 1, 2)             # events with some extent, as rain has
    pred = torch.roll(crop, (2, 3), (2, 3)) + 0.1 * torch.randn(shape, device="cuda", generator=g)
    target = torch.zeros(B, C, Ht, Wt, device="cuda")
    target[:, :, :H, :W] = crop
    levels = torch.tensor(LEVELS, dtype=torch.float32, device="cuda")
    thr = _hip.masked_quantiles(pred, target, levels)[0][0, :, :, 0].contiguous()
    T = len(LEVELS)
    scratch = torch.empty((2,) + tuple(shape), device="cuda")
    strip, band = _hip.fss_partition(B, C, H, W, T)
    legs = {"copy": (lambda: (scratch[0].copy_(pred), scratch[1].copy_(target[:, :, :H, :W])), 50)}
    check, split = {}, {}
    for n in WINDOWS:
        legs["entry n=%d" % n] = (lambda n=n: _hip.masked_fss(pred, target, thr, n), 20)
        if entry_only:
            continue
        legs["torch n=%d" % n] = (lambda n=n: torch_fss(pred, crop, thr, n), 2 if n < 100 else 1)
        got = _hip.masked_fss(pred, target, thr, n)[0].double()
        check[n] = float((got - torch_fss(pred, crop, thr, n)).abs().max())
        split[n] = _kernel_split(legs["entry n=%d" % n][0])
    for fn, _ in legs.values():                                      # warm-up: code objects, the allocator's blocks
        fn()
        fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, reps) in legs.items():
            ms[k].append(_ev(fn, reps))
    res = {"shape": list(shape), "target_hw": list(target_hw), "rounds": rounds, "levels": list(LEVELS), "field_bytes": field,
           "strip": strip, "band": band,
           "library": open(_hip.LIB_PATH + ".srchash").read().strip() if os.path.exists(_hip.LIB_PATH + ".srchash") else None,
           "max_abs_diff_to_torch": check, "split_ms": split, "legs": {}}
    for k in legs:
        mean = sum(ms[k]) / rounds
        res["legs"][k] = {"ms": round(mean, 4), "spread": round((max(ms[k]) - min(ms[k])) / mean, 4)}
    e = {n: res["legs"]["entry n=%d" % n]["ms"] for n in WINDOWS}
    res["entry n=129 / n=3"] = round(e[129] / e[3], 3)
    if entry_only:
        return res
    res["torch / entry"] = {n: round(res["legs"]["torch n=%d" % n]["ms"] / e[n], 2) for n in WINDOWS}
    res["entry / copy"] = {n: round(e[n] / res["legs"]["copy"]["ms"], 2) for n in WINDOWS}
    # the rows a plane's bands walk: every step of a band adds an entering row, every centre takes a leaving one
    walk = lambda n: sum(min(y0 + band, H) - max(y0 - 2 * (n // 2), -(n // 2)) for y0 in range(0, H, band)) + H
    res["rows walked"] = {n: walk(n) for n in WINDOWS}
    res["predicted window pass n=129 / n=3"] = round(walk(129) / walk(3), 3)
    if split[129] and split[3]:
        res["window pass n=129 / n=3"] = round(split[129]["fss_window_kernel"] / split[3]["fss_window_kernel"], 3)
    return res


KEEP = "## Ablations"                # what a profile holds from this heading on was written by hand from --entry-only runs: kept


def write_md(path, r):
    kept = ""
    if os.path.exists(path):
        old = open(path).read()
        kept = old[old.index(KEEP):] if KEEP in old else ""
    with open(path, "w") as f:
        f.write("# The fractions skill score: bit planes and the window pass (tools/fss_bench.py)\n\n")
        f.write("One MI355X, one process, all legs alternating, %d rounds after a warm-up, HIP events; prediction [%s] fp32 against a "
                "target [.., %s] read through its top-left crop; T = 3 thresholds (the pooled target quantiles at %s); strips of %d "
                "columns, bands of %d rows.  Library source hash `%s`.\n\n"
                % (r["rounds"], ", ".join(map(str, r["shape"])), ", ".join(map(str, r["target_hw"])),
                   ", ".join(map(str, r["levels"])), r["strip"], r["band"], r["library"]))
        f.write("`copy` is a device copy of the bytes the entry reads (the prediction, and the target's crop out of its larger rows) "
                "into a buffer of two fields: %.4f ms (spread %.1f %%), %.0f GB/s read + written.  "
                % (r["legs"]["copy"]["ms"], 100 * r["legs"]["copy"]["spread"], 4 * r["field_bytes"] / (1e6 * r["legs"]["copy"]["ms"])))
        f.write(                "`torch` is F.avg_pool2d(count_include_pad=True, zero padding) on thresholded floats, per threshold and field, then "
                "the squares and sums.  `bits` / `window` are the entry's two passes from the profiler's kernel records.\n\n")
        f.write("| window | entry ms (spread) | bits ms | window ms | entry / copy | torch ms (spread) | torch / entry | max abs diff to torch |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for n in WINDOWS:
            e, t, s = r["legs"]["entry n=%d" % n], r["legs"]["torch n=%d" % n], r["split_ms"][n]
            f.write("| %d | %.4f (%.1f %%) | %s | %s | %.2f | %.3f (%.1f %%) | %.2f | %.1e |\n"
                    % (n, e["ms"], 100 * e["spread"], "%.4f" % s["fss_bits_kernel"] if s else "n/a",
                       "%.4f" % s["fss_window_kernel"] if s else "n/a", r["entry / copy"][n], t["ms"], 100 * t["spread"],
                       r["torch / entry"][n], r["max_abs_diff_to_torch"][n]))
        f.write("\nEntry, n = 129 over n = 3: %.3f.  Window pass alone: %s.  The partition predicts %.3f for the window pass: the rows "
                "the bands of a plane walk, %d over %d (a band of `band` centres adds band + 2 r entering rows, the first band of a "
                "plane r fewer, and takes band leaving rows).\n"
                % (r["entry n=129 / n=3"], r.get("window pass n=129 / n=3", "n/a"), r["predicted window pass n=129 / n=3"],
                   r["rows walked"][129], r["rows walked"][3]))
        if kept:
            f.write("\n" + kept)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default="16,3,512,1024")
    ap.add_argument("--target-hw", default="721,1440")
    ap.add_argument("--entry-only", action="store_true")
    a = ap.parse_args()
    r = run(tuple(int(v) for v in a.shape.split(",")), tuple(int(v) for v in a.target_hw.split(",")), a.rounds, a.entry_only)
    print(json.dumps(r), flush=True)
    if a.md and not a.entry_only:
        write_md(a.md, r)


if __name__ == "__main__":
    main()
