#!/usr/bin/env python3
"""Cost of an MC-dropout ensemble: the streamed statistics against the stacked formulation, and the Welford kernel as a stream.

    python tools/mc_dropout_bench.py [--md profiles/mc_dropout.md] [--members 16] [--rounds 3]

Per configuration (interm_117m on a 64 x 128 grid at B = 1 and 8; interm_1b on 128 x 256 at B = 1 and 16) and N members:
  (a) `mc_dropout_statistics` + `.std` (one `orbit2_ensemble_update` per member, three fields live),
  (b) the reference's formulation: `get_monte_carlo_predictions` (N fields stacked) + `mean(0)` + `std(0)`,
timed in turn `--rounds` times in one process, host clock around work that ends in a synchronise, after a warm-up of each leg
at its own shape; time per member, the spread (max - min) / mean over the rounds, and each leg's peak allocated memory.
Then `orbit2_ensemble_update` alone at [16, 3, 512, 1024] (20 bytes per element: 12 read, 8 written) in GB/s against a
device-to-device `copy_` of the same byte count (half read, half written) timed in the same process with HIP events.
This is a tool beside bench.py, not part of it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]

CONFIGS = [("interm_117m", dict(embed_dim=1024, depth=8, num_heads=16, grid=(64, 128)), (1, 8)),
           ("interm_1b", dict(embed_dim=3072, depth=8, num_heads=24, grid=(128, 256)), (1, 16))]


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated()


def model_legs(name, m, B, members, rounds):
    import torch
    import climate_learn as cl
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.utils import get_monte_carlo_predictions, mc_dropout_statistics
    from oracle.harness import ERA5_OUT, ERA5_VARS
    dev = torch.device("cuda", 0)
    grid = m["grid"]
    torch.manual_seed(0)
    with torch.device(dev):
        model = Res_Slim_ViT(ERA5_VARS, grid, len(ERA5_VARS), len(ERA5_OUT), 1, patch_size=2, embed_dim=m["embed_dim"],
                             depth=m["depth"], decoder_depth=4, num_heads=m["num_heads"], drop_path=0.1, drop_rate=0.1)
    model.data_config(156.0, grid, len(ERA5_VARS), len(ERA5_OUT))
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, len(ERA5_VARS), *grid, generator=g).to(dev)
    y = torch.randn(B, len(ERA5_OUT), 4 * grid[0], 4 * grid[1], generator=g).to(dev)
    batch = (x, y, ERA5_VARS, ERA5_OUT)
    out = {}

    def streamed():
        cl.manual_seed(1)
        st = mc_dropout_statistics(batch, model, members)
        out["streamed"] = (st.mean, st.std)

    def stacked():
        cl.manual_seed(1)
        stack = get_monte_carlo_predictions(batch, model, members)
        out["stacked"] = (stack.mean(0), stack.std(0))
    legs = {"streamed": streamed, "stacked": stacked}
    for fn in legs.values():
        fn()
    err = max(float((a - b).abs().max()) for a, b in zip(out["streamed"], out["stacked"]))
    sec, peak = {k: [] for k in legs}, {}
    for _ in range(rounds):
        for k, fn in legs.items():
            out.clear()
            t, peak[k] = _timed(fn)
            sec[k].append(t)
    res = {"model": name, "grid": list(grid), "B": B, "members": members, "max_abs_diff_streamed_vs_stacked": err}
    for k in legs:
        mean = sum(sec[k]) / rounds
        res[k] = {"ms_per_member": round(1e3 * mean / members, 3), "spread": round((max(sec[k]) - min(sec[k])) / mean, 4),
                  "peak_MiB": round(peak[k] / 2 ** 20, 1)}
    del model, out
    torch.cuda.empty_cache()
    return res


def kernel_leg(rounds):
    import torch
    from climate_learn import _hip
    n = 16 * 3 * 512 * 1024
    x, mean, m2 = (torch.randn(n, device="cuda") for _ in range(3))
    src, dst = torch.randn(5 * n // 2, device="cuda"), torch.empty(5 * n // 2, device="cuda")    # 10 n bytes read + 10 n written
    reps = 20

    def ev(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    upd = lambda i: _hip.ensemble_update(x, mean, m2, i + 2)                # noqa: E731
    cpy = lambda i: dst.copy_(src)                                          # noqa: E731
    upd(0), cpy(0)
    ms = {"ensemble_update": [], "copy": []}
    for _ in range(rounds):
        ms["ensemble_update"].append(ev(upd))
        ms["copy"].append(ev(cpy))
    gbs = {k: 20.0 * n / (1e6 * (sum(v) / rounds)) for k, v in ms.items()}
    return {"elements": n, "bytes": 20 * n, "ms": {k: round(sum(v) / rounds, 4) for k, v in ms.items()},
            "GBps": {k: round(v, 1) for k, v in gbs.items()}, "ratio_to_copy": round(gbs["ensemble_update"] / gbs["copy"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md")
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    rows = []
    for name, m, batches in CONFIGS:
        if a.only and a.only != name:
            continue
        for B in batches:
            rows.append(model_legs(name, m, B, a.members, a.rounds))
            print(json.dumps(rows[-1]), flush=True)
    k = kernel_leg(a.rounds)
    print(json.dumps(k), flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write("# MC-dropout ensembles: streamed statistics against stacking (tools/mc_dropout_bench.py)\n\n")
            f.write("One MI355X, one process, legs alternating, %d rounds, N = %d members; host clock around work ending in a "
                    "synchronise.\n`streamed` = `mc_dropout_statistics` + `.std`; `stacked` = `get_monte_carlo_predictions` + "
                    "`mean(0)` + `std(0)`.\n\n" % (a.rounds, a.members))
            f.write("| model | grid | B | streamed ms / member (spread) | stacked ms / member (spread) | streamed peak MiB | "
                    "stacked peak MiB | max abs diff of mean / std |\n|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write("| %s | %dx%d | %d | %.3f (%.1f %%) | %.3f (%.1f %%) | %.1f | %.1f | %.2e |\n" % (
                    r["model"], r["grid"][0], r["grid"][1], r["B"], r["streamed"]["ms_per_member"], 100 * r["streamed"]["spread"],
                    r["stacked"]["ms_per_member"], 100 * r["stacked"]["spread"], r["streamed"]["peak_MiB"],
                    r["stacked"]["peak_MiB"], r["max_abs_diff_streamed_vs_stacked"]))
            f.write("\n`orbit2_ensemble_update` alone, %d elements (20 bytes each = %.0f MB), HIP events over 20 launches, against "
                    "`copy_` of the same byte count:\n\n| | ms | GB/s |\n|---|---|---|\n" % (k["elements"], k["bytes"] / 1e6))
            for key in ("ensemble_update", "copy"):
                f.write("| %s | %.4f | %.1f |\n" % (key, k["ms"][key], k["GBps"][key]))
            f.write("\nratio to the copy: %.3f\n" % k["ratio_to_copy"])


if __name__ == "__main__":
    main()
