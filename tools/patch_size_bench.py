#!/usr/bin/env python3
"""Cost of the patch size: the folded patch-embed kernels alone and a whole bf16 training step at patch sizes 1, 2 and 4.

    python tools/patch_size_bench.py [--md profiles/patch_size.md] [--rounds 3] [--seconds 0.5] [--legs LEG,LEG,...]
                                     [--root TREE]

A leg is `<model>:<H>x<W>:<B>:<patch>`; the default legs are interm_117m and interm_8m on the 32 x 64 grid of BASELINE configs[1]
at batch 8, patch sizes 2 and 4, and interm_8m at patch size 1 on the same grid.  Per leg one child process measures
  (a) `_hip.varagg_fwd` and `_hip.varagg_bwd` alone on random tables of the leg's shape (HIP events around a batch of calls),
  (b) one eager bf16 training step of the model under HipDataParallel: forward, bayesian_tv, backward, gradient sync, AdamW
      (host clock around steps that end in a synchronise).  No hipGraph replay at any patch size (capture is built for patch
      size 2 only), so the legs differ in the patch size alone.
Every timing is repeated `--rounds` times, alternating (a) and (b); the mean and the spread (max - min) / mean are reported.
`--root` imports `climate_learn` and `oracle` from another checkout of the project (an older commit, for the patch-size-2 legs:
same script, same box, same call); legs that tree refuses are reported as refused.  Each child runs under its own time limit
and the chain stops at the first failure.  The table-gradient kernel's own time comes from a kernel trace of `--child LEG
--embed-only` taken in a run of its own; `--counts LEG` prints its FLOP and byte counts from the shapes.
This is a tool beside bench.py, not part of it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"interm_8m": dict(embed_dim=256, depth=6, num_heads=4), "interm_117m": dict(embed_dim=1024, depth=8, num_heads=16)}
DEFAULT_LEGS = ["interm_117m:32x64:8:2", "interm_117m:32x64:8:4", "interm_8m:32x64:8:2", "interm_8m:32x64:8:4",
                "interm_8m:32x64:8:1"]


def parse_leg(leg):
    model, grid, B, p = leg.split(":")
    h, w = (int(v) for v in grid.split("x"))
    return model, (h, w), int(B), int(p)


def counts(leg, V=23):
    """operations and bytes the table-gradient stage needs, from the shapes: dgtab[v][c][i] = sum_t a pt dz is 2 V C D FLOP per
    token (+ D per (token, variable) for a * dz); dz is read once per variable (bf16), the slabs are written once (fp32)"""
    model, (h, w), B, p = parse_leg(leg)
    D, H = MODELS[model]["embed_dim"], MODELS[model]["num_heads"]
    C, ntok = p * p + 1, B * (h // p) * (w // p)
    flop = ntok * V * D * (2.0 * C + 1.0)
    byts = V * ntok * D * 2.0 + ntok * V * (C - 1) * 4.0 + 2.0 * ntok * H * V * 4.0
    return {"leg": leg, "tokens": ntok, "C": C, "flop": flop, "bytes_min": byts}


def _stats(ms):
    mean = sum(ms) / len(ms)
    return {"ms": round(mean, 4), "spread": round((max(ms) - min(ms)) / mean, 4), "rounds_ms": [round(v, 4) for v in ms]}


def child(leg, rounds, seconds, embed_only):
    import torch
    import torch.nn as nn
    import climate_learn as cl
    from climate_learn import _hip
    from climate_learn.metrics import Bayesian_TV
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.models.hub.components.vit_blocks import Block
    from climate_learn.trainer import training_step
    from oracle.harness import ERA5_OUT, ERA5_VARS, ERA5_VW
    name, grid, B, p = parse_leg(leg)
    m = MODELS[name]
    D, H, V = m["embed_dim"], m["num_heads"], len(ERA5_VARS)
    dev = torch.device("cuda", 0)
    try:
        model = Res_Slim_ViT(ERA5_VARS, grid, V, len(ERA5_OUT), 1, patch_size=p, embed_dim=D, depth=m["depth"], decoder_depth=4,
                             num_heads=H, drop_path=0.1, drop_rate=0.1, learn_pos_emb=True)
    except NotImplementedError as e:
        print("RESULT " + json.dumps({"leg": leg, "refused": str(e)[:200]}), flush=True)
        return
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, V, *grid, generator=g)
    y = torch.randn(B, len(ERA5_OUT), grid[0] * 4, grid[1] * 4, generator=g)
    C, ntok = p * p + 1, B * (grid[0] // p) * (grid[1] // p)
    xd = x.to(dev)
    stab = (0.3 * torch.randn(H, V, C, generator=g)).to(dev)
    gtab = (0.2 * torch.randn(V, C, D, generator=g)).to(dev)
    dz = torch.randn(ntok, D, generator=g).to(torch.bfloat16).to(dev)
    z, attw = _hip.varagg_fwd(xd, stab, gtab, H, D)

    def ev(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def wall(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    legs = {"embed_fwd": (ev, lambda: _hip.varagg_fwd(xd, stab, gtab, H, D)),
            "embed_bwd": (ev, lambda: _hip.varagg_bwd(xd, gtab, attw, dz, H, D))}
    if embed_only:
        for _, fn in legs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        print("RESULT " + json.dumps({"leg": leg, "embed_only": True}), flush=True)
        return
    model.data_config(156.0, grid, V, len(ERA5_OUT))
    eng = cl.HipDataParallel(model.to(dev), unit_types=(Block, nn.Sequential))
    opt = cl.load_optimizer(eng, "adamw", {"lr": 1e-4, "weight_decay": 1e-5, "betas": (0.9, 0.99)})
    lossf = Bayesian_TV(aggregate_only=True)
    eng.train()
    batch = (xd, y.to(dev), ERA5_VARS, ERA5_OUT)

    def step():
        loss = training_step(batch, 0, eng, dev, ERA5_VW, lossf)
        opt.zero_grad()
        loss.backward()
        eng.finish_grad_sync()
        opt.step()
    legs["train_step"] = (wall, step)
    n, ms = {}, {k: [] for k in legs}
    for k, (timer, fn) in legs.items():                 # warm-up at the leg's own shape, and the size of a batch of calls
        for _ in range(3):
            fn()
        n[k] = max(3, int(1e3 * seconds / max(timer(fn, 3), 1e-3)))
    for _ in range(rounds):
        for k, (timer, fn) in legs.items():
            ms[k].append(timer(fn, n[k]))
    res = {"leg": leg, "model": name, "grid": list(grid), "B": B, "patch": p, "tokens": ntok, "calls_per_round": n}
    res.update({k: _stats(v) for k, v in ms.items()})
    print("RESULT " + json.dumps(res), flush=True)


def markdown(results, root):
    out = ["## Patch size: the folded patch-embed kernels alone and one eager bf16 training step", "",
           "date %s, tree `%s`; per leg the mean of the rounds and their spread (max - min) / mean" % (
               time.strftime("%Y-%m-%d"), root), "",
           "| leg (model : grid : batch : patch) | tokens | embed fwd ms | embed bwd ms | train step ms | spread fwd / bwd / step | "
           "embed bwd share of the step |", "|---|---|---|---|---|---|---|"]
    for r in results:
        if "refused" in r:
            out.append("| %s | refused: %s |" % (r["leg"], r["refused"]))
            continue
        f, b, s = r["embed_fwd"], r["embed_bwd"], r["train_step"]
        out.append("| %s | %d | %.4f | %.4f | %.3f | %.1f %% / %.1f %% / %.1f %% | %.1f %% |" % (
            r["leg"], r["tokens"], f["ms"], b["ms"], s["ms"], 100 * f["spread"], 100 * b["spread"], 100 * s["spread"],
            100 * b["ms"] / s["ms"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--embed-only", action="store_true", help="with --child: a few embed forward / backward calls (for a trace)")
    ap.add_argument("--counts", default=None, metavar="LEG")
    ap.add_argument("--legs", default=",".join(DEFAULT_LEGS))
    ap.add_argument("--root", default=ROOT, help="the checkout to import climate_learn and oracle from")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--timeout", type=int, default=180, help="time limit of each child, seconds")
    ap.add_argument("--md", default=None, help="write the table as markdown to this file")
    a = ap.parse_args()
    if a.counts:
        print(json.dumps(counts(a.counts)))
        return 0
    root = os.path.abspath(a.root)
    if a.child:
        sys.path[:0] = [root, os.path.join(root, "orbit-2_amd")]
        return child(a.child, max(3, a.rounds), a.seconds, a.embed_only)
    results = []
    for leg in a.legs.split(","):
        # a fresh process per leg, under its own time limit; the chain stops at the first failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--root", root, "--rounds", str(a.rounds),
                                "--seconds", str(a.seconds)], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("leg %s exceeded %d s: stopping" % (leg, a.timeout), flush=True)
            return 1
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("leg %s failed (exit %d): stopping\n%s" % (leg, r.returncode, (r.stdout + r.stderr)[-3000:]), flush=True)
            return 1
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    md = markdown(results, os.path.relpath(root, ROOT))
    print(md, flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write(md)
    return 0


if __name__ == "__main__":
    sys.exit(main())
