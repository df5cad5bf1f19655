#!/usr/bin/env python3
"""Speed of the fp32 forward (`model.set_compute_dtype(torch.float32)`) against the reference's formulation in fp32 on the same card.

    python tools/fp32_forward_bench.py [--md profiles/fp32_forward.md] [--rounds 3] [--seconds 1.0]

Per configuration (interm_117m on a 64 x 128 grid at B = 4; interm_1b on 128 x 256 at B = 1) one child process times
  (a) the HIP fp32 forward,
  (b) the oracle's forward as eager fp32 PyTorch on the GPU (oracle.orbit2_oracle.forward on device tensors under no_grad, no
      autocast: library GEMMs; the full attention through F.scaled_dot_product_attention, as bench.py's GPU baseline does),
  (c) the HIP bf16 forward, for context (no engine here: the bf16 compute copies are cast from the masters in every forward).
Every leg is warmed up at its own shape; then (a), (b), (c) are timed in turn, `--rounds` times, each timing a batch of forwards
that fills about `--seconds`, host clock around work that ends in a synchronise.  The mean over the rounds and their spread
(max - min) / mean are reported.  A third child measures the fp32 GEMM and the fp32 attention alone (TF/s, HIP events) beside
their eager counterparts (torch.mm, SDPA).  Each child runs under its own time limit and the chain stops at the first failure.
This is a tool beside bench.py, not part of it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]

MODELS = {"interm_117m": dict(embed_dim=1024, depth=8, num_heads=16, grid=(64, 128), B=4),
          "interm_1b": dict(embed_dim=3072, depth=8, num_heads=24, grid=(128, 256), B=1)}


def _timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def _stats(ms):
    mean = sum(ms) / len(ms)
    return {"ms": round(mean, 3), "spread": round((max(ms) - min(ms)) / mean, 4), "rounds_ms": [round(v, 3) for v in ms]}


def child_model(name, rounds, seconds):
    import torch
    import torch.nn.functional as F
    from climate_learn.models.hub import Res_Slim_ViT
    from oracle import orbit2_oracle as O
    from oracle.harness import ERA5_OUT, ERA5_VARS
    m = MODELS[name]
    dev = torch.device("cuda", 0)
    grid, B = m["grid"], m["B"]
    cfg = O.Config(ERA5_VARS, grid, len(ERA5_OUT), m["embed_dim"], m["depth"], 4, m["num_heads"], spatial_resolution=156.0)
    sd = O.init_state_dict(cfg, len(ERA5_VARS), seed=0, fast=True)
    model = Res_Slim_ViT(ERA5_VARS, grid, len(ERA5_VARS), len(ERA5_OUT), 1, patch_size=2, embed_dim=m["embed_dim"],
                         depth=m["depth"], decoder_depth=4, num_heads=m["num_heads"], drop_path=0.0, drop_rate=0.0)
    model.load_state_dict(sd, strict=True)
    model.data_config(156.0, grid, len(ERA5_VARS), len(ERA5_OUT))
    model = model.to(dev).eval()
    sdd = {k: v.to(dev) for k, v in sd.items()}
    x = torch.randn(B, len(ERA5_VARS), *grid, generator=torch.Generator().manual_seed(0)).to(dev)
    naive = O.mha_core

    def sdpa(q, k, v, scale, pmask=None):
        if q.shape[-2] != k.shape[-2]:                 # the 1-query variable aggregation stays on the plain form
            return naive(q, k, v, scale, pmask)
        return F.scaled_dot_product_attention(q, k, v, scale=scale)
    O.mha_core = sdpa

    def hip32():
        return model.set_compute_dtype(torch.float32)(x, ERA5_VARS, ERA5_OUT)

    def hip16():
        return model.set_compute_dtype(torch.bfloat16)(x, ERA5_VARS, ERA5_OUT)

    def eager32():
        with torch.device(dev):                        # the oracle's constants follow the device
            return O.forward(sdd, cfg, x, ERA5_VARS, ERA5_OUT)
    legs = {"hip_fp32": hip32, "eager_fp32": eager32, "hip_bf16": hip16}
    with torch.no_grad():
        outs, n = {}, {}
        for k, fn in legs.items():                     # warm-up at the leg's own shape, and the size of a batch of forwards
            outs[k] = fn()
            fn()
            n[k] = max(1, int(seconds / max(_timed(fn, 1), 1e-4)))
        ms = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                ms[k].append(1e3 * _timed(fn, n[k]))
    ref = outs["eager_fp32"].double()
    err = {k: float((outs[k].double() - ref).abs().max() / ref.abs().max()) for k in ("hip_fp32", "hip_bf16")}
    res = {"config": name, "grid": list(grid), "B": B, "forwards_per_round": n, "err_vs_eager_fp32": err}
    res.update({k: _stats(v) for k, v in ms.items()})
    print("RESULT " + json.dumps(res), flush=True)


def child_kernels():
    import torch
    import torch.nn.functional as F
    from climate_learn import _hip

    def ev(fn, n):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    rows = []
    for tag, (M, N, K) in (("fc1 interm_117m (B=4, L=2048)", (8192, 4096, 1024)), ("fc1 interm_1b (B=1, L=8192)", (8192, 12288, 3072))):
        A, W = torch.randn(M, K, device="cuda"), torch.randn(N, K, device="cuda") * 0.02
        b, out = torch.randn(N, device="cuda"), torch.empty(M, N, device="cuda")
        t_hip = ev(lambda: _hip.gemm_f32(A, W, out, M, N, K, K, K, N, bias=b, act=1), 10)
        t_mm = ev(lambda: F.gelu(F.linear(A, W, b)), 10)
        t_mm0 = ev(lambda: torch.mm(A, W.t()), 10)
        fl = 2.0 * M * N * K
        rows.append({"kernel": "gemm_f32 + bias + GELU, " + tag, "hip_ms": round(t_hip, 3), "hip_tflops": round(fl / t_hip / 1e9, 1),
                     "eager_ms": round(t_mm, 3), "eager_tflops": round(fl / t_mm / 1e9, 1),
                     "eager_note": "F.gelu(F.linear) fp32; torch.mm alone %.3f ms = %.1f TF/s" % (t_mm0, fl / t_mm0 / 1e9)})
    for B, L, H, d in ((4, 2048, 16, 64), (1, 8192, 24, 128)):
        qkv = torch.randn(B, L, 3, H, d, device="cuda")
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        t_hip = ev(lambda: _hip.attn_fwd_f32(qkv, B, L, H, d), 5)
        t_sd = ev(lambda: F.scaled_dot_product_attention(q, k, v), 5)
        fl = 4.0 * B * H * L * L * d
        rows.append({"kernel": "attn_fwd_f32 L=%d d=%d (B=%d, H=%d)" % (L, d, B, H), "hip_ms": round(t_hip, 3),
                     "hip_tflops": round(fl / t_hip / 1e9, 1), "eager_ms": round(t_sd, 3),
                     "eager_tflops": round(fl / t_sd / 1e9, 1), "eager_note": "F.scaled_dot_product_attention fp32 on strided q, k, v views"})
    print("RESULT " + json.dumps({"kernels": rows}), flush=True)


def _digest():
    p = os.path.join(ROOT, "orbit-2_amd", "lib", "liborbit2_hip.so.srchash")
    return open(p).read().strip() if os.path.exists(p) else "unknown"


def markdown(results, kernels):
    out = ["## Speed: HIP fp32 forward against the oracle's forward as eager fp32 PyTorch on the same card", "",
           "date %s, library source digest `%s`" % (time.strftime("%Y-%m-%d"), _digest()), "",
           "| configuration | (a) HIP fp32 ms | (b) eager fp32 ms | (a) / (b) | (c) HIP bf16 ms | spread a / b / c | fp32 vs eager `pred` | bf16 vs eager `pred` |",
           "|---|---|---|---|---|---|---|---|"]
    for r in results:
        a, b, c = r["hip_fp32"], r["eager_fp32"], r["hip_bf16"]
        out.append("| %s %dx%d B=%d | %.2f | %.2f | %.2f | %.2f | %.1f %% / %.1f %% / %.1f %% | %.1e | %.1e |" % (
            r["config"], r["grid"][0], r["grid"][1], r["B"], a["ms"], b["ms"], a["ms"] / b["ms"], c["ms"],
            100 * a["spread"], 100 * b["spread"], 100 * c["spread"], r["err_vs_eager_fp32"]["hip_fp32"],
            r["err_vs_eager_fp32"]["hip_bf16"]))
    out += ["", "| kernel | HIP ms | HIP TF/s | eager ms | eager TF/s | eager counterpart |", "|---|---|---|---|---|---|"]
    for k in kernels:
        out.append("| %s | %.3f | %.1f | %.3f | %.1f | %s |" % (k["kernel"], k["hip_ms"], k["hip_tflops"], k["eager_ms"],
                                                               k["eager_tflops"], k["eager_note"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--timeout", type=int, default=240, help="time limit of each child, seconds")
    ap.add_argument("--md", default=None, help="write the tables as markdown to this file")
    a = ap.parse_args()
    if a.child == "kernels":
        return child_kernels()
    if a.child:
        return child_model(a.child, max(3, a.rounds), a.seconds)
    results, kernels = [], []
    for leg in list(MODELS) + ["kernels"]:
        # a fresh process per leg, under its own time limit; the chain stops at the first failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--rounds", str(a.rounds),
                                "--seconds", str(a.seconds)], capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print("leg %s exceeded %d s: stopping" % (leg, a.timeout), flush=True)
            return 1
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("leg %s failed (exit %d): stopping\n%s" % (leg, r.returncode, (r.stdout + r.stderr)[-3000:]), flush=True)
            return 1
        res = json.loads(line[-1][7:])
        print(json.dumps(res), flush=True)
        if leg == "kernels":
            kernels = res["kernels"]
        else:
            results.append(res)
    md = markdown(results, kernels)
    print(md, flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write(md)
    slower = [r["config"] for r in results if r["hip_fp32"]["ms"] > r["eager_fp32"]["ms"]]
    if slower:
        print("HIP fp32 forward slower than the eager fp32 forward on: %s" % ", ".join(slower), flush=True)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
