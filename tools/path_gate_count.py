#!/usr/bin/env python3
"""How many (sample, Block, branch) units does DropPath drop in the benchmark's timed steps?  The prediction of what the path gate
("Path gate") can save is  sum over branches of  drops x (the branch's kernel time per step / batch).

Runs bench.py's own main() in this process with climate_learn._hip.droppath_scales wrapped to keep the scale vectors it returns
(an eager step returns a fresh tensor per call; nothing is read back until the run is over, so the timed loop is undisturbed),
then prints one JSON line: per timed step and Block the number of zeros in dp1 (attention branch) and dp2 (MLP branch).
The masks depend on the seeds alone -- not on the gate, not on the build -- so one count serves every arm of an A/B.

    python tools/path_gate_count.py --gpus 1 --steps 20 --warmup 5        (bench.py's arguments; eager steps only)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "orbit-2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import bench
    from climate_learn import _hip
    args = bench.parse()
    out_fd = os.dup(1)                       # (bench.main keeps the process's stdout for its own result line)
    drawn, orig = [], _hip.droppath_scales

    def keep(*a, **k):
        t = orig(*a, **k)
        drawn.append(t)
        return t

    _hip.droppath_scales = keep
    try:
        bench.main()
    except SystemExit as e:
        if e.code not in (None, 0):
            raise
    finally:
        _hip.droppath_scales = orig
    if not drawn or len(drawn) % (args.warmup + args.steps):
        raise SystemExit("path_gate_count: %d DropPath draws over %d eager steps -- a captured step replays one set of tensors; "
                         "run with --graph off" % (len(drawn), args.warmup + args.steps))
    per_step = len(drawn) // (args.warmup + args.steps)          # 2 draws per Block: dp1, dp2
    timed = drawn[args.warmup * per_step:]
    zeros = [int((t == 0).sum()) for t in timed]
    batch = int(timed[0].numel())
    steps = [[zeros[s * per_step + 2 * b: s * per_step + 2 * b + 2] for b in range(per_step // 2)] for s in range(args.steps)]
    attn = sum(z[0] for s in steps for z in s)
    mlp = sum(z[1] for s in steps for z in s)
    # (Blocks whose DropPath rate is 0 -- the first one under linspace(0, p, depth) -- draw nothing and are not listed)
    os.write(out_fd, (json.dumps({"path_gate_count": {"steps": args.steps, "blocks": per_step // 2, "batch": batch,
                                          "dropped_attn_units": attn, "dropped_mlp_units": mlp,
                                          "dropped_attn_per_step": attn / args.steps, "dropped_mlp_per_step": mlp / args.steps,
                                          "units_per_step": per_step * batch,
                                          "per_step_block_[attn,mlp]": steps}}) + "\n").encode())


if __name__ == "__main__":
    main()
