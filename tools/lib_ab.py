"""The part that the same-process A/B tools of two builds of the library share (tools/loss_lib_ab.py, tools/varagg_lib_ab.py,
tools/gemm_lib_ab.py, tools/image_lib_ab.py):
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/<kernels>_lib_ab.py orbit-2_amd/lib/alt/<name>.so [other.so]
`libs` holds the working-tree library ("tree"; or other.so in its place: an A/A run of two builds of one revision) and the other
build ("alt"; of the same ABI version: _hip.load) side by side.  A tool calls every entry of its files in both and prints one line
per case through `tally`, then `summary`.  Every destination lies inside a NaN-filled buffer with a guard band on either side
(`guarded`) and the whole buffer is compared (`bitwise`); `+=` destinations are prefilled.  A timed line runs both builds
interleaved, the median of 5 rounds of 4 launches per build, and shows the relative gap of the medians."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "orbit-2_amd")]
import torch
from climate_learn import _hip

libs = {"alt": _hip.load(os.path.abspath(sys.argv[1])),
        "tree": _hip.load(os.path.abspath(sys.argv[2])) if len(sys.argv) > 2 else _hip.lib()}
P = lambda t: None if t is None else t.data_ptr()
S = lambda: torch.cuda.current_stream().cuda_stream
ok = lambda rc: rc == 0 or sys.exit("rc = %d" % rc)
GUARD = 64
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}
count = {}                                                                   # kind -> [lines, lines that pass]
gaps = []


def t(f, n=4):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
med = lambda v: sorted(v)[len(v) // 2]


def timed(run, outs):
    ms = {k: [] for k in libs}
    for _ in range(5):
        for k, lib in libs.items(): ms[k].append(t(lambda: run(lib, outs[k])))
    gap = med(ms["tree"]) / med(ms["alt"]) - 1
    return gap, "   alt %8.4f ms | tree %8.4f ms (%+.1f %%)" % (med(ms["alt"]), med(ms["tree"]), 100 * gap)


def tally(kind, line, passed, run=None, outs=None):
    count.setdefault(kind, [0, 0])
    count[kind][0] += 1; count[kind][1] += bool(passed)
    if run is not None:
        gap, text = timed(run, outs); gaps.append((gap, line.split(":")[0])); line += text
    print(line, flush=True)


def guarded(n, dtype, lead=GUARD, prefill=None):
    """per build: a NaN-filled buffer of lead + n + GUARD elements (the n in the middle prefilled where the entry adds)"""
    bufs = {k: torch.full((lead + n + GUARD,), float("nan"), dtype=dtype, device="cuda") for k in libs}
    if prefill is not None:
        for b in bufs.values(): b[lead:lead + n] = prefill
    return bufs


def bitwise(kind, tag, call, n, dtype, lead=GUARD, prefill=None, timing=False):
    """call(lib, address of the destination) in both builds; the whole buffers bit for bit, and the destination was written"""
    bufs = guarded(n, dtype, lead, prefill)
    run = lambda lib, b: ok(call(lib, b.data_ptr() + lead * b.element_size()))
    for k, lib in libs.items(): run(lib, bufs[k])
    torch.cuda.synchronize()
    eq = torch.equal(bufs["tree"].view(BITS[dtype]), bufs["alt"].view(BITS[dtype])) \
        and not bool(torch.isnan(bufs["tree"][lead:lead + n]).any())
    tally(kind, "%-9s %s: bitwise equal %s" % (kind, tag, eq), eq, run if timing else None, bufs)
    return bufs["tree"][lead:lead + n]


def summary(note=None):
    """the counts per kind, a tool's own note, the gaps of the timed lines; exit status 1 if a line did not pass"""
    worst = max(gaps, key=lambda v: abs(v[0]))
    parts = ["%d lines" % sum(v[0] for v in count.values()), "; ".join("%s: %d of %d" % (k, v[1], v[0]) for k, v in count.items())]
    parts += [note] if note else []
    parts += ["gaps of the medians in percent %s" % " ".join("%+.1f" % (100 * v[0]) for v in gaps),
              "largest %+.1f %% (%s)" % (100 * worst[0], worst[1])]
    print("; ".join(parts))
    sys.exit(any(v[0] != v[1] for v in count.values()))
