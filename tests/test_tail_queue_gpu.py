"""The tail queue (csrc/tail_queue.h): a launch whose last tiles go by ticket computes every tile exactly as the static
launch does, so every comparison here is torch.equal against the plain entry, on every output, and the counter words read zero
afterwards.  The `tail_queue=<tiles>` hook of the wrappers forces a queued part on problems of a few hundred tiles:

  GEMM       M = 5120, N = 4096, K = 512: 320 tiles of 256 x 256 = 256 static + 64 by ticket + 64 spare workgroups
  attention  d = 128, L = 1024, B = 8, H = 12: 384 forward / dQ tiles (256 + 128 + 128), 768 dK + dV tiles (640 + 128 + 128)

Outputs are pre-filled with NaN (or a sentinel): a tile that nobody took would show."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
M, N, K = 5120, 4096, 512
TAIL = 64                                     # GEMM tiles by ticket
ROWS = 512                                    # rows per gate entry (two tile rows): 10 samples
AB, AL, AH, AD = 8, 1024, 12, 128
ATAIL = 128


def _dev(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *shape, scale=0.5: (torch.randn(*shape, device="cuda", generator=g) * scale).to(BF)


def _ws_is_zero():
    from climate_learn import _hip
    torch.cuda.synchronize()
    return int(torch.count_nonzero(_hip.sched_workspace())) == 0


@pytest.fixture(scope="module")
def gemm_data():
    rnd = _dev(31)
    return dict(A=rnd(M, K), Bt=rnd(N, K), Bn=rnd(K, N), bias=rnd(N), residual=rnd(M, N), old=rnd(M, N),
                q14=torch.randint(-16384, 16384, (M, N), device="cuda", dtype=torch.int16))


def _gemm_cases(d):
    """name -> (b_kc, keyword arguments, side outputs, gated?): the 4-wave kernel's epilogue kinds in the forms that compile them, the
    runtime epilogue with beta != 0, and the gated forms with a dropped sample in the static part and one in the tail"""
    gate = torch.ones(M // ROWS, device="cuda", dtype=F32)
    gate[1] = 0.0                             # tile rows 2, 3: static ids
    gate[9] = 0.0                             # tile rows 18, 19: the last ids, taken by ticket
    gk = dict(gate=gate, rows_per_gate=ROWS)
    return {
        "nt_kind0_lean": (True, dict(bias=d["bias"], colscale=(256, 0.1275)), (), False),
        "nn_kind0_lean": (False, dict(), (), False),
        "nt_kind0_beta": (True, dict(bias=d["bias"], beta=0.5), (), False),
        "nt_kind1_save_dact": (True, dict(bias=d["bias"], act=1, drop_p=0.1, seed=77), ("save_dact",), False),
        "nt_kind2_residual": (True, dict(bias=d["bias"], drop_p=0.1, seed=78, residual=d["residual"], ldr=N), (), False),
        "nn_kind3_colsum": (False, dict(mul=d["q14"], want_colsum=True), ("colsum",), False),
        "nt_kind0_gated": (True, dict(bias=d["bias"], colscale=(256, 0.1275), **gk), (), True),
        "nn_kind0_gated": (False, dict(**gk), (), True),
        "nt_kind1_gated": (True, dict(bias=d["bias"], act=1, drop_p=0.1, seed=77, **gk), ("save_dact",), True),
        "nt_kind2_gated": (True, dict(bias=d["bias"], drop_p=0.1, seed=78, residual=d["residual"], ldr=N, rowscale=gate,
                                      rows_per_scale=ROWS, **gk), (), True),
        "nn_kind3_gated": (False, dict(mul=d["q14"], want_colsum=True, **gk), ("colsum",), True),
    }


def _run_gemm(d, case, tail_queue):
    from climate_learn import _hip
    b_kc, kw, side, _ = case
    kw = dict(kw)
    want_colsum = kw.pop("want_colsum", False)
    out = d["old"].clone() if kw.get("beta") else torch.full((M, N), NAN, device="cuda", dtype=BF)
    dact = None
    if "save_dact" in side:
        dact = torch.full((M, N), 12345, device="cuda", dtype=torch.int16)
        kw["save_dact"] = dact
    r = _hip.gemm(d["A"], d["Bt"] if b_kc else d["Bn"], out, M, N, K, K, K if b_kc else N, N, a_kc=True, b_kc=b_kc, tile=260,
                  want_colsum=want_colsum, tail_queue=tail_queue, **kw)
    outs = [out] + ([dact] if dact is not None else [])
    if want_colsum:
        assert r[1] is not None and r[1].shape == (M // 256, N)
        outs.append(r[1])
    return outs


@pytest.mark.parametrize("name", ["nt_kind0_lean", "nn_kind0_lean", "nt_kind0_beta", "nt_kind1_save_dact", "nt_kind2_residual",
                                  "nn_kind3_colsum", "nt_kind0_gated", "nn_kind0_gated", "nt_kind1_gated", "nt_kind2_gated",
                                  "nn_kind3_gated"])
def test_gemm_with_a_queued_tail_equals_the_static_launch(gemm_data, name):
    case = _gemm_cases(gemm_data)[name]
    ref = _run_gemm(gemm_data, case, None)
    got = _run_gemm(gemm_data, case, TAIL)
    assert len(ref) == len(got) == 1 + len(case[2])
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert not torch.isnan(ref[0].float()).any()
    if case[3]:                               # the gate did skip: both dropped samples hold the fill, in the static part and in the tail
        for e in (1, 9):
            rows = slice(e * ROWS, (e + 1) * ROWS)
            fill = gemm_data["residual"][rows] if "residual" in case[1] else torch.zeros_like(got[0][rows])
            assert torch.equal(got[0][rows], fill)
    assert _ws_is_zero()


def test_tails_the_plan_refuses_stay_static(gemm_data):
    """a tail larger than the launch, and the library's own sizing on a launch of fewer than six rounds: the plain launch"""
    case = _gemm_cases(gemm_data)["nt_kind0_lean"]
    ref = _run_gemm(gemm_data, case, None)
    for tq in (321, 100000, True):
        assert torch.equal(_run_gemm(gemm_data, case, tq)[0], ref[0])
    assert torch.equal(_run_gemm(gemm_data, case, 320)[0], ref[0])              # every tile by ticket: no static part at all
    assert _ws_is_zero()


def test_grouped_weight_gradients_with_a_queued_tail():
    """three weight gradients in one launch (4-wave TN kernel; 64 + 96 + 2 x 48 = 256 tiles): a K gate on every problem, the last
    problem split over the tokens into two half-length ones, the tail (100 tiles) spanning the split problems and part of the second"""
    from climate_learn import _hip
    rnd = _dev(32)
    rows, ns = 256, 6                         # six samples of 256 tokens
    m = rows * ns
    gate = torch.tensor([1, 0, 1, 1, 0, 1], device="cuda", dtype=F32) * (1.0 / 0.9)
    drop = (gate == 0).repeat_interleave(rows)
    shapes = [(2048, 2048), (2048, 3072), (2048, 1536)]
    dys = [rnd(m, n) for n, _ in shapes]
    xs = [rnd(m, k) for _, k in shapes]
    for dy in dys:
        dy[drop] = 0
    half = m // 2

    def run(tail_queue):
        outs = [torch.full((n, k), NAN, device="cuda", dtype=BF) for n, k in shapes[:2]]
        parts = torch.full((2, shapes[2][0], shapes[2][1]), NAN, device="cuda", dtype=BF)
        kw = dict(a_kc=False, b_kc=False)
        probs = [(dy, x, o, n, k, m, n, k, k, dict(kw, kgate=(gate, rows))) for dy, x, o, (n, k) in zip(dys, xs, outs, shapes)]
        n, k = shapes[2]
        for q in range(2):
            probs.append((dys[2][q * half:(q + 1) * half], xs[2][q * half:(q + 1) * half], parts[q], n, k, half, n, k, k,
                          dict(kw, kgate=(gate[q * 3:(q + 1) * 3], rows))))
        _hip.gemm_grouped(probs, tail_queue=tail_queue)
        return outs + [parts]

    ref, got = run(None), run(100)
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and not torch.isnan(a.float()).any()
    assert _ws_is_zero()


def test_plain_calls_leave_the_counter_storage_alone():
    """a call without tail_queue passes no counter: it neither allocates the device's counter buffer nor claims a word for its
    stream -- a fresh stream here, whose claim would show"""
    from climate_learn import _hip
    rnd = _dev(34)
    bufs, slots = dict(_hip._sched_bufs), dict(_hip._sched_slots)
    blank = lambda: torch.full((256, 256), NAN, device="cuda", dtype=BF)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        c = _hip.gemm(rnd(256, 64), rnd(256, 64), blank(), 256, 256, 64, 64, 64, 256, tile=260)
        a, b, outs = rnd(256, 128), rnd(256, 128), [blank(), blank()]
        _hip.gemm_grouped([(a, b, o, 256, 256, 128, 128, 128, 256, {}) for o in outs])
        qkv = rnd(256, 3 * 128)
        out, lse = _hip.attn_fwd(qkv, 1, 256, 1, 128, flags=_hip.ATTN_Q_PRESCALED)
        dqkv = _hip.attn_bwd(qkv, out, rnd(256, 128), lse, 1, 256, 1, 128, flags=_hip.ATTN_Q_PRESCALED)
    stream.synchronize()
    for t in (c, outs[0], outs[1], out, lse, dqkv):
        assert not torch.isnan(t.float()).any()                   # every call did launch
    assert _hip._sched_slots == slots
    assert _hip._sched_bufs.keys() == bufs.keys() and all(_hip._sched_bufs[k] is v for k, v in bufs.items())


@pytest.fixture(scope="module")
def attn_data():
    rnd = _dev(33)
    gate = torch.ones(AB, device="cuda", dtype=F32)
    gate[2] = 0.0
    gate[7] = 0.0
    return dict(qkv=rnd(AB * AL, 3 * AH * AD), dout=rnd(AB * AL, AH * AD), gate=gate)


def _attn(d, p, gate, tail_queue):
    """forward, then the backward on the forward's own results: (out, lse, dqkv)"""
    from climate_learn import _hip
    flags, seed = _hip.ATTN_Q_PRESCALED, 99
    out = torch.full((AB * AL, AH * AD), NAN, device="cuda", dtype=BF)
    out, lse = _hip.attn_fwd(d["qkv"], AB, AL, AH, AD, p, seed, flags=flags, out=out, gate=gate, tail_queue=tail_queue)
    dout = d["dout"]
    if gate is not None:                      # what the gated Block holds for a dropped sample
        dout = dout.clone()
        dout[(gate == 0).repeat_interleave(AL)] = 0
    dqkv = _hip.attn_bwd(d["qkv"], out, dout, lse, AB, AL, AH, AD, p, seed, flags=flags, gate=gate, tail_queue=tail_queue)
    return out, lse, dqkv


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_with_a_queued_tail_equals_the_static_launch(attn_data, p, gated):
    gate = attn_data["gate"] if gated else None
    ref = _attn(attn_data, p, gate, None)
    got = _attn(attn_data, p, gate, ATAIL)
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and not torch.isnan(a.float()).any()
    if gated:
        rows = (gate == 0).repeat_interleave(AL)
        assert torch.count_nonzero(got[0][rows]) == 0 and torch.count_nonzero(got[2][rows]) == 0
        assert torch.count_nonzero(got[1][gate == 0]) == 0
    assert _ws_is_zero()


def _pair(gemm_data, attn_data, tail):
    """the GEMM case and the attention forward case, one after the other on the current stream"""
    from climate_learn import _hip
    case = (True, dict(bias=gemm_data["bias"], drop_p=0.1, seed=78, residual=gemm_data["residual"], ldr=N), (), False)
    c = _run_gemm(gemm_data, case, TAIL if tail else None)[0]
    out = torch.full((AB * AL, AH * AD), NAN, device="cuda", dtype=BF)
    out, lse = _hip.attn_fwd(attn_data["qkv"], AB, AL, AH, AD, 0.1, 99, flags=_hip.ATTN_Q_PRESCALED, out=out,
                             tail_queue=ATAIL if tail else None)
    return c, out, lse


def test_back_to_back_two_streams_and_graph_replays(gemm_data, attn_data):
    """the counter is left zero by every launch: twice back to back on one stream; on two streams at the same time (a word per
    stream); captured once into a graph and replayed twice.  Equal results every time, the workspace all zeros afterwards."""
    ref = _pair(gemm_data, attn_data, False)
    torch.cuda.synchronize()

    def same(res):
        return all(torch.equal(a, b) for a, b in zip(res, ref))

    first, second = _pair(gemm_data, attn_data, True), _pair(gemm_data, attn_data, True)
    assert same(first) and same(second) and _ws_is_zero()

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    res = []
    for s in (s1, s2, s1, s2):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            res.append(_pair(gemm_data, attn_data, True))
    torch.cuda.synchronize()
    assert all(same(r) for r in res) and _ws_is_zero()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):             # the capture stream's allocations, uncaptured
        _pair(gemm_data, attn_data, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _pair(gemm_data, attn_data, True)
    for _ in range(2):
        for t in held:
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert same(held) and _ws_is_zero()
