"""The path gate ("Path gate"): kernels that are told which samples a Block's branch dropped (DropPath scale 0.0) may
skip them, and must then store what annihilated inputs give.  Every comparison here is torch.equal against the ungated call:
kept samples bit for bit, dropped samples exactly zero (the residual rows in the proj / fc2 form), nothing left unwritten.

The GEMM cases force the 4-wave 256 x 256 kernel (tile hint 260), the attention cases run d = 128 with L a multiple of 256: the
kernel families that implement the gate.  A NaN planted in the dropped samples' INPUT rows shows that they were skipped and not
merely computed and discarded; the Block and step cases mix gated families with families that ignore the gate."""
import pytest
import torch
import torch.nn as nn

from tests._child import run_child

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
ROWS = 512                                   # rows per gate entry: two 256-row tiles
GATE = [1.0, 0.0, 1.0 / 0.9, 0.0, 1.0]       # five samples: kept, dropped, kept (a DropPath scale), dropped, kept
M, N, K = ROWS * len(GATE), 512, 192


def _dev(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *shape, scale=0.5: (torch.randn(*shape, device="cuda", generator=g) * scale).to(BF)


def _dropped_rows(gate, rows):
    return (gate == 0).repeat_interleave(rows)


def _gemm_forms():
    """name -> (operand form, keyword arguments, side outputs) of each gated GEMM form the Block uses"""
    rnd = _dev(1)
    bias = rnd(N)
    q14 = torch.randint(-16384, 16384, (M, N), device="cuda", dtype=torch.int16)
    return {
        "nt_lean_colscale": (True, dict(bias=bias, colscale=(256, 0.1275)), ()),                          # qkv
        "nt_kind1_save_dact": (True, dict(bias=bias, act=1, drop_p=0.1, seed=77), ("save_dact",)),         # fc1
        "nn_lean": (False, dict(), ()),                                                                    # do, dh1, dh2
        "nn_kind3_colsum": (False, dict(mul=q14, want_colsum=True), ("colsum",)),                          # dpre
        "nt_kind2_rowscale": (True, dict(bias=bias, drop_p=0.1, seed=78, residual=rnd(M, N), ldr=N), ()),  # proj, fc2
    }


@pytest.mark.parametrize("form", ["nt_lean_colscale", "nt_kind1_save_dact", "nn_lean", "nn_kind3_colsum", "nt_kind2_rowscale"])
def test_gated_gemm_equals_ungated_on_kept_rows_and_fills_dropped_rows(form):
    from climate_learn import _hip
    rnd = _dev(2)
    b_kc, kw, side = _gemm_forms()[form]
    kw = dict(kw)
    want_colsum = kw.pop("want_colsum", False)
    A = rnd(M, K)
    B = rnd(N, K) if b_kc else rnd(K, N)
    gate = torch.tensor(GATE, device="cuda", dtype=F32)
    drop = _dropped_rows(gate, ROWS)
    residual = kw.get("residual")
    if residual is not None:                     # the gate of this form IS the row scale
        kw.update(rowscale=gate, rows_per_scale=ROWS)

    def run(A_, gate_):
        out = torch.full((M, N), NAN, device="cuda", dtype=BF)
        k2 = dict(kw)
        dact = None
        if "save_dact" in side:
            dact = torch.full((M, N), 12345, device="cuda", dtype=torch.int16)
            k2["save_dact"] = dact
        if residual is not None and gate_ is not None:
            k2["rowscale"] = gate_
        r = _hip.gemm(A_, B, out, M, N, K, K, K if b_kc else N, N, a_kc=True, b_kc=b_kc, tile=260, want_colsum=want_colsum,
                      **(dict(gate=gate_, rows_per_gate=ROWS) if gate_ is not None else {}), **k2)
        parts = r[1] if want_colsum else None
        if want_colsum:
            assert parts is not None and parts.shape == (M // 256, N)
        return out, dact, parts

    ref = run(A, None)
    # a gate of all ones reproduces the ungated call (kind 2: ones as the row scale on both sides)
    ones = torch.ones_like(gate)
    if residual is not None:
        kw["rowscale"] = ones
        ref_ones = run(A, None)
        kw["rowscale"] = gate
    else:
        ref_ones = ref
    for a, b in zip(run(A, ones), ref_ones):
        assert a is None or torch.equal(a, b)
    # the dropped samples' input rows poisoned: a kernel that skips them never sees the NaN
    A_poison = A.clone()
    A_poison[drop] = NAN
    for A_ in (A, A_poison):
        out, dact, parts = run(A_, gate)
        assert torch.equal(out[~drop], ref[0][~drop])
        assert not torch.isnan(out.float()).any()
        if residual is not None:
            assert torch.equal(out[drop], residual[drop]) and torch.equal(ref[0][drop], residual[drop])
        else:
            assert torch.count_nonzero(out[drop]) == 0
        if dact is not None:
            assert torch.equal(dact[~drop], ref[1][~drop]) and torch.count_nonzero(dact[drop]) == 0
        if parts is not None:
            tile_drop = _dropped_rows(gate, ROWS // 256)
            assert torch.equal(parts[~tile_drop], ref[2][~tile_drop]) and torch.count_nonzero(parts[tile_drop]) == 0


def test_gemm_tiles_that_straddle_gate_entries_compute():
    """rows_per_gate = 384: tile rows 256 .. 511 straddle entries 0 and 1 and compute; kept rows equal the ungated call everywhere,
    and a dropped entry's rows are either the ungated values or zeros, never unwritten"""
    from climate_learn import _hip
    rnd = _dev(3)
    rows, m = 384, 1536
    A, B = rnd(m, K), rnd(N, K)
    gate = torch.tensor([0.0, 1.0, 0.0, 1.0], device="cuda", dtype=F32)
    drop = _dropped_rows(gate, rows)
    ref = _hip.gemm(A, B, torch.full((m, N), NAN, device="cuda", dtype=BF), m, N, K, K, K, N, tile=260)
    out = _hip.gemm(A, B, torch.full((m, N), NAN, device="cuda", dtype=BF), m, N, K, K, K, N, tile=260, gate=gate, rows_per_gate=rows)
    assert torch.equal(out[~drop], ref[~drop]) and not torch.isnan(out.float()).any()
    same_or_zero = (out == ref) | (out == 0)
    assert bool(same_or_zero.all())
    assert torch.count_nonzero(out[:256]) == 0 and torch.equal(out[256:512], ref[256:512])      # whole tile of entry 0 / the straddler


def test_gated_weight_gradient_group_skips_dropped_samples():
    """the grouped weight-gradient launch with a K gate per problem (4-wave TN kernel: 2 x 100 tiles): the contraction sweeps the
    kept samples only -- a NaN in the dropped samples' rows of the activation operand never reaches the result -- and equals the
    ungated launch bit for bit: dropped samples first, last, in the middle, none, all"""
    from climate_learn import _hip
    rnd = _dev(6)
    rows, n = 256, 2560
    for pattern in ([0, 1, 0, 0, 1, 0], [1, 1, 0, 1, 1, 1], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]):
        gate = torch.tensor(pattern, device="cuda", dtype=F32) * (1.0 / 0.9)
        drop = _dropped_rows(gate, rows)
        m = rows * len(pattern)
        dys, xs = [rnd(m, n), rnd(m, n)], [rnd(m, n), rnd(m, n)]
        for dy in dys:
            dy[drop] = 0                                       # what the path gate leaves in a dropped sample's gradient rows

        def run(xs_, gated):
            outs = [torch.full((n, n), NAN, device="cuda", dtype=BF) for _ in dys]
            kw = dict(a_kc=False, b_kc=False)
            _hip.gemm_grouped([(dy, x, o, n, n, m, n, n, n, dict(kw, kgate=(gate, rows)) if gated else kw)
                               for dy, x, o in zip(dys, xs_, outs)])
            return outs

        ref = run(xs, False)
        poisoned = [x.clone() for x in xs]
        for x in poisoned:
            x[drop] = NAN
        for xs_ in (xs, poisoned) if any(pattern) else (xs,):
            for a, b in zip(run(xs_, True), ref):
                assert torch.equal(a, b) and not torch.isnan(a.float()).any()


def _attn_call(fwd, gate, *args):
    """the C entries themselves (the Python wrappers allocate lse / dqkv, which this test pre-fills)"""
    from climate_learn import _hip
    lib = _hip.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rc = (lib.orbit2_attn_fwd_ld if fwd else lib.orbit2_attn_bwd_ld)(*args, None if gate is None else gate.data_ptr(), None, -1, stream)
    assert rc == 0


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gated_attention_equals_ungated_on_kept_samples_and_zero_fills_dropped_samples(p):
    from climate_learn import _hip
    Bn, L, H, d = 3, 512, 2, 128
    rnd = _dev(4)
    qkv = rnd(Bn * L, 3 * H * d)
    dout = rnd(Bn * L, H * d)
    gate = torch.tensor([1.0 / 0.9, 0.0, 1.0], device="cuda", dtype=F32)
    drop_rows, drop_b = _dropped_rows(gate, L), gate == 0
    flags, seed = _hip.ATTN_Q_PRESCALED, 99

    def fwd(qkv_, gate_):
        out = torch.full((Bn * L, H * d), NAN, device="cuda", dtype=BF)
        lse = torch.full((Bn, H, L), NAN, device="cuda", dtype=F32)
        _attn_call(True, gate_, qkv_.data_ptr(), out.data_ptr(), lse.data_ptr(), Bn, L, H, d, p, seed, flags, 3 * H * d, H * d)
        return out, lse

    def bwd(qkv_, out_, dout_, lse_, gate_):
        dqkv = torch.full((Bn * L, 3 * H * d), NAN, device="cuda", dtype=BF)
        delta = torch.empty(_hip.lib().orbit2_attn_bwd_ws_floats(Bn, L, H), device="cuda", dtype=F32)
        _attn_call(False, gate_, qkv_.data_ptr(), out_.data_ptr(), dout_.data_ptr(), lse_.data_ptr(), delta.data_ptr(),
                   dqkv.data_ptr(), Bn, L, H, d, p, seed, flags, 3 * H * d, H * d)
        return dqkv

    out0, lse0 = fwd(qkv, None)
    dqkv0 = bwd(qkv, out0, dout, lse0, None)
    ones = torch.ones_like(gate)
    for a, b in zip(fwd(qkv, ones) + (bwd(qkv, out0, dout, lse0, ones),), (out0, lse0, dqkv0)):
        assert torch.equal(a, b)
    qkv_poison = qkv.clone()
    qkv_poison[drop_rows] = NAN                   # a skipped sample's q, k, v are never read
    for qkv_ in (qkv, qkv_poison):
        out, lse = fwd(qkv_, gate)
        assert torch.equal(out[~drop_rows], out0[~drop_rows]) and torch.equal(lse[~drop_b], lse0[~drop_b])
        assert torch.count_nonzero(out[drop_rows]) == 0 and torch.count_nonzero(lse[drop_b]) == 0
        # backward on what the gated Block holds for a dropped sample: zero out, lse and dout
        dout_g = dout.clone()
        dout_g[drop_rows] = 0
        dqkv = bwd(qkv_, out, dout_g, lse, gate)
        assert torch.equal(dqkv[~drop_rows], dqkv0[~drop_rows])
        assert torch.count_nonzero(dqkv[drop_rows]) == 0 and not torch.isnan(dqkv.float()).any()


def _record_gates(monkeypatch):
    """the DropPath scale vectors the Blocks draw, for the assertion that the case did drop and did keep samples"""
    from climate_learn import _hip
    drawn, orig = [], _hip.droppath_scales

    def spy(*a, **k):
        t = orig(*a, **k)
        drawn.append(t)
        return t

    monkeypatch.setattr(_hip, "droppath_scales", spy)
    return drawn


@pytest.mark.parametrize("recompute", [False, True])
def test_block_is_the_same_with_and_without_the_gate(monkeypatch, recompute):
    """width 1024, 8 heads of 128, 16 samples of 256 tokens: the qkv and fc1 GEMMs, the fc2 input gradient and the three generated
    attention kernels take the gate, the narrower GEMMs run the 128-tile kernel and ignore it"""
    import climate_learn as cl
    from climate_learn import _ops
    from climate_learn.models.hub.components.vit_blocks import Block
    drawn = _record_gates(monkeypatch)
    torch.manual_seed(5)
    blk = Block(1024, 8, qkv_bias=True, proj_drop=0.1, attn_drop=0.1, drop_path=0.5).cuda().train()
    blk.recompute = recompute
    x0 = (torch.randn(16, 256, 1024, device="cuda") * 0.5).to(BF)

    def run(gate_on):
        monkeypatch.setattr(_ops, "_PATH_GATE", gate_on)
        for p in blk.parameters():
            p.grad = None
        x = x0.clone().requires_grad_()
        cl.manual_seed(13, 0)
        y = blk(x)
        y.float().square().mean().backward()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in blk.parameters()]

    on, off = run(True), run(False)
    assert len(on) == 2 + 12
    for g in drawn[:2]:
        assert 0 < int((g == 0).sum()) < g.numel()
    for a, b in zip(on, off):
        assert torch.equal(a, b) and not torch.isnan(a.float()).any()


def test_train_step_is_the_same_with_and_without_the_gate():
    run_child(__file__, "child_train_step_is_the_same_with_and_without_the_gate")


def child_train_step_is_the_same_with_and_without_the_gate():
    """one training step of an interm_8m-sized model (width 256, 32 x 64 grid; two heads of 128 so that the generated attention
    kernels run) in train mode: the parameters after AdamW, gate on against gate off, eager and through a captured graph"""
    import gc
    import os
    import climate_learn as cl
    from climate_learn import _hip, _ops
    from climate_learn.graphs import GraphedTrainStep
    from climate_learn.metrics import Bayesian_TV
    from climate_learn.models.hub.components.vit_blocks import Block
    from climate_learn.trainer import training_step
    from oracle.harness import build_pair

    # the engines below replay their captured steps one after the other, each from salt 0: sharing the device's salt word is the point
    os.environ["ORBIT2_ALLOW_SHARED_SALT"] = "1"
    vw = {"total_precipitation_24hr": 1.0}
    loss_fn = Bayesian_TV(aggregate_only=True)
    drawn, orig = [], _hip.droppath_scales

    def spy(*a, **k):
        t = orig(*a, **k)
        if not torch.cuda.is_current_stream_capturing():
            drawn.append(t.clone())
        return t

    _hip.droppath_scales = spy

    def step(gate_on, graphed):
        _ops._PATH_GATE = gate_on
        model, sd, cfg, O, x, y, in_vars, out_vars = build_pair(D=256, depth=2, heads=2, grid=(32, 64), B=4, seed=23)
        for blk in model.blocks:
            blk.attn.attn_drop_p = blk.attn.proj_drop_p = blk.mlp.drop = 0.1
            blk.drop_path = 0.5
        model.pos_drop_p = 0.1
        model = model.cuda().train()
        eng = cl.HipDataParallel(model, unit_types=(Block, nn.Sequential))
        batch = (x, y, in_vars, out_vars)
        opt = cl.load_optimizer(eng, "adamw", {"lr": 1e-3, "betas": (0.9, 0.99), "weight_decay": 1e-5})
        scaler = cl.HipGradScaler(init_scale=64.0, growth_interval=1000)
        cl.manual_seed(7)
        _hip.seed_salt(0, add=False)
        if graphed:
            gs = GraphedTrainStep(eng, loss_fn, batch, vw, scaler=scaler)
            loss = gs().clone()
        else:
            eng.zero_grad()
            loss = training_step(batch, 0, eng, torch.device("cuda"), vw, loss_fn)
            (loss * scaler.get_scale()).backward()
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
        params = [p.detach().clone() for p in model.parameters()]
        del eng, model
        gc.collect()
        return float(loss), params

    try:
        for graphed in (False, True):
            drawn.clear()
            l_on, p_on = step(True, graphed)
            assert any(0 < int((g == 0).sum()) < g.numel() for g in drawn)
            l_off, p_off = step(False, graphed)
            assert l_on == l_off and l_on == l_on
            assert len(p_on) == len(p_off) > 20
            for a, b in zip(p_on, p_off):
                assert torch.equal(a, b)
    finally:
        _hip.seed_salt(0, add=False)
        _hip.droppath_scales = orig
