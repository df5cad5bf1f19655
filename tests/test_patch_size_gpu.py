"""GPU tests of patch sizes 1 and 4 (and of the patch-carrying entries at 2): the folded patch-embed + variable-aggregation
kernels against a dense restatement with the oracle's `patch_embed` / `variable_aggregation` (the pattern of
tests/test_hip_ops.py::test_varagg_fold_matches_dense_oracle), then the whole model, the data-parallel engine, tiled inference
and the two drivers.  Bounds are the project's: the figures of the patch-size-2 tests of the same quantities.  Every test prints
what it measured."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch
import yaml

from oracle import harness
from oracle import orbit2_oracle as O
from tests._child import free_port, run_child

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
TOL_F32 = 2e-5            # tests/test_fp32_ops_gpu.py::test_varagg_fwd_f32_matches_dense_oracle
TOL_MODEL_F32 = 1e-4      # tests/test_fp32_model_gpu.py


@pytest.fixture(scope="module")
def hip():
    from climate_learn import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip


def nerr(a, b):
    a = a.detach().float().cpu().double() if a.dtype != torch.float64 else a.detach().cpu()
    b = b.detach().float().cpu().double() if b.dtype != torch.float64 else b.detach().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def rt(t):
    return t.to(BF).float()


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------
def _tables(sd, heads, ids, D, P):
    """fp32 / fp64 table algebra of the folded variable aggregation (csrc/varagg.hip header) at patch size P: C = P*P + 1"""
    dh = D // heads
    Wq, Wkv = sd["var_agg.q.weight"], sd["var_agg.kv.weight"]
    Wk, Wv = Wkv[:D], Wkv[D:]
    qv = (sd["var_query"].view(1, D) @ Wq.t()).view(D)
    U = torch.stack([(qv[h * dh:(h + 1) * dh, None] * Wk[h * dh:(h + 1) * dh]).sum(0) for h in range(heads)]) * dh ** -0.5
    cm = []
    for v in ids:
        w = sd["token_embeds.%d.proj.weight" % v].view(D, P * P)          # row-major inside the patch
        c = sd["token_embeds.%d.proj.bias" % v] + sd["var_embed"][0, v]
        cm.append(torch.cat([w.t(), c.view(1, D)], 0))                    # [C, D]
    cm = torch.stack(cm)                                                  # [V, C, D]
    return torch.einsum("hd,vcd->hvc", U, cm).contiguous(), torch.einsum("vcd,id->vci", cm, Wv).contiguous()


# (D, heads, V, grid, B, P): a non-square token grid with an odd width (3 x 5), a partial last workgroup (45 tokens =
# 2 x 16 + 13), fewer tokens than one workgroup (8), exactly one workgroup (16), three full ones (48), head dims 16 / 64 / 128
# (16 is outside the MFMA set {64, 128, 256}), V up to 30
KCASES = {
    "p4_16tok_dh16": (64, 4, 5, (8, 16), 2, 4),            # token grid 2 x 4, exactly one workgroup of the forward
    "p4_45tok_dh64": (256, 4, 23, (12, 20), 3, 4),         # token grid 3 x 5 (odd width), 45 tokens: partial last workgroup
    "p4_48tok_dh128": (384, 3, 7, (16, 24), 2, 4),         # token grid 4 x 6, three full workgroups
    "p4_8tok_v30": (256, 2, 30, (8, 16), 1, 4),            # fewer tokens than one workgroup
    "p1_45tok_dh16": (64, 4, 5, (3, 5), 3, 1),             # token grid 3 x 5, 45 tokens
    "p1_64tok_dh64": (256, 4, 23, (4, 8), 2, 1),           # four full workgroups
    "p2_45tok_dh64": (256, 4, 23, (6, 10), 3, 2),          # 45 tokens = 2 x 16 + 13 = 32 + 13: partial last workgroup and MFMA chunk
    "p2_8tok_dh128": (384, 3, 7, (4, 8), 1, 2),            # fewer tokens than one workgroup and than one MFMA chunk
}


@functools.lru_cache(maxsize=None)
def _kcase(name):
    """the seeded case + its dense references, computed once and shared (never modified) by the tests below"""
    D, heads, V, hw, B, P = KCASES[name]
    cfg = O.Config(["v%d" % i for i in range(V + 2)], hw, 1, D, 1, 1, heads, patch_size=P)
    sd = O.init_state_dict(cfg, V, seed=1)
    g = torch.Generator().manual_seed(11)
    for k in ("var_embed", "var_query"):
        sd[k] = torch.randn(sd[k].shape, generator=g) * 0.5
    for k in list(sd):
        if k.startswith("var_agg") or k.startswith("token_embeds"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * (0.3 if "token" in k else 0.15)
    ids = list(range(1, V + 1))
    x = torch.randn(B, V, *hw, generator=g)

    def dense(s, xx, eye, zero):
        toks = [O.patch_embed(xx[:, i:i + 1], s["token_embeds.%d.proj.weight" % v], s["token_embeds.%d.proj.bias" % v], P)
                for i, v in enumerate(ids)]
        t = torch.stack(toks, 1) + s["var_embed"][:, ids].unsqueeze(2)
        return O.variable_aggregation(t, s["var_query"], s["var_agg.q.weight"], s["var_agg.kv.weight"], eye, zero, heads)

    names = [k for k in sd if k.startswith(("var_", "token_embeds"))]
    leaves = {k: sd[k].clone().requires_grad_() for k in names}
    zref = dense(leaves, x, torch.eye(D), torch.zeros(D))               # identity proj exposes z
    L = zref.shape[1]
    assert L == (hw[0] // P) * (hw[1] // P)
    dz = rt(torch.randn(B * L, D, generator=g))
    zref.reshape(B * L, D).backward(dz)
    s64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        zref64 = dense(s64, x.double(), torch.eye(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)).reshape(B * L, D)
        stab64, gtab64 = _tables(s64, heads, ids, D, P)
    return dict(D=D, heads=heads, V=V, hw=hw, B=B, P=P, sd=sd, ids=ids, x=x, names=names, L=L, dz=dz,
                zref=zref.detach().reshape(B * L, D), gref={k: leaves[k].grad for k in names if leaves[k].grad is not None},
                zref64=zref64, stab=stab64.float(), gtab=gtab64.float())


@pytest.mark.parametrize("name", list(KCASES))
def test_forward_matches_dense_oracle(hip, name):
    c = _kcase(name)
    st, gt, x = c["stab"].cuda(), c["gtab"].cuda(), c["x"].cuda()
    z, attw = hip.varagg_fwd(x, st, gt, c["heads"], c["D"])
    z32 = hip.varagg_fwd_f32(x, st, gt, c["heads"], c["D"])                  # attw = NULL
    z32b, attw32 = hip.varagg_fwd_f32(x, st, gt, c["heads"], c["D"], want_attw=True)
    torch.cuda.synchronize()
    ntok = c["B"] * c["L"]
    assert z.shape == (ntok, c["D"]) and z.dtype == BF and attw.shape == (ntok, c["heads"], c["V"])
    e16, e32 = nerr(z, c["zref"]), nerr(z32, c["zref64"])
    print("[patch %d fwd] %s: bf16 %.2e (bound 6e-3), fp32 %.2e (bound %.0e)" % (c["P"], name, e16, e32, TOL_F32))
    assert e16 < 6e-3
    assert z32.dtype == F32 and e32 < TOL_F32
    assert torch.equal(z32, z32b) and torch.equal(attw, attw32)              # with and without attw; the bf16 sibling's weights
    assert nerr(attw.sum(-1), torch.ones(ntok, c["heads"])) < 1e-5           # softmax rows
    assert nerr(z, z32) < 6e-3                                               # the bf16 z is the fp32 one rounded


@pytest.mark.parametrize("name", list(KCASES))
def test_backward_matches_dense_oracle_and_is_reproducible(hip, name):
    """parameter gradients through the tables against autograd of the dense form: normalised max error < 5e-5, the bound of
    tests/test_hip_ops.py::test_varagg_fold_matches_dense_oracle.  The new backward has no float atomics: two calls give the same
    bits, its `is_fixed_order` query says 1, and `_hip.atomics_in_grad_path` is left alone."""
    c = _kcase(name)
    D, heads, V, P, B = c["D"], c["heads"], c["V"], c["P"], c["B"]
    x, gt = c["x"].cuda(), c["gtab"].cuda()
    before = hip.atomics_in_grad_path
    z, attw = hip.varagg_fwd(x, c["stab"].cuda(), gt, heads, D)
    dz = c["dz"].to(BF).cuda()
    dstab, dgtab = hip.varagg_bwd(x, gt, attw, dz, heads, D)
    dstab2, dgtab2 = hip.varagg_bwd(x, gt, attw, dz, heads, D)
    torch.cuda.synchronize()
    assert dstab.shape == (heads, V, P * P + 1) and dgtab.shape == (V, P * P + 1, D)
    assert torch.equal(dstab, dstab2) and torch.equal(dgtab, dgtab2)
    assert hip.lib().orbit2_varagg_bwd_p_is_fixed_order(B, V, c["hw"][0], c["hw"][1], P, heads, D) == 1
    assert hip.atomics_in_grad_path == before
    leaves = {k: c["sd"][k].clone().requires_grad_() for k in c["names"]}
    stab, gtab = _tables(leaves, heads, c["ids"], D, P)
    torch.autograd.backward([stab, gtab], [dstab.cpu(), dgtab.cpu()])
    worst = max((nerr(leaves[k].grad, g), k) for k, g in c["gref"].items())
    print("[patch %d bwd] %s: worst parameter gradient %.2e (%s), bound 5e-5" % (P, name, worst[0], worst[1]))
    assert "token_embeds.1.proj.weight" in c["gref"] and tuple(c["gref"]["token_embeds.1.proj.weight"].shape) == (D, 1, P, P)
    for k, g in c["gref"].items():
        assert nerr(leaves[k].grad, g) < 5e-5, (k, nerr(leaves[k].grad, g))


def _raw(hip, entry, *args):
    """a direct call of a C entry: tensors become device pointers, the current stream is appended"""
    a = [t.data_ptr() if torch.is_tensor(t) else t for t in args]
    rc = getattr(hip.lib(), entry)(*a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("D,heads,V,hw", [(256, 4, 23, (16, 32)), (384, 3, 7, (12, 20))])
def test_patch_two_through_the_new_entries_is_the_old_call(hip, D, heads, V, hw):
    """two shapes of tests/test_hip_ops.py::test_varagg_fold_matches_dense_oracle (both take the fixed-order MFMA backward):
    z, attw, the fp32 z, dstab and dgtab of the patch-carrying entries at patch = 2 equal the old entries' bit for bit"""
    g = torch.Generator().manual_seed(5)
    B, (h, w) = 2, hw
    ntok = B * (h // 2) * (w // 2)
    x = torch.randn(B, V, h, w, generator=g).cuda()
    st = (0.3 * torch.randn(heads, V, 5, generator=g)).cuda()
    gt = (0.2 * torch.randn(V, 5, D, generator=g)).cuda()
    dz = torch.randn(ntok, D, generator=g).to(BF).cuda()
    z0, a0 = hip.varagg_fwd(x, st, gt, heads, D)
    f0 = hip.varagg_fwd_f32(x, st, gt, heads, D)
    ds0, dg0 = hip.varagg_bwd(x, gt, a0, dz, heads, D)
    z1, a1, f1 = torch.zeros_like(z0), torch.zeros_like(a0), torch.zeros_like(f0)
    assert _raw(hip, "orbit2_varagg_fwd_p", x, st, gt, z1, a1, B, V, h, w, 2, heads, D) == 0
    assert _raw(hip, "orbit2_varagg_fwd_f32_p", x, st, gt, f1, None, B, V, h, w, 2, heads, D) == 0
    n = hip.lib().orbit2_varagg_bwd_p_ws_floats(B, V, h, w, 2, heads, D)
    assert n == hip.lib().orbit2_varagg_bwd_ws_floats(B, V, h, w, heads, D) > 0
    assert hip.lib().orbit2_varagg_bwd_p_is_fixed_order(B, V, h, w, 2, heads, D) == 1
    ws = torch.empty(n, dtype=F32, device="cuda")
    ds1, dg1 = torch.zeros_like(ds0), torch.zeros_like(dg0)
    assert _raw(hip, "orbit2_varagg_bwd_p", x, gt, a0, dz, ds1, dg1, B, V, h, w, 2, heads, D, ws) == 0
    for name, a, b in (("z", z0, z1), ("attw", a0, a1), ("z fp32", f0, f1), ("dstab", ds0, ds1), ("dgtab", dg0, dg1)):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("name", ["p4_45tok_dh64", "p1_45tok_dh16", "p2_45tok_dh64"])
def test_outputs_accumulate_and_guard_rows_stay_untouched(hip, name):
    """dstab / dgtab are `+=` (buffers pre-filled with a constant come back as constant + gradient); z, the fp32 z and attw
    allocated with guard rows behind the last token keep them (45 tokens: the last workgroup is partial)"""
    c = _kcase(name)
    D, H, V, P, B, (h, w) = c["D"], c["heads"], c["V"], c["P"], c["B"], c["hw"]
    C, ntok, G = P * P + 1, c["B"] * c["L"], 5
    x, st, gt = c["x"].cuda(), c["stab"].cuda(), c["gtab"].cuda()
    z0, a0 = hip.varagg_fwd(x, st, gt, H, D)
    f0 = hip.varagg_fwd_f32(x, st, gt, H, D)
    z = torch.full((ntok + G, D), -7.0, dtype=BF, device="cuda")
    f = torch.full((ntok + G, D), -7.0, dtype=F32, device="cuda")
    a = torch.full((ntok + G, H, V), -7.0, dtype=F32, device="cuda")
    a2 = a.clone()
    assert _raw(hip, "orbit2_varagg_fwd_p", x, st, gt, z, a, B, V, h, w, P, H, D) == 0
    assert _raw(hip, "orbit2_varagg_fwd_f32_p", x, st, gt, f, a2, B, V, h, w, P, H, D) == 0
    assert torch.equal(z[:ntok], z0) and torch.equal(f[:ntok], f0) and torch.equal(a[:ntok], a0) and torch.equal(a2[:ntok], a0)
    for t in (z, f, a, a2):
        assert bool((t[ntok:] == -7.0).all())
    dz = c["dz"].to(BF).cuda()
    ds0, dg0 = hip.varagg_bwd(x, gt, a0, dz, H, D)
    n = hip.lib().orbit2_varagg_bwd_p_ws_floats(B, V, h, w, P, H, D)
    ws = torch.full((n + 64,), -7.0, dtype=F32, device="cuda")
    ds = torch.full((H, V, C), 0.5, dtype=F32, device="cuda")
    dg = torch.full((V, C, D), 0.5, dtype=F32, device="cuda")
    assert _raw(hip, "orbit2_varagg_bwd_p", x, gt, a0, dz, ds, dg, B, V, h, w, P, H, D, ws) == 0
    assert torch.equal(ds, ds0 + 0.5) and torch.equal(dg, dg0 + 0.5)
    assert bool((ws[n:] == -7.0).all())                                      # nothing written behind the queried workspace


def test_bad_arguments_are_refused_before_any_launch(hip):
    """a grid that is no multiple of the patch size (-1) and an LDS need over a CU's 160 KiB (-3: the backward at patch 4 with
    V = H = 32 needs 16 * (32 * 17 + 2 * 32 * 32 + 512) * 4 B = 194 KiB): the error code comes back and every output keeps its fill"""
    B, V, H, D, P = 1, 32, 32, 128, 4
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, V, 12, 16, generator=g).cuda()
    st = torch.randn(H, V, 17, generator=g).cuda()
    gt = torch.randn(V, 17, D, generator=g).cuda()
    ntok = 3 * 4
    z = torch.full((ntok, D), 3.0, dtype=BF, device="cuda")
    f = torch.full((ntok, D), 3.0, dtype=F32, device="cuda")
    a = torch.full((ntok, H, V), 3.0, dtype=F32, device="cuda")
    dz = torch.ones(ntok, D, dtype=BF, device="cuda")
    ds = torch.full((H, V, 17), 3.0, dtype=F32, device="cuda")
    dg = torch.full((V, 17, D), 3.0, dtype=F32, device="cuda")
    ws = torch.full((1 << 20,), 3.0, dtype=F32, device="cuda")
    for (h, w) in ((10, 16), (12, 18)):                                      # not multiples of 4
        assert _raw(hip, "orbit2_varagg_fwd_p", x, st, gt, z, a, B, V, h, w, P, H, D) == -1
        assert _raw(hip, "orbit2_varagg_fwd_f32_p", x, st, gt, f, a, B, V, h, w, P, H, D) == -1
        assert _raw(hip, "orbit2_varagg_bwd_p", x, gt, a, dz, ds, dg, B, V, h, w, P, H, D, ws) == -1
    assert _raw(hip, "orbit2_varagg_fwd_p", x, st, gt, z, a, B, V, 12, 16, 8, H, D) == -1          # patch 8
    assert _raw(hip, "orbit2_varagg_bwd_p", x, gt, a, dz, ds, dg, B, V, 12, 16, P, H, D, ws) == -3  # LDS over the limit
    assert hip.lib().orbit2_varagg_bwd_p_ws_floats(B, V, 12, 16, P, H, D) == 0
    assert hip.lib().orbit2_varagg_bwd_p_is_fixed_order(B, V, 12, 16, P, H, D) == 0
    for t in (z, f, a, ds, dg, ws):
        assert bool((t == 3.0).all())
    with pytest.raises(hip.HipBackendError, match="not a multiple of the patch size 4"):
        hip.varagg_fwd(x[:, :, :10].contiguous(), st, gt, H, D)
    with pytest.raises(hip.HipBackendError, match="LDS"):
        hip.varagg_bwd(x, gt, a, dz, H, D)
    with pytest.raises(hip.HipBackendError, match="coefficients per variable"):
        hip.varagg_fwd(x, st[:, :, :10].contiguous(), gt[:, :10].contiguous(), H, D)
    # the forward at this shape is served (16 * (32 * 17 + 32 * 32) * 4 B = 98 KiB)
    assert _raw(hip, "orbit2_varagg_fwd_p", x, st, gt, z, a, B, V, 12, 16, P, H, D) == 0
    assert nerr(a.sum(-1), torch.ones(ntok, H)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# model level (harness.build_pair fixes patch size 2: the pair is built here)
# ---------------------------------------------------------------------------------------------------------------------
CONST = ["land_sea_mask", "orography", "lattitude", "landcover"]
IN_VARS, OUT_VARS = CONST + ["total_precipitation_24hr"], ["total_precipitation_24hr"]
MGRID = {1: (4, 8), 4: (16, 32)}
VW = {"total_precipitation_24hr": 1.0}


def _pair(p, grid=None, B=2, D=128, seed=0):
    from climate_learn.models.hub import Res_Slim_ViT
    grid = grid or MGRID[p]
    cfg = O.Config(IN_VARS, grid, 1, D, 1, 1, 2, patch_size=p, spatial_resolution=156.0)
    sd = O.init_state_dict(cfg, len(IN_VARS), seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in ("var_embed", "var_query"):
        sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
    for k in sd:
        if k.endswith(".bias") and "norm" not in k:
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    x = torch.randn(B, len(IN_VARS), *grid, generator=g)
    y = torch.randn(B, 1, grid[0] * 4 + 1, grid[1] * 4 + 3, generator=g)
    y[:, 0] = torch.log1p(torch.relu(y[:, 0]))
    model = Res_Slim_ViT(IN_VARS, grid, len(IN_VARS), 1, 1, patch_size=p, embed_dim=D, depth=1, decoder_depth=1, num_heads=2,
                         drop_path=0.0, drop_rate=0.0, learn_pos_emb=True)
    model.load_state_dict(sd, strict=True)
    model.data_config(156.0, grid, len(IN_VARS), 1)
    return model, sd, cfg, x, y


@pytest.mark.parametrize("p", [1, 4])
def test_fp32_forward_vs_cpu_oracle(p):
    model, sd, cfg, x, y = _pair(p)
    model = model.cuda().eval()
    with torch.no_grad():
        ref = O.forward(sd, cfg, x, IN_VARS, OUT_VARS)
        bf = model(x.cuda(), IN_VARS, OUT_VARS)
        pred = model.set_compute_dtype(F32)(x.cuda(), IN_VARS, OUT_VARS)
    e32, e16 = nerr(pred, ref), nerr(bf, ref)
    print("[patch %d model] fp32 forward %.2e (bound %.0e; bf16 path %.2e)" % (p, e32, TOL_MODEL_F32, e16))
    assert pred.dtype == F32 and tuple(pred.shape) == tuple(ref.shape) and e32 <= TOL_MODEL_F32 and e32 < e16


@pytest.mark.parametrize("p", [1, 4])
def test_training_step_vs_cpu_oracle(p):
    """bf16 forward + one bayesian_tv step: the prediction, the loss and EVERY parameter gradient against the oracle; per tensor
    `harness.grad_tolerance` of the oracle's own bf16-vs-fp32 movement (`harness.oracle_bf16_spread`; no reference fixture
    exists for these cases), and the whole gradient's relative L2 as the patch-size-2 model tests bound it"""
    from climate_learn.metrics import Bayesian_TV
    from climate_learn.trainer import training_step
    model, sd, cfg, x, y = _pair(p)
    dev = torch.device("cuda:0")
    model = model.to(dev).eval()
    with torch.no_grad():
        pred = model(x.cuda(), IN_VARS, OUT_VARS)
    loss = training_step((x, y, IN_VARS, OUT_VARS), 0, model, dev, VW, Bayesian_TV(aggregate_only=True))
    loss.backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ref = O.training_loss(sdo, cfg, x, y, IN_VARS, OUT_VARS, "bayesian_tv", VW)
    ref.backward()
    with torch.no_grad():
        e_pred = nerr(pred, O.forward(sd, cfg, x, IN_VARS, OUT_VARS))
    e_loss = abs(float(loss) - float(ref)) / abs(float(ref))
    print("[patch %d model] bf16 prediction %.2e, loss %.2e (bounds 2e-2)" % (p, e_pred, e_loss))
    assert e_pred < 2e-2 and e_loss < 2e-2
    g32 = {k: v.grad.detach() for k, v in sdo.items() if v.grad is not None}
    spread = harness.oracle_bf16_spread(O, sd, cfg, x, y, IN_VARS, OUT_VARS, "bayesian_tv", VW, fp32_grads=g32)
    prm = dict(model.named_parameters())
    names = [n for n in prm if prm[n].grad is not None and n in g32]
    assert set(names) == set(g32) and len(names) > 25
    w = prm["token_embeds.4.proj.weight"]
    assert tuple(w.shape) == tuple(w.grad.shape) == (128, 1, p, p)
    bad = {}
    for n in names:
        e, tol = nerr(prm[n].grad, g32[n]), harness.grad_tolerance(spread[n], n)
        l2 = float((prm[n].grad.detach().cpu().double() - g32[n].double()).norm() / g32[n].double().norm().clamp_min(1e-30))
        tol2 = harness.grad_tolerance(spread["l2." + n])
        if e > tol or l2 > tol2:
            bad[n] = (e, tol, l2, tol2)
    worst = max((nerr(prm[n].grad, g32[n]), n) for n in names)
    e_all = harness.whole_gradient_rel_l2((prm[n].grad, g32[n]) for n in names)
    sp_all = harness.whole_gradient_spread({n: spread["l2." + n] for n in names}, g32)
    t_all = max(harness.TOL_FLOOR, harness.TOL_FACTOR * sp_all)
    print("[patch %d model] worst gradient %.2e (%s); whole gradient rel. L2 %.2e (oracle bf16 spread %.2e, bound %.2e)"
          % (p, worst[0], worst[1], e_all, sp_all, t_all))
    assert not bad, bad
    assert e_all <= t_all


def test_data_parallel_engine_at_patch_four():
    run_child(__file__, "child_data_parallel_engine_at_patch_four")


def child_data_parallel_engine_at_patch_four():
    """one HipDataParallel step at patch size 4 on a single rank with the collectives forced on (tests/test_dp_gpu.py's way): the
    table parameters take the ATen path (`_token_tables_layout` is not consulted), their gradients accumulate through autograd
    into the engine's buckets, and every gradient equals the plain model's"""
    import torch.distributed as dist
    import torch.nn as nn
    import climate_learn as cl
    from climate_learn.metrics import Bayesian_TV
    from climate_learn.models.hub.components.vit_blocks import Block
    from climate_learn.trainer import training_step
    os.environ.update(ORBIT2_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        plain, sd, cfg, x, y = _pair(4)
        managed = _pair(4)[0]
        plain, managed = plain.cuda().eval(), managed.cuda().eval()
        eng = cl.HipDataParallel(managed, unit_types=(Block, nn.Sequential))
        lossf = Bayesian_TV(aggregate_only=True)
        batch = (x, y, IN_VARS, OUT_VARS)
        eng.zero_grad()
        lm = training_step(batch, 0, eng, torch.device("cuda"), VW, lossf)
        assert managed.__dict__.get("_tables_pending", [0])[0] == 0          # the fused gather / scatter node was not used
        lm.backward()
        eng.finish_grad_sync()
        lp = training_step(batch, 0, plain, torch.device("cuda"), VW, lossf)
        lp.backward()
        torch.cuda.synchronize()
        assert float(lm) == float(lp)
        gm, gp = dict(managed.named_parameters()), dict(plain.named_parameters())
        n_eq = 0
        for n, q in gp.items():
            if q.grad is None:
                continue
            a = gm[n]._o2g if hasattr(gm[n], "_o2g") else gm[n].grad
            assert a is not None, n
            if a.dtype == q.grad.dtype:
                assert torch.equal(a, q.grad), (n, float((a - q.grad).abs().max()))
                n_eq += 1
            else:      # a bf16 gradient bucket: the plain fp32 gradient rounded once (half an ulp = 2^-9 per element at most)
                l2 = float((a.float() - q.grad.float()).norm() / q.grad.float().norm().clamp_min(1e-30))
                assert l2 <= 2.0 ** -9, (n, l2)
        names = [n for n in gp if n.startswith("token_embeds.") or n == "var_embed"]
        assert len(names) == 2 * len(IN_VARS) + 1 and all(gm[n].grad.dtype == F32 and torch.equal(gm[n].grad, gp[n].grad)
                                                           for n in names)
        print("[patch 4 engine] %d gradients bit-identical to the plain model's" % n_eq)
    finally:
        if created:
            dist.destroy_process_group()


def test_tiled_predict_at_patch_four():
    """2 x 2 tiles with overlap 2 of a 28 x 56 field: every tile is 16 x 32 with its halo, a multiple of 4.  The stitched fp32
    prediction against the oracle's forward of each tile placed with the same windows, at the tolerance of the patch-size-2 test
    of the same thing (tests/test_fp32_model_gpu.py::test_fp32_tiled_predict_vs_oracle_stitch); the bf16 stitch equals the
    per-tile bf16 forwards bit for bit; overlap 4 makes 18 x 36 tiles, refused by name"""
    from climate_learn.trainer import clip_replace_constant
    from climate_learn.utils.visualize import tile_windows, tiled_predict
    model, sd, cfg, x, y = _pair(4, B=1, seed=7)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(2)
    X = torch.randn(1, len(IN_VARS), 28, 56, generator=g)
    Y = torch.randn(1, 1, 112, 224, generator=g)
    div, ov = 2, 2
    wins = tile_windows(28, 56, 112, 224, div, ov)
    assert all((t["inp"][0][1] - t["inp"][0][0], t["inp"][1][1] - t["inp"][1][0]) == (16, 32) for t in wins)
    st16 = tiled_predict(model, X.cuda(), Y.cuda(), IN_VARS, OUT_VARS, div, ov)
    st32 = tiled_predict(model.set_compute_dtype(F32), X.cuda(), Y.cuda(), IN_VARS, OUT_VARS, div, ov)
    model.set_compute_dtype(BF)
    assert st32.shape == (1, 1, 112, 224) and tuple(model.img_size) == (16, 32)
    ref = torch.zeros(1, 1, 112, 224)
    with torch.no_grad():
        for t in wins:
            (yi1, yi2), (xi1, xi2) = t["inp"]
            (yo1, yo2), (xo1, xo2) = t["out"]
            (ya, yb), (xa, xb) = t["crop_out"]
            (ra, rb), (ca, cb) = t["place_out"]
            xt = X[:, :, yi1:yi2, xi1:xi2].contiguous()
            pr = O.clip_replace_constant(Y[:, :, yo1:yo2, xo1:xo2], O.forward(sd, cfg, xt, IN_VARS, OUT_VARS), OUT_VARS)
            ref[:, :, ra:rb, ca:cb] = pr[:, :, ya:yb, xa:xb]
            p16 = clip_replace_constant(Y[:, :, yo1:yo2, xo1:xo2].cuda(), model(xt.cuda(), IN_VARS, OUT_VARS), OUT_VARS)
            assert torch.equal(st16[:, :, ra:rb, ca:cb], p16[:, :, ya:yb, xa:xb].float())
    e = nerr(st32, ref)
    print("[patch 4 model] tiled_predict 2 x 2, overlap 2 vs oracle stitch: %.2e (bound %.0e)" % (e, TOL_MODEL_F32))
    assert e <= TOL_MODEL_F32
    with pytest.raises(ValueError, match=r"18 x 36 .*not a multiple of patch_size=4"):
        tiled_predict(model, X.cuda(), Y.cuda(), IN_VARS, OUT_VARS, 2, 4)
    assert tuple(model.img_size) == (16, 32)
    with pytest.raises(ValueError, match="not a multiple of patch_size=4"):
        model.data_config(156.0, (18, 36), len(IN_VARS), 1)
        model(torch.zeros(1, len(IN_VARS), 18, 36, device="cuda"), IN_VARS, OUT_VARS)


def test_parameter_sharding_engine_refuses_patch_four_by_name():
    import torch.nn as nn
    import climate_learn as cl
    from climate_learn.models.hub.components.vit_blocks import Block
    model, sd, cfg, x, y = _pair(4)
    fs = cl.HipFullyShardedDataParallel(model.cuda().eval(), unit_types=(Block, nn.Sequential))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="patch_size=4 under the parameter-sharding engine"):
        fs.module(x.cuda(), IN_VARS, OUT_VARS)


# ---------------------------------------------------------------------------------------------------------------------
# drivers (modelled on tests/test_drivers_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def _run(script, cfg, cwd):
    env = dict(os.environ, MASTER_PORT=str(free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), cfg], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_training_driver_at_patch_four(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "interm_8m.yaml")))
    conf["trainer"].update(max_epochs=2, batch_size=2)
    conf["model"].update(depth=1, decoder_depth=1, warmup_epochs=1, patch_size=4)
    conf["data"]["synthetic"]["ERA5_1"].update(steps_per_epoch=2)
    cfg = os.path.join(tmp_path, "p4.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("intermediate_downscaling.py", cfg, tmp_path)
    losses = [float(m) for m in re.findall(r"world_rank 0  loss  ([0-9.eE+-]+)", out)]
    assert len(losses) == 4 and all(l == l and 0 < l < 1e4 for l in losses)
    ck = torch.load(os.path.join(tmp_path, "checkpoints", "climate", "interm_epoch_1.ckpt"), map_location="cpu")
    assert tuple(ck["model_state_dict"]["token_embeds.0.proj.weight"].shape) == (256, 1, 4, 4)
    assert ck["model_state_dict"]["pos_embed"].shape[1] == (32 // 4) * (64 // 4)


def test_inference_driver_at_patch_four(tmp_path):
    conf = yaml.safe_load(open(os.path.join(ROOT, "configs", "inference.yaml")))
    conf["model"].update(embed_dim=256, depth=1, decoder_depth=1, num_heads=4, patch_size=4)
    conf["data"]["synthetic"]["ERA5_1"].update(lowres_hw=[32, 64], highres_hw=[128, 256])      # 2 x 2 tiles of 20 x 40 with the halo
    cfg = os.path.join(tmp_path, "inf4.yaml")
    yaml.safe_dump(conf, open(cfg, "w"))
    out = _run("visualize.py", cfg, tmp_path)
    assert "stitched" in out and "(128, 256)" in out
    for name in ("rmse", "pearson", "mean_bias"):
        m = re.search(name + r" \[([^\]]+)\]", out)
        assert m, out[-1500:]
        vals = [float(v) for v in m.group(1).split(",")]
        assert len(vals) == 4 and all(v == v for v in vals)          # 3 channels + aggregate, finite
