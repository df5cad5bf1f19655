"""Patch sizes 1, 2 and 4 of Res_Slim_ViT, the part that needs no GPU: construction against the oracle's state dict, the named
refusals, and the pin of the oracle's patch-size-1 / -4 path against the reference's own model (tests/golden/model_patch*.npz,
written by tests/golden/make_golden_patch.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import orbit2_oracle as O

CONST = ["land_sea_mask", "orography", "lattitude", "landcover"]
IN_VARS = CONST + ["total_precipitation_24hr"]
OUT_VARS = ["total_precipitation_24hr"]
TOL = 2e-5                      # tests/test_oracle_golden.py: prediction / loss bound of the patch-size-2 goldens
TOL_GRAD = 2e-4                 # ... and its bound for the parameter gradients of a whole-model step


def rel(a, b):
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-12))


def _model(p, grid=(16, 32), D=64, **kw):
    from climate_learn.models.hub import Res_Slim_ViT
    return Res_Slim_ViT(IN_VARS, grid, len(IN_VARS), 1, 1, patch_size=p, embed_dim=D, depth=1, decoder_depth=1, num_heads=2,
                        drop_path=0.0, drop_rate=0.0, learn_pos_emb=True, **kw)


@pytest.mark.parametrize("p", [1, 2, 4])
def test_construction_matches_the_oracle_state_dict(p):
    grid, D = (16, 32), 64
    cfg = O.Config(IN_VARS, grid, 1, D, 1, 1, 2, patch_size=p)
    sd = O.init_state_dict(cfg, len(IN_VARS), seed=3)
    m = _model(p, grid, D)
    L = (grid[0] // p) * (grid[1] // p)
    assert m.patch_size == p and m.num_patches == L == sd["pos_embed"].shape[1]
    assert tuple(m.pos_embed.shape) == tuple(sd["pos_embed"].shape) == (1, L, D)
    for i in range(len(IN_VARS)):
        w = m.token_embeds[i].proj.weight
        assert tuple(w.shape) == tuple(sd["token_embeds.%d.proj.weight" % i].shape) == (D, 1, p, p)
    head = m.head[-1].weight
    assert tuple(head.shape) == tuple(sd["head.2.weight"].shape) == (1 * (4 * p) ** 2, D)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.pos_embed.detach(), sd["pos_embed"])


@pytest.mark.parametrize("p", [3, 8, 16])
def test_other_patch_sizes_are_refused_by_name(p):
    with pytest.raises(NotImplementedError, match=r"patch_size=%d.*\(1, 2, 4\)" % p):
        _model(p, (48, 96))


def test_tensor_parallel_and_sharding_refuse_other_patch_sizes_by_name():
    with pytest.raises(NotImplementedError, match="tensor_par_size=2 with patch_size=4"):
        _model(4, tensor_par_size=2, tensor_par_group=object())
    with pytest.raises(NotImplementedError, match="tensor_par_size=2 with patch_size=1"):
        _model(1, tensor_par_size=2, tensor_par_group=object())
    # the parameter-sharding engine marks the parameters it keeps as chunks (`_o2_sharded`): the model refuses its first forward
    m = _model(4)
    m.blocks[0].attn.qkv.weight._o2_sharded = True
    with pytest.raises(NotImplementedError, match="patch_size=4 under the parameter-sharding engine"):
        m(torch.zeros(1, len(IN_VARS), 16, 32), IN_VARS, OUT_VARS)


def test_graph_capture_refuses_other_patch_sizes_by_name():
    from climate_learn.graphs import GraphedTrainStep

    class Engine:
        module = _model(4)

    with pytest.raises(NotImplementedError, match="GraphedTrainStep with patch_size=4"):
        GraphedTrainStep(Engine(), None, (None, None, IN_VARS, OUT_VARS), None)


def test_table_coefficient_count_names_the_patch_size():
    from climate_learn import _hip
    assert [_hip._patch_of(c, "gtab") for c in (2, 5, 17)] == [1, 2, 4]
    for bad in (1, 4, 10, 65):
        with pytest.raises(_hip.HipBackendError, match="coefficients per variable"):
            _hip._patch_of(bad, "gtab")


def test_a_grid_that_is_no_multiple_of_the_patch_is_refused_before_any_launch():
    """host-only: the entries return the bad-argument code for h % patch != 0 without touching their (never valid) pointers"""
    from climate_learn import _hip
    lib = _hip.lib()
    one = 0x10000
    assert lib.orbit2_varagg_fwd_p(one, one, one, one, one, 1, 5, 10, 16, 4, 2, 64, None) == -1
    assert lib.orbit2_varagg_fwd_f32_p(one, one, one, one, None, 1, 5, 8, 18, 4, 2, 64, None) == -1
    assert lib.orbit2_varagg_bwd_p(one, one, one, one, one, one, 1, 5, 10, 16, 4, 2, 64, one, None) == -1
    assert lib.orbit2_varagg_fwd_p(one, one, one, one, one, 1, 5, 8, 16, 3, 2, 64, None) == -1          # patch 3
    assert lib.orbit2_varagg_bwd_p_ws_floats(1, 5, 10, 16, 4, 2, 64) == 0
    assert lib.orbit2_varagg_bwd_p_is_fixed_order(1, 5, 10, 16, 4, 2, 64) == 0
    # the LDS need of the backward at patch 4, V = H = 32: 16 * (32 * 17 + 2 * 32 * 32 + 512) floats = 194 KiB > 160 KiB
    assert lib.orbit2_varagg_bwd_p(one, one, one, one, one, one, 1, 32, 8, 16, 4, 32, 128, one, None) == -3
    assert lib.orbit2_varagg_bwd_p_ws_floats(1, 32, 8, 16, 4, 32, 128) == 0
    assert lib.orbit2_varagg_bwd_p_is_fixed_order(1, 32, 8, 16, 4, 32, 128) == 0
    # a served shape: the path is the fixed-order one, and the workspace is ds + the two slab sets
    assert lib.orbit2_varagg_bwd_p_is_fixed_order(2, 5, 8, 16, 4, 4, 64) == 1
    ntok, C = 2 * 2 * 4, 17
    assert lib.orbit2_varagg_bwd_p_ws_floats(2, 5, 8, 16, 4, 4, 64) == ntok * 4 * 5 + 1 * (4 * 5 * C + 5 * C * 64)
    # patch 2 answers as the entries without the argument do
    for shape in ((2, 23, 16, 32, 4, 256), (2, 7, 12, 20, 3, 384), (2, 5, 8, 16, 4, 64)):
        B, V, h, w, H, D = shape
        assert lib.orbit2_varagg_bwd_p_ws_floats(B, V, h, w, 2, H, D) == lib.orbit2_varagg_bwd_ws_floats(*shape) > 0
        assert lib.orbit2_varagg_bwd_p_is_fixed_order(B, V, h, w, 2, H, D) == lib.orbit2_varagg_bwd_is_fixed_order(*shape)


@pytest.mark.parametrize("tag,p,grid", [("patch1", 1, (4, 8)), ("patch4", 4, (16, 32))])
def test_oracle_matches_the_reference_model_at_this_patch_size(golden_dir, tag, p, grid):
    z = np.load(os.path.join(golden_dir, "model_%s.npz" % tag))
    sd = {k[2:]: torch.from_numpy(z[k]).clone().requires_grad_() for k in z.files if k.startswith("p.")}
    cfg = O.Config(IN_VARS, grid, 1, 64, 1, 1, 2, patch_size=p, spatial_resolution=156.0)
    assert tuple(sd["token_embeds.0.proj.weight"].shape) == (64, 1, p, p)
    x, y = torch.from_numpy(z["x"]), torch.from_numpy(z["y"])
    pred = O.forward(sd, cfg, x, IN_VARS, OUT_VARS)
    e = rel(pred, z["pred"])
    print("[oracle vs reference, patch %d] pred %.2e" % (p, e))
    assert e < TOL
    yhat = O.clip_replace_constant(y, pred, OUT_VARS)
    tgt = O.crop_target(y, yhat)
    vw = {"total_precipitation_24hr": 1.0}
    assert rel(O.bayesian_tv(yhat, tgt, OUT_VARS, vw), z["loss.bayesian_tv"]) < TOL
    O.bayesian_tv(yhat, tgt, OUT_VARS, vw, True).backward()
    n = 0
    for k, v in sd.items():
        gk = "g.bayesian_tv." + k
        if gk in z.files:
            eg = rel(v.grad, z[gk])
            assert eg < TOL_GRAD, (gk, eg)
            n += 1
    assert n > 20 and "g.bayesian_tv.token_embeds.4.proj.weight" in z.files
