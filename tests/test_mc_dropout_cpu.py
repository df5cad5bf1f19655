"""CPU-side checks of MC-dropout mode: which dropout sites the mode wakes (decided on the host, no device needed), how the
mode is entered and left, what it refuses, and the C ABI declarations of the two new entries."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONST = ["land_sea_mask", "orography", "lattitude", "landcover"]
P, P_PATH = 0.3, 0.5


def _model(backend="HIP", depth=2):
    from climate_learn.models.hub import Res_Slim_ViT
    from climate_learn.utils.fused_attn import FusedAttn
    iv = CONST + ["total_precipitation_24hr"]
    m = Res_Slim_ViT(iv, (16, 32), len(iv), 1, 1, patch_size=2, embed_dim=128, depth=depth, decoder_depth=1, num_heads=2,
                     drop_rate=P, drop_path=P_PATH, FusedAttn_option=FusedAttn[backend])
    for blk in m.blocks:
        blk.drop_path = P_PATH                  # (the constructor ramps it up from 0 at the first block)
    return m


def _sites(m):
    """the host-side probabilities of the model: (pos_drop, per-block dictionaries)"""
    return m.pos_p(), [blk.dropout_probs() for blk in m.blocks]


# the issue's table: (element dropouts, DropPath, attention-probability dropout) in eval / MC / train mode per backend
ELEMENT = {"eval": 0.0, "mc": P, "train": P}
DROPPATH = {"eval": 0.0, "mc": 0.0, "train": P_PATH}
ATTN = {"CK": {"eval": P, "mc": P, "train": P}, "NONE": {"eval": 0.0, "mc": P, "train": P},
        "DEFAULT": {"eval": 0.0, "mc": 0.0, "train": P}, "HIP": {"eval": 0.0, "mc": P, "train": P}}


@pytest.mark.parametrize("backend", ["HIP", "CK", "DEFAULT", "NONE"])
def test_site_table_per_backend(backend):
    from climate_learn.utils import enable_dropout
    m = _model(backend)
    for mode in ("eval", "mc", "train", "eval"):
        if mode == "train":
            m.train()
        else:
            m.eval()
            if mode == "mc":
                enable_dropout(m)
        pos, blocks = _sites(m)
        assert pos == ELEMENT[mode], (backend, mode)
        for d in blocks:
            assert d["proj_drop"] == ELEMENT[mode] and d["mlp_drop"] == ELEMENT[mode], (backend, mode, d)
            assert d["drop_path"] == DROPPATH[mode], (backend, mode, d)
            assert d["attn_drop"] == ATTN[backend][mode], (backend, mode, d)
        for blk in m.blocks:                    # the stand-alone modules decide the same way as the fused Block
            assert blk.attn.attn_p() == ATTN[backend][mode] and blk.attn.proj_p() == ELEMENT[mode]
            assert blk.mlp.drop_p() == ELEMENT[mode]


def test_mode_is_left_by_train_and_eval_and_never_entered_unasked():
    from climate_learn.models.hub.components.mlp import McDropoutMode
    from climate_learn.utils import enable_dropout
    m = _model()
    flagged = [x for x in m.modules() if isinstance(x, McDropoutMode)]
    assert len(flagged) == 1 + 3 * len(m.blocks)                  # the model, and Block + Attention + Mlp per block
    for call in (lambda: m.eval(), lambda: m.train(), lambda: m.train(False), lambda: m.blocks[0].eval()):
        m.eval()
        assert not any(x.mc_dropout for x in flagged)
        enable_dropout(m)
        assert all(x.mc_dropout for x in flagged) and not m.training
        call()
        left = [x for x in flagged if not x.mc_dropout]
        assert m.blocks[0] in left and m.blocks[0].attn in left and m.blocks[0].mlp in left
    m.eval()
    assert _sites(m) == (0.0, [dict(attn_drop=0.0, proj_drop=0.0, mlp_drop=0.0, drop_path=0.0)] * len(m.blocks))
    assert "mc_dropout" not in "".join(m.state_dict())            # a mode, not state


def test_enable_dropout_on_components_and_inside_a_wrapper():
    from climate_learn.utils import enable_dropout
    from climate_learn.utils.mc_dropout import enable_dropout as same
    import climate_learn.utils as U
    assert same is enable_dropout and U.get_monte_carlo_predictions and U.mc_dropout_statistics

    class Wrapper(nn.Module):                                       # the nn.Module surface of HipDataParallel: `.module`
        def __init__(self, module):
            super().__init__()
            self.module = module

    m = _model()
    w = Wrapper(m).eval()
    enable_dropout(w)
    assert m.mc_dropout and m.pos_p() == P and m.blocks[1].dropout_probs()["mlp_drop"] == P
    w.eval()                                                        # the wrapper's eval() reaches the model
    assert not m.mc_dropout and m.pos_p() == 0.0
    blk = _model().blocks[0].eval()
    enable_dropout(blk)
    assert blk.dropout_probs() == dict(attn_drop=P, proj_drop=P, mlp_drop=P, drop_path=0.0)
    attn, mlp = _model().blocks[0].attn.eval(), _model().blocks[0].mlp.eval()
    enable_dropout(attn)
    enable_dropout(mlp)
    assert (attn.attn_p(), attn.proj_p(), mlp.drop_p()) == (P, P, P)
    with pytest.raises(TypeError, match="no module that decides a dropout probability"):
        enable_dropout(nn.Linear(4, 4))


def test_fp32_compute_with_mc_mode_is_refused_by_name():
    from climate_learn import _fp32
    from climate_learn.utils import enable_dropout
    m = _model().eval().set_compute_dtype(torch.float32)
    for p in m.parameters():
        p.requires_grad_(False)
    _fp32.refuse(m)                                                 # plain eval: served
    enable_dropout(m)
    with pytest.raises(RuntimeError, match="MC dropout is built for the bf16 path"):
        _fp32.refuse(m)
    m.eval()
    _fp32.refuse(m)


def test_tensor_parallel_and_sharded_models_are_refused_by_name():
    from climate_learn.utils import enable_dropout
    m = _model().eval()
    m.blocks[0].attn.tensor_par_size = 2
    with pytest.raises(RuntimeError, match="MC dropout is not built for tensor parallelism"):
        enable_dropout(m)
    assert not m.mc_dropout
    m.blocks[0].attn.tensor_par_size = 1
    m.norm.weight._o2_sharded = True
    with pytest.raises(RuntimeError, match="MC dropout is not built for the parameter-sharding engine"):
        enable_dropout(m)
    assert not any(getattr(x, "mc_dropout", False) for x in m.modules())


def test_statistics_need_two_members_and_scores_need_a_normal():
    from climate_learn.metrics.functional import gaussian_crps, gaussian_spread
    from climate_learn.utils import mc_dropout_statistics
    for n in (0, 1):
        with pytest.raises(ValueError, match="at least 2 ensemble members"):
            mc_dropout_statistics((None, None, [], []), _model(), n)
    with pytest.raises(TypeError, match="torch.distributions.Normal"):
        gaussian_spread(torch.zeros(1, 1, 4, 4))
    with pytest.raises(TypeError, match="torch.distributions.Normal"):
        gaussian_crps(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_new_entries_are_declared_in_header_binding_and_library():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    for name in ("orbit2_ensemble_update", "orbit2_gaussian_scores"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name), name
    I, I64, P_ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _hip.PROTOTYPES["orbit2_ensemble_update"] == (I, (P_, P_, P_, I64, I, P_))
    assert _hip.PROTOTYPES["orbit2_gaussian_scores"] == (I, (P_, P_, P_, I, I, P_, P_, I, I, I, I, P_))
    assert _hip.ABI_VERSION == 8                                   # (additive at 7; 8 folded the gated and queued bf16 entries)


def test_new_entries_refuse_bad_arguments_before_any_launch():
    """host-side argument checks only (no device is touched: every call returns before a launch)"""
    from climate_learn import _hip
    lib = _hip.lib()
    a, b, c, d = 0x10000, 0x20000, 0x30000, 0x40000               # never dereferenced
    assert lib.orbit2_ensemble_update(None, b, c, 16, 1, None) == -1
    assert lib.orbit2_ensemble_update(a, None, c, 16, 1, None) == -1
    assert lib.orbit2_ensemble_update(a, b, None, 16, 1, None) == -1
    assert lib.orbit2_ensemble_update(a, b, c, 0, 1, None) == -1
    assert lib.orbit2_ensemble_update(a, b, c, 16, 0, None) == -1
    assert lib.orbit2_ensemble_update(a, b, b, 16, 2, None) == -1   # aliased running buffers
    assert lib.orbit2_gaussian_scores(None, b, c, 8, 8, None, d, 1, 1, 8, 8, None) == -1
    assert lib.orbit2_gaussian_scores(a, None, c, 8, 8, None, d, 1, 1, 8, 8, None) == -1
    assert lib.orbit2_gaussian_scores(a, b, None, 8, 8, None, d, 1, 1, 8, 8, None) == -1
    assert lib.orbit2_gaussian_scores(a, b, c, 8, 8, None, None, 1, 1, 8, 8, None) == -1
    assert lib.orbit2_gaussian_scores(a, b, c, 7, 8, None, d, 1, 1, 8, 8, None) == -1      # target smaller than the prediction
    assert lib.orbit2_gaussian_scores(a, b, c, 8, 7, None, d, 1, 1, 8, 8, None) == -1
    assert lib.orbit2_gaussian_scores(a, b, c, 8, 8, None, d, 0, 1, 8, 8, None) == -1
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.gaussian_scores(x, x, x)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.ensemble_update(x, x.clone(), x.clone(), 1)
