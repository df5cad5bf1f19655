"""CPU-side checks of the fp32 forward option: the public switch on Res_Slim_ViT, and the C ABI declarations of the
fp32 entries (construction and the binding need no GPU)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONST = ["land_sea_mask", "orography", "lattitude", "landcover"]
F32_ENTRIES = ("orbit2_gemm_f32", "orbit2_attn_fwd_f32", "orbit2_layernorm_fwd_f32", "orbit2_varagg_fwd_f32",
               "orbit2_unpatchify_fwd_f32")


def _model():
    from climate_learn.models.hub import Res_Slim_ViT
    iv = CONST + ["total_precipitation_24hr"]
    return Res_Slim_ViT(iv, (16, 32), len(iv), 1, 1, patch_size=2, embed_dim=128, depth=1, decoder_depth=1, num_heads=2)


def test_compute_dtype_defaults_to_bf16_and_validates():
    m = _model()
    assert m.compute_dtype is torch.bfloat16
    for bad in (torch.float16, torch.float64, "float32", None):
        with pytest.raises(ValueError, match="compute_dtype"):
            m.set_compute_dtype(bad)
    assert m.compute_dtype is torch.bfloat16                       # a refused value changes nothing
    assert m.set_compute_dtype(torch.float32) is m and m.compute_dtype is torch.float32
    with pytest.raises(AttributeError):
        m.compute_dtype = torch.bfloat16                           # read-only: the setter method is the interface
    m.set_compute_dtype(torch.bfloat16)
    assert m.compute_dtype is torch.bfloat16


def test_compute_dtype_is_not_state_and_survives_rebinding():
    m = _model().set_compute_dtype(torch.float32)
    sd = m.state_dict()
    assert not any("compute" in k for k in sd)
    fresh = _model()
    assert set(sd) == set(fresh.state_dict())                      # the keys of a default model: nothing was added
    m.load_state_dict(fresh.state_dict())
    m.data_config(156.0, (8, 16), 5, 1)
    m.eval()
    m.to("cpu")
    assert m.compute_dtype is torch.float32
    fresh.load_state_dict(sd)                                      # and loading a switched model's weights does not switch
    assert fresh.compute_dtype is torch.bfloat16


def test_fp32_entries_are_declared_in_header_and_binding():
    from climate_learn import _hip
    hdr = open(os.path.join(ROOT, "include", "orbit2_hip.h")).read()
    for name in F32_ENTRIES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name), name
    # the fp32 entries keep the argument lists they were added with; each bf16 entry's list is the fp32 one with the hint
    # parameters (gate, rows_per_gate, sched_ws, tail / gate, sched_ws, tail) inserted in front of the stream
    I, F, U64, P, G = _hip._I, _hip._F, _hip._U64, _hip._P, _hip._G
    gemm_f32, attn_f32 = (I, (G, P)), (I, (P, P, P, I, I, I, I, F, U64, I, I, I, P))
    assert _hip.PROTOTYPES["orbit2_gemm_f32"] == gemm_f32
    assert _hip.PROTOTYPES["orbit2_attn_fwd_f32"] == attn_f32
    assert _hip.PROTOTYPES["orbit2_gemm_bf16"] == (I, gemm_f32[1][:-1] + (P, I, P, I) + gemm_f32[1][-1:])
    assert _hip.PROTOTYPES["orbit2_attn_fwd_ld"] == (I, attn_f32[1][:-1] + (P, P, I) + attn_f32[1][-1:])
    assert _hip.PROTOTYPES["orbit2_layernorm_fwd_f32"] == _hip.PROTOTYPES["orbit2_layernorm_fwd_ld"]
    assert _hip.ABI_VERSION == 8                                   # (the fp32 entries were additive at 7; 8 folded the bf16 entries)


def test_fp32_wrappers_refuse_cpu_and_wrong_dtype():
    from climate_learn import _hip
    a = torch.zeros(8, 8)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.gemm_f32(a, a, a.clone(), 8, 8, 8, 8, 8, 8)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.layernorm_fwd_f32(a, a[0], a[0])
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.attn_fwd_f32(torch.zeros(1, 4, 3 * 64), 1, 4, 1, 64)
    with pytest.raises(_hip.HipBackendError, match="GPU tensor"):
        _hip.unpatchify_fwd_f32(a, 1, 1, 2, 2, 2, 4)
