"""ctypes binding of liborbit2_hip.so (C ABI in include/orbit2_hip.h).

This is the ONLY compute backend of the package: there is no CPU or eager fallback.  Every wrapper
checks that its operands are contiguous device tensors of the expected dtype and passes raw device
pointers plus torch's current HIP stream across the ABI.  A missing library or a non-zero return
code raises immediately."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# $ORBIT2_HIP_LIB: another build of the same ABI (A/B timing of kernel variants on one box; tools/ab_build.sh)
LIB_PATH = os.environ.get("ORBIT2_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "liborbit2_hip.so")
_lib = None
ABI_VERSION = 8                 # ORBIT2_ABI_VERSION: load() refuses a build of any other version


class HipBackendError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int),
        ("a_kc", C.c_int), ("b_kc", C.c_int),
        ("bias", C.c_void_p),
        ("act", C.c_int),
        ("save_pre", C.c_void_p),
        ("dgelu_pre", C.c_void_p),
        ("drop_p", C.c_float),
        ("seed", C.c_uint64),
        ("rowscale", C.c_void_p),
        ("rows_per_scale", C.c_int),
        ("residual", C.c_void_p),
        ("ldr", C.c_int), ("res_mod", C.c_int), ("res_first", C.c_int),
        ("out_fp32", C.c_int),
        ("beta", C.c_float),
        ("tile_hint", C.c_int),
        ("colscale_n", C.c_int),
        ("colscale", C.c_float),
        ("save_dact", C.c_void_p),
        ("mul", C.c_void_p),
        ("colsum_ws", C.c_void_p),
    ]


# Every prototype of include/orbit2_hip.h: name -> (restype, argtypes).  The header has five parameter kinds: int, int64_t,
# uint64_t, float and pointers, which are all void* to ctypes except the GEMM's argument block.  With these declared, ctypes
# refuses a call with too few arguments or an argument of the wrong kind before it reaches the library.
_I, _I64, _U64, _F, _P, _G = C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_void_p, C.POINTER(GemmArgs)
PROTOTYPES = {
    "orbit2_abi_version": (_I, ()),
    "orbit2_gemm_bf16": (_I, (_G, _P, _I, _P, _I, _P)),
    "orbit2_gemm_bf16_colsum_rows": (_I, (_G,)),
    "orbit2_gemm_f32": (_I, (_G, _P)),
    "orbit2_gemm_bf16_grouped": (_I, (_G, _I, _P, _P, _P, _I, _P)),
    "orbit2_sgemm_f32_ws_floats": (_I64, (_I, _I, _I)),
    "orbit2_sgemm_f32_ws": (_I, (_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _P, _I64, _P)),
    "orbit2_layernorm_fwd_ld": (_I, (_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P)),
    "orbit2_layernorm_fwd_f32": (_I, (_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P)),
    "orbit2_layernorm_bwd": (_I, (_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _P)),
    "orbit2_layernorm_bwd_ws_floats": (_I, (_I, _I)),
    "orbit2_attn_bwd_ws_floats": (_I64, (_I, _I, _I)),
    "orbit2_attn_fwd_ld": (_I, (_P, _P, _P, _I, _I, _I, _I, _F, _U64, _I, _I, _I, _P, _P, _I, _P)),
    "orbit2_attn_fwd_f32": (_I, (_P, _P, _P, _I, _I, _I, _I, _F, _U64, _I, _I, _I, _P)),
    "orbit2_attn_bwd_ld": (_I, (_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _U64, _I, _I, _I, _P, _P, _I, _P)),
    "orbit2_varagg_fwd": (_I, (_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_varagg_fwd_f32": (_I, (_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_varagg_bwd_ws_floats": (_I64, (_I, _I, _I, _I, _I, _I)),
    "orbit2_varagg_bwd": (_I, (_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P)),
    "orbit2_tables_gather": (_I, (_P, _I64, _P, _I64, _P, _P, _P, _I, _I, _P)),
    "orbit2_tables_scatter": (_I, (_P, _P, _I64, _P, _I64, _P, _P, _I, _I, _P)),
    "orbit2_varagg_bwd_is_fixed_order": (_I, (_I, _I, _I, _I, _I, _I)),
    "orbit2_varagg_fwd_p": (_I, (_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_varagg_fwd_f32_p": (_I, (_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_varagg_bwd_p_ws_floats": (_I64, (_I, _I, _I, _I, _I, _I, _I)),
    "orbit2_varagg_bwd_p": (_I, (_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P)),
    "orbit2_varagg_bwd_p_is_fixed_order": (_I, (_I, _I, _I, _I, _I, _I, _I)),
    "orbit2_dropout_bwd": (_I, (_P, _P, _I, _I, _F, _U64, _P, _I, _P)),
    "orbit2_dropout_bwd_colsum": (_I, (_P, _P, _I, _I, _F, _U64, _P, _I, _P, _I, _F, _P, _I, _P)),
    "orbit2_post_reduce": (_I, (_P, _P, _I, _P, _P, _I, _I, _F, _U64, _P, _I, _P)),
    "orbit2_colsum": (_I, (_P, _I, _I, _I, _I, _P, _I, _F, _P, _I, _P)),
    "orbit2_colsum_ws_floats": (_I, (_I, _I)),
    "orbit2_batch_sum": (_I, (_P, _P, _I, _I, _I, _I, _F, _P)),
    "orbit2_droppath_scales": (_I, (_P, _I, _F, _U64, _P)),
    "orbit2_transpose_bf16": (_I, (_P, _P, _I, _I, _P)),
    "orbit2_cast_f32_to_bf16": (_I, (_P, _P, _I64, _P)),
    "orbit2_cast_bf16_to_f32": (_I, (_P, _P, _I64, _P)),
    "orbit2_add_rowvec": (_I, (_P, _P, _P, _I, _I, _P)),
    "orbit2_posembed_fwd": (_I, (_P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P)),
    "orbit2_posembed_bwd": (_I, (_P, _P, _I, _I, _I, _I, _I, _P)),
    "orbit2_unpatchify_fwd": (_I, (_P, _P, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_unpatchify_fwd_f32": (_I, (_P, _P, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_unpatchify_bwd": (_I, (_P, _P, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_conv3x3_fwd": (_I, (_P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_conv3x3_bwd_ws_floats": (_I64, (_I, _I, _I, _I, _I)),
    "orbit2_conv3x3_bwd": (_I, (_P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P)),
    "orbit2_clamp_channel": (_I, (_P, _I, _I, _I, _I, _P)),
    "orbit2_clamp_channel_bwd": (_I, (_P, _P, _I, _I, _I, _I, _P)),
    "orbit2_loss_fwd": (_I, (_P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P)),
    "orbit2_loss_bwd": (_I, (_P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P)),
    "orbit2_eval_moments": (_I, (_P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _P)),
    "orbit2_masked_loss_fwd": (_I, (_P, _P, _I, _I, _P, _I, _I64, _I64, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P)),
    "orbit2_masked_loss_bwd": (_I, (_P, _P, _I, _I, _P, _I, _I64, _I64, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P)),
    "orbit2_masked_moments": (_I, (_P, _P, _I, _I, _P, _I, _I64, _I64, _P, _P, _P, _I, _I, _I, _I, _P)),
    "orbit2_ensemble_update": (_I, (_P, _P, _P, _I64, _I, _P)),
    "orbit2_gaussian_scores": (_I, (_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _P)),
    "orbit2_ensemble_scores": (_I, (_P, _I64, _I, _P, _I, _I, _P, _P, _P, _I, _P, _U64, _P, _P, _I, _I, _I, _I, _I, _P)),
    "orbit2_ssim": (_I, (_P, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P)),
    "orbit2_resample_fwd": (_I, (_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_resample_moments": (_I, (_P, _P, _I, _P, _P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P)),
    "orbit2_im2col3x3": (_I, (_P, _P, _I, _I, _I, _I, _P)),
    "orbit2_col2im3x3": (_I, (_P, _P, _P, _P, _I, _I, _I, _I, _P)),
    "orbit2_maxpool2_fwd": (_I, (_P, _P, _I, _I, _I, _I, _P)),
    "orbit2_maxpool2_bwd": (_I, (_P, _P, _P, _P, _I, _I, _I, _I, _P)),
    "orbit2_lpips_conv1_fwd": (_I, (_P, _P, _P, _P, _I, _I, _I, _P)),
    "orbit2_lpips_conv1_bwd": (_I, (_P, _P, _P, _P, _F, _P, _P, _I, _I, _I, _P)),
    "orbit2_lpips_tap_ws_floats": (_I64, (_I, _I, _I)),
    "orbit2_lpips_tap_fwd": (_I, (_P, _P, _P, _I, _I, _I, _P, _P)),
    "orbit2_lpips_tap_bwd": (_I, (_P, _P, _P, _F, _P, _I, _I, _I, _P)),
    "orbit2_l1_mean_ws_floats": (_I64, (_I64,)),
    "orbit2_l1_mean": (_I, (_P, _P, _P, _I64, _P, _P)),
    "orbit2_adamw": (_I, (_P, _P, _P, _P, _I, _P, _I64, _F, _F, _F, _F, _F, _F, _F, _F, _P, _P)),
    "orbit2_check_finite": (_I, (_P, _I, _I64, _P, _P)),
    "orbit2_seed_salt": (_I, (_U64, _I, _P)),
    "orbit2_selftest": (_I, (_P, _P)),
    "orbit2_probe_read": (_I, (_P, _I64, _I, _I, _P, _P)),
}


def load(path: str) -> C.CDLL:
    """Open a build of the library with every entry of PROTOTYPES declared (lib() for this package's build; the A/B tools
    open other builds with it).  A build of another ABI version, or one that lacks a declared entry, is refused."""
    if not os.path.exists(path):
        raise HipBackendError(
            "liborbit2_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). This package has no CPU fallback." % path)
    so = C.CDLL(path)
    version = so.orbit2_abi_version() if hasattr(so, "orbit2_abi_version") else None
    if version != ABI_VERSION:
        raise HipBackendError("%s has ABI version %s, this binding needs %d" % (path, version, ABI_VERSION))
    missing = [name for name in PROTOTYPES if not hasattr(so, name)]
    if missing:
        raise HipBackendError("%s lacks %s" % (path, ", ".join(missing)))
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(so, name)
        fn.restype, fn.argtypes = restype, argtypes
    return so


def lib():
    """load(LIB_PATH), once; fails loudly if the library is absent (no fallback path exists)."""
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH)
    return _lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(rc: int, name: str):
    if rc != 0:
        raise HipBackendError("%s failed with code %d (-1 bad argument, -2 launch error, -3 unsupported)" % (name, rc))


def _dev(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise HipBackendError("%s must be a GPU tensor (HIP backend has no CPU path)" % name)
    if t.dtype != dtype:
        raise HipBackendError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise HipBackendError("%s must be contiguous" % name)
    return t


BF, F32 = torch.bfloat16, torch.float32


# ---- tail queue (include/orbit2_hip.h: orbit2_gemm_bf16) ----------------------------------------------------------------------
# One zeroed counter word per stream: launches on one stream run one after the other and each leaves its word zero, launches on
# different streams may overlap and must not share one.  The words live 128 bytes apart in one buffer per device that is never
# freed (a captured graph keeps the address), handed out in the order streams first ask.  A launch that was aborted half-way
# leaves a count behind: sched_reset() zeroes everything.
_SCHED_SLOTS, _SCHED_STRIDE = 256, 32           # words apart
_sched_bufs, _sched_slots = {}, {}


def sched_workspace(device=None):
    """the device's counter buffer (int32 [_SCHED_SLOTS * _SCHED_STRIDE]); all zeros whenever no tail-queue launch is running"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _sched_bufs:
        _sched_bufs[idx] = torch.zeros(_SCHED_SLOTS * _SCHED_STRIDE, dtype=torch.int32, device=torch.device("cuda", idx))
    return _sched_bufs[idx]


def sched_reset():
    for buf in _sched_bufs.values():
        buf.zero_()


def _sched_word(device) -> int:
    """the address of the current stream's counter word on `device`"""
    buf = sched_workspace(device)
    key = (buf.device.index, torch.cuda.current_stream(buf.device).cuda_stream)
    slot = _sched_slots.get(key)
    if slot is None:
        slot = len([k for k in _sched_slots if k[0] == key[0]])
        if slot >= _SCHED_SLOTS:
            raise HipBackendError("tail queue: more than %d streams asked for a counter word" % _SCHED_SLOTS)
        _sched_slots[key] = slot
    return buf.data_ptr() + 4 * _SCHED_STRIDE * slot


def _tail_arg(tail_queue):
    """tail_queue of the wrappers -> the entries' `tail`: None / False = -1 (static: the plain call), True = 0 (sized by the
    library), an int > 0 = that many tiles by ticket (tests)"""
    if tail_queue is None or tail_queue is False:
        return -1
    if tail_queue is True:
        return 0
    if int(tail_queue) <= 0:
        raise HipBackendError("tail_queue: True, or a positive number of tiles")
    return int(tail_queue)


def _dev_rows(t: torch.Tensor, dtype, name: str):
    """a GEMM operand / epilogue tensor handed over with an explicit leading dimension: rows contiguous, any row pitch"""
    if t.dim() == 2 and t.stride(1) == 1 and t.is_cuda and t.dtype == dtype:
        return t
    return _dev(t, dtype, name)


class KernelTimer:
    """Optional live timing of individual launches with HIP events recorded on the launch stream
    (bench.py uses it for the roofline of the dominant kernel).  Off unless `_hip.timer` is set."""

    def __init__(self):
        self.records = {}      # name -> [ (work, ev0, ev1) ]

    def span(self, name, work, nbytes=0.0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.setdefault(name, []).append((work, e0, e1, nbytes))
        return e0, e1

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = [r[1].elapsed_time(r[2]) for r in recs]
            out[name] = {"launches": len(recs), "work": float(sum(r[0] for r in recs)), "ms": float(sum(ms)),
                         "bytes": float(sum(r[3] for r in recs)) / max(1, len(recs))}
        return out


timer: Optional[KernelTimer] = None


@contextlib.contextmanager
def _timed(name, flops, nbytes=0.0):
    """records the launches inside the block as one span of `timer`; does nothing when no timer is set"""
    if timer is None:
        yield
        return
    e0, e1 = timer.span(name, flops, nbytes)
    e0.record()
    yield
    e1.record()


def _queue(tail, device):
    """the (sched_ws, tail, stream) that end a GEMM or attention entry's arguments: the stream's counter word on `device` when a
    tail queue is asked for (tail >= 0), NULL for a static call -- which so never allocates the counter buffer or claims a slot"""
    return (_sched_word(device) if tail >= 0 else None), tail, _stream()


# ------------------------------------------------------------------------------------------------
def _gemm_fill(a, A, B, out, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, bias=None, act=0, save_pre=None,
               dgelu_pre=None, drop_p=0.0, seed=0, rowscale=None, rows_per_scale=0, residual=None, ldr=0, res_mod=0,
               res_first=False, beta=0.0, tile=0, colscale=None, save_dact=None, mul=None):
    for t, nm in ((A, "A"), (B, "B")):
        _dev_rows(t, BF, nm)
    if out.dtype not in (BF, F32) or not out.is_cuda:
        raise HipBackendError("gemm out must be a bf16/fp32 GPU tensor")
    a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc = M, N, K, lda, ldb, ldc
    a.a_kc, a.b_kc = int(a_kc), int(b_kc)
    a.bias = None if bias is None else _dev(bias, BF, "bias").data_ptr()
    a.act = act
    a.save_pre = None if save_pre is None else _dev_rows(save_pre, BF, "save_pre").data_ptr()      # row pitch = ldc
    a.dgelu_pre = None if dgelu_pre is None else _dev_rows(dgelu_pre, BF, "dgelu_pre").data_ptr()  # row pitch = ldc
    a.drop_p, a.seed = float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF
    a.rowscale = None if rowscale is None else _dev(rowscale, F32, "rowscale").data_ptr()
    a.rows_per_scale = rows_per_scale
    a.residual = None if residual is None else _dev(residual, BF, "residual").data_ptr()
    a.ldr, a.res_mod, a.res_first = ldr, res_mod, int(res_first)
    a.out_fp32 = int(out.dtype == F32)
    a.beta = float(beta)
    a.tile_hint = int(tile)
    a.colscale_n, a.colscale = (0, 1.0) if colscale is None else (int(colscale[0]), float(colscale[1]))
    a.save_dact = None if save_dact is None else _dev_rows(save_dact, torch.int16, "save_dact").data_ptr()    # int16 q14, row pitch = ldc
    a.mul = None if mul is None else _dev_rows(mul, torch.int16, "mul").data_ptr()                   # int16 q14, row pitch = ldc
    a.colsum_ws = None
    return 2.0 * M * N * K, 2.0 * (M * K + N * K) + M * N * (4.0 if out.dtype == F32 else 2.0)


def gemm(A, B, out, M, N, K, lda, ldb, ldc, want_colsum=False, gate=None, rows_per_gate=0, tail_queue=None, **kw):
    """out[M,N] = epilogue(A x B); see include/orbit2_hip.h:orbit2_gemm_bf16.
    want_colsum: returns (out, parts) -- parts = fp32 [M / 256, N] per-tile-row column sums of the stored output when this call
    can fuse them (orbit2_gemm_bf16_colsum_rows), else None: the caller then runs `colsum` on `out` itself.
    gate: fp32 [ceil(M / rows_per_gate)] path gate: rows of an entry that is 0.0 may be stored as zeros
    (as the residual rows when `rowscale` is the gate) without being computed.
    tail_queue: True = the launch's last rounds by ticket (_tail_arg); the results are the same bits."""
    tail = _tail_arg(tail_queue)
    if gate is not None:
        _dev(gate, F32, "gate")
        if rows_per_gate <= 0 or gate.numel() * rows_per_gate < M:
            raise HipBackendError("gemm gate needs rows_per_gate > 0 and one entry per rows_per_gate rows")

    a = GemmArgs()
    flops, nbytes = _gemm_fill(a, A, B, out, M, N, K, lda, ldb, ldc, **kw)
    parts = None
    if want_colsum:
        rows = lib().orbit2_gemm_bf16_colsum_rows(C.byref(a))
        if rows > 0:
            parts = torch.empty(rows, N, dtype=F32, device=out.device)
            a.colsum_ws = parts.data_ptr()
    with _timed("gemm_bf16", flops, nbytes):
        _chk(lib().orbit2_gemm_bf16(C.byref(a), _p(gate), rows_per_gate if gate is not None else 0, *_queue(tail, out.device)),
             "orbit2_gemm_bf16")
    return (out, parts) if want_colsum else out


def gemm_f32(A, B, out, M, N, K, lda, ldb, ldc, bias=None, act=0, residual=None, ldr=0, res_mod=0, res_first=False, beta=0.0,
             tile=0, colscale=None):
    """out[M,N] = epilogue(A x B^T) in fp32 (include/orbit2_hip.h:orbit2_gemm_f32): A [M][lda], B [N][ldb] the fp32 weight as
    stored, every tensor fp32; forward form and forward epilogue only"""
    for t, nm in ((A, "A"), (B, "B"), (out, "out")):
        _dev_rows(t, F32, nm)
    a = GemmArgs()
    a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc = M, N, K, lda, ldb, ldc
    a.a_kc = a.b_kc = 1
    a.bias = None if bias is None else _dev(bias, F32, "bias").data_ptr()
    a.act = act
    a.residual = None if residual is None else _dev_rows(residual, F32, "residual").data_ptr()
    a.ldr, a.res_mod, a.res_first = ldr, res_mod, int(res_first)
    a.out_fp32 = 1
    a.beta = float(beta)
    a.tile_hint = int(tile)
    a.colscale_n, a.colscale = (0, 1.0) if colscale is None else (int(colscale[0]), float(colscale[1]))
    with _timed("gemm_f32", 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N)):
        _chk(lib().orbit2_gemm_f32(C.byref(a), _stream()), "orbit2_gemm_f32")
    return out


GEMM_MAX_GROUP = 12


def gemm_grouped(problems, tail_queue=None):
    """problems: list of (A, B, out, M, N, K, lda, ldb, ldc, kwargs) sharing one operand form; one launch
    (include/orbit2_hip.h:orbit2_gemm_bf16_grouped).  A problem's kwargs may hold kgate = (fp32 vector, rows of the contraction
    per entry): the K gate -- ranges of the contraction whose entry is 0.0 hold zero rows in A.
    tail_queue: as in gemm."""
    tail = _tail_arg(tail_queue)
    n = len(problems)
    if not 0 < n <= GEMM_MAX_GROUP:
        raise HipBackendError("gemm_grouped takes 1..%d problems" % GEMM_MAX_GROUP)
    arr = (GemmArgs * n)()
    kgates, kper, gated = (C.c_void_p * n)(), (C.c_int * n)(), False
    flops = nbytes = 0.0
    for i, (A, B, out, M, N, K, lda, ldb, ldc, kw) in enumerate(problems):
        kw = dict(kw)
        kg = kw.pop("kgate", None)
        if kg is not None:
            vec, per = kg
            if per <= 0 or _dev(vec, F32, "kgate").numel() * per < K:
                raise HipBackendError("gemm_grouped kgate needs one entry per k_per_gate rows of the contraction")
            kgates[i], kper[i], gated = vec.data_ptr(), per, True
        f, b = _gemm_fill(arr[i], A, B, out, M, N, K, lda, ldb, ldc, **kw)
        flops += f
        nbytes += b

    with _timed("gemm_bf16", flops, nbytes):
        _chk(lib().orbit2_gemm_bf16_grouped(arr, n, kgates if gated else None, kper if gated else None,
                                            *_queue(tail, problems[0][2].device)), "orbit2_gemm_bf16_grouped")


def sgemm(A, B, out, M, N, K, lda, ldb, ldc, ta=False, tb=False, alpha=1.0, beta=0.0):
    for t, nm in ((A, "A"), (B, "B"), (out, "C")):
        _dev(t, F32, nm)
    n = lib().orbit2_sgemm_f32_ws_floats(M, N, K)
    ws = torch.empty(n, dtype=F32, device=out.device) if n else None
    _chk(lib().orbit2_sgemm_f32_ws(_p(A), _p(B), _p(out), M, N, K, lda, ldb, ldc, int(ta), int(tb), alpha, beta, _p(ws), n,
                                   _stream()), "orbit2_sgemm_f32_ws")
    return out


def layernorm_fwd(x, gamma, beta, eps=1e-5, out=None):
    """out: optional [rows, D] bf16 destination with any row pitch (a view of a padded buffer: orbit2_layernorm_fwd_ld)"""
    _dev(x, BF, "x"); _dev(gamma, BF, "gamma"); _dev(beta, BF, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x) if out is None else _dev_rows(out, BF, "out")
    ldy = D if out is None else y.stride(0)
    mean = torch.empty(rows, dtype=F32, device=x.device)
    rstd = torch.empty(rows, dtype=F32, device=x.device)
    _chk(lib().orbit2_layernorm_fwd_ld(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, D, ldy, eps,
                                       _stream()), "orbit2_layernorm_fwd_ld")
    return y, mean, rstd


def layernorm_fwd_f32(x, gamma, beta, eps=1e-5, out=None, stats=False):
    """fp32 LayerNorm (orbit2_layernorm_fwd_f32); returns y, or (y, mean, rstd) with stats=True"""
    _dev(x, F32, "x"); _dev(gamma, F32, "gamma"); _dev(beta, F32, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x) if out is None else _dev_rows(out, F32, "out")
    ldy = D if out is None else y.stride(0)
    mean = torch.empty(rows, dtype=F32, device=x.device) if stats else None
    rstd = torch.empty(rows, dtype=F32, device=x.device) if stats else None
    _chk(lib().orbit2_layernorm_fwd_f32(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, D, ldy, eps,
                                        _stream()), "orbit2_layernorm_fwd_f32")
    return (y, mean, rstd) if stats else y


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, beta_acc=0.0):
    _dev(dy, BF, "dy"); _dev(x, BF, "x"); _dev(gamma, BF, "gamma")
    D = x.shape[-1]
    rows = x.numel() // D
    dx = torch.empty_like(x)
    n = lib().orbit2_layernorm_bwd_ws_floats(rows, D)
    ws = torch.empty(n, dtype=F32, device=x.device)
    fp32 = int(dgamma.dtype == F32)
    _chk(lib().orbit2_layernorm_bwd(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dgamma),
                                    _p(dbeta), fp32, beta_acc, _p(ws), n, rows, D, _stream()),
         "orbit2_layernorm_bwd")
    return dx


ATTN_4WAVES, ATTN_SPLIT_DKV, ATTN_Q_PRESCALED, ATTN_NO_W4 = 1, 2, 4, 8      # include/orbit2_hip.h: the kernel-variant flags of the attention entries (A/B, tests)


def probe_read(buf, blocks, inflight, sink):
    """diagnostic calibration stream (include/orbit2_hip.h: orbit2_probe_read)"""
    _chk(lib().orbit2_probe_read(_p(buf), buf.numel() * buf.element_size(), int(blocks), int(inflight), _p(sink),
                                 _stream()), "orbit2_probe_read")


def mall_calibration():
    """the calibration streams of the memory-side latency probe, in a fixed order that tools/summarize_prof.py `mall` decodes
    from the dispatch order of probe_read_kernel: Infinity-Cache-resident buffer (96 MB; first sweep = fill, not counted) at
    low / high load, then a 4 GB buffer (HBM) at low / high load"""
    sink = torch.zeros(1, dtype=F32, device="cuda")
    small = torch.ones(24 << 20, dtype=F32, device="cuda")          # 96 MB: beyond the 32 MB of L2, inside the Infinity Cache
    probe_read(small, 2048, 8, sink)                                 # fill
    for _ in range(6):
        probe_read(small, 64, 1, sink)                               # Infinity-Cache hits, lightly loaded
    for _ in range(6):
        probe_read(small, 2048, 8, sink)                             # ... under a saturating stream
    del small
    big = torch.ones(1 << 30, dtype=F32, device="cuda")             # 4 GB: every sweep reads HBM
    for _ in range(2):
        probe_read(big, 64, 1, sink)
    for _ in range(2):
        probe_read(big, 2048, 8, sink)
    del big
    torch.cuda.synchronize()


def _attn_gate(gate, B):
    if gate is not None and _dev(gate, F32, "gate").numel() < B:
        raise HipBackendError("attention gate needs one entry per sample")
    return gate


def attn_fwd(qkv, B, L, H, d, drop_p=0.0, seed=0, flags=0, out=None, gate=None, tail_queue=None):
    """out: optional [B * L, H * d] bf16 destination with any token-row pitch (orbit2_attn_fwd_ld); default [B, L, H * d].
    gate: fp32 [B] path gate: out and lse of a sample whose entry is 0.0 may be stored as zeros
    tail_queue: as in gemm"""
    tail = _tail_arg(tail_queue)
    _attn_gate(gate, B)
    _dev_rows(qkv, BF, "qkv")
    ldq = qkv.stride(0) if qkv.dim() == 2 else 3 * H * d       # [B * L, 3 * H * d] with a token-row pitch, or contiguous
    if out is None:
        out, ldo = torch.empty(B, L, H * d, dtype=BF, device=qkv.device), H * d
    else:
        out = _dev_rows(out, BF, "out")
        ldo = out.stride(0)
    lse = torch.empty(B, H, L, dtype=F32, device=qkv.device)
    # algorithmic bytes: qkv read once, out + lse written once
    with _timed("attn_fwd", 4.0 * B * H * L * L * d, 2.0 * 4 * B * L * H * d + 4.0 * B * H * L):
        _chk(lib().orbit2_attn_fwd_ld(_p(qkv), _p(out), _p(lse), B, L, H, d, drop_p, seed, int(flags), int(ldq), int(ldo), _p(gate),
                                      *_queue(tail, qkv.device)), "orbit2_attn_fwd_ld")
    return out, lse


def attn_fwd_f32(qkv, B, L, H, d, drop_p=0.0, flags=0, out=None):
    """fp32 attention core (orbit2_attn_fwd_f32): qkv fp32 [B * L, 3 * H * d] (any token-row pitch) or contiguous
    [B, L, 3, H, d]; returns (out [B, L, H * d] fp32 or the given `out`, lse [B, H, L])"""
    _dev_rows(qkv, F32, "qkv")
    ldq = qkv.stride(0) if qkv.dim() == 2 else 3 * H * d
    if out is None:
        out, ldo = torch.empty(B, L, H * d, dtype=F32, device=qkv.device), H * d
    else:
        out = _dev_rows(out, F32, "out")
        ldo = out.stride(0)
    lse = torch.empty(B, H, L, dtype=F32, device=qkv.device)
    with _timed("attn_fwd_f32", 4.0 * B * H * L * L * d, 4.0 * 4 * B * L * H * d + 4.0 * B * H * L):
        _chk(lib().orbit2_attn_fwd_f32(_p(qkv), _p(out), _p(lse), B, L, H, d, drop_p, 0, int(flags), int(ldq), int(ldo),
                                       _stream()), "orbit2_attn_fwd_f32")
    return out, lse


def attn_bwd(qkv, out, dout, lse, B, L, H, d, drop_p=0.0, seed=0, flags=0, gate=None, tail_queue=None):
    """gate: fp32 [B] path gate (orbit2_attn_bwd_ld): dqkv of a sample whose entry is 0.0 may be stored as zeros
    tail_queue: as in gemm"""
    tail = _tail_arg(tail_queue)
    _attn_gate(gate, B)
    _dev_rows(qkv, BF, "qkv"); _dev_rows(out, BF, "out"); _dev(dout, BF, "dout"); _dev(lse, F32, "lse")
    ldo = out.stride(0) if out.dim() == 2 else H * d           # [B * L, H * d] with a token-row pitch, or contiguous [B, L, H * d]
    ldq = qkv.stride(0) if qkv.dim() == 2 else 3 * H * d
    if ldq != 3 * H * d:                                        # dqkv carries qkv's pitch (it is a GEMM operand too)
        dqkv = torch.empty(B * L, ldq, dtype=BF, device=qkv.device)[:, :3 * H * d]
    else:
        dqkv = torch.empty_like(qkv)
    delta = torch.empty(lib().orbit2_attn_bwd_ws_floats(B, L, H), dtype=F32, device=qkv.device)
    # algorithmic: 2x the forward's FLOPs (recompute not credited); qkv, out, dout read once, dqkv written once
    with _timed("attn_bwd", 8.0 * B * H * L * L * d, 2.0 * 8 * B * L * H * d + 8.0 * B * H * L):
        _chk(lib().orbit2_attn_bwd_ld(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), B, L, H, d, drop_p, seed, int(flags),
                                      int(ldq), int(ldo), _p(gate), *_queue(tail, qkv.device)), "orbit2_attn_bwd_ld")
    return dqkv


PATCH_SIZES = (1, 2, 4)         # the patch sizes csrc/varagg.hip instantiates (C = p * p + 1 table coefficients per variable)


def _patch_of(C_, what):
    """the patch size p a table with C = p * p + 1 coefficients per variable was built for; any other C is refused"""
    for p in PATCH_SIZES:
        if C_ == p * p + 1:
            return p
    raise HipBackendError("%s has %d coefficients per variable: the folded patch-embed kernels take p * p + 1 for a patch size p "
                          "in %s" % (what, C_, PATCH_SIZES))


def _varagg_shapes(x, gtab, stab=None):
    """(B, V, h, w, p, tokens) of a folded patch-embed call: p from the tables' coefficient count, the grid a multiple of it"""
    B, V, h, w = x.shape
    if gtab.dim() != 3 or gtab.shape[0] != V:
        raise HipBackendError("gtab must be [V = %d, p * p + 1, D], got %s" % (V, tuple(gtab.shape)))
    p = _patch_of(gtab.shape[1], "gtab")
    if stab is not None and (stab.dim() != 3 or stab.shape[1] != V or stab.shape[2] != gtab.shape[1]):
        raise HipBackendError("stab must be [H, V = %d, %d] as gtab is %s, got %s" % (V, gtab.shape[1], tuple(gtab.shape),
                                                                                  tuple(stab.shape)))
    if h % p or w % p:
        raise HipBackendError("the grid %d x %d is not a multiple of the patch size %d" % (h, w, p))
    return B, V, h, w, p, B * (h // p) * (w // p)


def varagg_fwd(x, stab, gtab, H, D):
    """z bf16 [tokens, D], attw fp32 [tokens, H, V]; the patch size is the tables': stab [H, V, p*p+1], gtab [V, p*p+1, D]"""
    _dev(x, F32, "x"); _dev(stab, F32, "stab"); _dev(gtab, F32, "gtab")
    B, V, h, w, p, ntok = _varagg_shapes(x, gtab, stab)
    z = torch.empty(ntok, D, dtype=BF, device=x.device)
    attw = torch.empty(ntok, H, V, dtype=F32, device=x.device)
    if p == 2:
        _chk(lib().orbit2_varagg_fwd(_p(x), _p(stab), _p(gtab), _p(z), _p(attw), B, V, h, w, H, D, _stream()),
             "orbit2_varagg_fwd")
    else:
        _chk(lib().orbit2_varagg_fwd_p(_p(x), _p(stab), _p(gtab), _p(z), _p(attw), B, V, h, w, p, H, D, _stream()),
             "orbit2_varagg_fwd_p")
    return z, attw


def varagg_fwd_f32(x, stab, gtab, H, D, want_attw=False):
    """the folded variable aggregation with fp32 tokens (orbit2_varagg_fwd_f32); returns z, or (z, attw) with want_attw"""
    _dev(x, F32, "x"); _dev(stab, F32, "stab"); _dev(gtab, F32, "gtab")
    B, V, h, w, p, ntok = _varagg_shapes(x, gtab, stab)
    z = torch.empty(ntok, D, dtype=F32, device=x.device)
    attw = torch.empty(ntok, H, V, dtype=F32, device=x.device) if want_attw else None
    if p == 2:
        _chk(lib().orbit2_varagg_fwd_f32(_p(x), _p(stab), _p(gtab), _p(z), _p(attw), B, V, h, w, H, D, _stream()),
             "orbit2_varagg_fwd_f32")
    else:
        _chk(lib().orbit2_varagg_fwd_f32_p(_p(x), _p(stab), _p(gtab), _p(z), _p(attw), B, V, h, w, p, H, D, _stream()),
             "orbit2_varagg_fwd_f32_p")
    return (z, attw) if want_attw else z


def _ws(query, args, device):
    """fp32 workspace of a two-stage (slab + fixed-order combine) reduction: `query` is the entry's *_ws_floats function"""
    n = query(*args)
    if n <= 0:
        raise HipBackendError("workspace query failed for %r" % (args,))
    return torch.empty(n, dtype=F32, device=device)


# set once a gradient was accumulated with atomics (summation order not fixed): dist/tp.py ReplicaGuard then exchanges the
# tensor-parallel replicas' gradients instead of relying on their bitwise agreement
atomics_in_grad_path = False


def varagg_bwd(x, gtab, attw, dz, H, D):
    global atomics_in_grad_path
    _dev(x, F32, "x"); _dev(gtab, F32, "gtab"); _dev(attw, F32, "attw"); _dev(dz, BF, "dz")
    B, V, h, w, p, ntok = _varagg_shapes(x, gtab)
    C_ = p * p + 1
    dstab = torch.zeros(H, V, C_, dtype=F32, device=x.device)
    dgtab = torch.zeros(V, C_, D, dtype=F32, device=x.device)
    if p != 2:
        # the two-stage fixed-order backward (no float atomics anywhere): `atomics_in_grad_path` is not touched
        if not lib().orbit2_varagg_bwd_p_is_fixed_order(B, V, h, w, p, H, D):
            raise HipBackendError("orbit2_varagg_bwd_p does not serve B=%d V=%d grid %dx%d patch %d H=%d D=%d (its LDS need "
                                  "exceeds a CU's 160 KiB, or the shape is invalid)" % (B, V, h, w, p, H, D))
        ws = _ws(lib().orbit2_varagg_bwd_p_ws_floats, (B, V, h, w, p, H, D), x.device)
        _chk(lib().orbit2_varagg_bwd_p(_p(x), _p(gtab), _p(attw), _p(dz), _p(dstab), _p(dgtab), B, V, h, w, p, H, D, _p(ws),
                                       _stream()), "orbit2_varagg_bwd_p")
        return dstab, dgtab
    if not atomics_in_grad_path and not lib().orbit2_varagg_bwd_is_fixed_order(B, V, h, w, H, D):
        atomics_in_grad_path = True
    ws = _ws(lib().orbit2_varagg_bwd_ws_floats, (B, V, h, w, H, D), x.device)
    _chk(lib().orbit2_varagg_bwd(_p(x), _p(gtab), _p(attw), _p(dz), _p(dstab), _p(dgtab), B, V, h, w, H, D, _p(ws), _stream()),
         "orbit2_varagg_bwd")
    return dstab, dgtab


def tables_gather(w0, w_stride, b0, b_stride, var_embed, ids, V, D):
    """cmat [5 V, D] fp32 from the per-variable patch-embed parameters laid out at a uniform pitch (w0 / b0 = parameter 0)"""
    _dev(w0, F32, "token_embeds.0.proj.weight"); _dev(b0, F32, "token_embeds.0.proj.bias"); _dev(var_embed, F32, "var_embed")
    _dev(ids, torch.int32, "ids")
    cmat = torch.empty(5 * V, D, dtype=F32, device=w0.device)
    _chk(lib().orbit2_tables_gather(_p(w0), w_stride, _p(b0), b_stride, _p(var_embed), _p(ids), _p(cmat), V, D, _stream()),
         "orbit2_tables_gather")
    return cmat


def tables_scatter(dcmat, gw0, w_stride, gb0, b_stride, gvar_embed, ids, V, D):
    """accumulates the rows' gradient into the parameters' gradient buffers (same pitches)"""
    _dev(dcmat, F32, "dcmat"); _dev(gw0, F32, "dW"); _dev(gb0, F32, "db"); _dev(gvar_embed, F32, "dvar_embed")
    _chk(lib().orbit2_tables_scatter(_p(dcmat), _p(gw0), w_stride, _p(gb0), b_stride, _p(gvar_embed), _p(ids), V, D,
                                     _stream()), "orbit2_tables_scatter")


def dropout_bwd(dy, M, N, drop_p, seed, rowscale=None, rows_per_scale=0, out=None):
    _dev(dy, BF, "dy")
    out = torch.empty_like(dy) if out is None else out
    _chk(lib().orbit2_dropout_bwd(_p(dy), _p(out), M, N, drop_p, seed, _p(rowscale), rows_per_scale, _stream()),
         "orbit2_dropout_bwd")
    return out


def dropout_bwd_colsum(dy, M, N, drop_p, seed, rowscale, rows_per_scale, colsum_out, beta=0.0):
    """dym = dy * dropmask * rowscale and colsum_out[n] (+)= sum_m dym[m][n] in one pass"""
    _dev(dy, BF, "dy")
    out = torch.empty_like(dy)
    n = lib().orbit2_colsum_ws_floats(M, N)
    ws = torch.empty(n, dtype=F32, device=dy.device)
    _chk(lib().orbit2_dropout_bwd_colsum(_p(dy), _p(out), M, N, drop_p, seed, _p(rowscale), rows_per_scale, _p(colsum_out),
                                         int(colsum_out.dtype == F32), beta, _p(ws), n, _stream()), "orbit2_dropout_bwd_colsum")
    return out


def post_reduce(x, M, N, addend=None, res_mod=0, residual=None, drop_p=0.0, seed=0, rowscale=None, rows_per_scale=0,
                out=None):
    """y = residual + rowscale * dropout(x + addend[m % res_mod]); in place on x unless `out` is given"""
    _dev(x, BF, "x")
    for t, nm in ((addend, "addend"), (residual, "residual")):
        if t is not None:
            _dev(t, BF, nm)
    out = x if out is None else out
    _chk(lib().orbit2_post_reduce(_p(x), _p(addend), res_mod, _p(residual), _p(out), M, N, drop_p, seed, _p(rowscale),
                                  rows_per_scale, _stream()), "orbit2_post_reduce")
    return out


def colsum(x, M, N, ldx, out, beta=0.0):
    if x.dtype not in (BF, F32):
        raise HipBackendError("colsum input must be bf16/fp32")
    n = lib().orbit2_colsum_ws_floats(M, N)
    ws = torch.empty(n, dtype=F32, device=x.device)
    _chk(lib().orbit2_colsum(_p(x), int(x.dtype == F32), M, N, ldx, _p(out), int(out.dtype == F32), beta,
                             _p(ws), n, _stream()), "orbit2_colsum")
    return out


def batch_sum(x, B, rows, N, out, beta=0.0):
    _dev(x, BF, "x")
    _chk(lib().orbit2_batch_sum(_p(x), _p(out), B, rows, N, int(out.dtype == F32), beta, _stream()),
         "orbit2_batch_sum")
    return out


def cast_to_bf16(src, dst=None):
    _dev(src, F32, "src")
    dst = torch.empty(src.shape, dtype=BF, device=src.device) if dst is None else dst
    _chk(lib().orbit2_cast_f32_to_bf16(_p(src), _p(dst), src.numel(), _stream()), "orbit2_cast_f32_to_bf16")
    return dst


def cast_to_f32(src, dst=None):
    _dev(src, BF, "src")
    dst = torch.empty(src.shape, dtype=F32, device=src.device) if dst is None else dst
    _chk(lib().orbit2_cast_bf16_to_f32(_p(src), _p(dst), src.numel(), _stream()), "orbit2_cast_bf16_to_f32")
    return dst


def add_rowvec(a, vec, rows, N):
    _dev(a, BF, "a"); _dev(vec, BF, "vec")
    y = torch.empty_like(a)
    _chk(lib().orbit2_add_rowvec(_p(a), _p(vec), _p(y), rows, N, _stream()), "orbit2_add_rowvec")
    return y


def posembed_fwd(pe, sw, sb, res, oh, ow, nh, nw):
    """[nh*nw, D] fp32 = bicubic re-grid of the [oh*ow, D] table (identity when oh == nh) + sw * res + sb"""
    _dev(pe, F32, "pos_embed")
    D = pe.shape[-1]
    if sw is not None:
        _dev(sw, F32, "spatial_embed.weight"); _dev(sb, F32, "spatial_embed.bias")
    out = torch.empty(nh * nw, D, dtype=F32, device=pe.device)
    _chk(lib().orbit2_posembed_fwd(_p(pe), _p(sw), _p(sb), res, _p(out), oh, ow, nh, nw, D, _stream()),
         "orbit2_posembed_fwd")
    return out


def posembed_bwd(dout, oh, ow, nh, nw):
    _dev(dout, F32, "dposres")
    D = dout.shape[-1]
    dpe = torch.empty(oh * ow, D, dtype=F32, device=dout.device)
    _chk(lib().orbit2_posembed_bwd(_p(dout), _p(dpe), oh, ow, nh, nw, D, _stream()), "orbit2_posembed_bwd")
    return dpe


def unpatchify_fwd(t, B, Cc, h, w, p, s):
    _dev(t, BF, "t")
    img = torch.empty(B, Cc, h * s, w * s, dtype=F32, device=t.device)
    _chk(lib().orbit2_unpatchify_fwd(_p(t), _p(img), B, Cc, h, w, p, s, _stream()), "orbit2_unpatchify_fwd")
    return img


def unpatchify_fwd_f32(t, B, Cc, h, w, p, s):
    _dev(t, F32, "t")
    img = torch.empty(B, Cc, h * s, w * s, dtype=F32, device=t.device)
    _chk(lib().orbit2_unpatchify_fwd_f32(_p(t), _p(img), B, Cc, h, w, p, s, _stream()), "orbit2_unpatchify_fwd_f32")
    return img


def unpatchify_bwd(dimg, B, Cc, h, w, p, s):
    _dev(dimg, F32, "dimg")
    L = h * w // (p * p)
    dt = torch.empty(B, L, Cc * (s * p) ** 2, dtype=BF, device=dimg.device)
    _chk(lib().orbit2_unpatchify_bwd(_p(dimg), _p(dt), B, Cc, h, w, p, s, _stream()), "orbit2_unpatchify_bwd")
    return dt


def conv3x3_fwd(x, chan_idx, weight, bias, mode=0, r=1, addend=None):
    _dev(x, F32, "in"); _dev(weight, F32, "weight"); _dev(bias, F32, "bias")
    B, ctot, H, W = x.shape
    Cout, Cin = weight.shape[0], weight.shape[1]
    pre = None
    if mode == 0:
        out = torch.empty(B, Cout, H, W, dtype=F32, device=x.device)
    else:
        out = torch.empty(B, Cout // (r * r), H * r, W * r, dtype=F32, device=x.device)
        pre = torch.empty(B, Cout, H, W, dtype=F32, device=x.device)
    Ha = Wa = 0
    if addend is not None:
        _dev(addend, F32, "addend")
        Ha, Wa = addend.shape[2], addend.shape[3]
    _chk(lib().orbit2_conv3x3_fwd(_p(x), _p(chan_idx), ctot, _p(weight), _p(bias), _p(out), _p(pre), _p(addend), Ha, Wa,
                                  B, Cin, Cout, H, W, mode, r, _stream()), "orbit2_conv3x3_fwd")
    return out, pre


def conv3x3_bwd(dout, x, chan_idx, weight, pre, need_din, mode=0, r=1):
    _dev(dout, F32, "dout"); _dev(x, F32, "in"); _dev(weight, F32, "weight")
    B, ctot, H, W = x.shape
    Cout, Cin = weight.shape[0], weight.shape[1]
    din = torch.empty(B, Cin, H, W, dtype=F32, device=x.device) if need_din else None
    dw = torch.zeros_like(weight)
    db = torch.zeros(Cout, dtype=F32, device=x.device)
    ws = _ws(lib().orbit2_conv3x3_bwd_ws_floats, (B, Cin, Cout, H, W), x.device)
    _chk(lib().orbit2_conv3x3_bwd(_p(dout), _p(x), _p(chan_idx), ctot, _p(weight), _p(pre), _p(din), _p(dw), _p(db), B,
                                  Cin, Cout, H, W, mode, r, _p(ws), _stream()), "orbit2_conv3x3_bwd")
    return din, dw, db


def clamp_channel_(img, chan):
    _dev(img, F32, "img")
    B, Cc, H, W = img.shape
    _chk(lib().orbit2_clamp_channel(_p(img), B, Cc, H * W, chan, _stream()), "orbit2_clamp_channel")
    return img


def clamp_channel_bwd_(img_clamped, dimg, chan):
    _dev(img_clamped, F32, "img"); _dev(dimg, F32, "dimg")
    B, Cc, H, W = img_clamped.shape
    _chk(lib().orbit2_clamp_channel_bwd(_p(img_clamped), _p(dimg), B, Cc, H * W, chan, _stream()),
         "orbit2_clamp_channel_bwd")
    return dimg


def loss_fwd(pred, target, lat_w, chan_w, kind):
    _dev(pred, F32, "pred"); _dev(target, F32, "target")
    B, Cc, H, W = pred.shape
    Ht, Wt = target.shape[2], target.shape[3]
    out = torch.empty(Cc + 1, dtype=F32, device=pred.device)
    ws = torch.empty(2 * Cc * B * 64, dtype=F32, device=pred.device)
    _chk(lib().orbit2_loss_fwd(_p(pred), _p(target), Ht, Wt, _p(lat_w), _p(chan_w), _p(out), _p(ws), B, Cc, H, W, kind,
                               _stream()), "orbit2_loss_fwd")
    return out


def loss_bwd(pred, target, lat_w, chan_w, gscale, kind):
    B, Cc, H, W = pred.shape
    Ht, Wt = target.shape[2], target.shape[3]
    dpred = torch.empty_like(pred)
    _chk(lib().orbit2_loss_bwd(_p(pred), _p(target), Ht, Wt, _p(lat_w), _p(chan_w), _p(_dev(gscale, F32, "gscale")),
                               _p(dpred), B, Cc, H, W, kind, _stream()), "orbit2_loss_bwd")
    return dpred


def adamw(p, m, v, g, p16, n, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, found_inf=None):
    _dev(p, F32, "p"); _dev(m, F32, "m"); _dev(v, F32, "v")
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _chk(lib().orbit2_adamw(_p(p), _p(m), _p(v), _p(g), int(g.dtype == F32), _p(p16), n, lr, beta1, beta2, eps, wd, bc1, bc2,
                            grad_scale, _p(found_inf), _stream()), "orbit2_adamw")


def check_finite(g, n, found_inf):
    _chk(lib().orbit2_check_finite(_p(g), int(g.dtype == F32), n, _p(found_inf), _stream()),
         "orbit2_check_finite")


def selftest(device="cuda") -> int:
    buf = torch.zeros(512, dtype=torch.int32, device=device)
    _chk(lib().orbit2_selftest(_p(buf), _stream()), "orbit2_selftest")
    torch.cuda.synchronize()
    return int(buf[0].item())


def droppath_scales(B, p, seed, device):
    out = torch.empty(B, dtype=F32, device=device)
    _chk(lib().orbit2_droppath_scales(_p(out), B, p, seed, _stream()), "orbit2_droppath_scales")
    return out


def transpose_bf16(src, dst):
    _dev(src, BF, "src"); _dev(dst, BF, "dst")
    R, Cc = src.shape
    _chk(lib().orbit2_transpose_bf16(_p(src), _p(dst), R, Cc, _stream()), "orbit2_transpose_bf16")
    return dst


# ---- perceptual loss building blocks (csrc/lpips.hip) ----------------------------------------------------------
def im2col3x3(x, N, H, W, Cc):
    _dev(x, BF, "x")
    col = torch.empty(N * H * W, 9 * Cc, dtype=BF, device=x.device)
    _chk(lib().orbit2_im2col3x3(_p(x), _p(col), N, H, W, Cc, _stream()), "orbit2_im2col3x3")
    return col


def col2im3x3(dcol, N, H, W, Cc, act=None, tapg=None):
    _dev(dcol, BF, "dcol")
    out = torch.empty(N * H * W, Cc, dtype=BF, device=dcol.device)
    _chk(lib().orbit2_col2im3x3(_p(dcol), _p(act), _p(tapg), _p(out), N, H, W, Cc, _stream()), "orbit2_col2im3x3")
    return out


def maxpool2_fwd(x, N, H, W, Cc):
    _dev(x, BF, "x")
    y = torch.empty(N * (H // 2) * (W // 2), Cc, dtype=BF, device=x.device)
    _chk(lib().orbit2_maxpool2_fwd(_p(x), _p(y), N, H, W, Cc, _stream()), "orbit2_maxpool2_fwd")
    return y


def maxpool2_bwd(g, x, N, H, W, Cc, tapg=None):
    _dev(g, BF, "g"); _dev(x, BF, "x")
    dz = torch.empty(N * H * W, Cc, dtype=BF, device=g.device)
    _chk(lib().orbit2_maxpool2_bwd(_p(g), _p(x), _p(tapg), _p(dz), N, H, W, Cc, _stream()), "orbit2_maxpool2_bwd")
    return dz


def lpips_conv1_fwd(img, w1, b1):
    _dev(img, F32, "img"); _dev(w1, F32, "w1"); _dev(b1, F32, "b1")
    N, _, H, W = img.shape
    out = torch.empty(N * H * W, 64, dtype=BF, device=img.device)
    _chk(lib().orbit2_lpips_conv1_fwd(_p(img), _p(w1), _p(b1), _p(out), N, H, W, _stream()), "orbit2_lpips_conv1_fwd")
    return out


def lpips_conv1_bwd(dz, w1, pred, target, l1_coef, gscale=None):
    _dev(dz, BF, "dz"); _dev(pred, F32, "pred"); _dev(target, F32, "target")
    N, _, H, W = pred.shape
    dimg = torch.empty_like(pred)
    gs = None if gscale is None else _p(_dev(gscale, F32, "gscale"))
    _chk(lib().orbit2_lpips_conv1_bwd(_p(dz), _p(w1), _p(pred), _p(target), l1_coef, gs, _p(dimg), N, H, W,
                                      _stream()), "orbit2_lpips_conv1_bwd")
    return dimg


def lpips_tap_fwd(feats, lin, val, B, HW, Cc):
    _dev(feats, BF, "feats"); _dev(lin, F32, "lin"); _dev(val, F32, "val")
    ws = _ws(lib().orbit2_lpips_tap_ws_floats, (B, HW, Cc), feats.device)
    _chk(lib().orbit2_lpips_tap_fwd(_p(feats), _p(lin), _p(val), B, HW, Cc, _p(ws), _stream()), "orbit2_lpips_tap_fwd")


def lpips_tap_bwd(feats, lin, coef, B, HW, Cc, gscale=None):
    _dev(feats, BF, "feats"); _dev(lin, F32, "lin")
    g = torch.empty(B * HW, Cc, dtype=BF, device=feats.device)
    gs = None if gscale is None else _p(_dev(gscale, F32, "gscale"))
    _chk(lib().orbit2_lpips_tap_bwd(_p(feats), _p(lin), _p(g), coef, gs, B, HW, Cc, _stream()),
         "orbit2_lpips_tap_bwd")
    return g


def l1_mean(a, b, out):
    _dev(a, F32, "a"); _dev(b, F32, "b"); _dev(out, F32, "out")
    ws = _ws(lib().orbit2_l1_mean_ws_floats, (a.numel(),), a.device)
    _chk(lib().orbit2_l1_mean(_p(a), _p(b), _p(out), a.numel(), _p(ws), _stream()), "orbit2_l1_mean")


def _scored_pair(name, pred, target, lat_w=None, clim=None):
    """(B, C, H, W) of a prediction scored against `target`, after the checks every such entry shares: both [B,C,H,W] fp32
    contiguous device tensors, the target of the same [B,C] and spatially not smaller (it is read through its top-left crop),
    lat_w fp32 with at least H entries, clim [C,H,W] of the prediction's size.  `pred` may be the shape alone, for a prediction
    that is never stored (resample_moments)."""
    shape = tuple(pred.shape) if torch.is_tensor(pred) else tuple(pred)
    if len(shape) != 4 or not torch.is_tensor(target) or target.dim() != 4:
        raise HipBackendError("%s takes [B,C,H,W] fields" % name)
    if torch.is_tensor(pred):
        _dev(pred, F32, "pred")
    _dev(target, F32, "target")
    B, Cc, H, W = shape
    if tuple(target.shape[:2]) != (B, Cc):
        raise HipBackendError("%s: target %s does not match the prediction's [B,C] %s" % (name, tuple(target.shape), (B, Cc)))
    if target.shape[2] < H or target.shape[3] < W:             # (the wording serves every wrapper's tests: one of them pins the code)
        raise HipBackendError("%s: target %s is smaller than the prediction %s; the entry would return code -1 (bad argument)"
                              % (name, tuple(target.shape), shape))
    if lat_w is not None and _dev(lat_w, F32, "lat_w").numel() < H:
        raise HipBackendError("%s: lat_w has %d entries, the prediction %d rows" % (name, lat_w.numel(), H))
    if clim is not None and (tuple(_dev(clim, F32, "clim").shape[-3:]) != (Cc, H, W) or clim.numel() != Cc * H * W):
        raise HipBackendError("%s: climatology must be [C,H,W] of the prediction's size" % name)
    return B, Cc, H, W


def eval_moments(pred, target, lat_w=None, clim=None):
    """[B,C,12] float64 sums over a = pred - clim, b = target - clim (see include/orbit2_hip.h:orbit2_eval_moments)"""
    B, Cc, H, W = _scored_pair("eval_moments", pred, target, lat_w, clim)
    out = torch.empty(B, Cc, 12, dtype=torch.float64, device=pred.device)
    _chk(lib().orbit2_eval_moments(_p(pred), _p(target), target.shape[2], target.shape[3], _p(lat_w), _p(clim), _p(out),
                                   B, Cc, H, W, _stream()), "orbit2_eval_moments")
    return out


# ---- missing-data masks (csrc/masked.hip) --------------------------------------------------------------------------------------
def _mask_args(mask, strides, pred, target):
    """(pointer, row pitch, batch stride, channel stride) of the mask operand: uint8 device bytes whose `strides` =
    (pitch, batch stride, channel stride) address an H x W crop of at least the prediction's size; (None, 0, 0, 0) without one"""
    if mask is None:
        return None, 0, 0, 0
    _dev(mask, torch.uint8, "mask")
    pitch, sb, sc = (int(v) for v in strides)
    B, Cc, H, W = pred.shape
    if pitch < W or sb < 0 or sc < 0 or mask.numel() < (B - 1) * sb + (Cc - 1) * sc + (H - 1) * pitch + W:
        raise HipBackendError("mask of %d bytes does not hold [%d,%d,%d,%d] at pitch %d and strides (%d, %d)"
                              % (mask.numel(), B, Cc, H, W, pitch, sb, sc))
    return mask.data_ptr(), pitch, sb, sc


def masked_loss_fwd(pred, target, lat_w, chan_w, kind, mask=None, mask_strides=(0, 0, 0)):
    """(out fp32 [C+1], cnt int64 [C+1]) over the valid pixels (include/orbit2_hip.h:orbit2_masked_loss_fwd); kind 0 = mse,
    1 = bayesian_tv.  mask: uint8 bytes, mask_strides = (row pitch, batch stride, channel stride), a stride of 0 broadcasts."""
    B, Cc, H, W = _scored_pair("masked_loss_fwd", pred, target, lat_w)
    if chan_w is not None and _dev(chan_w, F32, "chan_w").numel() != Cc:
        raise HipBackendError("masked_loss_fwd: chan_w has %d entries for %d channels" % (chan_w.numel(), Cc))
    mp = _mask_args(mask, mask_strides, pred, target)
    out = torch.empty(Cc + 1, dtype=F32, device=pred.device)
    cnt = torch.empty(Cc + 1, dtype=torch.int64, device=pred.device)
    ws = torch.empty(2 * Cc * B * 64, dtype=F32, device=pred.device)
    _chk(lib().orbit2_masked_loss_fwd(_p(pred), _p(target), target.shape[2], target.shape[3], *mp, _p(lat_w), _p(chan_w),
                                      _p(out), _p(cnt), _p(ws), B, Cc, H, W, kind, _stream()), "orbit2_masked_loss_fwd")
    return out, cnt


def masked_loss_bwd(pred, target, lat_w, chan_w, gscale, cnt, kind, mask=None, mask_strides=(0, 0, 0)):
    """dpred = gscale[0] * d(out[C])/dpred; the divisor cnt[C] (masked_loss_fwd's count) is read on the device"""
    B, Cc, H, W = _scored_pair("masked_loss_bwd", pred, target, lat_w)
    if chan_w is not None and _dev(chan_w, F32, "chan_w").numel() != Cc:
        raise HipBackendError("masked_loss_bwd: chan_w has %d entries for %d channels" % (chan_w.numel(), Cc))
    if _dev(cnt, torch.int64, "cnt").numel() != Cc + 1:
        raise HipBackendError("masked_loss_bwd: cnt must be the [C+1] counts of masked_loss_fwd")
    mp = _mask_args(mask, mask_strides, pred, target)
    dpred = torch.empty_like(pred)
    _chk(lib().orbit2_masked_loss_bwd(_p(pred), _p(target), target.shape[2], target.shape[3], *mp, _p(lat_w), _p(chan_w),
                                      _p(_dev(gscale, F32, "gscale")), _p(cnt), _p(dpred), B, Cc, H, W, kind, _stream()),
         "orbit2_masked_loss_bwd")
    return dpred


def masked_moments(pred, target, lat_w=None, clim=None, mask=None, mask_strides=(0, 0, 0)):
    """[B,C,13] float64: the twelve sums of eval_moments over the valid pixels, then their number
    (include/orbit2_hip.h:orbit2_masked_moments)"""
    B, Cc, H, W = _scored_pair("masked_moments", pred, target, lat_w, clim)
    mp = _mask_args(mask, mask_strides, pred, target)
    out = torch.empty(B, Cc, 13, dtype=torch.float64, device=pred.device)
    _chk(lib().orbit2_masked_moments(_p(pred), _p(target), target.shape[2], target.shape[3], *mp, _p(lat_w), _p(clim), _p(out),
                                     B, Cc, H, W, _stream()), "orbit2_masked_moments")
    return out


def ensemble_update(member, mean, m2, k: int):
    """the k-th (1-based) Welford step of the running ensemble moments, in place on `mean` and `m2`
    (include/orbit2_hip.h:orbit2_ensemble_update); k = 1 initialises them, so they may be torch.empty"""
    _dev(member, F32, "member"); _dev(mean, F32, "mean"); _dev(m2, F32, "m2")
    if mean.shape != member.shape or m2.shape != member.shape:
        raise HipBackendError("ensemble_update: member %s, mean %s and m2 %s must have one shape"
                              % (tuple(member.shape), tuple(mean.shape), tuple(m2.shape)))
    _chk(lib().orbit2_ensemble_update(_p(member), _p(mean), _p(m2), member.numel(), int(k), _stream()),
         "orbit2_ensemble_update")


def gaussian_scores(mean, std, target, lat_w=None):
    """[B,C,4] float64 sums {w crps, w std^2, w (mean - target)^2, 1{|target - mean| <= std}} of a Gaussian prediction
    (include/orbit2_hip.h:orbit2_gaussian_scores); the target may be larger than the prediction (top-left crop)"""
    if _dev(std, F32, "std").shape != mean.shape:
        raise HipBackendError("gaussian_scores: mean %s and std %s differ in shape" % (tuple(mean.shape), tuple(std.shape)))
    B, Cc, H, W = _scored_pair("gaussian_scores", mean, target, lat_w)
    out = torch.empty(B, Cc, 4, dtype=torch.float64, device=mean.device)
    _chk(lib().orbit2_gaussian_scores(_p(mean), _p(std), _p(target), target.shape[2], target.shape[3], _p(lat_w), _p(out),
                                      B, Cc, H, W, _stream()), "orbit2_gaussian_scores")
    return out


ENSEMBLE_MAX_MEMBERS = 64       # ORBIT2_ENSEMBLE_MAX_MEMBERS
ENSEMBLE_MAX_QUANTILES = 16


def ensemble_scores(members, target, lat_w=None, *, sums=True, hist=False, seed=0, crps_field=None, quantiles=None):
    """All-member scores of an [N,B,C,H,W] fp32 ensemble against `target` in one pass (include/orbit2_hip.h:
    orbit2_ensemble_scores).  `members` is a contiguous stack or a view of one whose member stride is larger than a field.
    Returns a dict with the outputs that were asked for: "sums" float64 [B,C,4] (sums=True), "hist" int64 [B,C,N+1] (hist=True;
    `seed` breaks the ties), "crps_field" fp32 [B,C,H,W] (crps_field="empirical" or "fair"), "quantiles" fp32 [Q,B,C,H,W]
    (quantiles = levels in [0, 1], a sequence or a tensor)."""
    if not torch.is_tensor(members) or members.dim() != 5:
        raise HipBackendError("ensemble_scores takes an [N,B,C,H,W] stack of members")
    if not members.is_cuda:
        raise HipBackendError("members must be a GPU tensor (HIP backend has no CPU path)")
    if members.dtype != F32:
        raise HipBackendError("members must be %s, got %s" % (F32, members.dtype))
    N, B, Cc, H, W = members.shape
    if not 2 <= N <= ENSEMBLE_MAX_MEMBERS:
        raise HipBackendError("ensemble_scores: %d members, 2 to %d are served" % (N, ENSEMBLE_MAX_MEMBERS))
    field = B * Cc * H * W
    if not members[0].is_contiguous() or members.stride(0) < field:
        raise HipBackendError("ensemble_scores: every member must be a contiguous [B,C,H,W] field, members at least one field "
                              "apart (strides %s)" % (tuple(members.stride()),))
    _scored_pair("ensemble_scores", members[0], target, lat_w)
    if crps_field not in (None, "empirical", "fair"):
        raise HipBackendError("ensemble_scores: crps_field is None, 'empirical' or 'fair', got %r" % (crps_field,))
    levels = None
    if quantiles is not None:
        levels = torch.as_tensor(quantiles, dtype=F32).reshape(-1)
        if not 1 <= levels.numel() <= ENSEMBLE_MAX_QUANTILES:
            raise HipBackendError("ensemble_scores: %d quantile levels, 1 to %d are served"
                                  % (levels.numel(), ENSEMBLE_MAX_QUANTILES))
        if not bool(((levels >= 0) & (levels <= 1)).all()):
            raise HipBackendError("ensemble_scores: quantile levels must lie in [0, 1]")
        levels = levels.to(members.device).contiguous()
    if not (sums or hist or crps_field or levels is not None):
        raise HipBackendError("ensemble_scores: no output was asked for")
    dev, out = members.device, {}
    if sums:
        out["sums"] = torch.empty(B, Cc, 4, dtype=torch.float64, device=dev)
    if hist:
        out["hist"] = torch.empty(B, Cc, N + 1, dtype=torch.int64, device=dev)
    if crps_field:
        out["crps_field"] = torch.empty(B, Cc, H, W, dtype=F32, device=dev)
    if levels is not None:
        out["quantiles"] = torch.empty(levels.numel(), B, Cc, H, W, dtype=F32, device=dev)
    _chk(lib().orbit2_ensemble_scores(_p(members), members.stride(0), N, _p(target), target.shape[2], target.shape[3], _p(lat_w),
                                      _p(out.get("sums")), _p(out.get("crps_field")), int(crps_field == "fair"),
                                      _p(out.get("hist")), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(out.get("quantiles")), _p(levels),
                                      0 if levels is None else levels.numel(), B, Cc, H, W, _stream()),
         "orbit2_ensemble_scores")
    return out


SSIM_WIN = 7                    # ORBIT2_SSIM_WIN: the only window size built
SSIM_TILE = (32, 64)            # (ORBIT2_SSIM_TILE_H, ORBIT2_SSIM_TILE_W): window centres per workgroup


def ssim_sums(pred, target, lat_w=None, data_range=None, ssim_map=False):
    """[B,C,6] float64 sums {S, lat_w S, (pred - target)^2 over all pixels, target min, target max, data range used} of the
    7 x 7 structural similarity of every (b, c) image (include/orbit2_hip.h:orbit2_ssim); the target may be larger than the
    prediction (top-left crop).  `data_range`: None = max - min of every image's own target crop (found on the device), a
    number, or a tensor that broadcasts to [B,C].  With ssim_map=True returns (sums, map), map fp32 [B,C,H-6,W-6]: S at the
    centres whose window lies inside the image."""
    if pred.dim() == 4 and min(pred.shape[2:]) < SSIM_WIN:           # before the device check: a property of the call
        raise HipBackendError("ssim_sums: the prediction is %d x %d, the window needs at least %d x %d"
                              % (pred.shape[2], pred.shape[3], SSIM_WIN, SSIM_WIN))
    B, Cc, H, W = _scored_pair("ssim_sums", pred, target, lat_w)
    rng = None
    if data_range is not None:
        if torch.is_tensor(data_range):
            rng = data_range.detach().to(device=pred.device, dtype=F32).expand(B, Cc).contiguous()
        else:
            rng = torch.full((B, Cc), float(data_range), dtype=F32, device=pred.device)
    sums = torch.empty(B, Cc, 6, dtype=torch.float64, device=pred.device)
    smap = torch.empty(B, Cc, H - SSIM_WIN + 1, W - SSIM_WIN + 1, dtype=F32, device=pred.device) if ssim_map else None
    _chk(lib().orbit2_ssim(_p(pred), _p(target), target.shape[2], target.shape[3], _p(lat_w), _p(rng), _p(sums), _p(smap),
                           B, Cc, H, W, _stream()), "orbit2_ssim")
    return (sums, smap) if ssim_map else sums


RESAMPLE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}
RESAMPLE_TILE = (32, 256)       # (ORBIT2_RESAMPLE_TILE_H, ORBIT2_RESAMPLE_TILE_W): output pixels per workgroup
RESAMPLE_LDS_FLOATS = 10240     # ORBIT2_RESAMPLE_LDS_FLOATS: the staged source window of a tile


_RESAMPLE_IDX = {}              # (channels, device) -> the validated device int32 copy


def resample_staged(h: int, w: int, H: int, W: int) -> bool:
    """whether orbit2_resample_* stages a tile's source window in LDS at this pair of sizes (the header's rule: the full-tile
    footprint of the ratio fits the budget) or reads the taps from global memory"""
    th, tw = RESAMPLE_TILE
    return (-(-th * h // H) + 4) * (-(-tw * w // W) + 4) <= RESAMPLE_LDS_FLOATS


def _resample_args(x, size, mode, channels, scale, shift, what):
    """the checked operands both resample entries share: (B, Cin, h, w, C, H, W, mode code, chan_idx, scale, shift)"""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise HipBackendError("%s takes an [B,C,h,w] field" % what)
    if mode not in RESAMPLE_MODES:
        raise HipBackendError("%s: mode is one of %s, got %r" % (what, ", ".join(RESAMPLE_MODES), mode))
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise HipBackendError("%s: size is (H, W), got %r" % (what, size)) from None
    B, Cin, h, w = x.shape
    if min(B, Cin, h, w) < 1 or H < 1 or W < 1:
        raise HipBackendError("%s: every size must be positive (x %s, size %s)" % (what, tuple(x.shape), (H, W)))
    idx = None
    Cc = Cin
    if channels is not None:
        chans = [int(c) for c in (channels.tolist() if torch.is_tensor(channels) else channels)]
        if not chans:
            raise HipBackendError("%s: channels is empty" % what)
        bad = [c for c in chans if not 0 <= c < Cin]
        if bad:                                 # the C entry trusts the device copy: this is the only check
            raise HipBackendError("%s: channels %s outside 0..%d" % (what, bad, Cin - 1))
        Cc = len(chans)
    _dev(x, F32, "x")
    if x.requires_grad:
        raise HipBackendError("%s has no backward: x requires grad" % what)
    if channels is not None:
        key = (tuple(chans), str(x.device))     # cached: no host-to-device copy per call (a captured hipGraph forbids one)
        idx = _RESAMPLE_IDX.get(key)
        if idx is None:
            idx = _RESAMPLE_IDX[key] = torch.tensor(chans, dtype=torch.int32, device=x.device)
    if B * Cc > 65535:
        raise HipBackendError("%s: B * C = %d images, at most 65535 are served in one call" % (what, B * Cc))
    if (scale is None) != (shift is None):
        raise HipBackendError("%s: scale and shift are given together or not at all" % what)
    if scale is not None:
        scale = torch.as_tensor(scale, dtype=F32).detach().to(x.device).reshape(-1).contiguous()
        shift = torch.as_tensor(shift, dtype=F32).detach().to(x.device).reshape(-1).contiguous()
        if scale.numel() != Cc or shift.numel() != Cc:
            raise HipBackendError("%s: scale (%d) and shift (%d) need one entry per output channel (%d)"
                                  % (what, scale.numel(), shift.numel(), Cc))
    return B, Cin, h, w, Cc, H, W, RESAMPLE_MODES[mode], idx, scale, shift


def resample(x, size, mode="bilinear", channels=None, scale=None, shift=None, out=None):
    """fp32 [B,C,H,W]: F.interpolate(x[:, channels], size, mode, align_corners=False) * scale[c] + shift[c] in one kernel
    (include/orbit2_hip.h:orbit2_resample_fwd).  mode: nearest, bilinear or bicubic; channels: input channel of every output
    channel (None = all, in order); scale / shift: [C], both or neither; out: a contiguous fp32 [B,C,H,W] to write into."""
    B, Cin, h, w, Cc, H, W, m, idx, scale, shift = _resample_args(x, size, mode, channels, scale, shift, "resample")
    if out is None:
        out = torch.empty(B, Cc, H, W, dtype=F32, device=x.device)
    else:
        _dev(out, F32, "out")
        if tuple(out.shape) != (B, Cc, H, W):
            raise HipBackendError("resample: out is %s, the result %s" % (tuple(out.shape), (B, Cc, H, W)))
    _chk(lib().orbit2_resample_fwd(_p(x), _p(idx), Cin, _p(scale), _p(shift), _p(out), B, Cc, h, w, H, W, m, _stream()),
         "orbit2_resample_fwd")
    return out


def resample_moments(x, size, mode, target, channels=None, scale=None, shift=None, lat_w=None, clim=None):
    """[B,C,12] float64: eval_moments(resample(x, ...), target, lat_w, clim) without the resampled field ever being stored
    (include/orbit2_hip.h:orbit2_resample_moments); the target may be larger than (H, W) (top-left crop)"""
    B, Cin, h, w, Cc, H, W, m, idx, scale, shift = _resample_args(x, size, mode, channels, scale, shift, "resample_moments")
    _scored_pair("resample_moments", (B, Cc, H, W), target, lat_w, clim)
    out = torch.empty(B, Cc, 12, dtype=torch.float64, device=x.device)
    _chk(lib().orbit2_resample_moments(_p(x), _p(idx), Cin, _p(scale), _p(shift), _p(target), target.shape[2], target.shape[3],
                                       _p(lat_w), _p(clim), _p(out), B, Cc, h, w, H, W, m, _stream()),
         "orbit2_resample_moments")
    return out


def seed_salt(value: int, add: bool = False):
    """device-side salt xored into every kernel seed (see include/orbit2_hip.h:orbit2_seed_salt); stream-ordered"""
    _chk(lib().orbit2_seed_salt(value, int(add), _stream()), "orbit2_seed_salt")
