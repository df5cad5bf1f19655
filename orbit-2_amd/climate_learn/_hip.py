"""ctypes binding of liborbit2_hip.so (C ABI in include/orbit2_hip.h).

This is the ONLY compute backend of the package: there is no CPU or eager fallback.  A missing library
or a non-zero return code raises immediately.

Every launch goes through ONE call path, `_call(name, *args)`.  It looks the entry up by the one name
it is given, turns every tensor argument into its address through `_p`, appends torch's current HIP
stream, and raises HipBackendError naming that entry on a non-zero code.  What it guarantees:
  * `_p` is the only place an address is produced, and it refuses a tensor that is not on the device
    (`_on_device`, the one predicate `_dev` and `_dev_rows` ask too): no host pointer crosses the ABI,
    whatever a wrapper forgot;
  * the stream is always the last argument and always the current one;
  * the name in an error message is the entry that was called.
ctypes adds, from PROTOTYPES, that the argument count and kinds are the header's.

What a wrapper must do, since `_call` cannot: pass EVERY tensor its caller supplied through `_dev`
(contiguous), `_dev_rows` (rows contiguous, any row pitch) or their `_opt` forms (None passes) with the
dtype -- or tuple of dtypes -- the entry reads it as, and check the sizes the kernel relies on, BEFORE
the call.  Tensors the wrapper allocated itself need no check.  It hands `_call` tensors, never
addresses, and no stream.  The queries that launch nothing (`*_ws_floats`, `*_is_fixed_order`,
`*_colsum_rows`, `orbit2_abi_version`) are plain `lib().entry(...)` calls.  Two wrappers that differ
in a dtype share one body that takes it as a parameter; a constant of the header is mirrored once
here and pinned by tests/test_abi_cpu.py."""
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


def _on_device(t) -> bool:
    """whether `t` lives in device memory: the one such test of the module (_p, _dev and _dev_rows ask it)"""
    return t.is_cuda


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    """the address of a device tensor (None: NULL) -- the one place a pointer that crosses the ABI is produced"""
    if t is None:
        return None
    if not _on_device(t):
        raise HipBackendError("a pointer operand must be a GPU tensor (HIP backend has no CPU path)")
    return t.data_ptr()


def _chk(rc: int, name: str):
    if rc != 0:
        raise HipBackendError("%s failed with code %d (-1 bad argument, -2 launch error, -3 unsupported)" % (name, rc))


def _call(name: str, *args):
    """the one call path of every launching entry (module docstring): tensors become addresses, the current stream goes last"""
    _chk(getattr(lib(), name)(*[_p(a) if torch.is_tensor(a) else a for a in args], _stream()), name)


def _reads(dtype, t) -> bool:
    """whether an entry that reads `dtype` -- one dtype, or a tuple of those it takes -- reads t's"""
    return t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype


def _dev(t: torch.Tensor, dtype, name: str):
    """a contiguous device tensor of `dtype` (as in _reads)"""
    if not _on_device(t):
        raise HipBackendError("%s must be a GPU tensor (HIP backend has no CPU path)" % name)
    if not _reads(dtype, t):
        raise HipBackendError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise HipBackendError("%s must be contiguous" % name)
    return t


def _dev_rows(t: torch.Tensor, dtype, name: str):
    """an operand handed over with an explicit leading dimension: rows contiguous, any row pitch"""
    if t.dim() == 2 and t.stride(1) == 1 and _on_device(t) and _reads(dtype, t):
        return t
    return _dev(t, dtype, name)


def _dev_opt(t, dtype, name):
    return None if t is None else _dev(t, dtype, name)


def _dev_rows_opt(t, dtype, name):
    return None if t is None else _dev_rows(t, dtype, name)


BF, F32 = torch.bfloat16, torch.float32
I32 = torch.int32
BF_F32 = (BF, F32)              # a gradient sink or a reduction's output: the entry takes a flag that says which


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
    return _p(buf) + 4 * _SCHED_STRIDE * slot


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
    """the (sched_ws, tail) that end a GEMM or attention entry's arguments before the stream: the stream's counter word on `device`
    when a tail queue is asked for (tail >= 0), NULL for a static call -- which so never allocates the counter buffer or claims a
    slot"""
    return (_sched_word(device) if tail >= 0 else None), tail


# ------------------------------------------------------------------------------------------------
def _gemm_fill(a, A, B, out, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, bias=None, act=0, save_pre=None,
               dgelu_pre=None, drop_p=0.0, seed=0, rowscale=None, rows_per_scale=0, residual=None, ldr=0, res_mod=0,
               res_first=False, beta=0.0, tile=0, colscale=None, save_dact=None, mul=None):
    for t, nm in ((A, "A"), (B, "B")):
        _dev_rows(t, BF, nm)
    if out.dtype not in BF_F32 or not _on_device(out):
        raise HipBackendError("gemm out must be a bf16/fp32 GPU tensor")
    a.A, a.B, a.C = _p(A), _p(B), _p(out)
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc = M, N, K, lda, ldb, ldc
    a.a_kc, a.b_kc = int(a_kc), int(b_kc)
    a.bias = _p(_dev_opt(bias, BF, "bias"))
    a.act = act
    a.save_pre = _p(_dev_rows_opt(save_pre, BF, "save_pre"))            # row pitch = ldc
    a.dgelu_pre = _p(_dev_rows_opt(dgelu_pre, BF, "dgelu_pre"))         # row pitch = ldc
    a.drop_p, a.seed = float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF
    a.rowscale = _p(_dev_opt(rowscale, F32, "rowscale"))
    a.rows_per_scale = rows_per_scale
    a.residual = _p(_dev_opt(residual, BF, "residual"))
    a.ldr, a.res_mod, a.res_first = ldr, res_mod, int(res_first)
    a.out_fp32 = int(out.dtype == F32)
    a.beta = float(beta)
    a.tile_hint = int(tile)
    a.colscale_n, a.colscale = (0, 1.0) if colscale is None else (int(colscale[0]), float(colscale[1]))
    a.save_dact = _p(_dev_rows_opt(save_dact, torch.int16, "save_dact"))    # int16 q14, row pitch = ldc
    a.mul = _p(_dev_rows_opt(mul, torch.int16, "mul"))                      # int16 q14, row pitch = ldc
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
            a.colsum_ws = _p(parts)
    with _timed("gemm_bf16", flops, nbytes):
        _call("orbit2_gemm_bf16", C.byref(a), gate, rows_per_gate if gate is not None else 0, *_queue(tail, out.device))
    return (out, parts) if want_colsum else out


def gemm_f32(A, B, out, M, N, K, lda, ldb, ldc, bias=None, act=0, residual=None, ldr=0, res_mod=0, res_first=False, beta=0.0,
             tile=0, colscale=None):
    """out[M,N] = epilogue(A x B^T) in fp32 (include/orbit2_hip.h:orbit2_gemm_f32): A [M][lda], B [N][ldb] the fp32 weight as
    stored, every tensor fp32; forward form and forward epilogue only"""
    for t, nm in ((A, "A"), (B, "B"), (out, "out")):
        _dev_rows(t, F32, nm)
    a = GemmArgs()
    a.A, a.B, a.C = _p(A), _p(B), _p(out)
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc = M, N, K, lda, ldb, ldc
    a.a_kc = a.b_kc = 1
    a.bias = _p(_dev_opt(bias, F32, "bias"))
    a.act = act
    a.residual = _p(_dev_rows_opt(residual, F32, "residual"))
    a.ldr, a.res_mod, a.res_first = ldr, res_mod, int(res_first)
    a.out_fp32 = 1
    a.beta = float(beta)
    a.tile_hint = int(tile)
    a.colscale_n, a.colscale = (0, 1.0) if colscale is None else (int(colscale[0]), float(colscale[1]))
    with _timed("gemm_f32", 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N)):
        _call("orbit2_gemm_f32", C.byref(a))
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
            kgates[i], kper[i], gated = _p(vec), per, True
        f, b = _gemm_fill(arr[i], A, B, out, M, N, K, lda, ldb, ldc, **kw)
        flops += f
        nbytes += b

    with _timed("gemm_bf16", flops, nbytes):
        _call("orbit2_gemm_bf16_grouped", arr, n, kgates if gated else None, kper if gated else None,
              *_queue(tail, problems[0][2].device))


def sgemm(A, B, out, M, N, K, lda, ldb, ldc, ta=False, tb=False, alpha=1.0, beta=0.0):
    for t, nm in ((A, "A"), (B, "B"), (out, "C")):
        _dev(t, F32, nm)
    n = lib().orbit2_sgemm_f32_ws_floats(M, N, K)
    ws = torch.empty(n, dtype=F32, device=out.device) if n else None
    _call("orbit2_sgemm_f32_ws", A, B, out, M, N, K, lda, ldb, ldc, int(ta), int(tb), alpha, beta, ws, n)
    return out


def _layernorm_fwd(dtype, x, gamma, beta, eps, out, stats):
    """LayerNorm forward in `dtype` (BF: orbit2_layernorm_fwd_ld, F32: orbit2_layernorm_fwd_f32): (y, mean, rstd), the statistics
    None unless `stats`"""
    _dev(x, dtype, "x"); _dev(gamma, dtype, "gamma"); _dev(beta, dtype, "beta")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x) if out is None else _dev_rows(out, dtype, "out")
    ldy = D if out is None else y.stride(0)
    mean = torch.empty(rows, dtype=F32, device=x.device) if stats else None
    rstd = torch.empty(rows, dtype=F32, device=x.device) if stats else None
    _call("orbit2_layernorm_fwd_ld" if dtype == BF else "orbit2_layernorm_fwd_f32", x, gamma, beta, y, mean, rstd, rows, D, ldy, eps)
    return y, mean, rstd


def layernorm_fwd(x, gamma, beta, eps=1e-5, out=None):
    """out: optional [rows, D] bf16 destination with any row pitch (a view of a padded buffer: orbit2_layernorm_fwd_ld)"""
    return _layernorm_fwd(BF, x, gamma, beta, eps, out, True)


def layernorm_fwd_f32(x, gamma, beta, eps=1e-5, out=None, stats=False):
    """fp32 LayerNorm (orbit2_layernorm_fwd_f32); returns y, or (y, mean, rstd) with stats=True"""
    res = _layernorm_fwd(F32, x, gamma, beta, eps, out, stats)
    return res if stats else res[0]


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, beta_acc=0.0):
    """dgamma / dbeta: the two gradient sinks, both bf16 or both fp32 (the entry takes one flag for the pair); dres: bf16 or None"""
    _dev(dy, BF, "dy"); _dev(x, BF, "x"); _dev(gamma, BF, "gamma")
    _dev(mean, F32, "mean"); _dev(rstd, F32, "rstd"); _dev_opt(dres, BF, "dres")
    _dev(dgamma, BF_F32, "dgamma"); _dev(dbeta, dgamma.dtype, "dbeta")
    D = x.shape[-1]
    rows = x.numel() // D
    dx = torch.empty_like(x)
    n = lib().orbit2_layernorm_bwd_ws_floats(rows, D)
    ws = torch.empty(n, dtype=F32, device=x.device)
    _call("orbit2_layernorm_bwd", dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, int(dgamma.dtype == F32), beta_acc, ws, n,
          rows, D)
    return dx


ATTN_4WAVES, ATTN_SPLIT_DKV, ATTN_Q_PRESCALED, ATTN_NO_W4 = 1, 2, 4, 8      # include/orbit2_hip.h: the kernel-variant flags of the attention entries (A/B, tests)


def probe_read(buf, blocks, inflight, sink):
    """diagnostic calibration stream (include/orbit2_hip.h: orbit2_probe_read)"""
    _dev(buf, F32, "buf"); _dev(sink, F32, "sink")
    _call("orbit2_probe_read", buf, buf.numel() * buf.element_size(), int(blocks), int(inflight), sink)


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


def _attn_fwd(dtype, qkv, B, L, H, d, drop_p, seed, flags, out, gate=None, tail=-1):
    """the attention forward in `dtype`: BF = orbit2_attn_fwd_ld (seed, gate and tail queue), F32 = orbit2_attn_fwd_f32 (none of
    them).  qkv [B * L, 3 * H * d] with a token-row pitch, or contiguous; out likewise, default [B, L, H * d]"""
    _dev_rows(qkv, dtype, "qkv")
    ldq = qkv.stride(0) if qkv.dim() == 2 else 3 * H * d
    if out is None:
        out, ldo = torch.empty(B, L, H * d, dtype=dtype, device=qkv.device), H * d
    else:
        out = _dev_rows(out, dtype, "out")
        ldo = out.stride(0)
    lse = torch.empty(B, H, L, dtype=F32, device=qkv.device)
    name, ends = ("attn_fwd", (gate,) + _queue(tail, qkv.device)) if dtype == BF else ("attn_fwd_f32", ())
    # algorithmic bytes: qkv read once, out + lse written once
    with _timed(name, 4.0 * B * H * L * L * d, qkv.element_size() * 4.0 * B * L * H * d + 4.0 * B * H * L):
        _call("orbit2_attn_fwd_ld" if dtype == BF else "orbit2_attn_fwd_f32", qkv, out, lse, B, L, H, d, drop_p, seed, int(flags),
              int(ldq), int(ldo), *ends)
    return out, lse


def attn_fwd(qkv, B, L, H, d, drop_p=0.0, seed=0, flags=0, out=None, gate=None, tail_queue=None):
    """out: optional [B * L, H * d] bf16 destination with any token-row pitch (orbit2_attn_fwd_ld); default [B, L, H * d].
    gate: fp32 [B] path gate: out and lse of a sample whose entry is 0.0 may be stored as zeros
    tail_queue: as in gemm"""
    tail = _tail_arg(tail_queue)
    return _attn_fwd(BF, qkv, B, L, H, d, drop_p, seed, flags, out, _attn_gate(gate, B), tail)


def attn_fwd_f32(qkv, B, L, H, d, drop_p=0.0, flags=0, out=None):
    """fp32 attention core (orbit2_attn_fwd_f32): qkv fp32 [B * L, 3 * H * d] (any token-row pitch) or contiguous
    [B, L, 3, H, d]; returns (out [B, L, H * d] fp32 or the given `out`, lse [B, H, L])"""
    return _attn_fwd(F32, qkv, B, L, H, d, drop_p, 0, flags, out)


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
        _call("orbit2_attn_bwd_ld", qkv, out, dout, lse, delta, dqkv, B, L, H, d, drop_p, seed, int(flags), int(ldq), int(ldo), gate,
              *_queue(tail, qkv.device))
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


def _varagg_fwd(zdtype, x, stab, gtab, H, D, want_attw):
    """the folded variable aggregation with tokens in `zdtype` (BF: orbit2_varagg_fwd_p, F32: orbit2_varagg_fwd_f32_p): (z, attw).
    Every patch size goes through the _p entries: at patch 2 they are the plain entries' own code (include/orbit2_hip.h)"""
    _dev(x, F32, "x"); _dev(stab, F32, "stab"); _dev(gtab, F32, "gtab")
    B, V, h, w, p, ntok = _varagg_shapes(x, gtab, stab)
    z = torch.empty(ntok, D, dtype=zdtype, device=x.device)
    attw = torch.empty(ntok, H, V, dtype=F32, device=x.device) if want_attw else None
    _call("orbit2_varagg_fwd_p" if zdtype == BF else "orbit2_varagg_fwd_f32_p", x, stab, gtab, z, attw, B, V, h, w, p, H, D)
    return z, attw


def varagg_fwd(x, stab, gtab, H, D):
    """z bf16 [tokens, D], attw fp32 [tokens, H, V]; the patch size is the tables': stab [H, V, p*p+1], gtab [V, p*p+1, D]"""
    return _varagg_fwd(BF, x, stab, gtab, H, D, True)


def varagg_fwd_f32(x, stab, gtab, H, D, want_attw=False):
    """the folded variable aggregation with fp32 tokens (orbit2_varagg_fwd_f32_p); returns z, or (z, attw) with want_attw"""
    z, attw = _varagg_fwd(F32, x, stab, gtab, H, D, want_attw)
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
    """(dstab, dgtab) through orbit2_varagg_bwd_p at every patch size.  A shape the entry does not serve (workspace query 0) is
    refused; a served one whose sums are not in a fixed order (the atomics fallback, which exists at patch 2 only) sets
    `atomics_in_grad_path`"""
    global atomics_in_grad_path
    _dev(x, F32, "x"); _dev(gtab, F32, "gtab"); _dev(attw, F32, "attw"); _dev(dz, BF, "dz")
    B, V, h, w, p, ntok = _varagg_shapes(x, gtab)
    C_ = p * p + 1
    dstab = torch.zeros(H, V, C_, dtype=F32, device=x.device)
    dgtab = torch.zeros(V, C_, D, dtype=F32, device=x.device)
    fixed = lib().orbit2_varagg_bwd_p_is_fixed_order(B, V, h, w, p, H, D)
    n = lib().orbit2_varagg_bwd_p_ws_floats(B, V, h, w, p, H, D)
    if n <= 0:
        raise HipBackendError("orbit2_varagg_bwd_p does not serve B=%d V=%d grid %dx%d patch %d H=%d D=%d (its LDS need "
                              "exceeds a CU's 160 KiB, or the shape is invalid)" % (B, V, h, w, p, H, D))
    if not fixed:
        atomics_in_grad_path = True
    ws = torch.empty(n, dtype=F32, device=x.device)
    _call("orbit2_varagg_bwd_p", x, gtab, attw, dz, dstab, dgtab, B, V, h, w, p, H, D, ws)
    return dstab, dgtab


def tables_gather(w0, w_stride, b0, b_stride, var_embed, ids, V, D):
    """cmat [5 V, D] fp32 from the per-variable patch-embed parameters laid out at a uniform pitch (w0 / b0 = parameter 0)"""
    _dev(w0, F32, "token_embeds.0.proj.weight"); _dev(b0, F32, "token_embeds.0.proj.bias"); _dev(var_embed, F32, "var_embed")
    _dev(ids, I32, "ids")
    cmat = torch.empty(5 * V, D, dtype=F32, device=w0.device)
    _call("orbit2_tables_gather", w0, w_stride, b0, b_stride, var_embed, ids, cmat, V, D)
    return cmat


def tables_scatter(dcmat, gw0, w_stride, gb0, b_stride, gvar_embed, ids, V, D):
    """accumulates the rows' gradient into the parameters' gradient buffers (same pitches)"""
    _dev(dcmat, F32, "dcmat"); _dev(gw0, F32, "dW"); _dev(gb0, F32, "db"); _dev(gvar_embed, F32, "dvar_embed")
    _dev(ids, I32, "ids")
    _call("orbit2_tables_scatter", dcmat, gw0, w_stride, gb0, b_stride, gvar_embed, ids, V, D)


def dropout_bwd(dy, M, N, drop_p, seed, rowscale=None, rows_per_scale=0, out=None):
    _dev(dy, BF, "dy"); _dev_opt(rowscale, F32, "rowscale")
    out = torch.empty_like(dy) if out is None else _dev(out, BF, "out")
    _call("orbit2_dropout_bwd", dy, out, M, N, drop_p, seed, rowscale, rows_per_scale)
    return out


def dropout_bwd_colsum(dy, M, N, drop_p, seed, rowscale, rows_per_scale, colsum_out, beta=0.0):
    """dym = dy * dropmask * rowscale and colsum_out[n] (+)= sum_m dym[m][n] in one pass"""
    _dev(dy, BF, "dy"); _dev_opt(rowscale, F32, "rowscale"); _dev(colsum_out, BF_F32, "colsum_out")
    out = torch.empty_like(dy)
    n = lib().orbit2_colsum_ws_floats(M, N)
    ws = torch.empty(n, dtype=F32, device=dy.device)
    _call("orbit2_dropout_bwd_colsum", dy, out, M, N, drop_p, seed, rowscale, rows_per_scale, colsum_out,
          int(colsum_out.dtype == F32), beta, ws, n)
    return out


def post_reduce(x, M, N, addend=None, res_mod=0, residual=None, drop_p=0.0, seed=0, rowscale=None, rows_per_scale=0,
                out=None):
    """y = residual + rowscale * dropout(x + addend[m % res_mod]); in place on x unless `out` is given"""
    _dev(x, BF, "x"); _dev_opt(addend, BF, "addend"); _dev_opt(residual, BF, "residual"); _dev_opt(rowscale, F32, "rowscale")
    out = x if out is None else _dev(out, BF, "out")
    _call("orbit2_post_reduce", x, addend, res_mod, residual, out, M, N, drop_p, seed, rowscale, rows_per_scale)
    return out


def colsum(x, M, N, ldx, out, beta=0.0):
    """out[n] = beta * out[n] + sum_m x[m][n]; x bf16 or fp32 with rows ldx apart (a padded view, or the padded buffer itself)"""
    _dev_rows(x, BF_F32, "x"); _dev(out, BF_F32, "out")
    n = lib().orbit2_colsum_ws_floats(M, N)
    ws = torch.empty(n, dtype=F32, device=x.device)
    _call("orbit2_colsum", x, int(x.dtype == F32), M, N, ldx, out, int(out.dtype == F32), beta, ws, n)
    return out


def batch_sum(x, B, rows, N, out, beta=0.0):
    _dev(x, BF, "x"); _dev(out, BF_F32, "out")
    _call("orbit2_batch_sum", x, out, B, rows, N, int(out.dtype == F32), beta)
    return out


def _cast(name, to, src, dst):
    """dst (default: a new tensor of src's shape) = src in the dtype `to`; the entry `name` reads the other of bf16 / fp32"""
    _dev(src, F32 if to == BF else BF, "src")
    dst = torch.empty(src.shape, dtype=to, device=src.device) if dst is None else _dev(dst, to, "dst")
    _call(name, src, dst, src.numel())
    return dst


def cast_to_bf16(src, dst=None):
    return _cast("orbit2_cast_f32_to_bf16", BF, src, dst)


def cast_to_f32(src, dst=None):
    return _cast("orbit2_cast_bf16_to_f32", F32, src, dst)


def add_rowvec(a, vec, rows, N):
    _dev(a, BF, "a"); _dev(vec, BF, "vec")
    y = torch.empty_like(a)
    _call("orbit2_add_rowvec", a, vec, y, rows, N)
    return y


def posembed_fwd(pe, sw, sb, res, oh, ow, nh, nw):
    """[nh*nw, D] fp32 = bicubic re-grid of the [oh*ow, D] table (identity when oh == nh) + sw * res + sb"""
    _dev(pe, F32, "pos_embed"); _dev_opt(sw, F32, "spatial_embed.weight"); _dev_opt(sb, F32, "spatial_embed.bias")
    D = pe.shape[-1]
    out = torch.empty(nh * nw, D, dtype=F32, device=pe.device)
    _call("orbit2_posembed_fwd", pe, sw, sb, res, out, oh, ow, nh, nw, D)
    return out


def posembed_bwd(dout, oh, ow, nh, nw):
    _dev(dout, F32, "dposres")
    D = dout.shape[-1]
    dpe = torch.empty(oh * ow, D, dtype=F32, device=dout.device)
    _call("orbit2_posembed_bwd", dout, dpe, oh, ow, nh, nw, D)
    return dpe


def _unpatchify_fwd(dtype, t, B, Cc, h, w, p, s):
    """tokens in `dtype` (BF: orbit2_unpatchify_fwd, F32: orbit2_unpatchify_fwd_f32) -> the fp32 image"""
    _dev(t, dtype, "t")
    img = torch.empty(B, Cc, h * s, w * s, dtype=F32, device=t.device)
    _call("orbit2_unpatchify_fwd" if dtype == BF else "orbit2_unpatchify_fwd_f32", t, img, B, Cc, h, w, p, s)
    return img


def unpatchify_fwd(t, B, Cc, h, w, p, s):
    return _unpatchify_fwd(BF, t, B, Cc, h, w, p, s)


def unpatchify_fwd_f32(t, B, Cc, h, w, p, s):
    return _unpatchify_fwd(F32, t, B, Cc, h, w, p, s)


def unpatchify_bwd(dimg, B, Cc, h, w, p, s):
    _dev(dimg, F32, "dimg")
    L = h * w // (p * p)
    dt = torch.empty(B, L, Cc * (s * p) ** 2, dtype=BF, device=dimg.device)
    _call("orbit2_unpatchify_bwd", dimg, dt, B, Cc, h, w, p, s)
    return dt


def conv3x3_fwd(x, chan_idx, weight, bias, mode=0, r=1, addend=None):
    _dev(x, F32, "in"); _dev_opt(chan_idx, I32, "chan_idx"); _dev(weight, F32, "weight"); _dev(bias, F32, "bias")
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
    _call("orbit2_conv3x3_fwd", x, chan_idx, ctot, weight, bias, out, pre, addend, Ha, Wa, B, Cin, Cout, H, W, mode, r)
    return out, pre


def conv3x3_bwd(dout, x, chan_idx, weight, pre, need_din, mode=0, r=1):
    _dev(dout, F32, "dout"); _dev(x, F32, "in"); _dev_opt(chan_idx, I32, "chan_idx"); _dev(weight, F32, "weight")
    _dev_opt(pre, F32, "pre")
    B, ctot, H, W = x.shape
    Cout, Cin = weight.shape[0], weight.shape[1]
    din = torch.empty(B, Cin, H, W, dtype=F32, device=x.device) if need_din else None
    dw = torch.zeros_like(weight)
    db = torch.zeros(Cout, dtype=F32, device=x.device)
    ws = _ws(lib().orbit2_conv3x3_bwd_ws_floats, (B, Cin, Cout, H, W), x.device)
    _call("orbit2_conv3x3_bwd", dout, x, chan_idx, ctot, weight, pre, din, dw, db, B, Cin, Cout, H, W, mode, r, ws)
    return din, dw, db


def clamp_channel_(img, chan):
    _dev(img, F32, "img")
    B, Cc, H, W = img.shape
    _call("orbit2_clamp_channel", img, B, Cc, H * W, chan)
    return img


def clamp_channel_bwd_(img_clamped, dimg, chan):
    _dev(img_clamped, F32, "img"); _dev(dimg, F32, "dimg")
    B, Cc, H, W = img_clamped.shape
    _call("orbit2_clamp_channel_bwd", img_clamped, dimg, B, Cc, H * W, chan)
    return dimg


LOSS_BLOCKS = 64                # ORBIT2_LOSS_BLOCKS: the partial sums per (b, c) plane of the two loss forwards


def _loss_ws(B, Cc, device):
    """the fp32 workspace of orbit2_loss_fwd and orbit2_masked_loss_fwd: two partials per block of every (b, c) plane"""
    return torch.empty(2 * Cc * B * LOSS_BLOCKS, dtype=F32, device=device)


def _loss_pair(name, pred, target, lat_w, chan_w):
    """(B, C, H, W) of a loss wrapper's operands: the scored pair's checks, and chan_w fp32 with one entry per channel or None"""
    B, Cc, H, W = _scored_pair(name, pred, target, lat_w)
    if chan_w is not None and _dev(chan_w, F32, "chan_w").numel() != Cc:
        raise HipBackendError("%s: chan_w has %d entries for %d channels" % (name, chan_w.numel(), Cc))
    return B, Cc, H, W


def loss_fwd(pred, target, lat_w, chan_w, kind):
    B, Cc, H, W = _loss_pair("loss_fwd", pred, target, lat_w, chan_w)
    out = torch.empty(Cc + 1, dtype=F32, device=pred.device)
    ws = _loss_ws(B, Cc, pred.device)
    _call("orbit2_loss_fwd", pred, target, target.shape[2], target.shape[3], lat_w, chan_w, out, ws, B, Cc, H, W, kind)
    return out


def loss_bwd(pred, target, lat_w, chan_w, gscale, kind):
    B, Cc, H, W = _loss_pair("loss_bwd", pred, target, lat_w, chan_w)
    _dev(gscale, F32, "gscale")
    dpred = torch.empty_like(pred)
    _call("orbit2_loss_bwd", pred, target, target.shape[2], target.shape[3], lat_w, chan_w, gscale, dpred, B, Cc, H, W, kind)
    return dpred


def adamw(p, m, v, g, p16, n, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, found_inf=None):
    _dev(p, F32, "p"); _dev(m, F32, "m"); _dev(v, F32, "v")
    _dev(g, BF_F32, "g"); _dev_opt(p16, BF, "p16"); _dev_opt(found_inf, F32, "found_inf")
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _call("orbit2_adamw", p, m, v, g, int(g.dtype == F32), p16, n, lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale, found_inf)


def check_finite(g, n, found_inf):
    _dev(g, BF_F32, "g"); _dev(found_inf, F32, "found_inf")
    _call("orbit2_check_finite", g, int(g.dtype == F32), n, found_inf)


def selftest(device="cuda") -> int:
    buf = torch.zeros(512, dtype=torch.int32, device=device)
    _call("orbit2_selftest", buf)
    torch.cuda.synchronize()
    return int(buf[0].item())


def droppath_scales(B, p, seed, device):
    out = torch.empty(B, dtype=F32, device=device)
    _call("orbit2_droppath_scales", out, B, p, seed)
    return out


def transpose_bf16(src, dst):
    _dev(src, BF, "src"); _dev(dst, BF, "dst")
    R, Cc = src.shape
    _call("orbit2_transpose_bf16", src, dst, R, Cc)
    return dst


# ---- perceptual loss building blocks (csrc/lpips.hip) ----------------------------------------------------------
# The entries take N, H, W, C from the caller and index with them: every wrapper compares them with the tensors it hands over
# first, so a wrong argument is refused here instead of reading or writing past a buffer.
def _holds(t, n, name, at_least=False):
    """a tensor of exactly (at_least: no fewer than) n elements; None (an optional operand) passes"""
    if t is not None and (t.numel() < n if at_least else t.numel() != n):
        raise HipBackendError("%s holds %d elements, the sizes given need %s%d" % (name, t.numel(), "at least " if at_least else "", n))


def _nhwc_dims(name, N, H, W, Cc, pool=False):
    if min(N, H, W, Cc) <= 0 or Cc % 8:
        raise HipBackendError("%s needs positive N, H, W and a positive multiple of 8 for C, got %r" % (name, (N, H, W, Cc)))
    if pool and (H % 2 or W % 2):
        raise HipBackendError("%s needs even H and W, got %d x %d" % (name, H, W))


def _image_dims(name, img):
    """N, H, W of an [N,3,H,W] image"""
    if img.dim() != 4 or img.shape[1] != 3 or img.numel() == 0:
        raise HipBackendError("%s takes a non-empty [N,3,H,W] image, got %s" % (name, tuple(img.shape)))
    return img.shape[0], img.shape[2], img.shape[3]


def _tap_dims(name, feats, lin, B, HW, Cc):
    if B <= 0 or HW <= 0 or Cc not in (64, 128, 256, 512):
        raise HipBackendError("%s needs positive B and HW and C in {64, 128, 256, 512}, got %r" % (name, (B, HW, Cc)))
    _holds(feats, 2 * B * HW * Cc, "feats"); _holds(lin, Cc, "lin")


def im2col3x3(x, N, H, W, Cc):
    _dev(x, BF, "x")
    _nhwc_dims("im2col3x3", N, H, W, Cc); _holds(x, N * H * W * Cc, "x")
    col = torch.empty(N * H * W, 9 * Cc, dtype=BF, device=x.device)
    _call("orbit2_im2col3x3", x, col, N, H, W, Cc)
    return col


def col2im3x3(dcol, N, H, W, Cc, act=None, tapg=None):
    _dev(dcol, BF, "dcol"); _dev_opt(act, BF, "act"); _dev_opt(tapg, BF, "tapg")
    _nhwc_dims("col2im3x3", N, H, W, Cc)
    if tapg is not None and act is None:
        raise HipBackendError("col2im3x3 adds tapg only under the ReLU mask: tapg needs act")
    _holds(dcol, N * H * W * 9 * Cc, "dcol"); _holds(act, N * H * W * Cc, "act"); _holds(tapg, N * H * W * Cc, "tapg")
    out = torch.empty(N * H * W, Cc, dtype=BF, device=dcol.device)
    _call("orbit2_col2im3x3", dcol, act, tapg, out, N, H, W, Cc)
    return out


def maxpool2_fwd(x, N, H, W, Cc):
    _dev(x, BF, "x")
    _nhwc_dims("maxpool2_fwd", N, H, W, Cc, pool=True); _holds(x, N * H * W * Cc, "x")
    y = torch.empty(N * (H // 2) * (W // 2), Cc, dtype=BF, device=x.device)
    _call("orbit2_maxpool2_fwd", x, y, N, H, W, Cc)
    return y


def maxpool2_bwd(g, x, N, H, W, Cc, tapg=None):
    _dev(g, BF, "g"); _dev(x, BF, "x"); _dev_opt(tapg, BF, "tapg")
    _nhwc_dims("maxpool2_bwd", N, H, W, Cc, pool=True)
    _holds(g, N * (H // 2) * (W // 2) * Cc, "g"); _holds(x, N * H * W * Cc, "x"); _holds(tapg, N * H * W * Cc, "tapg")
    dz = torch.empty(N * H * W, Cc, dtype=BF, device=g.device)
    _call("orbit2_maxpool2_bwd", g, x, tapg, dz, N, H, W, Cc)
    return dz


def lpips_conv1_fwd(img, w1, b1):
    _dev(img, F32, "img"); _dev(w1, F32, "w1"); _dev(b1, F32, "b1")
    N, H, W = _image_dims("lpips_conv1_fwd", img)
    _holds(w1, 27 * 64, "w1"); _holds(b1, 64, "b1")
    out = torch.empty(N * H * W, 64, dtype=BF, device=img.device)
    _call("orbit2_lpips_conv1_fwd", img, w1, b1, out, N, H, W)
    return out


def lpips_conv1_bwd(dz, w1, pred, target, l1_coef, gscale=None):
    _dev(dz, BF, "dz"); _dev(w1, F32, "w1"); _dev(pred, F32, "pred"); _dev(target, F32, "target"); _dev_opt(gscale, F32, "gscale")
    N, H, W = _image_dims("lpips_conv1_bwd", pred)
    if target.shape != pred.shape:
        raise HipBackendError("lpips_conv1_bwd: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    _holds(dz, N * H * W * 64, "dz"); _holds(w1, 27 * 64, "w1"); _holds(gscale, 1, "gscale", at_least=True)
    dimg = torch.empty_like(pred)
    _call("orbit2_lpips_conv1_bwd", dz, w1, pred, target, l1_coef, gscale, dimg, N, H, W)
    return dimg


def lpips_tap_fwd(feats, lin, val, B, HW, Cc):
    _dev(feats, BF, "feats"); _dev(lin, F32, "lin"); _dev(val, F32, "val")
    _tap_dims("lpips_tap_fwd", feats, lin, B, HW, Cc); _holds(val, B, "val", at_least=True)
    ws = _ws(lib().orbit2_lpips_tap_ws_floats, (B, HW, Cc), feats.device)
    _call("orbit2_lpips_tap_fwd", feats, lin, val, B, HW, Cc, ws)


def lpips_tap_bwd(feats, lin, coef, B, HW, Cc, gscale=None):
    _dev(feats, BF, "feats"); _dev(lin, F32, "lin"); _dev_opt(gscale, F32, "gscale")
    _tap_dims("lpips_tap_bwd", feats, lin, B, HW, Cc); _holds(gscale, 1, "gscale", at_least=True)
    g = torch.empty(B * HW, Cc, dtype=BF, device=feats.device)
    _call("orbit2_lpips_tap_bwd", feats, lin, g, coef, gscale, B, HW, Cc)
    return g


def l1_mean(a, b, out):
    _dev(a, F32, "a"); _dev(b, F32, "b"); _dev(out, F32, "out")
    if a.numel() == 0:
        raise HipBackendError("l1_mean of no elements")
    _holds(b, a.numel(), "b"); _holds(out, 1, "out", at_least=True)
    ws = _ws(lib().orbit2_l1_mean_ws_floats, (a.numel(),), a.device)
    _call("orbit2_l1_mean", a, b, out, a.numel(), ws)


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
    _call("orbit2_eval_moments", pred, target, target.shape[2], target.shape[3], lat_w, clim, out, B, Cc, H, W)
    return out


# ---- missing-data masks (csrc/loss.hip) ----------------------------------------------------------------------------------------
def _mask_args(mask, strides, pred, target):
    """(mask, row pitch, batch stride, channel stride) of the mask operand: uint8 device bytes whose `strides` =
    (pitch, batch stride, channel stride) address an H x W crop of at least the prediction's size; (None, 0, 0, 0) without one"""
    if mask is None:
        return None, 0, 0, 0
    _dev(mask, torch.uint8, "mask")
    pitch, sb, sc = (int(v) for v in strides)
    B, Cc, H, W = pred.shape
    if pitch < W or sb < 0 or sc < 0 or mask.numel() < (B - 1) * sb + (Cc - 1) * sc + (H - 1) * pitch + W:
        raise HipBackendError("mask of %d bytes does not hold [%d,%d,%d,%d] at pitch %d and strides (%d, %d)"
                              % (mask.numel(), B, Cc, H, W, pitch, sb, sc))
    return mask, pitch, sb, sc


def masked_loss_fwd(pred, target, lat_w, chan_w, kind, mask=None, mask_strides=(0, 0, 0)):
    """(out fp32 [C+1], cnt int64 [C+1]) over the valid pixels (include/orbit2_hip.h:orbit2_masked_loss_fwd); kind 0 = mse,
    1 = bayesian_tv.  mask: uint8 bytes, mask_strides = (row pitch, batch stride, channel stride), a stride of 0 broadcasts."""
    B, Cc, H, W = _loss_pair("masked_loss_fwd", pred, target, lat_w, chan_w)
    mp = _mask_args(mask, mask_strides, pred, target)
    out = torch.empty(Cc + 1, dtype=F32, device=pred.device)
    cnt = torch.empty(Cc + 1, dtype=torch.int64, device=pred.device)
    ws = _loss_ws(B, Cc, pred.device)
    _call("orbit2_masked_loss_fwd", pred, target, target.shape[2], target.shape[3], *mp, lat_w, chan_w, out, cnt, ws, B, Cc, H, W,
          kind)
    return out, cnt


def masked_loss_bwd(pred, target, lat_w, chan_w, gscale, cnt, kind, mask=None, mask_strides=(0, 0, 0)):
    """dpred = gscale[0] * d(out[C])/dpred; the divisor cnt[C] (masked_loss_fwd's count) is read on the device"""
    B, Cc, H, W = _loss_pair("masked_loss_bwd", pred, target, lat_w, chan_w)
    if _dev(cnt, torch.int64, "cnt").numel() != Cc + 1:
        raise HipBackendError("masked_loss_bwd: cnt must be the [C+1] counts of masked_loss_fwd")
    mp = _mask_args(mask, mask_strides, pred, target)
    _dev(gscale, F32, "gscale")
    dpred = torch.empty_like(pred)
    _call("orbit2_masked_loss_bwd", pred, target, target.shape[2], target.shape[3], *mp, lat_w, chan_w, gscale, cnt, dpred,
          B, Cc, H, W, kind)
    return dpred


def masked_moments(pred, target, lat_w=None, clim=None, mask=None, mask_strides=(0, 0, 0)):
    """[B,C,13] float64: the twelve sums of eval_moments over the valid pixels, then their number
    (include/orbit2_hip.h:orbit2_masked_moments)"""
    B, Cc, H, W = _scored_pair("masked_moments", pred, target, lat_w, clim)
    mp = _mask_args(mask, mask_strides, pred, target)
    out = torch.empty(B, Cc, 13, dtype=torch.float64, device=pred.device)
    _call("orbit2_masked_moments", pred, target, target.shape[2], target.shape[3], *mp, lat_w, clim, out, B, Cc, H, W)
    return out


# ---- extreme-value scores (csrc/extremes.hip): two further kinds of orbit2_masked_loss_fwd ------------------------------------
MASKED_QUANTILES, MASKED_TAIL = 3, 4            # ORBIT2_MASKED_QUANTILES, ORBIT2_MASKED_TAIL: the kind proper (bits 0-3)
MASKED_PER_IMAGE, MASKED_LOWER = 16, 32         # ORBIT2_MASKED_PER_IMAGE, ORBIT2_MASKED_LOWER: flags or-ed into the kind
MASKED_MAX_LEVELS = 8                           # ORBIT2_MASKED_MAX_LEVELS: levels / thresholds per call (bits 8-15 of the kind)


def quantile_ws_words(G: int, Q: int) -> int:
    """ORBIT2_QUANTILE_WS_WORDS(G, Q)"""
    return 2 * G * (64 + 256 + 3 * 2 * Q * 256)


def tail_ws_words(B: int, Cc: int, T: int) -> int:
    """ORBIT2_TAIL_WS_WORDS(B, C, T)"""
    return B * Cc * LOSS_BLOCKS * 8 * T


def _levels(name, t, what, rows=None):
    """the fp32 device vector (rows=None) or [rows, n] matrix a call of the extreme-value kinds reads as chan_w; returns n"""
    _dev(t, F32, what)
    n = t.shape[-1] if t.dim() else 0
    if t.dim() != (1 if rows is None else 2) or not 1 <= n <= MASKED_MAX_LEVELS or (rows is not None and t.shape[0] != rows):
        raise HipBackendError("%s: %s must be fp32 %s with 1..%d entries per row, got %s"
                              % (name, what, "[n]" if rows is None else "[%d, n]" % rows, MASKED_MAX_LEVELS, tuple(t.shape)))
    return n


def _groups(name, B, Cc, H, W, per_image):
    G, pixels = (B * Cc, H * W) if per_image else (Cc, B * H * W)
    if pixels >= 1 << 31:
        raise HipBackendError("%s: a group of %d pixels; the entry takes fewer than 2^31 per group" % (name, pixels))
    return G


def masked_quantiles(pred, target, levels, mask=None, mask_strides=(0, 0, 0), per_image=False):
    """(out fp32 [2, G, Q, 3], cnt int64 [G]): for field 0 = target and 1 = pred and every group (G = C: a channel pooled over the
    batch; per_image: G = B * C) the linear quantile at every level of `levels` (fp32 [Q], Q <= 8, on the device) over the valid
    pixels, then its two bracketing order statistics, exact; cnt the valid pixels (include/orbit2_hip.h: ORBIT2_MASKED_QUANTILES).
    pred may be target itself."""
    B, Cc, H, W = _scored_pair("masked_quantiles", pred, target)
    Q = _levels("masked_quantiles", levels, "levels")
    mp = _mask_args(mask, mask_strides, pred, target)
    G = _groups("masked_quantiles", B, Cc, H, W, per_image)
    out = torch.empty(2, G, Q, 3, dtype=F32, device=pred.device)
    cnt = torch.empty(G, dtype=torch.int64, device=pred.device)
    ws = torch.empty(quantile_ws_words(G, Q), dtype=F32, device=pred.device)
    kind = MASKED_QUANTILES | (MASKED_PER_IMAGE if per_image else 0) | (Q << 8)
    _call("orbit2_masked_loss_fwd", pred, target, target.shape[2], target.shape[3], *mp, None, levels, out, cnt, ws, B, Cc, H, W,
          kind)
    return out, cnt


def masked_tail(pred, target, thresholds, lat_w=None, mask=None, mask_strides=(0, 0, 0), lower=False, per_image=False):
    """(sums fp32 [B, C, T, 4], cnt int64 [B, C, T, 4]) per image and threshold over the valid pixels whose target is at or beyond
    the threshold (lower: at or below): {sum w, sum w d^2, sum w |d|, sum d} and {tail pixels, hits, false alarms, valid pixels}
    (include/orbit2_hip.h: ORBIT2_MASKED_TAIL).  thresholds: fp32 [G, T] on the device, G = C or, per_image, B * C; T <= 8."""
    B, Cc, H, W = _scored_pair("masked_tail", pred, target, lat_w)
    G = _groups("masked_tail", B, Cc, H, W, per_image)
    T = _levels("masked_tail", thresholds, "thresholds", G)
    mp = _mask_args(mask, mask_strides, pred, target)
    out = torch.empty(B, Cc, T, 4, dtype=F32, device=pred.device)
    cnt = torch.empty(B, Cc, T, 4, dtype=torch.int64, device=pred.device)
    ws = torch.empty(tail_ws_words(B, Cc, T), dtype=F32, device=pred.device)
    kind = MASKED_TAIL | (MASKED_PER_IMAGE if per_image else 0) | (MASKED_LOWER if lower else 0) | (T << 8)
    _call("orbit2_masked_loss_fwd", pred, target, target.shape[2], target.shape[3], *mp, lat_w, thresholds, out, cnt, ws, B, Cc,
          H, W, kind)
    return out, cnt


# ---- the fractions skill score (csrc/fss.hip): one more kind of orbit2_masked_loss_fwd, its window in bits 16-23 ----------------
FSS_KIND = 5                    # ORBIT2_FSS_KIND
FSS_MAX_WINDOW = 255            # ORBIT2_FSS_MAX_WINDOW: odd windows 1 .. 255
FSS_STRIP = 256                 # csrc/fss_window.h FSS_STRIP: columns of a workgroup of the window pass
FSS_BANDS = (128, 32, 1024)     # FSS_MAX_BAND, FSS_MIN_BAND, FSS_FILL: centre rows of a workgroup, halved while the launch is small


def fss_ws_words(B: int, Cc: int, H: int, W: int, T: int) -> int:
    """ORBIT2_FSS_WS_WORDS(B, C, H, W, T)"""
    return 2 * B * Cc * (2 * T + 1) * H * ((W + 63) // 64)


def fss_partition(B: int, Cc: int, H: int, W: int, T: int):
    """(columns of a strip, centre rows of a band) of the window pass at these sizes (csrc/fss_window.h: fss_strips,
    fss_band_rows)"""
    band, low, fill = FSS_BANDS
    groups = B * Cc * T * ((W + FSS_STRIP - 1) // FSS_STRIP)
    while band > low and groups * ((H + band - 1) // band) < fill:
        band >>= 1
    return FSS_STRIP, band


def masked_fss(pred, target, thresholds, window, mask=None, mask_strides=(0, 0, 0), lower=False, per_image=False):
    """(fss fp32 [B, C, T], cnt int64 [B, C, T, 4]) per image and threshold: with cO / cM the numbers of target / prediction
    pixels at or beyond the threshold (lower: at or below) in the `window` x `window` neighbourhood of a pixel, zero beyond the
    plane and at invalid pixels, cnt = {valid centres, sum cO^2, sum cM^2, sum (cO - cM)^2} over the valid centres and
    fss = 1 - cnt[3] / (cnt[1] + cnt[2]), NaN at 0 / 0 (include/orbit2_hip.h: ORBIT2_FSS_KIND).  thresholds: fp32 [G, T] on the
    device, G = C or, per_image, B * C; T <= 8; window odd, 1 .. 255."""
    B, Cc, H, W = _scored_pair("masked_fss", pred, target)
    G = _groups("masked_fss", B, Cc, H, W, per_image)
    T = _levels("masked_fss", thresholds, "thresholds", G)
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= FSS_MAX_WINDOW or window % 2 == 0:
        raise HipBackendError("masked_fss: the window must be an odd int in 1..%d, got %r" % (FSS_MAX_WINDOW, window))
    mp = _mask_args(mask, mask_strides, pred, target)
    out = torch.empty(B, Cc, T, dtype=F32, device=pred.device)
    cnt = torch.empty(B, Cc, T, 4, dtype=torch.int64, device=pred.device)
    ws = torch.empty(fss_ws_words(B, Cc, H, W, T) // 2, dtype=torch.int64, device=pred.device)       # 8-byte aligned words
    kind = FSS_KIND | (MASKED_PER_IMAGE if per_image else 0) | (MASKED_LOWER if lower else 0) | (T << 8) | (window << 16)
    _call("orbit2_masked_loss_fwd", pred, target, target.shape[2], target.shape[3], *mp, None, thresholds, out, cnt, ws, B, Cc,
          H, W, kind)
    return out, cnt


def ensemble_update(member, mean, m2, k: int):
    """the k-th (1-based) Welford step of the running ensemble moments, in place on `mean` and `m2`
    (include/orbit2_hip.h:orbit2_ensemble_update); k = 1 initialises them, so they may be torch.empty"""
    _dev(member, F32, "member"); _dev(mean, F32, "mean"); _dev(m2, F32, "m2")
    if mean.shape != member.shape or m2.shape != member.shape:
        raise HipBackendError("ensemble_update: member %s, mean %s and m2 %s must have one shape"
                              % (tuple(member.shape), tuple(mean.shape), tuple(m2.shape)))
    _call("orbit2_ensemble_update", member, mean, m2, member.numel(), int(k))


def gaussian_scores(mean, std, target, lat_w=None):
    """[B,C,4] float64 sums {w crps, w std^2, w (mean - target)^2, 1{|target - mean| <= std}} of a Gaussian prediction
    (include/orbit2_hip.h:orbit2_gaussian_scores); the target may be larger than the prediction (top-left crop)"""
    if _dev(std, F32, "std").shape != mean.shape:
        raise HipBackendError("gaussian_scores: mean %s and std %s differ in shape" % (tuple(mean.shape), tuple(std.shape)))
    B, Cc, H, W = _scored_pair("gaussian_scores", mean, target, lat_w)
    out = torch.empty(B, Cc, 4, dtype=torch.float64, device=mean.device)
    _call("orbit2_gaussian_scores", mean, std, target, target.shape[2], target.shape[3], lat_w, out, B, Cc, H, W)
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
    if not _on_device(members):
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
    _call("orbit2_ensemble_scores", members, members.stride(0), N, target, target.shape[2], target.shape[3], lat_w,
          out.get("sums"), out.get("crps_field"), int(crps_field == "fair"), out.get("hist"), int(seed) & 0xFFFFFFFFFFFFFFFF,
          out.get("quantiles"), levels, 0 if levels is None else levels.numel(), B, Cc, H, W)
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
    _call("orbit2_ssim", pred, target, target.shape[2], target.shape[3], lat_w, rng, sums, smap, B, Cc, H, W)
    return (sums, smap) if ssim_map else sums


LOSS_SSIM_VJP = 3               # ORBIT2_LOSS_SSIM_VJP: the kind of orbit2_loss_bwd that is the backward of orbit2_ssim's sums
SSIM_VJP_TILE = (16, 64)        # (ORBIT2_SSIM_VJP_TILE_H, ORBIT2_SSIM_VJP_TILE_W): pixels of dpred per workgroup


def ssim_vjp(pred, target, lat_w, coef, data_range):
    """dpred fp32 [B,C,H,W] = the gradient with respect to pred of sum_bc coef[bc] * ssim_sums(...)[bc][1] (of [bc][0] with lat_w
    None), every image at its data range data_range[bc]: orbit2_loss_bwd at kind 3 (include/orbit2_hip.h).  coef and data_range
    are fp32 [B,C] device tensors; they are packed into the entry's gscale [2][B*C] on the device.  An image whose coef is 0.0 is
    zero-filled without being read."""
    if torch.is_tensor(pred) and pred.dim() == 4 and min(pred.shape[2:]) < SSIM_WIN:
        raise HipBackendError("ssim_vjp: the prediction is %d x %d, the window needs at least %d x %d"
                              % (pred.shape[2], pred.shape[3], SSIM_WIN, SSIM_WIN))
    B, Cc, H, W = _scored_pair("ssim_vjp", pred, target, lat_w)
    for name, t in (("coef", coef), ("data_range", data_range)):
        if not torch.is_tensor(t) or tuple(_dev(t, F32, name).shape) != (B, Cc):
            raise HipBackendError("ssim_vjp: %s must be an fp32 [B,C] = [%d,%d] device tensor" % (name, B, Cc))
    gscale = torch.stack((coef.detach(), data_range.detach())).contiguous()
    dpred = torch.empty_like(pred)
    _call("orbit2_loss_bwd", pred, target, target.shape[2], target.shape[3], lat_w, None, gscale, dpred, B, Cc, H, W,
          LOSS_SSIM_VJP)
    return dpred


RESAMPLE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}
RESAMPLE_TILE = (32, 256)       # (ORBIT2_RESAMPLE_TILE_H, ORBIT2_RESAMPLE_TILE_W): output pixels per workgroup
RESAMPLE_LDS_FLOATS = 10240     # ORBIT2_RESAMPLE_LDS_FLOATS: the staged source window of a tile
ANTIALIAS = 4                   # ORBIT2_ANTIALIAS: or-ed into the mode code of bilinear and bicubic
TRANSPOSE = 16                  # ORBIT2_TRANSPOSE: or-ed into 5 and 6 of orbit2_resample_fwd, the adjoint of the coarsening
RESAMPLE_ADJOINT_TILE = (32, 64)        # (ORBIT2_AT_TILE_H, ORBIT2_AT_TILE_W): fine pixels per workgroup of the adjoint


_RESAMPLE_IDX = {}              # (channels, device) -> the validated device int32 copy


def resample_staged(h: int, w: int, H: int, W: int) -> bool:
    """whether orbit2_resample_* stages a tile's source window in LDS at this pair of sizes (the header's rule: the full-tile
    footprint of the ratio fits the budget) or reads the taps from global memory"""
    th, tw = RESAMPLE_TILE
    return (-(-th * h // H) + 4) * (-(-tw * w // W) + 4) <= RESAMPLE_LDS_FLOATS


def _resample_args(x, size, mode, channels, scale, shift, what, antialias=False):
    """the checked operands both resample entries share: (B, Cin, h, w, C, H, W, mode code, chan_idx, scale, shift)"""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise HipBackendError("%s takes an [B,C,h,w] field" % what)
    if mode not in RESAMPLE_MODES:
        raise HipBackendError("%s: mode is one of %s, got %r" % (what, ", ".join(RESAMPLE_MODES), mode))
    if antialias and mode == "nearest":
        raise HipBackendError("%s: antialias goes with bilinear or bicubic, nearest has no antialiased form" % what)
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
    return B, Cin, h, w, Cc, H, W, RESAMPLE_MODES[mode] | (ANTIALIAS if antialias else 0), idx, scale, shift


def resample(x, size, mode="bilinear", channels=None, scale=None, shift=None, out=None, antialias=False):
    """fp32 [B,C,H,W]: F.interpolate(x[:, channels], size, mode, align_corners=False) * scale[c] + shift[c] in one kernel
    (include/orbit2_hip.h:orbit2_resample_fwd).  mode: nearest, bilinear or bicubic; channels: input channel of every output
    channel (None = all, in order); scale / shift: [C], both or neither; out: a contiguous fp32 [B,C,H,W] to write into;
    antialias: F.interpolate's antialias=True (bilinear and bicubic only), the mode code with ORBIT2_ANTIALIAS."""
    B, Cin, h, w, Cc, H, W, m, idx, scale, shift = _resample_args(x, size, mode, channels, scale, shift, "resample", antialias)
    if out is None:
        out = torch.empty(B, Cc, H, W, dtype=F32, device=x.device)
    else:
        _dev(out, F32, "out")
        if tuple(out.shape) != (B, Cc, H, W):
            raise HipBackendError("resample: out is %s, the result %s" % (tuple(out.shape), (B, Cc, H, W)))
    _call("orbit2_resample_fwd", x, idx, Cin, scale, shift, out, B, Cc, h, w, H, W, m)
    return out


def resample_moments(x, size, mode, target, channels=None, scale=None, shift=None, lat_w=None, clim=None, antialias=False):
    """[B,C,12] float64: eval_moments(resample(x, ...), target, lat_w, clim) without the resampled field ever being stored
    (include/orbit2_hip.h:orbit2_resample_moments); the target may be larger than (H, W) (top-left crop)"""
    B, Cin, h, w, Cc, H, W, m, idx, scale, shift = _resample_args(x, size, mode, channels, scale, shift, "resample_moments",
                                                                  antialias)
    _scored_pair("resample_moments", (B, Cc, H, W), target, lat_w, clim)
    out = torch.empty(B, Cc, 12, dtype=torch.float64, device=x.device)
    _call("orbit2_resample_moments", x, idx, Cin, scale, shift, target, target.shape[2], target.shape[3], lat_w, clim, out,
          B, Cc, h, w, H, W, m)
    return out


def resample_adjoint(g, size, mode="bilinear"):
    """fp32 [B,C,H,W]: the adjoint of resample(., (h, w), mode, antialias=True) on a field of `size` = (H, W), applied to the
    gradient g [B,C,h,w] of the coarsened field (include/orbit2_hip.h: orbit2_resample_fwd with ORBIT2_TRANSPOSE, mode codes 21
    and 22).  Coarsening only: H >= h and W >= w.  The weights are the forward kernel's bit for bit."""
    if not torch.is_tensor(g) or g.dim() != 4:
        raise HipBackendError("resample_adjoint takes an [B,C,h,w] gradient")
    if mode not in ("bilinear", "bicubic"):
        raise HipBackendError("resample_adjoint: mode is bilinear or bicubic (the antialiased modes), got %r" % (mode,))
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise HipBackendError("resample_adjoint: size is (H, W), got %r" % (size,)) from None
    B, C, h, w = g.shape
    if min(B, C, h, w) < 1:
        raise HipBackendError("resample_adjoint: every size must be positive (g %s)" % (tuple(g.shape),))
    if H < h or W < w:
        raise HipBackendError("resample_adjoint: only the adjoint of a coarsening is built: size %s is smaller than g's %s"
                              % ((H, W), (h, w)))
    _dev(g, F32, "g")
    if B * C > 65535:
        raise HipBackendError("resample_adjoint: B * C = %d images, at most 65535 are served in one call" % (B * C))
    out = torch.empty(B, C, H, W, dtype=F32, device=g.device)
    _call("orbit2_resample_fwd", g, None, C, None, None, out, B, C, h, w, H, W, RESAMPLE_MODES[mode] | ANTIALIAS | TRANSPOSE)
    return out


def seed_salt(value: int, add: bool = False):
    """device-side salt xored into every kernel seed (see include/orbit2_hip.h:orbit2_seed_salt); stream-ordered"""
    _call("orbit2_seed_salt", value, int(add))