"""CPU checks of the C-ABI library: it builds, loads, exports exactly what include/orbit2_hip.h declares, and climate_learn._hip
declares every prototype the way the header does."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "orbit2_hip.h")
# the forwarding entries ABI 7 and ABI 8 removed: each was a one-line call of the entry that replaced it
REMOVED = ("orbit2_attn_fwd", "orbit2_attn_fwd_ex", "orbit2_attn_bwd", "orbit2_attn_bwd_ex", "orbit2_layernorm_fwd",
           "orbit2_sgemm_f32",
           "orbit2_gemm_bf16_gated", "orbit2_gemm_bf16_tq", "orbit2_gemm_bf16_grouped_gated", "orbit2_gemm_bf16_grouped_tq",
           "orbit2_attn_fwd_gated", "orbit2_attn_fwd_tq", "orbit2_attn_bwd_gated", "orbit2_attn_bwd_tq")


def _header():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)


def _kind(param):
    """the parameter kind of one C parameter declaration: int, int64_t, uint64_t, float, void* or orbit2_gemm_args*"""
    decl = " ".join(param.split())
    if "*" in decl:
        return "orbit2_gemm_args*" if "orbit2_gemm_args" in decl else "void*"
    kind = decl.rsplit(" ", 1)[0]
    assert kind in ("int", "int64_t", "uint64_t", "float"), "unexpected parameter kind: " + param
    return kind


def _prototypes():
    """name -> (return kind, argument kinds) of every orbit2_* prototype of the header"""
    protos = {}
    for ret, name, params in re.findall(r"\b(int|int64_t)\s+(orbit2_\w+)\s*\(([^)]*)\)\s*;", _header()):
        assert name not in protos, "declared twice: " + name
        params = params.strip()
        protos[name] = (ret, tuple(_kind(p) for p in params.split(",")) if params not in ("", "void") else ())
    return protos


def _exports(path):
    """the orbit2_* functions the library defines in its dynamic symbol table"""
    readelf = shutil.which("llvm-readelf") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    out = subprocess.run([readelf, "--dyn-syms", "-W", path], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]        # Num: Value Size Type Bind Vis Ndx Name
    return {r[7] for r in rows if len(r) >= 8 and r[3] == "FUNC" and r[6] != "UND" and r[7].startswith("orbit2_")}


def test_library_exports_exactly_the_declared_symbols():
    import __graft_entry__ as ge
    ge.build()
    from climate_learn import _hip
    assert os.path.exists(_hip.LIB_PATH)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    hdr = open(HEADER).read()
    names = sorted(set(re.findall(r"\b(?:int|int64_t)\s+(orbit2_\w+)\s*\(", hdr)))
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "missing export " + n
    assert lib.orbit2_abi_version() == 8
    # ... and the other way: the library exports nothing the header does not declare, none of the removed entries among it
    exported = _exports(_hip.LIB_PATH)
    assert exported == set(_prototypes()), "exported, not declared: %s; declared, not exported: %s" % (
        sorted(exported - set(_prototypes())), sorted(set(_prototypes()) - exported))
    for n in REMOVED:
        assert n not in exported and n not in names and not hasattr(lib, n)


def test_binding_declares_every_prototype_as_the_header_does():
    from climate_learn import _hip
    kinds = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t", ctypes.c_float: "float",
             ctypes.c_void_p: "void*", ctypes.POINTER(_hip.GemmArgs): "orbit2_gemm_args*"}
    header = _prototypes()
    assert len(header) >= 50
    assert set(_hip.PROTOTYPES) == set(header)
    for name, (restype, argtypes) in _hip.PROTOTYPES.items():
        assert (kinds[restype], tuple(kinds[a] for a in argtypes)) == header[name], name
    # and load() applied exactly that table to the library the package uses
    lib = _hip.lib()
    for name, (restype, argtypes) in _hip.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


def test_binding_constants_match_the_header():
    from climate_learn import _hip
    defines = dict(re.findall(r"^#define\s+ORBIT2_(\w+)\s+(\d+)", _header(), flags=re.M))
    assert int(defines["ABI_VERSION"]) == _hip.ABI_VERSION == 8
    assert int(defines["GEMM_MAX_GROUP"]) == _hip.GEMM_MAX_GROUP
    assert int(defines["LOSS_BLOCKS"]) == _hip.LOSS_BLOCKS
    flags = {k: int(v) for k, v in defines.items() if k.startswith("ATTN_")}
    assert flags and flags == {k: getattr(_hip, k) for k in dir(_hip) if k.startswith("ATTN_")}
    assert _hip.lib().orbit2_abi_version() == 8


def test_load_refuses_another_abi_version(tmp_path):
    from climate_learn import _hip
    with pytest.raises(_hip.HipBackendError, match="not found"):
        _hip.load(str(tmp_path / "liborbit2_hip.so"))
    # a shared object of no version at all (ctypes' own extension module has no orbit2_abi_version) is refused before use
    import _ctypes
    with pytest.raises(_hip.HipBackendError, match="ABI version None"):
        _hip.load(_ctypes.__file__)


def test_mistyped_calls_never_reach_the_library():
    """host-only entries that launch nothing: a call with too few arguments or an argument of the wrong kind is refused by
    ctypes; the int64_t queries return int64_t whatever ran before them"""
    import torch
    from climate_learn import _hip
    lib = _hip.lib()
    assert lib.orbit2_colsum_ws_floats(1024, 64) > 0
    assert lib.orbit2_attn_bwd_ws_floats(64, 1 << 20, 64) == 2 * 64 * 64 * ((1 << 20) + 64)      # > 2^31: needs the int64_t
    with pytest.raises(TypeError):
        lib.orbit2_colsum_ws_floats(1024)
    with pytest.raises(TypeError):
        lib.orbit2_attn_bwd_ws_floats(2, 1024)
    with pytest.raises(TypeError):
        lib.orbit2_gemm_bf16_colsum_rows()
    with pytest.raises(ctypes.ArgumentError):
        lib.orbit2_colsum_ws_floats(1024.0, 64)                      # a float for an int
    with pytest.raises(ctypes.ArgumentError):
        lib.orbit2_attn_bwd_ws_floats(2, 1024, 16.5)
    with pytest.raises(ctypes.ArgumentError):
        lib.orbit2_gemm_bf16_colsum_rows(torch.zeros(46))             # a tensor for a pointer
    with pytest.raises(ctypes.ArgumentError):
        lib.orbit2_gemm_bf16_colsum_rows(0x10000)                     # an address for the argument block


def test_gemm_args_struct_matches_header():
    from climate_learn import _hip
    # field order/size contract with the C struct (8-byte pointers, 4-byte ints/floats, 8-byte seed)
    assert ctypes.sizeof(_hip.GemmArgs) == 184
    assert _hip.GemmArgs.colsum_ws.offset == 176          # ABI 5: the last field
    assert _hip.GemmArgs.seed.offset % 8 == 0


def test_no_cpu_fallback():
    import pytest
    import torch
    from climate_learn import _hip
    with pytest.raises(_hip.HipBackendError):
        _hip.layernorm_fwd(torch.zeros(4, 64, dtype=torch.bfloat16), torch.ones(64, dtype=torch.bfloat16),
                           torch.zeros(64, dtype=torch.bfloat16))


def test_gemm_colsum_dispatch_is_host_logic():
    """orbit2_gemm_bf16_colsum_rows mirrors the dispatch without touching the GPU: M / 256 rows for the factor-multiply input gradient
    on whole tiles that fill the chip (the only call that fills colsum_ws), 0 otherwise -- and a call with colsum_ws set that cannot
    fuse is refused (-3) before anything is launched"""
    from climate_learn import _hip
    lib = _hip.lib()

    def args(M, N, K, b_kc=False, mul=True, bias=False, tile=0):
        a = _hip.GemmArgs()
        a.A, a.B, a.C = 0x10000, 0x20000, 0x30000            # never dereferenced on the host
        a.M, a.N, a.K, a.lda, a.ldb, a.ldc = M, N, K, K, (K if b_kc else N), N
        a.a_kc, a.b_kc = 1, int(b_kc)
        a.mul = 0x40000 if mul else None
        a.bias = 0x50000 if bias else None
        a.tile_hint = tile
        return a

    assert lib.orbit2_gemm_bf16_colsum_rows(ctypes.byref(args(131072, 12288, 3072))) == 512      # fc2's input gradient, batch 16
    assert lib.orbit2_gemm_bf16_colsum_rows(ctypes.byref(args(768, 512, 192, tile=260))) == 3
    for bad in (args(768, 512, 192), args(131072, 12288, 3072, b_kc=True), args(131072, 12288, 3072, mul=False),
                args(131072, 12288, 3072, bias=True), args(131072, 12288, 3072, tile=256), args(131000, 12288, 3072)):
        assert lib.orbit2_gemm_bf16_colsum_rows(ctypes.byref(bad)) == 0
        bad.colsum_ws = 0x60000
        assert lib.orbit2_gemm_bf16(ctypes.byref(bad), None, 0, None, -1, None) == -3


def test_row_kernel_workspace_queries():
    """orbit2_layernorm_bwd_ws_floats and orbit2_colsum_ws_floats are host arithmetic over the kernels' partitions: the values of
    max(4 ceil(rows / 64), rows < 32768 ? ceil(rows / 4) : 0) * 2 D   and   ceil(M / (M >= 32768 ? 128 : 32)) * N"""
    from climate_learn import _hip
    lib = _hip.lib()
    for (rows, D), want in (((200, 64), 6400), ((4096, 1024), 2097152), ((33000, 3072), 12681216), ((131072, 3072), 50331648),
                            ((16384, 8192), 67108864)):
        assert lib.orbit2_layernorm_bwd_ws_floats(rows, D) == want, (rows, D)
    for (M, N), want in (((4096, 1024), 131072), ((131072, 12288), 12582912)):
        assert lib.orbit2_colsum_ws_floats(M, N) == want, (M, N)
