"""The call path of climate_learn._hip without a device: every wrapper runs on small host tensors against a stub library that
validates each call against _hip.PROTOTYPES and records it.  What it pins: one valid call per wrapper reaches the entry it names
with the stream last; every entry of PROTOTYPES is reached; a tensor operand that is not on the device, or of a dtype the entry
does not read, is refused in Python before ANY entry is called (these cases are not for a GPU test: there the failure mode of a
missing check would be a kernel reading a bad address); a non-zero code raises naming the entry and the code.

CASES is also the table tools and reviews can replay against another revision of the binding: every case takes the module."""
import ctypes

import pytest
import torch

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
STREAM, SCHED_WORD, ANSWER = 0x5EED, 0x7000, 8          # the stub's stream and counter word; what every query answers

# entries no wrapper call of CASES reaches, each with its reason; nothing else may be missing from the stub's record
NOT_REACHED = {
    "orbit2_abi_version": "asked by load() when it opens a library, never by a wrapper",
    "orbit2_selftest": "selftest() synchronises the device and reads the result back",
    "orbit2_varagg_fwd": "reached through orbit2_varagg_fwd_p with patch = 2 (the plain entry stays for C callers and raw tests)",
    "orbit2_varagg_fwd_f32": "reached through orbit2_varagg_fwd_f32_p with patch = 2",
    "orbit2_varagg_bwd": "reached through orbit2_varagg_bwd_p with patch = 2",
    "orbit2_varagg_bwd_ws_floats": "reached through orbit2_varagg_bwd_p_ws_floats with patch = 2",
    "orbit2_varagg_bwd_is_fixed_order": "reached through orbit2_varagg_bwd_p_is_fixed_order with patch = 2",
}


def is_query(name):
    """the entries that launch nothing and take no stream"""
    return name.endswith(("_ws_floats", "_is_fixed_order", "_colsum_rows")) or name == "orbit2_abi_version"


class StubLib:
    """stands in for the loaded library: an entry checks its arguments against PROTOTYPES, records (name, args) and answers
    `rc` (launches) or ANSWER (queries)"""

    def __init__(self, hip, rc=0):
        self.hip, self.rc, self.calls = hip, rc, []

    def __getattr__(self, name):
        restype, argtypes = self.hip.PROTOTYPES[name]           # KeyError: an entry the header does not declare

        def entry(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, got %d" % (name, len(argtypes), len(args))
            for i, (a, kind) in enumerate(zip(args, argtypes)):
                assert self.fits(a, kind), "%s argument %d: %r is no %s" % (name, i, a, kind.__name__)
            self.calls.append((name, args))
            return ANSWER if is_query(name) else self.rc

        return entry

    def fits(self, a, kind):
        if kind in (ctypes.c_int, ctypes.c_int64, ctypes.c_uint64):
            return isinstance(a, int)
        if kind is ctypes.c_float:
            return isinstance(a, (int, float))
        if kind is ctypes.c_void_p:                             # an address, NULL, or a ctypes array of them (the K gates)
            return a is None or isinstance(a, (int, ctypes.Array))
        block = a._obj if type(a).__name__ == "CArgObject" else a           # byref(GemmArgs) or an array of them
        return isinstance(block, self.hip.GemmArgs) or (isinstance(block, ctypes.Array) and block._type_ is self.hip.GemmArgs)


def on_device(t):
    """the replaced device predicate: every host tensor counts as a device tensor unless a test flagged it"""
    return not getattr(t, "flagged_host", False)


@pytest.fixture
def hip(monkeypatch):
    from climate_learn import _hip
    monkeypatch.setattr(_hip, "_on_device", on_device)
    monkeypatch.setattr(_hip, "_stream", lambda: STREAM)
    monkeypatch.setattr(_hip, "_sched_word", lambda device: SCHED_WORD)
    monkeypatch.setattr(_hip, "timer", None)
    stub = StubLib(_hip)
    monkeypatch.setattr(_hip, "lib", lambda: stub)
    _hip.stub = stub
    yield _hip
    del _hip.stub


def t(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


def rows(dtype, m, n, pad=8):
    """[m, n] with a row pitch of n + pad: what _dev_rows takes and _dev does not"""
    return torch.zeros(m, n + pad, dtype=dtype)[:, :n]


def _cases():
    """(wrapper, tensor operands by name, call(H, operands)): one valid call per launching wrapper, a second where a wrapper has
    a second path.  Only the operands that cross the ABI as they are handed over are named; what a wrapper converts first (a
    data range, a scale, a channel list) is written into the call."""
    B, C, Hh, W = 2, 3, 8, 12
    pair = dict(pred=t(F32, B, C, Hh, W), target=t(F32, B, C, Hh + 1, W + 4), lat_w=t(F32, Hh))
    loss = dict(pair, chan_w=t(F32, C))
    mask = dict(loss, mask=t(torch.uint8, B * C * Hh * W))
    ms = (W, C * Hh * W, Hh * W)
    M, N, K = 16, 24, 32
    gk = lambda o, *names: {k: o[k] for k in names}
    return [
        ("gemm", dict(A=rows(BF, M, K), B=t(BF, N, K), out=rows(BF, M, N), bias=t(BF, N), save_dact=rows(torch.int16, M, N),
                      rowscale=t(F32, 2), residual=t(BF, M, N), gate=t(F32, 2)),
         lambda H, o: H.gemm(o["A"], o["B"], o["out"], M, N, K, K + 8, K, N + 8, want_colsum=True, gate=o["gate"], rows_per_gate=8,
                             tail_queue=True, act=1, drop_p=0.1, seed=(1 << 63) + 5, rows_per_scale=8, ldr=N, colscale=(8, 0.5),
                             **gk(o, "bias", "save_dact", "rowscale", "residual"))),
        ("gemm", dict(A=t(BF, M, N), B=t(BF, N, K), out=t(F32, M, K), save_pre=t(BF, M, K), dgelu_pre=t(BF, M, K), mul=t(torch.int16, M, K)),
         lambda H, o: H.gemm(o["A"], o["B"], o["out"], M, K, N, N, K, K, b_kc=False, **gk(o, "save_pre", "dgelu_pre", "mul"))),
        ("gemm_f32", dict(A=rows(F32, M, K), B=t(F32, N, K), out=t(F32, M, N), bias=t(F32, N), residual=rows(F32, M, N)),
         lambda H, o: H.gemm_f32(o["A"], o["B"], o["out"], M, N, K, K + 8, K, N, bias=o["bias"], act=1, residual=o["residual"],
                                 ldr=N + 8)),
        ("gemm_grouped", dict(A0=t(BF, M, N), B0=t(BF, M, K), out0=t(BF, N, K), A1=t(BF, M, N), B1=t(BF, M, K), out1=t(F32, N, K),
                              kgate=t(F32, 2)),
         lambda H, o: H.gemm_grouped([(o["A0"], o["B0"], o["out0"], N, K, M, N, K, K, dict(a_kc=False, b_kc=False, beta=1.0)),
                                      (o["A1"], o["B1"], o["out1"], N, K, M, N, K, K,
                                       dict(a_kc=False, b_kc=False, kgate=(o["kgate"], 8)))], tail_queue=4)),
        ("sgemm", dict(A=t(F32, M, K), B=t(F32, K, N), out=t(F32, M, N)),
         lambda H, o: H.sgemm(o["A"], o["B"], o["out"], M, N, K, K, N, N, tb=True, alpha=2.0)),
        ("layernorm_fwd", dict(x=t(BF, M, N), gamma=t(BF, N), beta=t(BF, N), out=rows(BF, M, N)),
         lambda H, o: H.layernorm_fwd(o["x"], o["gamma"], o["beta"], out=o["out"])),
        ("layernorm_fwd_f32", dict(x=t(F32, M, N), gamma=t(F32, N), beta=t(F32, N)),
         lambda H, o: H.layernorm_fwd_f32(o["x"], o["gamma"], o["beta"], stats=True)),
        ("layernorm_fwd_f32", dict(x=t(F32, M, N), gamma=t(F32, N), beta=t(F32, N), out=rows(F32, M, N)),
         lambda H, o: H.layernorm_fwd_f32(o["x"], o["gamma"], o["beta"], eps=1e-6, out=o["out"])),
        ("layernorm_bwd", dict(dy=t(BF, M, N), x=t(BF, M, N), gamma=t(BF, N), mean=t(F32, M), rstd=t(F32, M), dres=t(BF, M, N),
                               dgamma=t(F32, N), dbeta=t(F32, N)),
         lambda H, o: H.layernorm_bwd(o["dy"], o["x"], o["gamma"], o["mean"], o["rstd"], o["dres"], o["dgamma"], o["dbeta"], 1.0)),
        ("layernorm_bwd", dict(dy=t(BF, M, N), x=t(BF, M, N), gamma=t(BF, N), mean=t(F32, M), rstd=t(F32, M), dgamma=t(BF, N),
                               dbeta=t(BF, N)),
         lambda H, o: H.layernorm_bwd(o["dy"], o["x"], o["gamma"], o["mean"], o["rstd"], None, o["dgamma"], o["dbeta"])),
        ("probe_read", dict(buf=t(F32, 64), sink=t(F32, 1)), lambda H, o: H.probe_read(o["buf"], 4, 2, o["sink"])),
        ("attn_fwd", dict(qkv=rows(BF, 2 * 16, 3 * 2 * 8), out=rows(BF, 2 * 16, 2 * 8), gate=t(F32, 2)),
         lambda H, o: H.attn_fwd(o["qkv"], 2, 16, 2, 8, 0.1, 77, flags=H.ATTN_Q_PRESCALED, out=o["out"], gate=o["gate"],
                                 tail_queue=True)),
        ("attn_fwd", dict(qkv=t(BF, 2, 16, 3 * 2 * 8)), lambda H, o: H.attn_fwd(o["qkv"], 2, 16, 2, 8)),
        ("attn_fwd_f32", dict(qkv=rows(F32, 2 * 16, 3 * 2 * 8), out=t(F32, 2 * 16, 2 * 8)),
         lambda H, o: H.attn_fwd_f32(o["qkv"], 2, 16, 2, 8, out=o["out"])),
        ("attn_bwd", dict(qkv=rows(BF, 2 * 16, 3 * 2 * 8), out=t(BF, 2, 16, 2 * 8), dout=t(BF, 2, 16, 2 * 8), lse=t(F32, 2, 2, 16),
                          gate=t(F32, 2)),
         lambda H, o: H.attn_bwd(o["qkv"], o["out"], o["dout"], o["lse"], 2, 16, 2, 8, 0.1, 77, gate=o["gate"])),
    ] + [
        (name, dict(x=t(F32, 2, 3, 8, 8), stab=t(F32, 2, 3, p * p + 1), gtab=t(F32, 3, p * p + 1, 16)), call)
        for p in (2, 4)
        for name, call in (("varagg_fwd", lambda H, o: H.varagg_fwd(o["x"], o["stab"], o["gtab"], 2, 16)),
                           ("varagg_fwd_f32", lambda H, o, p=p: H.varagg_fwd_f32(o["x"], o["stab"], o["gtab"], 2, 16, want_attw=p == 4)))
    ] + [
        ("varagg_bwd", dict(x=t(F32, 2, 3, 8, 8), gtab=t(F32, 3, p * p + 1, 16), attw=t(F32, 2 * 64 // (p * p), 2, 3),
                            dz=t(BF, 2 * 64 // (p * p), 16)),
         lambda H, o: H.varagg_bwd(o["x"], o["gtab"], o["attw"], o["dz"], 2, 16))
        for p in (2, 1)
    ] + [
        ("tables_gather", dict(w0=t(F32, 16, 4), b0=t(F32, 16), var_embed=t(F32, 3, 16), ids=t(I32, 3)),
         lambda H, o: H.tables_gather(o["w0"], 64, o["b0"], 16, o["var_embed"], o["ids"], 3, 16)),
        ("tables_scatter", dict(dcmat=t(F32, 15, 16), gw0=t(F32, 16, 4), gb0=t(F32, 16), gvar_embed=t(F32, 3, 16), ids=t(I32, 3)),
         lambda H, o: H.tables_scatter(o["dcmat"], o["gw0"], 64, o["gb0"], 16, o["gvar_embed"], o["ids"], 3, 16)),
        ("dropout_bwd", dict(dy=t(BF, M, N), rowscale=t(F32, 2), out=t(BF, M, N)),
         lambda H, o: H.dropout_bwd(o["dy"], M, N, 0.1, 5, o["rowscale"], 8, out=o["out"])),
        ("dropout_bwd", dict(dy=t(BF, M, N)), lambda H, o: H.dropout_bwd(o["dy"], M, N, 0.1, 5)),
        ("dropout_bwd_colsum", dict(dy=t(BF, M, N), rowscale=t(F32, 2), colsum_out=t(F32, N)),
         lambda H, o: H.dropout_bwd_colsum(o["dy"], M, N, 0.1, 5, o["rowscale"], 8, o["colsum_out"], beta=1.0)),
        ("post_reduce", dict(x=t(BF, M, N), addend=t(BF, 4, N), residual=t(BF, M, N), rowscale=t(F32, 2), out=t(BF, M, N)),
         lambda H, o: H.post_reduce(o["x"], M, N, addend=o["addend"], res_mod=4, residual=o["residual"], drop_p=0.1, seed=5,
                                    rowscale=o["rowscale"], rows_per_scale=8, out=o["out"])),
        ("post_reduce", dict(x=t(BF, M, N)), lambda H, o: H.post_reduce(o["x"], M, N)),
        ("colsum", dict(x=rows(BF, M, N), out=t(F32, N)), lambda H, o: H.colsum(o["x"], M, N, N + 8, o["out"], beta=0.5)),
        ("colsum", dict(x=t(F32, M, N), out=t(BF, N)), lambda H, o: H.colsum(o["x"], M, N, N, o["out"])),
        ("batch_sum", dict(x=t(BF, 2, M, N), out=t(F32, M, N)), lambda H, o: H.batch_sum(o["x"], 2, M, N, o["out"], beta=1.0)),
        ("cast_to_bf16", dict(src=t(F32, 40), dst=t(BF, 40)), lambda H, o: H.cast_to_bf16(o["src"], o["dst"])),
        ("cast_to_bf16", dict(src=t(F32, 5, 8)), lambda H, o: H.cast_to_bf16(o["src"])),
        ("cast_to_f32", dict(src=t(BF, 40), dst=t(F32, 40)), lambda H, o: H.cast_to_f32(o["src"], o["dst"])),
        ("add_rowvec", dict(a=t(BF, M, N), vec=t(BF, N)), lambda H, o: H.add_rowvec(o["a"], o["vec"], M, N)),
        ("posembed_fwd", dict(pe=t(F32, 8, 16), sw=t(F32, 16), sb=t(F32, 16)),
         lambda H, o: H.posembed_fwd(o["pe"], o["sw"], o["sb"], 0.5, 2, 4, 4, 8)),
        ("posembed_fwd", dict(pe=t(F32, 8, 16)), lambda H, o: H.posembed_fwd(o["pe"], None, None, 0.0, 2, 4, 2, 4)),
        ("posembed_bwd", dict(dout=t(F32, 32, 16)), lambda H, o: H.posembed_bwd(o["dout"], 2, 4, 4, 8)),
        ("unpatchify_fwd", dict(t=t(BF, 2, 8, 12)), lambda H, o: H.unpatchify_fwd(o["t"], 2, 3, 4, 8, 2, 1)),
        ("unpatchify_fwd_f32", dict(t=t(F32, 2, 8, 12)), lambda H, o: H.unpatchify_fwd_f32(o["t"], 2, 3, 4, 8, 2, 1)),
        ("unpatchify_bwd", dict(dimg=t(F32, 2, 3, 4, 8)), lambda H, o: H.unpatchify_bwd(o["dimg"], 2, 3, 4, 8, 2, 1)),
        ("conv3x3_fwd", dict(x=t(F32, 2, 5, 6, 8), chan_idx=t(I32, 3), weight=t(F32, 8, 3, 3, 3), bias=t(F32, 8),
                             addend=t(F32, 2, 2, 12, 16)),
         lambda H, o: H.conv3x3_fwd(o["x"], o["chan_idx"], o["weight"], o["bias"], 1, 2, o["addend"])),
        ("conv3x3_fwd", dict(x=t(F32, 2, 3, 6, 8), weight=t(F32, 8, 3, 3, 3), bias=t(F32, 8)),
         lambda H, o: H.conv3x3_fwd(o["x"], None, o["weight"], o["bias"])),
        ("conv3x3_bwd", dict(dout=t(F32, 2, 2, 12, 16), x=t(F32, 2, 5, 6, 8), chan_idx=t(I32, 3), weight=t(F32, 8, 3, 3, 3),
                             pre=t(F32, 2, 8, 6, 8)),
         lambda H, o: H.conv3x3_bwd(o["dout"], o["x"], o["chan_idx"], o["weight"], o["pre"], True, 1, 2)),
        ("conv3x3_bwd", dict(dout=t(F32, 2, 8, 6, 8), x=t(F32, 2, 3, 6, 8), weight=t(F32, 8, 3, 3, 3)),
         lambda H, o: H.conv3x3_bwd(o["dout"], o["x"], None, o["weight"], None, False)),
        ("clamp_channel_", dict(img=t(F32, B, C, Hh, W)), lambda H, o: H.clamp_channel_(o["img"], 1)),
        ("clamp_channel_bwd_", dict(img=t(F32, B, C, Hh, W), dimg=t(F32, B, C, Hh, W)),
         lambda H, o: H.clamp_channel_bwd_(o["img"], o["dimg"], 1)),
        ("loss_fwd", dict(loss), lambda H, o: H.loss_fwd(o["pred"], o["target"], o["lat_w"], o["chan_w"], 1)),
        ("loss_fwd", dict(gk(pair, "pred", "target")), lambda H, o: H.loss_fwd(o["pred"], o["target"], None, None, 2)),
        ("loss_bwd", dict(loss, gscale=t(F32, 1)),
         lambda H, o: H.loss_bwd(o["pred"], o["target"], o["lat_w"], o["chan_w"], o["gscale"], 1)),
        ("adamw", dict(p=t(F32, 40), m=t(F32, 40), v=t(F32, 40), g=t(BF, 40), p16=t(BF, 40), found_inf=t(F32, 1)),
         lambda H, o: H.adamw(o["p"], o["m"], o["v"], o["g"], o["p16"], 40, 1e-3, 0.9, 0.99, 1e-8, 1e-5, 3, 0.5, o["found_inf"])),
        ("adamw", dict(p=t(F32, 40), m=t(F32, 40), v=t(F32, 40), g=t(F32, 40)),
         lambda H, o: H.adamw(o["p"], o["m"], o["v"], o["g"], None, 40, 1e-3, 0.9, 0.99, 1e-8, 1e-5, 1)),
        ("check_finite", dict(g=t(BF, 40), found_inf=t(F32, 1)), lambda H, o: H.check_finite(o["g"], 40, o["found_inf"])),
        ("droppath_scales", {}, lambda H, o: H.droppath_scales(4, 0.1, 9, "cpu")),
        ("transpose_bf16", dict(src=t(BF, 8, 16), dst=t(BF, 16, 8)), lambda H, o: H.transpose_bf16(o["src"], o["dst"])),
        ("im2col3x3", dict(x=t(BF, 2 * 4 * 4, 8)), lambda H, o: H.im2col3x3(o["x"], 2, 4, 4, 8)),
        ("col2im3x3", dict(dcol=t(BF, 32, 72), act=t(BF, 32, 8), tapg=t(BF, 32, 8)),
         lambda H, o: H.col2im3x3(o["dcol"], 2, 4, 4, 8, act=o["act"], tapg=o["tapg"])),
        ("col2im3x3", dict(dcol=t(BF, 32, 72)), lambda H, o: H.col2im3x3(o["dcol"], 2, 4, 4, 8)),
        ("maxpool2_fwd", dict(x=t(BF, 32, 8)), lambda H, o: H.maxpool2_fwd(o["x"], 2, 4, 4, 8)),
        ("maxpool2_bwd", dict(g=t(BF, 8, 8), x=t(BF, 32, 8), tapg=t(BF, 32, 8)),
         lambda H, o: H.maxpool2_bwd(o["g"], o["x"], 2, 4, 4, 8, tapg=o["tapg"])),
        ("lpips_conv1_fwd", dict(img=t(F32, 2, 3, 4, 4), w1=t(F32, 27, 64), b1=t(F32, 64)),
         lambda H, o: H.lpips_conv1_fwd(o["img"], o["w1"], o["b1"])),
        ("lpips_conv1_bwd", dict(dz=t(BF, 32, 64), w1=t(F32, 27, 64), pred=t(F32, 2, 3, 4, 4), target=t(F32, 2, 3, 4, 4),
                                 gscale=t(F32, 1)),
         lambda H, o: H.lpips_conv1_bwd(o["dz"], o["w1"], o["pred"], o["target"], 0.01, gscale=o["gscale"])),
        ("lpips_tap_fwd", dict(feats=t(BF, 4, 16, 64), lin=t(F32, 64), val=t(F32, 2)),
         lambda H, o: H.lpips_tap_fwd(o["feats"], o["lin"], o["val"], 2, 16, 64)),
        ("lpips_tap_bwd", dict(feats=t(BF, 4, 16, 64), lin=t(F32, 64), gscale=t(F32, 1)),
         lambda H, o: H.lpips_tap_bwd(o["feats"], o["lin"], 0.5, 2, 16, 64, gscale=o["gscale"])),
        ("l1_mean", dict(a=t(F32, 40), b=t(F32, 40), out=t(F32, 1)), lambda H, o: H.l1_mean(o["a"], o["b"], o["out"])),
        ("eval_moments", dict(pair, clim=t(F32, C, Hh, W)),
         lambda H, o: H.eval_moments(o["pred"], o["target"], o["lat_w"], o["clim"])),
        ("masked_loss_fwd", dict(mask),
         lambda H, o: H.masked_loss_fwd(o["pred"], o["target"], o["lat_w"], o["chan_w"], 1, o["mask"], ms)),
        ("masked_loss_bwd", dict(mask, gscale=t(F32, 1), cnt=t(torch.int64, C + 1)),
         lambda H, o: H.masked_loss_bwd(o["pred"], o["target"], o["lat_w"], o["chan_w"], o["gscale"], o["cnt"], 0, o["mask"], ms)),
        ("masked_moments", dict(gk(mask, "pred", "target", "lat_w", "mask"), clim=t(F32, C, Hh, W)),
         lambda H, o: H.masked_moments(o["pred"], o["target"], o["lat_w"], o["clim"], o["mask"], ms)),
        ("masked_moments", dict(gk(pair, "pred", "target")), lambda H, o: H.masked_moments(o["pred"], o["target"])),
        ("ensemble_update", dict(member=t(F32, 4, 5), mean=t(F32, 4, 5), m2=t(F32, 4, 5)),
         lambda H, o: H.ensemble_update(o["member"], o["mean"], o["m2"], 2)),
        ("gaussian_scores", dict(pair, std=t(F32, B, C, Hh, W)),
         lambda H, o: H.gaussian_scores(o["pred"], o["std"], o["target"], o["lat_w"])),
        ("ensemble_scores", dict(gk(pair, "target", "lat_w"), members=t(F32, 3, B, C, Hh, W)),
         lambda H, o: H.ensemble_scores(o["members"], o["target"], o["lat_w"], hist=True, seed=11, crps_field="fair",
                                        quantiles=(0.1, 0.9))),
        ("ssim_sums", dict(pair), lambda H, o: H.ssim_sums(o["pred"], o["target"], o["lat_w"], data_range=2.0, ssim_map=True)),
        ("resample", dict(x=t(F32, 2, 4, 4, 6), out=t(F32, 2, 2, 8, 12)),
         lambda H, o: H.resample(o["x"], (8, 12), "bicubic", channels=[3, 1], scale=[1.0, 2.0], shift=[0.0, 1.0], out=o["out"])),
        ("resample_moments", dict(gk(pair, "target", "lat_w"), x=t(F32, B, C, 4, 6), clim=t(F32, C, Hh, W)),
         lambda H, o: H.resample_moments(o["x"], (Hh, W), "bilinear", o["target"], lat_w=o["lat_w"], clim=o["clim"])),
        ("seed_salt", {}, lambda H, o: H.seed_salt((1 << 64) - 3, add=True)),
    ]


CASES = _cases()
IDS = ["%s-%d" % (c[0], i) for i, c in enumerate(CASES)]
OPERANDS = [(i, k) for i, c in enumerate(CASES) for k in c[1]]
OPERAND_IDS = ["%s-%d-%s" % (CASES[i][0], i, k) for i, k in OPERANDS]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_valid_call_reaches_its_entries_with_the_stream_last(hip, case):
    name, operands, call = case
    call(hip, operands)
    launches = [(n, a) for n, a in hip.stub.calls if not is_query(n)]
    assert launches, name
    for entry, args in launches:
        assert args[-1] == STREAM, entry
        given = {v.data_ptr() for v in operands.values()}
        block = args[0]
        if entry.startswith("orbit2_gemm"):                     # the operands of a GEMM travel in its argument block(s)
            blocks = [block._obj] if type(block).__name__ == "CArgObject" else list(block)
            sent = {getattr(b, f) for b in blocks for f, kind in b._fields_ if kind is ctypes.c_void_p}
            sent |= {p for a in args[1:-1] if isinstance(a, ctypes.Array) for p in a}
        else:
            sent = set()
        sent |= {a for a in args[:-1] if isinstance(a, int)}
        assert given <= sent, "%s: an operand never reached %s" % (name, entry)


def test_every_entry_is_reached_or_named(hip):
    for _, operands, call in CASES:
        call(hip, operands)
    reached = {n for n, _ in hip.stub.calls}
    assert set(NOT_REACHED) <= set(hip.PROTOTYPES) and not reached & set(NOT_REACHED)
    assert set(hip.PROTOTYPES) - reached == set(NOT_REACHED)


@pytest.mark.parametrize("where", OPERANDS, ids=OPERAND_IDS)
def test_host_operand_is_refused_before_any_entry(hip, where):
    i, key = where
    _, operands, call = CASES[i]
    bad = operands[key].clone()
    bad.flagged_host = True
    with pytest.raises(hip.HipBackendError, match="GPU tensor"):
        call(hip, dict(operands, **{key: bad}))
    assert hip.stub.calls == []


@pytest.mark.parametrize("where", OPERANDS, ids=OPERAND_IDS)
def test_wrong_dtype_is_refused_before_any_entry(hip, where):
    """float64 is read by no entry as an operand a caller supplies (the float64 outputs are the wrappers' own)"""
    i, key = where
    _, operands, call = CASES[i]
    bad = torch.zeros(operands[key].shape, dtype=torch.float64)
    with pytest.raises(hip.HipBackendError):
        call(hip, dict(operands, **{key: bad}))
    assert hip.stub.calls == []


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_nonzero_code_names_the_entry(hip, case):
    name, operands, call = case
    hip.stub.rc = -1
    with pytest.raises(hip.HipBackendError) as err:
        call(hip, operands)
    entry = [n for n, _ in hip.stub.calls if not is_query(n)][-1]
    assert str(err.value).startswith("%s failed with code -1 " % entry)


def test_pointer_of_a_host_tensor_is_refused(hip):
    """_p is the one place an address is produced: whatever a wrapper forgot, no host pointer reaches an entry"""
    x = torch.zeros(4)
    assert hip._p(None) is None and hip._p(x) == x.data_ptr()
    x.flagged_host = True
    with pytest.raises(hip.HipBackendError, match="GPU tensor"):
        hip._p(x)
    with pytest.raises(hip.HipBackendError, match="GPU tensor"):
        hip._call("orbit2_l1_mean", x, x, x, 4, x)
    assert hip.stub.calls == []
