"""Same-box, same-process A/B of two builds of the variable-aggregation kernels (csrc/varagg.hip):
    tools/ab_build.sh <git-rev> <name>;   on the GPU box:  python tools/varagg_lib_ab.py orbit-2_amd/lib/alt/<name>.so [other.so]
tools/lib_ab.py loads the two builds, keeps the guarded buffers, times and sums up; this file calls every entry of varagg.hip in
both.  Cases, all taken from the test modules: tests/test_patch_size_gpu.py's KCASES and the shapes of
tests/test_hip_ops.py::test_varagg_fold_matches_dense_oracle (B = 2, patch 2), each through the bf16 forward, the fp32 forward with
and without attw, the backward, at patch 2 through the plain entries and their `_p` twins, with the workspace and fixed-order
queries of both; orbit2_tables_gather / _scatter at the V, D and pitches of tests/test_elementwise_ops_gpu.py.
Rules: every forward output, the gather / scatter outputs and every backward whose `is_fixed_order` query says 1 (the MFMA path, all
of patch 1 and 4) are bitwise equal, guard bands and workspace included.  The scalar backward adds with atomics (fp32 in HBM for
the tables once per 16 tokens, LDS for da once per 4 channels of a head): ATOMICS_ONE below, where every sum has one contributor,
is bitwise equal too; at the other shapes two runs of ONE build may differ, so the alt build (the parent) runs five times on the
same inputs, `noise` = the largest elementwise difference between any two of its results over the largest magnitude of the
float64 table, and the builds may differ by at most 4 x noise (0 -> bitwise); both must be within 5e-5 (the tests' bound) of the
float64 tables computed on the host from the same attw and dz.  The line shows the three figures.
Then forward and backward are timed, both builds interleaved: tools/varagg_bench.py's first two shapes at B = 4, patch 4 at
tools/patch_size_bench.py's interm_117m leg, the scalar backward at D = 256, H = 4, V = 30 on a 32 x 64 grid.  Exit status 1 if a
rule is broken."""
import itertools
import torch
from lib_ab import BITS, GUARD, P, S, count, guarded, libs, ok, summary, tally
from oracle.harness import ERA5_VARS
from tests import test_hip_ops, test_patch_size_gpu

BF, F32 = torch.bfloat16, torch.float32
FOLD_SHAPES = test_hip_ops.test_varagg_fold_matches_dense_oracle.pytestmark[0].args[1]        # (D, heads, V, hw)
CASES = [(name,) + c for name, c in test_patch_size_gpu.KCASES.items()] + [("fold", D, H, V, hw, 2, 2) for D, H, V, hw in FOLD_SHAPES]
ATOMICS_ONE = ("one contributor", 16, 4, 5, (4, 8), 1, 2)         # 8 tokens: one workgroup; head dim 4: one chunk per head
TOL_TABLES = 5e-5


def compare(kind, tag, call, dests, timing=False):
    """call(lib, one address per destination) in both builds.  dests: (elements, dtype, prefill or None, must be written); every
    buffer whole, bit for bit.  Returns the tree build's destinations."""
    G = [guarded(n, dtype, prefill=pre) for n, dtype, pre, _ in dests]
    run = lambda lib, key: ok(call(lib, *[g[key].data_ptr() + GUARD * g[key].element_size() for g in G]))
    for key, lib in libs.items(): run(lib, key)
    torch.cuda.synchronize()
    eq = all(torch.equal(g["tree"].view(BITS[d[1]]), g["alt"].view(BITS[d[1]])) for g, d in zip(G, dests)) \
        and not any(d[3] and bool(torch.isnan(g["tree"][GUARD:GUARD + d[0]]).any()) for g, d in zip(G, dests))
    tally(kind, "%-12s %s: bitwise equal %s" % (kind, tag, eq), eq, run if timing else None, {key: key for key in libs})
    return [g["tree"][GUARD:GUARD + d[0]] for g, d in zip(G, dests)]


def agree(kind, what, args):
    """a query of both builds gives one answer"""
    n = {k: getattr(lib, what)(*args) for k, lib in libs.items()}
    count.setdefault(kind, [0, 0])
    count[kind][0] += 1; count[kind][1] += n["tree"] == n["alt"]
    if n["tree"] != n["alt"]: print("%s%r: tree %d, alt %d" % (what, args, n["tree"], n["alt"]), flush=True)
    return n["tree"]


def inputs(D, H, V, hw, B, patch, seed=5):
    g = torch.Generator().manual_seed(seed)
    C, ntok = patch * patch + 1, B * (hw[0] // patch) * (hw[1] // patch)
    return (torch.randn(B, V, *hw, generator=g).cuda(), (0.3 * torch.randn(H, V, C, generator=g)).cuda(),
            (0.2 * torch.randn(V, C, D, generator=g)).cuda(), torch.randn(ntok, D, generator=g).to(BF).cuda(), ntok)


def tables64(x, gtab, attw, dz, H, patch):
    """the float64 dstab, dgtab of csrc/varagg.hip's header, on the host"""
    x, gtab, attw, dz = (v.double().cpu() for v in (x, gtab, attw, dz))
    B, V, h, w = x.shape
    D, ntok = gtab.shape[2], attw.numel() // (H * V)
    pt = x.view(B, V, h // patch, patch, w // patch, patch).permute(0, 2, 4, 1, 3, 5).reshape(ntok, V, patch * patch)
    pt = torch.cat([pt, torch.ones(ntok, V, 1, dtype=torch.float64)], 2)                         # [tokens, V, C]
    a, dzh = attw.view(ntok, H, V), dz.view(ntok, H, D // H)
    da = torch.einsum("thi,vchi,tvc->thv", dzh, gtab.view(V, -1, H, D // H), pt)
    ds = a * (da - (a * da).sum(-1, keepdim=True))
    return torch.einsum("thv,tvc->hvc", ds, pt), torch.einsum("thv,tvc,thi->vchi", a, pt, dzh).reshape(V, -1, D)


def forward_case(name, D, H, V, hw, B, patch, timing=False):
    x, st, gt, dz, ntok = inputs(D, H, V, hw, B, patch)
    tag = "%s D=%d H=%d V=%d %dx%d B=%d patch %d" % ((name, D, H, V) + tuple(hw) + (B, patch))
    h, w = hw
    zs = lambda dtype: [(ntok * D, dtype, None, True), (ntok * H * V, F32, None, True)]
    forms = [("_p", (patch,))] + ([("", ())] if patch == 2 else [])                                # the plain entries are patch 2
    for sfx, pa in forms[-1 if timing else 0:]:
        z, attw = compare("fwd" + sfx, tag, lambda lib, zp, ap: getattr(lib, "orbit2_varagg_fwd" + sfx)(
            P(x), P(st), P(gt), zp, ap, B, V, h, w, *pa, H, D, S()), zs(BF), timing)
        if timing: continue
        compare("fwd_f32" + sfx, tag, lambda lib, zp, ap: getattr(lib, "orbit2_varagg_fwd_f32" + sfx)(
            P(x), P(st), P(gt), zp, ap, B, V, h, w, *pa, H, D, S()), zs(F32))
        compare("fwd_f32" + sfx, tag + " attw NULL", lambda lib, zp: getattr(lib, "orbit2_varagg_fwd_f32" + sfx)(
            P(x), P(st), P(gt), zp, None, B, V, h, w, *pa, H, D, S()), zs(F32)[:1])
    return x, gt, attw.clone(), dz, ntok, tag, forms


def backward_case(name, D, H, V, hw, B, patch, timing=False, one_contributor=False):
    x, gt, attw, dz, ntok, tag, forms = forward_case(name, D, H, V, hw, B, patch, timing)
    h, w = hw
    C = patch * patch + 1
    ref = None
    for sfx, pa in forms[-1 if timing else 0:]:
        q = (B, V, h, w) + pa + (H, D)
        n = agree("queries", "orbit2_varagg_bwd%s_ws_floats" % sfx, q)
        fixed = agree("queries", "orbit2_varagg_bwd%s_is_fixed_order" % sfx, q)
        assert n > 0, (tag, n)
        dests = [(H * V * C, F32, 0.5, True), (V * C * D, F32, 0.5, True), (n, F32, None, False)]
        call = lambda lib, sp, gp, wp: getattr(lib, "orbit2_varagg_bwd" + sfx)(P(x), P(gt), P(attw), P(dz), sp, gp, B, V, h, w,
                                                                               *pa, H, D, wp, S())
        if fixed or one_contributor:
            compare(("bwd%s fixed" % sfx) if fixed else "bwd atomics", tag, call, dests, timing)
            continue
        # the scalar backward at a shape where the atomics have several contributors: the parent's own run-to-run noise decides
        ref = ref or tables64(x, gt, attw, dz, H, patch)

        def once(lib):
            G = [guarded(m, dt, prefill=pre) for m, dt, pre, _ in dests]
            ok(call(lib, *[g["tree"].data_ptr() + GUARD * 4 for g in G]))
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(g["tree"][:GUARD]).all()) and bool(torch.isnan(g["tree"][GUARD + d[0]:]).all())
                       for g, d in zip(G, dests)), "guard band written"
            return [g["tree"][GUARD:GUARD + d[0]].double().cpu() - 0.5 for g, d in zip(G[:2], dests)]
        parent = [once(libs["alt"]) for _ in range(5)]
        tree = once(libs["tree"])
        mags = [float(r.abs().max()) for r in ref]
        rel = lambda a, b: max(float((u - v.reshape(u.shape)).abs().max()) / m for u, v, m in zip(a, b, mags))
        noise = max(rel(p, q_) for p, q_ in itertools.combinations(parent, 2))
        diff, err_t, err_p = rel(tree, parent[0]), rel(tree, ref), max(rel(p, ref) for p in parent)
        passed = diff <= 4 * noise and max(err_t, err_p) < TOL_TABLES
        run = lambda lib, key: ok(call(lib, P(scratch[0]), P(scratch[1]), P(scratch[2])))
        scratch = [torch.zeros(m, device="cuda") for m, _, _, _ in dests] if timing else None
        tally("bwd%s atomics" % sfx, "%-12s %s: tree - parent %.3g, parent's noise over 5 runs %.3g (bound 4 x), to float64 tree %.3g "
              "parent %.3g (bound %.0e): within %s" % ("bwd%s atomics" % sfx, tag, diff, noise, err_t, err_p, TOL_TABLES, passed), passed,
              run if timing else None, {key: key for key in libs})


def tables_case(D):
    """the layout of tests/test_elementwise_ops_gpu.py::test_tables_gather_scatter: 5 of 7 variables, pitches larger than the rows"""
    VT, ids = 7, [5, 0, 3, 6, 2]
    V, ws, bs = len(ids), 4 * D + 8, D + 3
    g = torch.Generator().manual_seed(D)
    flat, E = torch.randn(VT * ws + VT * bs, generator=g).cuda(), torch.randn(VT, D, generator=g).cuda()
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    cm, = compare("gather", "V=%d D=%d" % (V, D), lambda lib, o: lib.orbit2_tables_gather(
        P(flat), ws, P(flat) + 4 * VT * ws, bs, P(E), P(ids_t), o, V, D, S()), [(5 * V * D, F32, None, True)])
    dc = cm.clone()
    g0, e0 = torch.randn(VT * ws + VT * bs, generator=g).cuda(), torch.randn(VT * D, generator=g).cuda()
    compare("scatter", "V=%d D=%d" % (V, D), lambda lib, go, eo: lib.orbit2_tables_scatter(
        P(dc), go, ws, go + 4 * VT * ws, bs, eo, P(ids_t), V, D, S()), [(g0.numel(), F32, g0, True), (e0.numel(), F32, e0, True)])


def main():
    for case in CASES:
        backward_case(*case)
    backward_case(*ATOMICS_ONE, one_contributor=True)
    for D in (64, 200):
        tables_case(D)
    V = len(ERA5_VARS)
    for name, D, H, Vc, hw, B, patch in (("timed", 3072, 24, 23, (128, 256), 4, 2), ("timed", 1024, 16, 23, (32, 64), 4, 2),
                                         ("timed interm_117m", 1024, 16, V, (32, 64), 8, 4), ("timed scalar", 256, 4, 30, (32, 64), 4, 2)):
        backward_case(name, D, H, Vc, hw, B, patch, timing=True)
    summary()


main()
