"""LayerNorm forward / backward at every kernel instantiation and partition edge (csrc/norm_elem.hip: ln_chunks, ln_bwd_plan),
against the float64 reference of tests/rowimage_ref.py on the bf16-rounded inputs.

Error measure: y and dx per row, dgamma / dbeta per column, never over the whole tensor.
  bf16 outputs (y, dx, bf16 sinks): |got - ref| <= 2^-8 |ref| + 4 b   -- one bf16 rounding, plus 4 x the fp32 baseline's largest
                                    absolute error b in that row (the same formulas in fp32 on the CPU; the factor 4 is the margin
                                    test_layernorm_fwd_f32_large_offset_relative_bound uses for a wave-tree sum against torch's order)
  fp32 outputs (mean, rstd, fp32 sinks): |got - ref| <= 4 b on every element.
For the one-dimensional outputs (mean, rstd, dgamma, dbeta) a "row" or "column" is one number, and one sample of a rounding error
bounds nothing (two correct fp32 sums differ by more than 4 x in one element out of six, and the mean of eight bf16 values is exact):
their b is the baseline's largest error over the vector -- for mean / rstd over the 130 rows every case is a prefix of -- and never
less than one fp32 rounding of the vector's largest magnitude (rowimage_ref.fp32_floor).  Every element is still held to it alone.
No bound is derived from the kernel's output.  Each test prints the share of its bound every output used ("[edge] ...").
"""
import functools

import pytest
import torch

from tests import rowimage_ref as R

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def hip():
    from climate_learn import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip


@functools.lru_cache(maxsize=2)
def per_row(D, nrows):
    """everything of one width that is a function of the row alone, computed once for the longest case and shared (read only):
    the float64 y, mean, rstd, dx (with and without dres) and the fp32 baseline's per-row error of each"""
    x, gam, bet, dy, dres = R.ln_inputs(D, nrows)
    ref = R.ln_fwd(x, gam, bet) + (R.ln_bwd(dy, x, gam, dres)[0], R.ln_bwd(dy, x, gam, None)[0])
    base = R.ln_fwd(x, gam, bet, dtype=F32) + (R.ln_bwd(dy, x, gam, dres, dtype=F32)[0], R.ln_bwd(dy, x, gam, None, dtype=F32)[0])
    names = ("y", "mean", "rstd", "dx", "dx_nores")
    out = {}
    for n, r, b in zip(names, ref, base):
        if r.dim() == 2:
            out[n] = (r, R.base_err(b, r, dim=1))                                    # b per row
        else:
            out[n] = (r, R.fp32_floor(R.base_err(b, r), r.abs().max()))              # b of the vector
    return out


def bf16_bound(ref, b):
    return R.EPS8 * ref.abs() + 4.0 * b


def report(tag, items):
    worst = {}
    for name, got, ref, bound in items:
        worst[name] = R.excess(got, ref, bound)
    print("[edge] ln %s " % tag + " ".join("%s %.3f" % kv for kv in worst.items()))
    bad = [n for n, e in worst.items() if not e <= 1.0]
    assert not bad, (tag, worst)


def run_case(hip, D, rows, nrows_shared):
    x, gam, bet, dy, dres = R.ln_inputs(D, rows)
    pr = per_row(D, nrows_shared)
    xd, gd, bd = x.to(BF).cuda(), gam.to(BF).cuda(), bet.to(BF).cuda()
    y, mean, rstd = hip.layernorm_fwd(xd, gd, bd)
    items = []
    (yr, yb), (mr, mb), (rr, rb) = pr["y"], pr["mean"], pr["rstd"]
    items.append(("y", y.float(), yr[:rows], bf16_bound(yr[:rows], yb[:rows, None])))
    items.append(("mean", mean, mr[:rows], 4.0 * mb.expand(rows)))
    items.append(("rstd", rstd, rr[:rows], 4.0 * rb.expand(rows)))
    dg, db = torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    dx = hip.layernorm_bwd(dy.to(BF).cuda(), xd, gd, mean, rstd, dres.to(BF).cuda(), dg, db)
    dxr, dxb = pr["dx"]
    items.append(("dx", dx.float(), dxr[:rows], bf16_bound(dxr[:rows], dxb[:rows, None])))
    _, dgr, dbr = R.ln_bwd(dy, x, gam, None)
    _, dg32, db32 = R.ln_bwd(dy, x, gam, None, dtype=F32)
    items.append(("dgamma", dg, dgr, 4.0 * R.fp32_floor(R.base_err(dg32, dgr), dgr.abs().max()).expand(D)))
    items.append(("dbeta", db, dbr, 4.0 * R.fp32_floor(R.base_err(db32, dbr), dbr.abs().max()).expand(D)))
    # no atomics anywhere: a second call gives the same bits in all three outputs
    dg2, db2 = torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    dx2 = hip.layernorm_bwd(dy.to(BF).cuda(), xd, gd, mean, rstd, dres.to(BF).cuda(), dg2, db2)
    report("D=%d rows=%d" % (D, rows), items)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)


@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("D", R.LN_WIDTHS)
def test_layernorm_every_width_and_row_tail(hip, D, rows):
    """D: one lane (8); NC 1 partial / full (200, 512); NC 2 with a masked half (768); NC 6 with its last chunk wholly masked
    (2560); NC 8 with one live lane in chunk 6 and full (3080, 4096); the row-shared backward non-exact with one live thread in
    chunk 2 and the NC 16 forward (4104), with one thread masked (8184), exact (1024, 8192).  rows: 1 and 3; the few-rows tail
    5 = 4 + 1; one row in wave 1 (17); 63 / 65 / 130 = a second block with one row, a third with two"""
    run_case(hip, D, rows, max(R.LN_ROWS))


@pytest.mark.parametrize("D,rows", R.LN_SWITCH)
def test_layernorm_partition_switch_at_32768_rows(hip, D, rows):
    """ln_shared_rpb goes from 4 to 64 rows per block at 32768 rows (D = 256: row-shared; 8192 partial rows before, 512 after);
    D = 64 keeps the per-wave form on both sides"""
    run_case(hip, D, rows, 32769)


@pytest.mark.parametrize("D", R.LN_SINK_WIDTHS)
def test_layernorm_sinks(hip, D):
    """dres = NULL; beta_acc = 1 into non-zero fp32 and bf16 sinks; beta_acc = 0 into bf16 sinks full of NaN (not read)"""
    rows = 65
    x, gam, bet, dy, _ = R.ln_inputs(D, rows)
    pr = per_row(D, max(R.LN_ROWS))
    xd, gd, dyd = x.to(BF).cuda(), gam.to(BF).cuda(), dy.to(BF).cuda()
    _, mean, rstd = hip.layernorm_fwd(xd, gd, bet.to(BF).cuda())
    dxr, dxb = pr["dx_nores"]
    g = torch.Generator().manual_seed(D)
    s0 = (R.rt(3 * torch.randn(D, generator=g)), R.rt(3 * torch.randn(D, generator=g)))
    items = []
    for tag, dtype, beta_acc, fill in (("f32+", F32, 1.0, None), ("bf16+", BF, 1.0, None), ("bf16nan", BF, 0.0, float("nan"))):
        sinks = tuple((t if fill is None else torch.full_like(t, fill)).to(dtype).cuda() for t in s0)
        dx = hip.layernorm_bwd(dyd, xd, gd, mean, rstd, None, sinks[0], sinks[1], beta_acc=beta_acc)
        _, dgr, dbr = R.ln_bwd(dy, x, gam, None, s0, beta_acc)
        _, dg32, db32 = R.ln_bwd(dy, x, gam, None, s0, beta_acc, dtype=F32)
        items.append(("dx/" + tag, dx.float(), dxr[:rows], bf16_bound(dxr[:rows], dxb[:rows, None])))
        for name, got, ref, b32 in (("dgamma/" + tag, sinks[0], dgr, dg32), ("dbeta/" + tag, sinks[1], dbr, db32)):
            b = R.fp32_floor(R.base_err(b32, ref), ref.abs().max()).expand(D)
            assert bool(torch.isfinite(got.float()).all()), name
            items.append((name, got.float(), ref, 4.0 * b if dtype == F32 else bf16_bound(ref, b)))
    report("sinks D=%d" % D, items)


@pytest.mark.parametrize("D", R.LN_WIDTHS)
def test_layernorm_forward_leaves_the_padding_alone(hip, D):
    """y with a row pitch of D + 8: the guard columns, and a guard row after the last, keep their sentinel"""
    rows = 5
    x, gam, bet, _, _ = R.ln_inputs(D, rows)
    buf = torch.full((rows + 1, D + 8), 777.0, dtype=BF, device="cuda")
    y, _, _ = hip.layernorm_fwd(x.to(BF).cuda(), gam.to(BF).cuda(), bet.to(BF).cuda(), out=buf[:rows, :D])
    yr, yb = per_row(D, max(R.LN_ROWS))["y"]
    report("pitch D=%d" % D, [("y", buf[:rows, :D].float(), yr[:rows], bf16_bound(yr[:rows], yb[:rows, None]))])
    assert bool((buf[:rows, D:] == 777.0).all()) and bool((buf[rows] == 777.0).all())
