"""AdamW and check_finite (csrc/norm_elem.hip) at the sizes where they take another path: fewer than four elements, a tail after
whole float4 groups, no bf16 copy, a second trip of the grid-stride loop (more than 4096 x 1024 elements for adamw_kernel, more
than 4096 x 256 for check_finite_kernel), both gradient types.  Reference: tests/rowimage_ref.adamw_step in float64, fed the
gradient values and the fp32 scalars the kernel reads."""
import pytest
import torch

from tests import rowimage_ref as R

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
TRIP = 4096 * 1024                       # elements of one trip of adamw_kernel's loop (4096 blocks x 256 threads x 4)
ADAMW_N = (1, 2, 3, 4, 5, 1023, TRIP + 5)


@pytest.fixture(scope="module")
def hip():
    from climate_learn import _hip
    _hip.lib()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip


def slices(n):
    """the whole buffer, its last five elements, and what lies past the first trip: each is held to the bound on its own"""
    out = [("all", slice(0, n)), ("last5", slice(max(0, n - 5), n))]
    if n > TRIP:
        out.append(("trip2", slice(TRIP, n)))
    return out


@pytest.mark.parametrize("with_p16", [True, False])
@pytest.mark.parametrize("gdtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_three_steps(hip, n, gdtype, with_p16):
    g = torch.Generator().manual_seed(40 + n % 1000)
    p0 = torch.randn(n, generator=g)
    grads = [(torch.randn(n, generator=g) * 4.0).to(gdtype) for _ in range(3)]
    fi = torch.zeros(1, device="cuda")                              # a found_inf of 0: the step must happen
    pd, md, vd = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p16 = torch.full((n,), 7.0, dtype=BF, device="cuda") if with_p16 else None
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step, gr in enumerate(grads, 1):
        hip.adamw(pd, md, vd, gr.cuda(), p16, n, step=step, grad_scale=0.25, found_inf=fi, **R.ADAMW)
        pr, mr, vr = R.adamw_step(pr, gr, mr, vr, step, grad_scale=0.25)
    for name, got, ref in (("p", pd, pr), ("m", md, mr), ("v", vd, vr)):
        for tag, sl in slices(n):
            err = float((got[sl].cpu().double() - ref[sl]).abs().max())
            scale = float(ref[sl].abs().max())
            print("[edge] adamw n=%d %s p16=%d %s/%s %.3e of the maximum" % (n, gdtype, with_p16, name, tag, err / scale))
            assert err <= 1e-6 * scale, (name, tag)
    if with_p16:
        assert torch.equal(p16, pd.to(BF))
    assert fi.item() == 0.0


@pytest.mark.parametrize("gdtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_skipped_step_changes_nothing(hip, n, gdtype):
    g = torch.Generator().manual_seed(41 + n % 1000)
    p, m, v = (torch.randn(n, generator=g).cuda() for _ in range(3))
    v = v.abs()
    p16 = torch.randn(n, generator=g).to(BF).cuda()
    before = [t.clone() for t in (p, m, v, p16)]
    gr = torch.randn(n, generator=g).to(gdtype).cuda()
    hip.adamw(p, m, v, gr, p16, n, step=2, grad_scale=0.25, found_inf=torch.ones(1, device="cuda"), **R.ADAMW)
    for a, b in zip(before, (p, m, v, p16)):
        assert torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))


FIN_TRIP = 4096 * 256                    # elements of one trip of check_finite_kernel's loop


@pytest.mark.parametrize("gdtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 63, 64, FIN_TRIP + 3])
def test_check_finite(hip, n, gdtype):
    g = torch.Generator().manual_seed(42)
    clean = ((torch.rand(n, generator=g) * 2 - 1) * 2.9e38).to(gdtype)
    clean[0], clean[n - 1] = 2.9e38, -2.9e38
    assert bool(torch.isfinite(clean.float()).all()) and float(clean.float().abs().max()) > 2.8e38
    buf = clean.cuda()
    flag = torch.zeros(1, device="cuda")
    hip.check_finite(buf, n, flag)
    assert flag.item() == 0.0                                      # values up to +-2.9e38 are finite: exactly 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        for at in sorted(a for a in {0, n - 1, FIN_TRIP} if a < n):
            buf = clean.cuda()
            buf[at] = bad
            flag = torch.zeros(1, device="cuda")
            hip.check_finite(buf, n, flag)
            assert flag.item() == 1.0, (bad, at)
    flag = torch.ones(1, device="cuda")
    hip.check_finite(clean.cuda(), n, flag)
    assert flag.item() == 1.0                                      # a flag already set stays set
