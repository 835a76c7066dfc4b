"""tests/split_ref.py against float64: the planes reproduce their operand to the residual the module states,
and the plane-product sums sit where the GPU tests' margins assume -- three bf16 products 1e-6 .. 1e-5 off
the exact result (about 4e-6, whatever K), six below 1e-7, the fp16 pair below 1e-6."""
import pytest
import torch

import split_ref as R


def _operands(kind, m, k, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(m, k, generator=g), torch.randn(k, n, generator=g)
    return torch.rand(m, k, generator=g) + 0.5, torch.rand(k, n, generator=g) - 0.5


def test_bf16_planes_residuals():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1 << 16, generator=g) * torch.logspace(-20, 20, 1 << 16)
    p = R.planes_bf(x, 3)
    xd, ax = x.double(), x.double().abs()
    for q in p:  # every plane is a bf16 value
        assert torch.equal(q, q.to(torch.bfloat16).float())
    assert ((xd - p[0].double()).abs() <= 2.0 ** -8 * ax).all()
    assert ((xd - p[0].double() - p[1].double()).abs() <= 2.0 ** -16 * ax).all()
    assert ((xd - p[0].double() - p[1].double() - p[2].double()).abs() <= 2.0 ** -24 * ax).all()
    # the residuals are exact in fp32: the same planes from float64 residuals
    r1 = xd - p[0].double()
    assert torch.equal(r1.float().double(), r1)
    assert torch.equal(p[1], r1.float().to(torch.bfloat16).float())
    r2 = r1 - p[1].double()
    assert torch.equal(r2.float().double(), r2)
    assert torch.equal(p[2], r2.float().to(torch.bfloat16).float())


def test_fp16_pair_residual():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1 << 16, generator=g) * torch.logspace(-6, 0, 1 << 16)
    s = R.h16_exp(float(x.abs().max()))
    assert 2.0 ** 14 <= float(x.abs().max()) * 2.0 ** s < 2.0 ** 15
    h0, h1 = R.planes_h16(x, s)
    xs = x.double() * 2.0 ** s
    err = (xs - h0.double() - h1.double()).abs()
    assert (err <= torch.maximum(2.0 ** -22 * xs.abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all()
    assert R.h16_exp(0.0) == 0 and R.h16_exp(1.0) == 14 and R.h16_exp(1e3) == 5
    w = torch.randn(4096, generator=g) * 0.05  # weights at the fixed exponent: |w| < 64 fits, every bit above 2^-13
    h0, h1 = R.planes_h16(w, R.H16_WS)
    ws = w.double() * 2.0 ** R.H16_WS
    assert ((ws - h0.double() - h1.double()).abs() <= torch.clamp(2.0 ** -22 * ws.abs(), min=2.0 ** -25)).all()


@pytest.mark.parametrize("kind", ["normal", "uniform"])
@pytest.mark.parametrize("k", [256, 4096, 65536])
def test_plane_products_against_float64(kind, k):
    a, b = _operands(kind, 32, k, 32, 3 + k)
    mm = lambda p, q: p @ q
    ref = a.double() @ b.double()
    e3 = R.rel_l2(R.plane_products(mm, a, b, 2), ref)
    e6 = R.rel_l2(R.plane_products(mm, a, b, 3), ref)
    eh = R.rel_l2(R.h16_products(mm, a, b, sb=R.h16_exp(float(b.abs().max()))), ref)
    e32 = R.rel_l2(a @ b, ref)
    print("%s K=%d: three products %.2e, six %.2e, fp16 pair %.2e, fp32 matmul %.2e" % (kind, k, e3, e6, eh, e32))
    assert 1e-6 <= e3 <= 1e-5
    assert e6 < 1e-7
    assert eh < 1e-6
