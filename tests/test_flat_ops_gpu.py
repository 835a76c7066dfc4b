"""Flat-generator kernels (csrc/flat.hip) through svae_op_flat_conv / _dgrad / _wgrad against
oracle.torch_twin.conv2d_same in float64 with autograd; bounds of tests/test_ops_gpu.py:
max|err| <= tol * (1 + max|ref|), tol 2e-5 forward and dgrad, 5e-5 wgrad.  Plain fp32 arithmetic (torch
CPU float32) on exactly these cases is 6e-7 / 2.3e-7 / 1.9e-6 off on that scale, so only a wrong tap,
pad or tail can exceed the bounds."""
import numpy as np
import pytest
import torch

from conftest import pkg_mod
from oracle import torch_twin as TT

pytestmark = pytest.mark.gpu

# n, h, cin, cout: images smaller than one block, a pixel count that is no multiple of the block,
# every reference channel pair of C = 3, the C = 1 extremes, both engine widths
CASES = [(3, 4, 3, 6), (2, 8, 6, 12), (1, 32, 12, 24), (2, 32, 24, 12), (3, 8, 12, 6), (2, 32, 6, 3),
         (3, 4, 1, 2), (2, 8, 8, 4), (1, 64, 3, 6), (1, 64, 24, 12)]


def _lib():
    return pkg_mod("_lib")


def _rand(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, size=shape).astype(np.float32))


def _ref_conv(x, w):
    return TT.conv2d_same(x.double().permute(0, 3, 1, 2), w.double(), 1).permute(0, 2, 3, 1)


def _close(got, ref, tol=2e-5):
    err = (got.double().cpu() - ref).abs().max().item()
    print("max|err| %.3e scale %.3e" % (err, 1 + ref.abs().max().item()))
    assert err <= tol * (1 + ref.abs().max().item()), err


def _fwd(L, xd, wd, n, h, cin, cout, bn=None, stats=False):
    y = torch.zeros(n, h, h, cout, device="cuda")
    st = torch.zeros(2 * cout, device="cuda") if stats else None
    m, i, b = bn if bn is not None else (None, None, None)
    L.check(L.lib().svae_op_flat_conv(L.ptr(xd), n, h, cin, L.ptr(wd), cout, L.ptr(m), L.ptr(i), L.ptr(b), L.ptr(y),
                                      L.ptr(st), L.stream_ptr()))
    torch.cuda.synchronize()
    return y, st


@pytest.mark.parametrize("case", CASES)
def test_flat_conv_fwd(case):
    n, h, cin, cout = case
    L = _lib()
    x, w = _rand((n, h, h, cin), 1), _rand((4, 4, cin, cout), 2) * 0.2
    xd, wd = x.cuda(), w.cuda()
    y, _ = _fwd(L, xd, wd, n, h, cin, cout)
    _close(y, _ref_conv(x, w))
    y2, _ = _fwd(L, xd, wd, n, h, cin, cout)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("case", CASES)
def test_flat_conv_fused_input_and_stats(case):
    """in_mean / in_invstd / in_beta: the conv reads lrelu(bn(x)), zeros padded AFTER the activation;
    stats_out = (sum, sum of squares) of y per channel, each column held to 1e-5 relative to the float64
    column sum of the reference."""
    n, h, cin, cout = case
    L = _lib()
    x, w = _rand((n, h, h, cin), 3) * 2 + 0.3, _rand((4, 4, cin, cout), 4) * 0.2
    mean, inv, beta = _rand((cin,), 5) * 0.5, _rand((cin,), 6).abs() + 0.5, _rand((cin,), 7) * 0.3
    z = (x.double() - mean.double()) * inv.double() + beta.double()
    act = torch.maximum(torch.minimum(0.1 * z, torch.zeros_like(z)), z)
    ref = _ref_conv(act, w)
    bn = (mean.cuda(), inv.cuda(), beta.cuda())
    y, st = _fwd(L, x.cuda(), w.cuda(), n, h, cin, cout, bn, True)
    _close(y, ref)
    st = st.double().cpu().view(cout, 2)
    s1, s2 = ref.reshape(-1, cout).sum(0), (ref.reshape(-1, cout) ** 2).sum(0)
    r1, r2 = ((st[:, 0] - s1).abs() / s1.abs()).max().item(), ((st[:, 1] - s2).abs() / s2.abs()).max().item()
    print("per-column relative error: sum %.3e, sum of squares %.3e (min |sum| / max |sum| %.2e)"
          % (r1, r2, (s1.abs().min() / s1.abs().max()).item()))
    assert r2 <= 1e-5, r2
    assert r1 <= 1e-5, r1
    y2, st2 = _fwd(L, x.cuda(), w.cuda(), n, h, cin, cout, bn, True)
    assert torch.equal(y, y2) and torch.equal(st.float(), st2.cpu().view(cout, 2))


# over 1024 row groups: a weight-gradient block then sums several groups (here 2, and the last block 1)
@pytest.mark.parametrize("case", CASES + [(151, 40, 3, 6)])
def test_flat_conv_dgrad_wgrad(case):
    n, h, cin, cout = case
    L = _lib()
    x = _rand((n, h, h, cin), 3).double().requires_grad_(True)
    w = (_rand((4, 4, cin, cout), 4) * 0.2).double().requires_grad_(True)
    y = _ref_conv(x, w)
    dy = _rand(tuple(y.shape), 5).double()
    (y * dy).sum().backward()
    dyd, wd, xd = dy.float().cuda(), w.detach().float().cuda(), x.detach().float().cuda()
    scratch = torch.empty(4 << 20, device="cuda")

    def run():
        dx = torch.zeros(n, h, h, cin, device="cuda")
        dw = torch.zeros(4, 4, cin, cout, device="cuda")
        L.check(L.lib().svae_op_flat_dgrad(L.ptr(dyd), n, h, cin, L.ptr(wd), cout, L.ptr(dx), L.stream_ptr()))
        L.check(L.lib().svae_op_flat_wgrad(L.ptr(xd), n, h, cin, L.ptr(dyd), cout, L.ptr(dw), L.ptr(scratch),
                                           scratch.numel() * 4, L.stream_ptr()))
        torch.cuda.synchronize()
        return dx, dw

    dx, dw = run()
    _close(dx, x.grad)
    _close(dw, w.grad, tol=5e-5)
    dx2, dw2 = run()
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)


def test_flat_ops_reject_what_does_not_fit():
    L = _lib()
    t = torch.zeros(16, device="cuda")
    args = (L.ptr(t), 1, 8, 33, L.ptr(t), 4, None, None, None, L.ptr(t), None, L.stream_ptr())
    assert L.lib().svae_op_flat_conv(*args) == -1           # more than 32 channels
    assert L.lib().svae_op_flat_dgrad(L.ptr(t), 1, 512, 3, L.ptr(t), 3, L.ptr(t), L.stream_ptr()) == -1  # a row over 256 pixels
