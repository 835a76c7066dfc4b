"""The split mode's conv weight gradients (dtype bf16x6: two bf16 planes per operand, three plane products)
through svae_op_wgrad_bf16 with the split bit (path | 64): wgrad_halo2_kernel<..., NSP = 2> with its
128-pixel-chunk instances, wgrad_smallc_kernel<CI, 2> and the tap-merged wgrad_bf16_kernel<..., NSP = 2>
that takes every layer wgrad_halo2 refuses (the 4x4 layers among them).  Every case asserts the kernel the
library reports for the call (svae_op_wgrad_last_kernel) and makes two comparisons, both with references:

1. with the plane model of the same fp32 operands (tests/split_ref.py plane_products, NS = 2, products and
   sums in float64): only the fp32 accumulation order differs, so the bound is the fp32 one of
   test_split_gather_gpu.py, 2e-6 relative L2 and 2e-5 of max|ref| pointwise;
2. with float64 autograd of the unrounded operands (oracle/torch_twin.py): at most twice the plane model's
   own relative L2 error against the same float64 result, computed here per case (about 4e-6, tests/
   test_split_ref.py; the factor leaves room for the fp32 accumulation on top).

Shapes are the smallest that reach each instance.  Measured: profiles/split_wgrad_dense_parity.txt."""
import pytest
import torch

import split_ref as R
from conftest import pkg_mod
from oracle import torch_twin

pytestmark = pytest.mark.gpu

TAP_MERGED, HALO, HALO2, SMALLC = 1, 2, 3, 4  # include/svae_hip.h SVAE_WGRAD_*

# (n, h_in, cin, cout, stride, transpose), path, kernel, x distribution
CASES = [
    # wgrad_halo2 NSP = 2
    ((4, 8, 32, 32, 1, 0), 2, HALO2, "randn"),      # two 128-pixel chunks in one split, gradient written directly
    ((1, 16, 32, 32, 2, 0), 2, HALO2, "randn"),     # one 64-pixel chunk, gradient written directly
    ((16, 8, 128, 128, 1, 0), 2, HALO2, "randn"),   # two splits: slab plus wgrad_reduce
    ((1, 16, 64, 64, 1, 0), 2, HALO2, "randn"),     # 128-pixel chunks, a chunk is half an image
    ((2, 16, 64, 32, 1, 1), 2, HALO2, "randn"),     # conv-T, 32-column tile (WN = 1)
    ((1, 32, 32, 32, 1, 0), 2, HALO2, "randn"),     # 32-wide, 128-pixel chunks
    ((4, 16, 32, 64, 2, 0), 2, HALO2, "randn"),     # stride 2, 64-pixel chunks
    ((4, 8, 128, 64, 2, 1), 2, HALO2, "randn"),
    # tap-merged NSP = 2: the layers wgrad_halo2 refuses
    ((4, 4, 128, 128, 1, 0), 2, TAP_MERGED, "randn"),   # the 4x4 layers
    ((8, 8, 128, 128, 2, 0), 2, TAP_MERGED, "randn"),
    ((4, 4, 384, 128, 2, 1), 2, TAP_MERGED, "randn"),
    ((3, 8, 8, 8, 2, 0), 2, TAP_MERGED, "randn"),       # M, N < 32
    ((3, 4, 16, 24, 2, 0), 2, TAP_MERGED, "randn"),     # row-space width 2: the scalar gather
    ((3, 8, 32, 32, 1, 0), 2, TAP_MERGED, "randn"),     # rows not a multiple of the chunk
    # 128 rows: wgrad_halo2_ok asks for whole 256-pixel chunks at this width although the split instances
    # walk 128-pixel ones, so a single 128-pixel chunk never reaches wgrad_halo2
    ((2, 8, 32, 32, 1, 0), 2, TAP_MERGED, "randn"),
    # tap-merged on a layer the halo kernel would take (several splits through the slab)
    ((16, 8, 128, 128, 1, 0), 0, TAP_MERGED, "randn"),
    # wgrad_smallc NSP = 2: image convs and the output conv-T
    ((2, 64, 3, 32, 2, 0), 2, SMALLC, "randn"),
    ((2, 64, 1, 64, 2, 0), 2, SMALLC, "randn"),
    ((2, 32, 32, 4, 2, 1), 2, SMALLC, "randn"),
    # post-lrelu activations are not zero-mean
    ((1, 16, 64, 64, 1, 0), 2, HALO2, "act"),
    ((4, 4, 128, 128, 1, 0), 2, TAP_MERGED, "act"),
]


def _id(c):
    s, path, kern, dist = c
    return "n%d_h%d_%dto%d_s%d_%s_p%d_%s" % (s[0], s[1], s[2], s[3], s[4], "T" if s[5] else "C", path, dist)


def _wgrad64(shape):
    """dW of the TF-SAME conv / conv-T as a function of float64 NHWC (x, dy): linear in each."""
    n, h, cin, cout, s, tr = shape
    wshape = (4, 4, cout, cin) if tr else (4, 4, cin, cout)

    def f(x, dy):
        w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
        xr = x.permute(0, 3, 1, 2)
        y = torch_twin.conv2d_t_same(xr, w, s) if tr else torch_twin.conv2d_same(xr, w, s)
        return torch.autograd.grad(y, w, dy.permute(0, 3, 1, 2))[0]
    return f, wshape


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_split_wgrad(case):
    L = pkg_mod("_lib")
    shape, path, kern, dist = case
    n, h, cin, cout, s, tr = shape
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    ho = h * s if tr else h // s
    x = torch.randn(n, h, h, cin, generator=g) if dist == "randn" else torch.rand(n, h, h, cin, generator=g) + 0.5
    dy = torch.randn(n, ho, ho, cout, generator=g)
    f, wshape = _wgrad64(shape)
    dw = torch.full(wshape, float("nan"), device="cuda")
    scratch = torch.empty(8 << 20, device="cuda")
    xd, dyd = x.cuda(), dy.cuda()
    L.check(L.lib().svae_op_wgrad_bf16(L.ptr(xd), n, h, cin, L.ptr(dyd), cout, s, tr, path | 64, L.ptr(dw),
                                       L.ptr(scratch), scratch.numel() * 4, L.stream_ptr()))
    assert L.lib().svae_op_wgrad_last_kernel() == kern
    torch.cuda.synchronize()
    out = dw.cpu().double()
    assert torch.isfinite(out).all()
    ref = f(x.double(), dy.double())
    model = R.plane_products(f, x, dy, 2)
    rel_m, max_m = R.rel_l2(out, model), R.max_rel(out, model)
    rel_k, rel_s = R.rel_l2(out, ref), R.rel_l2(model, ref)
    print("split wgrad %s: vs plane model rel %.2e max %.2e; vs float64 kernel %.2e (max %.2e), model %.2e (max %.2e)"
          % (_id(case), rel_m, max_m, rel_k, R.max_rel(out, ref), rel_s, R.max_rel(model, ref)))
    assert rel_m <= 2e-6 and max_m <= 2e-5, (rel_m, max_m)
    assert rel_k <= 2.0 * rel_s, (rel_k, rel_s)


def test_split_bit_excludes_storage_bits():
    L = pkg_mod("_lib")
    t = torch.zeros(2 * 8 * 8 * 32, device="cuda")
    dw = torch.zeros(16 * 32 * 32, device="cuda")
    for bits in (16, 32, 48):
        rc = L.lib().svae_op_wgrad_bf16(L.ptr(t), 2, 8, 32, L.ptr(t), 32, 1, 0, 2 | 64 | bits, L.ptr(dw), L.ptr(t),
                                        t.numel() * 4, L.stream_ptr())
        assert rc == -2  # SVAE_EBADARG
