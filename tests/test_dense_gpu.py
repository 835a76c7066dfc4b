"""The FC GEMMs of the bf16 and split modes, kernel by kernel: svae_op_dense_bf16 (csrc/dense_kw.hip in its
three forms -- plain bf16, NS = 3 bf16 planes, NS = 2 scaled fp16 planes with the per-wave running exponent
-- with and without grid split-K through splitk_reduce_kernel, and the tiled per-tap kernel a dense launch
falls to) and svae_op_fc_wgrad (the FC weight gradient: the fp32 weight-GEMM, the tap-merged bf16 kernel and
its NSP = 3 split form).  One entry covers the FC forward and the FC input gradient: the same launch at
shapes (b, k, nout) = (batch, in, out) and (batch, out, in).

References, never another kernel:
  bf16 mode    float64 of the same bf16-rounded operands; test_gather_bf16_gpu.py's bound 2e-5 relative L2,
               1e-4 of max|ref| pointwise.  A bf16-tensor x (+ 64) equals the fp32 call on the rounded
               values bit for bit (opload.h).
  split modes  float64 of the unrounded operands; the fp32 bound of test_split_gather_gpu.py, 2e-6 relative
               L2 and 2e-5 of max|ref| pointwise (tests/split_ref.py: six bf16 products about 6e-9 off
               float64, the fp16 pair about 7e-8, fp32 accumulation about 3e-7).
  fc_wgrad     mode 0 test_ops_gpu.py's 5e-5, mode 1 the bf16 bound, mode 2 the fp32 bound.
Every case asserts the kernel the library reports.  Measured: profiles/split_wgrad_dense_parity.txt."""
import ctypes

import pytest
import torch

import split_ref as R
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

TILED, KW, KW_SPLITK = 0, 1, 2  # include/svae_hip.h SVAE_DENSE_*
EBADARG = -2

# (b, k, nout): variant in bf16 mode with scratch, in the split modes with scratch (None: SVAE_EBADARG)
SHAPES = [
    ((128, 2048, 384), KW_SPLITK, KW_SPLITK),  # encoder FC: grid split-K
    ((128, 384, 2048), KW_SPLITK, KW_SPLITK),  # an input gradient
    ((4, 256, 64), KW_SPLITK, KW_SPLITK),      # row masking, TN = 2
    ((100, 272, 96), KW_SPLITK, KW_SPLITK),    # b % 32 != 0, 17 K steps, TN = 1
    ((32, 48, 32), TILED, KW),                 # three K steps
    ((128, 40, 96), TILED, None),              # k % 16 != 0
    ((128, 48, 4096), KW, KW),                 # a grid that fills the chip: plain bf16 in one pass
]
IDS = ["b%d_k%d_n%d" % s[0] for s in SHAPES]


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _split_planes(w):
    """csrc/common.h: three bf16 planes, then the scaled fp16 pair at exponent H16_WS (raw 16-bit words)."""
    p = R.planes_bf(w, 3)
    h = R.planes_h16(w, R.H16_WS)
    return torch.stack([q.to(torch.bfloat16) for q in p] +
                       [q.to(torch.float16).view(torch.bfloat16) for q in h]).contiguous()


def _operands(shape, seed):
    b, k, n = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, k, generator=g), torch.randn(n, k, generator=g) * 0.05


def _dense(x, w_dev, shape, path, scratch=True):
    """y, return code and variant of one svae_op_dense_bf16 call (x: a device tensor, fp32 or bf16)."""
    L = pkg_mod("_lib")
    b, k, n = shape
    y = torch.full((b, n), float("nan"), device="cuda")
    sc = torch.empty(4 << 20, device="cuda") if scratch else None
    var = ctypes.c_int32(-1)
    rc = L.lib().svae_op_dense_bf16(L.ptr(x), b, k, L.ptr(w_dev), n, path, L.ptr(y), L.ptr(sc),
                                    sc.numel() * 4 if scratch else 0, ctypes.byref(var), L.stream_ptr())
    torch.cuda.synchronize()
    return y, rc, var.value


def _check(y, ref, tag, rel_tol, max_tol):
    yd = y.cpu().double()
    assert torch.isfinite(yd).all(), tag
    rel, mx = R.rel_l2(yd, ref), R.max_rel(yd, ref)
    print("%s: rel L2 %.2e, max %.2e" % (tag, rel, mx))
    assert rel <= rel_tol and mx <= max_tol, (tag, rel, mx)


@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_dense_bf16_mode(case):
    L = pkg_mod("_lib")
    shape, want, _ = case
    x, w = _operands(shape, 11)
    ref = _bf(x).double() @ _bf(w).double().t()
    wd = w.to(torch.bfloat16).cuda()
    x32, xr32 = x.cuda(), _bf(x).cuda()
    x16 = xr32.to(torch.bfloat16)
    runs = [(2, True, want), (0, True, TILED)]
    if shape == (4, 256, 64):
        runs.append((2, False, TILED))  # no scratch: no grid split, and one block does not fill the chip
    for path, scratch, variant in runs:
        tag = "dense bf16 %s path %d%s" % (shape, path, "" if scratch else " no scratch")
        y, rc, var = _dense(x32, wd, shape, path, scratch)
        L.check(rc)
        assert var == variant, (tag, var)
        _check(y, ref, tag, 2e-5, 1e-4)
        # bf16-tensor x against the fp32 call on the same rounded values
        yr, rc, var_r = _dense(xr32, wd, shape, path, scratch)
        L.check(rc)
        yb, rc, var_b = _dense(x16, wd, shape, path | 64, scratch)
        L.check(rc)
        assert var_b == variant and var_r == variant, (tag, var_b, var_r)
        _check(yb, ref, tag + " +64", 2e-5, 1e-4)
        assert torch.equal(yb, yr), tag


@pytest.mark.parametrize("bits", [16 | 32, 16], ids=["fp16_planes", "bf16_planes"])
@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_dense_split_modes(case, bits):
    L = pkg_mod("_lib")
    shape, _, want = case
    x, w = _operands(shape, 12)
    ref = x.double() @ w.double().t()
    wp = _split_planes(w).cuda()
    xd = x.cuda()
    for scratch in (True, False):
        tag = "dense split %s bits %d%s" % (shape, bits, "" if scratch else " no scratch")
        y, rc, var = _dense(xd, wp, shape, 2 | bits, scratch)
        if want is None:
            assert rc == EBADARG, tag
            continue
        L.check(rc)
        assert var == (want if scratch else KW), (tag, var)
        _check(y, ref, tag, 2e-6, 2e-5)
    # the tiled kernel has no split form, and a bf16-tensor x no planes
    assert _dense(xd, wp, shape, 0 | bits, True)[1] == EBADARG
    assert _dense(xd, wp, shape, 2 | bits | 64, True)[1] == EBADARG


def _range_x(shape, order, seed):
    b, k, n = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, k, generator=g)
    scale = torch.tensor(order).repeat(k // 1024 + 1)[:k // 256]
    return x * scale.repeat_interleave(256)


@pytest.mark.parametrize("order", [(1e-3, 1e3, 0.0, 1.0), (1.0, 0.0, 1e3, 1e-3)], ids=["rising", "falling"])
@pytest.mark.parametrize("shape", [(128, 2048, 384), (4, 1024, 64)], ids=lambda s: "b%d_k%d_n%d" % s)
def test_dense_fp16_planes_ranges(shape, order):
    """Blocks of 256 columns of x along K at magnitudes 1e-3, 1e3, 0, 1 (and in reverse): a wave's K batch
    spans 256 columns, so in one pass (no scratch) its running exponent falls when a later batch raises the
    maximum (the accumulators are rescaled), an all-zero batch leaves it, and small terms follow large ones.
    With scratch the grid split gives every block less than one batch: the exponent is set once per block."""
    L = pkg_mod("_lib")
    x = _range_x(shape, order, 13)
    _, w = _operands(shape, 14)
    ref = x.double() @ w.double().t()
    wp = _split_planes(w).cuda()
    for scratch, variant in ((False, KW), (True, KW_SPLITK)):
        tag = "dense fp16 ranges %s %s%s" % (shape, order, "" if scratch else " no scratch")
        y, rc, var = _dense(x.cuda(), wp, shape, 2 | 16 | 32, scratch)
        L.check(rc)
        assert var == variant, (tag, var)
        model = R.h16_products(lambda p, q: p @ q.t(), x, w)
        print("%s: plane model at the whole tensor's exponent %.2e off float64" % (tag, R.rel_l2(model, ref)))
        _check(y, ref, tag, 2e-6, 2e-5)


def test_dense_fp16_planes_zero_x():
    L = pkg_mod("_lib")
    shape = (4, 1024, 64)
    _, w = _operands(shape, 15)
    wp = _split_planes(w).cuda()
    for scratch in (False, True):
        y, rc, _ = _dense(torch.zeros(shape[0], shape[1], device="cuda"), wp, shape, 2 | 16 | 32, scratch)
        L.check(rc)
        assert torch.equal(y, torch.zeros_like(y))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(128, 2048, 384), (100, 64, 96), (4, 40, 96)], ids=lambda s: "b%d_k%d_n%d" % s)
def test_fc_wgrad(shape, mode):
    L = pkg_mod("_lib")
    b, k, n = shape
    g = torch.Generator().manual_seed(16 + mode)
    x, dy = torch.randn(b, k, generator=g), torch.randn(b, n, generator=g)

    def run(xs, ds, m):
        dw = torch.full((k, n), float("nan"), device="cuda")
        L.check(L.lib().svae_op_fc_wgrad(L.ptr(xs), b, k, L.ptr(ds), n, m, L.ptr(dw), L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.isfinite(dw).all()
        return dw

    xd, dyd = x.cuda(), dy.cuda()
    out = run(xd, dyd, mode)
    tag = "fc_wgrad %s mode %d" % (shape, mode)
    if mode == 0:
        ref = x.double().t() @ dy.double()
        err = float((out.cpu().double() - ref).abs().max())
        print("%s: max abs error %.2e, max|ref| %.2e" % (tag, err, float(ref.abs().max())))
        assert err <= 5e-5 * (1 + float(ref.abs().max())), err
    elif mode == 2:
        _check(out, x.double().t() @ dy.double(), tag, 2e-6, 2e-5)
    else:
        ref = _bf(x).double().t() @ _bf(dy).double()
        _check(out, ref, tag, 2e-5, 1e-4)
        xr, dyr = _bf(x).cuda(), _bf(dy).cuda()
        base = run(xr, dyr, 1)
        for bits in (16, 32, 48):
            o = run(xr.to(torch.bfloat16) if bits & 16 else xr, dyr.to(torch.bfloat16) if bits & 32 else dyr, 1 | bits)
            _check(o, ref, tag + " +%d" % bits, 2e-5, 1e-4)
            assert torch.equal(o, base), bits  # one kernel for every storage: rounded storage changes no bit
    # storage bits belong to the bf16 mode
    if mode != 1:
        dw = torch.zeros(k, n, device="cuda")
        assert L.lib().svae_op_fc_wgrad(L.ptr(xd), b, k, L.ptr(dyd), n, mode | 16, L.ptr(dw), L.stream_ptr()) == EBADARG
