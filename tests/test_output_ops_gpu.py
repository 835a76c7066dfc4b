"""The output tail of a chain step, kernel by kernel: pack_out + the output conv-T in its three modes (fp32 small-N
gather, bf16, split: svae_op_output_convt), the small-N gather's dual-pointer form and accumulate = 1
(svae_op_gconv_smalln), its lp<4,8,16> instances (through svae_op_conv_dgrad), output_fwd + loss_reduce
(svae_op_output_fwd) and output_bwd + colsum_small (svae_op_output_bwd), against the float64 restatements of tests/output_ref.py
(held to the oracle by tests/test_output_ref.py), at the smallest shapes that reach every kernel instance, both code
paths (the 16-byte rows of C = 3 and the scalar rows), every tail and the second grid-stride pass.

Every case asserts the reported kernel, keeps sentinels around every buffer the op may write (and inside the ones it
must leave alone), runs twice (bitwise equal) and prints the kernel's error beside the float32 twin's on the scale of
the bound.  Bounds: the project's, max|err| <= tol (1 + max|ref|), tol 2e-5 per element and 5e-5 for sums over pixels
or batch (db, rec_img, stats); tests/test_output_ref.py shows that the float32 twin stays inside them on these inputs
and that a dropped ratio term does not.  Measured worst cases ("Output tail and chain kernels per kernel"):
a_out 1.8e-7, xhat 1.9e-7, rec_img 7.5e-8, stats 5.8e-8, da 2.2e-7, dxprev 1.0e-7, db_out 8.5e-7, db_ratio 5.4e-7;
the float32 twin's: 3.1e-7, 1.6e-7, 7.9e-7, 6.4e-7, 2.1e-7, 9.0e-8, 7.9e-6, 5.5e-6."""
import ctypes

import numpy as np
import pytest
import torch

import output_ref as R
from conftest import pkg_mod
from oracle import torch_twin as TT

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32


def _lib():
    return pkg_mod("_lib")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _variant():
    return (ctypes.c_int32 * 2)(-1, -1)


def _cid(c):
    return "-".join(str(int(v)) if float(v).is_integer() else str(v) for v in c)


# ------------------------------------------------------------------------------------------------ output conv-T
@pytest.mark.parametrize("case", R.CONVT_CASES, ids=_cid)
def test_output_convt(case):
    f1, c, hs, n, ratio = case
    L = _lib()
    x, w_out, w_ratio, b_out, b_ratio = R.convt_inputs(case)
    ref = R.output_convt(x, w_out, w_ratio, b_out, b_ratio, F64)
    twin = R.output_convt(x, w_out, w_ratio, b_out, b_ratio, F32)
    d = [_dev(v) for v in (x, w_out, w_ratio, b_out, b_ratio)]

    def run():
        g = R.Guarded()
        wpack = g.new("wpack", (16 * (c + 1) * f1 + 4,))
        a_out = g.new("a_out", (n, 2 * hs, 2 * hs, c + 1))
        var = _variant()
        L.check(L.lib().svae_op_output_convt(L.ptr(d[0]), n, hs, f1, L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]),
                                             c, 0, L.ptr(wpack), None, L.ptr(a_out), None, 0, var, L.stream_ptr()))
        torch.cuda.synchronize()
        return g, tuple(var)

    g, var = run()
    assert var == R.CONVT_VARIANT[f1]
    assert g.intact()
    assert np.array_equal(g.view["wpack"].cpu().numpy(), R.pack_out(w_out, w_ratio, b_out, b_ratio))  # pack_out: copies
    R.report("a_out", g.get("a_out"), ref, twin, R.FWD_TOL)
    if not ratio:  # no ratio layer: the column is exactly the packed zero bias
        assert not g.get("a_out")[..., c].any()
    g2, _ = run()
    assert R.same_bits(g.snapshot(), g2.snapshot())


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).double().numpy()


@pytest.mark.parametrize("case", R.CONVT_MODE_CASES, ids=_cid)
def test_output_convt_bf16_and_split(case):
    """Modes 1 (bf16) and 2 (split) through the engine's gemm() branch with the packed bias epilogue.  Mode 1 is held to
    the bound of tests/test_gather_bf16_gpu.py against the float64 conv-T of the bf16-rounded operands (2e-5 in L2,
    1e-4 of max|ref| pointwise); mode 2 carries 24 mantissa bits per operand (three bf16 planes), so it is held to the
    fp32 bound against the unrounded reference, like mode 0."""
    mode, f1, c, hs, n = case
    L = _lib()
    x, w_out, w_ratio, b_out, b_ratio = R.convt_inputs((f1, c, hs, n, True))
    ref = R.output_convt(x, w_out, w_ratio, b_out, b_ratio, F64)
    twin = R.output_convt(x, w_out, w_ratio, b_out, b_ratio, F32)
    d = [_dev(v) for v in (x, w_out, w_ratio, b_out, b_ratio)]
    nw = 16 * (c + 1) * f1
    planes = 3 if mode == 2 else 1
    scratch = torch.empty(2 << 20, device="cuda")

    def run():
        g = R.Guarded()
        wpack = g.new("wpack", (nw + 4,))
        wpack_h = g.new("wpack_h", (planes * nw,), dtype=torch.bfloat16)
        a_out = g.new("a_out", (n, 2 * hs, 2 * hs, c + 1))
        var = _variant()
        L.check(L.lib().svae_op_output_convt(L.ptr(d[0]), n, hs, f1, L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]),
                                             c, mode, L.ptr(wpack), L.ptr(wpack_h), L.ptr(a_out), L.ptr(scratch),
                                             scratch.numel() * 4, var, L.stream_ptr()))
        torch.cuda.synchronize()
        return g, tuple(var)

    g, var = run()
    print("VARIANT %s -> %s (%s)" % (case, var, L.lib().svae_kernel_name(var[0]).decode() if var[0] < 100 else "own"))
    assert g.intact()
    packed = R.pack_out(w_out, w_ratio, b_out, b_ratio)
    assert np.array_equal(g.view["wpack"].cpu().numpy(), packed)
    # the bf16 planes: plane q = bf16(w - the earlier planes), round to nearest even
    rest, hp = torch.from_numpy(packed[:nw].copy()), g.view["wpack_h"].cpu().view(planes, nw)
    for q in range(planes):
        b = rest.to(torch.bfloat16)
        assert torch.equal(hp[q].view(torch.int16), b.view(torch.int16)), "plane %d" % q
        rest = rest - b.float()
    got = g.get("a_out")
    if mode == 1:
        rb = R.output_convt(_bf(x), _bf(w_out), _bf(w_ratio), b_out, b_ratio, F64)
        rel = float(np.linalg.norm(got - rb) / np.linalg.norm(rb))
        mx = float(np.abs(got - rb).max() / np.abs(rb).max())
        print("ERR a_out(bf16)      kernel L2 %.3e max %.3e   (bounds 2e-05, 1e-04)" % (rel, mx))
        assert rel <= 2e-5 and mx <= 1e-4, (rel, mx)
    else:
        R.report("a_out(split)", got, ref, twin, R.FWD_TOL)
    assert var == (R.CONVT_MODE_VARIANT[(mode, f1, hs)], 0)
    g2, _ = run()
    assert R.same_bits(g.snapshot(), g2.snapshot())


# (k, n0, n1): plain scalar, plain vector, s2t<8>, lp<32>; n1 > 0: the ratio row through the second weight pointer
GCONV_RAW = [(6, 3, 1), (8, 1, 1), (32, 3, 1), (128, 3, 1), (32, 4, 0), (6, 2, 0)]
GCONV_RAW_VARIANT = {6: (0, 0), 8: (0, 0), 32: (2, 8), 128: (1, 32)}


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", GCONV_RAW, ids=_cid)
def test_gconv_smalln_dual_pointer_and_accumulate(case, accumulate):
    """The launcher's W0 / W1 form (two weight tensors and two biases, as before pack_out) and accumulate = 1 (the
    layer-0 input gradients that add into the chain's dx) on the stride-2 conv-T, n = 3 images of 7 x 7."""
    k, n0, n1 = case
    n, hs = 3, 7
    L = _lib()
    rng = np.random.default_rng(700 + k + n0 + 10 * n1)
    sc = 1.5 / np.sqrt(k)
    x = rng.uniform(-1, 1, (n, hs, hs, k)).astype(F32)
    w0, b0 = (rng.uniform(-1, 1, (4, 4, n0, k)) * sc).astype(F32), rng.uniform(-1, 1, n0).astype(F32)
    w1, b1 = ((rng.uniform(-1, 1, (4, 4, n1, k)) * sc).astype(F32), rng.uniform(-1, 1, n1).astype(F32)) if n1 else (None, None)
    c0 = rng.uniform(-1, 1, (n, 2 * hs, 2 * hs, n0 + n1)).astype(F32)
    w = w0 if w1 is None else np.concatenate([w0, w1], axis=2)
    b = b0 if b1 is None else np.concatenate([b0, b1])
    f = lambda dt: R.convt_s2(x, w, dt) + b.astype(dt) + (c0.astype(dt) if accumulate else 0)
    ref, twin = f(F64), f(F32)
    d = [_dev(v) for v in (x, w0, w1, b0, b1)]

    def run():
        g = R.Guarded()
        out = g.new("c", c0.shape, init=c0)
        var = _variant()
        L.check(L.lib().svae_op_gconv_smalln(L.ptr(d[0]), n, hs, hs, k, L.ptr(d[1]), n0, L.ptr(d[2]), n1, L.ptr(d[3]),
                                             L.ptr(d[4]), 1, 2, accumulate, L.ptr(out), var, L.stream_ptr()))
        torch.cuda.synchronize()
        return g, tuple(var)

    g, var = run()
    assert var == GCONV_RAW_VARIANT[k]
    assert g.intact()
    R.report("c(acc%d)" % accumulate, g.get("c"), ref, twin, R.FWD_TOL)
    g2, _ = run()
    assert R.same_bits(g.snapshot(), g2.snapshot())


@pytest.mark.parametrize("case", R.LP_DGRAD_CASES, ids=_cid)
def test_gconv_lp_through_conv_dgrad(case):
    """gconv_smalln_lp_kernel<4,8,16>: no model's layer reaches them (the output layer and every layer-0 input gradient
    are stride 2 and take s2t at these widths); svae_op_conv_dgrad dispatches to them for a stride-1 conv with cin in
    {1, 3}: a conv-T gather of dy [n,h,h,cout] with the conv's own weights [tap][cin][cout].  The instance is read back
    from the launcher's own record of the launch."""
    n, h, cin, cout = case
    L = _lib()
    rng = np.random.default_rng(600 + cin + cout)
    w = (rng.uniform(-1, 1, (4, 4, cin, cout)) * 0.2).astype(F32)
    dy = rng.uniform(-1, 1, (n, h, h, cout)).astype(F32)
    xt = torch.zeros(n, cin, h, h, dtype=torch.float64, requires_grad=True)
    y = TT.conv2d_same(xt, torch.from_numpy(w).double(), 1)
    (y * torch.from_numpy(dy).double().permute(0, 3, 1, 2)).sum().backward()
    ref = xt.grad.permute(0, 2, 3, 1).numpy()
    dyd, wd = _dev(dy), _dev(w)

    def run():
        g = R.Guarded()
        dx = g.new("dx", (n, h, h, cin))
        L.check(L.lib().svae_op_conv_dgrad(L.ptr(dyd), n, h, cin, L.ptr(wd), cout, 1, 0, L.ptr(dx), L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    var = _variant()
    L.check(L.lib().svae_op_gconv_last_kernel(var))
    assert tuple(var) == (1, cout // 4)   # recorded by gconv_smalln when it launched
    assert g.intact()
    twin = R.conv_same_dgrad(dy, w, F32)
    assert R.rel_err(R.conv_same_dgrad(dy, w, F64), ref) <= 1e-12
    R.report("dx(lp%d)" % (cout // 4), g.get("dx"), ref, twin, R.FWD_TOL)
    assert R.same_bits(g.snapshot(), run().snapshot())


# ------------------------------------------------------------------------------------------------ output_fwd / loss_reduce
@pytest.mark.parametrize("case", R.OUT_CASES + R.OUT_BIG_B, ids=_cid)
def test_output_fwd(case):
    c, h, w, b, xp, lo, hi = case
    L = _lib()
    a, xprev, target, kl, _ = R.out_inputs(case)
    f = lambda dt: R.output_fwd(a, xprev, target, kl, lo, hi, R.OUT_MINH, R.OUT_MAXH, dt)
    ref, twin = f(F64), f(F32)
    nblk = -(-h * w // 256)
    ad, xd, td, kd = _dev(a), _dev(xprev), _dev(target), _dev(kl)

    def run():
        g = R.Guarded()
        xhat, part = g.new("xhat", (b, h, w, c)), g.new("rec_part", (b, nblk))
        rec_img, stats = g.new("rec_img", (b,)), g.new("stats", (2,))
        L.check(L.lib().svae_op_output_fwd(L.ptr(ad), b, h, w, c, L.ptr(xd), L.ptr(td), lo, hi, R.OUT_MINH, R.OUT_MAXH,
                                           L.ptr(kd), L.ptr(xhat), L.ptr(part), L.ptr(rec_img), L.ptr(stats),
                                           L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()
    R.report("xhat", g.get("xhat"), ref[0], twin[0], R.FWD_TOL)
    R.report("rec_part", g.get("rec_part").sum(1) / (h * w * c), ref[1], twin[1], R.SUM_TOL)
    R.report("rec_img", g.get("rec_img"), ref[1], twin[1], R.SUM_TOL)
    R.report("stats", g.get("stats"), ref[2], twin[2], R.SUM_TOL)
    assert R.same_bits(g.snapshot(), run().snapshot())


# ------------------------------------------------------------------------------------------------ output_bwd / colsum_small
BWD_CASES = [(case, v) for case in R.OUT_CASES for v in R.OUT_BWD_VARIANTS] + [(case, (1, 0.37)) for case in R.OUT_COLSUM]


@pytest.mark.parametrize("case,variant", BWD_CASES, ids=lambda v: _cid(v))
def test_output_bwd(case, variant):
    c, h, w, b, xp, lo, hi = case
    has_dx, rec_coef = variant
    L = _lib()
    a, xprev, target, kl, dxhat = R.out_inputs(case)
    dxhat = dxhat if has_dx else None
    # the forward's xhat as the kernel receives it: the float64 value rounded to fp32
    xhat = R.output_fwd(a, xprev, target, kl, lo, hi, R.OUT_MINH, R.OUT_MAXH, F64)[0].astype(F32)
    f = lambda dt: R.output_bwd(a, xprev, xhat, target, lo, hi, R.OUT_MINH, R.OUT_MAXH, rec_coef, dxhat, dt)
    ref, twin = f(F64), f(F32)
    ad, xd, hd, td, dd = _dev(a), _dev(xprev), _dev(xhat), _dev(target), _dev(dxhat)
    want_db = c <= 3

    def run():
        g = R.Guarded()
        da, dxprev = g.new("da", (b, h, w, c + 1)), g.new("dxprev", (b, h, w, c))
        db_out = g.new("db_out", (c,)) if want_db else None
        # the ratio-bias gradient: kept with xprev, dropped (NULL) without, as the engine does at step 0
        db_ratio = g.new("db_ratio", (1,)) if (want_db and xp) else None
        scratch = g.new("scratch", (1024,))
        L.check(L.lib().svae_op_output_bwd(L.ptr(ad), b, h, w, c, L.ptr(xd), L.ptr(hd), L.ptr(td), lo, hi, R.OUT_MINH,
                                           R.OUT_MAXH, rec_coef, L.ptr(dd), L.ptr(da), L.ptr(dxprev), L.ptr(db_out),
                                           L.ptr(db_ratio), L.ptr(scratch), 4096, L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()   # with db_ratio NULL this includes the sentinel right behind db_out[c - 1]
    R.report("da", g.get("da"), ref[0], twin[0], R.FWD_TOL)
    if xp:
        R.report("dxprev", g.get("dxprev"), ref[1], twin[1], R.FWD_TOL)
    else:
        assert g.untouched("dxprev")
        assert not g.get("da")[..., c].any()   # the ratio column is exactly zero
    if want_db:
        R.report("db_out", g.get("db_out"), ref[2][:c], twin[2][:c], R.SUM_TOL)
        if xp:
            R.report("db_ratio", g.get("db_ratio"), ref[2][c:], twin[2][c:], R.SUM_TOL)
    assert R.same_bits(g.snapshot(), run().snapshot())
