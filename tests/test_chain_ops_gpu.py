"""Every kernel of csrc/chain.hip through its entry point (svae_op_sd_layer, _sd_layer_bwd, _sd_head_fwd,
_sd_head_bwd, _chain_noise, _imp_seed, _sqdiff_img) against the float64 restatements of tests/output_ref.py (held to
the oracle's stddevs_prediction, the tape's loss terms and autograd by tests/test_output_ref.py).  Shapes: pixel counts
below one block (32), with a live / dead tail inside a block (320, 432), H != W, and 9216 pixels = 36 block partials
(more than the 32 lanes of sd_stat_fin's strided loop; 16 statistic columns at Co = 8, two rounds of its slots).

Every case keeps sentinels around all it may write, runs twice (bitwise equal) and prints the kernel's error beside the
float32 twin's.  Bounds: the project's, max|err| <= tol (1 + max|ref|), tol 2e-5 per element and 5e-5 for sums over
pixels (dbeta, dw, dw5, db5, the NLL partials); tests/test_output_ref.py shows on these inputs that the twin stays
inside and that a shifted tap, pad 2 / 1, a block missing from a BN sum, rotated W5 columns and dead lanes adding
0.5 log 2 pi do not.

The lrelu derivative steps at y = 0, so the backward cases take mean / invstd / beta / pre as free inputs with every
float64 |y| at least 1e-3 (asserted): no element is excluded from any comparison."""
import numpy as np
import pytest
import torch

import output_ref as R
from conftest import pkg_mod

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32


def _lib():
    return pkg_mod("_lib")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cid(c):
    return "-".join(str(int(v)) if float(v).is_integer() else str(v) for v in c)


# ------------------------------------------------------------------------------------------------ stddev layer
@pytest.mark.parametrize("case", R.SD_CASES, ids=_cid)
def test_sd_layer(case):
    ci, co, n, h, w, l0 = case
    L = _lib()
    x, wt, beta = R.sd_inputs(case)
    ref, twin = R.sd_layer(x, l0, wt, beta, F64), R.sd_layer(x, l0, wt, beta, F32)
    nblk = -(-n * h * w // 256)
    xd, wd, bd = _dev(x), _dev(wt), _dev(beta)

    def run():
        g = R.Guarded()
        pre, act = g.new("pre", (n, h, w, co)), g.new("act", (n, h, w, co))
        mean, invstd = g.new("mean", (co,)), g.new("invstd", (co,))
        scratch = g.new("scratch", (nblk * 2 * co,), dtype=torch.float64)
        L.check(L.lib().svae_op_sd_layer(L.ptr(xd), ci + l0, l0, n, h, w, ci, L.ptr(wd), co, L.ptr(bd), L.ptr(pre),
                                         L.ptr(mean), L.ptr(invstd), L.ptr(act), L.ptr(scratch), nblk * 2 * co * 8,
                                         L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()
    for k, r_, t_ in zip(("pre", "mean", "invstd", "act"), ref, twin):
        R.report(k, g.get(k), r_, t_, R.FWD_TOL)
    assert R.same_bits(g.snapshot(), run().snapshot())


@pytest.mark.parametrize("case", R.SD_CASES, ids=_cid)
def test_sd_layer_bwd(case):
    ci, co, n, h, w, l0 = case
    L = _lib()
    x, wt, beta, mean, invstd, pre, dact, da0 = R.sd_bwd_inputs(case)
    assert np.abs(R.sd_y(pre, mean, invstd, beta)).min() >= R.KINK
    f = lambda dt: R.sd_layer_bwd(dact, pre, mean, invstd, beta, x, l0, wt, l0, da0, dt)
    ref, twin = f(F64), f(F32)
    nblk = -(-n * h * w // 256)
    part_bytes = (nblk * 2 * co * 8 + 15) // 16 * 16
    sbytes = part_bytes + 64 + n * (h // 4) * 16 * ci * co * 4
    d = [_dev(v) for v in (dact, pre, mean, invstd, beta, x, wt)]
    ldd = ci + l0

    def run():
        g = R.Guarded()
        dpre, dbeta, dw = g.new("dpre", (n, h, w, co)), g.new("dbeta", (co,)), g.new("dw", (4, 4, ci, co))
        din = g.new("din", (n, h, w, ldd), init=da0)   # layer 0: the non-zero da it accumulates onto
        scratch = g.new("scratch", (sbytes // 4,))
        L.check(L.lib().svae_op_sd_layer_bwd(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), L.ptr(d[5]),
                                             ci + l0, l0, n, h, w, ci, L.ptr(d[6]), co, l0, L.ptr(dpre), L.ptr(dbeta),
                                             L.ptr(dw), L.ptr(din), ldd, L.ptr(scratch), sbytes, L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()
    R.report("dpre", g.get("dpre"), ref[0], twin[0], R.FWD_TOL)
    R.report("dbeta", g.get("dbeta"), ref[1], twin[1], R.SUM_TOL)
    R.report("dw", g.get("dw"), ref[2], twin[2], R.SUM_TOL)
    R.report("din(mode%d)" % l0, g.get("din"), ref[3], twin[3], R.FWD_TOL)
    if l0:  # the ratio column of da is not the stddev network's to touch
        assert np.array_equal(g.view["din"].cpu().numpy()[..., ci], da0[..., ci])
    assert R.same_bits(g.snapshot(), run().snapshot())


# ------------------------------------------------------------------------------------------------ stddev head
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=_cid)
def test_sd_head_fwd(case):
    ci, c, n, h, w, smax, reg = case
    L = _lib()
    act, w5, b5, mle, target, noise, _ = R.head_inputs(case)
    f = lambda dt: R.sd_head_fwd(act, w5, b5, smax, mle, target, noise, reg, dt)
    ref, twin = f(F64), f(F32)
    nblk = -(-h * w // 256)
    d = [_dev(v) for v in (act, w5, np.array([b5], dtype=F32), mle, target, noise)]

    def run():
        g = R.Guarded()
        sd, sample, part = g.new("sd", (n, h, w)), g.new("sample", (n, h, w, c)), g.new("rec_part", (n, nblk))
        L.check(L.lib().svae_op_sd_head_fwd(L.ptr(d[0]), ci, L.ptr(d[1]), L.ptr(d[2]), smax, L.ptr(d[3]), L.ptr(d[4]),
                                            L.ptr(d[5]), reg, n, h, w, c, L.ptr(sd), L.ptr(sample), L.ptr(part),
                                            L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()
    R.report("sd", g.get("sd"), ref[0], twin[0], R.FWD_TOL)
    R.report("sample", g.get("sample"), ref[1], twin[1], R.FWD_TOL)
    R.report("nll_img", g.get("rec_part").sum(1), ref[2], twin[2], R.SUM_TOL)
    assert R.same_bits(g.snapshot(), run().snapshot())


@pytest.mark.parametrize("with_dsample", [0, 1])
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=_cid)
def test_sd_head_bwd(case, with_dsample):
    ci, c, n, h, w, smax, reg = case
    L = _lib()
    act, w5, b5, mle, target, noise, dsample = R.head_inputs(case)
    dsample = dsample if with_dsample else None
    f = lambda dt: R.sd_head_bwd(act, w5, b5, smax, mle, target, noise, reg, R.HEAD_NLL_COEF, dsample, dt)
    ref, twin = f(F64), f(F32)
    nblk = -(-n * h * w // 256)
    d = [_dev(v) for v in (act, w5, np.array([b5], dtype=F32), mle, target, noise, dsample)]

    def run():
        g = R.Guarded()
        dmle, dact = g.new("dmle", (n, h, w, c)), g.new("dact", (n, h, w, ci))
        dw5, db5 = g.new("dw5", (ci,)), g.new("db5", (1,))
        scratch = g.new("scratch", (nblk * (ci + 1),))
        L.check(L.lib().svae_op_sd_head_bwd(L.ptr(d[0]), ci, L.ptr(d[1]), L.ptr(d[2]), smax, L.ptr(d[3]), L.ptr(d[4]),
                                            L.ptr(d[5]), reg, R.HEAD_NLL_COEF, L.ptr(d[6]), n, h, w, c, L.ptr(dmle),
                                            L.ptr(dact), L.ptr(dw5), L.ptr(db5), L.ptr(scratch), nblk * (ci + 1) * 4,
                                            L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()
    for k, r_, t_, tol in zip(("dmle", "dact", "dw5", "db5"), ref, twin, (R.FWD_TOL, R.FWD_TOL, R.SUM_TOL, R.SUM_TOL)):
        R.report(k, g.get(k), r_, t_, tol)
    assert R.same_bits(g.snapshot(), run().snapshot())


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("n", R.SMALL_N)
def test_chain_noise(n):
    L = _lib()
    rng = np.random.default_rng(n)
    mle, noise = rng.uniform(-1, 1, n).astype(F32), rng.standard_normal(n).astype(F32)
    md, nd = _dev(mle), _dev(noise)
    g = R.Guarded()
    out = g.new("sample", (n,))
    L.check(L.lib().svae_op_chain_noise(L.ptr(md), L.ptr(nd), 0.35, n, L.ptr(out), L.stream_ptr()))
    torch.cuda.synchronize()
    assert g.intact()
    R.report("chain_noise", g.get("sample"), R.chain_noise(mle, noise, 0.35, F64), R.chain_noise(mle, noise, 0.35, F32),
             R.FWD_TOL)
    g2 = R.Guarded()
    out2 = g2.new("sample", (n,))
    L.check(L.lib().svae_op_chain_noise(L.ptr(md), L.ptr(nd), 0.35, n, L.ptr(out2), L.stream_ptr()))
    torch.cuda.synchronize()
    assert R.same_bits(g.snapshot(), g2.snapshot())


@pytest.mark.parametrize("n", R.SMALL_N)
@pytest.mark.parametrize("mask", range(9))
def test_imp_seed(n, mask):
    """mask bits: dxin, xp, xn present; mask 8: all three, in place (out == dxin) as engine.cpp calls it."""
    L = _lib()
    inplace = mask == 8
    bits = 7 if inplace else mask
    rng = np.random.default_rng(100 + n)
    dxin, xp, x, xn = (rng.uniform(-1, 1, n).astype(F32) for _ in range(4))
    dxin, xp, xn = (dxin if bits & 1 else None), (xp if bits & 2 else None), (xn if bits & 4 else None)
    ref, twin = R.imp_seed(dxin, xp, x, xn, -0.21, F64), R.imp_seed(dxin, xp, x, xn, -0.21, F32)
    pd, xd, nd = _dev(xp), _dev(x), _dev(xn)

    def run():
        g = R.Guarded()
        out = g.new("out", (n,), init=dxin if inplace else None)
        din = out if inplace else _dev(dxin)
        L.check(L.lib().svae_op_imp_seed(L.ptr(din), L.ptr(pd), L.ptr(xd), L.ptr(nd), -0.21, n, L.ptr(out),
                                         L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()
    R.report("imp_seed", g.get("out"), np.broadcast_to(ref, (n,)), np.broadcast_to(twin, (n,)), R.FWD_TOL)
    assert R.same_bits(g.snapshot(), run().snapshot())


@pytest.mark.parametrize("per_img,b", R.SQDIFF_CASES)
def test_sqdiff_img(per_img, b):
    L = _lib()
    rng = np.random.default_rng(per_img + b)
    x, y = rng.uniform(-1, 1, (b, per_img)).astype(F32), rng.uniform(-1, 1, (b, per_img)).astype(F32)
    xd, yd = _dev(x), _dev(y)

    def run():
        g = R.Guarded()
        out = g.new("out", (b,))
        L.check(L.lib().svae_op_sqdiff_img(L.ptr(xd), L.ptr(yd), b, per_img, L.ptr(out), L.stream_ptr()))
        torch.cuda.synchronize()
        return g

    g = run()
    assert g.intact()
    R.report("sqdiff_img", g.get("out"), R.sqdiff_img(x, y, F64), R.sqdiff_img(x, y, F32), R.SUM_TOL)
    assert R.same_bits(g.snapshot(), run().snapshot())
