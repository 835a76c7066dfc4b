"""Float64 restatements (numpy, NHWC) of the output tail of a chain step and of the chain-variant kernels: the packed
[C | ratio] output conv-T, output / highway / MSE, the stddev network's layer and head with their backwards, and the
three small kernels.  tests/test_output_ref.py holds them to the oracle (oracle/torch_twin.py, oracle/model.py,
oracle/tape.py) and to autograd; tests/test_output_ops_gpu.py and tests/test_chain_ops_gpu.py compare the HIP kernels
with them.

Every function takes dt: np.float64 is the reference; np.float32 is its twin, the same formula with every operand,
product and sum rounded to fp32 and every sum taken sequentially (np.cumsum), which is the rounding baseline the GPU
tests print beside the kernels' errors.  The keyword arguments named `wrong_*` build the deliberately wrong twins of
tests/test_output_ref.py; nothing else uses them.

The shapes, inputs and bounds of the GPU cases live here as well, so that the CPU test of the bounds and the GPU tests
work on the same numbers."""
import math

import numpy as np

FWD_TOL, SUM_TOL = 2e-5, 5e-5   # tests/test_ops_gpu.py, tests/test_flat_ops_gpu.py: max|err| <= tol (1 + max|ref|)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
EPS = 1e-3
KINK = 1e-3                     # the backward cases keep every |y| of the lrelu input at least this far from 0


def rel_err(got, ref):
    """max|got - ref| / (1 + max|ref|): the scale every bound of these tests is stated on."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / (1.0 + np.abs(ref).max()))


def ssum(a, axis, dt):
    """Sum over one axis: float64 as numpy does it; float32 strictly in order (no pairwise tree)."""
    if dt == np.float64:
        return a.sum(axis=axis)
    return np.take(np.cumsum(a, axis=axis, dtype=dt), -1, axis=axis)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))   # keeps x's dtype


def lrelu(y):
    return np.maximum(np.minimum(y * y.dtype.type(0.1), 0), y)


# ---------------------------------------------------------------------------------------------- convolutions
def conv_same(x, w, dt, wrong_pad_before=1, wrong_tap_shift=0):
    """TF conv2d SAME, 4x4, stride 1 (pad 1 before, 2 after): x [N,H,W,Ci], w [4,4,Ci,Co] -> [N,H,W,Co]."""
    x, w = x.astype(dt), w.astype(dt)
    N, H, W, Ci = x.shape
    pb = wrong_pad_before
    xp = np.pad(x, ((0, 0), (pb, 3 - pb), (pb, 3 - pb), (0, 0)))
    if wrong_tap_shift:
        xp = np.roll(xp, wrong_tap_shift, axis=2)
    y = np.zeros((N, H, W, w.shape[3]), dtype=dt)
    for ky in range(4):
        for kx in range(4):
            for ci in range(Ci):
                y += xp[:, ky:ky + H, kx:kx + W, ci:ci + 1] * w[ky, kx, ci]
    return y


def conv_same_dgrad(dy, w, dt):
    """Adjoint of conv_same in x: dy [N,H,W,Co] -> [N,H,W,Ci]."""
    dy, w = dy.astype(dt), w.astype(dt)
    N, H, W, Co = dy.shape
    dxp = np.zeros((N, H + 3, W + 3, w.shape[2]), dtype=dt)
    for ky in range(4):
        for kx in range(4):
            for co in range(Co):
                dxp[:, ky:ky + H, kx:kx + W, :] += dy[..., co:co + 1] * w[ky, kx, :, co]
    return dxp[:, 1:1 + H, 1:1 + W, :]


def conv_same_wgrad(x, dy, dt, wrong_tap_shift=0):
    """Adjoint of conv_same in w: [4,4,Ci,Co], each element a sum over all pixels."""
    x, dy = x.astype(dt), dy.astype(dt)
    N, H, W, Ci = x.shape
    xp = np.pad(x, ((0, 0), (1, 2), (1, 2), (0, 0)))
    if wrong_tap_shift:
        xp = np.roll(xp, wrong_tap_shift, axis=2)
    dw = np.zeros((4, 4, Ci, dy.shape[3]), dtype=dt)
    d2 = dy.reshape(-1, dy.shape[3])
    for ky in range(4):
        for kx in range(4):
            win = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Ci)
            dw[ky, kx] = ssum(win[:, :, None] * d2[:, None, :], 0, dt)
    return dw


def convt_s2(x, w, dt):
    """TF conv2d_transpose SAME, 4x4, stride 2: x [N,h,h,K], w [4,4,Co,K] -> [N,2h,2h,Co] (the full
    transpose's rows and columns 1 .. 2h)."""
    x, w = x.astype(dt), w.astype(dt)
    N, h, _, K = x.shape
    Co = w.shape[2]
    full = np.zeros((N, 2 * h + 2, 2 * h + 2, Co), dtype=dt)
    for ky in range(4):
        for kx in range(4):
            full[:, ky:ky + 2 * h:2, kx:kx + 2 * h:2, :] += ssum(x[..., None, :] * w[ky, kx], -1, dt)
    return full[:, 1:1 + 2 * h, 1:1 + 2 * h, :]


def pack_out(w_out, w_ratio, b_out, b_ratio):
    """misc.hip pack_out: [tap][C+1][F1] weights (ratio row zero without w_ratio), then [b_out | b_ratio | 0..] (4)."""
    C, F1 = w_out.shape[2], w_out.shape[3]
    wp = np.zeros((16, C + 1, F1), dtype=w_out.dtype)
    wp[:, :C] = w_out.reshape(16, C, F1)
    bias = np.zeros(4, dtype=w_out.dtype)
    bias[:C] = b_out
    if w_ratio is not None:
        wp[:, C] = w_ratio.reshape(16, F1)
        bias[C] = b_ratio[0]
    return np.concatenate([wp.ravel(), bias])


def output_convt(x, w_out, w_ratio, b_out, b_ratio, dt):
    """a_out [N,2h,2h,C+1]: the output conv-T plus bias in columns 0..C-1, the ratio conv-T plus bias in column C
    (exactly the packed zero bias without a ratio layer)."""
    C = w_out.shape[2]
    wr = w_ratio if w_ratio is not None else np.zeros((4, 4, 1, w_out.shape[3]))
    br = b_ratio if b_ratio is not None else np.zeros(1)
    w = np.concatenate([w_out, wr], axis=2)
    return convt_s2(x, w, dt) + np.concatenate([b_out, br]).astype(dt)


# ---------------------------------------------------------------------------------------------- output / highway / MSE
def output_fwd(a, xprev, target, kl_img, lo, hi, minh, maxh, dt, wrong_drop_ratio=False):
    """xhat [B,H,W,C], rec_img [B] (mean squared error per image), stats (mean_b rec_img, mean_b kl_img)."""
    a, target, kl_img = a.astype(dt), target.astype(dt), kl_img.astype(dt)
    lo, hi, minh, maxh = dt(lo), dt(hi), dt(minh), dt(maxh)
    C = a.shape[-1] - 1
    out = (hi - lo) * sigmoid(a[..., :C]) + lo
    if xprev is not None and not wrong_drop_ratio:
        r = minh + (maxh - minh) * sigmoid(a[..., C:])
        xhat = r * out + (1 - r) * xprev.astype(dt)
    else:
        xhat = out
    d = (xhat - target).reshape(a.shape[0], -1)
    rec_img = ssum(d * d, 1, dt) / dt(d.shape[1])
    stats = np.array([ssum(rec_img, 0, dt) / dt(a.shape[0]), ssum(kl_img, 0, dt) / dt(a.shape[0])], dtype=dt)
    return xhat, rec_img, stats


def output_bwd(a, xprev, xhat, target, lo, hi, minh, maxh, rec_coef, dxhat_in, dt):
    """Gradient of sum(dxhat_in * xhat) + rec_coef * sum((xhat - target)^2) in a (da [B,H,W,C+1]) and in xprev
    (dxprev, None without xprev); db [C+1] = column sums of da."""
    a, xhat, target = a.astype(dt), xhat.astype(dt), target.astype(dt)
    lo, hi, minh, maxh, rec_coef = dt(lo), dt(hi), dt(minh), dt(maxh), dt(rec_coef)
    C = a.shape[-1] - 1
    g = rec_coef * 2 * (xhat - target)
    if dxhat_in is not None:
        g = g + dxhat_in.astype(dt)
    o = sigmoid(a[..., :C])
    out = (hi - lo) * o + lo
    da = np.zeros_like(a)
    dxprev = None
    if xprev is not None:
        sr = sigmoid(a[..., C:])
        r = minh + (maxh - minh) * sr
        da[..., :C] = r * g * (hi - lo) * o * (1 - o)
        drr = ssum(g * (out - xprev.astype(dt)), -1, dt)
        da[..., C] = drr * (maxh - minh) * sr[..., 0] * (1 - sr[..., 0])
        dxprev = (1 - r) * g
    else:
        da[..., :C] = g * (hi - lo) * o * (1 - o)
    db = ssum(da.reshape(-1, C + 1), 0, dt)
    return da, dxprev, db


# ---------------------------------------------------------------------------------------------- stddev network
def sd_layer(x, in_sig, w, beta, dt, wrong_skip_block=None, **wrong):
    """conv2d_same + training BN over all pixels (biased variance, eps 1e-3, beta only) + lrelu.  x [N,H,W,ldi]
    (only the first Ci = w.shape[2] columns are read; in_sig: through a sigmoid)."""
    Ci = w.shape[2]
    xin = x[..., :Ci].astype(dt)
    if in_sig:
        xin = sigmoid(xin)
    pre = conv_same(xin, w, dt, **wrong)
    flat = pre.reshape(-1, pre.shape[-1])
    n = dt(flat.shape[0])
    stat = flat
    if wrong_skip_block is not None:
        stat = np.delete(flat, np.s_[256 * wrong_skip_block:256 * (wrong_skip_block + 1)], axis=0)
    mean = ssum(stat, 0, dt) / n
    var = np.maximum(ssum(stat * stat, 0, dt) / n - mean * mean, 0)
    invstd = 1 / np.sqrt(var + dt(EPS))
    act = lrelu((pre - mean) * invstd + beta.astype(dt))
    return pre, mean, invstd, act


def sd_y(pre, mean, invstd, beta):
    """The lrelu input, in float64 (where the backward's step sits)."""
    return (pre.astype(np.float64) - mean) * invstd + beta


def sd_layer_bwd(dact, pre, mean, invstd, beta, x, in_sig, w, mode, da0, dt, wrong_skip_block=None, **wrong):
    """Backward of sd_layer with mean / invstd / beta / pre as given: dpre, dbeta, dw and the input gradient (mode 0:
    din [N,H,W,Ci]; mode 1: da0 (pitch ldi) with din * s (1 - s) added to its first Ci columns, s = sigmoid(x))."""
    dact, pre, mean, invstd, beta = (v.astype(dt) for v in (dact, pre, mean, invstd, beta))
    Ci = w.shape[2]
    xin = x[..., :Ci].astype(dt)
    s = sigmoid(xin) if in_sig else None
    y = (pre - mean) * invstd + beta
    dz = dact * np.where(y > 0, dt(1), dt(0.1))
    xh = (pre - mean) * invstd
    fz, fx = dz.reshape(-1, dz.shape[-1]), (dz * xh).reshape(-1, dz.shape[-1])
    if wrong_skip_block is not None:
        sl = np.s_[256 * wrong_skip_block:256 * (wrong_skip_block + 1)]
        fz, fx = np.delete(fz, sl, axis=0), np.delete(fx, sl, axis=0)
    S, Q = ssum(fz, 0, dt), ssum(fx, 0, dt)
    inv_n = dt(1) / dt(dz.size // dz.shape[-1])
    dpre = invstd * (dz - S * inv_n - xh * (Q * inv_n))
    dw = conv_same_wgrad(s if in_sig else xin, dpre, dt, **wrong)
    din = conv_same_dgrad(dpre, w, dt)
    if mode == 1:
        out = da0.astype(dt).copy()
        out[..., :Ci] += din * s * (1 - s)
        din = out
    return dpre, S, dw, din


def sd_head_fwd(act, w5, b5, smax, mle, target, noise, reg, dt, wrong_dead_lanes=False):
    """sd [B,H,W] = smax sigmoid(act . w5 + b5); sample = mle + reg sd noise; nll_img [B] = the image's SUM over
    pixels and channels of log sd + 0.5 log 2pi + 0.5 ((mle - target) / sd)^2."""
    act, w5, mle, target, noise = (v.astype(dt) for v in (act, w5, mle, target, noise))
    a = ssum(act * w5, -1, dt) + dt(b5)
    sd = dt(smax) * sigmoid(a)
    sample = mle + dt(reg) * sd[..., None] * noise
    d = (mle - target) / sd[..., None]
    e = np.log(sd)[..., None] + dt(HALF_LOG_2PI) + dt(0.5) * d * d
    nll = ssum(e.reshape(e.shape[0], -1), 1, dt)
    if wrong_dead_lanes:  # every idle lane of the image's last block adds one channel's constant
        hw = act.shape[1] * act.shape[2]
        nll = nll + dt((-hw % 256) * HALF_LOG_2PI)
    return sd, sample, nll


def sd_head_bwd(act, w5, b5, smax, mle, target, noise, reg, nll_coef, dsample, dt):
    """Gradient of sum(dsample * sample) + nll_coef * sum(nll_img): dmle, dact, dw5 [Ci], db5."""
    act, w5, mle, target, noise = (v.astype(dt) for v in (act, w5, mle, target, noise))
    smax, reg, nll_coef = dt(smax), dt(reg), dt(nll_coef)
    sg = sigmoid(ssum(act * w5, -1, dt) + dt(b5))
    isd = (1 / (smax * sg))[..., None]
    g = dsample.astype(dt) if dsample is not None else np.zeros_like(mle)
    d = mle - target
    dmle = g + nll_coef * d * isd * isd
    dsd = ssum(reg * noise * g + nll_coef * (isd - d * d * isd * isd * isd), -1, dt)
    da5 = dsd * smax * sg * (1 - sg)
    dact = da5[..., None] * w5
    dw5 = ssum((act * da5[..., None]).reshape(-1, act.shape[-1]), 0, dt)
    db5 = ssum(da5.ravel(), 0, dt)
    return dmle, dact, dw5, db5


# ---------------------------------------------------------------------------------------------- the small kernels
def chain_noise(mle, noise, scale, dt):
    return mle.astype(dt) + dt(scale) * noise.astype(dt)


def imp_seed(dxin, xp, x, xn, coef, dt):
    x = x.astype(dt)
    g = np.zeros_like(x)
    if xp is not None:
        g = g + (x - xp.astype(dt))
    if xn is not None:
        g = g - (xn.astype(dt) - x)
    return (dxin.astype(dt) if dxin is not None else 0) + 2 * dt(coef) * g


def sqdiff_img(a, b, dt):
    d = a.astype(dt) - b.astype(dt)
    return ssum((d * d).reshape(d.shape[0], -1), 1, dt)


# ---------------------------------------------------------------------------------------------- the cases and their inputs
def _u(rng, shape, scale=1.0):
    return (rng.uniform(-1, 1, size=shape) * scale).astype(np.float32)


# output conv-T, mode 0: (f1, c, hs, n, ratio); n = 3 at hs = 7 (588 output pixels: no multiple of 256 / LP)
CONVT_VARIANT = {6: (0, 0), 8: (0, 0), 16: (2, 4), 32: (2, 8), 64: (2, 16), 128: (1, 32), 256: (1, 64)}
CONVT_CASES = [(f1, c, hs, 3 if hs == 7 else 2, True) for f1 in (6, 8, 16, 32, 64, 128, 256) for c in (1, 3)
               for hs in (2, 7, 16)] + [(6, 1, 2, 2, False), (16, 3, 7, 3, False), (128, 3, 2, 2, False)]


def convt_inputs(case):
    f1, c, hs, n, ratio = case
    rng = np.random.default_rng(1000 + f1 * 7 + c * 3 + hs)
    sc = 1.5 / math.sqrt(f1)  # 4 taps x f1 channels per output: pre-activations of a few units
    x = _u(rng, (n, hs, hs, f1))
    w_out, b_out = _u(rng, (4, 4, c, f1), sc), _u(rng, (c,), 0.5)
    w_ratio, b_ratio = (_u(rng, (4, 4, 1, f1), sc), _u(rng, (1,), 0.5)) if ratio else (None, None)
    return x, w_out, w_ratio, b_out, b_ratio


# modes 1 (bf16) and 2 (split): (mode, f1, c, hs, n); hs = 16: the widths the bf16 small-N conv-T takes, hs = 14: MNIST's
CONVT_MODE_CASES = [(m, f1, c, hs, 2) for m in (1, 2) for f1 in (16, 32, 64) for c in (1, 3) for hs in (16, 14)]
# the kernel each runs: 100 = convt_smalln_kernel, 101 = the fp32 gather-GEMM (split mode without a split kernel),
# else the bf16 GEMM instance id of csrc/kernels.h
CONVT_MODE_VARIANT = {(1, 16, 16): 3, (1, 16, 14): 3,     # per-tap igemm_bf16_kernel<256, 32>, scalar gather (f1 % 32)
                      (1, 32, 16): 100, (1, 64, 16): 100,  # convt_smalln_kernel<1>: f1 % 32 == 0 and hs % 16 == 0
                      (1, 32, 14): 2, (1, 64, 14): 2,      # per-tap igemm_bf16_kernel<256, 32>
                      (2, 16, 16): 101, (2, 16, 14): 101, (2, 32, 14): 101, (2, 64, 14): 101,   # no split kernel: fp32
                      (2, 32, 16): 100, (2, 64, 16): 100}  # convt_smalln_kernel<3>

# lp<4,8,16> through svae_op_conv_dgrad: (n, h, cin, cout), stride-1 conv with cin % 4 != 0
LP_DGRAD_CASES = [(3, 5, cin, cout) for cin in (1, 3) for cout in (16, 32, 64)]

OUT_HW = [(4, 4), (12, 12), (28, 28), (8, 20)]
OUT_MINH, OUT_MAXH = 0.1, 0.9
# (c, h, w, b, xprev, lo, hi)
OUT_CASES = [(c, h, w, b, xp, lo, hi) for c in (1, 2, 3, 4) for (h, w) in OUT_HW for b in (1, 5) for xp in (0, 1)
             for (lo, hi) in ((0.0, 1.0), (-1.0, 1.0))]
OUT_BIG_B = [(1, 4, 4, 300, 1, 0.0, 1.0), (1, 28, 28, 300, 0, -1.0, 1.0)]      # loss_reduce past 256 images, nblk 1 | 4
OUT_COLSUM = [(1, 20, 20, 175, 1, 0.0, 1.0), (3, 20, 20, 175, 1, -1.0, 1.0)]    # 70 000 rows: a second grid-stride pass
# backward variants: (dxhat_in given, rec_coef)
OUT_BWD_VARIANTS = [(0, 0.37), (1, 0.0), (1, 0.37), (0, 0.0)]


def out_inputs(case):
    c, h, w, b, xp, lo, hi = case
    rng = np.random.default_rng(2000 + c * 1000 + h * 31 + w * 7 + b)
    a = _u(rng, (b, h, w, c + 1), 6.0)   # the sigmoids leave their linear range
    r = lambda: (lo + (hi - lo) * rng.uniform(0, 1, size=(b, h, w, c))).astype(np.float32)
    xprev, target = (r() if xp else None), r()
    kl_img, dxhat = _u(rng, (b,), 2.0), _u(rng, (b, h, w, c))
    return a, xprev, target, kl_img, dxhat


SD_CH = [(1, 1), (3, 5), (5, 8), (8, 3), (4, 8)]
SD_SHAPES = [(3, 12, 12), (2, 4, 4), (2, 8, 20), (9, 32, 32)]   # the last: 36 blocks of 256 pixels
# (ci, co, n, h, w, layer0): layer0 = the input is sigmoid(a_out) at pitch ci + 1
SD_CASES = [(ci, co, n, h, w, 0) for (ci, co) in SD_CH for (n, h, w) in SD_SHAPES] + \
           [(ci, co, n, h, w, 1) for (ci, co) in SD_CH[:2] for (n, h, w) in SD_SHAPES]


def sd_inputs(case):
    ci, co, n, h, w, l0 = case
    rng = np.random.default_rng(3000 + ci * 100 + co * 10 + n + h + l0)
    x = _u(rng, (n, h, w, ci + l0), 3.0 if l0 else 1.0)
    wt, beta = _u(rng, (4, 4, ci, co), 1.0 / math.sqrt(4 * ci)), _u(rng, (co,), 0.3)
    return x, wt, beta


def sd_bwd_inputs(case):
    """Free mean / invstd / beta / pre; every element whose float64 |y| is below KINK is moved out to 1.5 KINK on its
    own side before anything is computed (1.5: the moved pre is rounded to fp32 again)."""
    ci, co, n, h, w, l0 = case
    x, wt, beta = sd_inputs(case)
    rng = np.random.default_rng(4000 + ci * 100 + co * 10 + n + h + l0)
    mean = _u(rng, (co,), 0.5)
    invstd = rng.uniform(0.5, 2.0, size=(co,)).astype(np.float32)
    pre, dact = _u(rng, (n, h, w, co), 2.0), _u(rng, (n, h, w, co))
    y = sd_y(pre, mean, invstd, beta)
    near = np.abs(y) < KINK
    ynew = np.where(y >= 0, 1.5 * KINK, -1.5 * KINK)
    moved = mean.astype(np.float64) + (ynew - beta) / invstd
    pre = np.where(near, moved, pre).astype(np.float32)
    da0 = _u(rng, (n, h, w, ci + 1)) if l0 else None
    return x, wt, beta, mean, invstd, pre, dact, da0


# (ci, c, n, h, w, smax, reg)
HEAD_CASES = [(ci, c, n, h, w, smax, reg) for ci in (1, 5, 8) for c in (1, 3) for (n, h, w) in SD_SHAPES
              for smax in (0.5, 2.0) for reg in (0.0, 0.7)]
HEAD_NLL_COEF = 0.013


def head_inputs(case):
    """A head pre-activation within +-3 and targets within +-1 of the MLE: 1 / sd^3 stays below about 10^3."""
    ci, c, n, h, w, smax, reg = case
    rng = np.random.default_rng(5000 + ci * 100 + c * 10 + n + h + int(smax * 2))
    act = _u(rng, (n, h, w, ci))
    w5, b5 = _u(rng, (ci,), 2.5 / ci), float(_u(rng, (1,), 0.5)[0])
    mle = _u(rng, (n, h, w, c))
    target = (mle + _u(rng, (n, h, w, c))).astype(np.float32)
    noise, dsample = rng.standard_normal((n, h, w, c)).astype(np.float32), _u(rng, (n, h, w, c))
    return act, w5, b5, mle, target, noise, dsample


SMALL_N = [1, 255, 257, 4099]
SQDIFF_CASES = [(per, b) for per in (7, 256, 2352) for b in (1, 5)]


# ---------------------------------------------------------------------------------------------- GPU-test helpers
SENT = 777.0
PAD = 64   # floats of sentinel on either side of a buffer (256 bytes: the buffer keeps a 16-byte alignment)


class Guarded:
    """Device buffers inside sentinels: new(name, shape[, init]) gives the view a kernel writes; intact() is true while
    every sentinel stands; untouched(name) while the buffer itself is all sentinel; snapshot() is everything, for the
    bitwise comparison of two runs."""

    def __init__(self):
        import torch
        self.torch, self.full, self.view = torch, {}, {}

    def new(self, name, shape, init=None, dtype=None):
        t = self.torch
        n = int(np.prod(shape))
        full = t.full((n + 2 * PAD,), SENT, device="cuda", dtype=dtype or t.float32)
        v = full[PAD:PAD + n].view(*shape)
        if init is not None:
            v.copy_(t.from_numpy(np.ascontiguousarray(init)))
        assert v.data_ptr() % 16 == 0
        self.full[name], self.view[name] = full, v
        return v

    def intact(self):
        return all(bool((f[:PAD] == SENT).all()) and bool((f[-PAD:] == SENT).all()) for f in self.full.values())

    def untouched(self, name):
        return bool((self.full[name] == SENT).all())

    def get(self, name):
        return self.view[name].double().cpu().numpy()

    def snapshot(self):
        return {k: f.clone() for k, f in self.full.items()}


def same_bits(a, b):
    import torch
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def report(name, got, ref, twin, tol):
    """Print the kernel's and the float32 twin's error on the bound's scale, then hold the kernel to the bound."""
    e, t = rel_err(got, ref), rel_err(twin, ref)
    print("ERR %-16s kernel %.3e   twin %.3e   (bound %.0e)" % (name, e, t, tol))
    assert e <= tol, (name, e, tol)
