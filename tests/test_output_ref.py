"""tests/output_ref.py without a GPU.  (1) Its float64 restatements equal the oracle's own operations to 1e-12:
oracle/model.py's generator_ladder output expression and stddevs_prediction on a `tiny` predicted-stddev
configuration, oracle/torch_twin.py's conv2d_t_same / conv2d_same / bn_train / lrelu / Twin.stddevs, and
oracle/tape.py's loss terms; the hand-written backward expressions equal autograd.  (2) The bounds of the GPU tests
(tests/test_output_ops_gpu.py, tests/test_chain_ops_gpu.py) discriminate: on the GPU cases' own inputs the float32
twin stays inside each bound and the deliberately wrong float32 twins leave it."""
import numpy as np
import pytest
import torch

import output_ref as R
from oracle import model, spec
from oracle import tape as T
from oracle import torch_twin as TT

F64, F32 = np.float64, np.float32
TIGHT = 1e-12


def _eq(got, ref, tol=TIGHT):
    assert R.rel_err(got, ref) <= tol, R.rel_err(got, ref)


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F64)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).detach().numpy()


# ------------------------------------------------------------------------------------------------ (1) the oracle
@pytest.fixture(scope="module")
def tiny_pgn():
    """Step 1 (the first with a ratio layer) of `tiny` with predicted stddevs, through the oracle's own generator."""
    cfg = spec.make_config("tiny", add_noise_to_chain=True, predict_generator_noise=True)
    _, struct, params = spec.init_params(cfg, seed=3)
    rng = np.random.default_rng(11)
    B, H, W, C = 4, cfg["H"], cfg["W"], cfg["C"]
    lo, hi = cfg["range"]
    tp = T.Tape()
    P = {k: tp.leaf(v) for k, v in params.items()}
    st = struct[1]
    xprev = tp.leaf(rng.uniform(lo, hi, size=(B, H, W, C)))
    z = tp.leaf(rng.standard_normal((B, cfg["latent_dim"])))
    rec = {}
    xhat = model.generator_ladder(tp, P, cfg, st["generator"], xprev, z, st.get("encoder"), rec)
    sd = model.stddevs_prediction(tp, P, cfg, st["generator"]["stddev"], rec["conv_output"])
    return dict(cfg=cfg, st=st, params=params, xprev=xprev.v, z=z.v, struct=struct, s1=rec["s1_act_0"].v, conv_output=rec["conv_output"].v,
                xhat=xhat.v, sd=sd.v, rng=rng)


def _a_out(t):
    g, p = t["st"]["generator"], t["params"]
    return R.output_convt(t["s1"], p[g["out"]["w"]], p[g["ratio"]["w"]], p[g["out"]["b"]], p[g["ratio"]["b"]], F64)


def test_output_tail_is_the_oracles_generator_output(tiny_pgn):
    t, cfg = tiny_pgn, tiny_pgn["cfg"]
    a = _a_out(t)
    C = cfg["C"]
    _eq(R.sigmoid(a[..., :C]), t["conv_output"])
    lo, hi = cfg["range"]
    target = t["rng"].uniform(lo, hi, size=t["xhat"].shape)
    kl = t["rng"].uniform(0, 2, size=a.shape[0])
    xhat, rec_img, stats = R.output_fwd(a, t["xprev"], target, kl, lo, hi, cfg["min_highway"], cfg["max_highway"], F64)
    _eq(xhat, t["xhat"])
    tp = T.Tape()
    rec = T.mean_sq_err_per_row(tp, tp.leaf(t["xhat"]), target)
    _eq(rec_img, rec.v)
    _eq(stats, [T.mean_all(tp, rec).v, kl.mean()])
    # without xprev: the first step's expression
    x0, _, _ = R.output_fwd(a, None, target, kl, lo, hi, 0.1, 0.9, F64)
    _eq(x0, (hi - lo) * t["conv_output"] + lo)


def test_output_tail_is_the_torch_twins_generator_output(tiny_pgn):
    """The same step through oracle/torch_twin.py's Twin.generator: its conv_output and its output expression."""
    t, cfg = tiny_pgn, tiny_pgn["cfg"]
    tw = TT.Twin(cfg, t["struct"], t["params"], dtype=torch.float64, requires_grad=False)
    out = tw.generator(t["st"]["generator"], _nchw(t["xprev"]), torch.from_numpy(t["z"]), t["st"].get("encoder"))
    a = _a_out(t)
    _eq(R.sigmoid(a[..., :cfg["C"]]), _nhwc(tw._conv_output))
    lo, hi = cfg["range"]
    xhat, _, _ = R.output_fwd(a, t["xprev"], t["xhat"], np.zeros(a.shape[0]), lo, hi, cfg["min_highway"],
                              cfg["max_highway"], F64)
    _eq(xhat, _nhwc(out))


def test_stddev_network_is_the_oracles_stddevs_prediction(tiny_pgn):
    t, cfg = tiny_pgn, tiny_pgn["cfg"]
    sst, p = t["st"]["generator"]["stddev"], t["params"]
    cur, in_sig = _a_out(t), 1     # layer 0 reads sigmoid(a_out) at pitch C + 1
    for lay in sst["convs"]:       # (the conv bias the oracle adds cancels in the BN: the engine has none)
        _, _, _, cur = R.sd_layer(cur, in_sig, p[lay["w"]], p[lay["beta"]], F64)
        in_sig = 0
    smax = cfg["predict_generator_stddev_max"]
    w5, b5 = p[sst["out"]["w"]].reshape(-1), float(p[sst["out"]["b"]][0])
    B, H, W, C = t["xhat"].shape
    target, noise = t["rng"].uniform(-1, 1, size=(B, H, W, C)), t["rng"].standard_normal((B, H, W, C))
    sd, sample, nll = R.sd_head_fwd(cur, w5, b5, smax, t["xhat"], target, noise, 0.7, F64)
    _eq(sd, t["sd"][..., 0])
    # the torch twin's restatement of the same network
    tw = TT.Twin(cfg, None, p, dtype=torch.float64, requires_grad=False)
    _eq(sd, _nhwc(tw.stddevs(sst, _nchw(t["conv_output"])))[..., 0])
    # oracle/tape.py: the noisy sample and the Gaussian NLL (its per-image MEAN; the kernels carry the sum)
    tp = T.Tape()
    xh, sdn = tp.leaf(t["xhat"]), tp.leaf(t["sd"])
    _eq(sample, T.add_scaled_noise(tp, xh, sdn, noise, 0.7).v)
    _eq(nll / (H * W * C), T.nll_per_row(tp, xh, target, sdn).v)


def test_tape_backward_of_the_head_terms():
    """d / d mle and d / d sd of the tape's add_scaled_noise + nll_per_row are the head backward's two inner terms."""
    case = (5, 3, 3, 12, 12, 2.0, 0.7)
    act, w5, b5, mle, target, noise, dsample = (np.asarray(v, dtype=F64) for v in R.head_inputs(case))
    sd, _, _ = R.sd_head_fwd(act, w5, b5, 2.0, mle, target, noise, 0.7, F64)
    tp = T.Tape()
    xh, sdn = tp.leaf(mle), tp.leaf(sd[..., None])
    sample = T.add_scaled_noise(tp, xh, sdn, noise, 0.7)
    nll = T.nll_per_row(tp, xh, target, sdn)
    m = mle[0].size
    loss = T.scalar_sum(tp, [T.mean_all(tp, nll), T.mean_all(tp, T.mul(tp, sample, tp.leaf(dsample)))],
                        [R.HEAD_NLL_COEF * m * mle.shape[0], float(mle.size)])
    tp.backward(loss)
    dmle, dact, _, _ = R.sd_head_bwd(act, w5, b5, 2.0, mle, target, noise, 0.7, R.HEAD_NLL_COEF, dsample, F64)
    _eq(dmle, xh.g)
    sg = sd / 2.0
    _eq(dact, (sdn.g[..., 0] * 2.0 * sg * (1 - sg))[..., None] * w5)


@pytest.mark.parametrize("case", [(6, 1, 2, 2, True), (16, 3, 7, 3, True), (16, 3, 7, 3, False)])
def test_convt_is_the_oracles_conv2d_transpose(case):
    x, w_out, w_ratio, b_out, b_ratio = R.convt_inputs(case)
    a = R.output_convt(x, w_out, w_ratio, b_out, b_ratio, F64)
    C = w_out.shape[2]
    _eq(a[..., :C], _nhwc(TT.conv2d_t_same(_nchw(x), torch.from_numpy(w_out).double(), 2)) + b_out.astype(F64))
    if w_ratio is None:
        assert np.array_equal(a[..., C], np.zeros_like(a[..., C]))
        assert np.array_equal(R.pack_out(w_out, None, b_out, None).reshape(-1)[-4 + C:], np.zeros(4 - C, dtype=F32))
    else:
        _eq(a[..., C:], _nhwc(TT.conv2d_t_same(_nchw(x), torch.from_numpy(w_ratio).double(), 2)) + float(b_ratio[0]))
    # the packed table the gather reads: [tap][C + 1][F1]
    wp = R.pack_out(w_out, w_ratio, b_out, b_ratio)[:-4].reshape(4, 4, C + 1, -1)
    _eq(R.convt_s2(x, wp, F64) + R.pack_out(w_out, w_ratio, b_out, b_ratio)[-4:][:C + 1], a)


def test_small_kernels_are_the_tapes_terms():
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-1, 1, (5, 4, 4, 3)), rng.uniform(-1, 1, (5, 4, 4, 3))
    tp = T.Tape()
    an, bn = tp.leaf(a), tp.leaf(b)
    sq = T.sq_norm_diff_per_row(tp, an, bn)
    _eq(R.sqdiff_img(a, b, F64), sq.v)
    _eq(R.chain_noise(a, b, 0.3, F64), T.add_scaled_noise(tp, an, 0.6, b, 0.5).v)
    # imp_seed: the gradient in x_t of coef * (||x_t - x_{t-1}||^2 + ||x_{t+1} - x_t||^2), plus dxin
    x, xp, xn, dxin = (rng.uniform(-1, 1, (2, 3, 3, 1)) for _ in range(4))
    tp = T.Tape()
    xl = tp.leaf(x)
    terms = [T.mean_all(tp, T.sq_norm_diff_per_row(tp, xl, tp.leaf(xp))),
             T.mean_all(tp, T.sq_norm_diff_per_row(tp, tp.leaf(xn), xl))]
    tp.backward(T.scalar_sum(tp, terms, [0.25 * 2, 0.25 * 2]))   # mean over 2 images: coef = 0.25
    _eq(R.imp_seed(dxin, xp, x, xn, 0.25, F64), dxin + xl.g)
    _eq(R.imp_seed(None, None, x, xn, 0.25, F64), -2 * 0.25 * (xn - x))
    _eq(R.imp_seed(None, xp, x, None, 0.25, F64), 2 * 0.25 * (x - xp))
    assert np.array_equal(R.imp_seed(dxin, None, x, None, 0.25, F64), dxin)


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("case", [(3, 12, 12, 5, 1, -1.0, 1.0), (1, 8, 20, 1, 1, 0.0, 1.0), (4, 4, 4, 5, 0, 0.0, 1.0)])
def test_output_bwd_is_autograd(case):
    a, xprev, target, kl, dxhat = R.out_inputs(case)
    c, lo, hi = case[0], case[5], case[6]
    at = torch.from_numpy(a).double().requires_grad_(True)
    xt = torch.from_numpy(xprev).double().requires_grad_(True) if xprev is not None else None
    out = (hi - lo) * torch.sigmoid(at[..., :c]) + lo
    if xt is not None:
        r = R.OUT_MINH + (R.OUT_MAXH - R.OUT_MINH) * torch.sigmoid(at[..., c:])
        out = r * out + (1 - r) * xt
    xhat, _, _ = R.output_fwd(a, xprev, target, kl, lo, hi, R.OUT_MINH, R.OUT_MAXH, F64)
    _eq(xhat, out.detach().numpy())
    tg = torch.from_numpy(target).double()
    ((out * torch.from_numpy(dxhat).double()).sum() + 0.37 * ((out - tg) ** 2).sum()).backward()
    da, dxprev, db = R.output_bwd(a, xprev, xhat, target, lo, hi, R.OUT_MINH, R.OUT_MAXH, 0.37, dxhat, F64)
    if xt is None:
        assert dxprev is None and not da[..., c].any()
        _eq(da[..., :c], at.grad.numpy()[..., :c])
    else:
        _eq(da, at.grad.numpy())
        _eq(dxprev, xt.grad.numpy())
    _eq(db, at.grad.numpy().reshape(-1, c + 1).sum(0))


@pytest.mark.parametrize("case", [(3, 5, 3, 12, 12, 0), (3, 5, 2, 8, 20, 1), (8, 3, 2, 4, 4, 0)])
def test_sd_layer_and_its_backward_are_the_oracles_ops_under_autograd(case):
    ci, co, n, h, w, l0 = case
    x, wt, beta = R.sd_inputs(case)
    pre, mean, invstd, act = R.sd_layer(x, l0, wt, beta, F64)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    wtt = torch.from_numpy(wt).double().requires_grad_(True)
    bt = torch.from_numpy(beta).double().requires_grad_(True)
    xin = xt[..., :ci]
    pt = TT.conv2d_same((torch.sigmoid(xin) if l0 else xin).permute(0, 3, 1, 2), wtt, 1)
    pt.retain_grad()
    at = TT.lrelu(TT.bn_train(pt, bt))
    _eq(pre, _nhwc(pt))
    _eq(act, _nhwc(at))
    dact = np.random.default_rng(9).uniform(-1, 1, size=act.shape)
    (at * _nchw(dact)).sum().backward()
    da0 = np.random.default_rng(10).uniform(-1, 1, size=x.shape) if l0 else None
    dpre, dbeta, dw, din = R.sd_layer_bwd(dact, pre, mean, invstd, beta, x, l0, wt, l0, da0, F64)
    _eq(dpre, _nhwc(pt.grad))
    _eq(dbeta, bt.grad.numpy())
    _eq(dw, wtt.grad.numpy())
    if l0:
        _eq(din[..., :ci], da0[..., :ci] + xt.grad.numpy()[..., :ci])
        assert np.array_equal(din[..., ci], da0[..., ci])
    else:
        _eq(din, xt.grad.numpy())


@pytest.mark.parametrize("case", [(5, 3, 3, 12, 12, 2.0, 0.7), (1, 1, 2, 4, 4, 0.5, 0.0), (8, 3, 2, 8, 20, 0.5, 0.7)])
def test_sd_head_bwd_is_autograd(case):
    ci, c, n, h, w, smax, reg = case
    act, w5, b5, mle, target, noise, dsample = R.head_inputs(case)
    tt = lambda v: torch.from_numpy(np.asarray(v)).double().requires_grad_(True)
    a_t, w_t, b_t, m_t = tt(act), tt(w5), tt(np.array([b5])), tt(mle)
    sd = smax * torch.sigmoid((a_t * w_t).sum(-1) + b_t)
    sample = m_t + reg * sd[..., None] * torch.from_numpy(noise).double()
    e = torch.log(sd)[..., None] + R.HALF_LOG_2PI + 0.5 * ((m_t - torch.from_numpy(target).double()) / sd[..., None]) ** 2
    rs, rsample, rnll = R.sd_head_fwd(act, w5, b5, smax, mle, target, noise, reg, F64)
    _eq(rs, sd.detach().numpy())
    _eq(rsample, sample.detach().numpy())
    _eq(rnll, e.sum(dim=(1, 2, 3)).detach().numpy())
    ((sample * torch.from_numpy(dsample).double()).sum() + R.HEAD_NLL_COEF * e.sum()).backward()
    dmle, dact, dw5, db5 = R.sd_head_bwd(act, w5, b5, smax, mle, target, noise, reg, R.HEAD_NLL_COEF, dsample, F64)
    for got, ref in ((dmle, m_t.grad), (dact, a_t.grad), (dw5, w_t.grad), (db5, b_t.grad[0])):
        _eq(got, ref.numpy())


# ------------------------------------------------------------------------------------------------ (2) the bounds
def _inside(name, twin, ref, tol, worst):
    e = R.rel_err(twin, ref)
    worst[name] = max(worst.get(name, 0.0), e)
    assert e <= tol, (name, e, tol)


def _outside(name, wrong, ref, tol):
    e = R.rel_err(wrong, ref)
    assert e > tol, ("a wrong twin passes the bound", name, e, tol)


def _report(worst):
    for k in sorted(worst):
        print("twin %-22s worst err / (1 + max|ref|) = %.2e" % (k, worst[k]))


def test_convt_twin_is_inside_the_bound():
    worst = {}
    for case in R.CONVT_CASES:
        args = R.convt_inputs(case)
        _inside("a_out", R.output_convt(*args, F32), R.output_convt(*args, F64), R.FWD_TOL, worst)
    _report(worst)


def test_output_bounds_discriminate():
    worst = {}
    for case in R.OUT_CASES:
        a, xprev, target, kl, dxhat = R.out_inputs(case)
        lo, hi = case[5], case[6]
        f = lambda dt, **kw: R.output_fwd(a, xprev, target, kl, lo, hi, R.OUT_MINH, R.OUT_MAXH, dt, **kw)
        ref, twin = f(F64), f(F32)
        _inside("xhat", twin[0], ref[0], R.FWD_TOL, worst)
        _inside("rec_img", twin[1], ref[1], R.SUM_TOL, worst)
        _inside("stats", twin[2], ref[2], R.SUM_TOL, worst)
        if xprev is not None:
            wrong = f(F32, wrong_drop_ratio=True)
            _outside("xhat without the ratio term", wrong[0], ref[0], R.FWD_TOL)
            _outside("rec_img without the ratio term", wrong[1], ref[1], R.SUM_TOL)
        for has_dx, rc in R.OUT_BWD_VARIANTS:
            b = lambda dt: R.output_bwd(a, xprev, ref[0], target, lo, hi, R.OUT_MINH, R.OUT_MAXH, rc,
                                        dxhat if has_dx else None, dt)
            rb, tb = b(F64), b(F32)
            _inside("da", tb[0], rb[0], R.FWD_TOL, worst)
            _inside("db", tb[2], rb[2], R.SUM_TOL, worst)
            if xprev is not None:
                _inside("dxprev", tb[1], rb[1], R.FWD_TOL, worst)
    _report(worst)


def test_sd_layer_bounds_discriminate():
    worst = {}
    for case in R.SD_CASES:
        ci, co, n, h, w, l0 = case
        x, wt, beta = R.sd_inputs(case)
        names = ("pre", "mean", "invstd", "act")
        ref, twin = R.sd_layer(x, l0, wt, beta, F64), R.sd_layer(x, l0, wt, beta, F32)
        for k, t_, r_ in zip(names, twin, ref):
            _inside(k, t_, r_, R.FWD_TOL, worst)
        _outside("pre, tap shifted", R.sd_layer(x, l0, wt, beta, F32, wrong_tap_shift=1)[0], ref[0], R.FWD_TOL)
        _outside("pre, pad 2 / 1", R.sd_layer(x, l0, wt, beta, F32, wrong_pad_before=2)[0], ref[0], R.FWD_TOL)
        blocks = -(-n * h * w // 256)
        if blocks > 1:
            wrong = R.sd_layer(x, l0, wt, beta, F32, wrong_skip_block=blocks // 2)
            _outside("mean, a block left out", wrong[1], ref[1], R.FWD_TOL)
        # backward
        x, wt, beta, mean, invstd, pre, dact, da0 = R.sd_bwd_inputs(case)
        assert np.abs(R.sd_y(pre, mean, invstd, beta)).min() >= R.KINK
        b = lambda dt, **kw: R.sd_layer_bwd(dact, pre, mean, invstd, beta, x, l0, wt, l0, da0, dt, **kw)
        rb, tb = b(F64), b(F32)
        _inside("dpre", tb[0], rb[0], R.FWD_TOL, worst)
        _inside("dbeta", tb[1], rb[1], R.SUM_TOL, worst)
        _inside("dw", tb[2], rb[2], R.SUM_TOL, worst)
        _inside("din", tb[3], rb[3], R.FWD_TOL, worst)
        _outside("dw, tap shifted", b(F32, wrong_tap_shift=1)[2], rb[2], R.SUM_TOL)
        if blocks > 1:
            _outside("dbeta, a block left out", b(F32, wrong_skip_block=blocks // 2)[1], rb[1], R.SUM_TOL)
    _report(worst)


def test_sd_head_bounds_discriminate():
    worst = {}
    for case in R.HEAD_CASES:
        ci, c, n, h, w, smax, reg = case
        act, w5, b5, mle, target, noise, dsample = R.head_inputs(case)
        f = lambda dt, w_=w5, **kw: R.sd_head_fwd(act, w_, b5, smax, mle, target, noise, reg, dt, **kw)
        ref, twin = f(F64), f(F32)
        _inside("sd", twin[0], ref[0], R.FWD_TOL, worst)
        _inside("sample", twin[1], ref[1], R.FWD_TOL, worst)
        _inside("nll_img", twin[2], ref[2], R.SUM_TOL, worst)
        if ci > 1:
            _outside("sd, W5 rotated", f(F32, w_=np.roll(w5, 1))[0], ref[0], R.FWD_TOL)
        if (h * w) % 256:
            _outside("nll_img, dead lanes", f(F32, wrong_dead_lanes=True)[2], ref[2], R.SUM_TOL)
        for ds in (None, dsample):
            b = lambda dt, w_=w5: R.sd_head_bwd(act, w_, b5, smax, mle, target, noise, reg, R.HEAD_NLL_COEF, ds, dt)
            rb, tb = b(F64), b(F32)
            for k, t_, r_, tol in zip(("dmle", "dact", "dw5", "db5"), tb, rb,
                                      (R.FWD_TOL, R.FWD_TOL, R.SUM_TOL, R.SUM_TOL)):
                _inside(k, t_, r_, tol, worst)
            if ci > 1:
                _outside("dw5, W5 rotated", np.roll(b(F32)[2], 1), rb[2], R.SUM_TOL)
    _report(worst)
