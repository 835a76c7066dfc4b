"""tests/recog_ref.py (the float64 reference of tests/test_recog_ops_gpu.py) against the project's own oracle
ops: oracle/tape.py clip, sigmoid, kl_per_row, kl_uniform_per_row and the FC + BN + lrelu of
oracle/model.py split_latent, forward and gradient, to 1e-12 -- a mistake in the new reference cannot
become the truth.  Runs without a GPU."""
import numpy as np
import pytest
import torch

import recog_ref as R
from oracle import model, tape as T

CLIP, PRIOR = 1.0, 0.5


def _rng(seed):
    return np.random.default_rng(seed)


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * (1 + np.abs(b).max()), np.abs(a - b).max()


def _latent_case():
    r = _rng(11)
    g, ns, b, dz = 2, 3, 5, 9
    part = r.uniform(-1, 1, (g, ns, b, 2 * dz))
    bm, bs = np.round(r.uniform(-0.5, 0.5, (g, dz)) * 64) / 64, r.uniform(-0.5, 0.5, (g, dz))  # bm: exact in binary
    # two means exactly on the clip bounds (the gradient passes there), and more than a few beyond them
    part[0, :, 1, 2] = 0.0
    part[0, 0, 1, 2] = CLIP - bm[0, 2]
    part[1, :, 3, 4] = 0.0
    part[1, 0, 3, 4] = -CLIP - bm[1, 4]
    eps, dzv = r.uniform(-1, 1, (g, b, dz)), r.uniform(-1, 1, (g, b, dz))
    return part, bm, bs, eps, dzv, np.array([0.37, 1.3])


@pytest.mark.parametrize("uniform", [0, 1])
def test_latent_matches_the_oracle_ops(uniform):
    part, bm, bs, eps, dzv, kc = _latent_case()
    g, _, b, dz2 = part.shape
    dz = dz2 // 2
    tt = torch.from_numpy
    mu, sig, z, kl = R.latent_fwd(tt(part), tt(bm), tt(bs), tt(eps), CLIP, PRIOR, uniform)
    dhead = R.latent_bwd(mu, sig, tt(eps), tt(dzv), tt(kc), CLIP, PRIOR, uniform)
    s = part.sum(1)
    assert (np.abs(s[..., :dz] + bm[:, None]) > CLIP).mean() > 0.05
    assert mu[0, 1, 2].item() == CLIP and mu[1, 3, 4].item() == -CLIP
    for gi in range(g):
        tp = T.Tape()
        m_raw = tp.leaf(s[gi, :, :dz] + bm[gi])
        s_pre = tp.leaf(s[gi, :, dz:] + bs[gi])
        mc = T.clip(tp, m_raw, -CLIP, CLIP)
        sg = T.sigmoid(tp, s_pre)
        zz = T.add(tp, mc, T.mul(tp, sg, tp.leaf(eps[gi])))
        klr = T.kl_uniform_per_row(tp, sg) if uniform else T.kl_per_row(tp, mc, sg, PRIOR)
        # sum(dz * z) + kc * sum_n kl[n]
        loss = T.scalar_sum(tp, [T.mean_all(tp, T.mul(tp, zz, tp.leaf(dzv[gi]))), T.mean_all(tp, klr)],
                            [float(b * dz), float(kc[gi] * b)])
        tp.backward(loss)
        _close(mu[gi], m_raw.v)
        _close(sig[gi], sg.v)
        _close(z[gi], zz.v)
        _close(kl[gi], klr.v)
        _close(dhead[gi, :, :dz], m_raw.g)
        _close(dhead[gi, :, dz:], s_pre.g)
    # the gradient of the mean passes on the bounds and is zero beyond them
    m = mu.numpy()
    assert (dhead[..., :dz].numpy()[np.abs(m) > CLIP] == 0).all()
    assert dhead[0, 1, 2].item() != 0 and dhead[1, 3, 4].item() != 0


def test_heads_are_the_oracle_matmul():
    r = _rng(12)
    x, wm, ws = r.uniform(-1, 1, (2, 5, 40)), r.uniform(-1, 1, (2, 40, 3)), r.uniform(-1, 1, (2, 40, 3))
    dm, ds, dx0 = r.uniform(-1, 1, (2, 5, 3)), r.uniform(-1, 1, (2, 5, 3)), r.uniform(-1, 1, (2, 5, 40))
    tt = torch.from_numpy
    m, s = R.heads(tt(x), tt(wm), tt(ws))
    dx, dwm, dws, dbm, dbs = R.heads_bwd(tt(x), tt(wm), tt(ws), tt(dm), tt(ds), tt(dx0))
    for gi in range(2):
        tp = T.Tape()
        xn, wmn, wsn = tp.leaf(x[gi]), tp.leaf(wm[gi]), tp.leaf(ws[gi])
        bmn, bsn = tp.leaf(np.zeros(3)), tp.leaf(np.zeros(3))
        mn, sn = T.bias_add(tp, T.matmul(tp, xn, wmn), bmn), T.bias_add(tp, T.matmul(tp, xn, wsn), bsn)
        loss = T.scalar_sum(tp, [T.mean_all(tp, T.mul(tp, mn, tp.leaf(dm[gi]))),
                                 T.mean_all(tp, T.mul(tp, sn, tp.leaf(ds[gi])))], [15.0, 15.0])
        tp.backward(loss)
        _close(m[gi], mn.v)
        _close(s[gi], sn.v)
        _close(dx[gi], dx0[gi] + xn.g)
        _close(dwm[gi], wmn.g)
        _close(dws[gi], wsn.g)
        _close(dbm[gi], bmn.g)
        _close(dbs[gi], bsn.g)


def test_splitfc_matches_the_oracle_split_latent():
    """Both levels of a two-level split_latent: level 0 is reshaped to [b, S, S, F] (the concat buffer's
    (j // f, j % f) addressing), level 1 stays flat."""
    r = _rng(13)
    b, dims, S, F, jtop = 7, [3, 5], 2, 4, 10
    cfg = {"levels": 2, "filter_sizes": [0, F, 0], "image_sizes": [0, S, 0], "latent_dims": dims}
    J = [S * S * F, jtop]
    z = r.uniform(-1, 1, (b, sum(dims)))
    tp = T.Tape()
    P, st = {}, {"split": []}
    for i in range(2):
        P["w%d" % i] = tp.leaf(r.uniform(-1, 1, (dims[i], J[i])))
        P["b%d" % i] = tp.leaf(r.uniform(-1, 1, (J[i],)))  # the FC bias, which batch norm removes
        P["beta%d" % i] = tp.leaf(r.uniform(-0.5, 0.5, (J[i],)))
        st["split"].append({"w": "w%d" % i, "b": "b%d" % i, "beta": "beta%d" % i})
    zn = tp.leaf(z)
    ladder = model.split_latent(tp, P, cfg, st, zn)
    dout = [r.uniform(-1, 1, ladder[i].v.shape) for i in range(2)]
    loss = T.scalar_sum(tp, [T.mean_all(tp, T.mul(tp, ladder[i], tp.leaf(dout[i]))) for i in range(2)],
                        [float(dout[0].size), float(dout[1].size)])
    tp.backward(loss)
    tt = torch.from_numpy
    zoff = 0
    for i in range(2):
        w, beta = tt(P["w%d" % i].v), tt(P["beta%d" % i].v)
        out, mean, inv, y = R.splitfc(tt(z), zoff, dims[i], w, beta)
        assert y.abs().min().item() > 1e-9  # no element on the lrelu kink
        _close(out, ladder[i].v.reshape(b, J[i]))
        pre = z[:, zoff:zoff + dims[i]] @ P["w%d" % i].v
        _close(mean, pre.mean(0))
        _close(inv, 1.0 / np.sqrt(pre.var(0) + 1e-3))
        dw, dbeta, dzl = R.splitfc_bwd(tt(z), zoff, dims[i], w, beta, tt(dout[i].reshape(b, J[i])))
        _close(dw, P["w%d" % i].g)
        _close(dbeta, P["beta%d" % i].g)
        _close(dzl, zn.g[:, zoff:zoff + dims[i]])
        zoff += dims[i]
    # the concat-buffer addressing of level 0 is the NHWC reshape when ldo = f and o_n = j
    off = R.splitfc_offsets(b, J[0], F, F, J[0])
    assert torch.equal(off, torch.arange(b * J[0]).view(b, J[0]))
    off = R.splitfc_offsets(2, 6, 3, 5, 20)
    assert off.tolist() == [[0, 1, 2, 5, 6, 7], [20, 21, 22, 25, 26, 27]]
