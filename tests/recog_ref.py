"""Plain torch restatements of the recognition heads, the reparameterised latent with its KL term and the
split-latent FC + BN + lrelu (csrc/misc.hip), with autograd for the gradients.  Every function computes in
the dtype of its inputs: float64 is the reference of tests/test_recog_ops_gpu.py, float32 the "plain fp32
arithmetic" whose distance from it sizes that file's bounds.  tests/test_recog_ref.py holds these
restatements to the oracle's own ops (oracle/tape.py, oracle/model.py) on the CPU.

Layouts (include/svae_hip.h): a leading group axis where the engine batches chain steps; the heads of one
level own columns coff .. coff + d - 1 (mean) and cols / 2 + coff .. (stddev) of a [.., b, cols] tensor."""
import torch


def head_cols(t, d, coff):
    """(mean, stddev) column blocks of one level in a [.., cols] partial / gradient tensor."""
    h = t.shape[-1] // 2
    return t[..., coff:coff + d], t[..., h + coff:h + coff + d]


def heads(x, wm, ws):
    """x [g, b, k] @ wm, ws [g, k, d]."""
    return x @ wm, x @ ws


def heads_bwd(x, wm, ws, dh_m, dh_s, dx0=None):
    """Gradients of sum(dh_m * (x @ wm + bm)) + sum(dh_s * (x @ ws + bs)): dx (+ dx0), dwm, dws, dbm, dbs."""
    x, wm, ws = (t.detach().clone().requires_grad_(True) for t in (x, wm, ws))
    g, d = wm.shape[0], wm.shape[2]
    bm, bs = (torch.zeros(g, 1, d, dtype=x.dtype, requires_grad=True) for _ in range(2))
    m, s = heads(x, wm, ws)
    ((m + bm) * dh_m).sum().add(((s + bs) * dh_s).sum()).backward()
    dx = x.grad if dx0 is None else dx0 + x.grad
    return dx, wm.grad, ws.grad, bm.grad[:, 0], bs.grad[:, 0]


def latent(mu, spre, eps, clip, prior, uniform):
    """mu: raw mean, spre: pre-sigmoid value -> (sig, z, kl_img); kl_img is the mean over the last axis."""
    mc = torch.clamp(mu, -clip, clip)
    sig = torch.sigmoid(spre)
    z = mc + sig * eps
    if uniform:
        kl = (-torch.log(sig)).mean(-1)
    else:
        p2 = prior * prior
        kl = (-0.5 - torch.log(sig) + 0.5 * sig * sig / p2 + 0.5 * mc * mc / p2).mean(-1)
    return sig, z, kl


def latent_fwd(part, bm, bs, eps, clip, prior, uniform):
    """part [g, nsplit, b, 2 Dz] (mean | stddev partial sums), bm, bs [g, Dz], eps [g, b, Dz] ->
    mu (raw), sig, z [g, b, Dz], kl_img [g, b]."""
    dz = bm.shape[-1]
    s = part.sum(1)
    mu = s[..., :dz] + bm[:, None]
    sig, z, kl = latent(mu, s[..., dz:] + bs[:, None], eps, clip, prior, uniform)
    return mu, sig, z, kl


def latent_bwd(mu, sig, eps, dz, kl_coef, clip, prior, uniform):
    """Gradient of sum(dz * z) + kl_coef[g] * sum_n kl_img[g, n] with respect to the raw mean and to the
    pre-sigmoid value logit(sig), as dhead [g, b, 2 Dz].  mu, sig [g, b, Dz] are the stored forward values."""
    mu = mu.detach().clone().requires_grad_(True)
    spre = (torch.log(sig) - torch.log1p(-sig)).detach().requires_grad_(True)
    _, z, kl = latent(mu, spre, eps, clip, prior, uniform)
    ((dz * z).sum() + (kl_coef[:, None] * kl).sum()).backward()
    return torch.cat([mu.grad, spre.grad], -1)


def lrelu(y):
    """max(min(0.1 y, 0), y) with the gradient 0.1 at y <= 0 (oracle/tape.py lrelu)."""
    return torch.where(y > 0, y, 0.1 * y)


def splitfc(z, zoff, k, w, beta):
    """z [b, ldz], w [k, j], beta [j] -> out [b, j], mean [j], invstd [j], y = xhat + beta [b, j]."""
    pre = z[:, zoff:zoff + k] @ w
    mean = pre.mean(0)
    inv = 1.0 / torch.sqrt(((pre - mean) ** 2).mean(0) + 1e-3)
    y = (pre - mean) * inv + beta
    return lrelu(y), mean, inv, y


def splitfc_bwd(z, zoff, k, w, beta, dout):
    """Gradients of sum(dout * out): dw [k, j], dbeta [j], dz [b, k] (of the level's own columns)."""
    zl = z[:, zoff:zoff + k].detach().clone().requires_grad_(True)
    w, beta = (t.detach().clone().requires_grad_(True) for t in (w, beta))
    out = splitfc(zl, 0, k, w, beta)[0]
    (out * dout).sum().backward()
    return w.grad, beta.grad, zl.grad


def splitfc_offsets(b, j, f, ldo, o_n):
    """Flat offsets [b, j] of the elements of out in the concat buffer: n * o_n + (jj // f) * ldo + jj % f."""
    jj = torch.arange(j)
    return torch.arange(b)[:, None] * o_n + ((jj // f) * ldo + jj % f)[None, :]
