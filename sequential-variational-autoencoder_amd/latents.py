"""What a chain step's latent code carries: the "ELBO surgery" split of the mean KL (Hoffman & Johnson 2016) on
one svae_op_mixture_logdensity launch sequence (csrc/latents.hip) per call.

With q_n = N(mean_n, sigma_n^2) the posterior of image n, z_n one draw from it, q(z) = 1/N sum_n q_n(z) the
aggregate posterior over the N images and p(z) = N(0, p^2) the prior,

    mean_n KL(q_n || p)  =  I(x; z)  +  KL(q(z) || p(z)),

and the total correlation TC = KL(q(z) || prod_j q(z_j)) says how far the aggregate is from factorising.  All
three need log q(z_n) for every n: an N x N x D pairwise Gaussian log-density and a logsumexp, which is the op.
There is no torch formulation behind it: without the library the call raises.

Every quantity is a plain Monte-Carlo mean over the same N draws (sums over j in the segment S, means over n):

    own_n  = sum_j log N(z_nj; mean_nj, sigma_nj)
    logq_n = log sum_m exp(sum_j log N(z_nj; mean_mj, sigma_mj)) - log N        (the op, minus log N)
    logp_n = sum_j log N(z_nj; 0, p)
    mi          = mean(own - logq)          kl_sample = mean(own - logp) = mi + marginal_kl, identically
    marginal_kl = mean(logq - logp)         kl        = mean_n sum_j KL(N(mean, sigma^2) || N(0, p^2)), analytic
    tc          = mean(logq_S - sum_{j in S} logq_{dim j})
    active_units = #{j in S: Var_n(mean_nj) > 0.01}   (Burda et al. 2016; the population variance)

``mi`` cannot exceed log N (z_n's own component is in the mixture, so logq_n >= own_n - log N): ``mi_ceiling``
= log N comes with every report, and a value within a few percent of it means "saturated: the N images are
told apart completely, use more images", not "log N nats".  Under use_uniform_prior there is no proper prior:
marginal_kl, kl_sample and kl are None.  The engine's SVAE_BUF_KL_IMG is the reference's expression, a mean over
the dimensions without the log p term; ``kl`` here is the KL itself, summed over the dimensions, and the two
agree (times Dz) at p = 1.
"""
import ctypes
import math

import torch

from . import _lib

TILE = _lib.LATENTS_TILE
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def segments_for(cfg):
    """The report's segments as [(name, offset, length)]: "all" = (0, Dz), then "level0" .. "level{L-1}", then
    "dim0" .. "dim{Dz-1}".  The engine lays the ladder levels into the Dz columns in ascending order: level i
    (the one whose code enters the generator at resolution image_sizes[i + 1], level L - 1 at the top) owns the
    columns [sum(latent_dims[:i]), sum(latent_dims[:i + 1])) of SVAE_BUF_MU / _SIGMA / _Z, as the recognition
    network concatenates its heads and split_latent cuts z (oracle/model.py)."""
    dims = [int(d) for d in cfg.latent_dims]
    dz = sum(dims)
    segs, off = [("all", 0, dz)], 0
    for i, d in enumerate(dims):
        segs.append(("level%d" % i, off, d))
        off += d
    return segs + [("dim%d" % j, j, 1) for j in range(dz)]


def _rows(t, what):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise ValueError("mixture_logdensity takes %s as a float32 [rows, d] GPU tensor with contiguous rows" % what)
    return int(t.stride(0))


def mixture_logdensity(z, mu, sigma, segments, out=None):
    """[nq, n_seg] fp64 device tensor: out[n][s] = log sum_m exp(sum_{j in S_s} log N(z[n][j]; mu[m][j],
    sigma[m][j]^2)), without the log nm.  z [nq, d], mu and sigma [nm, d] (one row stride for both) are float32
    tensors on one GPU whose rows are contiguous (a row stride above d is passed on as the leading dimension);
    ``segments`` is a list of (offset, length), or of (name, offset, length) as segments_for gives.  ``out``: a
    contiguous fp64 device tensor of at least nq * n_seg elements to write into.  The launches go to z's
    device's current stream, nothing synchronises."""
    ldz, ldm = _rows(z, "z"), _rows(mu, "mu")
    if _rows(sigma, "sigma") != ldm or mu.shape != sigma.shape or mu.shape[1] != z.shape[1]:
        raise ValueError("mixture_logdensity takes mu and sigma of one shape and row stride, and z of their width")
    if mu.device != z.device or sigma.device != z.device:
        raise ValueError("mixture_logdensity takes tensors on one GPU")
    segs = [tuple(s)[-2:] for s in segments]
    n_seg, nq, nm, d = len(segs), int(z.shape[0]), int(mu.shape[0]), int(z.shape[1])
    flat = (ctypes.c_int32 * max(1, 2 * n_seg))(*[int(v) for s in segs for v in s])
    if out is None:
        out = torch.empty(nq, n_seg, dtype=torch.float64, device=z.device)
    elif out.dtype != torch.float64 or out.device != z.device or not out.is_contiguous() or out.numel() < nq * n_seg:
        raise ValueError("out must be a contiguous float64 tensor of at least nq * n_seg elements on z's device")
    _lib.check(_lib.lib().svae_op_mixture_logdensity(
        ctypes.c_void_p(z.data_ptr()), nq, ldz, ctypes.c_void_p(mu.data_ptr()), ctypes.c_void_p(sigma.data_ptr()),
        nm, ldm, d, flat, n_seg, _lib.ptr(out), _lib.stream_ptr(torch.cuda.current_stream(z.device))))
    return out.view(-1)[:nq * n_seg].view(nq, n_seg)


class Layout:
    """Where the numbers of one information() table sit: the table is the concatenation of
    [mi, marginal_kl, kl_sample, kl] per segment ([n_seg, 4] flattened), tc and active_units per group segment
    ("all" and the levels, [1 + L, 2] flattened) and the non-finite count."""

    def __init__(self, segments):
        self.segments = [tuple(s) for s in segments]
        self.names = [s[0] for s in self.segments]
        self.dim_col = {s[1]: i for i, s in enumerate(self.segments) if s[2] == 1 and s[0].startswith("dim")}
        self.groups = [i for i, s in enumerate(self.segments) if not s[0].startswith("dim")]
        self.size = 4 * len(self.segments) + 2 * len(self.groups) + 1

    def report(self, row, uniform):
        """One step's {"all", "levels", "dims", "nonfinite"} from its table as a host list."""
        n = len(self.segments)

        def entry(i, g=None):
            mi, mkl, kls, kl = row[4 * i:4 * i + 4]
            e = {"mi": mi, "marginal_kl": None if uniform else mkl, "kl_sample": None if uniform else kls,
                 "kl": None if uniform else kl}
            if g is not None:
                e["tc"], e["active_units"] = row[4 * n + 2 * g], int(row[4 * n + 2 * g + 1])
            return e

        groups = {self.names[i]: entry(i, g) for g, i in enumerate(self.groups)}
        dims = [entry(self.dim_col[j]) for j in sorted(self.dim_col)]
        return {"all": groups["all"],
                "levels": [groups[k] for k in self.names if k.startswith("level")],
                "dims": {k: (None if uniform and k != "mi" else [d[k] for d in dims])
                         for k in ("mi", "marginal_kl", "kl")},
                "nonfinite": int(row[-1])}


def _segments(cfg_or_segments):
    return segments_for(cfg_or_segments) if hasattr(cfg_or_segments, "latent_dims") else list(cfg_or_segments)


def information(z, mean, sigma, cfg_or_segments, prior_stddev):
    """The estimators of the module docstring for one chain step, as a flat fp64 device tensor laid out as
    Layout(segments) says (so a caller stacks T steps and copies once): z, mean, sigma are [N, Dz] float32 on
    one GPU, z_n drawn from N(mean_n, sigma_n^2) with ``mean`` the clipped posterior mean
    (clamp(SVAE_BUF_MU, +-cfg.latent_mean_clip): the buffer holds the pre-clip value).  ``cfg_or_segments``: a
    config (segments_for's list) or such a list of (name, offset, length) holding "all", levels and every
    "dim<j>".  ``prior_stddev`` None is the uniform prior: the three prior columns are then zeros that
    Layout.report turns into None.  Under predict_latent_code the posteriors are the recognition network's as the
    engine ran them, q(z_t | x_{t-1}); the definitions do not change.

    One mixture_logdensity call with nq = nm = N; the rest is torch fp64 on the device."""
    lay = Layout(_segments(cfg_or_segments))
    N, dz = int(z.shape[0]), int(z.shape[1])
    if sorted(lay.dim_col) != list(range(dz)):
        raise ValueError("information needs a 'dim<j>' segment for every one of the %d dimensions" % dz)
    lse = mixture_logdensity(z, mean, sigma, lay.segments)
    logq = lse - math.log(N)
    zd, md, sd = z.double(), mean.double(), sigma.double()
    own_d = -0.5 * ((zd - md) / sd) ** 2 - torch.log(sd) - _HALF_LOG_2PI
    if prior_stddev is not None:
        p = float(prior_stddev)
        logp_d = -0.5 * (zd / p) ** 2 - math.log(p) - _HALF_LOG_2PI
        kl_d = math.log(p) - torch.log(sd) + (sd * sd + md * md) / (2.0 * p * p) - 0.5
    var = md.var(dim=0, unbiased=False)
    cols = torch.zeros(len(lay.segments), 4, dtype=torch.float64, device=z.device)
    grp = torch.zeros(len(lay.groups), 2, dtype=torch.float64, device=z.device)
    dcols = [lay.dim_col[j] for j in range(dz)]
    logq_d = logq[:, dcols]  # [N, Dz]: column j is the single dimension j
    # the single dimensions at once, then the few group segments one by one
    cols[dcols, 0] = (own_d - logq_d).mean(0)
    if prior_stddev is not None:
        cols[dcols, 1] = (logq_d - logp_d).mean(0)
        cols[dcols, 2] = (own_d - logp_d).mean(0)
        cols[dcols, 3] = kl_d.mean(0)
    for g, i in enumerate(lay.groups):
        _, off, ln = lay.segments[i]
        own = own_d[:, off:off + ln].sum(1)
        cols[i, 0] = (own - logq[:, i]).mean()
        if prior_stddev is not None:
            logp = logp_d[:, off:off + ln].sum(1)
            cols[i, 1] = (logq[:, i] - logp).mean()
            cols[i, 2] = (own - logp).mean()
            cols[i, 3] = kl_d[:, off:off + ln].sum(1).mean()
        grp[g, 0] = (logq[:, i] - logq_d[:, off:off + ln].sum(1)).mean()
        grp[g, 1] = (var[off:off + ln] > 0.01).sum()
    bad = (~torch.isfinite(lse)).sum().double().reshape(1)
    return torch.cat([cols.reshape(-1), grp.reshape(-1), bad])
