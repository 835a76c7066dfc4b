"""numpy float64 reference of svae_op_mixture_logdensity and of latents.information (no package import).

``mixture_logdensity`` is the two-pass form: every exponent of a query row, their maximum, then the sum of
exp(e - max).  ``information`` restates the estimator definitions of the package's latents.py on top of it.
"""
import math

import numpy as np

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def log_normal(z, mean, sigma):
    """Elementwise log N(z; mean, sigma^2) in float64."""
    z, mean, sigma = (np.asarray(a, np.float64) for a in (z, mean, sigma))
    return -0.5 * ((z - mean) / sigma) ** 2 - np.log(sigma) - HALF_LOG_2PI


def mixture_logdensity(z, mu, sigma, segments, block=64):
    """out[n][s] = log sum_m exp(sum_{j in S_s} log N(z[n][j]; mu[m][j], sigma[m][j]^2)); segments = (offset,
    length) pairs.  Query rows are taken ``block`` at a time to bound the [block, nm, d] intermediate."""
    z, mu, sigma = (np.asarray(a, np.float64) for a in (z, mu, sigma))
    nq = z.shape[0]
    out = np.empty((nq, len(segments)), np.float64)
    with np.errstate(all="ignore"):
        for a in range(0, nq, block):
            t = log_normal(z[a:a + block, None, :], mu[None], sigma[None])  # [b, nm, d]
            for s, (off, ln) in enumerate(segments):
                e = t[:, :, off:off + ln].sum(axis=2)
                m = e.max(axis=1)
                out[a:a + block, s] = m + np.log(np.exp(e - m[:, None]).sum(axis=1))
    return out


def segments_for(latent_dims):
    """[(name, offset, length)]: "all", "level<i>" (ascending slices of the columns), "dim<j>"."""
    dz = int(sum(latent_dims))
    segs, off = [("all", 0, dz)], 0
    for i, n in enumerate(latent_dims):
        segs.append(("level%d" % i, off, int(n)))
        off += int(n)
    return segs + [("dim%d" % j, j, 1) for j in range(dz)]


def information(z, mean, sigma, latent_dims, prior_stddev):
    """The report of one chain step from z, mean, sigma [N, Dz] (mean already clipped); prior_stddev None: the
    uniform prior.  Returns {"mi_ceiling", "nonfinite", "all": {...}, "levels": [{...}], "dims": {...}}."""
    z, mean, sigma = (np.asarray(a, np.float64) for a in (z, mean, sigma))
    n, dz = z.shape
    named = segments_for(latent_dims)
    lse = mixture_logdensity(z, mean, sigma, [(o, l) for _, o, l in named])
    logq = lse - math.log(n)
    own_d = log_normal(z, mean, sigma)
    uniform = prior_stddev is None
    if not uniform:
        p = float(prior_stddev)
        logp_d = log_normal(z, 0.0, p)
        kl_d = np.log(p / sigma) + (sigma ** 2 + mean ** 2) / (2.0 * p * p) - 0.5
    var = mean.var(axis=0)
    dim_col = {j: 1 + len(latent_dims) + j for j in range(dz)}

    def entry(col, off, ln, with_tc):
        sl = slice(off, off + ln)
        own = own_d[:, sl].sum(axis=1)
        e = {"mi": float(np.mean(own - logq[:, col]))}
        if uniform:
            e["marginal_kl"] = e["kl_sample"] = e["kl"] = None
        else:
            logp = logp_d[:, sl].sum(axis=1)
            e["marginal_kl"] = float(np.mean(logq[:, col] - logp))
            e["kl_sample"] = float(np.mean(own - logp))
            e["kl"] = float(np.mean(kl_d[:, sl].sum(axis=1)))
        if with_tc:
            e["tc"] = float(np.mean(logq[:, col] - sum(logq[:, dim_col[j]] for j in range(off, off + ln))))
            e["active_units"] = int(np.sum(var[sl] > 0.01))
        return e

    res = {"mi_ceiling": math.log(n), "nonfinite": int(np.sum(~np.isfinite(lse)))}
    res["all"] = entry(0, 0, dz, True)
    res["levels"] = [entry(1 + i, named[1 + i][1], named[1 + i][2], True) for i in range(len(latent_dims))]
    dims = [entry(dim_col[j], j, 1, False) for j in range(dz)]
    res["dims"] = {k: [d[k] for d in dims] for k in ("mi", "marginal_kl", "kl")}
    if uniform:
        res["dims"]["marginal_kl"] = res["dims"]["kl"] = None
    return res
