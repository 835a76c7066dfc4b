"""numpy float64 reference for svae_op_pairwise_knn and quality.manifold, by the direct form d2 = sum_k (x - y)^2
(quality_ref.sqdist): the k smallest distances per row, the per-column ball counts, and improved precision / recall
(Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) on squared distances."""
import numpy as np

from quality_ref import sqdist


def knn_stats(x, groups, k, radii=None, self_group=None):
    """(knn_d2 [n, G, k], inside [n, G, n_radii], nonfinite [n, G], d2 per group).  ``radii``: per group an
    [m_g, n_radii] array of squared radii or None (counts 0).  A NaN d2 is counted in nonfinite and enters nothing
    else; the pairs (i, i) of ``self_group`` are left out; fewer than k admitted columns pad with +inf."""
    n, G = len(x), len(groups)
    radii = [None] * G if radii is None else list(radii)
    nr = max([np.asarray(r).shape[1] for r in radii if r is not None], default=0)
    knn = np.full((n, G, k), np.inf)
    inside = np.zeros((n, G, nr), np.int64)
    bad = np.zeros((n, G), np.int64)
    d2s = []
    with np.errstate(invalid="ignore", over="ignore"):
        for g, y in enumerate(groups):
            d2 = sqdist(x, y)
            d2s.append(d2)
            ok = np.ones(d2.shape, bool)
            if self_group == g:
                ok[np.arange(n), np.arange(n)] = False
            nan = ~np.isfinite(d2)
            bad[:, g] = (ok & nan).sum(1)
            ok &= ~nan
            s = np.sort(np.where(ok, d2, np.inf), 1)[:, :k]
            knn[:, g, :s.shape[1]] = s
            if radii[g] is not None:
                r = np.asarray(radii[g], np.float64)
                inside[:, g, :] = (ok[:, :, None] & (d2[:, :, None] <= r[None, :, :])).sum(1)
    return knn, inside, bad, d2s


def self_radii(y, ks):
    """[m, len(ks)]: the squared distance of every point to its k-th nearest other point."""
    knn, _, _, _ = knn_stats(y, [y], max(ks), self_group=0)
    return knn[:, 0, [k - 1 for k in ks]]


def manifold(x, y, ks=(3, 5)):
    """quality.manifold's dict (module docstring of quality.py) in float64."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, m, ks = len(x), len(y), [int(k) for k in ks]
    if min(n, m) < max(ks) + 1:
        raise ValueError("manifold at k = %d needs %d points per set" % (max(ks), max(ks) + 1))
    ry, rx = self_radii(y, ks), self_radii(x, ks)
    _, ixy, bx, _ = knn_stats(x, [y], 0, radii=[ry])
    kyx, iyx, by, _ = knn_stats(y, [x], 1, radii=[rx])
    kk = np.asarray(ks, np.float64)
    return {"k": ks, "precision": (ixy[:, 0] > 0).mean(0).tolist(), "recall": (iyx[:, 0] > 0).mean(0).tolist(),
            "density": (ixy[:, 0].sum(0) / (kk * n)).tolist(), "coverage": (kyx[:, 0, :1] <= ry).mean(0).tolist(),
            "nonfinite": int(bx.sum() + by.sum())}
