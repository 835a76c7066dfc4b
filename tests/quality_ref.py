"""numpy float64 reference for quality.py and svae_op_pairwise_stats, by the direct form d2 = sum_k (x - y)^2 (no
norms, no inner product: nothing cancels)."""
import numpy as np

SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)


def sqdist(x, y):
    """[n, m] float64: sum_k (x[i][k] - y[j][k])^2, one row of x at a time."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((x.shape[0], y.shape[0]))
    for i in range(x.shape[0]):
        out[i] = np.square(y - x[i]).sum(1)
    return out


def pairwise_stats(x, groups, bandwidths, self_group=None):
    """(ksum [n, G, n_bw], nn_d2 [n, G], nn_idx [n, G], d2 per group) for sigma^2 in ``bandwidths``; with
    self_group = g the pairs (i, i) of group g are left out.  No admissible column: +inf and -1."""
    n, G, bw = len(x), len(groups), [float(b) for b in bandwidths]
    ksum = np.zeros((n, G, len(bw)))
    nn_d2 = np.full((n, G), np.inf)
    nn_idx = np.full((n, G), -1, np.int64)
    d2s = []
    for g, y in enumerate(groups):
        d2 = sqdist(x, y)
        d2s.append(d2)
        ok = np.ones(d2.shape, bool)
        if self_group == g:
            ok[np.arange(n), np.arange(n)] = False
        for l, s2 in enumerate(bw):
            ksum[:, g, l] = np.where(ok, np.exp(-d2 / (2.0 * s2)), 0.0).sum(1)
        masked = np.where(ok, d2, np.inf)
        has = ok.any(1)
        nn_idx[has, g] = masked[has].argmin(1)  # the first smallest
        nn_d2[has, g] = masked[has].min(1)
    return ksum, nn_d2, nn_idx, d2s


def sigma0_sq(real):
    """The mean squared distance between distinct rows, closed form from the first two moments."""
    r = np.asarray(real, np.float64)
    N = r.shape[0]
    return 2.0 * N / (N - 1) * (np.square(r).sum(1).mean() - np.square(r.mean(0)).sum())


def bandwidths(real):
    return [sigma0_sq(real) * s for s in SCALES]


def two_sample(x, y, bw=None):
    """quality.two_sample's dict (module docstring of quality.py) in float64."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, m, d = len(x), len(y), x.shape[1]
    bw = bandwidths(y) if bw is None else list(bw)
    kx, dx, _, _ = pairwise_stats(x, [x, y], bw, self_group=0)
    ky, dy, _, _ = pairwise_stats(y, [y, x], bw, self_group=0)
    mmd2 = kx[:, 0].sum(0) / (n * (n - 1.0)) + ky[:, 0].sum(0) / (m * (m - 1.0)) - 2.0 * kx[:, 1].sum(0) / (n * m)
    cx, cy = (dx[:, 0] < dx[:, 1]).sum(), (dy[:, 0] < dy[:, 1]).sum()
    rms = np.sqrt(dx[:, 1] / d)
    return {"mmd2": [float(v) for v in mmd2], "mmd2_at_sigma0": float(mmd2[len(bw) // 2]),
            "nn_accuracy": {"x": cx / n, "y": cy / m, "all": (cx + cy) / (n + m)},
            "nn_other": {"mean": float(rms.mean()), "median": float(np.median(rms)), "min": float(rms.min())},
            "sigma0": float(bw[len(bw) // 2]) ** 0.5}
