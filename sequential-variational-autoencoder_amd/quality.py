"""How close a set of generated images is to a set of real ones, without a pretrained network: the kernel MMD^2
two-sample estimate (Gretton et al. 2012, unbiased form), the leave-one-out 1-nearest-neighbour two-sample
accuracy (Lopez-Paz & Oquab 2017) and nearest-neighbour distances, all on svae_op_pairwise_stats
(csrc/pairwise.hip): row-wise Gaussian-kernel sums and nearest columns of the pairwise squared distances, with no
[n, m] intermediate.  There is no torch formulation behind it: without the library the calls raise.

With k_s(a, b) = exp(-|a - b|^2 / (2 s^2)), x [n, d] and y [m, d]:

    mmd2(s)     = sum_{i != j} k_s(x_i, x_j) / (n (n - 1)) + sum_{i != j} k_s(y_i, y_j) / (m (m - 1))
                  - 2 sum_{i, j} k_s(x_i, y_j) / (n m)                    (0 in expectation for one distribution)
    nn_accuracy = the share of points whose nearest OTHER point of their own set is strictly closer than their
                  nearest point of the other set (a tie counts as wrong): 0.5 indistinguishable, 1.0 separable
    nn_other    = mean / median / min over x of the distance to the nearest y, as per-element RMS sqrt(d2 / d)

at the bandwidths s^2 = sigma0^2 * SCALES, sigma0^2 the mean squared distance between distinct points of y
(bandwidths(): closed form from the first two moments, no [m, m] pass).

Those numbers say that two sets differ, not how.  The k-nearest-neighbour manifold metrics split the difference into
fidelity and diversity: improved precision and recall (Kynkaanniemi et al. 2019) and their outlier-robust versions,
density and coverage (Naeem et al. 2020), on svae_op_pairwise_knn (csrc/knn.hip: the k smallest squared distances
per row and the number of per-column balls a row falls into, on the same distance tile, again with no [n, m]
intermediate and no torch formulation behind it).  With r_k(p)^2 the squared distance of p to its k-th nearest
OTHER point of its own set, inside(p; S, r) = #{s in S : |p - s|^2 <= r(s)^2}, x [n, d] the samples and y [m, d]
the real points (manifold()):

    precision_k = mean_i [ inside(x_i; y, r_k(y)) > 0 ]     the share of samples inside the real manifold (fidelity)
    density_k   = mean_i   inside(x_i; y, r_k(y)) / k       how many real balls hold a sample; 1 in expectation for
                                                            one distribution, unbounded above
    recall_k    = mean_j [ inside(y_j; x, r_k(x)) > 0 ]     the share of real points inside the sample manifold
    coverage_k  = mean_j [ min_i |y_j - x_i|^2 <= r_k(y_j)^2 ]   the share of real balls that hold a sample (diversity)

All comparisons are on squared distances.  These are manifolds in PIXEL space, as crude as pixel-space MMD: the
papers measure in the feature space of a pretrained network, which this project does without.  Read them against
the calibration line the report gives (held-out real images against training images), not against 1.
"""
import ctypes

import torch

from . import _lib

TILE_ROWS, TILE_COLS, TILE_K = _lib.PAIRWISE_TILE_ROWS, _lib.PAIRWISE_TILE_COLS, _lib.PAIRWISE_TILE_K
MAX_GROUPS, MAX_BW = _lib.PAIRWISE_MAX_GROUPS, _lib.PAIRWISE_MAX_BW
KNN_MAX_K, KNN_MAX_RADII = _lib.KNN_MAX_K, _lib.KNN_MAX_RADII
SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)

_scratch = {}  # device -> kept uint8 scratch tensor (grown, never shrunk)


def _rows(t, what, op="pairwise_stats"):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.shape[0] < 1 or t.shape[1] < 1 \
            or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("%s takes %s as a float32 [rows, d] GPU tensor with contiguous rows" % (op, what))
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def _out(out, key, shape, dtype, device):
    n = 1
    for s in shape:
        n *= s
    if out is None or out.get(key) is None:
        return torch.empty(shape, dtype=dtype, device=device)
    t = out[key]
    if t.dtype != dtype or t.device != device or not t.is_contiguous() or t.numel() < n:
        raise ValueError("out[%r] must be a contiguous %s tensor of at least %d elements on x's device" % (key, dtype, n))
    return t.view(-1)[:n].view(shape)


def pairwise_stats(x, groups, bandwidths, self_group=None, out=None, ksum=True, nn=True):
    """(ksum [n, G, n_bw] fp64, nn_d2 [n, G] fp64, nn_idx [n, G] int64) device tensors of svae_op_pairwise_stats
    for the rows x [n, d] against the column groups ``groups`` (a list of [m_g, d] tensors): the Gaussian-kernel
    sums at the variances ``bandwidths`` (a list of sigma^2), the smallest squared distance and its column, per
    row and group.  float32 tensors on one GPU whose rows are contiguous (a row stride above d is passed on as
    the leading dimension, so column or row slices of a larger tensor need no copy).  ``self_group`` = g: x is
    groups[g] itself and the pairs (i, i) are left out.  ``ksum`` / ``nn`` False (or an empty ``bandwidths``)
    skips that part and returns None for it.  ``out``: a dict with any of "ksum", "nn_d2", "nn_idx" to write
    into.  The launches go to x's device's current stream, nothing synchronises; the scratch the op needs is
    kept per device and grown on demand."""
    ldx = _rows(x, "x")
    groups = list(groups)
    G, n, d = len(groups), int(x.shape[0]), int(x.shape[1])
    ldy = [_rows(y, "group %d" % g) for g, y in enumerate(groups)]
    for y in groups:
        if y.device != x.device or y.shape[1] != d:
            raise ValueError("pairwise_stats takes groups of x's width on x's device")
    bw = [float(b) for b in bandwidths]
    ksum = bool(ksum) and len(bw) > 0
    if not ksum:
        bw = []
    sg = -1 if self_group is None else int(self_group)
    dev = x.device
    m = (ctypes.c_int64 * max(1, G))(*[int(y.shape[0]) for y in groups])
    L = _lib.lib()
    need = int(L.svae_op_pairwise_scratch_bytes(n, m, G, len(bw)))
    scratch = _scratch.get(dev)
    if need > 0 and (scratch is None or scratch.numel() < need):
        _scratch[dev] = scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    ks = _out(out, "ksum", (n, G, len(bw)), torch.float64, dev) if ksum else None
    nd = _out(out, "nn_d2", (n, G), torch.float64, dev) if nn else None
    ni = _out(out, "nn_idx", (n, G), torch.int64, dev) if nn else None
    yp = (ctypes.c_void_p * max(1, G))(*[y.data_ptr() for y in groups])
    ld = (ctypes.c_int64 * max(1, G))(*ldy)
    inv = (ctypes.c_double * max(1, len(bw)))(*[0.5 / b if b != 0.0 else float("inf") for b in bw])
    _lib.check(L.svae_op_pairwise_stats(
        ctypes.c_void_p(x.data_ptr()), n, ldx, yp, m, ld, G, d, sg, inv, len(bw),
        None if ks is None else ctypes.c_void_p(ks.data_ptr()), None if nd is None else ctypes.c_void_p(nd.data_ptr()),
        None if ni is None else ctypes.c_void_p(ni.data_ptr()),
        None if scratch is None else ctypes.c_void_p(scratch.data_ptr()),
        _lib.stream_ptr(torch.cuda.current_stream(dev))))
    return ks, nd, ni


def knn_stats(x, groups, k, radii=None, self_group=None, out=None):
    """(knn_d2 [n, G, k] fp64, inside [n, G, n_radii] int64, nonfinite [n, G] int64) device tensors of
    svae_op_pairwise_knn for the rows x [n, d] against the column groups ``groups`` (a list of [m_g, d] tensors, as
    pairwise_stats takes them): the k smallest squared distances in ascending order (+inf past the admitted
    columns), the number of columns j whose squared radius radii[g][j, r] is at least the distance, and the number of
    NaN distances, which enter neither.  ``radii``: a list with one [m_g, n_radii] contiguous fp64 tensor or None
    (no radii for that group: its counts are 0) per group, or None for no counts at all; ``k`` = 0 skips the
    distances.  A skipped part is returned as None.  ``self_group`` = g: x is groups[g] itself and the pairs (i, i)
    are left out.  ``out``: a dict with any of "knn_d2", "inside", "nonfinite" to write into.  The launches go to
    x's device's current stream, nothing synchronises; the scratch is pairwise_stats' own kept one."""
    ldx = _rows(x, "x", "knn_stats")
    groups = list(groups)
    G, n, d, k = len(groups), int(x.shape[0]), int(x.shape[1]), int(k)
    ldy = [_rows(y, "group %d" % g, "knn_stats") for g, y in enumerate(groups)]
    for y in groups:
        if y.device != x.device or y.shape[1] != d:
            raise ValueError("knn_stats takes groups of x's width on x's device")
    radii = [None] * G if radii is None else list(radii)
    if len(radii) != G:
        raise ValueError("knn_stats takes one radii tensor (or None) per group")
    nr = 0
    for g, r in enumerate(radii):
        if r is None:
            continue
        if r.dim() != 2 or r.dtype != torch.float64 or r.device != x.device or not r.is_contiguous() \
                or r.shape[0] != groups[g].shape[0] or r.shape[1] < 1 or (nr and r.shape[1] != nr):
            raise ValueError("knn_stats takes radii[%d] as a contiguous float64 [m_g, n_radii] tensor on x's device, "
                             "n_radii the same for every group" % g)
        nr = int(r.shape[1])
    sg = -1 if self_group is None else int(self_group)
    dev = x.device
    m = (ctypes.c_int64 * max(1, G))(*[int(y.shape[0]) for y in groups])
    L = _lib.lib()
    need = int(L.svae_op_knn_scratch_bytes(n, m, G, k, nr))
    scratch = _scratch.get(dev)
    if need > 0 and (scratch is None or scratch.numel() < need):
        _scratch[dev] = scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    kd = _out(out, "knn_d2", (n, G, k), torch.float64, dev) if k > 0 else None
    ins = _out(out, "inside", (n, G, nr), torch.int64, dev) if nr > 0 else None
    nf = _out(out, "nonfinite", (n, G), torch.int64, dev)
    yp = (ctypes.c_void_p * max(1, G))(*[y.data_ptr() for y in groups])
    ld = (ctypes.c_int64 * max(1, G))(*ldy)
    rp = (ctypes.c_void_p * max(1, G))(*[None if r is None else r.data_ptr() for r in radii])
    _lib.check(L.svae_op_pairwise_knn(
        ctypes.c_void_p(x.data_ptr()), n, ldx, yp, m, ld, G, d, sg, k,
        None if kd is None else ctypes.c_void_p(kd.data_ptr()), rp if nr > 0 else None, nr,
        None if ins is None else ctypes.c_void_p(ins.data_ptr()), ctypes.c_void_p(nf.data_ptr()),
        None if scratch is None else ctypes.c_void_p(scratch.data_ptr()),
        _lib.stream_ptr(torch.cuda.current_stream(dev))))
    return kd, ins, nf


def bandwidths(real):
    """[sigma0^2 * s for s in SCALES] as a fp64 device tensor: sigma0^2 = the mean squared distance between
    distinct rows of ``real`` [N, d], in closed form,  2 N / (N - 1) (mean |r|^2 - |mean r|^2), fp64."""
    r = real.double()
    N = r.shape[0]
    if N < 2:
        raise ValueError("bandwidths needs at least two points")
    s0 = 2.0 * N / (N - 1) * (r.square().sum(1).mean() - r.mean(0).square().sum())
    return s0 * torch.tensor(SCALES, dtype=torch.float64, device=real.device)


def self_sums(y, bw):
    """What two_sample keeps of a set against itself: (ksum [m, n_bw], nn_d2 [m]) with the pairs (i, i) left out.
    ``y`` must be the centred copy two_sample would make (center())."""
    ks, nd, _ = pairwise_stats(y, [y], bw, self_group=0)
    return ks[:, 0].clone(), nd[:, 0].clone()


def center(x, y):
    """(x - mean row of y, y - mean row of y) as fp32 copies: the distances do not change, the norms shrink and
    the fp32 inner product's error with them."""
    mu = y.double().mean(0).float()
    return x - mu, y - mu


def median(v):
    """The median along the last dimension, the mean of the two middle values for an even count (torch.median
    gives the lower one)."""
    s = v.sort(-1).values
    n = v.shape[-1]
    return 0.5 * (s[..., (n - 1) // 2] + s[..., n // 2])


def two_sample_device(xc, yc, bw, yy=None):
    """two_sample's numbers for centred sets as one flat fp64 device tensor:
    [mmd2 (n_bw), acc_x, acc_y, acc_all, nn_other mean, median, min, non-finite count]."""
    bw = [float(b) for b in bw]
    n, m, d = int(xc.shape[0]), int(yc.shape[0]), int(xc.shape[1])
    if n < 2 or m < 2:
        raise ValueError("two_sample needs at least two points per set")
    kx, dx, _ = pairwise_stats(xc, [xc, yc], bw, self_group=0)
    kyy, dyy = self_sums(yc, bw) if yy is None else yy
    _, dyx, _ = pairwise_stats(yc, [xc], [], ksum=False)  # the votes of y: the nearest x only
    mmd2 = kx[:, 0].sum(0) / (n * (n - 1.0)) + kyy.sum(0) / (m * (m - 1.0)) - 2.0 * kx[:, 1].sum(0) / (float(n) * m)
    cx = (dx[:, 0] < dx[:, 1]).double().sum()
    cy = (dyy < dyx[:, 0]).double().sum()
    rms = (dx[:, 1] / d).sqrt()
    bad = (~torch.isfinite(kx)).sum() + (~torch.isfinite(kyy)).sum() \
        + torch.isnan(dx).sum() + torch.isnan(dyy).sum() + torch.isnan(dyx).sum()
    return torch.cat([mmd2, torch.stack([cx / n, cy / m, (cx + cy) / (n + m), rms.mean(), median(rms), rms.min(),
                                         bad.double()])])


def unpack(row, n_bw=len(SCALES)):
    """two_sample's dict from two_sample_device's table as a host list."""
    mmd2 = [float(v) for v in row[:n_bw]]
    ax, ay, aa, mean, med, mn, bad = row[n_bw:n_bw + 7]
    return {"mmd2": mmd2, "mmd2_at_sigma0": mmd2[n_bw // 2], "nn_accuracy": {"x": ax, "y": ay, "all": aa},
            "nn_other": {"mean": mean, "median": med, "min": mn}, "nonfinite": int(bad)}


def two_sample(x, y, yy=None, bw=None):
    """{"mmd2": [5], "mmd2_at_sigma0", "nn_accuracy": {"x", "y", "all"}, "nn_other": {"mean", "median", "min"},
    "sigma0", "nonfinite"} for x [n, d] against y [m, d] (float32, one GPU, n, m >= 2), by the module docstring's
    definitions at the bandwidths bandwidths(y).  y's mean row is subtracted from both in copies; three
    pairwise_stats calls (x against {x itself, y}, y against itself, y against x), then a few fp64 torch
    reductions and one device -> host copy.  ``yy`` = self_sums(centred y, bw) of an earlier call with the same
    y reuses the y-against-y pass (``bw`` then names that call's bandwidths)."""
    xc, yc = center(x, y)
    if bw is None:
        bw = bandwidths(yc).tolist()
    row = two_sample_device(xc, yc, bw, yy=yy).cpu().tolist()
    rep = unpack(row, len(bw))
    rep["sigma0"] = float(bw[len(bw) // 2]) ** 0.5
    return rep


def _ks(ks, n, m):
    ks = [int(k) for k in ks]
    if not ks or len(ks) > KNN_MAX_RADII or any(k < 1 or k > KNN_MAX_K for k in ks):
        raise ValueError("manifold takes 1 to %d values of k in 1 .. %d, got %r" % (KNN_MAX_RADII, KNN_MAX_K, ks))
    if min(n, m) < max(ks) + 1:
        raise ValueError("manifold at k = %d needs %d points per set, got %d and %d" % (max(ks), max(ks) + 1, n, m))
    return ks


def self_radii(y, ks):
    """What manifold keeps of a set against itself: (r2 [m, len(ks)] fp64, the squared distance of every point to
    its k-th nearest other point for k in ``ks``, and the number of NaN distances met, a 0-dim int64 tensor).
    ``y`` must be the centred copy manifold would make (center())."""
    ks = _ks(ks, int(y.shape[0]), int(y.shape[0]))
    kd, _, nf = knn_stats(y, [y], max(ks), self_group=0)
    return kd[:, 0, [k - 1 for k in ks]].contiguous(), nf.sum()


def manifold_device(xc, yc, ks=(3, 5), yy=None):
    """manifold's numbers for centred sets as one flat fp64 device tensor: [precision (len(ks)), recall, density,
    coverage, non-finite count].  ``yy`` = self_radii(yc, ks) of an earlier call with the same y and ks reuses the
    y-against-y pass."""
    n, m = int(xc.shape[0]), int(yc.shape[0])
    ks = _ks(ks, n, m)
    col = [k - 1 for k in ks]
    ry, bad = self_radii(yc, ks) if yy is None else yy
    kx, ix, nx = knn_stats(xc, [xc, yc], max(ks), radii=[None, ry], self_group=0)
    rx = kx[:, 0, col].contiguous()
    ky, iy, ny = knn_stats(yc, [xc], 1, radii=[rx])
    kk = torch.tensor(ks, dtype=torch.float64, device=xc.device)
    hit = ix[:, 1].double()
    precision = (ix[:, 1] > 0).double().mean(0)
    density = hit.sum(0) / (kk * n)
    recall = (iy[:, 0] > 0).double().mean(0)
    coverage = (ky[:, 0, :1] <= ry).double().mean(0)
    bad = bad + nx.sum() + ny.sum()
    return torch.cat([precision, recall, density, coverage, bad.double().reshape(1)])


def unpack_manifold(row, ks):
    """manifold's dict from manifold_device's table as a host list."""
    nk = len(ks)
    return {"k": [int(k) for k in ks], "precision": [float(v) for v in row[:nk]],
            "recall": [float(v) for v in row[nk:2 * nk]], "density": [float(v) for v in row[2 * nk:3 * nk]],
            "coverage": [float(v) for v in row[3 * nk:4 * nk]], "nonfinite": int(row[4 * nk])}


def manifold(x, y, ks=(3, 5), yy=None):
    """{"k": [..], "precision": [..], "recall": [..], "density": [..], "coverage": [..], "nonfinite"} for the samples
    x [n, d] against the real points y [m, d] (float32, one GPU), one value per k in ``ks`` (at most KNN_MAX_RADII
    values in 1 .. KNN_MAX_K; every set needs max(ks) + 1 points), by the module docstring's definitions.  y's mean
    row is subtracted from both in copies; three knn_stats calls (y against itself; x against {x itself, y with
    y's radii}; y against x with x's radii), then a few fp64 torch reductions and one device -> host copy.
    "nonfinite" counts the NaN distances the three calls met: they enter no number.  ``yy`` = self_radii(centred
    y, ks) of an earlier call reuses the y-against-y pass."""
    xc, yc = center(x, y)
    ks = _ks(ks, int(x.shape[0]), int(y.shape[0]))
    return unpack_manifold(manifold_device(xc, yc, ks, yy=yy).cpu().tolist(), ks)
