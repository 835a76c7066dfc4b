"""Float64 restatement of svae_op_image_metrics' column table (include/svae_hip.h) with direct windowed sums,
and the bound a conforming implementation may differ from it by.

metrics_ref(x, y, data_range) -> (rows [n][4], bound [n][4]) for x [n,h,w,c] and y [ny,h,w,c] (image i against
image i % ny):  sum (x - y)^2,  sum |x - y|,  mean SSIM over the (h - 10)(w - 10) c valid positions,  the
non-finite count of the two images.  An image pair with a non-finite element gets NaN in columns 0 .. 2
(assert_rows then holds only its column 3).

The window is W[a][b] = g[a] g[b], g[k] = exp(-(k - 5)^2 / (2 1.5^2)) / sum, applied directly: 121 terms per
position and quantity, one vectorised pass per (a, b).  No separable pass, no convolution routine.

Bound.  u = 2^-53.  Any evaluation of an n-term sum in fp64 in which a term passes through at most k roundings
is within gamma_k sum |term| of the exact sum, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability, §4.2).

* Columns 0 and 1.  d = x - y of two fp32 values is one rounding in fp64, d^2 enters through an fma or one more
  rounding, and the sum over the N = h w c elements adds at most N - 1 roundings in any order: gamma_{N+1}.  The
  reference sums with math.fsum (one rounding).  Held to (N + 2) 2^-52 sum |term|, twice gamma_{N+2}, as
  tests/stats_ref.py does.
* One window sum S = sum_ab W_ab q_ab (q = x, y, x^2, y^2 or x y; products of fp32 values are exact in fp64).
  Implementation: each 1-D weight is the rounded quotient of a rounded exp and a rounded 11-term sum, within
  8 u relative, so the pair g[a] g[b] carries 16 u; a separable evaluation sends every term through 11 roundings
  of the horizontal chain and 11 of the vertical one (a direct one through 121): at most gamma_38 A for the
  separable form, A = sum_ab W_ab |q_ab|.  Reference (this file): the same 16 u on the weights, one rounding each
  for W_ab and W_ab q_ab, 120 roundings of the running sum: gamma_138 A.  Together |S_impl - S_ref| <=
  KSUM u A with KSUM = 192 (> 38 + 138, with room for the 1 / (1 - k u) factors).
* Through SSIM, first order kept exactly and second-order products kept as written; r = 4 u covers the
  roundings of one product or sum on both sides.  With e_m = KSUM u A_x etc.:
    var = S_xx - mu^2      e_var = e_xx + (2 |mu| + e_m) e_m + r (|S_xx| + mu^2)
    cov = S_xy - mu_x mu_y e_cov = e_xy + |mu_x| e_my + |mu_y| e_mx + e_mx e_my + r (|S_xy| + |mu_x mu_y|)
    A1 = 2 mu_x mu_y + C1  e_A1 = 2 (|mu_x| e_my + |mu_y| e_mx + e_mx e_my) + r (|2 mu_x mu_y| + C1)
    A2 = 2 cov + C2        e_A2 = 2 e_cov + r (|2 cov| + C2)
    B1 = mu_x^2 + mu_y^2 + C1 (>= C1)   e_B1 = (2 |mu_x| + e_mx) e_mx + (2 |mu_y| + e_my) e_my + 2 r B1
    B2 = var_x + var_y + C2             e_B2 = e_varx + e_vary + r (|var_x| + |var_y| + C2)
    num = A1 A2   e_num = |A1| e_A2 + |A2| e_A1 + e_A1 e_A2 + r |num|
    den = B1 B2   e_den = B1 e_B2 + B2 e_B1 + e_B1 e_B2 + r den
    Q = num / den: |num'/den' - num/den| = |(num' - num) den - num (den' - den)| / (den den')
                   <= (e_num + |Q| e_den) / (den - e_den), plus r |Q| for the division; e_den < den / 2 is asserted.
  This is where C2 = (0.03 L)^2 enters: a flat window has var near 0, so e_Q is about KSUM u A / C2, near 1e-11 for
  data in [-1, 1] and L = 2.
* The mean over the P = (h - 10)(w - 10) c positions: the reference uses math.fsum; an implementation adds P terms
  in some order, gamma_{P-1} sum |Q|, and divides: bound = mean e_Q + (P + 2) u mean |Q|.
"""
import math

import numpy as np

WINDOW, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
COLS = 4
U = 2.0 ** -53
KSUM = 192.0
R = 4.0 * U


def gaussian_window():
    k = np.arange(WINDOW, dtype=np.float64) - WINDOW // 2
    g = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def _window_sums(q, vh, vw):
    """sum_ab W_ab q[.., a:a+vh, b:b+vw, :] of q [n,h,w,c] and the same of |q|, term by term."""
    g = gaussian_window()
    s = np.zeros(q.shape[:1] + (vh, vw) + q.shape[3:], dtype=np.float64)
    a_ = np.zeros_like(s)
    for a in range(WINDOW):
        for b in range(WINDOW):
            wab = g[a] * g[b]
            t = wab * q[:, a:a + vh, b:b + vw, :]
            s += t
            a_ += np.abs(t)
    return s, a_


def ssim_map(x, y, data_range):
    """(Q, e_Q) [n, h-10, w-10, c] for float64 arrays x, y [n,h,w,c]: the SSIM of every valid window position
    and its error bound (module docstring)."""
    vh, vw = x.shape[1] - (WINDOW - 1), x.shape[2] - (WINDOW - 1)
    L = float(data_range)
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
    mx, ax = _window_sums(x, vh, vw)
    my, ay = _window_sums(y, vh, vw)
    sxx, _ = _window_sums(x * x, vh, vw)
    syy, _ = _window_sums(y * y, vh, vw)
    sxy, axy = _window_sums(x * y, vh, vw)
    ku = KSUM * U
    e_mx, e_my, e_xx, e_yy, e_xy = ku * ax, ku * ay, ku * sxx, ku * syy, ku * axy
    amx, amy = np.abs(mx), np.abs(my)
    vx, vy, cxy = sxx - mx * mx, syy - my * my, sxy - mx * my
    e_vx = e_xx + (2 * amx + e_mx) * e_mx + R * (np.abs(sxx) + mx * mx)
    e_vy = e_yy + (2 * amy + e_my) * e_my + R * (np.abs(syy) + my * my)
    e_cxy = e_xy + amx * e_my + amy * e_mx + e_mx * e_my + R * (np.abs(sxy) + amx * amy)
    a1 = 2 * mx * my + c1
    a2 = 2 * cxy + c2
    b1 = mx * mx + my * my + c1
    b2 = vx + vy + c2
    e_a1 = 2 * (amx * e_my + amy * e_mx + e_mx * e_my) + R * (2 * amx * amy + c1)
    e_a2 = 2 * e_cxy + R * (np.abs(2 * cxy) + c2)
    e_b1 = (2 * amx + e_mx) * e_mx + (2 * amy + e_my) * e_my + 2 * R * b1
    e_b2 = e_vx + e_vy + R * (np.abs(vx) + np.abs(vy) + c2)
    num, den = a1 * a2, b1 * b2
    e_num = np.abs(a1) * e_a2 + np.abs(a2) * e_a1 + e_a1 * e_a2 + R * np.abs(num)
    e_den = b1 * e_b2 + b2 * e_b1 + e_b1 * e_b2 + R * den
    assert np.all(e_den < 0.5 * den), "the denominator's error bound must stay below half of it"
    q = num / den
    e_q = (e_num + np.abs(q) * e_den) / (den - e_den) + R * np.abs(q)
    return q, e_q


def metrics_ref(x, y, data_range):
    """(rows [n][4], bound [n][4]); x [n,h,w,c], y [ny,h,w,c] float32, n a multiple of ny."""
    x = np.asarray(x, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    n, ny = x.shape[0], y.shape[0]
    assert x.ndim == 4 and x.shape[1:] == y.shape[1:] and n % ny == 0
    assert x.shape[1] >= WINDOW and x.shape[2] >= WINDOW
    yy = y[np.arange(n) % ny]
    rows = np.zeros((n, COLS), dtype=np.float64)
    bound = np.zeros_like(rows)
    rows[:, 3] = (~np.isfinite(x)).reshape(n, -1).sum(1) + (~np.isfinite(yy)).reshape(n, -1).sum(1)
    ok = rows[:, 3] == 0
    rows[~ok, :3] = np.nan
    bound[~ok, :3] = np.nan
    if not ok.any():
        return rows, bound
    xd, yd = x[ok].astype(np.float64), yy[ok].astype(np.float64)
    q, e_q = ssim_map(xd, yd, data_range)
    per = xd[0].size
    for j, i in enumerate(np.flatnonzero(ok)):
        d = (xd[j] - yd[j]).ravel()
        for col, t in ((0, d * d), (1, np.abs(d))):
            rows[i, col] = math.fsum(t.tolist())
            bound[i, col] = (per + 2) * 2.0 ** -52 * rows[i, col]
        p = q[j].size
        rows[i, 2] = math.fsum(q[j].ravel().tolist()) / p
        bound[i, 2] = (math.fsum(e_q[j].ravel().tolist()) + (p + 2) * U * math.fsum(np.abs(q[j]).ravel().tolist())) / p
    return rows, bound


def psnr_ref(sse, n_elem, data_range, sse_bound=0.0):
    """(10 log10(L^2 n_elem / sse), bound): d psnr = 10 / ln 10 * d arg / arg, where the argument carries
    sse_bound / sse and 8 * 2^-52 for its products and quotients on either side, plus 8 * 2^-52 |psnr| for a
    logarithm good to a few units in the last place on either side.  (+inf, 0) at sse = 0."""
    if sse == 0.0:
        return math.inf, 0.0
    v = 10.0 * math.log10(float(data_range) ** 2 * n_elem / sse)
    return v, 10.0 / math.log(10.0) * (sse_bound / sse + 8 * 2.0 ** -52) + 8 * 2.0 ** -52 * abs(v)


def assert_rows(got, want, bound, what=""):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, 3], want[:, 3]), "%s: non-finite counts %s, want %s" % (what, got[:, 3], want[:, 3])
    ok = want[:, 3] == 0
    err = np.abs(got[ok, :3] - want[ok, :3])
    bad = np.argwhere(~(err <= bound[ok, :3]))
    assert bad.size == 0, "%s: (finite row, column) %s: got %r want %r bound %r" % (
        what, bad[0].tolist(), got[ok][tuple(bad[0])], want[ok][tuple(bad[0])], bound[ok][tuple(bad[0])])
