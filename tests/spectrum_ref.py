"""numpy restatement of svae_op_power_spectrum (include/svae_hip.h), in the op's own order of operations.

Every product, sum and difference below is one numpy operation on float64 arrays, so each is rounded once and none
is fused; the sums run in explicit loops over xx, yy, v and u in the order the header states, and only the
independent (row, column) positions are vectorised.  The op's result is therefore expected bit for bit.
"""
import numpy as np


def multiplicity(w):
    m = np.full(w // 2 + 1, 2.0)
    m[0] = 1.0
    if w % 2 == 0:
        m[w // 2] = 1.0
    return m


def half_power(a, tw_y, tw_x):
    """P[v][u] (with the multiplicity) of one windowed fp64 plane a [h][w]: the row pass, then the column pass."""
    h, w = a.shape
    wu = w // 2 + 1
    u = np.arange(wu)
    tr, ti = np.zeros((h, wu)), np.zeros((h, wu))
    for xx in range(w):
        k = (u * xx) % w
        col = a[:, xx:xx + 1]
        tr = tr + col * tw_x[k, 0][None, :]
        ti = ti + col * tw_x[k, 1][None, :]
    v = np.arange(h)
    fr, fi = np.zeros((h, wu)), np.zeros((h, wu))
    for yy in range(h):
        k = (v * yy) % h
        c, s = tw_y[k, 0][:, None], tw_y[k, 1][:, None]
        row_r, row_i = tr[yy:yy + 1], ti[yy:yy + 1]
        pr = row_r * c - row_i * s
        pi = row_r * s + row_i * c
        fr = fr + pr
        fi = fi + pi
    return (fr * fr + fi * fi) * multiplicity(w)[None, :]


def bin_power(p, table, n_bins):
    """out[b] = sum_u (sum over ascending v with table[v][u] == b of p[v][u]), the outer sum over ascending u."""
    h, wu = p.shape
    part = np.zeros((wu, n_bins))
    cols = np.arange(wu)
    for v in range(h):
        b = table[v]
        keep = (b >= 0) & (b < n_bins)
        part[cols[keep], b[keep]] = part[cols[keep], b[keep]] + p[v, keep]  # one entry per column: no repeats
    out = np.zeros(n_bins)
    for u in range(wu):
        out = out + part[u]
    return out


def power_spectrum_ref(x, y, win_y, win_x, tw_y, tw_x, table, n_bins):
    """out [n][c][2][n_bins] (plane 1 NaN where y is None) and nonfinite [n][c] for fp32 x [n,h,w,c], y [ny,h,w,c]."""
    n, h, w, c = x.shape
    out = np.full((n, c, 2, n_bins), np.nan)
    bad = np.zeros((n, c), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            for k in range(c):
                xv = x[i, :, :, k]
                planes = [xv.astype(np.float64)]
                bad[i, k] = np.count_nonzero(~np.isfinite(xv))
                if y is not None:
                    yv = y[i % y.shape[0], :, :, k]
                    planes.append(xv.astype(np.float64) - yv.astype(np.float64))
                    bad[i, k] += np.count_nonzero(~np.isfinite(yv))
                for p, val in enumerate(planes):
                    a = (val * win_y[:, None]) * win_x[None, :]
                    out[i, k, p] = bin_power(half_power(a, tw_y, tw_x), table, n_bins)
    return out, bad
