"""Float64 restatement of svae_op_tensor_stats' column table (include/svae_hip.h), exactly rounded.

For every segment and y = clamp(x, -c, +c): the finite count, sum y, sum |y|, sum y^2, max |x| over the finite
elements, the count of finite |x| > c, the non-finite count, 0.  The sums go through math.fsum, so the
reference carries one rounding in all.  An fp32 value and the square of one are exact in float64.

bounds(): what the kernel may differ by.  It adds n fp64 terms with one rounding per addition, so
|got - want| <= n * 2^-52 * sum |term| for the three sums (the standard bound (n - 1) u sum |term| with
u = 2^-53, and room for the reference's own rounding); the counts and the maximum are exact.
"""
import math

import numpy as np

COLS = 8


def stats_ref(x, offsets, lengths, c):
    """(rows [n_seg][8], bound [n_seg][8]) for a float32 array x."""
    x = np.asarray(x, dtype=np.float32)
    rows = np.zeros((len(offsets), COLS), dtype=np.float64)
    bound = np.zeros_like(rows)
    for s, (o, n) in enumerate(zip(offsets, lengths)):
        v = x[o:o + n]
        fin = np.isfinite(v)
        f = v[fin].astype(np.float64)
        y = np.clip(f, -c, c) if c != math.inf else f
        terms = (y, np.abs(y), y * y)
        rows[s, 0] = f.size
        for q, t in enumerate(terms):
            rows[s, 1 + q] = math.fsum(t.tolist())
            bound[s, 1 + q] = f.size * 2.0 ** -52 * math.fsum(np.abs(t).tolist())
        rows[s, 4] = np.abs(f).max() if f.size else 0.0
        rows[s, 5] = np.count_nonzero(np.abs(f) > c)
        rows[s, 6] = n - f.size
    return rows, bound


def assert_rows(got, want, bound, what=""):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, "%s: (segment, column) %s: got %r want %r bound %r" % (
        what, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], bound[tuple(bad[0])])
