"""numpy restatement of svae_op_jpeg_batch's contract (include/svae_hip.h), the reference of tests/test_jpeg_ref.py,
test_jpeg_batch_gpu.py and test_jpeg_trainer_gpu.py.  Philox and the thresholds are tests/batch_ref.py's.

Draws and the quantisation tables are integer arithmetic.  Two modes:

  "fp32"  every product, sum and division rounded to float32 in the order the contract states: what the kernel must
          return bit for bit.
  "fp64"  the same mathematics in float64 (the constants are still the contract's float32 ones).

The tables and constants are the JPEG standard's (Annex K, JFIF's BT.601 matrix) and IJG's published quality scaling.
"""
import numpy as np

from batch_ref import MASK, philox4x32_10, threshold

STREAM = 5

LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64).reshape(8, 8)

# 1 / sqrt(8), then cos(m pi / 16) / 2 for m = 1 .. 7: the literals of the contract
MAGNITUDES = ("0.353553391", "0.490392640", "0.461939766", "0.415734806", "0.353553391", "0.277785117",
              "0.191341716", "0.0975451610")


def dct_matrix(dt=np.float32):
    """C[u][x] from the eight float32 magnitudes, the angle folded into the first octant."""
    mag = [np.float32(m) for m in MAGNITUDES]
    C = np.empty((8, 8), np.float32)
    for u in range(8):
        for x in range(8):
            if u == 0:
                C[u, x] = mag[0]
                continue
            m = ((2 * x + 1) * u) % 32
            if m > 16:
                m = 32 - m
            neg = m > 8
            if neg:
                m = 16 - m
            C[u, x] = -mag[m] if neg else mag[m]
    return C.astype(dt)


def quant_table(base, q):
    """IJG's scaling of a base table, all integer."""
    q = int(q)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def image_words(n, seed, offset):
    """[n, 4] uint64: the words of stream c2 = 5, c3 = 0 for images 0 .. n - 1 (counter offset + b)."""
    ctr = [(int(offset) + b) & 0xFFFFFFFFFFFFFFFF for b in range(n)]
    lo = np.array([c & MASK for c in ctr], dtype=np.uint64)
    hi = np.array([c >> 32 for c in ctr], dtype=np.uint64)
    w = philox4x32_10(lo, hi, np.uint64(STREAM), np.uint64(0), int(seed) & MASK, (int(seed) >> 32) & MASK)
    return np.stack(w, axis=1)


def draws(n, p, q_lo, q_hi, seed, offset):
    """[n] int32: the quality of every image, 0 where it is not compressed."""
    w = image_words(n, seed, offset)
    thr, span = threshold(p), int(q_hi) - int(q_lo) + 1
    return np.array([int(q_lo) + ((int(a[1]) * span) >> 32) if int(a[0]) < thr else 0 for a in w], dtype=np.int32)


def _level(v):
    return np.clip(np.rint(v), 0, 255)


def _blocks(plane, dt):
    """[h, w] -> [H/8, W/8, 8, 8] after replicating the last row and column up to multiples of 8, less 128."""
    h, w = plane.shape
    H, W = -(-h // 8) * 8, -(-w // 8) * 8
    ext = plane[np.minimum(np.arange(H), h - 1)][:, np.minimum(np.arange(W), w - 1)]
    f = (ext - dt(128)).astype(dt)
    return f.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b, h, w):
    nby, nbx = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nby * 8, nbx * 8)[:h, :w]


def _codec_plane(plane, T, C, dt):
    """Steps 4 - 6 on one plane [h, w] in dtype dt with the integer table T [8, 8] (indexed [v][u])."""
    h, w = plane.shape
    f = _blocks(plane, dt)                                   # [.., y, x]
    Tf = T.astype(dt)
    # row pass: t[y][u] = sum_x f[y][x] C[u][x]
    t = np.zeros(f.shape, dt)
    for x in range(8):
        t = (t + (f[..., :, x, None] * C[None, :, x]).astype(dt)).astype(dt)
    # column pass: F[v][u] = sum_y C[v][y] t[y][u]
    F = np.zeros(f.shape, dt)
    for y in range(8):
        F = (F + (C[:, y, None] * t[..., y, None, :]).astype(dt)).astype(dt)
    G = (np.rint((F / Tf).astype(dt)) * Tf).astype(dt)
    # inverse column pass: s[y][u] = sum_v C[v][y] G[v][u]
    s = np.zeros(f.shape, dt)
    for v in range(8):
        s = (s + (C[v, :, None] * G[..., v, None, :]).astype(dt)).astype(dt)
    # inverse row pass: g[y][x] = sum_u s[y][u] C[u][x]
    g = np.zeros(f.shape, dt)
    for u in range(8):
        g = (g + (s[..., :, u, None] * C[None, u, :]).astype(dt)).astype(dt)
    return _unblocks(_level((g + dt(128)).astype(dt)).astype(dt), h, w)


def _chroma_means(plane, dt):
    """ceil(h/2) x ceil(w/2) means of the in-image pixels of every 2 x 2 block: sequential adds, one division."""
    h, w = plane.shape
    out = np.empty((-(-h // 2), -(-w // 2)), dt)
    for ci in range(out.shape[0]):
        for cj in range(out.shape[1]):
            blk = plane[2 * ci:2 * ci + 2, 2 * cj:2 * cj + 2]
            acc = dt(0)
            for v in blk.reshape(-1):
                acc = dt(acc + v)
            out[ci, cj] = dt(acc / dt(blk.size))
    return out


def codec(L, q, subsample, dt=np.float32):
    """Steps 2 - 8 on the levels L [h, w, c] (whole numbers in 0 .. 255, dtype dt): the decoded levels."""
    h, w, c = L.shape
    C = dct_matrix(dt)
    Tl, Tc = quant_table(LUMA, q), quant_table(CHROMA, q)
    k = lambda s: dt(np.float32(s))
    if c == 1:
        return _codec_plane(L[:, :, 0], Tl, C, dt)[:, :, None]
    R, G, B = L[:, :, 0], L[:, :, 1], L[:, :, 2]
    Y = _level(k("0.299") * R + k("0.587") * G + k("0.114") * B).astype(dt)
    Cb = _level(dt(128) - k("0.168735892") * R - k("0.331264108") * G + k("0.5") * B).astype(dt)
    Cr = _level(dt(128) + k("0.5") * R - k("0.418687589") * G - k("0.081312411") * B).astype(dt)
    if subsample == 2:
        Cb, Cr = _chroma_means(Cb, dt), _chroma_means(Cr, dt)
    Y, Cb, Cr = _codec_plane(Y, Tl, C, dt), _codec_plane(Cb, Tc, C, dt), _codec_plane(Cr, Tc, C, dt)
    if subsample == 2:
        ii, jj = np.arange(h) // 2, np.arange(w) // 2
        Cb, Cr = Cb[ii][:, jj], Cr[ii][:, jj]
    db, dr = (Cb - dt(128)).astype(dt), (Cr - dt(128)).astype(dt)
    out = np.empty((h, w, 3), dt)
    out[:, :, 0] = _level(Y + k("1.402") * dr)
    out[:, :, 1] = _level(Y - k("0.344136286") * db - k("0.714136286") * dr)
    out[:, :, 2] = _level(Y + k("1.772") * db)
    return out


def jpeg_batch(x, p, q_lo, q_hi, subsample, lo, hi, seed, offset, mode="fp32"):
    """dict(out [n,h,w,c] in the mode's dtype, quality [n] int32, levels [n,h,w,c] (the decoded levels; the input's
    own levels where an image was not compressed)).  x: float32 [n,h,w,c]."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[3] in (1, 3) and mode in ("fp64", "fp32")
    dt = np.float64 if mode == "fp64" else np.float32
    n = x.shape[0]
    lo32, hi32 = np.float32(lo), np.float32(hi)
    span = float(hi32) - float(lo32)
    if mode == "fp32":
        qinv, qscale = np.float32(255.0 / span), np.float32(span / 255.0)
    else:
        qinv, qscale = 255.0 / span, span / 255.0
    quality = draws(n, p, q_lo, q_hi, seed, offset)
    out = x.astype(dt)
    levels = _level(((x.astype(dt) - dt(lo32)).astype(dt) * qinv).astype(dt)).astype(dt)
    for b in range(n):
        if quality[b] == 0:
            continue
        with np.errstate(invalid="ignore"):
            levels[b] = codec(levels[b], int(quality[b]), subsample if x.shape[3] == 3 else 1, dt)
        out[b] = (dt(lo32) + (levels[b] * qscale).astype(dt)).astype(dt)
    return dict(out=out, quality=quality, levels=levels)
