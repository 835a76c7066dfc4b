"""numpy restatement of Philox4x32-10 and of svae_op_make_batch's contract (include/svae_hip.h), the
reference of tests/test_batch_pipeline.py, test_make_batch_gpu.py and test_trainer_gpu.py.

Words and thresholds are integer arithmetic.  u = (w + 0.5) 2^-32 and the angle 2 pi u are formed in
float32 as the kernel forms them; everything after is float64 (log, sqrt, cos, sin, the mix), so the
restatement carries none of the error of the device's fast fp32 transcendentals.  The uint8 dequantisation
exists twice: `target64` (exact, lo + u8 (hi - lo) / 255 in float64) and `target` (float32, each operation
rounded on its own as the kernel's, which the corrupted input is formed from)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (broadcast against each other)."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def threshold(p):
    """thr(p) = min(floor(p 2^32), 2^32 - 1) of the float32 probability the entry point receives."""
    return min(int(np.floor(float(np.float32(p)) * 4294967296.0)), MASK)


def words(n_elem, seed, offset, stream):
    """The word of every flat element e < n_elem from stream c2 = `stream`: group e // 4, lane e % 4."""
    G = (n_elem + 3) // 4
    ctr = [(int(offset) + g) & 0xFFFFFFFFFFFFFFFF for g in range(G)]
    lo = np.array([c & MASK for c in ctr], dtype=np.uint64)
    hi = np.array([c >> 32 for c in ctr], dtype=np.uint64)
    w = philox4x32_10(lo, hi, np.uint64(stream), np.uint64(0), int(seed) & MASK, (int(seed) >> 32) & MASK)
    return np.stack(w, axis=1).reshape(-1)[:n_elem]


def normals(n_elem, seed, offset):
    """float64 N(0,1) of every flat element: Box-Muller on words (0,1) and (2,3) of each group."""
    G = (n_elem + 3) // 4
    w = words(4 * G, seed, offset, 0).reshape(G, 4)
    # (float)w + 0.5f, then * 2^-32: two float32 roundings (the second is exact)
    u = (w.astype(np.float32) + np.float32(0.5)) * np.float32(2.3283064365386963e-10)
    ang = (np.float32(6.2831853) * u[:, [1, 3]]).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u[:, [0, 2]].astype(np.float64)))
    out = np.empty((G, 4), np.float64)
    out[:, 0], out[:, 1] = r[:, 0] * np.cos(ang[:, 0]), r[:, 0] * np.sin(ang[:, 0])
    out[:, 2], out[:, 3] = r[:, 1] * np.cos(ang[:, 1]), r[:, 1] * np.sin(ang[:, 1])
    return out.reshape(-1)[:n_elem]


def make_batch(data, idx, start, n, lo, hi, pepper, salt, scale, seed, offset):
    """dict(target64, target, unclipped, input): [n, per_image] arrays.  data [N, per_image] uint8 or
    float32; idx a list of rows or None (rows start .. start + n)."""
    data = np.asarray(data)
    data = data.reshape(data.shape[0], -1)
    rows = np.asarray(idx, dtype=np.int64) if idx is not None else np.arange(start, start + n)
    assert len(rows) == n
    x = data[rows]
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if data.dtype == np.uint8:
        t64 = float(lo32) + x.astype(np.float64) * ((float(hi32) - float(lo32)) / 255.0)
        qs = np.float32((float(hi32) - float(lo32)) / 255.0)
        t32 = lo32 + x.astype(np.float32) * qs  # numpy rounds the product, then the sum
    else:
        assert data.dtype == np.float32
        t64, t32 = x.astype(np.float64), x
    E = t32.size
    keep = (words(E, seed, offset, 1) >= np.uint64(threshold(pepper))).astype(np.float64).reshape(t32.shape)
    add = (words(E, seed, offset, 2) < np.uint64(threshold(salt))).astype(np.float64).reshape(t32.shape)
    v = t32.astype(np.float64) * keep + add
    if float(scale) != 0.0:
        v = v + float(np.float32(scale)) * normals(E, seed, offset).reshape(t32.shape)
    return dict(target64=t64, target=t32, unclipped=v, input=np.clip(v, float(lo32), float(hi32)))
