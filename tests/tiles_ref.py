"""numpy restatement of svae_op_extract_tiles and svae_op_blend_tiles (include/svae_hip.h): the geometry in
integers, the dequantisation in fp32 with separate roundings, the blend in float64 in the stated order with one
division and one cast, the quantiser in fp32.  Written for clarity, pixel by pixel where the order matters; the
covering tiles are found by enumeration, not by the closed form the kernel uses."""
import numpy as np


def count(L, t, s):
    """k = ceil((L - t) / s) + 1"""
    assert 1 <= s <= t <= L
    return -((t - L) // s) + 1


def origins(L, t, s):
    return [min(i * s, L - t) for i in range(count(L, t, s))]


def w1(p, t):
    return min(p + 1, t - p)


def covering(x, L, t, s):
    """Indices of the tiles that cover position x, ascending."""
    return [i for i, o in enumerate(origins(L, t, s)) if o <= x < o + t]


def n_tiles(nimg, H, W, th, tw, sy, sx):
    return nimg * count(H, th, sy) * count(W, tw, sx)


def tile_of(tid, nimg, H, W, th, tw, sy, sx):
    """(m, oy, ox) of tile id tid."""
    ky, kx = count(H, th, sy), count(W, tw, sx)
    m, rest = divmod(tid, ky * kx)
    i, j = divmod(rest, kx)
    return m, origins(H, th, sy)[i], origins(W, tw, sx)[j]


def dequant(q, lo, hi):
    """lo + q * ((hi - lo) / 255): the constant, the product and the sum each rounded to fp32."""
    qscale = np.float32((float(hi) - float(lo)) / 255.0)
    p = (np.asarray(q).astype(np.float32) * qscale).astype(np.float32)
    return (np.float32(lo) + p).astype(np.float32)


def quant(v, lo, hi):
    """(uint8) min(max(rint((v - lo) * (255 / (hi - lo))), 0), 255) in fp32, every operation rounded on its own."""
    qinv = np.float32(255.0 / (float(hi) - float(lo)))
    d = (np.asarray(v, dtype=np.float32) - np.float32(lo)).astype(np.float32)
    r = np.rint((d * qinv).astype(np.float32))
    return np.minimum(np.maximum(r, np.float32(0)), np.float32(255)).astype(np.uint8)


def as_float(images, lo, hi):
    return dequant(images, lo, hi) if images.dtype == np.uint8 else images.astype(np.float32)


def extract(images, th, tw, sy, sx, lo=-1.0, hi=1.0, first=0, cnt=None):
    """tiles [cnt, th, tw, c] fp32: row r is tile (first + r) mod n_tiles."""
    nimg, H, W, c = images.shape
    n = n_tiles(nimg, H, W, th, tw, sy, sx)
    cnt = n if cnt is None else cnt
    x = as_float(images, lo, hi)
    out = np.empty((cnt, th, tw, c), np.float32)
    for r in range(cnt):
        m, oy, ox = tile_of((first + r) % n, nimg, H, W, th, tw, sy, sx)
        out[r] = x[m, oy:oy + th, ox:ox + tw]
    return out


def blend(tiles, nimg, H, W, c, th, tw, sy, sx, source=None, known=None, lo=-1.0, hi=1.0):
    """tiles [nstack, n_tiles, th, tw, c] -> (out fp32, out_u8), both [nstack, nimg, H, W, c]."""
    nstack = tiles.shape[0]
    ky, kx = count(H, th, sy), count(W, tw, sx)
    oy, ox = origins(H, th, sy), origins(W, tw, sx)
    assert tiles.shape[1:] == (nimg * ky * kx, th, tw, c)
    t64 = tiles.astype(np.float64)
    out = np.empty((nstack, nimg, H, W, c), np.float32)
    cov_y = [covering(y, H, th, sy) for y in range(H)]
    cov_x = [covering(x, W, tw, sx) for x in range(W)]
    for y in range(H):
        for x in range(W):
            acc = np.zeros((nstack, nimg, c), np.float64)
            wsum = 0
            for i in cov_y[y]:
                for j in cov_x[x]:
                    w = w1(y - oy[i], th) * w1(x - ox[j], tw)
                    ids = (np.arange(nimg) * ky + i) * kx + j
                    acc = acc + np.float64(w) * t64[:, ids, y - oy[i], x - ox[j], :]
                    wsum += w
            out[:, :, y, x, :] = (acc / np.float64(wsum)).astype(np.float32)
    if known is not None:
        src = as_float(source, lo, hi)
        k = np.asarray(known).astype(bool)
        out[:, k] = src[k]
    return out, quant(out, lo, hi)
