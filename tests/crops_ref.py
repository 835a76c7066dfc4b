"""numpy restatement of svae_op_crop_batch's contract (include/svae_hip.h), the reference of tests/test_crops_ref.py,
test_crop_batch_gpu.py and test_patch_trainer_gpu.py.  Philox is tests/batch_ref.py's.

Draws are integer arithmetic.  A uint8 block is summed as integers, divided once in float32 (numpy's float32
division is correctly rounded) and dequantised with the product and the sum each rounded to float32; a float32
block is summed in float32 from 0 in row-major order (p outside, q inside) and divided once.  The symmetry is the
index map of the contract written as an index map: nothing here is taken from the kernel."""
import numpy as np

import batch_ref as br

STREAM = 4
MASK = 0xFFFFFFFF


def _words(n, seed, offset, block):
    """[n, 4] Philox words of rows 0 .. n - 1: counter offset + b, c2 = 4, c3 = block."""
    ctr = [(int(offset) + b) & 0xFFFFFFFFFFFFFFFF for b in range(n)]
    lo = np.array([c & MASK for c in ctr], dtype=np.uint64)
    hi = np.array([c >> 32 for c in ctr], dtype=np.uint64)
    w = br.philox4x32_10(lo, hi, np.uint64(STREAM), np.uint64(block), int(seed) & MASK, (int(seed) >> 32) & MASK)
    return np.stack(w, axis=1)


def _mulhi(w, n):
    return (np.asarray(w, dtype=np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)


def draw(n, nimg, H, W, h, w, scales, symmetries, seed, offset):
    """[n, 5] int32 rows (m, s, g, y0, x0)."""
    a = _words(n, seed, offset, 0)
    b = _words(n, seed, offset, 1)
    sc = np.asarray(scales, dtype=np.int64)
    m = _mulhi(a[:, 0], nimg).astype(np.int64)
    s = sc[_mulhi(a[:, 1], len(sc)).astype(np.int64)]
    g = _mulhi(a[:, 2], symmetries).astype(np.int64)
    y0 = _mulhi(b[:, 0], H - s * h + 1).astype(np.int64)
    x0 = _mulhi(b[:, 1], W - s * w + 1).astype(np.int64)
    return np.stack([m, s, g, y0, x0], axis=1).astype(np.int32)


def block_means(img, s, y0, x0, h, w):
    """The [h, w, c] float32 means of the s x s blocks of the window at (y0, x0) of one image: qbar for uint8 (not
    yet dequantised), the value for float32."""
    win = img[y0:y0 + s * h, x0:x0 + s * w]
    assert win.shape[:2] == (s * h, s * w), "the window leaves the image"
    blk = win.reshape(h, s, w, s, -1)
    if img.dtype == np.uint8:
        total = blk.astype(np.int64).sum(axis=(1, 3))
        mean = total.astype(np.float32)
        return mean / np.float32(s * s) if s > 1 else mean
    assert img.dtype == np.float32
    if s == 1:
        return blk[:, 0, :, 0].copy()
    acc = np.zeros((h, w, blk.shape[-1]), np.float32)
    for p in range(s):
        for q in range(s):
            acc = acc + blk[:, p, :, q]  # float32 + float32: rounded once
    return acc / np.float32(s * s)


def symmetry(x, g):
    """out[i, j] = x[i', j'] with (i', j') = (j, i) if g & 4 else (i, j); i' <- h - 1 - i' if g & 2; j' <- w - 1 - j'
    if g & 1 (h, w: the extents of x, equal when g & 4)."""
    h, w = x.shape[:2]
    assert not (g & 4) or h == w
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ip, jp = (j, i) if g & 4 else (i, j)
    if g & 2:
        ip = h - 1 - ip
    if g & 1:
        jp = w - 1 - jp
    return x[ip, jp]


def crop_batch(images, h, w, scales=(1,), symmetries=1, seed=0, offset=0, n=1, lo=-1.0, hi=1.0, crops=None):
    """dict(target [n,h,w,c] float32, target_u8 (uint8 images only, else None), meta [n,5] int32)."""
    images = np.asarray(images)
    nimg, H, W, c = images.shape
    meta = np.asarray(crops, dtype=np.int32).reshape(n, 5) if crops is not None else \
        draw(n, nimg, H, W, h, w, scales, symmetries, seed, offset)
    u8 = images.dtype == np.uint8
    target = np.empty((n, h, w, c), np.float32)
    target_u8 = np.empty((n, h, w, c), np.uint8) if u8 else None
    lo32, hi32 = np.float32(lo), np.float32(hi)
    qs = np.float32((float(hi32) - float(lo32)) / 255.0)
    for b, (m, s, g, y0, x0) in enumerate(meta.tolist()):
        mean = symmetry(block_means(images[m], s, y0, x0, h, w), g)
        if u8:
            target[b] = lo32 + mean * qs  # numpy rounds the product, then the sum
            target_u8[b] = np.minimum(np.float32(255), np.rint(mean)).astype(np.uint8)  # rint: ties to even
        else:
            target[b] = mean
    return dict(target=target, target_u8=target_u8, meta=meta)
