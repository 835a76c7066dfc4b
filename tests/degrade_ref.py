"""numpy restatement of svae_op_degrade_batch's contract (include/svae_hip.h), the reference of
tests/test_degrade_ref.py, test_degrade_gpu.py and test_degrade_trainer_gpu.py.  Philox, the thresholds and the
pixel noise are tests/batch_ref.py's.

Draws and box geometry are integer arithmetic; sigma and the tap radius are formed in float32 as the kernel forms
them.  Two modes:

  "fp64"  the truth: weights, both blur passes, the block means and the pixel noise in float64.
  "fp32"  every product, sum and division rounded to float32 in the order the contract states (blur, block means);
          the pixel noise as batch_ref.make_batch forms it from a float32 batch.  Without blur this mode is what the
          kernel must return bit for bit (with gaussian_scale = 0: the kernel's normals are fast fp32 ones).
"""
from collections import namedtuple

import numpy as np

import batch_ref
from batch_ref import MASK, philox4x32_10, threshold

Spec = namedtuple("Spec", "p_blur sigma_lo sigma_hi p_down factor p_cut boxes min_side max_side fill "
                          "pepper_prob salt_prob gaussian_scale")
IDENTITY = Spec(0.0, 0.0, 0.0, 0.0, 1, 0.0, 0, 1, 1, 0.0, 0.0, 0.0, 0.0)
RMAX = 12


def image_words(n, seed, offset, block):
    """[n, 4] uint64: the words of stream c2 = 3, c3 = `block` for images 0 .. n - 1 (counter offset + b)."""
    ctr = [(int(offset) + b) & 0xFFFFFFFFFFFFFFFF for b in range(n)]
    lo = np.array([c & MASK for c in ctr], dtype=np.uint64)
    hi = np.array([c >> 32 for c in ctr], dtype=np.uint64)
    w = philox4x32_10(lo, hi, np.uint64(3), np.uint64(block), int(seed) & MASK, (int(seed) >> 32) & MASK)
    return np.stack(w, axis=1)


def image_counters(n, offset):
    """The 64-bit counters the images of one call draw under."""
    return [(int(offset) + b) & 0xFFFFFFFFFFFFFFFF for b in range(n)]


def draws(n, h, w, spec, seed, offset):
    """Per image: dict(blur, sigma (float32), r, down, cut, boxes [(y0, x0, bh, bw)] * spec.boxes)."""
    a = image_words(n, seed, offset, 0)
    bx = [image_words(n, seed, offset, 1 + k) for k in range(spec.boxes)]
    s_lo, s_hi = np.float32(spec.sigma_lo), np.float32(spec.sigma_hi)
    span = int(spec.max_side) - int(spec.min_side) + 1
    out = []
    for b in range(n):
        a0, a1, a2, a3 = (int(v) for v in a[b])
        u = np.float32(a1 >> 8) * np.float32(2.0 ** -24)
        sigma = np.float32(s_lo + np.float32(u * np.float32(s_hi - s_lo)))
        blur = a0 < threshold(spec.p_blur)
        r = min(int(np.ceil(np.float32(3.0) * sigma)), RMAX) if blur else 0
        boxes = []
        for k in range(spec.boxes):
            b0, b1, b2, b3 = (int(v) for v in bx[k][b])
            bh = min(h, spec.min_side + ((b0 * span) >> 32))
            bw = min(w, spec.min_side + ((b1 * span) >> 32))
            boxes.append(((b2 * (h - bh + 1)) >> 32, (b3 * (w - bw + 1)) >> 32, bh, bw))
        out.append(dict(blur=blur, sigma=sigma, r=r, down=a2 < threshold(spec.p_down) and spec.factor > 1,
                        cut=a3 < threshold(spec.p_cut) and spec.boxes > 0, boxes=boxes))
    return out


def weights(sigma, r, dt):
    """w_0 .. w_r in dtype dt (float32: every operation rounded as the kernel's, numpy's exp for expf)."""
    sigma = dt(sigma)
    den = dt(2.0) * sigma * sigma
    g = [dt(1.0)]
    s = dt(0.0)
    with np.errstate(divide="ignore"):
        for k in range(1, r + 1):
            g.append(dt(np.exp(dt(-dt(k * k) / den))))
            s = dt(s + g[k])
    norm = dt(dt(1.0) + dt(dt(2.0) * s))
    return [dt(v / norm) for v in g]


def _pass(x, wt, r, axis, dt):
    """sum_{k=-r..r} w_|k| x[clamp(i + k)] along `axis`, from 0 in ascending k, in dtype dt."""
    n = x.shape[axis]
    idx = np.arange(n)
    acc = np.zeros(x.shape, dt)
    for k in range(-r, r + 1):
        tap = np.take(x, np.clip(idx + k, 0, n - 1), axis=axis)
        acc = (acc + (wt[abs(k)] * tap).astype(dt)).astype(dt)
    return acc


def blur(img, sigma, r, dt):
    """img [h, w, c] in dt: horizontal pass, then vertical pass."""
    if r == 0:
        return img
    wt = weights(sigma, r, dt)
    return _pass(_pass(img, wt, r, 1, dt), wt, r, 0, dt)


def downsample(img, f, dt):
    """Block means of img [h, w, c]: sequential adds from 0 in row-major order, one division by the count."""
    h, w, _ = img.shape
    out = np.empty(img.shape, dt)
    for i0 in range(0, h, f):
        for j0 in range(0, w, f):
            blk = img[i0:i0 + f, j0:j0 + f]
            acc = np.zeros(img.shape[2], dt)
            for ii in range(blk.shape[0]):
                for jj in range(blk.shape[1]):
                    acc = (acc + blk[ii, jj]).astype(dt)
            out[i0:i0 + f, j0:j0 + f] = (acc / dt(blk.shape[0] * blk.shape[1])).astype(dt)
    return out


def box_mask(h, w, boxes):
    m = np.zeros((h, w), bool)
    for y0, x0, bh, bw in boxes:
        m[y0:y0 + bh, x0:x0 + bw] = True
    return m


def pixel_noise(x, lo, hi, spec, seed, offset):
    """batch_ref.make_batch's corruption of the [n, per_image] batch x, in float64: make_batch itself on a float32
    batch, the same expressions on a float64 one (which make_batch does not take)."""
    if x.dtype == np.float32:
        return batch_ref.make_batch(x, None, 0, x.shape[0], lo, hi, spec.pepper_prob, spec.salt_prob,
                                    spec.gaussian_scale, seed, offset)["input"]
    lo32, hi32 = np.float32(lo), np.float32(hi)
    E = x.size
    keep = (batch_ref.words(E, seed, offset, 1) >= np.uint64(threshold(spec.pepper_prob))).astype(np.float64)
    add = (batch_ref.words(E, seed, offset, 2) < np.uint64(threshold(spec.salt_prob))).astype(np.float64)
    v = x.astype(np.float64) * keep.reshape(x.shape) + add.reshape(x.shape)
    if float(spec.gaussian_scale) != 0.0:
        v = v + float(np.float32(spec.gaussian_scale)) * batch_ref.normals(E, seed, offset).reshape(x.shape)
    return np.clip(v, float(lo32), float(hi32))


def degrade(target, spec, lo, hi, seed, offset, mode="fp64"):
    """dict(input [n,h,w,c] float64, mask [n,h,w] float32, structured (the batch before the pixel noise, in the
    mode's dtype), draws).  target: float32 [n,h,w,c]."""
    target = np.asarray(target)
    assert target.dtype == np.float32 and target.ndim == 4 and mode in ("fp64", "fp32")
    dt = np.float64 if mode == "fp64" else np.float32
    n, h, w, c = target.shape
    d = draws(n, h, w, spec, seed, offset)
    out = np.empty(target.shape, dt)
    mask = np.zeros((n, h, w), np.float32)
    for b in range(n):
        img = blur(target[b].astype(dt), d[b]["sigma"], d[b]["r"], dt)
        if d[b]["down"]:
            img = downsample(img, spec.factor, dt)
        if d[b]["cut"]:
            m = box_mask(h, w, d[b]["boxes"])
            img = np.where(m[:, :, None], dt(np.float32(spec.fill)), img)
            mask[b] = m
        out[b] = img
    inp = pixel_noise(out.reshape(n, -1), lo, hi, spec, seed, offset).reshape(target.shape)
    return dict(input=inp, mask=mask, structured=out, draws=d)
