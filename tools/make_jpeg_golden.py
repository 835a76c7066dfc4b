"""Write tests/golden/jpeg/jpeg_libjpeg.npz: a few small uint8 images and what libjpeg (through PIL) decodes after
compressing them, the outside evidence tests/test_jpeg_ref.py holds the contract of svae_op_jpeg_batch to.

    python tools/make_jpeg_golden.py [--out tests/golden/jpeg/jpeg_libjpeg.npz]

Cases: (64,64,3) and (13,21,3) RGB at subsampling=0 (4:4:4) and (28,28,1) grey, each at quality 10, 30, 50, 75, 90
and 100.  The inputs are smooth images (a few low-frequency waves per channel) plus mild noise, generated from a
seed: not white noise, which no codec is meant for.  4:2:0 is left out on purpose: libjpeg's chroma down- and
up-sampling filters differ from the contract's block means and replication by design.

Keys: "in_<name>" uint8 [h,w,c]; "out_<name>_q<Q>" uint8 [h,w,c].  PIL is needed here only, never by the library.
"""
import argparse
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"rgb64": (64, 64, 3), "rgb13x21": (13, 21, 3), "grey28": (28, 28, 1)}
QUALITIES = (10, 30, 50, 75, 90, 100)


def make_input(name):
    """The uint8 image of a case: per channel a sum of three low-frequency waves, plus Gaussian noise of 3 levels."""
    h, w, c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20240)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, c), np.float64)
    for ch in range(c):
        v = np.zeros((h, w))
        for _ in range(3):
            fy, fx = rng.uniform(0.2, 2.5, size=2)
            ph = rng.uniform(0, 2 * np.pi, size=2)
            v += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * fy * yy / h + ph[0]) * np.cos(2 * np.pi * fx * xx / w + ph[1])
        img[:, :, ch] = 128 + 100 * v / max(np.abs(v).max(), 1e-9) * 0.9
    img += rng.normal(0, 3.0, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def libjpeg_round_trip(img, quality):
    """Decoded output of PIL's JPEG encoder at `quality`, 4:4:4, for a uint8 [h,w,c] image."""
    from PIL import Image
    pil = Image.fromarray(img[:, :, 0], "L") if img.shape[2] == 1 else Image.fromarray(img, "RGB")
    buf = io.BytesIO()
    pil.save(buf, format="JPEG", quality=int(quality), subsampling=0)
    out = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
    return out.reshape(img.shape).astype(np.uint8)


def build():
    arrays = {}
    for name in sorted(CASES):
        img = make_input(name)
        arrays["in_" + name] = img
        for q in QUALITIES:
            arrays["out_%s_q%d" % (name, q)] = libjpeg_round_trip(img, q)
    return arrays


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "jpeg", "jpeg_libjpeg.npz"))
    a = ap.parse_args()
    arrays = build()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print("%s: %d arrays, %d bytes" % (a.out, len(arrays), os.path.getsize(a.out)))
