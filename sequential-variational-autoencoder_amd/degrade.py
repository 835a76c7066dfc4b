"""Structured corruptions of a clean device batch: blur, down-sampling and cut-out ahead of the trainer's pixel
noise, in one svae_op_degrade_batch launch (csrc/degrade.hip), and JPEG compression artefacts after it, in one
svae_op_jpeg_batch launch (csrc/jpeg.hip); the contracts are in include/svae_hip.h.

A ``Degradation`` names the stages; all are off by default.  ``NoisyTrainer(degradation=...)`` corrupts every
training, test and evaluation batch with it; ``degrade_batch`` and ``jpeg_batch`` are the ops on a given batch.
"""
import dataclasses
import functools

import torch

from . import _lib


@dataclasses.dataclass(frozen=True)
class Degradation:
    """blur = (p, sigma_lo, sigma_hi): with probability p per image a Gaussian blur, sigma uniform in [lo, hi] (hi <= 4).
    downsample = (p, factor): with probability p the means of factor x factor blocks, replicated back (factor 1, 2, 4, 8).
    cutout = (p, boxes, min_side, max_side, fill): with probability p, `boxes` (0 .. 4) boxes with sides uniform in
    [min_side, max_side] (cut to the image) set to `fill` in all channels.
    jpeg = (p, q_lo, q_hi, subsample): with probability p a JPEG round trip at an IJG quality uniform in q_lo .. q_hi
    (1 .. 100), chroma 4:4:4 (subsample 1) or 4:2:0 (2, the default of a 3-tuple); applied after the pixel noise."""
    blur: tuple = (0.0, 0.0, 0.0)
    downsample: tuple = (0.0, 1)
    cutout: tuple = (0.0, 0, 1, 1, 0.0)
    jpeg: tuple = (0.0, 75, 75, 2)

    def __post_init__(self):
        b, d, c, j = tuple(self.blur), tuple(self.downsample), tuple(self.cutout), tuple(self.jpeg)
        if len(c) == 4:
            c = c + (0.0,)
        if len(j) == 3:
            j = j + (2,)
        if len(b) != 3 or len(d) != 2 or len(c) != 5:
            raise ValueError("blur = (p, lo, hi), downsample = (p, factor), cutout = (p, boxes, min, max[, fill])")
        if len(j) != 4:
            raise ValueError("jpeg = (p, q_lo, q_hi[, subsample])")
        j = (float(j[0]), int(j[1]), int(j[2]), int(j[3]))
        if not 0.0 <= j[0] <= 1.0 or not 1 <= j[1] <= j[2] <= 100 or j[3] not in (1, 2):
            raise ValueError("jpeg needs p in [0, 1], 1 <= q_lo <= q_hi <= 100 and subsample 1 or 2, got %r" % (j,))
        object.__setattr__(self, "jpeg", j)
        object.__setattr__(self, "blur", (float(b[0]), float(b[1]), float(b[2])))
        object.__setattr__(self, "downsample", (float(d[0]), int(d[1])))
        object.__setattr__(self, "cutout", (float(c[0]), int(c[1]), int(c[2]), int(c[3]), float(c[4])))

    @classmethod
    def from_flags(cls, blur=None, downsample=None, cutout=None, jpeg=None):
        """The command-line form: "P,LO,HI", "P,F", "P,K,MIN,MAX[,FILL]" and "P,QLO,QHI[,SUB]" (None: that stage
        off); None when all four are None."""
        if blur is None and downsample is None and cutout is None and jpeg is None:
            return None
        kw = {}
        if blur is not None:
            kw["blur"] = tuple(float(v) for v in blur.split(","))
        if downsample is not None:
            p, f = downsample.split(",")
            kw["downsample"] = (float(p), int(f))
        if cutout is not None:
            v = cutout.split(",")
            if len(v) not in (4, 5):
                raise ValueError("--cutout takes P,K,MIN,MAX[,FILL]")
            kw["cutout"] = (float(v[0]), int(v[1]), int(v[2]), int(v[3])) + ((float(v[4]),) if len(v) == 5 else ())
        if jpeg is not None:
            v = jpeg.split(",")
            if len(v) not in (3, 4):
                raise ValueError("--jpeg takes P,QLO,QHI[,SUB]")
            kw["jpeg"] = (float(v[0]),) + tuple(int(t) for t in v[1:])
        return cls(**kw)

    def c_spec(self, noise=(0.0, 0.0, 0.0)):
        """svae_degrade_spec with the pixel noise (pepper_prob, salt_prob, gaussian_scale)."""
        return _c_spec(self, tuple(float(v) for v in noise))

    def jpeg_spec(self):
        """svae_jpeg_spec of the jpeg stage."""
        return _jpeg_spec(self.jpeg)


@functools.lru_cache(maxsize=64)
def _c_spec(deg, noise):
    # one struct per (Degradation, noise): the per-step call passes it by reference and never writes it
    return _lib.SvaeDegradeSpec(*deg.blur, *deg.downsample, *deg.cutout, *noise)


@functools.lru_cache(maxsize=64)
def _jpeg_spec(jpeg):
    return _lib.SvaeJpegSpec(*jpeg)


def add_flags(ap):
    """--blur, --downsample, --cutout and --jpeg of tools/train.py and tools/evaluate.py."""
    ap.add_argument("--blur", default=None, metavar="P,LO,HI",
                    help="blur each input image with probability P, Gaussian sigma uniform in [LO, HI] (HI <= 4)")
    ap.add_argument("--downsample", default=None, metavar="P,F",
                    help="with probability P replace each input image by the means of its F x F blocks (F 1, 2, 4, 8)")
    ap.add_argument("--cutout", default=None, metavar="P,K,MIN,MAX[,FILL]",
                    help="with probability P cut K (0 .. 4) boxes with sides in [MIN, MAX] out of each input image, "
                         "set to FILL (default 0)")
    ap.add_argument("--jpeg", default=None, metavar="P,QLO,QHI[,SUB]",
                    help="with probability P put each input image through a JPEG round trip at a quality uniform in "
                         "QLO .. QHI (1 .. 100), after the pixel noise; SUB 1: 4:4:4 chroma, 2 (default): 4:2:0")


def degrade_batch(target, spec, lo, hi, noise=(0.0, 0.0, 0.0), seed=0, offset=0, out=None, mask=None):
    """One svae_op_degrade_batch launch on the current stream: the degraded copy of the clean contiguous float32
    device batch ``target`` [n,h,w,c] under ``spec`` (a Degradation), then the pixel noise ``noise`` =
    (pepper_prob, salt_prob, gaussian_scale) and the clip to [lo, hi].  ``out`` (default: a new tensor) receives it
    and is returned; ``mask`` [n,h,w] float32, when given, receives 1 where a pixel was cut out.  The caller
    advances ``offset`` by ceil(n h w c / 4) per call, as for svae_op_make_batch."""
    if target.dtype != torch.float32 or target.dim() != 4 or not target.is_cuda:
        raise ValueError("degrade_batch takes a float32 [n,h,w,c] device batch")
    n, h, w, c = (int(v) for v in target.shape)
    if out is None:
        out = torch.empty_like(target)
    if out.dtype != torch.float32 or out.device != target.device or out.numel() != target.numel():
        raise ValueError("out must be a float32 tensor of the batch's size on its device")
    if mask is not None and (mask.dtype != torch.float32 or mask.device != target.device or mask.numel() != n * h * w):
        raise ValueError("mask must be a float32 [n,h,w] tensor on the batch's device")
    cs = spec.c_spec(noise)
    _lib.check(_lib.lib().svae_op_degrade_batch(
        _lib.ptr(target), n, h, w, c, lo, hi, cs, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
        _lib.ptr(out), _lib.ptr(mask), _lib.stream_ptr(torch.cuda.current_stream(target.device))))
    return out


def jpeg_batch(x, spec, lo, hi, seed=0, offset=0, out=None, quality=None):
    """One svae_op_jpeg_batch launch on the current stream: the contiguous float32 device batch ``x`` [n,h,w,c]
    (c 1 or 3, values in [lo, hi]) with the JPEG artefacts of ``spec`` (a Degradation: its jpeg stage).  ``out`` =
    None works in place on ``x``; ``quality`` [n] int32, when given, receives the quality of every image (0: not
    compressed).  Image b draws under the counter offset + b.  Returns the output tensor."""
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda:
        raise ValueError("jpeg_batch takes a float32 [n,h,w,c] device batch")
    n, h, w, c = (int(v) for v in x.shape)
    if out is None:
        out = x
    if out.dtype != torch.float32 or out.device != x.device or out.numel() != x.numel():
        raise ValueError("out must be a float32 tensor of the batch's size on its device")
    if quality is not None and (quality.dtype != torch.int32 or quality.device != x.device or quality.numel() != n):
        raise ValueError("quality must be an int32 [n] tensor on the batch's device")
    _lib.check(_lib.lib().svae_op_jpeg_batch(
        _lib.ptr(x), n, h, w, c, lo, hi, spec.jpeg_spec(), int(seed) & 0xFFFFFFFFFFFFFFFF,
        int(offset) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(out), _lib.ptr(quality),
        _lib.stream_ptr(torch.cuda.current_stream(x.device))))
    return out
