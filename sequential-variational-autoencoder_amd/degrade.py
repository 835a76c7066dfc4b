"""Structured corruptions of a clean device batch: blur, down-sampling and cut-out ahead of the trainer's pixel
noise, in one svae_op_degrade_batch launch (csrc/degrade.hip; the contract is in include/svae_hip.h).

A ``Degradation`` names the stages; all are off by default.  ``NoisyTrainer(degradation=...)`` corrupts every
training, test and evaluation batch with it; ``degrade_batch`` is the op on a given batch.
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
    [min_side, max_side] (cut to the image) set to `fill` in all channels."""
    blur: tuple = (0.0, 0.0, 0.0)
    downsample: tuple = (0.0, 1)
    cutout: tuple = (0.0, 0, 1, 1, 0.0)

    def __post_init__(self):
        b, d, c = tuple(self.blur), tuple(self.downsample), tuple(self.cutout)
        if len(c) == 4:
            c = c + (0.0,)
        if len(b) != 3 or len(d) != 2 or len(c) != 5:
            raise ValueError("blur = (p, lo, hi), downsample = (p, factor), cutout = (p, boxes, min, max[, fill])")
        object.__setattr__(self, "blur", (float(b[0]), float(b[1]), float(b[2])))
        object.__setattr__(self, "downsample", (float(d[0]), int(d[1])))
        object.__setattr__(self, "cutout", (float(c[0]), int(c[1]), int(c[2]), int(c[3]), float(c[4])))

    @classmethod
    def from_flags(cls, blur=None, downsample=None, cutout=None):
        """The command-line form: "P,LO,HI", "P,F" and "P,K,MIN,MAX[,FILL]" (None: that stage off); None when all
        three are None."""
        if blur is None and downsample is None and cutout is None:
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
        return cls(**kw)

    def c_spec(self, noise=(0.0, 0.0, 0.0)):
        """svae_degrade_spec with the pixel noise (pepper_prob, salt_prob, gaussian_scale)."""
        return _c_spec(self, tuple(float(v) for v in noise))


@functools.lru_cache(maxsize=64)
def _c_spec(deg, noise):
    # one struct per (Degradation, noise): the per-step call passes it by reference and never writes it
    return _lib.SvaeDegradeSpec(*deg.blur, *deg.downsample, *deg.cutout, *noise)


def add_flags(ap):
    """--blur, --downsample and --cutout of tools/train.py and tools/evaluate.py."""
    ap.add_argument("--blur", default=None, metavar="P,LO,HI",
                    help="blur each input image with probability P, Gaussian sigma uniform in [LO, HI] (HI <= 4)")
    ap.add_argument("--downsample", default=None, metavar="P,F",
                    help="with probability P replace each input image by the means of its F x F blocks (F 1, 2, 4, 8)")
    ap.add_argument("--cutout", default=None, metavar="P,K,MIN,MAX[,FILL]",
                    help="with probability P cut K (0 .. 4) boxes with sides in [MIN, MAX] out of each input image, "
                         "set to FILL (default 0)")


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
