"""Random crops of large device-resident images as clean batches: window, integer box scale and mirror / rotation
per row, in one svae_op_crop_batch launch (csrc/crops.hip; the contract is in include/svae_hip.h).

A ``CropSpec`` names the scales and the symmetry group; ``crop_batch`` is the op on given images.
``data.PatchDataset`` holds the large images and hands ``NoisyTrainer`` a fresh batch of crops every step.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import torch

from . import _lib

META_COLS = 5  # (m, s, g, y0, x0)
calls = 0      # svae_op_crop_batch launches made through crop_batch (tests assert on it)


@dataclasses.dataclass(frozen=True)
class CropSpec:
    """scales: up to four distinct integer box factors in 1 .. 8 (a crop at scale s averages s x s source blocks of an
    s h x s w window); symmetries: 1 none, 2 mirror x, 4 mirror x and / or y, 8 the dihedral group (square tiles)."""
    scales: tuple = (1,)
    symmetries: int = 1

    def __post_init__(self):
        sc = tuple(int(s) for s in self.scales)
        if not 1 <= len(sc) <= 4 or len(set(sc)) != len(sc) or min(sc) < 1 or max(sc) > 8:
            raise ValueError("scales: one to four distinct integers in 1 .. 8, got %r" % (self.scales,))
        if int(self.symmetries) not in (1, 2, 4, 8):
            raise ValueError("symmetries must be 1, 2, 4 or 8, got %r" % (self.symmetries,))
        object.__setattr__(self, "scales", sc)
        object.__setattr__(self, "symmetries", int(self.symmetries))

    @classmethod
    def from_flags(cls, patch_scales="1", patch_symmetries=1):
        """The command-line form: "1,2" and N."""
        return cls(tuple(int(v) for v in str(patch_scales).split(",")), int(patch_symmetries))

    def c_spec(self):
        return _c_spec(self)


@functools.lru_cache(maxsize=64)
def _c_spec(spec):
    # one struct per CropSpec: the per-step call passes it by reference and never writes it
    sc = spec.scales + (0,) * (4 - len(spec.scales))
    return _lib.SvaeCropSpec(len(spec.scales), (ctypes.c_int32 * 4)(*sc), spec.symmetries)


def add_flags(ap):
    """--patches, --patch_scales, --patch_symmetries and --eval_crops of tools/train.py and tools/evaluate.py."""
    ap.add_argument("--patches", action="store_true",
                    help="--data (or --synthetic) holds large images: train on fresh random crops of the preset's "
                         "image size (data.PatchDataset) and evaluate on a fixed set of crops")
    ap.add_argument("--patch_scales", default="1", metavar="S[,S..]",
                    help="integer box down-scaling factors (1 .. 8, up to four) a crop draws from")
    ap.add_argument("--patch_symmetries", type=int, default=1, choices=[1, 2, 4, 8],
                    help="1 none, 2 mirror x, 4 mirror x and / or y, 8 the dihedral group (square images)")
    ap.add_argument("--eval_crops", type=int, default=256, metavar="N",
                    help="crops in each of the fixed train and test evaluation sets")


def check_crops(crops, nimg, H, W, h, w):
    """Raise unless every (m, s, g, y0, x0) of a host [n,5] array is in the range the op's contract names."""
    c = np.asarray(crops, dtype=np.int64).reshape(-1, META_COLS)
    m, s, g, y0, x0 = c.T
    ok = (m >= 0) & (m < nimg) & (s >= 1) & (s <= 8) & (g >= 0) & (g < (8 if h == w else 4)) & (y0 >= 0) & (x0 >= 0) \
        & (y0 + s * h <= H) & (x0 + s * w <= W)
    if not ok.all():
        raise ValueError("crop %d is out of range: (m, s, g, y0, x0) = %s" % (int(np.argmin(ok)), c[np.argmin(ok)].tolist()))
    return c.astype(np.int32)


def crop_batch(images, tile, spec=CropSpec(), n=None, seed=0, offset=0, range=(-1.0, 1.0), crops=None, out=None,
               out_u8=None, meta=None):
    """One svae_op_crop_batch launch on the current stream: ``n`` crops of tile size ``tile`` = (h, w) of the
    contiguous device images [nimg,H,W,c] (uint8 or float32).  Rows are drawn under (seed, offset + b), or are
    ``crops``: an [n,5] int32 device tensor of (m, s, g, y0, x0) used as it is (the caller's contract), or a host
    array / list, which is range-checked and uploaded.  ``out`` float32 [n,h,w,c] and ``out_u8`` uint8 (uint8 images
    only) receive the batch; with neither given a new float32 tensor does.  ``meta`` int32 [n,5], when given,
    receives the rows' parameters.  Returns ``out`` (or ``out_u8`` when only that was given)."""
    global calls
    if images.dim() != 4 or images.dtype not in (torch.uint8, torch.float32) or not images.is_cuda:
        raise ValueError("crop_batch takes uint8 or float32 [nimg,H,W,c] device images")
    nimg, H, W, c = (int(v) for v in images.shape)
    h, w = int(tile[0]), int(tile[1])
    if crops is not None and not isinstance(crops, torch.Tensor):
        crops = torch.from_numpy(check_crops(crops, nimg, H, W, h, w)).to(images.device)
    if crops is not None:
        if crops.dtype != torch.int32 or crops.device != images.device or crops.dim() != 2 or crops.shape[1] != META_COLS:
            raise ValueError("crops must be an int32 [n,5] tensor on the images' device")
        n = int(crops.shape[0]) if n is None else int(n)
        if int(crops.shape[0]) < n:
            raise ValueError("crops holds %d rows, n is %d" % (int(crops.shape[0]), n))
    if n is None:
        raise ValueError("crop_batch needs n or crops")
    if out is None and out_u8 is None:
        out = torch.empty([n, h, w, c], dtype=torch.float32, device=images.device)
    for t, dt in ((out, torch.float32), (out_u8, torch.uint8), (meta, torch.int32)):
        want = n * META_COLS if t is meta else n * h * w * c
        if t is not None and (t.dtype != dt or t.device != images.device or t.numel() != want):
            raise ValueError("out, out_u8 and meta must be float32 / uint8 [n,h,w,c] and int32 [n,5] on the images' device")
    lo, hi = range
    calls += 1
    _lib.check(_lib.lib().svae_op_crop_batch(
        _lib.ptr(images), 1 if images.dtype == torch.uint8 else 0, nimg, H, W, c, h, w, spec.c_spec(), _lib.ptr(crops),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, n, lo, hi, _lib.ptr(out), _lib.ptr(out_u8),
        _lib.ptr(meta), _lib.stream_ptr(torch.cuda.current_stream(images.device))))
    return out if out is not None else out_u8
