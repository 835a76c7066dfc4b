"""A dataset that lives on the device, and the reference's batch cursor over it.

The reference's dataset objects (dataset/dataset_celeba.py and its siblings) decode files into a host
float32 cache and hand numpy batches to the trainer.  Here the images stay where the training step reads
them: uint8 (CelebA at 64x64x3 is 2.4 GB) or fp32 [N, H, W, C] tensors on the device, and a batch is a
(start, B) window that svae_op_make_batch gathers, dequantises and corrupts in one launch
(trainer.NoisyTrainer).  File decoders are out of scope: from_array takes what a decoder produced.

PatchDataset holds images larger than the network's and serves random crops of them (svae_op_crop_batch).
"""
import math

import numpy as np
import torch


class DeviceDataset:
    def __init__(self, train, test, range=(-1.0, 1.0), name="dataset"):
        for t in (train, test):
            if t.dim() != 4 or t.dtype not in (torch.uint8, torch.float32):
                raise ValueError("DeviceDataset holds uint8 or float32 [N, H, W, C] tensors")
        if tuple(train.shape[1:]) != tuple(test.shape[1:]) or train.dtype != test.dtype:
            raise ValueError("train and test must agree in image shape and dtype")
        self.train, self.test = train.contiguous(), test.contiguous()
        self.range = (float(range[0]), float(range[1]))
        self.name = name
        self.data_dims = list(train.shape[1:])
        self.train_size, self.test_size = int(train.shape[0]), int(test.shape[0])
        self.train_idx = 0
        self.test_idx = 0

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_array(cls, arr, test_fraction=0.2, range=(-1.0, 1.0), name="array", device=None):
        """The reference's split (dataset_celeba.py:16-19): the first floor(N (1 - test_fraction)) images
        train, the rest test.  arr: uint8 or float [N, H, W, C] (numpy or torch)."""
        t = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr))
        if t.dtype != torch.uint8:
            t = t.to(torch.float32)
        n_train = int(math.floor(t.shape[0] * (1.0 - test_fraction)))
        if n_train <= 0 or n_train >= t.shape[0]:
            raise ValueError("the split leaves an empty part")
        if device is not None:
            t = t.to(device)
        return cls(t[:n_train], t[n_train:], range=range, name=name)

    @classmethod
    def synthetic(cls, n, h, w, c, seed=0, test_fraction=0.2, range=(-1.0, 1.0), device=None):
        """n seeded uint8 images (smooth gradients plus noise: something a network can fit)."""
        g = torch.Generator().manual_seed(seed)
        yy = torch.linspace(0, 1, h).view(1, h, 1, 1)
        xx = torch.linspace(0, 1, w).view(1, 1, w, 1)
        a = torch.rand(n, 1, 1, c, generator=g)
        b = torch.rand(n, 1, 1, c, generator=g)
        img = a * yy + b * xx * (1 - a) + 0.1 * torch.rand(n, h, w, c, generator=g)
        u8 = (img.clamp(0, 1) * 255).round().to(torch.uint8)
        return cls.from_array(u8, test_fraction=test_fraction, range=range, name="synthetic", device=device)

    # ------------------------------------------------------------------ the reference's cursor
    @staticmethod
    def _advance(cursor, batch_size, size):
        """dataset_celeba.py:34-41: advance; past the end, restart at [0, B).  Returns (start, cursor)."""
        if batch_size > size:
            raise ValueError("batch %d exceeds the %d images" % (batch_size, size))
        prev = cursor
        cursor += batch_size
        if cursor > size:
            cursor = batch_size
            prev = 0
        return prev, cursor

    def next_batch(self, batch_size):
        start, self.train_idx = self._advance(self.train_idx, batch_size, self.train_size)
        return start, batch_size

    def next_test_batch(self, batch_size):
        start, self.test_idx = self._advance(self.test_idx, batch_size, self.test_size)
        return start, batch_size

    # ------------------------------------------------------------------ views
    @property
    def per_image(self):
        return int(np.prod(self.data_dims))

    def rows(self, window, test=False):
        """The window's images as stored (uint8 or fp32), a view."""
        start, b = window
        return (self.test if test else self.train)[start:start + b]

    def display(self, x):
        """(x - lo) / (hi - lo) clipped to [0, 1] (dataset_celeba.py:112-114 at (-1, 1))."""
        lo, hi = self.range
        if isinstance(x, torch.Tensor):
            return ((x.to(torch.float32) - lo) / (hi - lo)).clamp(0.0, 1.0)
        return np.clip((np.asarray(x, dtype=np.float64) - lo) / (hi - lo), 0.0, 1.0)

    def state_dict(self):
        return {"train_idx": self.train_idx, "test_idx": self.test_idx}

    def load_state_dict(self, s):
        self.train_idx, self.test_idx = int(s["train_idx"]), int(s["test_idx"])


class PatchDataset(DeviceDataset):
    """Large images on the device, seen through a network of tile size ``tile`` = (h, w): every training batch is a
    set of fresh random crops (window, integer box scale, mirror / rotation: crops.CropSpec) made by one
    svae_op_crop_batch launch (csrc/crops.hip), so neither a cut copy of the images nor a fixed tiling exists.

    ``train_images`` / ``test_images`` are uint8 or float32 [N, H, W, C] device tensors of one dtype and channel
    count (their extents may differ).  ``data_dims`` is the tile's [h, w, C].  ``.train`` and ``.test`` are fixed
    sets of ``eval_crops`` crops each, made once here by the same op under ``eval_seed`` (rows 0 .. eval_crops - 1
    of that key from the training images, the next eval_crops rows from the test images), uint8 for uint8 images
    (the rounded block mean) and float32 otherwise: the cursor, test(), evaluate(), latent_information(),
    sample_quality() and visualize walk them as they walk any DeviceDataset.  ``patch_batch`` is the training
    batch; NoisyTrainer calls it instead of gathering rows of ``.train``."""

    def __init__(self, train_images, test_images, tile, scales=(1,), symmetries=1, eval_crops=256, eval_seed=0,
                 range=(-1.0, 1.0), name="patches"):
        from . import crops
        for t in (train_images, test_images):
            if t.dim() != 4 or t.dtype not in (torch.uint8, torch.float32) or not t.is_cuda:
                raise ValueError("PatchDataset holds uint8 or float32 [N, H, W, C] device tensors")
        if train_images.dtype != test_images.dtype or train_images.shape[3] != test_images.shape[3]:
            raise ValueError("train and test images must agree in dtype and channels")
        h, w = int(tile[0]), int(tile[1])
        self.spec = crops.CropSpec(tuple(scales), symmetries)
        if self.spec.symmetries == 8 and h != w:
            raise ValueError("the dihedral group needs a square tile, got %d x %d" % (h, w))
        smax = max(self.spec.scales)
        for t in (train_images, test_images):
            if smax * h > t.shape[1] or smax * w > t.shape[2]:
                raise ValueError("a %d x %d tile at scale %d exceeds the %d x %d images"
                                 % (h, w, smax, t.shape[1], t.shape[2]))
        if int(eval_crops) <= 0:
            raise ValueError("eval_crops must be positive")
        self.tile = (h, w)
        self.train_images, self.test_images = train_images.contiguous(), test_images.contiguous()
        self.eval_crops, self.eval_seed = int(eval_crops), int(eval_seed) & 0xFFFFFFFFFFFFFFFF
        u8 = train_images.dtype == torch.uint8
        fixed = []
        for k, images in enumerate((self.train_images, self.test_images)):
            out = torch.empty([self.eval_crops, h, w, int(images.shape[3])], dtype=images.dtype, device=images.device)
            crops.crop_batch(images, self.tile, self.spec, self.eval_crops, self.eval_seed, k * self.eval_crops, range,
                             out=None if u8 else out, out_u8=out if u8 else None)
            fixed.append(out)
        super().__init__(fixed[0], fixed[1], range=range, name=name)

    @classmethod
    def from_array(cls, arr, tile, test_fraction=0.2, range=(-1.0, 1.0), name="array", device=None, **kw):
        """DeviceDataset.from_array's split of the large images: the first floor(N (1 - test_fraction)) train, the
        rest test.  arr: uint8 or float [N, H, W, C] (numpy or torch); ``kw``: scales, symmetries, eval_crops,
        eval_seed."""
        t = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr))
        if t.dtype != torch.uint8:
            t = t.to(torch.float32)
        n_train = int(math.floor(t.shape[0] * (1.0 - test_fraction)))
        if n_train <= 0 or n_train >= t.shape[0]:
            raise ValueError("the split leaves an empty part")
        if device is not None:
            t = t.to(device)
        return cls(t[:n_train], t[n_train:], tile, range=range, name=name, **kw)

    def patch_batch(self, batch_size, seed, offset, out, meta=None):
        """Fill the float32 [B, h, w, C] device tensor ``out`` with fresh crops of the training images: row b under
        (seed, offset + b).  ``meta`` int32 [B, 5], when given, receives (m, s, g, y0, x0) per row."""
        from . import crops
        return crops.crop_batch(self.train_images, self.tile, self.spec, batch_size, seed, offset, self.range, out=out,
                                meta=meta)
