"""A dataset that lives on the device, and the reference's batch cursor over it.

The reference's dataset objects (dataset/dataset_celeba.py and its siblings) decode files into a host
float32 cache and hand numpy batches to the trainer.  Here the images stay where the training step reads
them: uint8 (CelebA at 64x64x3 is 2.4 GB) or fp32 [N, H, W, C] tensors on the device, and a batch is a
(start, B) window that svae_op_make_batch gathers, dequantises and corrupts in one launch
(trainer.NoisyTrainer).  File decoders are out of scope: from_array takes what a decoder produced.
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
