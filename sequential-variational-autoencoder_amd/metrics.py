"""Image quality metrics on the device: one svae_op_image_metrics launch (csrc/metrics.hip) per call.

``image_metrics(x, y, data_range)`` scores every image of ``x`` against image ``i % ny`` of ``y`` and returns the
op's [n, 4] fp64 table: sum (x - y)^2, sum |x - y|, mean SSIM (Wang et al. 2004: 11 x 11 Gaussian window,
sigma 1.5, valid positions, K1 = 0.01, K2 = 0.03, L = data_range) and the non-finite count.  ``psnr`` turns the
first column into decibels.  There is no torch formulation behind it: without the library the call raises.
"""
import math

import torch

from . import _lib

COLS = 4
COL_SSE, COL_SAE, COL_SSIM, COL_NONFINITE = range(4)


def image_metrics(x, y, data_range, out=None):
    """[n, 4] fp64 device tensor for x [n,H,W,C] (or [k,B,H,W,C], n = k B, row j B + b for x[j, b]) against
    y [ny,H,W,C], n a multiple of ny: image i of x is compared with image i % ny of y.  Both are contiguous
    float32 tensors on one GPU.  ``out``: a contiguous fp64 device tensor of at least n rows of 4 to write
    into (its first n rows are returned); the launch goes to x's device's current stream, nothing
    synchronises."""
    if x.dim() == 5 and x.is_contiguous():
        x = x.view(-1, *x.shape[2:])
    if x.dim() != 4 or y.dim() != 4 or tuple(x.shape[1:]) != tuple(y.shape[1:]):
        raise ValueError("image_metrics takes x [n,H,W,C] or [k,B,H,W,C] and y [ny,H,W,C], got %s / %s"
                         % (tuple(x.shape), tuple(y.shape)))
    for t in (x, y):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.device != x.device:
            raise ValueError("image_metrics takes contiguous float32 tensors on one GPU")
    n, h, w, c = (int(v) for v in x.shape)
    if out is None:
        out = torch.empty(n, COLS, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or out.device != x.device or not out.is_contiguous() or out.numel() < n * COLS:
        raise ValueError("out must be a contiguous float64 tensor of at least n * 4 elements on x's device")
    _lib.check(_lib.lib().svae_op_image_metrics(_lib.ptr(x), n, _lib.ptr(y), int(y.shape[0]), h, w, c,
                                                float(data_range), _lib.ptr(out),
                                                _lib.stream_ptr(torch.cuda.current_stream(x.device))))
    return out.view(-1)[:n * COLS].view(n, COLS)


def psnr(sse, n_elem, data_range):
    """10 log10(L^2 / mse) with mse = sse / n_elem; +inf at mse = 0.  ``sse`` is a number or a tensor (the
    result is then a tensor on its device, nothing synchronises)."""
    peak = float(data_range) ** 2
    if isinstance(sse, torch.Tensor):
        return 10.0 * torch.log10(peak / (sse.double() / n_elem))  # x / 0 = +inf, log10(+inf) = +inf
    mse = float(sse) / n_elem
    return math.inf if mse == 0.0 else 10.0 * math.log10(peak / mse)
