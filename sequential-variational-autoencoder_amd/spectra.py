"""Radially averaged power spectra on the device: one svae_op_power_spectrum launch (csrc/spectrum.hip) per call.

``power_spectrum(x, y)`` returns the op's [n, c, 2, n_bins] fp64 table for a stack of images x and reference images
y: per image and channel the power of the windowed image (plane 0) and of the windowed difference x - y (plane 1),
summed over the annuli of ``radial_bins``.  PSNR and SSIM both reward a smooth output; the spectrum says at which
spatial frequencies an output still differs from the clean image, and whether it is as sharp.  The op computes its
DFT from the caller's tables in a fixed order (include/svae_hip.h), so two reports are comparable bit for bit and no
[n, h, w / 2 + 1] complex intermediate exists.  There is no torch formulation behind it: without the library the
call raises.  The module itself imports without a GPU (the tables and the report arithmetic are numpy and floats).
"""
import math

import numpy as np

WINDOWS = ("hann", "none")


def twiddles(n):
    """[n, 2] fp64: tw[k] = (cos 2 pi k / n, -sin 2 pi k / n), the op's tw_y / tw_x table."""
    a = 2.0 * np.pi * np.arange(int(n), dtype=np.float64) / float(n)
    return np.stack([np.cos(a), -np.sin(a)], 1)


def window(n, kind="hann"):
    """[n] fp64: the periodic Hann window 0.5 - 0.5 cos(2 pi k / n), or ones for "none"."""
    if kind == "none":
        return np.ones(int(n), dtype=np.float64)
    if kind != "hann":
        raise ValueError("window must be one of %s, got %r" % (WINDOWS, kind))
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(n), dtype=np.float64) / float(n))


def multiplicity(w):
    """[w // 2 + 1] fp64: how many entries of the full spectrum column u of the half spectrum stands for."""
    m = np.full(w // 2 + 1, 2.0)
    m[0] = 1.0
    if w % 2 == 0:
        m[w // 2] = 1.0
    return m


def radial_bins(h, w):
    """(table, n_bins, counts): the int32 [h, w // 2 + 1] bin of every half-spectrum entry, the number of bins and
    the fp64 [n_bins] entry counts including the multiplicity (a profile is a bin's power over its count).  Entry
    (v, u) has the signed frequencies fy = v (v <= h / 2) or v - h, fx = u, the radius
    rho = sqrt((fy / h)^2 + (fx / w)^2) * min(h, w) and the bin floor(rho + 1/2), kept up to min(h, w) // 2 and -1
    beyond: the corners are dropped, only whole annuli count."""
    h, w = int(h), int(w)
    v = np.arange(h)
    fy = np.where(v <= h // 2, v, v - h).astype(np.float64)
    fx = np.arange(w // 2 + 1, dtype=np.float64)
    rho = np.sqrt((fy[:, None] / h) ** 2 + (fx[None, :] / w) ** 2) * min(h, w)
    b = np.floor(rho + 0.5).astype(np.int64)
    n_bins = min(h, w) // 2 + 1
    table = np.where(b < n_bins, b, -1).astype(np.int32)
    counts = np.zeros(n_bins, dtype=np.float64)
    m = multiplicity(w)
    for u in range(w // 2 + 1):
        for vv in range(h):
            if table[vv, u] >= 0:
                counts[table[vv, u]] += m[u]
    return table, n_bins, counts


_tables = {}


def device_tables(h, w, kind, device):
    """The op's device tables for (h, w, window), made once per device: (win_y, win_x, tw_y, tw_x, bin, n_bins,
    counts), counts a host numpy array."""
    import torch
    key = (str(device), int(h), int(w), kind)
    if key not in _tables:
        table, n_bins, counts = radial_bins(h, w)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        _tables[key] = (dev(window(h, kind)), dev(window(w, kind)), dev(twiddles(h)), dev(twiddles(w)), dev(table),
                        n_bins, counts)
    return _tables[key]


def power_spectrum(x, y=None, window="hann", out=None, nonfinite=None):
    """[n, c, 2, n_bins] fp64 device tensor for x [n,H,W,C] (or [k,B,H,W,C], n = k B) against y [ny,H,W,C], n a
    multiple of ny (image i of x is paired with image i % ny of y), over the annuli of radial_bins(H, W).  With
    y = None only plane 0 is computed (a fresh result then holds zeros in plane 1; a given ``out`` keeps what it
    held).  Both are contiguous float32 tensors on one GPU.  ``out``: a contiguous fp64 device tensor of at least
    n * c * 2 * n_bins elements to write into; ``nonfinite``: a contiguous int64 device tensor of at least n * c
    elements for the op's per-(image, channel) non-finite counts.  The launch goes to x's device's current stream,
    nothing synchronises."""
    import torch

    from . import _lib
    if x.dim() == 5 and x.is_contiguous():
        x = x.view(-1, *x.shape[2:])
    if x.dim() != 4 or (y is not None and (y.dim() != 4 or tuple(x.shape[1:]) != tuple(y.shape[1:]))):
        raise ValueError("power_spectrum takes x [n,H,W,C] or [k,B,H,W,C] and y [ny,H,W,C] or None, got %s / %s"
                         % (tuple(x.shape), None if y is None else tuple(y.shape)))
    for t in (x,) if y is None else (x, y):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.device != x.device:
            raise ValueError("power_spectrum takes contiguous float32 tensors on one GPU")
    n, h, w, c = (int(v) for v in x.shape)
    win_y, win_x, tw_y, tw_x, table, n_bins, _ = device_tables(h, w, window, x.device)
    size = n * c * 2 * n_bins
    if out is None:
        out = (torch.zeros if y is None else torch.empty)(size, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or out.device != x.device or not out.is_contiguous() or out.numel() < size:
        raise ValueError("out must be a contiguous float64 tensor of at least n * c * 2 * n_bins elements on x's device")
    if nonfinite is not None and (nonfinite.dtype != torch.int64 or nonfinite.device != x.device
                                  or not nonfinite.is_contiguous() or nonfinite.numel() < n * c):
        raise ValueError("nonfinite must be a contiguous int64 tensor of at least n * c elements on x's device")
    _lib.check(_lib.lib().svae_op_power_spectrum(
        _lib.ptr(x), n, _lib.ptr(y), n if y is None else int(y.shape[0]), h, w, c, _lib.ptr(win_y), _lib.ptr(win_x),
        _lib.ptr(tw_y), _lib.ptr(tw_x), _lib.ptr(table), n_bins, _lib.ptr(out), _lib.ptr(nonfinite),
        _lib.stream_ptr(torch.cuda.current_stream(x.device))))
    return out.view(-1)[:size].view(n, c, 2, n_bins)


# ---------------------------------------------------------------------- the report's arithmetic (host floats)
def _db(num, den=1.0):
    """10 log10(num / den): -inf for num = 0, +inf for den = 0 (0 / 0 and a NaN: NaN)."""
    if num != num or den != den or (num == 0.0 and den == 0.0):
        return math.nan
    if den == 0.0:
        return math.inf
    if num == 0.0:
        return -math.inf
    return 10.0 * math.log10(num / den)


def hf_first(n_bins):
    """The first bin of the high-frequency band: the bins above n_bins / 2."""
    return n_bins // 2 + 1


def profile_report(power, target, counts, err=None):
    """One entry of NoisyTrainer.spectrum's report from per-bin mean powers (channels summed, mean over images,
    not yet divided by the bins' counts): ``power`` of the images, ``target`` of the clean ones, ``err`` of the
    difference (None: no band SNR and no cutoff).
      power_db[b]            10 log10(power[b] / counts[b])
      band_snr_db[b]         10 log10(target[b] / err[b])
      log_spectral_distance  the RMS over b >= 1 of the dB difference between the two profiles
      hf_ratio               the power in the bins above n_bins / 2 over the target's there
      cutoff                 the first b >= 1 with band SNR below 0 dB, over n_bins; 1.0 if there is none"""
    nb = len(counts)
    res = {"power_db": [_db(power[b] / counts[b]) if counts[b] else math.nan for b in range(nb)]}
    if err is not None:
        res["band_snr_db"] = [_db(target[b], err[b]) for b in range(nb)]
    d = [_db(power[b], target[b]) for b in range(1, nb) if counts[b]]
    res["log_spectral_distance"] = math.sqrt(sum(v * v for v in d) / len(d)) if d else math.nan
    k = hf_first(nb)
    top, ref = sum(power[k:]), sum(target[k:])
    res["hf_ratio"] = top / ref if ref else math.nan
    if err is not None:
        below = [b for b in range(1, nb) if res["band_snr_db"][b] < 0.0]
        res["cutoff"] = below[0] / nb if below else 1.0
    return res
