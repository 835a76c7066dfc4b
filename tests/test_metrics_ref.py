"""CPU checks of tests/metrics_ref.py (the float64 restatement the GPU tests of svae_op_image_metrics are held
to) and of the entry point's argument checks, which run on the host before any device call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import metrics_ref
from conftest import ROOT, pkg_mod


def _images(n, h, w, c, seed):
    """Smooth images plus noise in [-1, 1], float32 [n,h,w,c]."""
    rng = np.random.default_rng(seed)
    yy = np.linspace(0, 1, h).reshape(1, h, 1, 1)
    xx = np.linspace(0, 1, w).reshape(1, 1, w, 1)
    a, b = rng.uniform(-1, 1, (2, n, 1, 1, c))
    img = 0.6 * (a * np.cos(3 * yy + b) + b * np.sin(4 * xx * (1 + a))) + 0.25 * rng.uniform(-1, 1, (n, h, w, c))
    return np.clip(img, -1, 1).astype(np.float32)


def test_constants_match_the_header_and_the_binding():
    L = pkg_mod("_lib")
    txt = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    hdr = {k: float(re.search(r"#define SVAE_%s ([0-9.]+)" % k, txt).group(1))
           for k in ("SSIM_WINDOW", "SSIM_SIGMA", "SSIM_K1", "SSIM_K2", "METRICS_TILE")}
    assert (hdr["SSIM_WINDOW"], hdr["SSIM_SIGMA"], hdr["SSIM_K1"], hdr["SSIM_K2"]) == (
        metrics_ref.WINDOW, metrics_ref.SIGMA, metrics_ref.K1, metrics_ref.K2)
    assert (L.SSIM_WINDOW, L.SSIM_SIGMA, L.SSIM_K1, L.SSIM_K2, L.METRICS_TILE) == (
        hdr["SSIM_WINDOW"], hdr["SSIM_SIGMA"], hdr["SSIM_K1"], hdr["SSIM_K2"], hdr["METRICS_TILE"])
    g = metrics_ref.gaussian_window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5


@pytest.mark.parametrize("shape", [(2, 11, 11, 1), (2, 12, 13, 3), (3, 32, 32, 1), (2, 20, 37, 2)])
def test_helper_agrees_with_separable_correlation(shape):
    """An independent formulation: scipy.ndimage.correlate1d along both image axes, cropped to the valid region.
    It is a separable evaluation, which is what the helper's bound is derived for."""
    from scipy.ndimage import correlate1d
    n, h, w, c = shape
    x, y = _images(n, h, w, c, 1), _images(n, h, w, c, 2)
    want, bound = metrics_ref.metrics_ref(x, y, 2.0)
    g = metrics_ref.gaussian_window()
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    blur = lambda q: correlate1d(correlate1d(q, g, axis=1, mode="constant"), g, axis=2, mode="constant")[:, 5:-5, 5:-5]
    mx, my = blur(xd), blur(yd)
    vx, vy, cxy = blur(xd * xd) - mx * mx, blur(yd * yd) - my * my, blur(xd * yd) - mx * my
    c1, c2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    q = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    assert q.shape == (n, h - 10, w - 10, c)
    got = np.zeros_like(want)
    got[:, 0] = ((xd - yd) ** 2).reshape(n, -1).sum(1)
    got[:, 1] = np.abs(xd - yd).reshape(n, -1).sum(1)
    got[:, 2] = q.reshape(n, -1).mean(1)
    print("max |ssim difference| %.3e, bound %.3e .. %.3e" % (np.abs(got[:, 2] - want[:, 2]).max(), bound[:, 2].min(),
                                                              bound[:, 2].max()))
    metrics_ref.assert_rows(got, want, bound, str(shape))
    assert np.all(bound[:, 2] < 1e-9) and np.all(want[:, 2] < 0.999) and np.all(want[:, 0] > 0)


def test_ssim_of_an_image_with_itself_is_one_and_ssim_is_symmetric():
    x, y = _images(3, 16, 19, 3, 3), _images(3, 16, 19, 3, 4)
    same, bound = metrics_ref.metrics_ref(x, x, 2.0)
    assert np.all(same[:, :2] == 0.0) and np.all(bound[:, :2] == 0.0)
    assert np.all(np.abs(same[:, 2] - 1.0) <= 1e-15)
    ab, _ = metrics_ref.metrics_ref(x, y, 2.0)
    ba, _ = metrics_ref.metrics_ref(y, x, 2.0)
    assert np.array_equal(ab, ba)


def test_pairing_and_non_finite_rows():
    x, y = _images(6, 12, 12, 2, 5), _images(2, 12, 12, 2, 6)
    rows, bound = metrics_ref.metrics_ref(x, y, 2.0)
    for i in range(6):
        one, _ = metrics_ref.metrics_ref(x[i:i + 1], y[i % 2:i % 2 + 1], 2.0)
        assert np.array_equal(rows[i], one[0])
    x[4, 3, 2, 1] = np.nan
    y[1, 0, 0, 0] = np.inf
    rows2, _ = metrics_ref.metrics_ref(x, y, 2.0)
    assert rows2[:, 3].tolist() == [0, 1, 0, 1, 1, 1]
    assert np.all(np.isnan(rows2[[1, 3, 4, 5], :3])) and np.array_equal(rows2[[0, 2]], rows[[0, 2]])


@pytest.mark.parametrize("a,b", [(0.25, -0.5), (0.7, 0.7), (0.0, 1.0)])
def test_constant_images_have_the_closed_form(a, b):
    """Flat windows: mu = a, b and zero (co)variance, so SSIM = (2 a b + C1) / (a^2 + b^2 + C1)."""
    x = np.full((1, 14, 15, 2), a, dtype=np.float32)
    y = np.full((1, 14, 15, 2), b, dtype=np.float32)
    rows, bound = metrics_ref.metrics_ref(x, y, 2.0)
    a, b = float(np.float32(a)), float(np.float32(b))
    c1 = (0.01 * 2.0) ** 2
    assert abs(rows[0, 2] - (2 * a * b + c1) / (a * a + b * b + c1)) <= bound[0, 2]
    assert rows[0, 0] == pytest.approx((a - b) ** 2 * 14 * 15 * 2, rel=1e-14)
    assert rows[0, 1] == pytest.approx(abs(a - b) * 14 * 15 * 2, rel=1e-14)


def test_psnr_helper_and_package_psnr():
    M = pkg_mod("metrics")
    v, bound = metrics_ref.psnr_ref(3.0, 12, 2.0, 0.0)
    assert abs(v - 10 * math.log10(4.0 / 0.25)) < 1e-13 and 0 < bound < 1e-13
    assert abs(M.psnr(3.0, 12, 2.0) - v) <= bound
    assert M.psnr(0.0, 12, 2.0) == math.inf and metrics_ref.psnr_ref(0.0, 12, 2.0) == (math.inf, 0.0)
    import torch
    t = M.psnr(torch.tensor([3.0, 0.0], dtype=torch.float64), 12, 2.0)
    assert abs(float(t[0]) - v) <= bound and float(t[1]) == math.inf


def test_entry_point_is_exported_and_bound(built_lib):
    L = pkg_mod("_lib")
    assert "svae_op_image_metrics" in L.EXPORTED
    assert hasattr(ctypes.CDLL(built_lib), "svae_op_image_metrics")
    assert L.lib().svae_op_image_metrics.restype is ctypes.c_int32


def test_image_metrics_rejects_bad_arguments_without_a_gpu(built_lib):
    """SVAE_EBADARG (-2) for every case include/svae_hip.h lists, before any device call: the pointers are
    never dereferenced."""
    lib = pkg_mod("_lib").lib()
    p = ctypes.c_void_p(4096)
    good = [p, 6, p, 2, 11, 11, 1, 2.0, p, None]  # x, n, y, ny, h, w, c, data_range, out, stream
    cases = [(0, None), (2, None), (8, None),          # a null pointer
             (1, 0), (1, -6), (3, 0), (3, -2), (6, 0), (6, -1),  # n, ny, c <= 0
             (1, 5), (3, 4),                            # n % ny != 0
             (4, 10), (5, 10), (4, 0), (5, -3),         # h or w < 11
             (7, 0.0), (7, -1.0), (7, float("nan"))]    # data_range <= 0 or NaN
    for i, bad in cases:
        args = list(good)
        args[i] = bad
        assert lib.svae_op_image_metrics(*args) == -2, (i, bad)
        assert b"image_metrics" in lib.svae_last_error(None)
