"""CPU checks of the power-spectrum report's fixed parts: the numpy restatement of svae_op_power_spectrum
(tests/spectrum_ref.py) against numpy's FFT, the tables of spectra.py, the entry point's argument checks (all made
on the host before any device call) and the report's arithmetic.

Bound of the FFT comparison: the restatement is a plain DFT with sums of up to n = 64 terms per pass, so its error
is of the order n * eps = 1.4e-14 of the largest value; 1e-12 of the largest power leaves two decades (errors of
1.3e-15 were measured when the bound was written).  Parseval's identity compares two sums of the same h * w
squares and is held to 1e-12 relative (2.2e-16 measured).
"""
import ctypes

import numpy as np
import pytest

import spectrum_ref
from conftest import pkg_mod

SHAPES = [(7, 9), (8, 8), (12, 5), (28, 28), (64, 64)]


def _tables(h, w, kind):
    S = pkg_mod("spectra")
    table, n_bins, counts = S.radial_bins(h, w)
    return S.window(h, kind), S.window(w, kind), S.twiddles(h), S.twiddles(w), table, n_bins, counts


@pytest.mark.parametrize("kind", ["hann", "none"])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_matches_rfft2(shape, kind):
    h, w = shape
    wy, wx, ty, tx, table, n_bins, _ = _tables(h, w, kind)
    rng = np.random.default_rng(100 * h + w)
    img = rng.uniform(-1, 1, (h, w)).astype(np.float32)
    a = (img.astype(np.float64) * wy[:, None]) * wx[None, :]
    got = spectrum_ref.half_power(a, ty, tx)
    want = np.abs(np.fft.rfft2(a)) ** 2 * spectrum_ref.multiplicity(w)[None, :]
    err = np.abs(got - want).max() / want.max()
    print("%s %s: largest error %.2e of the largest power" % (shape, kind, err))
    assert err <= 1e-12
    # Parseval with no entry skipped: every entry in one bin
    everything = np.zeros((h, w // 2 + 1), dtype=np.int32)
    total = spectrum_ref.bin_power(got, everything, 1)[0]
    want_total = h * w * np.sum(a * a)
    print("Parseval: relative difference %.2e" % (abs(total - want_total) / want_total))
    assert abs(total - want_total) <= 1e-12 * want_total
    # and the binned sums are the FFT's, annulus by annulus
    binned = spectrum_ref.bin_power(got, table, n_bins)
    for b in range(n_bins):
        assert abs(binned[b] - want[table == b].sum()) <= 1e-12 * want.max() * max(1, (table == b).sum())


@pytest.mark.parametrize("shape", SHAPES + [(96, 96), (6, 64), (2, 2)])
def test_radial_bins(shape):
    S = pkg_mod("spectra")
    h, w = shape
    table, n_bins, counts = S.radial_bins(h, w)
    wu = w // 2 + 1
    assert table.shape == (h, wu) and table.dtype == np.int32 and n_bins == min(h, w) // 2 + 1
    assert counts.shape == (n_bins,) and counts.dtype == np.float64
    m = spectrum_ref.multiplicity(w)
    kept = 0.0
    for v in range(h):
        fy = v if v <= h // 2 else v - h
        for u in range(wu):
            rho = np.sqrt((fy / h) ** 2 + (u / w) ** 2) * min(h, w)
            b = table[v, u]
            if b >= 0:
                assert b < n_bins and abs(rho - b) <= 0.5 + 1e-12, (v, u)  # within half a bin of its radius
                kept += m[u]
            else:
                assert b == -1 and rho >= n_bins - 0.5 - 1e-12, (v, u)     # only what lies beyond the last annulus
    assert counts.sum() == kept and table[0, 0] == 0
    for v in range(1, h):                                                  # symmetric under v <-> h - v
        assert np.array_equal(table[v], table[h - v])
    if h == w and h > 2:
        assert np.all(counts > 0) and (table == -1).any() and counts[0] == 1.0  # whole annuli, the corners dropped


def test_windows_and_twiddles():
    S = pkg_mod("spectra")
    for n in (2, 5, 8, 64):
        k = np.arange(n)
        assert np.array_equal(S.window(n, "none"), np.ones(n))
        hann = S.window(n, "hann")
        assert hann.dtype == np.float64 and hann[0] == 0.0
        np.testing.assert_allclose(hann, np.sin(np.pi * k / n) ** 2, atol=1e-15)   # periodic: no zero at the end
        assert n == 2 or hann[-1] > 0.0
        tw = S.twiddles(n)
        assert tw.shape == (n, 2) and tw.dtype == np.float64 and tw[0, 0] == 1.0 and tw[0, 1] == 0.0
        np.testing.assert_allclose(tw[:, 0] + 1j * tw[:, 1], np.exp(-2j * np.pi * k / n), atol=1e-15)
    with pytest.raises(ValueError):
        S.window(8, "hamming")


@pytest.mark.parametrize("freq", [(3, 5), (-4, 2), (0, 9), (7, 0), (16, 16)])
def test_a_pure_cosine_lands_in_its_bin_alone(freq):
    h = w = 32
    fy, fx = freq
    wy, wx, ty, tx, table, n_bins, _ = _tables(h, w, "none")
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.cos(2 * np.pi * (fy * yy / h + fx * xx / w)).astype(np.float32)
    x = img.reshape(1, h, w, 1)
    out, bad = spectrum_ref.power_spectrum_ref(x, None, wy, wx, ty, tx, table, n_bins)
    assert bad.sum() == 0 and np.all(np.isnan(out[0, 0, 1]))
    p = out[0, 0, 0]
    b = int(np.floor(np.hypot(fy, fx) + 0.5))
    total = h * w * float(np.sum(img.astype(np.float64) ** 2))
    if b < n_bins:
        assert abs(p[b] - total) <= 1e-6 * total       # the fp32 rounding of the samples leaks 1e-7 of the amplitude
        assert np.delete(p, b).max() <= 1e-12 * total
    else:
        assert p.max() <= 1e-12 * total                # a corner frequency: dropped


def test_symbol_is_exported_and_bound(built_lib):
    L = pkg_mod("_lib")
    assert "svae_op_power_spectrum" in L.EXPORTED
    fn = L.lib().svae_op_power_spectrum
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 16
    hdr = open(pkg_mod("build").INCLUDE + "/svae_hip.h").read()
    assert "#define SVAE_SPECTRUM_MAX_DIM %d\n" % L.SPECTRUM_MAX_DIM in hdr
    assert "#define SVAE_SPECTRUM_MAX_BINS %d\n" % L.SPECTRUM_MAX_BINS in hdr
    assert L.SPECTRUM_MAX_DIM >= 64
    assert "spectrum.hip" in pkg_mod("build").SOURCES


def test_argument_checks_run_on_the_host(built_lib):
    """Every SVAE_EBADARG and SVAE_EBADCONFIG case returns before any device call: the pointers are never read."""
    L = pkg_mod("_lib")
    fn = L.lib().svae_op_power_spectrum
    p = ctypes.c_void_p(0x1000)
    good = dict(x=p, n=4, y=p, ny=2, h=8, w=8, c=3, win_y=p, win_x=p, tw_y=p, tw_x=p, bin=p, n_bins=5, out=p,
                nonfinite=None, stream=None)
    order = list(good)

    def call(**over):
        a = dict(good, **over)
        return fn(*[a[k] for k in order])

    for name in ("x", "win_y", "win_x", "tw_y", "tw_x", "bin", "out"):
        assert call(**{name: None}) == -2, name
        assert b"power_spectrum" in L.lib().svae_last_error(None)
    for name in ("n", "ny", "c", "n_bins"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -2, name
    assert call(y=None, ny=0) == -2
    assert call(h=1) == -2 and call(w=1) == -2 and call(h=0) == -2
    assert call(n=5) == -2                       # 5 images against 2 targets
    big = L.SPECTRUM_MAX_DIM + 1
    assert call(h=big) == -1 and call(w=big) == -1
    assert call(n_bins=L.SPECTRUM_MAX_BINS + 1) == -1
    assert call(n=2 ** 30, c=4, ny=2) == -1      # n * c past 2^31 - 1
    assert b"power_spectrum" in L.lib().svae_last_error(None)


def test_spectra_imports_without_a_gpu_and_reports():
    S = pkg_mod("spectra")
    counts = np.array([1.0, 8.0, 12.0, 16.0, 20.0, 24.0])
    target = [4.0, 80.0, 60.0, 32.0, 20.0, 12.0]
    same = S.profile_report(target, target, counts, err=[0.0] * 6)
    assert same["log_spectral_distance"] == 0.0 and same["hf_ratio"] == 1.0 and same["cutoff"] == 1.0
    assert same["band_snr_db"] == [float("inf")] * 6
    assert same["power_db"][1] == pytest.approx(10.0)
    # a blurred output: the power falls off and the error takes over from bin 3
    blurred = [4.0, 80.0, 30.0, 3.2, 0.2, 0.012]
    err = [0.0, 0.8, 6.0, 40.0, 20.0, 12.0]
    r = S.profile_report(blurred, target, counts, err=err)
    assert S.hf_first(6) == 4
    assert r["hf_ratio"] == pytest.approx((0.2 + 0.012) / 32.0)
    assert r["cutoff"] == 3 / 6
    assert r["band_snr_db"][1] == pytest.approx(20.0) and r["band_snr_db"][4] == 0.0
    want = np.sqrt(np.mean((10 * np.log10(np.array(blurred[1:]) / np.array(target[1:]))) ** 2))
    assert r["log_spectral_distance"] == pytest.approx(want)
    s = S.profile_report(blurred, target, counts)
    assert sorted(s) == ["hf_ratio", "log_spectral_distance", "power_db"]
