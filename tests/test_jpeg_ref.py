"""The contract of svae_op_jpeg_batch as tests/jpeg_ref.py restates it, on the CPU.

Against a real codec: tests/golden/jpeg/jpeg_libjpeg.npz (tools/make_jpeg_golden.py) holds small smooth-plus-noise uint8
images and libjpeg's decoded output at 4:4:4 / grey for qualities 10 .. 100.  libjpeg's integer DCT and colour
arithmetic flip some quantiser decisions, so equality is not expected; the condition is a mean absolute difference
below 1 level in every case (a wrong table entry, colour constant or a missing 8-bit rounding of the planes gives
means near or above 1).  4:2:0 is not compared: libjpeg's chroma down- and up-sampling filters differ from the
contract's block means and replication by design.

Then properties that need no restatement of the DCT, and the fp32 mode against the fp64 mode: the inputs are whole
numbers, so quantiser ties exist and the two modes differ in whole blocks, which is why the kernel is held bitwise
to the fp32 mode and not to a tolerance."""
import fractions
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import jpeg_ref as jr
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg", "jpeg_libjpeg.npz")
CASES = ("rgb64", "rgb13x21", "grey28")
QUALITIES = (10, 30, 50, 75, 90, 100)


def _tool():
    spec = importlib.util.spec_from_file_location("svae_make_jpeg_golden", os.path.join(ROOT, "tools", "make_jpeg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _round_trip(img_u8, q, subsample=1, mode="fp64"):
    """The restatement on uint8 levels: lo = 0, hi = 255 make x the level itself."""
    x = img_u8.astype(np.float32)[None]
    r = jr.jpeg_batch(x, 1.0, q, q, subsample, 0.0, 255.0, 1, 0, mode)
    assert list(r["quality"]) == [q]
    np.testing.assert_array_equal(r["out"], r["levels"])
    return r["levels"][0]


def test_fixture_holds_the_listed_cases(golden):
    tool = _tool()
    assert tuple(sorted(CASES)) == tuple(sorted(tool.CASES)) and tuple(tool.QUALITIES) == QUALITIES
    assert sorted(golden) == sorted(["in_" + n for n in CASES] + ["out_%s_q%d" % (n, q) for n in CASES for q in QUALITIES])
    for n in CASES:
        assert golden["in_" + n].shape == tool.CASES[n] and golden["in_" + n].dtype == np.uint8
        np.testing.assert_array_equal(golden["in_" + n], tool.make_input(n))
    assert os.path.getsize(GOLDEN) < 100 * 1024


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_against_libjpeg(golden, name, q):
    img, want = golden["in_" + name], golden["out_%s_q%d" % (name, q)].astype(np.float64)
    got = _round_trip(img, q)
    d = np.abs(got - want)
    print("%s q %d: mean |diff| %.4f level, max %.0f, %.2f %% of pixels off by more than 2"
          % (name, q, d.mean(), d.max(), 100.0 * (d > 2).mean()))
    assert d.mean() < 1.0
    # the artefacts themselves are there: the round trip is not the identity below the top quality
    if q <= 50:
        assert np.abs(got - img).mean() > 0.5


def test_tool_reproduces_the_fixture(golden):
    pytest.importorskip("PIL")
    built = _tool().build()
    assert sorted(built) == sorted(golden)
    for k in built:
        np.testing.assert_array_equal(built[k], golden[k], err_msg=k)


def _nearest_f32(x):
    """The float32 nearest to the exact rational x (ties do not occur for these constants)."""
    f = np.float32(float(x))
    best = min((np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))),
               key=lambda c: abs(fractions.Fraction(float(c)) - x))
    return np.float32(best)


def test_literals_are_the_float32_constants_they_name():
    """The contract's decimal literals, as numpy parses them, are the float32 values a compiler gives them, and the
    eight DCT magnitudes are the float32 nearest to 1 / sqrt(8) and cos(m pi / 16) / 2."""
    lits = list(jr.MAGNITUDES) + ["0.299", "0.587", "0.114", "0.168735892", "0.331264108", "0.418687589", "0.081312411",
                                  "1.402", "0.344136286", "0.714136286", "1.772"]
    for s in lits:
        assert np.float32(s) == _nearest_f32(fractions.Fraction(s)), s
    exact = [1.0 / math.sqrt(8.0)] + [math.cos(m * math.pi / 16.0) / 2.0 for m in range(1, 8)]
    for s, e in zip(jr.MAGNITUDES, exact):
        assert np.float32(s) == np.float32(e), s
    C = jr.dct_matrix(np.float64)
    want = np.array([[(math.sqrt(0.125) if u == 0 else 0.5 * math.cos((2 * x + 1) * u * math.pi / 16)) for x in range(8)]
                     for u in range(8)])
    assert np.abs(C - want).max() < 3e-8
    assert np.abs(C @ C.T - np.eye(8)).max() < 1e-7   # orthonormal: the inverse is the transpose


def test_quantisation_tables():
    """IJG's scaling: quality 50 is the base table, 100 is all ones, 1 saturates at 255, 75 halves."""
    np.testing.assert_array_equal(jr.quant_table(jr.LUMA, 50), jr.LUMA)
    np.testing.assert_array_equal(jr.quant_table(jr.CHROMA, 50), jr.CHROMA)
    assert (jr.quant_table(jr.LUMA, 100) == 1).all() and (jr.quant_table(jr.CHROMA, 100) == 1).all()
    assert (jr.quant_table(jr.LUMA, 1) == 255).all()
    np.testing.assert_array_equal(jr.quant_table(jr.LUMA, 75), (jr.LUMA * 50 + 50) // 100)
    np.testing.assert_array_equal(jr.CHROMA, jr.CHROMA.T)
    # the kernel's copy of the base tables and of the eight magnitudes is this file's
    src = open(os.path.join(ROOT, "sequential-variational-autoencoder_amd", "csrc", "jpeg.hip")).read()
    body = src[src.index("JP_BASE[128] = {") + 16:]
    base = [int(v) for v in body[:body.index("}")].replace("\n", " ").split(",")]
    np.testing.assert_array_equal(np.array(base).reshape(2, 8, 8), np.stack([jr.LUMA, jr.CHROMA]))
    mag = src[src.index("constexpr float jp_mag"):src.index("constexpr float jp_c")]
    assert tuple(re.findall(r"(0\.\d+)f", mag)) == jr.MAGNITUDES


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
@pytest.mark.parametrize("subsample", [1, 2])
@pytest.mark.parametrize("shape", [(13, 21, 3), (16, 8, 1)])
def test_constant_image_stays_constant(shape, subsample, mode):
    for level in (0, 37, 128, 255):
        img = np.full(shape, level, np.uint8)
        for q in (1, 10, 50, 90, 100):
            out = _round_trip(img, q, subsample, mode)
            assert (out == out[0, 0]).all(), (level, q)
            if q == 100:
                np.testing.assert_array_equal(out, img.astype(out.dtype))


def test_constant_float_image_at_q100_is_its_own_quantisation():
    lo, hi = -1.0, 1.0
    x = np.full((1, 9, 10, 3), 0.3137, np.float32)
    r = jr.jpeg_batch(x, 1.0, 100, 100, 2, lo, hi, 3, 0, "fp32")
    level = np.clip(np.rint((np.float32(0.3137) - np.float32(lo)) * np.float32(127.5)), 0, 255)
    want = np.float32(lo) + np.float32(level) * np.float32(2.0 / 255.0)
    assert r["out"].dtype == np.float32 and (r["out"] == want).all()


def test_p0_is_the_identity_and_p1_compresses_all():
    x = np.random.default_rng(0).uniform(-1, 1, size=(5, 9, 11, 3)).astype(np.float32)
    r = jr.jpeg_batch(x, 0.0, 10, 90, 2, -1.0, 1.0, 7, 11, "fp32")
    assert (r["quality"] == 0).all()
    np.testing.assert_array_equal(r["out"].view(np.int32), x.view(np.int32))
    r = jr.jpeg_batch(x, 1.0, 10, 90, 2, -1.0, 1.0, 7, 11, "fp32")
    assert (r["quality"] > 0).all() and not np.array_equal(r["out"], x)


def test_quality_draw_covers_the_range_and_nothing_else():
    q = jr.draws(4000, 1.0, 37, 44, 5, 2 ** 32 - 100)
    assert sorted(set(q.tolist())) == list(range(37, 45))
    assert np.bincount(q)[37:].min() > 400            # uniform: 500 expected per value
    q = jr.draws(2000, 0.5, 1, 100, 5, 0)
    assert q.min() == 0 and set(q[q > 0].tolist()) <= set(range(1, 101)) and 0.4 < (q > 0).mean() < 0.6
    assert (jr.draws(50, 1.0, 75, 75, 9, 0) == 75).all()
    # image b of a call at offset o is image 0 of a call at offset o + b
    np.testing.assert_array_equal(jr.draws(6, 0.5, 5, 95, 3, 2 ** 32 - 2)[2:], jr.draws(4, 0.5, 5, 95, 3, 2 ** 32))


def test_chroma_subsampling_only_touches_colour():
    rng = np.random.default_rng(4)
    grey = rng.integers(0, 256, size=(13, 21, 1)).astype(np.uint8)
    np.testing.assert_array_equal(_round_trip(grey, 40, 1, "fp32"), _round_trip(grey, 40, 2, "fp32"))
    rgb = _tool().make_input("rgb13x21")
    a, b = _round_trip(rgb, 40, 1, "fp32"), _round_trip(rgb, 40, 2, "fp32")
    assert not np.array_equal(a, b)
    # an RGB image without colour has flat chroma planes (128): both modes code the same Y and agree
    flat = np.repeat(grey, 3, axis=2)
    np.testing.assert_array_equal(_round_trip(flat, 40, 1, "fp32"), _round_trip(flat, 40, 2, "fp32"))


def test_fp32_mode_against_fp64_mode(golden):
    """Share of 8 x 8 pixel blocks in which the two modes differ: not zero, because whole-number inputs put
    coefficients on quantiser ties (most often at quality 100, where half of the blocks of a small image can hold one)."""
    worst = 0.0
    differ = 0
    for name in CASES:
        img = golden["in_" + name]
        for q in QUALITIES:
            a, b = _round_trip(img, q, 1, "fp32").astype(np.float64), _round_trip(img, q, 1, "fp64")
            h, w, _ = a.shape
            blocks = [(a[i:i + 8, j:j + 8] != b[i:i + 8, j:j + 8]).any() for i in range(0, h, 8) for j in range(0, w, 8)]
            share = float(np.mean(blocks))
            print("%s q %d: %.2f %% of blocks differ, max |diff| %.0f levels" % (name, q, 100 * share, np.abs(a - b).max()))
            worst = max(worst, share)
            differ += int(np.sum(blocks))
    # ties are real (at quality 100 T = 1 and the DC of whole-number pixels is a multiple of 1/8, often k + 1/2), so
    # a tolerance cannot hold the kernel to either mode; they are still the exception among all blocks
    assert differ > 0 and worst < 1.0
    print("blocks that differ over all cases: %d" % differ)


def test_degradation_jpeg_field_and_flags():
    """The Python side that needs no device: the field's default and validation, the flag's parser."""
    from conftest import pkg_mod
    D = pkg_mod("degrade")
    old = D.Degradation((0.5, 0.5, 3.0), (0.5, 4), (0.5, 2, 4, 12))
    assert old.jpeg == (0.0, 75, 75, 2) and old == D.Degradation(blur=(0.5, 0.5, 3.0), downsample=(0.5, 4),
                                                               cutout=(0.5, 2, 4, 12, 0.0))
    assert D.Degradation(jpeg=(0.5, 10, 90)).jpeg == (0.5, 10, 90, 2)
    assert D.Degradation.from_flags() is None and D.Degradation.from_flags(blur="0.5,1,2").jpeg == (0.0, 75, 75, 2)
    assert D.Degradation.from_flags(jpeg="1,30,30,1") == D.Degradation(jpeg=(1.0, 30, 30, 1))
    for bad in ((0.5, 10), (0.5, 0, 90), (0.5, 90, 10), (1.5, 10, 90), (0.5, 10, 90, 3), (0.5, 10, 101), (-0.1, 10, 90)):
        with pytest.raises(ValueError):
            D.Degradation(jpeg=bad)
    s = D.Degradation(jpeg=(0.25, 10, 90, 1)).jpeg_spec()
    assert (s.p, s.q_lo, s.q_hi, s.subsample) == (0.25, 10, 90, 1) and s is D.Degradation(jpeg=(0.25, 10, 90, 1)).jpeg_spec()
