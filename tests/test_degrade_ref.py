"""The numpy restatement of svae_op_degrade_batch (tests/degrade_ref.py) against its own contract: no GPU."""
import numpy as np
import pytest

import batch_ref
import degrade_ref as dr
from conftest import pkg_mod

SEED = 0x0123456789ABCDEF


def _images(n, h, w, c, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, size=(n, h, w, c)).astype(np.float32)


@pytest.mark.parametrize("noise", [(0.0, 0.0, 0.0), (0.3, 0.2, 0.0), (0.1, 0.1, 0.1)])
@pytest.mark.parametrize("mode", ["fp64", "fp32"])
def test_identity_spec_is_make_batch(noise, mode):
    x = _images(3, 5, 7, 3)
    spec = dr.IDENTITY._replace(pepper_prob=noise[0], salt_prob=noise[1], gaussian_scale=noise[2])
    got = dr.degrade(x, spec, -1.0, 1.0, SEED, 41, mode)
    ref = batch_ref.make_batch(x.reshape(3, -1), None, 0, 3, -1.0, 1.0, *noise, SEED, 41)
    np.testing.assert_array_equal(got["input"].reshape(3, -1), ref["input"])
    assert not got["mask"].any()


@pytest.mark.parametrize("h,w", [(7, 9), (28, 28), (1, 5), (64, 3)])
@pytest.mark.parametrize("sides", [(1, 1), (1, 4), (3, 70), (100, 200), (1, 2 ** 31 - 1)])
def test_every_box_lies_inside_the_image(h, w, sides):
    spec = dr.IDENTITY._replace(p_cut=1.0, boxes=4, min_side=sides[0], max_side=sides[1])
    seen_h, seen_w = set(), set()
    for d in dr.draws(64, h, w, spec, SEED, 5):
        assert d["cut"] and len(d["boxes"]) == 4
        for y0, x0, bh, bw in d["boxes"]:
            assert 1 <= bh <= h and 1 <= bw <= w and 0 <= y0 and y0 + bh <= h and 0 <= x0 and x0 + bw <= w
            assert bh == h or sides[0] <= bh <= sides[1]
            assert bw == w or sides[0] <= bw <= sides[1]
            seen_h.add(bh), seen_w.add(bw)
    if sides[0] >= max(h, w):
        assert seen_h == {h} and seen_w == {w}  # a box at least the image's size covers it
    m = dr.degrade(_images(2, h, w, 2), spec._replace(fill=0.5), -1.0, 1.0, SEED, 5)
    assert m["mask"].any() and np.all(m["input"][m["mask"] == 1] == 0.5)


@pytest.mark.parametrize("mode,dt", [("fp64", np.float64), ("fp32", np.float32)])
@pytest.mark.parametrize("value", [0.7, -0.3333333])
def test_constant_image_survives_blur_and_downsampling(mode, dt, value):
    x = np.full((4, 13, 11, 3), value, np.float32)
    spec = dr.IDENTITY._replace(p_blur=1.0, sigma_lo=0.3, sigma_hi=4.0, p_down=1.0, factor=4)
    got = dr.degrade(x, spec, -1.0, 1.0, SEED, 0, mode)
    assert {d["r"] for d in got["draws"]} - {0} and all(d["down"] for d in got["draws"])
    # the truth stays within 1 ulp of the float32 value.  The fp32 mode rounds every operation: per blur pass the
    # weights sum to 1 within 2 r + 2 roundings (their sum and one division each) and the taps add 2 r + 1 products
    # and as many sums, so at most 6 r + 4 roundings of 2^-24 |v| per pass, and the block mean adds f^2 more
    ulp = float(np.spacing(np.float32(abs(value))))
    r = max(d["r"] for d in got["draws"])
    bound = ulp if mode == "fp64" else (2 * (6 * r + 4) + 4 * 4) * 2.0 ** -24 * abs(value)
    err = np.abs(got["structured"].astype(np.float64) - float(np.float32(value))).max()
    print(mode, "max deviation %.3e, ulp %.3e, bound %.3e" % (err, ulp, bound))
    assert err <= bound


@pytest.mark.parametrize("f", [2, 4, 8])
def test_downsampling_twice_is_downsampling_once(f):
    img = _images(1, 13, 22, 3)[0]
    # the second pass averages m = f^2 (or fewer) equal values v: m - 1 sequential adds and one division, each
    # within half an ulp, so |twice - once| <= m (eps / 2) |v| to first order; |v| <= 1 here
    for dt in (np.float64, np.float32):
        once = dr.downsample(img.astype(dt), f, dt)
        twice = dr.downsample(once, f, dt)
        err = np.abs(twice.astype(np.float64) - once.astype(np.float64)).max()
        print(dt.__name__, "f = %d: max |twice - once| %.3e (bound %.3e)" % (f, err, f * f * np.finfo(dt).eps / 2))
        assert once.dtype == dt and err <= f * f * np.finfo(dt).eps / 2
        assert not np.array_equal(once, img.astype(dt))
        # every block is constant after one pass
        np.testing.assert_array_equal(once[:f, :f], np.broadcast_to(once[0, 0], once[:f, :f].shape))


def test_gates_fire_half_the_time():
    spec = dr.IDENTITY._replace(p_blur=0.5, sigma_lo=0.5, sigma_hi=2.0, p_down=0.5, factor=2, p_cut=0.5, boxes=1,
                                min_side=2, max_side=3)
    d = dr.draws(4096, 8, 8, spec, SEED, 123)
    for gate in ("blur", "down", "cut"):
        fired = sum(bool(x[gate]) for x in d)
        print(gate, fired)
        assert abs(fired - 2048) <= 128  # four binomial standard deviations of 32
    sig = np.array([float(x["sigma"]) for x in d])
    assert 0.5 <= sig.min() and sig.max() <= 2.0 and 1.2 < sig.mean() < 1.3
    # p = 0 never fires, p = 1 always does (thr = 2^32 - 1: all but the word 2^32 - 1)
    off = dr.draws(256, 8, 8, spec._replace(p_blur=0.0, p_down=0.0, p_cut=0.0), SEED, 123)
    on = dr.draws(256, 8, 8, spec._replace(p_blur=1.0, p_down=1.0, p_cut=1.0), SEED, 123)
    assert not any(x["blur"] or x["down"] or x["cut"] for x in off)
    assert all(x["blur"] and x["down"] and x["cut"] for x in on)


@pytest.mark.parametrize("shape", [(2, 1, 2, 2), (3, 7, 9, 3), (128, 64, 64, 3), (5, 1, 1, 4)])
def test_offsets_one_batch_apart_share_no_image_counter(shape):
    n, h, w, c = shape
    assert h * w * c >= 4
    step = (n * h * w * c + 3) // 4
    for off in (0, 17, 2 ** 32 - 2, 2 ** 64 - step - 1):
        a = set(dr.image_counters(n, off))
        b = set(dr.image_counters(n, off + step))
        assert len(a) == n and len(b) == n and not (a & b)


def test_structural_stream_is_not_a_pixel_stream():
    """c2 = 3 is a Philox stream of its own: the gate words differ from the words of streams 0 .. 2 at the same
    counter."""
    a = dr.image_words(8, SEED, 9, 0)
    for stream in (0, 1, 2):
        w = batch_ref.words(32, SEED, 9, stream).reshape(8, 4)
        assert not np.any(a == w)


def test_binding_matches_the_header_struct():
    import ctypes
    L = pkg_mod("_lib")
    assert ctypes.sizeof(L.SvaeDegradeSpec) == 13 * 4
    assert [f[0] for f in L.SvaeDegradeSpec._fields_] == list(dr.Spec._fields)
    assert "svae_op_degrade_batch" in L.EXPORTED
    D = pkg_mod("degrade").Degradation
    s = D(blur=(0.5, 0.5, 2), downsample=(1, 4), cutout=(0.25, 2, 3, 9)).c_spec((0.1, 0.2, 0.3))
    got = dr.Spec(*(getattr(s, k) for k in dr.Spec._fields))
    assert got == dr.Spec(0.5, 0.5, 2.0, 1.0, 4, 0.25, 2, 3, 9, 0.0, np.float32(0.1), np.float32(0.2), np.float32(0.3))
    assert D() == D.from_flags("0,0,0", "0,1", "0,0,1,1") and D.from_flags() is None
    assert D.from_flags("0.5,0.5,2", None, "0.25,2,3,9,-1") == D(blur=(0.5, 0.5, 2.0), cutout=(0.25, 2, 3, 9, -1.0))
