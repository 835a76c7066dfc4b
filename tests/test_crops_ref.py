"""tests/crops_ref.py, the numpy restatement of svae_op_crop_batch's contract, against plain numpy: slicing and
batch_ref's dequantisation, np.flip / transpose, reshaped block sums, the ranges of the draws, and the rounding of
target_u8.  No GPU."""
import numpy as np
import pytest

import batch_ref as br
import crops_ref as cr

LO, HI = -1.0, 1.0


def _images(nimg, H, W, c, u8, seed=0):
    rng = np.random.default_rng(seed + nimg + H + W + c)
    if u8:
        return rng.integers(0, 256, (nimg, H, W, c), dtype=np.uint8)
    return (rng.standard_normal((nimg, H, W, c)) * np.exp(rng.uniform(-8, 8, (nimg, H, W, c)))).astype(np.float32)


def _bitwise(a, b):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
def test_plain_crops_are_slices_through_make_batch(u8):
    nimg, H, W, c, h, w = 3, 37, 53, 3, 8, 12
    img = _images(nimg, H, W, c, u8)
    crops = [(0, 1, 0, 0, 0), (2, 1, 0, H - h, W - w), (1, 1, 0, 5, 17), (1, 1, 0, 29, 0)]
    got = cr.crop_batch(img, h, w, n=len(crops), lo=LO, hi=HI, crops=crops)
    tiles = np.stack([img[m, y:y + h, x:x + w] for m, _, _, y, x in crops])
    want = br.make_batch(tiles, None, 0, len(crops), LO, HI, 0.0, 0.0, 0.0, 0, 0)["target"]
    _bitwise(got["target"].reshape(len(crops), -1), want)
    np.testing.assert_array_equal(got["meta"], np.asarray(crops, np.int32))
    if u8:
        np.testing.assert_array_equal(got["target_u8"], tiles)  # s = 1: the bytes themselves
    else:
        assert got["target_u8"] is None


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
def test_the_eight_symmetries_are_flips_and_a_transpose(u8):
    nimg, H, W, c, h = 2, 20, 23, 3, 7
    img = _images(nimg, H, W, c, u8)
    plain = cr.crop_batch(img, h, h, n=1, crops=[(1, 2, 0, 3, 4)])["target"][0]
    seen = set()
    for g in range(8):
        got = cr.crop_batch(img, h, h, n=1, crops=[(1, 2, g, 3, 4)])["target"][0]
        # the source is mirrored (bit 0: columns, bit 1: rows), then read transposed (bit 2)
        want = plain
        if g & 1:
            want = np.flip(want, axis=1)
        if g & 2:
            want = np.flip(want, axis=0)
        if g & 4:
            want = np.transpose(want, (1, 0, 2))
        _bitwise(got, want)
        seen.add(got.tobytes())
    assert len(seen) == 8
    # a tile that is not square: the four mirrors
    wide = cr.crop_batch(img, 5, 9, n=1, crops=[(0, 1, 0, 2, 1)])["target"][0]
    for g in range(4):
        got = cr.crop_batch(img, 5, 9, n=1, crops=[(0, 1, g, 2, 1)])["target"][0]
        want = np.flip(wide, axis=1) if g & 1 else wide
        _bitwise(got, np.flip(want, axis=0) if g & 2 else want)


@pytest.mark.parametrize("s", [2, 3, 8])
def test_box_means_are_block_sums_divided_in_fp32(s):
    nimg, H, W, c, h, w = 2, 70, 90, 3, 8, 11
    y0, x0 = H - s * h, 1
    img = _images(nimg, H, W, c, True)
    got = cr.crop_batch(img, h, w, n=1, crops=[(1, s, 0, y0, x0)])
    win = img[1, y0:y0 + s * h, x0:x0 + s * w].astype(np.int64)
    total = win.reshape(h, s, w, s, c).transpose(0, 2, 4, 1, 3).reshape(h, w, c, s * s).sum(-1)
    qbar = total.astype(np.float32) / np.float32(s * s)
    qs = np.float32((np.float64(np.float32(HI)) - np.float64(np.float32(LO))) / 255.0)
    _bitwise(got["target"][0], np.float32(LO) + qbar * qs)
    np.testing.assert_array_equal(got["target_u8"][0], np.minimum(255, np.rint(qbar)).astype(np.uint8))
    # fp32: the sum runs p outside, q inside, every add rounded
    f = _images(nimg, H, W, c, False)
    got = cr.crop_batch(f, h, w, n=1, crops=[(0, s, 0, y0, x0)])["target"][0]
    acc = np.zeros((h, w, c), np.float32)
    for p in range(s):
        for q in range(s):
            acc = (acc + f[0, y0 + p:y0 + s * h:s, x0 + q:x0 + s * w:s]).astype(np.float32)
    _bitwise(got, acc / np.float32(s * s))
    # the order matters at this dynamic range: a pairwise float64 sum differs somewhere
    exact = f[0, y0:y0 + s * h, x0:x0 + s * w].astype(np.float64).reshape(h, s, w, s, c).sum((1, 3)) / (s * s)
    assert (exact.astype(np.float32) != got).any()


def test_draws_are_in_range_and_reach_both_ends():
    nimg, H, W, h, w = 5, 40, 45, 8, 8
    scales, sym, n = (1, 2, 3), 8, 4096
    meta = cr.draw(n, nimg, H, W, h, w, scales, sym, seed=0x1234567887654321, offset=(1 << 32) - 100)
    m, s, g, y0, x0 = meta.T
    assert m.min() == 0 and m.max() == nimg - 1
    assert set(s.tolist()) == set(scales)
    assert g.min() == 0 and g.max() == sym - 1
    for sc in scales:
        k = s == sc
        assert y0[k].min() == 0 and y0[k].max() == H - sc * h, sc
        assert x0[k].min() == 0 and x0[k].max() == W - sc * w, sc
    assert (y0 >= 0).all() and (x0 >= 0).all() and (y0 + s * h <= H).all() and (x0 + s * w <= W).all()
    # ranges of one value draw that value
    one = cr.draw(64, 1, 24, 24, 8, 8, (3,), 1, seed=5, offset=0)
    np.testing.assert_array_equal(one, np.tile(np.array([0, 3, 0, 0, 0], np.int32), (64, 1)))
    # symmetries 2 and 4 stay below 2 and 4
    for sym in (2, 4):
        g = cr.draw(512, 2, 20, 20, 8, 8, (1,), sym, seed=1, offset=0)[:, 2]
        assert set(g.tolist()) == set(range(sym))


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
def test_a_row_is_a_function_of_seed_and_offset_plus_b(u8):
    nimg, H, W, c, h, w = 3, 37, 53, 3, 8, 8
    img = _images(nimg, H, W, c, u8)
    kw = dict(scales=(1, 2, 3), symmetries=8, seed=99, lo=LO, hi=HI)
    o = (1 << 32) - 7  # the counter's low word wraps inside the batch
    whole = cr.crop_batch(img, h, w, offset=o, n=16, **kw)
    first = cr.crop_batch(img, h, w, offset=o, n=6, **kw)
    rest = cr.crop_batch(img, h, w, offset=o + 6, n=10, **kw)
    for key in ("target", "meta") + (("target_u8",) if u8 else ()):
        np.testing.assert_array_equal(whole[key], np.concatenate([first[key], rest[key]]))
    other = cr.crop_batch(img, h, w, offset=o, n=16, **dict(kw, seed=100))
    assert (other["meta"] != whole["meta"]).any()
    assert len({tuple(r) for r in whole["meta"].tolist()}) > 8


def test_target_u8_rounds_ties_to_even():
    img = np.zeros((1, 4, 8, 1), np.uint8)
    # 2 x 2 blocks with sums 2, 6, 10 and 1018: means 0.5, 1.5, 2.5 and 254.5, each exactly halfway
    img[0, 0, 0], img[0, 0, 1] = 1, 1
    img[0, 0, 2], img[0, 1, 2] = 3, 3
    img[0, 0, 4], img[0, 1, 5] = 5, 5
    img[0, 0:2, 6:8] = np.array([[255, 255], [254, 254]], np.uint8).reshape(2, 2, 1)
    img[0, 2:4, 0:2] = 255  # and the largest mean
    got = cr.crop_batch(img, 2, 4, n=1, crops=[(0, 2, 0, 0, 0)], lo=0.0, hi=1.0)
    qbar = np.array([0.5, 1.5, 2.5, 254.5, 255.0, 0.0, 0.0, 0.0], np.float32).reshape(2, 4, 1)
    np.testing.assert_array_equal(got["target_u8"][0], np.array([0, 2, 2, 254, 255, 0, 0, 0], np.uint8).reshape(2, 4, 1))
    _bitwise(got["target"][0], np.float32(0.0) + qbar * np.float32(1.0 / 255.0))
