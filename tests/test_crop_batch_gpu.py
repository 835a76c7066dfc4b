"""svae_op_crop_batch (csrc/crops.hip) against its numpy restatement (tests/crops_ref.py), bit for bit: target,
target_u8 and meta.  The draws are integer arithmetic, a uint8 block mean is an exact sum and one fp32 division, an
fp32 block mean a sum in a stated order and one division, so nothing is compared within a tolerance.  Every output
sits between NaN (uint8: 0xA5, int32: -7) guard bands that must survive.

The kernel gives a block a tile of 32 x 32 output pixels while the source patch of the largest listed scale fits
32 KB of LDS, of 16 x 16 while it fits 64 KB, and reads from global memory beyond that; the shapes below take each of
the three paths with one block and with several blocks per row."""
import ctypes

import numpy as np
import pytest
import torch

import crops_ref as cr
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
GUARD = 64
EBADCONFIG, EBADARG = -1, -2
NIMG, H, W = 3, 37, 53


def _images(nimg, Hh, Ww, c, u8, seed=0):
    rng = np.random.default_rng(seed + 7 * nimg + Hh + Ww + c + int(u8))
    if u8:
        return rng.integers(0, 256, (nimg, Hh, Ww, c), dtype=np.uint8)
    return (rng.standard_normal((nimg, Hh, Ww, c)) * np.exp(rng.uniform(-8, 8, (nimg, Hh, Ww, c)))).astype(np.float32)


def _to_device(a, shift=0):
    """The array on the device, its first element ``shift`` elements past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:shift + t.numel()]
    d.copy_(t)
    assert d.data_ptr() % 16 == (shift * t.element_size()) % 16
    return d


def _guarded(n, dtype, shift=0):
    """(the n-element output ``shift`` elements past a 16-byte boundary inside guard bands, check -> numpy)."""
    fill = {torch.float32: float("nan"), torch.uint8: 0xA5, torch.int32: -7}[dtype]
    buf = torch.full((n + 2 * GUARD + 16,), fill, dtype=dtype, device="cuda")
    a = GUARD + shift

    def check():
        hst = buf.cpu().numpy()
        outside = np.concatenate([hst[:a], hst[a + n:]])
        assert np.isnan(outside).all() if dtype == torch.float32 else (outside == fill).all(), "wrote outside the output"
        return hst[a:a + n]
    return buf[a:a + n], check


def _spec(scales, symmetries):
    return pkg_mod("crops").CropSpec(tuple(scales), symmetries).c_spec()


def _crop(img, h, w, scales=(1,), symmetries=1, n=1, seed=0, offset=0, crops=None, src_shift=0, out_shift=0,
          want=("f32", "u8", "meta"), lo=LO, hi=HI):
    """dict(target, target_u8, meta) of one launch; outputs not asked for (or not legal) stay None."""
    L = pkg_mod("_lib")
    nimg, Hh, Ww, c = img.shape
    u8 = img.dtype == np.uint8
    src = _to_device(img, src_shift)
    cd = None if crops is None else torch.from_numpy(np.asarray(crops, np.int32).reshape(n, 5)).cuda()
    out, chk = _guarded(n * h * w * c, torch.float32, out_shift)
    out8, chk8 = _guarded(n * h * w * c, torch.uint8, out_shift)
    meta, chkm = _guarded(n * 5, torch.int32)
    use8 = u8 and "u8" in want
    L.check(L.lib().svae_op_crop_batch(
        L.ptr(src), int(u8), nimg, Hh, Ww, c, h, w, _spec(scales, symmetries), L.ptr(cd), seed, offset, n, lo, hi,
        L.ptr(out) if "f32" in want else None, L.ptr(out8) if use8 else None, L.ptr(meta) if "meta" in want else None,
        L.stream_ptr()))
    torch.cuda.synchronize()
    got, got8, gotm = chk(), chk8(), chkm()
    if "f32" not in want:
        assert np.isnan(got).all()
    if not use8:
        assert (got8 == 0xA5).all()
    assert src.cpu().numpy().tobytes() == np.ascontiguousarray(img).tobytes()
    return dict(target=got.reshape(n, h, w, c) if "f32" in want else None,
                target_u8=got8.reshape(n, h, w, c) if use8 else None,
                meta=gotm.reshape(n, 5) if "meta" in want else None)


def _same(got, ref):
    """Bitwise equality (torch.equal on the bytes) of every output the launch produced."""
    for key in ("target", "target_u8", "meta"):
        if got[key] is None:
            continue
        a = torch.from_numpy(np.ascontiguousarray(got[key])).reshape(-1).view(torch.uint8)
        b = torch.from_numpy(np.ascontiguousarray(ref[key])).reshape(-1).view(torch.uint8)
        assert a.numel() == b.numel() and torch.equal(a, b), key


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "peel"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h,w,sym", [(8, 8, 8), (8, 12, 4)], ids=["8x8-dihedral", "8x12-mirrors"])
def test_drawn_crops_are_bitwise(h, w, sym, c, shift, u8):
    """nimg = 3, H = 37, W = 53, n = 16, scales (1, 2, 3); ``peel``: the images start 1 byte (uint8) or 4 bytes (fp32)
    past a 16-byte boundary, so no source row is aligned."""
    img = _images(NIMG, H, W, c, u8)
    kw = dict(scales=(1, 2, 3), symmetries=sym, n=16, seed=0xC0FFEE1234, offset=(1 << 32) - 5)
    got = _crop(img, h, w, src_shift=shift, **kw)
    ref = cr.crop_batch(img, h, w, lo=LO, hi=HI, **kw)
    _same(got, ref)
    assert len(set(ref["meta"][:, 1].tolist())) == 3 and len(set(ref["meta"][:, 2].tolist())) > sym // 2


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
@pytest.mark.parametrize("out_shift", [0, 1], ids=["aligned", "output_off"])
def test_corners_at_the_largest_scale_and_every_symmetry(u8, out_shift):
    h = w = 8
    s = 3
    img = _images(NIMG, H, W, 3, u8, seed=1)
    corners = [(0, 0), (0, W - s * w), (H - s * h, 0), (H - s * h, W - s * w)]
    # (the first image's first pixel and the last image's last: the ends of the buffer, where the kernel peels)
    crops = [((0, 1, 1, NIMG - 1)[k], s, g, y0, x0) for k, (y0, x0) in enumerate(corners) for g in range(8)]
    got = _crop(img, h, w, scales=(1, 2, 3), symmetries=8, n=len(crops), crops=crops, src_shift=1, out_shift=out_shift)
    _same(got, cr.crop_batch(img, h, w, n=len(crops), crops=crops, lo=LO, hi=HI))
    np.testing.assert_array_equal(got["meta"], np.asarray(crops, np.int32))


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
def test_a_tile_equal_to_the_image(u8):
    img = _images(NIMG, 8, 12, 3, u8, seed=2)
    kw = dict(scales=(1,), symmetries=4, n=16, seed=3, offset=0)
    got = _crop(img, 8, 12, **kw)
    ref = cr.crop_batch(img, 8, 12, lo=LO, hi=HI, **kw)
    _same(got, ref)
    assert (ref["meta"][:, 3:] == 0).all() and set(ref["meta"][:, 0].tolist()) == {0, 1, 2}


# (h, w, scales, symmetries): several 32 x 32 blocks per row with ragged edges; the same transposed; 16 x 16 blocks
BLOCKS = [(40, 36, (1, 2), 4), (40, 40, (1, 2), 8), (20, 20, (1, 4), 8)]


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
@pytest.mark.parametrize("h,w,scales,sym", BLOCKS, ids=["40x36", "40x40", "20x20-s4"])
def test_rows_of_several_blocks_are_bitwise(h, w, scales, sym, u8):
    img = _images(2, 90, 101, 3, u8, seed=3)
    kw = dict(scales=scales, symmetries=sym, n=12, seed=11, offset=5)
    got = _crop(img, h, w, src_shift=1, **kw)
    ref = cr.crop_batch(img, h, w, lo=LO, hi=HI, **kw)
    _same(got, ref)
    assert set(ref["meta"][:, 1].tolist()) == set(scales)


@pytest.fixture(scope="module")
def large():
    """tile 64 x 64 x 3 at s = 8 of two 520 x 520 images: (images, kw, reference) per dtype, computed once."""
    cache = {}

    def get(u8):
        if u8 not in cache:
            img = _images(2, 520, 520, 3, u8, seed=4)
            crops = [(1, 8, 7, 8, 8), (0, 8, 0, 0, 3), (1, 8, 5, 3, 0), (0, 8, 2, 1, 7)]
            cache[u8] = (img, crops, cr.crop_batch(img, 64, 64, n=len(crops), crops=crops, lo=LO, hi=HI))
        return cache[u8]
    return get


@pytest.mark.parametrize("u8", [True, False], ids=["uint8-lds", "fp32-global"])
def test_the_largest_patch_is_bitwise_on_both_paths(u8, large):
    """At s = 8 and three channels the patch of a 16 x 16 tile is 128 rows of 384 elements: 50 KB of uint8, which is
    staged, and 194 KB of fp32, which is not (the fallback: every block reduces from global memory).  Both are held to
    the one contract through the reference; the uint8 images with the listed scale 1 and explicit crops at s = 8 take
    the fallback too (a block whose patch exceeds what the launch reserved), and give the staged path's bytes."""
    img, crops, ref = large(u8)
    got = _crop(img, 64, 64, scales=(8,), symmetries=8, n=len(crops), crops=crops, src_shift=1)
    _same(got, ref)
    if u8:
        unstaged = _crop(img, 64, 64, scales=(1,), symmetries=8, n=len(crops), crops=crops, src_shift=1)
        _same(unstaged, ref)
        assert unstaged["target"].tobytes() == got["target"].tobytes()


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
def test_plain_crops_equal_make_batch_on_the_sliced_tiles(u8):
    L = pkg_mod("_lib")
    h, w, c, n = 8, 12, 3, 16
    img = _images(NIMG, H, W, c, u8, seed=5)
    rng = np.random.default_rng(0)
    crops = [(int(rng.integers(NIMG)), 1, 0, int(rng.integers(H - h + 1)), int(rng.integers(W - w + 1))) for _ in range(n)]
    got = _crop(img, h, w, n=n, crops=crops, src_shift=1)
    tiles = np.stack([img[m, y:y + h, x:x + w] for m, _, _, y, x in crops])
    d = torch.from_numpy(tiles).cuda()
    out = torch.empty([n, h, w, c], dtype=torch.float32, device="cuda")
    L.check(L.lib().svae_op_make_batch(L.ptr(d), int(u8), None, 0, n, h * w * c, LO, HI, 0.0, 0.0, 0.0, 0, 0, L.ptr(out),
                                       None, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(got["target"]).view(torch.int32), out.cpu().view(torch.int32))
    if u8:
        np.testing.assert_array_equal(got["target_u8"], tiles)


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
def test_two_calls_and_a_split_call_give_the_same_bytes(u8):
    img = _images(NIMG, H, W, 3, u8, seed=6)
    kw = dict(scales=(1, 2, 3), symmetries=8, seed=21)
    o, n1, n = (1 << 40) + 3, 6, 16
    whole = _crop(img, 8, 8, n=n, offset=o, **kw)
    again = _crop(img, 8, 8, n=n, offset=o, src_shift=1, out_shift=1, **kw)
    first = _crop(img, 8, 8, n=n1, offset=o, **kw)
    rest = _crop(img, 8, 8, n=n - n1, offset=o + n1, **kw)
    for key in ("target", "meta") + (("target_u8",) if u8 else ()):
        assert whole[key].tobytes() == again[key].tobytes(), key
        assert whole[key].tobytes() == np.concatenate([first[key], rest[key]]).tobytes(), key


@pytest.mark.parametrize("want", [("f32",), ("u8",), ("f32", "u8"), ("f32", "meta")], ids="+".join)
def test_only_the_outputs_asked_for_are_written(want):
    img = _images(NIMG, H, W, 3, True, seed=7)
    kw = dict(scales=(1, 2), symmetries=2, n=5, seed=8, offset=9)
    _same(_crop(img, 8, 12, want=want, **kw), cr.crop_batch(img, 8, 12, lo=LO, hi=HI, **kw))


def _bad(over=None, u8=True, spec=((1, 2), 4), outputs=("f32",), null=()):
    """The return code of a call on 2 images of 16 x 20 x 3 (tile 8 x 8, n = 4) with the arguments ``over`` replaces;
    a refused call has written nothing."""
    L = pkg_mod("_lib")
    a = dict(nimg=2, H=16, W=20, c=3, h=8, w=8, n=4, lo=LO, hi=HI)
    a.update(over or {})
    img = torch.zeros(2 * 16 * 20 * 3, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    out, chk = _guarded(4 * 8 * 8 * 3, torch.float32)
    out8, chk8 = _guarded(4 * 8 * 8 * 3, torch.uint8)
    sc = tuple(spec[0])
    sp = L.SvaeCropSpec(len(sc), (ctypes.c_int32 * 4)(*(sc + (0,) * (4 - len(sc)))), spec[1])
    rc = L.lib().svae_op_crop_batch(
        None if "images" in null else L.ptr(img), int(u8), a["nimg"], a["H"], a["W"], a["c"], a["h"], a["w"],
        None if "spec" in null else sp, None, 1, 2, a["n"], a["lo"], a["hi"], L.ptr(out) if "f32" in outputs else None,
        L.ptr(out8) if "u8" in outputs else None, None, L.stream_ptr())
    torch.cuda.synchronize()
    if rc != 0:
        assert np.isnan(chk()).all() and (chk8() == 0xA5).all(), "a refused call launched"
        assert L.lib().svae_last_error(None)
    return rc


BAD_ARGS = [
    dict(null=("images",)), dict(null=("spec",)), dict(outputs=()),
    dict(u8=False, outputs=("f32", "u8")),          # target_u8 with fp32 images
    dict(over=dict(nimg=0)), dict(over=dict(H=0)), dict(over=dict(W=-1)), dict(over=dict(c=0)), dict(over=dict(h=0)),
    dict(over=dict(w=0)), dict(over=dict(n=0)),
    dict(spec=((), 1)),
    dict(spec=((0,), 1)), dict(spec=((9,), 1)), dict(spec=((1, 2, 1), 1)),
    dict(spec=((1, 3), 1)),                         # 3 * 8 > 16 = H
    dict(over=dict(w=11), spec=((1, 2), 1)),        # 2 * 11 > 20 = W
    dict(spec=((1,), 3)), dict(spec=((1,), 0)), dict(spec=((1,), 16)),
    dict(over=dict(w=10), spec=((1,), 8)),          # the dihedral group with h != w
    dict(over=dict(lo=1.0, hi=1.0)), dict(over=dict(lo=2.0, hi=1.0)),
    dict(over=dict(lo=1.0, hi=1.0), outputs=("u8",)),
]


def test_bad_arguments_are_refused_before_any_launch():
    assert _bad() == 0 and _bad(outputs=("u8",)) == 0 and _bad(u8=False) == 0
    assert _bad(dict(w=10), spec=((1, 2), 1)) == 0           # 2 * 10 <= 20 = W is legal
    assert _bad(dict(lo=1.0, hi=1.0), u8=False) == 0         # lo >= hi matters only with a uint8 side
    for case in BAD_ARGS:
        assert _bad(**case) == EBADARG, case
    # sizes: H W c beyond 2^31 - 1 (nothing is launched, so the small buffer is never read)
    assert _bad(dict(H=65536, W=65536, c=1)) == EBADCONFIG
    assert _bad(dict(H=46341, W=46341, c=1, h=46341, w=46341), spec=((1,), 1)) == EBADCONFIG


def test_python_wrapper_draws_checks_and_counts():
    C = pkg_mod("crops")
    img = _images(NIMG, H, W, 3, True, seed=9)
    d = torch.from_numpy(img).cuda()
    spec = C.CropSpec((1, 2, 3), 8)
    before = C.calls
    meta = torch.empty([16, 5], dtype=torch.int32, device="cuda")
    out = C.crop_batch(d, (8, 8), spec, 16, seed=4, offset=6, range=(LO, HI), meta=meta)
    ref = cr.crop_batch(img, 8, 8, (1, 2, 3), 8, 4, 6, 16, LO, HI)
    assert C.calls == before + 1 and tuple(out.shape) == (16, 8, 8, 3)
    _same(dict(target=out.cpu().numpy(), target_u8=None, meta=meta.cpu().numpy()), ref)
    out8 = torch.empty([16, 8, 8, 3], dtype=torch.uint8, device="cuda")
    assert C.crop_batch(d, (8, 8), spec, crops=meta, range=(LO, HI), out_u8=out8) is out8
    np.testing.assert_array_equal(out8.cpu().numpy(), ref["target_u8"])
    with pytest.raises(ValueError, match="out of range"):
        C.crop_batch(d, (8, 8), spec, crops=[(0, 3, 0, H - 24 + 1, 0)])
    with pytest.raises(ValueError, match="out of range"):
        C.crop_batch(d, (8, 12), spec, crops=[(0, 1, 4, 0, 0)])  # a transposition of a tile that is not square
    with pytest.raises(ValueError):
        C.CropSpec((1, 1), 1)
    assert C.calls == before + 2
