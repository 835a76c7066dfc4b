"""svae_op_extract_tiles and svae_op_blend_tiles (csrc/tiles.hip) against their numpy restatement
(tests/tiles_ref.py), bit for bit: the extraction is a copy or an fp32 dequantisation with stated roundings, the
blend is fp64 in a stated order with one division and one cast, the quantiser is fp32 with stated roundings.
Every output sits between NaN (uint8: 0xA5) guard bands that must survive."""
import numpy as np
import pytest
import torch

import tiles_ref as tr
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
GUARD = 64
# (nimg, H, W, c, th, tw, sy, sx)
SHAPES = [(2, 7, 9, 3, 4, 5, 3, 2),          # odd sizes, clamped last tile on both axes, nothing aligned
          (1, 32, 32, 3, 32, 32, 32, 32),    # one tile
          (3, 32, 32, 1, 32, 32, 16, 16),    # one tile per image, one channel
          (1, 6, 6, 1, 4, 4, 1, 1),          # dense stride
          (1, 80, 72, 3, 32, 32, 16, 16)]    # 4 x 4 tiles, the last column clamped


def _images(shape, u8):
    nimg, H, W, c = shape[:4]
    rng = np.random.default_rng(sum(shape) + int(u8))
    if u8:
        return rng.integers(0, 256, (nimg, H, W, c), dtype=np.uint8)
    return rng.uniform(-1, 1, (nimg, H, W, c)).astype(np.float32)


def _to_device(a, shift=0):
    """The array on the device, its first element ``shift`` elements past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[shift:shift + t.numel()]
    d.copy_(t)
    assert d.data_ptr() % 16 == (shift * t.element_size()) % 16
    return d


def _guarded(n, dtype, shift):
    """(whole buffer, the n-element output inside it ``shift`` elements past a 16-byte boundary, check)."""
    fill = float("nan") if dtype == torch.float32 else 0xA5
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD + per16,), fill, dtype=dtype, device="cuda")
    a = GUARD + shift
    assert buf.data_ptr() % 16 == 0 and GUARD % per16 == 0

    def check():
        h = buf.cpu().numpy()
        ok = np.isnan(h[:a]).all() and np.isnan(h[a + n:]).all() if dtype == torch.float32 else \
            (h[:a] == 0xA5).all() and (h[a + n:] == 0xA5).all()
        assert ok, "wrote outside the output"
        return h[a:a + n]
    return buf, buf[a:a + n], check


def _extract(img, shape, first=0, count=None, src_shift=0, out_shift=0, lo=LO, hi=HI):
    L = pkg_mod("_lib")
    nimg, H, W, c, th, tw, sy, sx = shape
    n = tr.n_tiles(nimg, H, W, th, tw, sy, sx)
    count = n if count is None else count
    src = _to_device(img, src_shift)
    _, out, check = _guarded(count * th * tw * c, torch.float32, out_shift)
    L.check(L.lib().svae_op_extract_tiles(L.ptr(src), int(img.dtype == np.uint8), *shape, lo, hi, first, count,
                                          L.ptr(out), L.stream_ptr()))
    torch.cuda.synchronize()
    return check().reshape(count, th, tw, c)


def _blend(tiles, shape, source=None, known=None, want=("f32", "u8"), tiles_shift=0, out_shift=0, stride=None,
           lo=LO, hi=HI):
    """tiles: numpy [nstack, n_tiles, th, tw, c], or with ``stride`` the flat float array of the sets as they lie."""
    L = pkg_mod("_lib")
    nimg, H, W, c, th, tw, sy, sx = shape
    nstack = tiles.shape[0] if stride is None else (tiles.size - tr.n_tiles(nimg, H, W, th, tw, sy, sx) * th * tw * c) // stride + 1
    set_elems = tr.n_tiles(nimg, H, W, th, tw, sy, sx) * th * tw * c
    t = _to_device(tiles, tiles_shift)
    n = nstack * nimg * H * W * c
    _, out, check = _guarded(n, torch.float32, out_shift)
    _, out8, check8 = _guarded(n, torch.uint8, 4 * out_shift)  # 4 bytes past a 16-byte boundary, as out
    src = None if source is None else _to_device(source)
    kn = None if known is None else _to_device(known)
    L.check(L.lib().svae_op_blend_tiles(
        L.ptr(t), nstack, set_elems if stride is None else stride, *shape, L.ptr(src),
        int(source is not None and source.dtype == np.uint8), L.ptr(kn), lo, hi,
        L.ptr(out) if "f32" in want else None, L.ptr(out8) if "u8" in want else None, L.stream_ptr()))
    torch.cuda.synchronize()
    got, got8 = check(), check8()
    if "f32" not in want:
        assert np.isnan(got).all()
    if "u8" not in want:
        assert (got8 == 0xA5).all()
    tiles_after = t.cpu().numpy()
    return got.reshape(nstack, nimg, H, W, c), got8.reshape(nstack, nimg, H, W, c), tiles_after


def _bitwise(got, ref):
    np.testing.assert_array_equal(got.view(np.int32), np.asarray(ref, dtype=np.float32).view(np.int32))


def _random_tiles(shape, nstack, seed=0):
    nimg, H, W, c, th, tw, sy, sx = shape
    n = tr.n_tiles(nimg, H, W, th, tw, sy, sx)
    return np.random.default_rng(seed + sum(shape)).uniform(-1.2, 1.2, (nstack, n, th, tw, c)).astype(np.float32)


@pytest.fixture(scope="module")
def blend_refs():
    """shape -> (tiles [2, n_tiles, th, tw, c], the restatement's out, out_u8), computed once."""
    cache = {}

    def get(shape):
        if shape not in cache:
            tiles = _random_tiles(shape, 2)
            cache[shape] = (tiles,) + tr.blend(tiles, *shape)
        return cache[shape]
    return get


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
@pytest.mark.parametrize("align", ["aligned", "source_off", "output_off"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_extract_is_bitwise(shape, align, u8):
    img = _images(shape, u8)
    got = _extract(img, shape, src_shift=1 if align == "source_off" else 0, out_shift=1 if align == "output_off" else 0)
    _bitwise(got, tr.extract(img, *shape[4:], LO, HI))


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
def test_extract_wraps_around(u8):
    shape = SHAPES[0]
    n = tr.n_tiles(*shape[:3], *shape[4:])
    img = _images(shape, u8)
    got = _extract(img, shape, first=n - 2, count=n + 3)
    _bitwise(got, tr.extract(img, *shape[4:], LO, HI, first=n - 2, cnt=n + 3))
    again = _extract(img, shape, first=n - 2, count=n + 3)
    assert got.tobytes() == again.tobytes()


@pytest.mark.parametrize("align", ["aligned", "source_off", "output_off"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_blend_is_bitwise(shape, align, blend_refs):
    tiles, ref, ref8 = blend_refs(shape)
    out, out8, _ = _blend(tiles, shape, tiles_shift=1 if align == "source_off" else 0,
                          out_shift=1 if align == "output_off" else 0)
    _bitwise(out, ref)
    np.testing.assert_array_equal(out8, ref8)
    if shape == SHAPES[4]:  # the quantiser's clamp is exercised on both sides
        assert len(np.unique(ref8)) > 100 and ref8.min() == 0 and ref8.max() == 255 and ref.min() < -1 and ref.max() > 1


@pytest.mark.parametrize("nstack", [2, 4])
def test_blend_with_many_blocks_is_bitwise(nstack):
    """The shapes above are small enough for one output row per block (csrc/tiles.hip halves a block's band of 8 rows
    while the launch has under 1 024 blocks); here 1 280 blocks own 4 rows (nstack = 2) and 8 rows (nstack = 4)."""
    shape = (64, 40, 36, 1, 16, 16, 8, 8)
    tiles = _random_tiles(shape, nstack, seed=nstack)
    ref, ref8 = tr.blend(tiles, *shape)
    out, out8, _ = _blend(tiles, shape)
    _bitwise(out, ref)
    np.testing.assert_array_equal(out8, ref8)


@pytest.mark.parametrize("want", [("f32",), ("u8",), ("f32", "u8")], ids=["out", "out_u8", "both"])
def test_blend_writes_the_outputs_asked_for(want, blend_refs):
    shape = SHAPES[0]
    tiles, ref, ref8 = blend_refs(shape)
    out, out8, _ = _blend(tiles, shape, want=want)
    if "f32" in want:
        _bitwise(out, ref)
    if "u8" in want:
        np.testing.assert_array_equal(out8, ref8)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]], ids=str)
def test_blend_stacks_with_a_gap_between_the_sets(shape):
    """nstack = 3 with stack_stride 37 floats above a set: the NaN in the gaps neither enters the result nor is
    overwritten."""
    tiles = _random_tiles(shape, 3, seed=9)
    set_elems = tiles[0].size
    stride = set_elems + 37
    flat = np.full(2 * stride + set_elems, np.nan, np.float32)
    for k in range(3):
        flat[k * stride:k * stride + set_elems] = tiles[k].reshape(-1)
    ref, ref8 = tr.blend(tiles, *shape)
    out, out8, after = _blend(flat, shape, stride=stride)
    assert out.shape[0] == 3
    _bitwise(out, ref)
    np.testing.assert_array_equal(out8, ref8)
    assert after.tobytes() == flat.tobytes()


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=str)
def test_known_pixels_are_the_source(shape, u8):
    nimg, H, W, c = shape[:4]
    tiles = _random_tiles(shape, 2, seed=3)
    src = _images(shape, u8)
    known = (np.random.default_rng(11).uniform(size=(nimg, H, W)) < 0.4).astype(np.uint8) * 3
    ref, ref8 = tr.blend(tiles, *shape, source=src, known=known)
    out, out8, _ = _blend(tiles, shape, source=src, known=known)
    _bitwise(out, ref)
    np.testing.assert_array_equal(out8, ref8)
    k = known.astype(bool)
    assert k.any() and not k.all()
    for s in range(2):
        _bitwise(out[s][k], tr.as_float(src, LO, HI)[k])
        if u8:
            np.testing.assert_array_equal(out8[s][k], src[k])
    free, _ = tr.blend(tiles, *shape)
    _bitwise(out[:, ~k], free[:, ~k])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identity_a_on_the_device(shape):
    rng = np.random.default_rng(sum(shape))
    img = (rng.standard_normal(shape[:4]) * np.exp(rng.uniform(-20, 20, shape[:4]))).astype(np.float32)
    tiles = _extract(img, shape)
    out, _, _ = _blend(tiles[None], shape, want=("f32",))
    _bitwise(out[0], img)


@pytest.mark.parametrize("lo,hi", [(-1.0, 1.0), (0.0, 1.0)])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identity_b_on_the_device(shape, lo, hi):
    img = _images(shape, True)
    img.reshape(-1)[:256] = np.arange(256)[:img.size]  # every byte value where the image holds 256 pixels
    tiles = _extract(img, shape, lo=lo, hi=hi)
    out, out8, _ = _blend(tiles[None], shape, lo=lo, hi=hi)
    np.testing.assert_array_equal(out8[0], img)
    _bitwise(out[0], tr.dequant(img, lo, hi))


def test_two_calls_give_the_same_bytes(blend_refs):
    shape = SHAPES[4]
    tiles = blend_refs(shape)[0]
    a, a8, _ = _blend(tiles, shape)
    b, b8, _ = _blend(tiles, shape)
    assert a.tobytes() == b.tobytes() and a8.tobytes() == b8.tobytes()


def test_python_wrappers_round_trip_on_the_current_stream():
    R = pkg_mod("restore")
    shape = SHAPES[4]
    g = R.TileGrid(*shape)
    img = _images(shape, True)
    d = torch.from_numpy(img).cuda()
    tiles = R.extract_tiles(d, g, range=(LO, HI))
    assert tuple(tiles.shape) == (g.n_tiles, g.th, g.tw, g.C)
    _bitwise(tiles.cpu().numpy(), tr.extract(img, *shape[4:], LO, HI))
    out, out8 = R.blend_tiles(tiles, g, as_uint8=True)
    assert out is None and out8.dtype == torch.uint8 and tuple(out8.shape) == (1,) + img.shape
    np.testing.assert_array_equal(out8[0].cpu().numpy(), img)
    known = torch.zeros(img.shape[:3], dtype=torch.bool, device="cuda")
    known[0, 3:9, 5:50] = True
    out, _ = R.blend_tiles(torch.zeros_like(tiles), g, source=d, known=known)
    ref = np.where(known.cpu().numpy()[..., None], tr.dequant(img, LO, HI), np.float32(0))
    _bitwise(out[0].cpu().numpy(), ref)
