"""The tile geometry and the numpy restatement of svae_op_extract_tiles / svae_op_blend_tiles
(tests/tiles_ref.py) against their contract, the package's TileGrid against the restatement, and the host-side
argument checks of the two entry points: no GPU."""
import ctypes

import numpy as np
import pytest

import tiles_ref as tr
from conftest import pkg_mod

# (L, t, s): L == t, s == t, s == 1, (L - t) % s != 0, and mixtures of them
SWEEP = [(4, 4, 4), (4, 4, 1), (9, 5, 2), (7, 4, 3), (6, 4, 1), (32, 32, 16), (80, 32, 16), (72, 32, 16),
         (10, 5, 5), (11, 5, 5), (13, 4, 4), (64, 64, 32), (100, 64, 32), (5, 1, 1), (17, 6, 4), (20, 7, 7)]
# the shapes of tests/test_tiles_gpu.py
SHAPES = [(2, 7, 9, 3, 4, 5, 3, 2), (1, 32, 32, 3, 32, 32, 32, 32), (3, 32, 32, 1, 32, 32, 16, 16),
          (1, 6, 6, 1, 4, 4, 1, 1), (1, 80, 72, 3, 32, 32, 16, 16)]


@pytest.mark.parametrize("L,t,s", SWEEP)
def test_every_pixel_is_covered_and_origins_do_not_decrease(L, t, s):
    o = tr.origins(L, t, s)
    assert len(o) == tr.count(L, t, s) == -(-(L - t) // s) + 1
    assert o[0] == 0 and all(a <= b for a, b in zip(o, o[1:]))
    assert all(0 <= a and a + t <= L for a in o)
    for x in range(L):
        assert tr.covering(x, L, t, s), x


@pytest.mark.parametrize("L,t,s", SWEEP)
def test_last_origin_is_the_edge_and_covering_sets_are_contiguous(L, t, s):
    o = tr.origins(L, t, s)
    assert o[-1] == L - t
    if len(o) > 1:
        assert o[-2] < L - t  # no tile is superfluous: the one before the last does not reach the edge
    for x in range(L):
        c = tr.covering(x, L, t, s)
        assert c == list(range(c[0], c[-1] + 1)), (x, c)
        assert len(c) <= -(-t // s) + 1
    assert [tr.w1(p, t) for p in range(t)] == [tr.w1(t - 1 - p, t) for p in range(t)]
    assert tr.w1(0, t) == 1 and max(tr.w1(p, t) for p in range(t)) == (t + 1) // 2


@pytest.mark.parametrize("shape", SHAPES + [(2, L, L + 3, 2, t, t, s, s) for L, t, s in SWEEP if L + 3 >= t])
def test_tilegrid_agrees_with_the_restatement(shape):
    nimg, H, W, c, th, tw, sy, sx = shape
    g = pkg_mod("restore").TileGrid(*shape)
    assert (g.ky, g.kx) == (tr.count(H, th, sy), tr.count(W, tw, sx))
    assert g.n_tiles == tr.n_tiles(nimg, H, W, th, tw, sy, sx)
    assert g.oy.tolist() == tr.origins(H, th, sy) and g.ox.tolist() == tr.origins(W, tw, sx)
    assert g.w1y.tolist() == [tr.w1(p, th) for p in range(th)] and g.w1x.tolist() == [tr.w1(q, tw) for q in range(tw)]
    assert g.weight().shape == (th, tw) and g.weight()[1 % th, 0] == tr.w1(1 % th, th)
    for tid in range(g.n_tiles):
        m, i, j = g.tile(tid)
        assert g.tile_id(m, i, j) == tid
        assert (m, int(g.oy[i]), int(g.ox[j])) == tr.tile_of(tid, nimg, H, W, th, tw, sy, sx)
    for y in range(H):
        assert g.covering(0, y) == tr.covering(y, H, th, sy)
    for x in range(W):
        assert g.covering(1, x) == tr.covering(x, W, tw, sx)


def test_tilegrid_refuses_bad_geometry_and_windows_follow_the_rule():
    R = pkg_mod("restore")
    for bad in [(1, 4, 4, 1, 5, 4, 1, 1), (1, 4, 4, 1, 4, 5, 1, 1), (1, 4, 4, 1, 2, 2, 3, 1), (1, 4, 4, 1, 2, 2, 1, 0),
                (0, 4, 4, 1, 2, 2, 1, 1), (1, 4, 4, 0, 2, 2, 1, 1)]:
        with pytest.raises(ValueError):
            R.TileGrid(*bad)
    assert R.windows(16, 4) == [(0, 4, 4), (4, 4, 4), (8, 4, 4), (12, 4, 4)]
    assert R.windows(6, 4) == [(0, 4, 4), (2, 4, 2)]
    assert R.windows(1, 4) == [(0, 4, 1)]
    assert R.windows(961, 128)[-1] == (833, 128, 65) and len(R.windows(961, 128)) == 8


@pytest.mark.parametrize("shape", SHAPES)
def test_identity_a_blend_of_extract_is_the_image_bitwise(shape):
    nimg, H, W, c, th, tw, sy, sx = shape
    rng = np.random.default_rng(sum(shape))
    img = (rng.standard_normal((nimg, H, W, c)) * np.exp(rng.uniform(-20, 20, (nimg, H, W, c)))).astype(np.float32)
    tiles = tr.extract(img, th, tw, sy, sx)
    assert tiles.shape == (tr.n_tiles(nimg, H, W, th, tw, sy, sx), th, tw, c)
    out, _ = tr.blend(tiles[None], nimg, H, W, c, th, tw, sy, sx)
    np.testing.assert_array_equal(out[0].view(np.int32), img.view(np.int32))


@pytest.mark.parametrize("lo,hi", [(-1.0, 1.0), (0.0, 1.0)])
def test_identity_b_every_byte_survives_extract_and_blend(lo, hi):
    img = np.arange(256, dtype=np.uint8).reshape(1, 8, 32, 1)
    img = np.concatenate([img, img[:, ::-1, ::-1]], axis=3)
    np.testing.assert_array_equal(tr.quant(tr.dequant(np.arange(256, dtype=np.uint8), lo, hi), lo, hi), np.arange(256))
    tiles = tr.extract(img, 5, 12, 2, 7, lo, hi)
    out, out_u8 = tr.blend(tiles[None], 1, 8, 32, 2, 5, 12, 2, 7, lo=lo, hi=hi)
    np.testing.assert_array_equal(out_u8[0], img)
    np.testing.assert_array_equal(out[0], tr.dequant(img, lo, hi))


def test_restatement_wraps_masks_and_weighs():
    img = np.random.default_rng(5).uniform(-1, 1, (2, 7, 9, 3)).astype(np.float32)
    n = tr.n_tiles(2, 7, 9, 4, 5, 3, 2)
    assert n == 2 * 2 * 3
    full = tr.extract(img, 4, 5, 3, 2)
    wrapped = tr.extract(img, 4, 5, 3, 2, first=n - 2, cnt=n + 3)
    np.testing.assert_array_equal(wrapped, np.concatenate([full[n - 2:], full, full[:1]]))
    # two different constant tiles over one pixel: the window-weighted mean
    tiles = np.stack([np.full((4, 4, 1), 1.0, np.float32), np.full((4, 4, 1), 3.0, np.float32)])
    out, _ = tr.blend(tiles[None], 1, 4, 6, 1, 4, 4, 4, 2)
    assert out[0, 0, 0, 0, 0] == 1.0 and out[0, 0, 0, 5, 0] == 3.0
    assert out[0, 0, 0, 2, 0] == np.float32((2 * 1.0 + 1 * 3.0) / 3)  # x = 2: w1(2) = 2 in tile 0, w1(0) = 1 in tile 1
    known = np.zeros((1, 4, 6), np.uint8)
    known[0, 1, 2] = 7
    src = np.full((1, 4, 6, 1), 200, np.uint8)
    out, out_u8 = tr.blend(tiles[None], 1, 4, 6, 1, 4, 4, 4, 2, source=src, known=known)
    assert out_u8[0, 0, 1, 2, 0] == 200 and out[0, 0, 1, 2, 0] == tr.dequant(np.uint8(200), -1.0, 1.0)
    assert out[0, 0, 0, 2, 0] == np.float32(5.0 / 3) and out_u8[0, 0, 0, 2, 0] == 255


def test_entry_points_are_exported_and_bound(built_lib):
    L = pkg_mod("_lib")
    for name in ("svae_op_extract_tiles", "svae_op_blend_tiles"):
        assert name in L.EXPORTED
        assert hasattr(ctypes.CDLL(built_lib), name)
        assert getattr(L.lib(), name).restype is ctypes.c_int32
    assert "tiles.hip" in pkg_mod("build").SOURCES


def test_restore_imports_without_a_gpu():
    R = pkg_mod("restore")
    assert callable(R.extract_tiles) and callable(R.blend_tiles) and callable(R.restore)
    assert callable(pkg_mod("sequential_vae").SequentialVAE.restore)


def test_extract_tiles_rejects_bad_arguments_without_a_gpu(built_lib):
    """SVAE_EBADARG (-2) for every case include/svae_hip.h lists, before any device call: the pointers are never
    dereferenced."""
    lib = pkg_mod("_lib").lib()
    p = ctypes.c_void_p(4096)
    # images, data_u8, nimg, H, W, c, th, tw, sy, sx, lo, hi, first, count, tiles, stream: 2 x 2 x 3 = 12 tiles
    good = [p, 1, 2, 7, 9, 3, 4, 5, 3, 2, -1.0, 1.0, 0, 12, p, None]
    cases = [(0, None), (14, None)]                                          # a null pointer
    cases += [(i, v) for i in (2, 3, 4, 5, 6, 7, 8, 9, 13) for v in (0, -1)]  # a count, extent or stride <= 0
    cases += [(6, 8), (7, 10), (8, 5), (9, 6)]                               # th > H, tw > W, sy > th, sx > tw
    cases += [(12, -1), (12, 12), (12, 13)]                                  # first outside [0, n_tiles)
    cases += [(11, -1.0), (11, -2.0), (11, float("nan"))]                    # lo >= hi with uint8 images
    for i, bad in cases:
        args = list(good)
        args[i] = bad
        assert lib.svae_op_extract_tiles(*args) == -2, (i, bad)
        assert b"extract_tiles" in lib.svae_last_error(None)


def test_blend_tiles_rejects_bad_arguments_without_a_gpu(built_lib):
    lib = pkg_mod("_lib").lib()
    p = ctypes.c_void_p(4096)
    # tiles, nstack, stack_stride, nimg, H, W, c, th, tw, sy, sx, source, source_u8, known, lo, hi, out, out_u8, stream
    good = [p, 2, 12 * 60, 2, 7, 9, 3, 4, 5, 3, 2, p, 1, p, -1.0, 1.0, p, p, None]

    def call(changes):
        args = list(good)
        for i, v in changes:
            args[i] = v
        return lib.svae_op_blend_tiles(*args)

    cases = [[(0, None)], [(16, None), (17, None)]]                          # null tiles, both outputs null
    cases += [[(11, None)], [(13, None)]]                                    # known without source and the reverse
    cases += [[(i, v)] for i in (1, 3, 4, 5, 6, 7, 8, 9, 10) for v in (0, -1)]
    cases += [[(7, 8)], [(8, 10)], [(9, 5)], [(10, 6)]]                      # th > H, tw > W, sy > th, sx > tw
    cases += [[(2, 12 * 60 - 1)], [(2, 0)], [(2, -5)]]                       # stack_stride below a set
    cases += [[(15, -1.0)], [(15, float("nan"))]]                            # lo >= hi: uint8 output and source
    cases += [[(15, -1.0), (17, None)]]                                      # ... uint8 source alone
    cases += [[(15, -1.0), (11, None), (13, None), (16, None)]]              # ... uint8 output alone
    for ch in cases:
        assert call(ch) == -2, ch
        assert b"blend_tiles" in lib.svae_last_error(None)
