"""SequentialVAE.restore on the GPU: preset ``tiny`` (B = 4, 32x32x3, T = 3, fp32).

Every result is recomputed here from the specification on an identically initialised network: the restatement's
extraction (tests/tiles_ref.py), the windows written out below, forward(inp, inp, eps, 1.0, noise) with the stated
eps, x_hat_t, the restatement's blend.  Both sides run the same forwards in the same order and the engine's
forward is reproducible (tests/test_checkpoint_gpu.py relies on it), so the comparison is bitwise."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import tiles_ref as tr
from conftest import ROOT, pkg_mod

pytestmark = pytest.mark.gpu

B, H, W, C, T = 4, 32, 32, 3, 3
LO, HI = -1.0, 1.0
STRIDE = 16


def _net(preset="tiny", seed=0):
    cfg = pkg_mod("config").preset(preset, batch=B, dtype="fp32")
    assert (cfg.height, cfg.width, cfg.channels, cfg.mc_steps) == (H, W, C, T)
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _images(n, h, w, seed=1):
    """Smooth uint8 images with some noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 90 * np.sin(yy / (5.0 + k) + m) * np.cos(xx / (7.0 - k) + 2 * m) for m in range(n)
                    for k in range(C)]).reshape(n, C, h, w).transpose(0, 2, 3, 1)
    return np.clip(img + rng.uniform(-20, 20, img.shape), 0, 255).astype(np.uint8)


def _recompute(img, windows, seed=None, preset="tiny", known=None):
    """(out [T,N,H,W,C] fp32, out_u8) by the specification; ``windows`` = [(first, rows not yet produced)]."""
    net = _net(preset)
    n_img, h, w, _ = img.shape
    geom = (n_img, h, w, C, H, W, STRIDE, STRIDE)
    n = tr.n_tiles(n_img, h, w, H, W, STRIDE, STRIDE)
    tiles = tr.extract(img, H, W, STRIDE, STRIDE, LO, HI)
    kept = np.full((T, n, H, W, C), np.nan, np.float32)
    gen = None if seed is None else torch.Generator(device="cuda").manual_seed(seed)
    Dz = net.cfg.latent_dim
    for first, fresh in windows:
        ids = [(first + r) % n for r in range(B)]
        inp = torch.from_numpy(tiles[ids]).cuda()
        noise = None
        if gen is None:
            eps = torch.zeros([T, B, Dz], device="cuda")
            if net.cfg.add_noise_to_chain:
                noise = torch.zeros([T, B, H, W, C], device="cuda")
        else:
            eps = torch.randn([T, B, Dz], generator=gen, dtype=torch.float32, device="cuda")
            if net.cfg.add_noise_to_chain:
                noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device="cuda")
        net.forward(inp, inp, eps, 1.0, noise=noise)
        for t in range(T):
            x = net.xhat(t).cpu().numpy()
            if n < B:
                kept[t] = x[:n]
            else:
                kept[t, first + B - fresh:first + B] = x[B - fresh:]
    assert not np.isnan(kept).any()
    return tr.blend(kept, *geom, source=None if known is None else img, known=known, lo=LO, hi=HI)


def _bitwise(got, ref):
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), np.asarray(ref, dtype=np.float32).view(np.int32))


CASES = {
    "one_80x72": ((1, 80, 72), [(0, 4), (4, 4), (8, 4), (12, 4)]),   # 16 tiles in four windows
    "six_32x32": ((6, 32, 32), [(0, 4), (2, 2)]),                    # the last window is [2, 6), two rows new
    "one_32x32": ((1, 32, 32), [(0, 1)]),                            # one tile, four times in the wrapping window
}


@pytest.fixture(scope="module")
def recomputed():
    """case -> (images, out, out_u8) with eps = 0, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            shape, windows = CASES[name]
            img = _images(*shape)
            cache[name] = (img,) + _recompute(img, windows)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(CASES))
def test_restore_is_the_recomputation_bitwise(name, recomputed):
    img, ref, ref8 = recomputed(name)
    R = pkg_mod("restore")
    assert [(f, fr) for f, _, fr in R.windows(tr.n_tiles(*img.shape[:3], H, W, STRIDE, STRIDE), B)] == CASES[name][1]
    net = _net()
    last = net.restore(img)                                     # uint8 in, uint8 out, the last step
    assert last.dtype == torch.uint8 and tuple(last.shape) == img.shape and last.is_cuda
    np.testing.assert_array_equal(last.cpu().numpy(), ref8[-1])
    every = net.restore(torch.from_numpy(img), steps="all", as_uint8=False)
    assert every.dtype == torch.float32 and tuple(every.shape) == (T,) + img.shape
    _bitwise(every, ref)
    _bitwise(net.restore(img, steps=0, stride=(STRIDE, STRIDE), as_uint8=False), ref[0])
    _bitwise(net.restore(img, steps=-2, as_uint8=False), ref[T - 2])
    # float images already in the data range are the same restoration
    as_float = net.restore(tr.dequant(img, LO, HI), steps="all")
    assert as_float.dtype == torch.float32
    _bitwise(as_float, ref)
    if name != "one_32x32":
        # (a lone tile fills its wrapping window with copies of itself: the batch statistics of the FC layers
        # have no variance and the untrained network answers with a flat image)
        assert ref8[-1].std() > 1 and not np.array_equal(ref[0], ref[-1])


def test_a_single_hwc_image_is_one_image(recomputed):
    img, ref, ref8 = recomputed("one_80x72")
    out = _net().restore(img[0])
    assert tuple(out.shape) == img.shape
    np.testing.assert_array_equal(out.cpu().numpy(), ref8[-1])


@pytest.mark.parametrize("preset", ["tiny", "tiny_flat"])
def test_a_seed_draws_eps_then_chain_noise_from_one_generator(preset):
    shape, windows = CASES["six_32x32"]
    img = _images(*shape)
    net = _net(preset)
    got = net.restore(img, steps="all", seed=5, as_uint8=False)
    ref, _ = _recompute(img, windows, seed=5, preset=preset)
    _bitwise(got, ref)
    again = net.restore(img, steps="all", seed=5, as_uint8=False)
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    mean = net.restore(img, steps="all", as_uint8=False)
    assert not torch.equal(mean, got)
    zero, _ = _recompute(img, windows, seed=None, preset=preset)
    _bitwise(mean, zero)
    assert not torch.equal(net.restore(img, steps="all", seed=6, as_uint8=False), got)


def test_known_pixels_come_back_as_given(recomputed):
    img, ref, ref8 = recomputed("one_80x72")
    known = np.random.default_rng(2).uniform(size=img.shape[:3]) < 0.5
    net = _net()
    got8 = net.restore(img, known=known).cpu().numpy()
    got = net.restore(img, known=torch.from_numpy(known[0].astype(np.uint8)), as_uint8=False).cpu().numpy()
    np.testing.assert_array_equal(got8[known], img[known])
    np.testing.assert_array_equal(got[known], tr.dequant(img, LO, HI)[known])
    np.testing.assert_array_equal(got8[~known], ref8[-1][~known])   # the forward does not see the mask
    np.testing.assert_array_equal(got[~known], ref[-1][~known])
    assert not np.array_equal(got8, img) and not np.array_equal(got8, ref8[-1])
    full, full8 = _recompute(img, CASES["one_80x72"][1], known=known.astype(np.uint8))
    np.testing.assert_array_equal(got8, full8[-1])
    np.testing.assert_array_equal(got, full[-1])


def test_an_image_smaller_than_the_tile_keeps_its_size():
    img = _images(1, 20, 40, seed=4)
    net = _net()
    out = net.restore(img, steps="all")
    assert out.dtype == torch.uint8 and tuple(out.shape) == (T, 1, 20, 40, C)
    padded = np.pad(img, ((0, 0), (0, 12), (0, 0), (0, 0)), mode="edge")   # edge-replicated up to 32 x 40: two tiles
    whole = net.restore(padded, steps="all")
    assert tuple(whole.shape) == (T, 1, 32, 40, C)
    assert torch.equal(out, whole[:, :, :20])
    known = np.zeros((20, 40), bool)
    known[3:9, 30:] = True
    got = net.restore(img, known=known).cpu().numpy()
    assert tuple(got.shape) == (1, 20, 40, C)
    np.testing.assert_array_equal(got[0][known], img[0][known])


def test_bad_arguments_raise():
    net = _net()
    img = _images(1, 40, 40)
    for kw in [dict(stride=0), dict(stride=33), dict(stride=(16, 40)), dict(steps=3), dict(steps=-4), dict(steps="last"),
               dict(range=(1.0, 1.0)), dict(known=np.zeros((40, 41), bool)), dict(known=np.zeros((40, 40), np.float32))]:
        with pytest.raises(ValueError):
            net.restore(img, **kw)
    with pytest.raises(ValueError):
        net.restore(img[..., :2])
    with pytest.raises(ValueError):
        net.restore(img.astype(np.int32))
    with pytest.raises(ValueError, match=r"\b49152\b.*\b1000\b.*fewer images"):
        net.restore(img, max_bytes=1000)   # 2 x 2 tiles of 32 x 32 x 3 floats, one step


def test_restoring_moves_nothing_of_a_training_run():
    """Every draw of a restoration is injected: a network that restores before and between its training steps
    (whose eps is drawn on the device) ends with the parameters and losses of a twin that never does."""
    a, b = _net(), _net()
    img = _images(2, 48, 40, seed=8)
    batch = tr.dequant(_images(B, H, W, seed=9), LO, HI)
    before = (a.iteration, a.adam_updates, a.learning_rate, a.params.clone())
    a.restore(img)
    a.restore(img, seed=3, steps="all")
    torch.cuda.synchronize()
    assert (a.iteration, a.adam_updates, a.learning_rate) == before[:3] and torch.equal(a.params, before[3])
    for k in range(3):
        la, lb = a.train(batch, batch), b.train(batch, batch)
        assert la == lb, k
        assert a.loss_value() == b.loss_value(), k
        if k < 2:
            a.restore(img, seed=k)
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    assert (a.iteration, a.adam_updates, a.learning_rate) == (b.iteration, b.adam_updates, b.learning_rate)
    ma, va = a._adam_state()
    mb, vb = b._adam_state()
    assert torch.equal(ma, mb) and torch.equal(va, vb)


def test_the_tool_round_trips_an_npy_through_a_checkpoint(tmp_path):
    spec = importlib.util.spec_from_file_location("svae_tools_restore", os.path.join(ROOT, "tools", "restore.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    net = _net(seed=5)   # not the seed the tool builds its network with: the checkpoint must be what it runs
    os.makedirs(tmp_path / "models" / "tiny_v2")
    net.save_checkpoint(str(tmp_path / "models" / "tiny_v2" / "model.safetensors"))
    img = _images(1, 50, 45, seed=6)
    known = np.zeros((1, 50, 45), np.uint8)
    known[:, 10:20] = 1
    np.save(tmp_path / "in.npy", img)
    np.save(tmp_path / "known.npy", known)
    common = ["--netname", "tiny", "--version", "2", "--batch_size", str(B), "--dtype", "fp32",
              "--models_dir", str(tmp_path / "models"), "--input", str(tmp_path / "in.npy")]
    assert tool.main(common + ["--output", str(tmp_path / "out.npy")]) == 0
    out = np.load(tmp_path / "out.npy")
    assert out.dtype == np.uint8 and out.shape == img.shape
    np.testing.assert_array_equal(out, net.restore(img).cpu().numpy())
    assert not np.array_equal(out, _net(seed=0).restore(img).cpu().numpy())
    assert tool.main(common + ["--output", str(tmp_path / "all.npy"), "--steps", "all", "--stride", "8", "--seed", "4",
                               "--known", str(tmp_path / "known.npy"), "--range=-1,1"]) == 0
    every = np.load(tmp_path / "all.npy")
    assert every.shape == (T,) + img.shape
    np.testing.assert_array_equal(every, net.restore(img, steps="all", stride=8, seed=4, known=known).cpu().numpy())
    np.testing.assert_array_equal(every[:, :, 10:20], np.broadcast_to(img[:, 10:20], (T, 1, 10, 45, C)))
    assert tool.main(common + ["--output", str(tmp_path / "out.png")]) == 1
    assert tool.main(common[:3] + ["7"] + common[4:] + ["--output", str(tmp_path / "out.npy")]) == 1   # no such checkpoint
