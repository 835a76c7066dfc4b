"""NoisyTrainer, sibling contexts and the chain views on the GPU: preset ``tiny`` (B = 4, 32x32x3, T = 3)
and a synthetic uint8 dataset of 12 train / 8 test images."""
import os

import numpy as np
import pytest
import torch

from conftest import pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77


def _net(preset="tiny", batch=4, dtype="fp32", seed=0, **over):
    cfg = pkg_mod("config").preset(preset, batch=batch, dtype=dtype, **over)
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _dataset():
    ds = pkg_mod("data").DeviceDataset.synthetic(20, 32, 32, 3, seed=3, test_fraction=0.4, device="cuda")
    assert (ds.train_size, ds.test_size) == (12, 8)
    return ds


def _trainer(net, ds=None, **kw):
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


def _manual_batch(ds, start, offset, seed=SEED, test=False, noise=(0.1, 0.1, 0.1)):
    """(input, target) of the window by a direct svae_op_make_batch call."""
    L = pkg_mod("_lib")
    data = ds.test if test else ds.train
    tgt = torch.empty(4, 32, 32, 3, device="cuda")
    inp = torch.empty_like(tgt)
    L.check(L.lib().svae_op_make_batch(L.ptr(data), 1, None, start, 4, 32 * 32 * 3, -1.0, 1.0, *noise, seed, offset,
                                       L.ptr(tgt), L.ptr(inp), L.stream_ptr()))
    return inp, tgt


def test_denoise_training_matches_a_manual_loop():
    """Four trainer.step() calls = a second, identically seeded network driven by hand with
    svae_op_make_batch + train(): parameters bitwise, losses equal.  With 12 images and B = 4 the windows
    are [0,4) [4,8) [8,12) [0,4): the fourth batch is the one that wraps the cursor."""
    a, b = _net(), _net()
    tr = _trainer(a, denoise_train=True)
    ds = _dataset()
    groups = (4 * 32 * 32 * 3 + 3) // 4
    for k, start in enumerate([0, 4, 8, 0]):
        got = tr.step()
        inp, tgt = _manual_batch(ds, start, k * groups)
        want = b.train(inp, tgt)
        assert got == want, (k, got, want)
        assert not torch.equal(inp, tgt)
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    assert (tr.iteration, a.iteration, tr.train_offset, tr.dataset.train_idx) == (4, 4, 4 * groups, 4)
    with pytest.raises(RuntimeError):
        _trainer(_net(), denoise_train=False).apply_noise(torch.zeros(4, 32, 32, 3, device="cuda"))


def test_apply_noise_is_the_kernel_in_place():
    tr = _trainer(_net(), denoise_train=True)
    ds = tr.dataset
    _, clean = _manual_batch(ds, 4, 0, noise=(0.0, 0.0, 0.0))
    want, _ = _manual_batch(ds, 4, 0)
    got = tr.apply_noise(clean.clone())
    assert torch.equal(got, want) and tr.train_offset == (4 * 32 * 32 * 3 + 3) // 4


@pytest.mark.parametrize("denoise", [False, True])
def test_trainer_test_error(denoise):
    """trainer.test = sum((xhat - clean)^2) / (H W) / B of the same forward, within 1e-4 relative (the
    bound tests/test_golden_gpu.py holds the per-step reconstruction to)."""
    a, b = _net(), _net()
    tr = _trainer(a, denoise_train=denoise)
    got = tr.test(0, num_iters=3)  # test windows [0,4) [4,8) [0,4)
    ds = _dataset()
    groups = (4 * 32 * 32 * 3 + 3) // 4
    want = 0.0
    for k, start in enumerate([0, 4, 0]):
        noise = (0.1, 0.1, 0.1) if denoise else (0.0, 0.0, 0.0)
        inp, tgt = _manual_batch(ds, start, k * groups, seed=SEED ^ tr.test_seed_xor, test=True, noise=noise)
        b.forward(inp, tgt, None, 1.0)
        want += float((b.xhat(-1).double() - tgt.double()).square().sum()) / (32 * 32) / 4
    want /= 3
    print("trainer.test %.8f, torch %.8f" % (got, want))
    assert abs(got - want) <= 1e-4 * abs(want)
    assert tr.test_offset == (3 * groups if denoise else 0) and tr.train_offset == 0


def test_trainer_test_error_under_predicted_noise():
    """predict_generator_noise: SVAE_BUF_REC_IMG holds the NLL, the error comes from x_hat."""
    over = dict(add_noise_to_chain=True, predict_generator_noise=True)
    a, b = _net(**over), _net(**over)
    tr = _trainer(a, denoise_train=True)
    got = tr.test(0, num_iters=1)
    inp, tgt = _manual_batch(_dataset(), 0, 0, seed=SEED ^ tr.test_seed_xor, test=True)
    b.forward(inp, tgt, None, 1.0)
    want = float((b.xhat(-1).double() - tgt.double()).square().sum()) / (32 * 32) / 4
    assert abs(got - want) <= 1e-4 * abs(want)


@pytest.mark.parametrize("preset,dtype", [("tiny", "fp32"), ("tiny", "bf16x6"), ("tiny_homog", "fp32")])
def test_sibling_reads_the_owners_parameters(preset, dtype):
    """The owner at B = 4 trains two steps; sibling(6).test(x) is bitwise a stand-alone B = 6 network given
    the owner's parameters with set_param.  A sibling created BEFORE the training catches stale bf16 and
    shared-weight copies."""
    owner = _net(preset, 4, dtype)
    sib = owner.sibling(6)
    assert sib is owner.sibling(6) and owner.sibling(4) is owner and sib.params is owner.params
    x6 = torch.rand(6, 32, 32, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1
    sib.test(x6)  # builds its weight copies from the initial parameters
    tr = _trainer(owner, denoise_train=True)
    tr.step()
    tr.step()
    got = sib.test(x6)
    alone = _net(preset, 6, dtype, seed=5)
    for p in alone.table:
        alone.set_param(p["name"], owner.param(p["name"]))
    alone.test(x6)  # the same number of forwards: the engine's own eps counter advances per forward
    want = alone.test(x6)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    with pytest.raises(RuntimeError):
        sib.train(x6, x6)


def test_training_mc_samples_and_visualize(tmp_path):
    x = torch.rand(4, 32, 32, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1
    net = _net("tiny")
    z = net.training_mc_samples(x)
    assert len(z) == 3 and all(a.shape == (4, 32, 32, 3) for a in z)
    np.testing.assert_array_equal(z[2], net.sample(2).cpu().numpy())
    flat = _net("tiny_flat")
    z = flat.training_mc_samples(x)
    assert len(z) == 6
    for t in range(3):
        np.testing.assert_array_equal(z[t], flat.xhat(t).cpu().numpy())
        np.testing.assert_array_equal(z[3 + t], flat.sample(t).cpu().numpy())
    assert not np.array_equal(z[0], z[3])  # step 0's chain noise is live
    ds = _dataset()
    for n, per, first in ((net, 1, 0), (flat, 2, 6)):
        base = str(tmp_path / ("v%d" % per))
        test_c, train_c = n.visualize(7, ds, base, batch_size=6)
        assert test_c.shape == train_c.shape == (per * 6 * 32, 4 * 32, 3)
        assert 0.0 <= test_c.min() and train_c.max() <= 1.0
        names = sorted(os.path.splitext(f)[0] for f in os.listdir(base + "/samples"))
        assert names == ["test_current", "test_epoch7", "train_current", "train_epoch7"]
        # column 0 of the training canvas is the input batch as displayed
        want = ds.display(-1.0 + ds.train[first].float() * (2.0 / 255.0)).cpu().numpy()
        np.testing.assert_allclose(train_c[:32, :32], want, atol=1e-6)
    assert ds.train_idx == 12  # two training windows of 6


def test_resume_reproduces_the_corrupted_batch(tmp_path):
    """Two steps, save, new objects, load, one more step: iteration, cursors and offsets equal the
    uninterrupted run's, and the third corrupted batch is bitwise the same (parameters are not compared:
    the engine's own eps counter is not part of a checkpoint)."""
    full = _trainer(_net(), denoise_train=True)
    full.test(0, num_iters=1)
    for _ in range(3):
        full.step()
    third = full._input.clone()
    part = _trainer(_net(), denoise_train=True)
    part.test(0, num_iters=1)
    part.step()
    part.step()
    part.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["model.safetensors", "trainer.json"]
    again = _trainer(_net(seed=9), denoise_train=True)
    again.load(str(tmp_path))
    assert again.network.iteration == 2
    again.step()
    assert again.state_dict() == full.state_dict()
    assert again.state_dict()["iteration"] == 3 and again.state_dict()["train_idx"] == 12
    assert torch.equal(again._input, third)
