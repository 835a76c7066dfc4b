"""NoisyTrainer on a data.PatchDataset: preset ``tiny`` (B = 4, 32x32x3, T = 3) over synthetic uint8 images of
80 x 96 pixels, three tiles wide.  The clean target of a training step is svae_op_crop_batch under the trainer's
seed and train_offset, recomputed here by tests/crops_ref.py bit for bit; the input is derived from it by the ops the
plain trainer uses."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import crops_ref as cr
from conftest import ROOT, pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
BIG_H, BIG_W = 80, 96
GROUPS = (B * H * W * C + 3) // 4
SCALES, SYM, EVAL = (1, 2), 8, 11


def _net(seed=0):
    cfg = pkg_mod("config").preset("tiny", batch=B, dtype="fp32")
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _big(n=10):
    return pkg_mod("data").DeviceDataset.synthetic(n, BIG_H, BIG_W, C, seed=3, device="cuda")


def _dataset(**kw):
    big = _big()
    kw = dict(dict(scales=SCALES, symmetries=SYM, eval_crops=EVAL, eval_seed=5), **kw)
    return pkg_mod("data").PatchDataset(big.train, big.test, (H, W), **kw)


def _trainer(net, ds=None, **kw):
    kw.setdefault("denoise_train", True)
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


def _degradation():
    return pkg_mod("degrade").Degradation(blur=(0.5, 0.5, 2.0), downsample=(0.5, 2), cutout=(0.5, 2, 4, 12, 0.0))


def _bitwise(t, ref):
    assert torch.equal(t.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(ref)).view(torch.int32))


def test_the_fixed_sets_are_the_op_under_eval_seed():
    ds = _dataset()
    assert isinstance(ds, pkg_mod("data").DeviceDataset) and ds.data_dims == [H, W, C]
    assert (ds.train_size, ds.test_size) == (EVAL, EVAL) and ds.train.dtype == torch.uint8
    for k, (fixed, images) in enumerate(((ds.train, ds.train_images), (ds.test, ds.test_images))):
        ref = cr.crop_batch(images.cpu().numpy(), H, W, SCALES, SYM, 5, k * EVAL, EVAL, -1.0, 1.0)
        np.testing.assert_array_equal(fixed.cpu().numpy(), ref["target_u8"])
    again = _dataset()
    assert torch.equal(again.train, ds.train) and torch.equal(again.test, ds.test)
    assert not torch.equal(_dataset(eval_seed=6).test, ds.test)
    # fp32 images give fp32 sets; from_array splits the large images as DeviceDataset.from_array splits rows
    big = _big()
    arr = torch.cat([big.train, big.test]).cpu().numpy()
    f = pkg_mod("data").PatchDataset.from_array(arr.astype(np.float32) / 255, (H, W), range=(-1.0, 1.0), device="cuda",
                                                scales=(2,), eval_crops=5)
    assert f.train.dtype == torch.float32 and tuple(f.test.shape) == (5, H, W, C)
    assert (int(f.train_images.shape[0]), int(f.test_images.shape[0])) == (8, 2)
    with pytest.raises(ValueError):
        pkg_mod("data").PatchDataset(big.train, big.test, (H, W), scales=(1, 3))  # 3 * 32 > 80
    with pytest.raises(ValueError):
        pkg_mod("data").PatchDataset(big.train, big.test, (H, 48), symmetries=8)


@pytest.mark.parametrize("mode", ["denoise", "degradation", "degradation+denoise", "plain"])
def test_steps_draw_fresh_crops_and_give_finite_losses(mode):
    deg = _degradation() if "degradation" in mode else None
    tr = _trainer(_net(), denoise_train=mode.endswith("denoise"), degradation=deg)
    images = tr.dataset.train_images.cpu().numpy()
    metas = []
    for k in range(3):
        loss = tr.step()
        assert np.isfinite(loss), (mode, k)
        ref = cr.crop_batch(images, H, W, SCALES, SYM, SEED, k * GROUPS, B, -1.0, 1.0)
        _bitwise(tr._target, ref["target"])
        metas.append(ref["meta"])
        assert tr.train_offset == (k + 1) * GROUPS and tr.dataset.train_idx == 0
    # successive steps draw different crops (through meta), whatever the corruption
    assert not (metas[0] == metas[1]).all() and not (metas[1] == metas[2]).all()
    meta = torch.empty([B, 5], dtype=torch.int32, device="cuda")
    out = torch.empty_like(tr._target)
    tr.dataset.patch_batch(B, SEED, 2 * GROUPS, out, meta=meta)
    np.testing.assert_array_equal(meta.cpu().numpy(), metas[2])  # the same draws for the same (seed, offset)
    assert torch.equal(out, tr._target)
    if mode == "plain":
        inp, tgt = tr._next()
        assert inp is tgt and tr.train_offset == 4 * GROUPS
    else:
        assert not torch.equal(tr._input, tr._target)
    if mode == "denoise":
        # the input is svae_op_make_batch's noise on the fp32 target under the same seed and offset
        L = pkg_mod("_lib")
        want = torch.empty_like(tr._target)
        L.check(L.lib().svae_op_make_batch(L.ptr(tr._target), 0, None, 0, B, H * W * C, -1.0, 1.0, tr.pepper_prob,
                                           tr.salt_prob, tr.gaussian_noise_scale, SEED, 2 * GROUPS, None, L.ptr(want),
                                           L.stream_ptr()))
        assert torch.equal(want, tr._input)


def test_test_batches_walk_the_fixed_set():
    tr = _trainer(_net())
    err = tr.test(0, num_iters=3)
    assert np.isfinite(err) and tr.dataset.test_idx == 4 and tr.test_offset == 3 * GROUPS and tr.train_offset == 0
    # (11 crops: windows [0, 4), [4, 8), then the cursor restarts at [0, 4))


def test_resume_draws_the_crops_of_the_uninterrupted_run(tmp_path):
    full = _trainer(_net())
    for _ in range(4):
        full.step()
    part = _trainer(_net())
    part.step(), part.step()
    part.save(str(tmp_path))
    plain_keys = {"iteration", "train_offset", "test_offset", "seed", "denoise_train", "train_idx", "test_idx"}
    assert set(json.load(open(tmp_path / "trainer.json"))) == plain_keys  # no new state
    again = _trainer(_net(seed=9))
    again.load(str(tmp_path))
    again.step(), again.step()
    torch.cuda.synchronize()
    assert again.state_dict() == full.state_dict() and again.iteration == 4
    assert torch.equal(again._target, full._target) and torch.equal(again._input, full._input)
    assert torch.equal(again.network.params.view(torch.int32), full.network.params.view(torch.int32))


def test_evaluation_repeats_and_moves_nothing():
    tr = _trainer(_net())
    tr.step()
    before = (tr.state_dict(), tr.network.iteration, tr.network.adam_updates, tr.network.params.clone())
    res = tr.evaluate()
    assert res["images"] == EVAL and tr.evaluate() == res
    assert json.loads(json.dumps(res)) == res
    assert tr.state_dict() == before[0] and (tr.dataset.train_idx, tr.dataset.test_idx) == (0, 0)
    assert (tr.network.iteration, tr.network.adam_updates) == before[1:3]
    assert torch.equal(tr.network.params, before[3])
    info = tr.latent_information(num_batches=1)
    assert info["images"] == B and tr.state_dict() == before[0]
    # the device RNG: a trainer that evaluates between its steps ends where one that never does ends
    a, b = _trainer(_net()), _trainer(_net())
    a.step(), b.step()
    for k in range(2):
        a.evaluate(num_batches=1)
        la, lb = a.step(), b.step()
        assert la == lb, k
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params) and a.state_dict() == b.state_dict()


def test_a_plain_dataset_never_launches_the_crop_kernel():
    crops = pkg_mod("crops")
    ds = _dataset()
    plain = pkg_mod("data").DeviceDataset(ds.train, ds.test)
    before = crops.calls
    tr = _trainer(_net(), plain)
    tr.step(), tr.step()
    tr.test(0, num_iters=1)
    tr.evaluate(num_batches=1)
    assert crops.calls == before and plain.train_idx == 2 * B
    # and the same trainer on the PatchDataset launches it once per training step only
    tp = _trainer(_net(), ds)
    tp.step(), tp.step()
    tp.test(0, num_iters=1)
    tp.evaluate(num_batches=1)
    assert crops.calls == before + 2


def test_command_line_flags_round_trip():
    for tool in ("train", "evaluate"):
        spec = importlib.util.spec_from_file_location("svae_patch_tool_" + tool, os.path.join(ROOT, "tools", tool + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        base = ["--synthetic", "10", "--netname", "tiny"]
        assert mod.patch_options(mod.parse(base)) is None
        a = mod.parse(base + ["--patches"])
        assert mod.patch_options(a) == dict(scales=(1,), symmetries=1, eval_crops=256)
        a = mod.parse(base + ["--patches", "--patch_scales", "1,2", "--patch_symmetries", "8", "--eval_crops", "11"])
        assert mod.patch_options(a) == dict(scales=SCALES, symmetries=SYM, eval_crops=EVAL)
        cfg = pkg_mod("config").preset("tiny", batch=B)
        ds = mod.dataset(a, cfg, 5)
        assert isinstance(ds, pkg_mod("data").PatchDataset) and ds.data_dims == [H, W, C]
        assert ds.spec == pkg_mod("crops").CropSpec(SCALES, SYM) and (ds.train_size, ds.eval_seed) == (EVAL, 5)
        assert tuple(ds.train_images.shape[1:]) == (4 * H, 4 * W, C)
        assert type(mod.dataset(mod.parse(base), cfg, 5)) is pkg_mod("data").DeviceDataset
        with pytest.raises(SystemExit):
            mod.parse(base + ["--patches", "--patch_symmetries", "3"])
