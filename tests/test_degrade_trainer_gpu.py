"""NoisyTrainer(degradation=...) on the GPU: preset ``tiny`` (B = 4, 32x32x3, T = 3) on DeviceDataset.synthetic.

The trainer's input under a Degradation is svae_op_make_batch (target only) followed by svae_op_degrade_batch under
the seed and offset the noisy batch uses today.  It is recomputed here by tests/degrade_ref.py from the trainer's own
clean target: bitwise where no blur is involved (the Gaussian pixel noise through svae_op_make_batch in place, as in
tests/test_degrade_gpu.py), within that file's blur bound otherwise."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import degrade_ref as dr
from conftest import ROOT, pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
GROUPS = (B * H * W * C + 3) // 4
NORMAL_BOUND = 4 * 1.9405e-6  # tests/test_make_batch_gpu.py


def _net(seed=0):
    cfg = pkg_mod("config").preset("tiny", batch=B, dtype="fp32")
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _dataset(n=55):
    return pkg_mod("data").DeviceDataset.synthetic(n, H, W, C, seed=3, device="cuda")


def _trainer(net, ds=None, **kw):
    kw.setdefault("denoise_train", True)
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


def _all_on():
    return pkg_mod("degrade").Degradation(blur=(0.5, 0.5, 3.0), downsample=(0.5, 4), cutout=(0.5, 2, 4, 12, 0.0))


def _no_blur():
    return pkg_mod("degrade").Degradation(downsample=(0.5, 2), cutout=(0.5, 3, 4, 12, 0.5))


def _spec(deg, noise):
    return dr.Spec(*deg.blur, *deg.downsample, *deg.cutout, *noise)


def _make_batch_in_place(x, noise, seed, offset):
    L = pkg_mod("_lib")
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    L.check(L.lib().svae_op_make_batch(L.ptr(d), 0, None, 0, B, H * W * C, -1.0, 1.0, *noise, seed, offset, None,
                                       L.ptr(d), L.stream_ptr()))
    torch.cuda.synchronize()
    return d.cpu().numpy()


def test_no_degradation_is_the_trainer_as_it_was():
    a, b = _trainer(_net()), _trainer(_net(), degradation=None)
    for k in range(3):
        la, lb = a.step(), b.step()
        assert la == lb, k
        assert torch.equal(a._input, b._input) and torch.equal(a._target, b._target)
    assert a.state_dict() == b.state_dict() and a.train_offset == 3 * GROUPS
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params)
    # without denoise_train the input is the clean target and no offset moves
    c = _trainer(_net(), denoise_train=False, degradation=None)
    inp, tgt = c._next()
    assert inp is tgt and (c.train_offset, c.test_offset) == (0, 0)


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("test_split", [False, True])
def test_input_is_the_reference_applied_to_the_target(denoise, test_split):
    NT = pkg_mod("trainer").NoisyTrainer
    noise = (NT.pepper_prob, NT.salt_prob, NT.gaussian_noise_scale) if denoise else (0.0, 0.0, 0.0)
    seed = SEED ^ NT.test_seed_xor if test_split else SEED
    # without blur: bitwise, two consecutive batches (the second at the advanced offset)
    tr = _trainer(_net(), denoise_train=denoise, degradation=_no_blur())
    fired = set()
    for k in range(2):
        inp, tgt = tr._next(test=test_split)
        assert inp is tr._input and tgt is tr._target
        ref = dr.degrade(tgt.cpu().numpy(), _spec(_no_blur(), noise)._replace(gaussian_scale=0.0), -1.0, 1.0, seed,
                         k * GROUPS, "fp32")
        want = _make_batch_in_place(ref["structured"], noise, seed, k * GROUPS)
        np.testing.assert_array_equal(inp.cpu().numpy().view(np.int32), want.view(np.int32))
        fired |= {(g, bool(d[g])) for d in ref["draws"] for g in ("down", "cut")}
    assert fired == {(g, v) for g in ("down", "cut") for v in (False, True)}
    assert (tr.test_offset, tr.train_offset) == ((2 * GROUPS, 0) if test_split else (0, 2 * GROUPS))
    # all stages on: within 4 x the restatement's own fp32 - fp64 deviation, plus the normals' bound times the scale
    tr = _trainer(_net(), denoise_train=denoise, degradation=_all_on())
    inp, tgt = tr._next(test=test_split)
    x = tgt.cpu().numpy()
    truth = dr.degrade(x, _spec(_all_on(), noise), -1.0, 1.0, seed, 0, "fp64")
    own = dr.degrade(x, _spec(_all_on(), noise), -1.0, 1.0, seed, 0, "fp32")
    assert {bool(d["blur"]) for d in truth["draws"]} == {False, True}
    self_dev = float(np.abs(own["input"] - truth["input"]).max())
    dev = float(np.abs(inp.cpu().numpy().astype(np.float64) - truth["input"]).max())
    bound = 4 * self_dev + NORMAL_BOUND * noise[2]
    print("device - fp64 %.3e, fp32 mode - fp64 %.3e, bound %.3e" % (dev, self_dev, bound))
    assert self_dev > 0 and dev <= bound
    assert not torch.equal(inp, tgt)


def test_resume_reproduces_the_degraded_batch(tmp_path):
    full = _trainer(_net(), degradation=_all_on())
    full.test(0, num_iters=1)
    for _ in range(3):
        full.step()
    third = full._input.clone()
    part = _trainer(_net(), degradation=_all_on())
    part.test(0, num_iters=1)
    part.step()
    part.step()
    second = part._input.clone()
    part.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["model.safetensors", "trainer.json"]
    assert sorted(json.load(open(tmp_path / "trainer.json"))) == sorted(_trainer(_net()).state_dict())  # no new state
    again = _trainer(_net(seed=9), degradation=_all_on())
    again.load(str(tmp_path))
    again.step()
    assert again.state_dict() == full.state_dict() and again.state_dict()["iteration"] == 3
    assert torch.equal(again._input, third) and not torch.equal(second, third)


@pytest.fixture(scope="module")
def degraded_eval():
    tr = _trainer(_net(), degradation=_all_on())
    before = (tr.state_dict(), tr.network.iteration, tr.network.adam_updates, tr.network.params.clone())
    return tr, tr.evaluate(), before


def test_evaluation_under_a_degradation_moves_nothing_and_repeats(degraded_eval):
    tr, res, (state, it, adam, params) = degraded_eval
    assert tr.state_dict() == state and (tr.dataset.train_idx, tr.dataset.test_idx) == (0, 0)
    assert (tr.train_offset, tr.test_offset, tr.iteration) == (0, 0, 0)
    assert (tr.network.iteration, tr.network.adam_updates) == (it, adam)
    assert torch.equal(tr.network.params, params)
    assert tr.evaluate() == res and res["images"] == 11
    assert json.loads(json.dumps(res)) == res
    # the structured damage comes on top of the pixel noise: the baseline is worse than the noise's alone
    plain = _trainer(tr.network).evaluate()
    print("input psnr: degraded %.4f, noise only %.4f" % (res["input"]["psnr"], plain["input"]["psnr"]))
    assert res["input"]["psnr"] < plain["input"]["psnr"] and res["input"]["mse"] > plain["input"]["mse"]
    # and without any pixel noise the degraded input is still not the clean image
    quiet = _trainer(tr.network, denoise_train=False, degradation=_all_on()).evaluate()
    assert quiet["input"]["mse"] > 0 and quiet["input"]["ssim"] < 1  # (psnr is +inf where an image drew no stage)
    info = tr.latent_information(num_batches=1)
    assert info["images"] == 4 and tr.state_dict() == state and tr.latent_information(num_batches=1) == info


def test_training_is_bitwise_the_same_with_evaluations_between_steps():
    """No draw of an evaluation under a degradation comes from the network's device Philox counter, and no cursor or
    offset moves: a trainer that evaluates between its steps ends with the parameters of one that never does."""
    a, b = _trainer(_net(), degradation=_all_on()), _trainer(_net(), degradation=_all_on())
    a.step(), b.step()
    a.evaluate()
    for k in range(2):
        la, lb = a.step(), b.step()
        assert la == lb, k
        a.evaluate(split="train", num_batches=1)
        a.latent_information(num_batches=1)
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params)
    assert a.state_dict() == b.state_dict()


def test_command_line_flags_give_the_same_degradation():
    for tool in ("train", "evaluate"):
        spec = importlib.util.spec_from_file_location("svae_tool_" + tool, os.path.join(ROOT, "tools", tool + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        base = ["--synthetic", "64", "--netname", "tiny"]
        a = mod.parse(base + ["--blur", "0.5,0.5,3", "--downsample", "0.5,4", "--cutout", "0.5,2,4,12"])
        assert mod.degradation(a) == _all_on()
        a = mod.parse(base + ["--downsample", "0.5,2", "--cutout", "0.5,3,4,12,0.5"])
        assert mod.degradation(a) == _no_blur()
        assert mod.degradation(mod.parse(base)) is None
