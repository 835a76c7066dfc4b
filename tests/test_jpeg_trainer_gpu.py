"""NoisyTrainer with a Degradation whose jpeg stage is on, on the GPU: preset ``tiny`` (B = 4, 32x32x3, T = 3) on
DeviceDataset.synthetic, as tests/test_degrade_trainer_gpu.py.

The trainer's input is svae_op_degrade_batch's output put through svae_op_jpeg_batch in place under the same seed
and offset.  It is recomputed here by running svae_op_degrade_batch on the trainer's own clean target (that op is
held to its restatement in tests/test_degrade_gpu.py) and applying tests/jpeg_ref.py's fp32 mode to it: bitwise."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import jpeg_ref as jr
from conftest import ROOT, pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
GROUPS = (B * H * W * C + 3) // 4
JPEG = (0.5, 10, 90, 2)


def _net(seed=0):
    cfg = pkg_mod("config").preset("tiny", batch=B, dtype="fp32")
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _dataset(n=55):
    return pkg_mod("data").DeviceDataset.synthetic(n, H, W, C, seed=3, device="cuda")


def _trainer(net, ds=None, **kw):
    kw.setdefault("denoise_train", True)
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


def _deg(jpeg=JPEG, **kw):
    kw = dict(dict(downsample=(0.5, 2), cutout=(0.5, 3, 4, 12, 0.5)), **kw)
    return pkg_mod("degrade").Degradation(jpeg=jpeg, **kw)


def test_the_draws_of_the_batches_below_fire_and_do_not():
    NT = pkg_mod("trainer").NoisyTrainer
    for seed in (SEED, SEED ^ NT.test_seed_xor):
        q = np.concatenate([jr.draws(B, JPEG[0], JPEG[1], JPEG[2], seed, k * GROUPS) for k in range(2)])
        assert {bool(v) for v in q} == {False, True}


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("test_split", [False, True])
def test_input_is_the_restatement_applied_to_the_degrade_output(denoise, test_split):
    NT, D = pkg_mod("trainer").NoisyTrainer, pkg_mod("degrade")
    noise = (NT.pepper_prob, NT.salt_prob, NT.gaussian_noise_scale) if denoise else (0.0, 0.0, 0.0)
    seed = SEED ^ NT.test_seed_xor if test_split else SEED
    tr = _trainer(_net(), denoise_train=denoise, degradation=_deg())
    for k in range(2):
        inp, tgt = tr._next(test=test_split)
        assert inp is tr._input and tgt is tr._target
        degraded = D.degrade_batch(tgt, _deg(), -1.0, 1.0, noise, seed, k * GROUPS)
        ref = jr.jpeg_batch(degraded.cpu().numpy(), *JPEG, -1.0, 1.0, seed, k * GROUPS, "fp32")
        np.testing.assert_array_equal(inp.cpu().numpy().view(np.int32), ref["out"].view(np.int32))
        for b in range(B):
            assert torch.equal(inp[b], degraded[b]) == (ref["quality"][b] == 0)
    assert (tr.test_offset, tr.train_offset) == ((2 * GROUPS, 0) if test_split else (0, 2 * GROUPS))


def test_jpeg_alone_without_pixel_noise():
    """Only the jpeg stage on, denoise_train off: the input is the restatement of the clean target."""
    tr = _trainer(_net(), denoise_train=False, degradation=pkg_mod("degrade").Degradation(jpeg=(1.0, 20, 20, 1)))
    inp, tgt = tr._next()
    ref = jr.jpeg_batch(tgt.cpu().numpy(), 1.0, 20, 20, 1, -1.0, 1.0, SEED, 0, "fp32")
    np.testing.assert_array_equal(inp.cpu().numpy().view(np.int32), ref["out"].view(np.int32))
    assert inp is tr._input and not torch.equal(inp, tgt) and tr.train_offset == GROUPS


def test_default_jpeg_field_feeds_the_inputs_of_today(monkeypatch):
    """A Degradation built as before this stage existed (positionally, or by keywords without jpeg) has jpeg at
    p = 0: no svae_op_jpeg_batch launch is made and inputs, losses and parameters are byte for byte those of a
    Degradation that names jpeg = (0, ...) itself."""
    D = pkg_mod("degrade")
    old_style = D.Degradation((0.5, 0.5, 3.0), (0.5, 4), (0.5, 2, 4, 12, 0.0))
    assert old_style == D.Degradation(blur=(0.5, 0.5, 3.0), downsample=(0.5, 4), cutout=(0.5, 2, 4, 12))
    assert old_style.jpeg == (0.0, 75, 75, 2)
    explicit = D.Degradation((0.5, 0.5, 3.0), (0.5, 4), (0.5, 2, 4, 12, 0.0), (0.0, 10, 90))
    a, b = _trainer(_net(), degradation=old_style), _trainer(_net(), degradation=explicit)
    c = _trainer(_net(), degradation=D.Degradation((0.5, 0.5, 3.0), (0.5, 4), (0.5, 2, 4, 12, 0.0), (1.0, 10, 90)))

    def forbidden(*args, **kw):
        raise AssertionError("jpeg_batch launched with the stage off")
    for k in range(3):
        with monkeypatch.context() as m:
            m.setattr(D, "jpeg_batch", forbidden)
            la, lb = a.step(), b.step()
        c.step()
        assert la == lb, k
        assert torch.equal(a._input, b._input) and torch.equal(a._target, b._target)
        assert torch.equal(a._target, c._target) and not torch.equal(a._input, c._input)
    assert a.state_dict() == b.state_dict() == c.state_dict() and a.train_offset == 3 * GROUPS
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params)


def test_four_steps_equal_two_steps_save_load_two_steps(tmp_path):
    full = _trainer(_net(), degradation=_deg())
    for _ in range(4):
        full.step()
    part = _trainer(_net(), degradation=_deg())
    part.step()
    part.step()
    part.save(str(tmp_path))
    again = _trainer(_net(seed=9), degradation=_deg())
    again.load(str(tmp_path))
    again.step()
    again.step()
    torch.cuda.synchronize()
    assert again.state_dict() == full.state_dict() and again.state_dict()["iteration"] == 4
    assert sorted(again.state_dict()) == sorted(_trainer(_net()).state_dict())  # no new state
    assert torch.equal(again._input, full._input)
    assert torch.equal(again.network.params.view(torch.int32), full.network.params.view(torch.int32))


def test_evaluation_baseline_is_worse_at_quality_10_than_at_90():
    net = _net()
    res = {}
    for q in (10, 90):
        tr = _trainer(net, denoise_train=False, degradation=pkg_mod("degrade").Degradation(jpeg=(1.0, q, q)))
        state = tr.state_dict()
        res[q] = tr.evaluate()
        assert tr.state_dict() == state and tr.evaluate() == res[q]
    print("input psnr: q 10 %.3f dB, q 90 %.3f dB" % (res[10]["input"]["psnr"], res[90]["input"]["psnr"]))
    assert res[10]["input"]["psnr"] < res[90]["input"]["psnr"]
    assert res[10]["input"]["mse"] > res[90]["input"]["mse"] > 0
    info = tr.latent_information(num_batches=1)
    assert info["images"] == B and tr.latent_information(num_batches=1) == info


def test_command_line_flags_round_trip():
    D = pkg_mod("degrade")
    assert D.Degradation.from_flags() is None
    assert D.Degradation.from_flags(jpeg="0.5,10,90") == D.Degradation(jpeg=(0.5, 10, 90, 2))
    assert D.Degradation.from_flags(jpeg="1,30,30,1") == D.Degradation(jpeg=(1.0, 30, 30, 1))
    for bad in ("0.5,10", "0.5,0,90", "0.5,90,10", "1.5,10,90", "0.5,10,90,3", "0.5,10,101"):
        with pytest.raises(ValueError):
            D.Degradation.from_flags(jpeg=bad)
    for tool in ("train", "evaluate"):
        spec = importlib.util.spec_from_file_location("svae_tool_" + tool, os.path.join(ROOT, "tools", tool + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        base = ["--synthetic", "64", "--netname", "tiny"]
        a = mod.parse(base + ["--jpeg", "0.5,10,90"])
        assert mod.degradation(a) == D.Degradation(jpeg=(0.5, 10, 90, 2))
        a = mod.parse(base + ["--downsample", "0.5,2", "--cutout", "0.5,3,4,12,0.5", "--jpeg", "0.5,10,90,2"])
        assert mod.degradation(a) == _deg()
        assert mod.degradation(mod.parse(base)) is None
