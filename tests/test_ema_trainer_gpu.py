"""Polyak averaging through SequentialVAE.enable_ema / NoisyTrainer(ema_decay=...) on the GPU: preset ``tiny``
(B = 4, 32x32x3, T = 3) on DeviceDataset.synthetic, 5 steps, fp32 and bf16x6.

The averages are held bitwise to tests/ema_ref.py's recursion over per-step parameter snapshots: the engine
averages every live parameter once per step, after its last Adam update, so the parameters as they stand after
train() are what went into the average.  Training itself must not notice averaging at all."""
import numpy as np
import pytest
import torch

import ema_ref as er
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
STEPS = 5
IMP = dict(add_improvement_maximization_loss=True, latent_pred_loss_coeff=0.01)


def _net(dtype="fp32", preset="tiny", seed=0, **over):
    cfg = pkg_mod("config").preset(preset, batch=B, dtype=dtype, **over)
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _trainer(net, n=24, **kw):
    ds = pkg_mod("data").DeviceDataset.synthetic(n, H, W, C, seed=3, device="cuda")
    kw.setdefault("denoise_train", True)
    return pkg_mod("trainer").NoisyTrainer(net, ds, seed=SEED, **kw)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _state(net):
    m, v = net._adam_state()
    torch.cuda.synchronize()
    return [net.params.clone(), m, v]


def _run_tracked(tr, steps=STEPS):
    """Step the trainer; returns (initial parameters, [parameters after every step])."""
    p0 = tr.network.params.cpu().numpy().copy()
    snaps = []
    for _ in range(steps):
        tr.step()
        snaps.append(tr.network.params.cpu().numpy().copy())
    return p0, snaps


@pytest.mark.parametrize("dtype", ["fp32", "bf16x6"])
def test_training_is_byte_for_byte_what_it_is_without_averaging(dtype):
    plain, avg = _trainer(_net(dtype)), _trainer(_net(dtype), ema_decay=0.99)
    assert plain.network.ema is None and avg.network.ema is not None
    la = [plain.step() for _ in range(STEPS)]
    lb = [avg.step() for _ in range(STEPS)]
    assert la == lb
    for a, b in zip(_state(plain.network), _state(avg.network)):
        _same(a, b)
    assert (plain.train_offset, plain.network.adam_updates) == (avg.train_offset, avg.network.adam_updates)
    assert avg.network.ema_updates == STEPS
    assert not torch.equal(avg.network.ema, avg.network.params)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x6"])
@pytest.mark.parametrize("warmup,every", [(True, 1), (False, 1), (True, 2)])
def test_average_is_the_recursion_over_parameter_snapshots(dtype, warmup, every):
    tr = _trainer(_net(dtype), ema_decay=0.99, ema_warmup=warmup, ema_every=every)
    net = tr.network
    p0, snaps = _run_tracked(tr)
    want, n = er.track(p0, snaps, net.n_live, 0.99, warmup, every)
    assert net.ema_updates == n == STEPS // every
    _same(net.ema, torch.from_numpy(want))
    # the dead tail is the caller's: the copy enable_ema made
    np.testing.assert_array_equal(net.ema.cpu().numpy()[net.n_live:], p0[net.n_live:])


@pytest.mark.parametrize("dtype", ["fp32", "bf16x6"])
def test_shared_weights_take_the_unfused_adam_path(dtype):
    tr = _trainer(_net(dtype, preset="tiny_homog"), ema_decay=0.99)
    net = tr.network
    p0, snaps = _run_tracked(tr)
    want, n = er.track(p0, snaps, net.n_live, 0.99)
    assert n == STEPS
    _same(net.ema, torch.from_numpy(want))


@pytest.mark.parametrize("dtype", ["fp32", "bf16x6"])
def test_improvement_loss_averages_recognition_weights_once_after_the_second_update(dtype):
    tr = _trainer(_net(dtype, **IMP), ema_decay=0.99)
    net = tr.network
    assert net.grads_imp is not None and 0 < net.phi_end < net.n_live
    p0, snaps = _run_tracked(tr)
    assert net.adam_updates == 2 * STEPS
    want, _ = er.track(p0, snaps, net.n_live, 0.99)
    _same(net.ema, torch.from_numpy(want))
    # and training is what it is without averaging
    plain = _trainer(_net(dtype, **IMP))
    for _ in range(STEPS):
        plain.step()
    for a, b in zip(_state(plain.network), _state(net)):
        _same(a, b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x6"])
def test_save_and_load_resume_the_average(dtype, tmp_path):
    kw = dict(ema_decay=0.99, ema_every=1)
    whole = _trainer(_net(dtype), **kw)
    for _ in range(4):
        whole.step()
    first = _trainer(_net(dtype), **kw)
    for _ in range(2):
        first.step()
    first.save(str(tmp_path))
    second = _trainer(_net(dtype, seed=5), **kw)
    second.load(str(tmp_path))
    assert second.network.ema_updates == 2 and second.network.ema_from_checkpoint
    _same(second.network.ema, first.network.ema)
    for _ in range(2):
        second.step()
    _same(second.network.params, whole.network.params)
    _same(second.network.ema, whole.network.ema)
    assert second.network.ema_updates == whole.network.ema_updates == 4


def test_checkpoints_with_and_without_averages_load_either_way(tmp_path):
    from safetensors import safe_open
    plain, avg = _trainer(_net()), _trainer(_net(), ema_decay=0.99)
    for _ in range(2):
        plain.step()
        avg.step()
    pa, pb = str(tmp_path / "plain.safetensors"), str(tmp_path / "avg.safetensors")
    plain.network.save_checkpoint(pa)
    avg.network.save_checkpoint(pb)
    with safe_open(pa, framework="pt") as f:
        assert not [k for k in f.keys() if "ExponentialMovingAverage" in k] and "ema_decay" not in f.metadata()
    with safe_open(pb, framework="pt") as f:
        keys, meta = set(f.keys()), f.metadata()
    live = [p["name"] for p in avg.network.table if p["offset"] + p["size"] <= avg.network.n_live]
    assert {k for k in keys if k.endswith("/ExponentialMovingAverage")} == \
        {n + "/ExponentialMovingAverage" for n in live}
    assert (float(meta["ema_decay"]), meta["ema_warmup"], meta["ema_every"], meta["ema_updates"]) == \
        (0.99, "1", "1", "2")
    # no averages in the file: the average restarts from the loaded parameters
    net = _net(seed=9)
    net.enable_ema(0.99)
    net.ema_updates = 7
    net.load_checkpoint(pa)
    assert net.ema_updates == 0 and not net.ema_from_checkpoint
    _same(net.ema, plain.network.params)
    _same(net.params, plain.network.params)
    # averages in the file, none in the network: ignored, everything else as ever
    net2 = _net(seed=9)
    net2.load_checkpoint(pb)
    assert net2.ema is None and net2.iteration == 2
    for a, b in zip(_state(net2), _state(avg.network)):
        _same(a, b)
    with pytest.raises(RuntimeError, match="enable_ema"):
        net2.averaged()


@pytest.mark.parametrize("dtype", ["fp32", "bf16x6"])
def test_evaluate_on_the_average_equals_a_network_holding_it_and_moves_nothing(dtype):
    tr, twin = _trainer(_net(dtype), ema_decay=0.99), _trainer(_net(dtype), ema_decay=0.99)
    for _ in range(3):
        tr.step()
        twin.step()
    net = tr.network
    before = (tr.state_dict(), net.iteration, net.adam_updates, net.ema_updates)
    got = tr.evaluate(seed=11, weights="ema")
    assert got["weights"] == "ema" and tr.evaluate(seed=11)["weights"] == "train"
    # a fresh network whose parameters are the tracked average
    fresh = _net(dtype, seed=4)
    fresh.params.copy_(net.ema)
    fresh.params_updated()
    want = _trainer(fresh).evaluate(seed=11)
    assert {k: v for k, v in got.items() if k != "weights"} == {k: v for k, v in want.items() if k != "weights"}
    assert got["steps"] != tr.evaluate(seed=11)["steps"]
    # the run: state, parameters, averages, and the next step
    assert before == (tr.state_dict(), net.iteration, net.adam_updates, net.ema_updates)
    for a, b in zip(_state(net) + [net.ema], _state(twin.network) + [twin.network.ema]):
        _same(a, b)
    assert tr.step() == twin.step()
    for a, b in zip(_state(net) + [net.ema], _state(twin.network) + [twin.network.ema]):
        _same(a, b)
    # the averaged context has its own arena: an evaluation on it leaves the training context's last forward
    xh = net.xhat(-1).clone()
    tr.evaluate(seed=11, weights="ema")
    _same(net.xhat(-1), xh)
    with pytest.raises(RuntimeError, match="train the owner"):
        net.averaged().train(tr._input, tr._target)
    with pytest.raises(ValueError, match="weights"):
        tr.evaluate(weights="best")


def test_restore_on_the_average_equals_a_network_holding_it():
    tr = _trainer(_net(), ema_decay=0.99)
    for _ in range(3):
        tr.step()
    net = tr.network
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, 48, 40, C), dtype=np.uint8)
    got = net.restore(img, weights="ema")
    fresh = _net(seed=4)
    fresh.params.copy_(net.ema)
    fresh.params_updated()
    want = fresh.restore(img)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 48, 40, C)
    assert torch.equal(got, want)
    assert not torch.equal(got, net.restore(img))
    gf, wf = net.restore(img, weights="ema", as_uint8=False, seed=3), fresh.restore(img, as_uint8=False, seed=3)
    _same(gf, wf)


def test_trainer_arguments_and_writers(tmp_path):
    import json
    net = _net()
    net.enable_ema(0.9)
    with pytest.raises(ValueError, match="decay"):
        _trainer(net, ema_decay=0.99)
    with pytest.raises(RuntimeError, match="owner"):
        net.sibling(8).enable_ema()
    tr = _trainer(net, ema_decay=0.9, base_dir=str(tmp_path), eval_frequency=2)
    for _ in range(2):
        tr.step()
    rows = [json.loads(s) for s in (tmp_path / "evaluation.jsonl").read_text().splitlines()]
    assert [(r["iteration"], r["weights"]) for r in rows] == [(2, "train"), (2, "ema")]
    assert rows[0]["steps"] != rows[1]["steps"]
    # generate on the averaged weights: through averaged()
    z = torch.zeros(3, B, net.cfg.latent_dim)
    assert not torch.equal(net.averaged().generate(z)[-1], net.generate(z)[-1])
