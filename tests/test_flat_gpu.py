"""Flat generator (generator_flat, sequential_vae.py:1880-1936) on the HIP engine against its float64
restatement (tests/flat_ref.py): tiny_flat (B=4, 32x32x3, T=3, reg 0.7), injected eps and chain noise.

Bounds of tests/test_engine_gpu.py: loss 1e-4 relative, per-image ELBO rtol 1e-4, x_hat_t and sample_t
1e-4 relative L2, gradient vector 1e-3, median per-tensor gradient 1e-4 over tensors with ||g|| > 1e-7.
The restatement's own gradient moves 1.3e-5 (vector) / 4.7e-6 (median) when x moves by 1e-6, so the fixed
bounds hold without widening.  The flat layers are fp32 in every dtype mode; step 0's ladder differs."""
import math

import numpy as np
import pytest
import torch

import flat_ref
from conftest import pkg_mod
from oracle import model, spec

pytestmark = pytest.mark.gpu

REG = 0.7
_L = lambda: pkg_mod("_lib")


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-30))


def _grad_stats(g, ref):
    live = [k for k, v in ref.items() if np.linalg.norm(v) > 1e-7]
    cat = lambda d: np.concatenate([np.ravel(d[k]) for k in live])
    return _rel(cat(g), cat(ref)), float(np.median([_rel(g[k], ref[k]) for k in live]))


def _c1():
    return dict(channels=1, filter_sizes=[1, 8, 8, 16, 24, 16])


def _setup(preset="tiny_flat", base="tiny", batch=4, oracle_over=None, **over):
    cfg = pkg_mod("config").preset(preset, batch=batch, **over)
    net = pkg_mod("sequential_vae").SequentialVAE(cfg, seed=0)
    cd = flat_ref.make_cfg(base, batch=batch, **(oracle_over or {}))
    x, tgt, eps = spec.make_inputs(cd, batch=batch)
    tgt = np.clip(x + 0.1 * np.random.default_rng(9).standard_normal(x.shape).astype(np.float32), *cd["range"])
    noise = spec.make_chain_noise(cd, batch=batch)
    return net, cfg, cd, x, tgt, eps, noise


_ORACLE = {}


def _oracle(key, net, cfg, cd, x, tgt, eps, noise, reg=REG):
    """One float64 run per (configuration, parameters): shared by the tests that need it, never modified."""
    if key in _ORACLE:
        return _ORACLE[key]
    _, struct, fstruct = flat_ref.build_params(cd)
    pub = {k: v.astype(np.float64) for k, v in net.param_dict().items()}
    sh = cfg.share_theta_weights or cfg.share_phi_weights
    params = pub
    if sh:
        params = {p["name"]: pub[flat_ref.shared_name(p["name"], cfg.share_theta_weights, cfg.share_phi_weights)]
                  for p in flat_ref.build_params(cd)[0]}
    o = flat_ref.forward_backward_flat(cd, struct, fstruct, params, x, tgt, eps, reg, noise)
    if sh:
        o["grads"] = flat_ref.sum_shared_grads(o["grads"], cfg.share_theta_weights, cfg.share_phi_weights)
    _ORACLE[key] = o
    return o


def _check_fwd(net, cfg, o, reg=REG):
    stats = net.step_stats().cpu().numpy()
    loss = net.loss_value(stats, reg)
    print("loss %.8e oracle %.8e" % (loss, o["loss"]))
    assert abs(loss - o["loss"]) <= 1e-4 * abs(o["loss"]), (loss, o["loss"])
    np.testing.assert_allclose(net.elbo_per_image().cpu().numpy(), o["elbo_img"], rtol=1e-4)
    for t in range(cfg.mc_steps):
        ex = _rel(net.xhat(t).cpu().numpy(), o["xhat"][t])
        es = _rel(net.sample(t).cpu().numpy(), o["sample"][t])
        print("step %d xhat %.2e sample %.2e" % (t, ex, es))
        assert ex <= 1e-4 and es <= 1e-4, (t, ex, es)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x6"])
@pytest.mark.parametrize("preset", ["tiny_flat", "tiny_flat_homog"])
def test_flat_fwd_bwd_matches_restatement(preset, dtype):
    net, cfg, cd, x, tgt, eps, noise = _setup(preset, dtype=dtype)
    net.forward(x, tgt, eps, REG, noise=noise)
    net.backward()
    torch.cuda.synchronize()
    o = _oracle((preset, "init"), net, cfg, cd, x, tgt, eps, noise)
    _check_fwd(net, cfg, o)
    gv, gm = _grad_stats(net.grad_dict(), o["grads"])
    print("grads vector %.2e median %.2e" % (gv, gm))
    assert gv <= 1e-3 and gm <= 1e-4, (gv, gm)
    for k, v in o["grads"].items():
        if np.linalg.norm(v) <= 1e-7:
            assert np.abs(net.grad_dict()[k]).max() <= 1e-5, k
    # d loss / d z_t through the generator: the ladder's at step 0, nothing at a flat step (KL only)
    Dz = cfg.latent_dim
    for t in range(cfg.mc_steps):
        dz = net.copy_out(_L().BUF_DZ, t, cfg.batch * Dz).cpu().numpy().reshape(cfg.batch, Dz)
        if t == 0:
            print("dz_0 rel %.2e" % _rel(dz, o["dz"][0]))
        else:
            assert np.abs(dz - o["dz"][t]).max() <= 1e-4 * max(1.0, np.abs(o["dz"][0]).max())
            assert np.abs(dz).max() == 0.0
    # run to run bitwise
    g1 = net.grads.clone()
    net.forward(x, tgt, eps, REG, noise=noise)
    net.backward()
    torch.cuda.synchronize()
    assert torch.equal(g1, net.grads)
    assert net.grads[net.n_live:].abs().max().item() == 0.0


def test_flat_single_channel():
    """C = 1: flat sizes 1, 2, 4, 8, 4, 2, 1 (the MNIST netname's channel widths)."""
    oo = dict(C=1, filter_sizes=[1, 8, 8, 16, 24, 16])
    net, cfg, cd, x, tgt, eps, noise = _setup(oracle_over=oo, **_c1())
    assert cfg.flat_sizes() == [1, 2, 4, 8, 4, 2, 1]
    net.forward(x, tgt, eps, REG, noise=noise)
    net.backward()
    torch.cuda.synchronize()
    o = _oracle(("c1", "init"), net, cfg, cd, x, tgt, eps, noise)
    _check_fwd(net, cfg, o)
    gv, gm = _grad_stats(net.grad_dict(), o["grads"])
    print("grads vector %.2e median %.2e" % (gv, gm))
    assert gv <= 1e-3 and gm <= 1e-4, (gv, gm)


def test_flat_train_step_matches_adam_of_restatement():
    net, cfg, cd, x, tgt, eps, noise = _setup()
    twin, *_ = _setup()
    p0 = {k: v.astype(np.float64) for k, v in net.param_dict().items()}
    reg = 1.0 - math.exp(-1 / cfg.reg_coeff_rate)
    o = _oracle(("tiny_flat", "train-reg"), net, cfg, cd, x, tgt, eps, noise, reg)
    net.train(x, tgt, eps=eps, noise=noise)
    torch.cuda.synchronize()
    assert net.adam_updates == 1
    live = [p["name"] for p in net.table if not p["zero_grad"]]
    m = {k: np.zeros_like(p0[k]) for k in live}
    v = {k: np.zeros_like(p0[k]) for k in live}
    p1, _, _ = model.adam_update({k: p0[k] for k in live}, {k: o["grads"][k] for k in live}, m, v, 1)
    got = net.param_dict()
    d = np.concatenate([np.ravel(got[k] - p1[k]) for k in live])
    du_e = np.concatenate([np.ravel(got[k] - p0[k]) for k in live])
    du_o = np.concatenate([np.ravel(p1[k] - p0[k]) for k in live])
    upd = float(np.linalg.norm(du_e - du_o) / np.linalg.norm(du_o))
    print("train step: max|d| %.2e update rel L2 %.2e" % (np.abs(d).max(), upd))
    assert upd <= 0.1 and np.abs(d).max() <= 2.5 * cfg.learning_rate
    flat = [k for k in live if "generative_flat_step_" in k]
    assert flat and all(np.abs(got[k] - p0[k]).max() > 0 for k in flat)
    # a second train() (backward_apply) == backward + apply_gradients on a twin, bit for bit
    twin.train(x, tgt, eps=eps, noise=noise)
    assert torch.equal(twin.params, net.params)
    net.train(x, tgt, eps=eps, noise=noise)
    twin.iteration += 1
    twin.learning_rate *= twin.cfg.learning_rate_decay
    twin.forward(x, tgt, eps, 1.0 - math.exp(-2 / cfg.reg_coeff_rate), noise=noise)
    twin.backward()
    twin.apply_gradients(twin.learning_rate)
    torch.cuda.synchronize()
    assert torch.equal(twin.params, net.params)


def test_flat_generate_matches_restatement():
    net, cfg, cd, x, tgt, eps, noise = _setup()
    z = np.random.default_rng(4).standard_normal((cfg.mc_steps, cfg.batch, cfg.latent_dim)).astype(np.float32)
    outs = net.generate(z, noise=noise)
    torch.cuda.synchronize()
    _, struct, fstruct = flat_ref.build_params(cd)
    params = {k: v.astype(np.float64) for k, v in net.param_dict().items()}
    ref = flat_ref.generate_flat(cd, struct, fstruct, params, z, noise, 1.0)
    lo, hi = cfg.range
    for t in range(cfg.mc_steps):
        got = outs[t].cpu().numpy()
        e = _rel(got, ref[t])
        print("generate step %d %.2e" % (t, e))
        assert e <= 1e-4
        assert got.min() >= lo - 1e-6 and got.max() <= hi + 1e-6


def test_flat_checkpoint_resume_bitwise(tmp_path):
    net, cfg, cd, x, tgt, eps, noise = _setup()
    net.train(x, tgt, eps=eps, noise=noise)
    path = str(tmp_path / "flat.safetensors")
    net.save_checkpoint(path)
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        keys = set(f.keys())
    for k in ("theta/generative_flat_step_1/Conv_5/weights", "theta/generative_flat_step_1/Conv_5/weights/Adam",
              "theta/generative_flat_step_1/Conv_5/weights/Adam_1", "theta/generative_flat_step_2/BatchNorm/beta"):
        assert k in keys, k
    other, *_ = _setup()
    other.load_checkpoint(path)
    a = net.train(x, tgt, eps=eps, noise=noise)
    b = other.train(x, tgt, eps=eps, noise=noise)
    torch.cuda.synchronize()
    assert a == b and torch.equal(net.params, other.params)


def test_c_infusion_test_engine_width():
    """The netname's real width (64x64, flat channels 3..24) at B=4, two steps = one flat step."""
    net, cfg, cd, x, tgt, eps, noise = _setup("c_infusion_test", "celeba", 4, dict(mc_steps=2), mc_steps=2)
    net.forward(x, tgt, eps, REG, noise=noise)
    net.backward()
    torch.cuda.synchronize()
    o = _oracle(("c_infusion", "init"), net, cfg, cd, x, tgt, eps, noise)
    _check_fwd(net, cfg, o)
    assert torch.isfinite(net.grads).all()
