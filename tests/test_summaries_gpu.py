"""SequentialVAE.summaries() and the trainer's summaries.jsonl on the GPU.

Every scalar is recomputed in float64 (math.fsum, exactly rounded sums) from what the network hands out:
param_dict(), grad_dict() clipped at +-clip_grad_value, latent(SVAE_BUF_MU / SIGMA, t) with the mean clamped,
step_stats().  Bound: the kernel adds at most n = n_total fp64 terms per sum, so a sum is within
n 2^-52 sum |term| (tests/stats_ref.py); a norm is the square root of such a sum of non-negative terms and
inherits the relative bound n 2^-52, a ratio of two norms twice that; 16 more units for the handful of
float64 operations on the host.  Loss terms are copies of fp32 values (exact), counts and maxima are exact.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import pkg_mod

pytestmark = pytest.mark.gpu


def _net(preset="tiny", seed=0, **over):
    cfg = pkg_mod("config").preset(preset, batch=4, dtype="fp32", **over)
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _batch(seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(4, 32, 32, 3, generator=g) * 2 - 1).cuda()


def _fsum(a):
    return math.fsum(np.ravel(a).astype(np.float64).tolist())


def _expected(net, lr):
    """{name: (value, absolute bound)} from the network's own accessors, in float64."""
    L = pkg_mod("_lib")
    cfg = net.cfg
    T, clip = cfg.mc_steps, cfg.clip_grad_value
    u = (net.n_total + 16) * 2.0 ** -52
    P, G = net.param_dict(), net.grad_dict()
    st = net.step_stats().double().cpu().numpy()
    exp = {"loss": (net.loss_value(), 0.0)}
    noise = cfg.noise_list()
    for t in range(T):
        mu = np.clip(net.latent(L.BUF_MU, t).double().cpu().numpy(), -cfg.latent_mean_clip, cfg.latent_mean_clip)
        sig = net.latent(L.BUF_SIGMA, t).double().cpu().numpy()
        exp["reconstruction_loss_step_%d" % t] = (st[t, 0], 0.0)
        exp["regularization_loss_step_%d" % t] = (st[t, 1], 0.0)
        mag = _fsum(np.abs(mu)) / mu.size
        exp["latent_mean_avg_magnitude_step_%d" % t] = (mag, u * mag)
        exp["latent_mean_avg_step_%d" % t] = (_fsum(mu) / mu.size, u * mag)
        exp["latent_stddev_avg_step_%d" % t] = (_fsum(sig) / sig.size, u * _fsum(np.abs(sig)) / sig.size)
        exp["training_stddev_avg_magnitude_step_%d" % t] = (abs(noise[t]) if cfg.add_noise_to_chain else 0.0, 0.0)
    norm = {}
    for grp in ("theta", "phi"):
        names = [p["name"] for p in net.table if grp in p["name"]]
        wn = math.sqrt(math.fsum(_fsum(np.square(P[k].astype(np.float64))) for k in names))
        gc = {k: np.clip(G[k].astype(np.float64), -clip, clip) for k in names}
        gn = math.sqrt(math.fsum(_fsum(np.square(gc[k])) for k in names))
        norm[grp] = (wn, gn)
        exp["%s_weights_norm" % grp] = (wn, u * wn)
        exp["%s_elbo_grads_norm" % grp] = (gn, u * gn)
        exp["%s_elbo_update_ratio" % grp] = (lr * gn / wn, 2 * u * lr * gn / wn)
        n = sum(G[k].size for k in names)
        exp["debug/%s_grads_clipped_fraction" % grp] = (sum(int((np.abs(G[k]) > clip).sum()) for k in names) / n, 0.0)
        exp["debug/%s_grads_max_abs" % grp] = (max(float(np.abs(G[k]).max()) for k in names), 0.0)
    exp["debug/grads_nonfinite"] = (0.0, 0.0)
    exp["debug/weights_nonfinite"] = (0.0, 0.0)
    return exp


def _check(net, lr, got=None):
    S = pkg_mod("summaries")
    exp = _expected(net, lr)
    got = net.summaries(lr) if got is None else got
    assert list(got) == S.summary_names(net.cfg) and set(got) == set(exp)
    for k, (want, bound) in exp.items():
        assert abs(got[k] - want) <= bound, (k, got[k], want, bound)
    return got


@pytest.mark.parametrize("preset", ["tiny", "tiny_flat"])
def test_summaries_match_float64_formulas(preset):
    net = _net(preset)
    x = _batch()
    net.forward(x, x, None, 0.7)
    net.backward()
    got = _check(net, 3e-4)
    assert got["theta_elbo_grads_norm"] > 0.0 and got["phi_elbo_grads_norm"] > 0.0
    assert got["loss"] == net.loss_value() and got["latent_stddev_avg_step_0"] > 0.0
    # lr defaults to the network's learning rate
    d = net.summaries()
    assert d["phi_elbo_update_ratio"] == net.learning_rate * d["phi_elbo_grads_norm"] / d["phi_weights_norm"]
    assert {k: v for k, v in d.items() if "ratio" not in k} == {k: v for k, v in got.items() if "ratio" not in k}
    # the frozen tail: parameters counted in the weight norms, gradient statistics zero
    sm = net._summaries
    rows = sm.res.cpu().numpy()[:sm.rows * 8].reshape(sm.rows, 8)
    tab = sorted(net.table, key=lambda p: p["offset"])
    tail = [i for i, p in enumerate(tab) if p["offset"] >= net.n_live]
    assert tail and any("theta" in tab[i]["name"] for i in tail) and any("phi" in tab[i]["name"] for i in tail)
    for i in tail:
        assert rows[sm.r_grads + i].tolist() == [float(tab[i]["size"]), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        assert rows[sm.r_params + i, 0] == tab[i]["size"]


def test_latent_mean_clip_enters_the_latent_scalars():
    L = pkg_mod("_lib")
    net = _net("tiny", latent_mean_clip=0.5)
    for p in net.table:  # head biases of +-1: raw means beyond the clip
        if p["name"].startswith("phi/") and "fully_connected" in p["name"] and p["name"].endswith("/biases") \
                and p["offset"] < net.n_live:
            net.set_param(p["name"], np.resize(np.array([1.0, -1.0], dtype=np.float32), p["shape"]))
    x = _batch(6)
    net.forward(x, x, None, 1.0)
    net.backward()
    raw = torch.stack([net.latent(L.BUF_MU, t) for t in range(3)]).abs()
    assert (raw > 0.5).any() and (raw < 0.5).any()  # the clamp matters, and not everywhere
    got = _check(net, 1e-3)
    for t in range(3):
        assert got["latent_mean_avg_magnitude_step_%d" % t] <= 0.5
        assert got["latent_mean_avg_magnitude_step_%d" % t] < float(raw[t].double().mean())


def test_clipped_fraction_and_max_abs():
    net = _net("tiny")
    x = _batch(7)
    net.forward(x, x, None, 1.0)
    net.backward()
    before = net.summaries()
    p = net._by_name["theta/generative_step_0/Conv2d_transpose_1/weights"]
    g = net.grads[p["offset"]:p["offset"] + p["size"]]
    g *= 15.0 / float(g.abs().max())  # in place: the largest entry is now 15, part of the tensor beyond +-10
    n_over = int((g.abs() > 10.0).sum())
    assert 0 < n_over < p["size"]
    got = _check(net, 1e-3)
    n_theta = sum(q["size"] for q in net.table if "theta" in q["name"])
    assert got["debug/theta_grads_max_abs"] == float(g.abs().max()) and got["debug/theta_grads_max_abs"] > 14.9
    if before["debug/theta_grads_clipped_fraction"] == 0.0:
        assert got["debug/theta_grads_clipped_fraction"] == n_over / n_theta
    assert got["debug/phi_grads_clipped_fraction"] == before["debug/phi_grads_clipped_fraction"]
    # the norm is that of the clipped gradient, not of the raw one
    raw = math.sqrt(float(sum(net.grads[q["offset"]:q["offset"] + q["size"]].double().square().sum()
                              for q in net.table if "theta" in q["name"])))
    assert got["theta_elbo_grads_norm"] < raw


def test_non_finite_gradients_are_counted():
    net = _net("tiny")
    x = _batch(8)
    net.forward(x, x, None, 1.0)
    net.backward()
    clean = net.summaries()
    p = net._by_name["phi/inference_step_1/Conv_1/weights"]
    net.grads[p["offset"] + 3] = float("nan")
    net.grads[p["offset"] + 10] = float("inf")
    got = net.summaries()
    assert got["debug/grads_nonfinite"] == 2.0 and clean["debug/grads_nonfinite"] == 0.0
    assert all(math.isfinite(v) for v in got.values())
    assert got["theta_elbo_grads_norm"] == clean["theta_elbo_grads_norm"]


def test_summaries_before_any_forward_raise():
    net = _net("tiny")
    with pytest.raises(RuntimeError, match="forward"):
        net.summaries()


def test_improvement_loss_scalars():
    L = pkg_mod("_lib")
    net = _net("tiny", predict_latent_code=True, add_improvement_maximization_loss=True)
    x = _batch(9)
    net.forward(x, x, None, 0.6)
    net.backward()
    net.backward_imp()
    got = net.summaries(2e-4)
    assert list(got) == pkg_mod("summaries").summary_names(net.cfg)
    u = (net.n_total + 16) * 2.0 ** -52
    tot = 0.0
    for t in (1, 2):
        img = net.copy_out(L.BUF_IMP_IMG, t, 4).double().cpu().numpy()
        want = -0.6 * net.cfg.latent_pred_loss_coeff * float(img.mean())
        assert abs(got["improvement_maximization_loss_step_%d" % t] - want) <= 4 * 2.0 ** -52 * abs(want)
        tot += got["improvement_maximization_loss_step_%d" % t]
    assert abs(tot - net.imp_loss_value()) <= 1e-12 * abs(tot)
    gi = net.grads_imp.cpu().numpy().astype(np.float64)
    want = math.sqrt(math.fsum(_fsum(np.square(np.clip(gi[p["offset"]:p["offset"] + p["size"]], -10.0, 10.0)))
                               for p in net.table if "phi" in p["name"]))
    assert abs(got["phi_latent_pred_grads_norm"] - want) <= u * want and want > 0.0
    ratio = 2e-4 * want / got["phi_weights_norm"]
    assert abs(got["phi_latent_pred_update_ratio"] - ratio) <= 2 * u * ratio


def test_training_is_bitwise_unchanged_by_summaries():
    a, b = _net("tiny", seed=3), _net("tiny", seed=3)
    for k in range(3):
        x = _batch(20 + k)
        la, lb = a.train(x, x), b.train(x, x)
        assert la == lb
        s = b.summaries()
        assert s["reconstruction_loss_step_2"] / 32 / 32 == lb  # the step's own loss term
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    # after train(): the updated weights, and the gradients that produced the update
    _check(b, b.learning_rate)


def _dataset():
    return pkg_mod("data").DeviceDataset.synthetic(20, 32, 32, 3, seed=3, test_fraction=0.4, device="cuda")


def test_trainer_writes_summaries_jsonl(tmp_path):
    S, NT = pkg_mod("summaries"), pkg_mod("trainer").NoisyTrainer
    net = _net("tiny")
    base = str(tmp_path / "run")
    tr = NT(net, _dataset(), base_dir=base, seed=1, summary_freq=2)
    for _ in range(4):
        tr.step()
    lines = [json.loads(l) for l in open(os.path.join(base, "summaries.jsonl"))]
    assert [l["iteration"] for l in lines] == [2, 4]
    keys = ["iteration", "learning_rate", "reg_coeff"] + S.summary_names(net.cfg)
    for l in lines:
        assert list(l) == keys
        assert l["learning_rate"] == net.cfg.learning_rate and 0.0 < l["reg_coeff"] < 1.0
    assert lines[1] == {**{k: lines[1][k] for k in keys[:3]}, **net.summaries()}
    assert sorted(os.listdir(base)) == ["summaries.jsonl"]


def test_trainer_default_writes_no_summaries(tmp_path):
    NT = pkg_mod("trainer").NoisyTrainer
    net = _net("tiny")
    base = str(tmp_path / "run")
    tr = NT(net, _dataset(), base_dir=base, seed=1)
    assert tr.summary_freq == 0
    for _ in range(2):
        tr.step()
    assert not os.path.exists(base) and getattr(net, "_summaries", None) is None
    tr.save(base)
    assert sorted(os.listdir(base)) == ["model.safetensors", "trainer.json"]
