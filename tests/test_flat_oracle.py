"""The float64 restatement of the flat generator (tests/flat_ref.py) checked on its own: its gradient
against central differences, and the recognition ladder of a flat step sees the KL term only."""
import numpy as np

import flat_ref
from oracle import spec

REG = 0.7


def _small():
    cfg = flat_ref.make_cfg("tiny", H=8, W=8, levels=2, filter_sizes=[3, 8, 8, 16], latent_dims=[2, 2],
                            mc_steps=2, batch=2)
    table, struct, fstruct, params = flat_ref.init_params(cfg, seed=3)
    rng = np.random.default_rng(11)
    for p in table:  # away from the all-zero betas / biases, so every coordinate has a gradient
        if p["init"] == "zeros" and not p["zero_grad"]:
            params[p["name"]] = 0.1 * rng.standard_normal(p["shape"])
    x, tgt, eps = spec.make_inputs(cfg, batch=2)
    tgt = np.clip(x + 0.1 * rng.standard_normal(x.shape), -1, 1)
    noise = spec.make_chain_noise(cfg, batch=2)
    return cfg, table, struct, fstruct, params, x, tgt, eps, noise


def test_flat_ref_gradient_matches_central_differences():
    cfg, table, struct, fstruct, params, x, tgt, eps, noise = _small()
    run = lambda p, g=False: flat_ref.forward_backward_flat(cfg, struct, fstruct, p, x, tgt, eps, REG, noise, want_grads=g)
    grads = run(params, True)["grads"]
    names = ["theta/generative_flat_step_1/Conv/weights", "theta/generative_flat_step_1/Conv_2/weights",
             "theta/generative_flat_step_1/Conv_4/weights", "theta/generative_flat_step_1/Conv_5/weights",
             "theta/generative_flat_step_1/BatchNorm/beta", "theta/generative_flat_step_1/BatchNorm_3/beta",
             "theta/generative_flat_step_1/Conv_5/biases", "theta/generative_step_0/Conv2d_transpose_1/weights",
             "theta/generative_step_0/fully_connected_2/weights", "theta/generative_step_0/Conv2d_transpose_2/weights"]
    rng = np.random.default_rng(5)
    h, worst, n = 1e-5, 0.0, 0
    for name in names:
        for _ in range(3):
            idx = tuple(int(rng.integers(0, s)) for s in params[name].shape)
            vals = []
            for sgn in (1.0, -1.0):
                p = dict(params)
                p[name] = params[name].copy()
                p[name][idx] += sgn * h
                vals.append(run(p)["loss"])
            cd = (vals[0] - vals[1]) / (2 * h)
            g = grads[name][idx]
            rel = abs(cd - g) / max(abs(g), abs(cd), 1e-300)
            print("%-60s %s cd %.10e grad %.10e rel %.2e" % (name, idx, cd, g, rel))
            worst = max(worst, rel)
            n += 1
    assert n >= 20
    assert worst <= 1e-5, worst


def test_flat_step_latent_sees_only_its_kl_term():
    """Nothing in generator_flat reads z_1: d loss / d z_1 through the generator is zero, and the
    recognition ladder of step 1 receives exactly the gradient of reg * mean_b KL_1."""
    cfg, table, struct, fstruct, params, x, tgt, eps, noise = _small()
    o = flat_ref.forward_backward_flat(cfg, struct, fstruct, params, x, tgt, eps, REG, noise)
    assert np.abs(o["dz"][1]).max() == 0.0
    assert np.abs(o["dz"][0]).max() > 0.0
    kl = flat_ref.kl_term_grads(cfg, struct, params, x, REG, 1)
    seen = 0
    for k, g in o["grads"].items():
        if k.startswith("phi/inference_step_1/"):
            np.testing.assert_allclose(g, kl[k], rtol=1e-12, atol=1e-18)
            seen += np.abs(g).max() > 0
    assert seen >= 4
