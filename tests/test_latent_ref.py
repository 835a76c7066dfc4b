"""tests/latent_ref.py (the numpy float64 reference of svae_op_mixture_logdensity and latents.information) against
closed forms; no GPU."""
import math

import numpy as np

import latent_ref as R


def _rand(rng, n, d):
    mu = rng.normal(0, 1, (n, d))
    sigma = np.exp(rng.uniform(math.log(1e-2), 0.0, (n, d)))
    return mu, sigma


def test_one_component_is_the_gaussian_log_density():
    rng = np.random.default_rng(0)
    mu, sigma = _rand(rng, 1, 5)
    z = rng.normal(0, 1, (7, 5))
    got = R.mixture_logdensity(z, mu, sigma, [(0, 5), (1, 3), (4, 1)])
    t = -0.5 * ((z - mu) / sigma) ** 2 - np.log(sigma) - 0.5 * math.log(2 * math.pi)
    want = np.stack([t.sum(1), t[:, 1:4].sum(1), t[:, 4]], axis=1)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-14)
    # against the textbook normal pdf, written independently
    pdf = np.exp(-(z[:, 4] - mu[0, 4]) ** 2 / (2 * sigma[0, 4] ** 2)) / (sigma[0, 4] * math.sqrt(2 * math.pi))
    np.testing.assert_allclose(np.exp(got[:, 2]), pdf, rtol=1e-12)


def test_two_identical_components_add_log_two():
    rng = np.random.default_rng(1)
    mu, sigma = _rand(rng, 1, 4)
    z = rng.normal(0, 2, (5, 4))
    segs = [(0, 4), (2, 2)]
    one = R.mixture_logdensity(z, mu, sigma, segs)
    two = R.mixture_logdensity(z, np.repeat(mu, 2, 0), np.repeat(sigma, 2, 0), segs)
    np.testing.assert_allclose(two, one + math.log(2.0), rtol=1e-14, atol=1e-14)


def test_a_segment_ignores_the_other_dimensions():
    rng = np.random.default_rng(2)
    mu, sigma = _rand(rng, 6, 5)
    mu[:, 3:], sigma[:, 3:] = mu[0, 3:], sigma[0, 3:]   # every component identical outside [0, 3)
    z = rng.normal(0, 1, (9, 5))
    a = R.mixture_logdensity(z, mu, sigma, [(0, 3)])
    z2, mu2, sigma2 = z.copy(), mu.copy(), sigma.copy()
    z2[:, 3:] += 5.0
    mu2[:, 3:] -= 2.0
    sigma2[:, 3:] *= 0.5
    assert np.array_equal(a, R.mixture_logdensity(z2, mu2, sigma2, [(0, 3)]))
    # and the whole code factorises into that segment times the shared rest
    whole = R.mixture_logdensity(z, mu, sigma, [(0, 5)])[:, 0]
    rest = R.log_normal(z[:, 3:], mu[0, 3:], sigma[0, 3:]).sum(1)
    np.testing.assert_allclose(whole, a[:, 0] + rest, rtol=1e-13, atol=1e-13)


def _draw(rng, mean, sigma):
    return mean + sigma * rng.normal(0, 1, mean.shape)


def test_kl_sample_is_mi_plus_marginal_kl_and_mi_is_below_log_n():
    rng = np.random.default_rng(3)
    dims = [2, 1, 3]
    for n in (2, 10, 33):
        mean, sigma = _rand(rng, n, 6)
        res = R.information(_draw(rng, mean, sigma), mean, sigma, dims, 0.7)
        assert res["mi_ceiling"] == math.log(n) and res["nonfinite"] == 0
        for e in [res["all"]] + res["levels"]:
            assert abs(e["kl_sample"] - (e["mi"] + e["marginal_kl"])) <= 1e-12 * max(1.0, abs(e["kl_sample"]))
            assert e["mi"] <= math.log(n) + 1e-12
        assert all(v <= math.log(n) + 1e-12 for v in res["dims"]["mi"])
        assert len(res["levels"]) == 3 and len(res["dims"]["mi"]) == 6
        # the analytic KL of the whole code is the sum of its dimensions'
        assert abs(res["all"]["kl"] - sum(res["dims"]["kl"])) <= 1e-12 * abs(res["all"]["kl"])


def test_identical_product_posteriors_carry_nothing():
    rng = np.random.default_rng(4)
    n, dims = 50, [2, 2]
    mean = np.tile(rng.normal(0, 1, (1, 4)), (n, 1))
    sigma = np.tile(np.exp(rng.uniform(-2, 0, (1, 4))), (n, 1))
    res = R.information(_draw(rng, mean, sigma), mean, sigma, dims, 1.0)
    for e in [res["all"]] + res["levels"]:
        assert abs(e["mi"]) <= 1e-12 and abs(e["tc"]) <= 1e-12 and e["active_units"] == 0
    assert max(abs(v) for v in res["dims"]["mi"]) <= 1e-12


def test_far_apart_posteriors_saturate_at_log_n():
    rng = np.random.default_rng(5)
    n, dims = 20, [1, 2]
    mean = 100.0 * np.arange(n)[:, None] + rng.normal(0, 1, (n, 3))
    sigma = np.full((n, 3), 0.1)
    res = R.information(_draw(rng, mean, sigma), mean, sigma, dims, 1.0)
    assert abs(res["all"]["mi"] - math.log(n)) <= 1e-12
    assert all(abs(v - math.log(n)) <= 1e-12 for v in res["dims"]["mi"])
    assert res["all"]["active_units"] == 3 and [e["active_units"] for e in res["levels"]] == [1, 2]


def test_uniform_prior_has_no_prior_terms():
    rng = np.random.default_rng(6)
    mean, sigma = _rand(rng, 8, 3)
    res = R.information(_draw(rng, mean, sigma), mean, sigma, [3], None)
    e = res["all"]
    assert e["marginal_kl"] is None and e["kl_sample"] is None and e["kl"] is None
    assert math.isfinite(e["mi"]) and math.isfinite(e["tc"])
    assert res["dims"]["marginal_kl"] is None and res["dims"]["kl"] is None and len(res["dims"]["mi"]) == 3


def test_segments_for_order():
    assert R.segments_for([2, 1]) == [("all", 0, 3), ("level0", 0, 2), ("level1", 2, 1), ("dim0", 0, 1),
                                      ("dim1", 1, 1), ("dim2", 2, 1)]
    from conftest import pkg_mod
    for name in ("tiny", "celeba", "lsun"):
        cfg = pkg_mod("config").preset(name)
        segs = pkg_mod("latents").segments_for(cfg)
        assert segs == R.segments_for(cfg.latent_dims)
        assert len(segs) == 1 + cfg.levels + cfg.latent_dim and segs[0] == ("all", 0, cfg.latent_dim)
