"""Flat generator (generator_flat, sequential_vae.py:1880-1936): configuration, parameter table,
presets and gradient buckets of the engine against the float64 restatement's table (tests/flat_ref.py).
Host only."""
import ctypes

import numpy as np
import pytest

import flat_ref
from conftest import pkg_mod
from oracle import weightgen

KEY = lambda p: (p["name"], tuple(p["shape"]), p["dead"], p["zero_grad"], p["init"])
BASE = {"tiny_flat": "tiny", "c_infusion_test": "celeba"}


@pytest.mark.parametrize("preset", ["tiny_flat", "c_infusion_test"])
def test_flat_layout_matches_restatement(built_lib, preset):
    W = pkg_mod("weights")
    cfg = pkg_mod("config").preset(preset)
    table, n_total, n_live = W.param_table(cfg)
    otab = flat_ref.build_params(flat_ref.make_cfg(BASE[preset]))[0]
    assert sorted(map(KEY, table)) == sorted(map(KEY, otab))
    names = [p["name"] for p in table]
    assert not [n for n in names if "generative_encoder" in n]
    assert not [n for n in names if n.startswith("theta/generative_step_") and not n.startswith("theta/generative_step_0/")]
    for t in range(1, cfg.mc_steps):
        assert "theta/generative_flat_step_%d/Conv_5/weights" % t in names
        assert "theta/generative_flat_step_%d/BatchNorm_4/beta" % t in names
    spans = sorted((p["offset"], p["offset"] + p["size"], p["dead"] or p["zero_grad"]) for p in table)
    pos = 0
    for a, b, frozen in spans:
        assert a % 64 == 0 and a >= pos
        assert (a >= n_live) == frozen
        pos = b
    assert pos <= n_total and n_live % 64 == 0


def test_flat_homog_layout_matches_sharing(built_lib):
    W, cfgmod = pkg_mod("weights"), pkg_mod("config")
    for preset, base in [("tiny_flat_homog", "tiny"), ("c_homog_infusion_test", "celeba")]:
        table, n_total, n_live = W.param_table(cfgmod.preset(preset))
        ref = flat_ref.shared_table(flat_ref.make_cfg(base), True, True)
        assert sorted(map(KEY, table)) == sorted(map(KEY, ref))
        names = [p["name"] for p in table]
        assert "theta/generative_network_flat/Conv_5/weights" in names
        assert not [n for n in names if "generative_flat_step_" in n or "generative_encoder" in n]
        for p in table:
            assert (p["offset"] < n_live) == (not p["zero_grad"]), p["name"]


@pytest.mark.parametrize("preset", ["tiny_flat", "c_infusion_test", "m_infusion_test"])
def test_flat_step_buckets_tile_live_region(built_lib, preset):
    W, par = pkg_mod("weights"), pkg_mod("parallel")
    cfg = pkg_mod("config").preset(preset)
    table, _, n_live = W.param_table(cfg)
    theta, phi = par.step_buckets(table, n_live)
    assert [t for t, _, _ in theta] == list(range(cfg.mc_steps - 1, -1, -1))
    ranges = sorted([phi] + [(lo, hi) for _, lo, hi in theta])
    assert ranges[0][0] == 0 and ranges[-1][1] == n_live
    for (a, b), (c, d) in zip(ranges, ranges[1:]):
        assert b == c and a < b
    for t, lo, hi in theta:  # a flat step's bucket holds exactly its flat scope
        if t >= 1:
            inside = [p["name"] for p in table if lo <= p["offset"] < hi]
            assert inside and all(n.startswith("theta/generative_flat_step_%d/" % t) for n in inside)


REJECT = [
    (dict(add_noise_to_chain=False), b"add_noise_to_chain"),
    (dict(predict_generator_noise=True), b"predict_generator_noise"),
    (dict(predict_latent_code=True), b"predict_latent_code"),
    (dict(add_improvement_maximization_loss=True), b"add_improvement_maximization_loss"),
    (dict(external_generator_from=1), b"external_generator_from"),
    (dict(flat_conv_layers=0), b"flat_conv_layers"),
    (dict(flat_conv_layers=9, flat_conv_filter_sizes=(3,) * 10), b"flat_conv_layers"),
    (dict(flat_conv_filter_sizes=(3, 6, 33, 24, 12, 6, 3)), b"flat_conv_filter_sizes"),
    (dict(flat_conv_filter_sizes=(3, 6, 0, 24, 12, 6, 3)), b"flat_conv_filter_sizes"),
]


@pytest.mark.parametrize("over,field", REJECT)
def test_flat_rejected_combinations(built_lib, over, field):
    L = pkg_mod("_lib")
    c = pkg_mod("config").preset("tiny_flat", **over).to_c()
    n = ctypes.c_int64()
    assert L.lib().svae_param_count(ctypes.byref(c), ctypes.byref(n), None, None) == -1
    msg = L.lib().svae_last_error(None)
    assert b"flat_generator" in msg or field.startswith(b"flat_"), msg
    assert field in msg, msg


def test_infusion_netnames_resolve(built_lib):
    cfgmod = pkg_mod("config")
    c = cfgmod.preset("c_infusion_test")
    assert c.flat_generator and c.add_noise_to_chain and c.mc_steps == 8 and not c.share_theta_weights
    h = cfgmod.preset("c_homog_infusion_test")
    assert h.flat_generator and h.share_theta_weights and h.share_phi_weights and h.mc_steps == 8
    m = cfgmod.preset("m_infusion_test")
    assert (m.height, m.channels, m.levels, m.mc_steps, m.batch) == (32, 1, 3, 5, 64)
    assert m.latent_dims == [2, 2, 2] and m.filter_sizes == [1, 64, 128, 192, 256] and m.range == (0.0, 1.0)
    assert c.flat_sizes() == [3, 6, 12, 24, 12, 6, 3] and m.flat_sizes() == [1, 2, 4, 8, 4, 2, 1]
    cc = c.to_c()
    assert cc.flat_generator == 1 and cc.flat_conv_layers == 6
    assert [cc.flat_conv_filter_sizes[i] for i in range(7)] == [3, 6, 12, 24, 12, 6, 3]
    d = c.as_dict()
    assert d["flat_generator"] and d["flat_conv_layers"] == 6 and d["flat_conv_filter_sizes"][3] == 24
    W = pkg_mod("weights")
    for name in ("c_infusion_test", "c_homog_infusion_test", "m_infusion_test"):
        assert W.param_table(cfgmod.preset(name))[2] > 0
    # the default presets do not change: the new fields are off
    assert not cfgmod.preset("celeba").flat_generator and cfgmod.preset("celeba").to_c().flat_generator == 0


def test_flat_weight_generators_agree(built_lib):
    W = pkg_mod("weights")
    table, _, _ = W.param_table(pkg_mod("config").preset("tiny_flat"))
    flat = [p for p in table if "generative_flat_step_" in p["name"]]
    assert len(flat) == 2 * (5 * 3 + 2)
    for p in flat:
        a = W.init_value(p["name"], p["shape"], p["init"], 7)
        b = weightgen.generate(p["name"], p["shape"], p["init"], 7).ravel()
        np.testing.assert_array_equal(a, b)
