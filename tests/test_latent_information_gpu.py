"""NoisyTrainer.latent_information on the GPU: preset ``tiny`` (B = 4, 32x32x3, T = 3, Dz = 9 in levels of 2, 2, 3,
2) on DeviceDataset.synthetic(50, ...), whose 10 test images make two whole windows and the partial one [6, 10), of
which rows 8 and 9 are new.

The report is recomputed from the specification: the windows, the svae_op_make_batch call under the key
seed ^ eval_seed_xor from offset 0, eps and then the chain noise of every window from one
torch.Generator(device).manual_seed(seed), forward at reg_coeff 1.0 on an identically initialised network, the
rows not yet counted of SVAE_BUF_MU (clamped) / _SIGMA / _Z gathered by hand, and tests/latent_ref.py on them.
"""
import json
import math

import numpy as np
import pytest
import torch

import latent_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
PER = H * W * C
GROUPS = (B * PER + 3) // 4
WINDOWS = [(0, 4), (4, 4), (6, 2)]  # (start, rows not yet counted) over the 10 test images
REL = 1e-9


def _net(preset="tiny", seed=0, **over):
    cfg = pkg_mod("config").preset(preset, batch=B, dtype="fp32", **over)
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _dataset(n=50):
    return pkg_mod("data").DeviceDataset.synthetic(n, H, W, C, seed=3, device="cuda")


def _trainer(net, ds=None, **kw):
    kw.setdefault("denoise_train", True)
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


def _gather(seed, preset="tiny", **over):
    """mean (clamped), sigma, z as [T, 10, Dz] numpy, the per-image SVAE_BUF_KL_IMG [T, 10], and the largest
    |z - (mean + sigma eps)| over its fp32 rounding allowance, by the specification."""
    L_ = pkg_mod("_lib")
    net, ds = _net(preset, **over), _dataset()
    tr = pkg_mod("trainer").NoisyTrainer  # its constants
    T, Dz = net.cfg.mc_steps, net.cfg.latent_dim
    clip = float(net.cfg.latent_mean_clip)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rows = {k: [[] for _ in range(T)] for k in ("mean", "sigma", "z", "kl")}
    seen, worst, clipped = [], 0.0, 0
    for k, (start, fresh) in enumerate(WINDOWS):
        tgt = torch.empty(B, H, W, C, device="cuda")
        inp = torch.empty_like(tgt)
        L_.check(L_.lib().svae_op_make_batch(L_.ptr(ds.test), 1, None, start, B, PER, -1.0, 1.0, tr.pepper_prob,
                                             tr.salt_prob, tr.gaussian_noise_scale, seed ^ tr.eval_seed_xor,
                                             k * GROUPS, L_.ptr(tgt), L_.ptr(inp), L_.stream_ptr()))
        eps = torch.randn([T, B, Dz], generator=gen, dtype=torch.float32, device="cuda")
        noise = None
        if net.cfg.add_noise_to_chain:
            noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device="cuda")
        net.forward(inp, tgt, eps, 1.0, noise=noise)
        seen += list(range(start + B - fresh, start + B))
        for t in range(T):
            raw = net.latent(L_.BUF_MU, t).cpu().numpy()
            m = np.clip(raw, -clip, clip)
            s = net.latent(L_.BUF_SIGMA, t).cpu().numpy()
            z = net.latent(L_.BUF_Z, t).cpu().numpy()
            clipped += int(np.sum(np.abs(raw) > clip))
            # z = mean + sigma eps in fp32, fused or not: two roundings of the terms' magnitude at the most
            e = eps[t].cpu().numpy().astype(np.float64)
            diff = np.abs(z.astype(np.float64) - (m.astype(np.float64) + s.astype(np.float64) * e))
            allow = 2.0 ** -22 * (np.abs(m) + np.abs(s * e)) + 1e-30
            worst = max(worst, float((diff / allow).max()))
            rows["mean"][t].append(m[B - fresh:])
            rows["sigma"][t].append(s[B - fresh:])
            rows["z"][t].append(z[B - fresh:])
            rows["kl"][t].append(net.copy_out(L_.BUF_KL_IMG, t, B).cpu().numpy()[B - fresh:])
    assert seen == list(range(10))  # every test image once
    out = {k: np.stack([np.concatenate(v[t]) for t in range(T)]) for k, v in rows.items()}
    return out, net.cfg, worst, clipped


def _close(got, want, what):
    if want is None or got is None:
        assert got is None and want is None, what
        return
    print("%-28s got %.17g want %.17g" % (what, got, want))
    assert abs(got - want) <= REL * abs(want), what


def _check(res, seed, preset="tiny", **over):
    g, cfg, worst, clipped = _gather(seed, preset, **over)
    T, Dz = cfg.mc_steps, cfg.latent_dim
    prior = None if cfg.use_uniform_prior else float(cfg.latent_prior_stddev)
    assert sorted(res) == ["images", "mi_ceiling", "nonfinite", "prior_stddev", "seed", "split", "steps"]
    assert (res["split"], res["images"], res["seed"], res["nonfinite"]) == ("test", 10, seed, 0)
    assert res["mi_ceiling"] == math.log(10) and res["prior_stddev"] == prior and len(res["steps"]) == T
    for t in range(T):
        want = latent_ref.information(g["z"][t], g["mean"][t], g["sigma"][t], cfg.latent_dims, prior)
        got = res["steps"][t]
        assert sorted(got) == ["all", "dims", "levels"] and len(got["levels"]) == len(cfg.latent_dims)
        for name, a, b in [("all", got["all"], want["all"])] + [("level%d" % i, x, y) for i, (x, y) in
                                                                 enumerate(zip(got["levels"], want["levels"]))]:
            assert sorted(a) == ["active_units", "kl", "kl_sample", "marginal_kl", "mi", "tc"]
            for q in ("mi", "marginal_kl", "kl_sample", "kl", "tc"):
                _close(a[q], b[q], "step %d %s %s" % (t, name, q))
            assert a["active_units"] == b["active_units"] and isinstance(a["active_units"], int)
            assert a["mi"] <= res["mi_ceiling"]
        assert sorted(got["dims"]) == ["kl", "marginal_kl", "mi"]
        for q in ("mi", "marginal_kl", "kl"):
            if want["dims"][q] is None:
                assert got["dims"][q] is None
                continue
            assert len(got["dims"][q]) == Dz
            for j in range(Dz):
                _close(got["dims"][q][j], want["dims"][q][j], "step %d dim%d %s" % (t, j, q))
    print("z - (clamp(mu) + sigma eps): worst error / fp32 allowance %.3f; %d means beyond the clip" % (worst, clipped))
    assert worst <= 1.0
    return g, cfg, clipped


@pytest.fixture(scope="module")
def tiny_info():
    """One report of the tiny network's test split (shared, never modified), its trainer and what it was before."""
    tr = _trainer(_net())
    before = (tr.state_dict(), tr.network.iteration, tr.network.adam_updates, tr.network.params.clone())
    return tr, tr.latent_information(), before


def test_every_number_matches_a_recomputation(tiny_info):
    tr, res, _ = tiny_info
    g, cfg, _ = _check(res, SEED)
    assert cfg.latent_prior_stddev == 1.0 and not math.isfinite(cfg.latent_mean_clip)
    # p = 1 and no clip: the analytic KL of the whole code is Dz times the engine's per-image KL (a mean over the
    # dimensions, oracle/tape.py kl_per_row), which evaluate() reports per step; the engine reduces in fp32
    ev = tr.evaluate()
    assert tr.latent_information() == res  # the evaluation in between changes nothing
    for t in range(cfg.mc_steps):
        got, want = res["steps"][t]["all"]["kl"], cfg.latent_dim * ev["steps"][t]["kl"]
        print("step %d kl %.9g, Dz * evaluate()'s %.9g" % (t, got, want))
        assert abs(got - want) <= 1e-5 * abs(want)
        assert abs(cfg.latent_dim * float(g["kl"][t].astype(np.float64).mean()) - want) <= 1e-12 * abs(want)


def test_the_posterior_mean_is_the_clipped_one():
    tr = _trainer(_net(latent_mean_clip=0.5))
    res = tr.latent_information()
    _, _, clipped = _check(res, SEED, latent_mean_clip=0.5)
    assert clipped > 0  # SVAE_BUF_MU holds the pre-clip mean, and some of these are beyond it


def test_the_report_moves_nothing_and_repeats(tiny_info):
    tr, res, (state, it, adam, params) = tiny_info
    assert tr.state_dict() == state and (tr.dataset.train_idx, tr.dataset.test_idx) == (0, 0)
    assert (tr.train_offset, tr.test_offset, tr.iteration) == (0, 0, 0)
    assert (tr.network.iteration, tr.network.adam_updates) == (it, adam)
    assert torch.equal(tr.network.params, params)
    assert tr.latent_information() == res
    assert json.loads(json.dumps(res)) == res
    other = tr.latent_information(seed=SEED + 1)
    assert other["seed"] == SEED + 1 and other["steps"] != res["steps"]
    assert other["steps"][0]["all"]["mi"] != res["steps"][0]["all"]["mi"]
    first = tr.latent_information(num_batches=1)
    assert first["images"] == 4 and first["mi_ceiling"] == math.log(4)
    assert tr.latent_information(split="train", num_batches=2)["images"] == 8
    with pytest.raises(ValueError):
        tr.latent_information(split="validation")
    with pytest.raises(ValueError):
        tr.latent_information(num_batches=0)
    small = _trainer(tr.network, _dataset(15))  # 12 train / 3 test images
    with pytest.raises(ValueError):
        small.latent_information()


def test_uniform_prior_reports_no_prior_terms():
    tr = _trainer(_net(use_uniform_prior=True))
    res = tr.latent_information()
    assert res["prior_stddev"] is None
    for step in res["steps"]:
        for e in [step["all"]] + step["levels"]:
            assert e["marginal_kl"] is None and e["kl_sample"] is None and e["kl"] is None
            assert math.isfinite(e["mi"]) and math.isfinite(e["tc"])
        assert step["dims"]["marginal_kl"] is None and step["dims"]["kl"] is None
        assert all(math.isfinite(v) for v in step["dims"]["mi"])
    _check(res, SEED, use_uniform_prior=True)


def test_training_is_bitwise_the_same_with_reports_between_steps():
    a, b = _trainer(_net()), _trainer(_net())
    a.step(), b.step()
    a.latent_information()
    for k in range(3):
        la, lb = a.step(), b.step()
        assert la == lb, k
        if k < 2:
            a.latent_information(split="train", num_batches=1)
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params)
    assert a.state_dict() == b.state_dict()
    (ma, va), (mb, vb) = a.network._adam_state(), b.network._adam_state()
    torch.cuda.synchronize()
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert (a.network.iteration, a.network.adam_updates) == (b.network.iteration, b.network.adam_updates)


def test_info_frequency_writes_latent_information_jsonl(tmp_path):
    tr = _trainer(_net(), base_dir=str(tmp_path / "on"), info_frequency=2)
    plain = _trainer(_net(), base_dir=str(tmp_path / "off"))
    for _ in range(4):
        tr.step(), plain.step()
    lines = (tmp_path / "on" / "latent_information.jsonl").read_text().splitlines()
    assert len(lines) == 2
    rows = [json.loads(s) for s in lines]
    assert [r["iteration"] for r in rows] == [2, 4] and rows[0]["steps"] != rows[1]["steps"]
    assert rows[1] == dict(iteration=4, **tr.latent_information())
    assert torch.equal(tr.network.params, plain.network.params)  # the option changes no training step
    assert not (tmp_path / "off" / "latent_information.jsonl").exists() and not (tmp_path / "off").exists()
