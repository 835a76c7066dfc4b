"""NoisyTrainer.spectrum on the GPU: preset ``tiny`` at fp32 (B = 4, 32x32x3, T = 3) on DeviceDataset.synthetic(55, ...),
whose 11 test images make two whole windows and a partial one, [7, 11) with 3 rows not yet counted.

The report is recomputed from the specification: evaluate()'s draws (the corruption under seed ^ eval_seed_xor from
offset 0, eps and then the chain noise of every window from one torch.Generator(device).manual_seed(seed)), forward
on an identically initialised network, and tests/spectrum_ref.py on the very same fp32 arrays; the samples from
generate() under sample_quality()'s draws (z, then the chain noise, from a second generator of the same seed).

Bounds.  The op equals the restatement bit for bit (tests/test_power_spectrum_gpu.py), so the report and the
recomputation differ only in the order in which at most 11 * 3 per-image values are added before one division: a
profile agrees to 1e-12 relative (n * 2^-53 = 4e-15 with room).  In decibels that is 10 / ln 10 * 1e-12 for a
power, twice that for a ratio of two profiles (band SNR, the spectral distance's terms) and 2e-12 relative for
hf_ratio.
"""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import spectrum_ref
from conftest import ROOT, pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
PER = H * W * C
GROUPS = (B * PER + 3) // 4
WINDOWS = [(0, 4), (4, 4), (7, 3)]  # (start, rows not yet counted) of the 11 test images
REL = 1e-12
DB = 10.0 / math.log(10.0) * REL


def _net(preset="tiny", seed=0):
    cfg = pkg_mod("config").preset(preset, batch=B, dtype="fp32")
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _dataset(n=55):
    return pkg_mod("data").DeviceDataset.synthetic(n, H, W, C, seed=3, device="cuda")


def _trainer(net, ds=None, **kw):
    kw.setdefault("denoise_train", True)
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


def _binned(x, y, kind):
    """[n, c, 2, n_bins] of the restatement under spectra.py's tables."""
    S = pkg_mod("spectra")
    table, n_bins, _ = S.radial_bins(H, W)
    return spectrum_ref.power_spectrum_ref(x, y, S.window(H, kind), S.window(W, kind), S.twiddles(H), S.twiddles(W),
                                           table, n_bins)[0]


def _recompute(preset, seed, kind="hann", windows=WINDOWS):
    """The per-bin means by the specification: (slots [T + 1, 2, n_bins], target [n_bins], samples [T, n_bins])."""
    L_ = pkg_mod("_lib")
    net, ds = _net(preset), _dataset()
    tr = pkg_mod("trainer").NoisyTrainer  # its constants
    T, Dz = net.cfg.mc_steps, net.cfg.latent_dim
    gen = torch.Generator(device="cuda").manual_seed(seed)
    slots, target, images = 0.0, 0.0, 0
    for k, (start, fresh) in enumerate(windows):
        tgt = torch.empty(B, H, W, C, device="cuda")
        inp = torch.empty_like(tgt)
        L_.check(L_.lib().svae_op_make_batch(L_.ptr(ds.test), 1, None, start, B, PER, -1.0, 1.0, tr.pepper_prob,
                                             tr.salt_prob, tr.gaussian_noise_scale, seed ^ tr.eval_seed_xor, k * GROUPS,
                                             L_.ptr(tgt), L_.ptr(inp), L_.stream_ptr()))
        eps = torch.randn([T, B, Dz], generator=gen, dtype=torch.float32, device="cuda")
        noise = None
        if net.cfg.add_noise_to_chain:
            noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device="cuda")
        net.forward(inp, tgt, eps, 1.0, noise=noise)
        stack = np.stack([inp.cpu().numpy()] + [net.xhat(t).cpu().numpy() for t in range(T)])
        clean = tgt.cpu().numpy()
        rows = _binned(stack.reshape(-1, H, W, C), clean, kind).reshape(T + 1, B, C, 2, -1)[:, B - fresh:]
        slots = slots + rows.sum((1, 2))
        target = target + _binned(clean, None, kind)[B - fresh:, :, 0].sum((0, 1))
        images += fresh
    gen = torch.Generator(device="cuda").manual_seed(seed)
    samples, nwin = 0.0, sum(1 for _, f in windows if f == B)
    for _ in range(nwin):
        z = torch.randn([T, B, Dz], generator=gen, dtype=torch.float32, device="cuda")
        noise = None
        if net.cfg.add_noise_to_chain:
            noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device="cuda")
        xs = np.stack([x.cpu().numpy() for x in net.generate(z, noise=noise)])
        samples = samples + _binned(xs.reshape(-1, H, W, C), None, kind).reshape(T, B, C, 2, -1)[:, :, :, 0].sum((1, 2))
    return slots / images, target / images, samples / (nwin * B), net.cfg, images


def _close_db(got, want, tol, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        if math.isinf(w) or math.isinf(g):
            assert g == w, (what, b)
        else:
            assert abs(g - w) <= tol, (what, b, g, w)


def _check_entry(S, got, power, target, counts, err, what):
    want = S.profile_report(list(power), list(target), counts, err=None if err is None else list(err))
    assert sorted(got) == sorted(want), what
    _close_db(got["power_db"], want["power_db"], DB, what + " power_db")
    for b in range(len(counts)):  # the profile itself, back from decibels: 1e-12 relative
        mean = 10.0 ** (got["power_db"][b] / 10.0) * counts[b]
        assert abs(mean - power[b]) <= (REL + 1e-14) * power[b], (what, b)
    assert abs(got["log_spectral_distance"] - want["log_spectral_distance"]) <= 2 * DB, what
    assert abs(got["hf_ratio"] - want["hf_ratio"]) <= 2 * REL * want["hf_ratio"], what
    if err is not None:
        _close_db(got["band_snr_db"], want["band_snr_db"], 2 * DB, what + " band_snr_db")
        if min(abs(v) for v in want["band_snr_db"][1:]) > 2 * DB:  # no annulus sits on the 0 dB line
            assert got["cutoff"] == want["cutoff"], what
    print("%-10s hf_ratio %.6g, spectral distance %.4g dB, cutoff %s" % (what, got["hf_ratio"],
                                                                          got["log_spectral_distance"], got.get("cutoff")))


def _check(res, seed, preset="tiny", kind="hann", windows=WINDOWS):
    S = pkg_mod("spectra")
    slots, target, samples, cfg, images = _recompute(preset, seed, kind, windows)
    T = cfg.mc_steps
    _, n_bins, counts = S.radial_bins(H, W)
    assert sorted(res) == ["bins", "counts", "images", "input", "nonfinite", "sample_images", "samples", "seed", "split",
                           "steps", "target", "window"]
    nwin = sum(1 for _, f in windows if f == B)
    assert (res["split"], res["images"], res["seed"], res["window"], res["nonfinite"], res["sample_images"]) == \
        ("test", images, seed, kind, 0, nwin * B)
    assert res["bins"] == [b / 32 for b in range(n_bins)] and res["counts"] == list(counts) and n_bins == 17
    assert len(res["steps"]) == T and len(res["samples"]) == T and sorted(res["target"]) == ["power_db"]
    _close_db(res["target"]["power_db"], S.profile_report(list(target), list(target), counts)["power_db"], DB, "target")
    _check_entry(S, res["input"], slots[0, 0], target, counts, slots[0, 1], "input")
    for t in range(T):
        _check_entry(S, res["steps"][t], slots[1 + t, 0], target, counts, slots[1 + t, 1], "step %d" % t)
        _check_entry(S, res["samples"][t], samples[t], target, counts, None, "samples %d" % t)
    return cfg


@pytest.fixture(scope="module")
def tiny_spectrum():
    """One report of the tiny network's test split (shared, never modified), its trainer and what it was before."""
    tr = _trainer(_net())
    before = (tr.state_dict(), tr.network.iteration, tr.network.adam_updates, tr.network.params.clone())
    return tr, tr.spectrum(), before


def test_every_number_matches_a_recomputation(tiny_spectrum):
    """Also the partial last window: its first row was scored in the window before and is counted once."""
    _, res, _ = tiny_spectrum
    assert res["images"] == 11 and res["sample_images"] == 8
    cfg = _check(res, SEED)
    assert not cfg.add_noise_to_chain
    # the noisy input is far from the clean image at high frequencies; the target against itself would be 1 and 0
    assert res["input"]["hf_ratio"] > 1.0 and res["input"]["cutoff"] < 1.0


def test_chain_noise_window_kind_and_a_limited_walk():
    tr = _trainer(_net("tiny_flat"))
    res = tr.spectrum(seed=5, window="none", num_batches=2)
    cfg = _check(res, 5, "tiny_flat", "none", WINDOWS[:2])
    assert cfg.add_noise_to_chain and res["images"] == 8
    assert tr.spectrum(seed=5, window="none", num_batches=2, samples=False)["samples"] == []


def test_the_report_moves_nothing_and_repeats(tiny_spectrum):
    tr, res, (state, it, adam, params) = tiny_spectrum
    assert tr.state_dict() == state and (tr.dataset.train_idx, tr.dataset.test_idx) == (0, 0)
    assert (tr.train_offset, tr.test_offset, tr.iteration) == (0, 0, 0)
    assert (tr.network.iteration, tr.network.adam_updates) == (it, adam)
    assert torch.equal(tr.network.params, params)
    assert json.dumps(tr.spectrum()) == json.dumps(res)
    assert json.loads(json.dumps(res)) == res
    other = tr.spectrum(seed=SEED + 1)
    assert other["seed"] == SEED + 1 and other["steps"] != res["steps"] and other["samples"] != res["samples"]
    assert other["target"] == res["target"]  # the clean images have no draws
    quiet = tr.spectrum(samples=False)
    assert quiet["samples"] == [] and quiet["sample_images"] == 0 and quiet["steps"] == res["steps"]
    assert tr.spectrum(split="train", num_batches=2)["images"] == 8
    with pytest.raises(ValueError):
        tr.spectrum(split="validation")
    with pytest.raises(ValueError):
        tr.spectrum(num_batches=0)
    with pytest.raises(ValueError):
        tr.spectrum(window="hamming")
    small = _trainer(tr.network, _dataset(15))  # 12 train / 3 test images
    with pytest.raises(ValueError):
        small.spectrum()
    head = pkg_mod("config").preset("tiny", batch=B, dtype="fp32")
    head.external_generator_from = 1
    net = tr.network
    real, net.cfg = net.cfg, head
    try:
        with pytest.raises(ValueError, match="PixelVAE"):
            tr.spectrum()
    finally:
        net.cfg = real


def test_training_is_bitwise_the_same_with_reports_between_steps():
    """Every draw of the report is injected: a trainer that reports before and between its steps (whose eps the
    network draws on the device) ends with the losses, parameters and Adam state of a twin that never does."""
    a, b = _trainer(_net()), _trainer(_net())
    a.spectrum()
    a.step(), b.step()
    for k in range(3):
        la, lb = a.step(), b.step()
        assert la == lb, k
        if k < 2:
            a.spectrum(split="train", num_batches=2)
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params)
    assert a.state_dict() == b.state_dict()
    (ma, va), (mb, vb) = a.network._adam_state(), b.network._adam_state()
    torch.cuda.synchronize()
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert (a.network.iteration, a.network.adam_updates) == (b.network.iteration, b.network.adam_updates)
    assert (a.dataset.train_idx, a.dataset.test_idx) == (b.dataset.train_idx, b.dataset.test_idx)
    assert (a.train_offset, a.test_offset) == (b.train_offset, b.test_offset)


def test_spectrum_frequency_writes_spectrum_jsonl(tmp_path):
    tr = _trainer(_net(), base_dir=str(tmp_path / "on"), spectrum_frequency=2)
    plain = _trainer(_net(), base_dir=str(tmp_path / "off"))
    for _ in range(4):
        tr.step(), plain.step()
    lines = (tmp_path / "on" / "spectrum.jsonl").read_text().splitlines()
    assert len(lines) == 2
    rows = [json.loads(s) for s in lines]
    assert [r["iteration"] for r in rows] == [2, 4] and rows[0]["steps"] != rows[1]["steps"]
    assert rows[1] == dict(iteration=4, **tr.spectrum())
    assert torch.equal(tr.network.params, plain.network.params)  # the option changes no training step
    assert not (tmp_path / "off").exists()


def test_the_tool_reports_on_a_checkpoint(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("svae_tool_evaluate_spectrum", os.path.join(ROOT, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    net = _net(seed=5)  # not the seed the tool builds its network with: the checkpoint must be what it scores
    base = tmp_path / "models" / "tiny_v3"
    os.makedirs(base)
    net.save_checkpoint(str(base / "model.safetensors"))
    args = ["--netname", "tiny", "--version", "3", "--batch_size", str(B), "--dtype", "fp32", "--synthetic", "55",
            "--denoise_train", "--models_dir", str(tmp_path / "models"), "--seed", str(SEED)]
    assert tool.main(args + ["--spectrum"]) == 0
    row = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert json.loads((base / "spectrum.json").read_text()) == row
    ds = pkg_mod("data").DeviceDataset.synthetic(55, H, W, C, seed=0, device="cuda")  # the run's seed: no trainer.json
    want = pkg_mod("trainer").NoisyTrainer(net, ds, denoise_train=True, seed=0).spectrum(seed=SEED)
    assert row == dict(iteration=row["iteration"], **want) and row["images"] == 11
    assert tool.main(args + ["--spectrum", "--sample_quality"]) == 1
    assert tool.parse(["--synthetic", "8"]).spectrum is False
    spec = importlib.util.spec_from_file_location("svae_tool_train_spectrum", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    assert train.parse(["--synthetic", "8", "--spectrum_frequency", "3"]).spectrum_frequency == 3
    assert train.parse(["--synthetic", "8"]).spectrum_frequency == 0


def test_a_blurred_input_reads_as_blurred():
    """A batch blurred by Degradation(blur=(1, 2, 2)) against the same batch unblurred.  Both inputs carry a light
    Gaussian pixel noise (scale 0.02, no salt, no pepper): an error that is only an attenuation by a gain g in
    [0, 1] has the band SNR -20 log10(1 - g) >= 0 at every frequency, so a cutoff needs an error that does not
    shrink with the signal.  The synthetic images hold white noise of variance 0.2^2 / 12 above their gradients,
    eight times the pixel noise's 0.02^2: unblurred, every annulus stays above 0 dB; blurred (sigma = 2 pixels: a gain
    below 0.06 from annulus 6 of 17 on), that content is gone from the input and present in the error.  In the
    high band the input's power over the target's is then the two variances' ratio, 0.02^2 / (0.2^2 / 12) = 0.12,
    blurred, and 1.12 unblurred; the assertions leave a factor of two around the 0.12."""
    reports = []
    for deg in (pkg_mod("degrade").Degradation(blur=(1.0, 2.0, 2.0)), None):
        tr = _trainer(_net(), degradation=deg)
        tr.pepper_prob, tr.salt_prob, tr.gaussian_noise_scale = 0.0, 0.0, 0.02
        reports.append(tr.spectrum(num_batches=2, samples=False))
    blurred, plain = (r["input"] for r in reports)
    print("blurred: hf_ratio %.4g cutoff %.4g; unblurred: hf_ratio %.4g cutoff %.4g" % (
        blurred["hf_ratio"], blurred["cutoff"], plain["hf_ratio"], plain["cutoff"]))
    assert reports[0]["target"] == reports[1]["target"]
    assert blurred["hf_ratio"] < 1.0 and blurred["cutoff"] < plain["cutoff"]
    assert 0.06 < blurred["hf_ratio"] < 0.24 and 1.06 < plain["hf_ratio"] < 1.24 and plain["cutoff"] == 1.0
    assert blurred["log_spectral_distance"] > plain["log_spectral_distance"]
