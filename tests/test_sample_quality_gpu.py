"""NoisyTrainer.sample_quality on the GPU: preset ``tiny`` at fp32 (B = 4, 32x32x3, T = 3, Dz = 9) on
DeviceDataset.synthetic(50, ...), whose 10 test images make two whole windows, N = 8 (the partial window is dropped).

The report is recomputed from the specification: the clean windows by svae_op_make_batch without noise, z [T,B,Dz]
and then (tiny_flat) the chain noise [T,B,H,W,C] of every window from one torch.Generator(device).manual_seed(seed),
generate() on an identically initialised network, everything centred on R's mean row by the same fp32 expression, and
tests/quality_ref.py (numpy float64, direct form) on the very same fp32 arrays.

Bounds: the op's bound propagated.  With tau = max over all pairs of 2 (D + 2) u sum_k |x_k y_k| + 4 2^-53 (a + b)
(u = 2^-24; tests/test_pairwise_stats_gpu.py derives it) every computed d2 is within tau of the reference, so
  * a kernel value moves by at most a factor exp(+-tau / (2 sigma_l^2)); mmd2 is three means of values <= 1 with
    weights 1, 1, 2:   |mmd2_l - ref| <= 4 (exp(tau / (2 sigma_l^2)) - 1) + 1e-12;
  * a point's nearest-neighbour vote can flip only if its two nearest distances are within 2 tau of each other:
    |accuracy - ref| n <= the number of such points (none, usually: then the accuracies are equal);
  * a per-element RMS sqrt(d2 / D) moves by at most sqrt((dmin + tau) / D) - sqrt(dmin / D), dmin the smallest
    reference d2 of the set, and so do the mean, the median and the minimum of such values;
  * sigma0 is fp64 arithmetic on the same inputs on both sides: 1e-12 relative.
"""
import json
import math

import numpy as np
import pytest
import torch

import quality_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
D = H * W * C
NWIN = 2
N = NWIN * B
U = 2.0 ** -24


def _net(preset="tiny", seed=0, **over):
    cfg = pkg_mod("config").preset(preset, batch=B, dtype="fp32", **over)
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _dataset(n=50):
    return pkg_mod("data").DeviceDataset.synthetic(n, H, W, C, seed=3, device="cuda")


def _trainer(net, ds=None, **kw):
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


def _clean(data, start):
    L_ = pkg_mod("_lib")
    tgt = torch.empty(B, H, W, C, device="cuda")
    L_.check(L_.lib().svae_op_make_batch(L_.ptr(data), 1, None, start, B, D, -1.0, 1.0, 0.0, 0.0, 0.0, 0, 0, L_.ptr(tgt),
                                         None, L_.stream_ptr()))
    return tgt.view(B, D).clone()


def _gather(seed, preset, train_images=N):
    """The centred sets [T][N, D], R [N, D] and the training images [train_images, D] as fp32 numpy, by the
    specification."""
    net, ds = _net(preset), _dataset()
    T, Dz = net.cfg.mc_steps, net.cfg.latent_dim
    gen = torch.Generator(device="cuda").manual_seed(seed)
    real, xs = [], [[] for _ in range(T)]
    for w in range(NWIN):
        real.append(_clean(ds.test, w * B))
        z = torch.randn([T, B, Dz], generator=gen, dtype=torch.float32, device="cuda")
        noise = None
        if net.cfg.add_noise_to_chain:
            noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device="cuda")
        for t, xh in enumerate(net.generate(z, noise=noise)):
            xs[t].append(xh.reshape(B, D).clone())
    R = torch.cat(real)
    train = torch.cat([_clean(ds.train, s) for s in range(0, train_images, B)])[:train_images]
    mu = R.double().mean(0).float()
    cen = lambda a: (a - mu).cpu().numpy()
    return [cen(torch.cat(x)) for x in xs], cen(R), cen(train), net.cfg


def _tau(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((2.0 * (D + 2) * U * (np.abs(a) @ np.abs(b).T)
                  + 4.0 * 2.0 ** -53 * (np.square(a).sum(1)[:, None] + np.square(b).sum(1)[None, :])).max())


def _rms_close(got, d2, tau, what):
    """got {"mean", "median", "min"} against the reference nearest d2 per point."""
    rms = np.sqrt(d2 / D)
    slack = math.sqrt((d2.min() + tau) / D) - math.sqrt(d2.min() / D) + 1e-15
    for key, want in (("mean", rms.mean()), ("median", np.median(rms)), ("min", rms.min())):
        print("%-24s %-6s got %.12g want %.12g (error / bound %.3e)" % (what, key, got[key], want,
                                                                        abs(got[key] - want) / slack))
        assert abs(got[key] - want) <= slack, (what, key)
    assert sorted(got) == ["mean", "median", "min"]


def _votes_close(got, own, other, tau, n, what):
    """an accuracy against the reference's nearest own / other d2 per point"""
    want = float((own < other).sum())
    unsure = int((np.abs(own - other) <= 2.0 * tau).sum())
    print("%-24s got %.6g want %.6g, %d of %d points within 2 tau" % (what, got, want / n, unsure, n))
    assert abs(got * n - want) <= unsure + 1e-9, what
    return want, unsure


def _check(res, seed, preset="tiny"):
    xs, R, train, cfg = _gather(seed, preset, res["train_images"])
    T = cfg.mc_steps
    assert sorted(res) == ["bandwidth_scales", "images", "nonfinite", "real", "seed", "sigma0", "split", "steps",
                           "train_images"]
    assert (res["split"], res["images"], res["seed"], res["nonfinite"], res["train_images"]) == ("test", N, seed, 0, N)
    assert res["bandwidth_scales"] == [0.25, 0.5, 1.0, 2.0, 4.0] and len(res["steps"]) == T
    bw = quality_ref.bandwidths(R)
    assert abs(res["sigma0"] - math.sqrt(bw[2])) <= 1e-12 * math.sqrt(bw[2])
    tau = max(_tau(a, b) for a in xs + [R] for b in xs + [R, train])
    print("tau %.4g, sigma0^2 %.6g" % (tau, bw[2]))
    dr = quality_ref.pairwise_stats(R, [train], [])[1][:, 0]
    _rms_close(res["real"]["nn_train"], dr, tau, "real nn_train")
    assert sorted(res["real"]) == ["nn_train"]
    for t in range(T):
        got = res["steps"][t]
        assert sorted(got) == ["mmd2", "mmd2_at_sigma0", "nn_accuracy", "nn_real", "nn_train"]
        want = quality_ref.two_sample(xs[t], R)
        for l in range(5):
            bound = 4.0 * math.expm1(tau / (2.0 * bw[l])) + 1e-12
            err = abs(got["mmd2"][l] - want["mmd2"][l])
            print("step %d mmd2[%d] got %.12g want %.12g (error / bound %.3e)" % (t, l, got["mmd2"][l],
                                                                                 want["mmd2"][l], err / bound))
            assert err <= bound
        assert got["mmd2_at_sigma0"] == got["mmd2"][2]
        _, dx, _, _ = quality_ref.pairwise_stats(xs[t], [xs[t], R], [], self_group=0)
        _, dy, _, _ = quality_ref.pairwise_stats(R, [R, xs[t]], [], self_group=0)
        assert sorted(got["nn_accuracy"]) == ["all", "real", "samples"]
        ws, us = _votes_close(got["nn_accuracy"]["samples"], dx[:, 0], dx[:, 1], tau, N, "step %d samples" % t)
        wr, ur = _votes_close(got["nn_accuracy"]["real"], dy[:, 0], dy[:, 1], tau, N, "step %d real" % t)
        assert abs(got["nn_accuracy"]["all"] * 2 * N - (ws + wr)) <= us + ur + 1e-9
        _rms_close(got["nn_real"], dx[:, 1], tau, "step %d nn_real" % t)
        dt = quality_ref.pairwise_stats(xs[t], [train], [])[1][:, 0]
        _rms_close(got["nn_train"], dt, tau, "step %d nn_train" % t)
    return cfg


@pytest.fixture(scope="module")
def tiny_quality():
    """One report of the tiny network (shared, never modified), its trainer and what it was before."""
    tr = _trainer(_net())
    before = (tr.state_dict(), tr.network.iteration, tr.network.adam_updates, tr.network.params.clone())
    return tr, tr.sample_quality(), before


def test_every_number_matches_a_recomputation(tiny_quality):
    _, res, _ = tiny_quality
    cfg = _check(res, SEED)
    assert not cfg.add_noise_to_chain


def test_chain_noise_is_drawn_after_z():
    tr = _trainer(_net("tiny_flat"))
    res = tr.sample_quality(seed=5)
    cfg = _check(res, 5, "tiny_flat")
    assert cfg.add_noise_to_chain


def test_the_report_moves_nothing_and_repeats(tiny_quality):
    tr, res, (state, it, adam, params) = tiny_quality
    assert tr.state_dict() == state and (tr.dataset.train_idx, tr.dataset.test_idx) == (0, 0)
    assert (tr.train_offset, tr.test_offset, tr.iteration) == (0, 0, 0)
    assert (tr.network.iteration, tr.network.adam_updates) == (it, adam)
    assert torch.equal(tr.network.params, params)
    assert json.dumps(tr.sample_quality()) == json.dumps(res)
    assert json.loads(json.dumps(res)) == res
    other = tr.sample_quality(seed=SEED + 1)
    assert other["seed"] == SEED + 1 and other["steps"] != res["steps"]
    assert other["real"] == res["real"] and other["sigma0"] == res["sigma0"]  # the real side has no draws
    assert tr.sample_quality(split="train", num_batches=3, train_images=5)["images"] == 12
    assert tr.sample_quality(train_images=5)["train_images"] == 5
    with pytest.raises(ValueError):
        tr.sample_quality(split="validation")
    with pytest.raises(ValueError):
        tr.sample_quality(train_images=0)


def test_fewer_than_two_windows_raise(tiny_quality):
    tr = tiny_quality[0]
    with pytest.raises(ValueError, match="two whole windows"):
        tr.sample_quality(num_batches=1)
    small = _trainer(tr.network, _dataset(35))  # 28 train / 7 test images: one whole window
    with pytest.raises(ValueError, match="two whole windows"):
        small.sample_quality()


def test_training_is_bitwise_the_same_with_reports_between_steps():
    """Also the device Philox counter: step() draws its eps from it, so a moved counter would change the loss."""
    a, b = _trainer(_net(), denoise_train=True), _trainer(_net(), denoise_train=True)
    a.step(), b.step()
    a.sample_quality()
    for k in range(3):
        la, lb = a.step(), b.step()
        assert la == lb, k
        if k < 2:
            a.sample_quality(split="train", num_batches=2)
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params)
    assert a.state_dict() == b.state_dict()
    (ma, va), (mb, vb) = a.network._adam_state(), b.network._adam_state()
    torch.cuda.synchronize()
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert (a.network.iteration, a.network.adam_updates) == (b.network.iteration, b.network.adam_updates)
    assert (a.dataset.train_idx, a.dataset.test_idx) == (b.dataset.train_idx, b.dataset.test_idx)
    assert (a.train_offset, a.test_offset) == (b.train_offset, b.test_offset)


def test_quality_frequency_writes_sample_quality_jsonl(tmp_path):
    tr = _trainer(_net(), base_dir=str(tmp_path / "on"), quality_frequency=2)
    plain = _trainer(_net(), base_dir=str(tmp_path / "off"))
    for _ in range(4):
        tr.step(), plain.step()
    lines = (tmp_path / "on" / "sample_quality.jsonl").read_text().splitlines()
    assert len(lines) == 2
    rows = [json.loads(s) for s in lines]
    assert [r["iteration"] for r in rows] == [2, 4] and rows[0]["steps"] != rows[1]["steps"]
    assert rows[1] == dict(iteration=4, **tr.sample_quality())
    assert torch.equal(tr.network.params, plain.network.params)  # the option changes no training step
    assert not (tmp_path / "off" / "sample_quality.jsonl").exists() and not (tmp_path / "off").exists()


def test_a_shifted_copy_is_told_apart():
    """quality.two_sample on the synthetic images: x against x + 0.5 is separable (every point's nearest neighbour
    is of its own set) and further apart in MMD than two disjoint halves of the same images; the numbers agree
    with the reference within the propagated bound."""
    Qm = pkg_mod("quality")
    ds = _dataset()
    imgs = torch.cat([_clean(ds.train, s) for s in range(0, 40, B)])  # 40 clean train images
    x, other = imgs[:20].contiguous(), imgs[20:].contiguous()
    y = x + 0.5
    far, same = Qm.two_sample(x, y), Qm.two_sample(x, other)
    print("shifted: mmd2 %.6g accuracy %s; halves: mmd2 %.6g accuracy %s" % (
        far["mmd2_at_sigma0"], far["nn_accuracy"], same["mmd2_at_sigma0"], same["nn_accuracy"]))
    assert far["nn_accuracy"]["all"] == 1.0 and far["nn_accuracy"]["x"] == 1.0 and far["nn_accuracy"]["y"] == 1.0
    assert far["mmd2_at_sigma0"] > same["mmd2_at_sigma0"]
    assert far["nonfinite"] == 0 and same["nonfinite"] == 0
    mu = y.double().mean(0).float()
    xc, yc = (x - mu).cpu().numpy(), (y - mu).cpu().numpy()
    want = quality_ref.two_sample(xc, yc)
    tau = max(_tau(a, b) for a in (xc, yc) for b in (xc, yc))
    for l, s2 in enumerate(quality_ref.bandwidths(yc)):
        assert abs(far["mmd2"][l] - want["mmd2"][l]) <= 4.0 * math.expm1(tau / (2.0 * s2)) + 1e-12
    assert abs(far["sigma0"] - want["sigma0"]) <= 1e-12 * want["sigma0"]
    # the cached y-against-y pass gives the same report
    bw = Qm.bandwidths(torch.from_numpy(yc).cuda()).tolist()
    yy = Qm.self_sums(torch.from_numpy(yc).cuda(), bw)
    assert Qm.two_sample(x, y, yy=yy, bw=bw) == far
