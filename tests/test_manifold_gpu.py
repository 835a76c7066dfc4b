"""quality.manifold (k-NN precision / recall / density / coverage on svae_op_pairwise_knn) and
NoisyTrainer.sample_quality(manifold_k=...) on the GPU against tests/manifold_ref.py (numpy float64, direct form).

Bounds: the op's bound propagated.  Every computed d2 is within tau_ij = 2 (d + 2) u sum_k |a_ik b_jk| + 4 2^-53
(|a_i|^2 + |b_j|^2) of the reference (u = 2^-24; tests/test_pairwise_stats_gpu.py derives it), and a computed k-th
radius of point j, an order statistic of such values, within T_j = max_l tau_jl over its own set.  Each of the four
metrics is a mean of indicators that compare a distance with a radius:
    d2(p, s) <= r_k(s)^2  is decided by the reference where  |ref d2 - ref r^2| > tau_ps + T_s,
    min_i d2(y_j, x_i) <= r_k(y_j)^2  (coverage: a minimum is an order statistic too) where the margin exceeds
    max_i tau_ji + T_j.
An indicator is compared only where the reference decides it; the counts and the four means are then bracketed by
the decided pairs (undecided ones counted out below and in above), and the share of undecided (pair, k) entries is
capped from the reference alone as in tests/test_pairwise_knn_gpu.py: 0.1 % for d <= 48, 1 % for d = 3072.

The trainer part sets up preset ``tiny`` at fp32 (B = 4, 32x32x3, T = 3) on DeviceDataset.synthetic(50, ...), N = 8,
as tests/test_sample_quality_gpu.py does, and recomputes every manifold number from samples gathered by the
specification (the brackets above, no cap at that size).
"""
import json

import numpy as np
import pytest
import torch

import manifold_ref
import quality_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED = 77
B, H, W, C = 4, 32, 32, 3
D = H * W * C
NWIN = 2
N = NWIN * B
KEYS = ("precision", "recall", "density", "coverage")


def _tau(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return 2.0 * (a.shape[1] + 2) * U * (np.abs(a) @ np.abs(b).T) \
        + 4.0 * 2.0 ** -53 * (np.square(a).sum(1)[:, None] + np.square(b).sum(1)[None, :])


def _brackets(x, y, ks):
    """From the reference alone, for centred fp32 sets: per metric and k the (low, high) bracket of the mean, the
    per-point count brackets of inside(x; y) and inside(y; x), and the numbers of undecided and of all entries."""
    n, m = len(x), len(y)
    dxy = quality_ref.sqdist(x, y)
    txy = _tau(x, y)
    rx, ry = manifold_ref.self_radii(x, ks), manifold_ref.self_radii(y, ks)
    Tx = np.where(np.eye(n, dtype=bool), 0.0, _tau(x, x)).max(1)
    Ty = np.where(np.eye(m, dtype=bool), 0.0, _tau(y, y)).max(1)
    out = {key: [] for key in KEYS}
    out["inside_xy"], out["inside_yx"] = [], []
    und = 0
    for c, k in enumerate(ks):
        # x_i in the ball of y_j
        mar = txy + Ty[None, :]
        lo, hi = dxy <= ry[None, :, c] - mar, dxy <= ry[None, :, c] + mar
        und += int((hi & ~lo).sum())
        out["inside_xy"].append((lo.sum(1), hi.sum(1)))
        out["precision"].append((lo.any(1).mean(), hi.any(1).mean()))
        out["density"].append((lo.sum() / (k * n), hi.sum() / (k * n)))
        # y_j in the ball of x_i
        mar = txy.T + Tx[None, :]
        lo, hi = dxy.T <= rx[None, :, c] - mar, dxy.T <= rx[None, :, c] + mar
        und += int((hi & ~lo).sum())
        out["inside_yx"].append((lo.sum(1), hi.sum(1)))
        out["recall"].append((lo.any(1).mean(), hi.any(1).mean()))
        # the ball of y_j holds an x
        mar = txy.max(0) + Ty
        lo, hi = dxy.min(0) <= ry[:, c] - mar, dxy.min(0) <= ry[:, c] + mar
        und += int((hi & ~lo).sum())
        out["coverage"].append((lo.mean(), hi.mean()))
    out["undecided"], out["entries"] = und, len(ks) * (2 * n * m + m)
    return out


def _within(rep, br, ks, what):
    assert rep["k"] == list(ks) and rep["nonfinite"] == 0
    assert sorted(rep) == ["coverage", "density", "k", "nonfinite", "precision", "recall"]
    for key in KEYS:
        for c, k in enumerate(ks):
            lo, hi = br[key][c]
            print("%-22s %-9s k = %d: %.6g in [%.6g, %.6g]" % (what, key, k, rep[key][c], lo, hi))
            assert lo - 1e-12 <= rep[key][c] <= hi + 1e-12, (what, key, k)


@pytest.mark.parametrize("n,m,d,cap", [(60, 70, 48, 0.001), (40, 40, 3072, 0.01)])
def test_manifold_matches_the_reference(n, m, d, cap):
    Qm = pkg_mod("quality")
    ks = (1, 3, 5)
    rng = np.random.default_rng(100 * n + d)
    x = rng.normal(0, 1, (n, d)).astype(np.float32)
    y = rng.normal(0, 1, (m, d)).astype(np.float32)
    y[:m // 2] += np.float32(0.5) * rng.normal(0, 1, (m // 2, d)).astype(np.float32)  # half of y is wider than x
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    rep = Qm.manifold(xd, yd, ks=ks)
    xc, yc = (t.cpu().numpy() for t in Qm.center(xd, yd))
    br = _brackets(xc, yc, ks)
    share = br["undecided"] / br["entries"]
    print("n %d m %d d %d: undecided share %.4f %% (cap %.2f %%)" % (n, m, d, 100 * share, 100 * cap))
    assert share <= cap
    _within(rep, br, ks, "%dx%dx%d" % (n, m, d))
    # every indicator where the reference decides it: the three calls manifold makes, point by point
    xt, yt = torch.from_numpy(xc).cuda(), torch.from_numpy(yc).cuda()
    ry, bad = Qm.self_radii(yt, ks)
    kx, ix, _ = Qm.knn_stats(xt, [xt, yt], max(ks), radii=[None, ry], self_group=0)
    rx = kx[:, 0, [k - 1 for k in ks]].contiguous()
    ky, iy, _ = Qm.knn_stats(yt, [xt], 1, radii=[rx])
    assert int(bad) == 0
    for c in range(len(ks)):
        lo, hi = br["inside_xy"][c]
        got = ix[:, 1, c].cpu().numpy()
        assert np.all((lo <= got) & (got <= hi))
        lo, hi = br["inside_yx"][c]
        got = iy[:, 0, c].cpu().numpy()
        assert np.all((lo <= got) & (got <= hi))
    # and the report is those counts' means
    assert rep["precision"] == (ix[:, 1] > 0).double().mean(0).tolist()
    assert rep["recall"] == (iy[:, 0] > 0).double().mean(0).tolist()
    # the cached y-against-y pass gives the same report
    assert Qm.manifold(xd, yd, ks=ks, yy=(ry, bad)) == rep
    want = manifold_ref.manifold(xc, yc, ks)
    print("reference: %s" % want)
    with pytest.raises(ValueError):
        Qm.manifold(xd[:5], yd, ks=(5,))  # five points have no fifth other neighbour
    with pytest.raises(ValueError):
        Qm.manifold(xd, yd, ks=(0, 3))
    with pytest.raises(ValueError):
        Qm.manifold(xd, yd, ks=(pkg_mod("_lib").KNN_MAX_K + 1,))


# ------------------------------------------------------------------ the synthetic images and the tiny trainer
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


def _gather(seed, net, train_images=N):
    """The centred sets [T][N, D], R [N, D] and the training images [train_images, D] as fp32 numpy, by the
    specification of sample_quality (z [T,B,Dz] per window from one generator, generate(), centred on R's mean)."""
    ds = _dataset()
    T, Dz = net.cfg.mc_steps, net.cfg.latent_dim
    gen = torch.Generator(device="cuda").manual_seed(seed)
    real, xs = [], [[] for _ in range(T)]
    for w in range(NWIN):
        real.append(_clean(ds.test, w * B))
        z = torch.randn([T, B, Dz], generator=gen, dtype=torch.float32, device="cuda")
        for t, xh in enumerate(net.generate(z, noise=None)):
            xs[t].append(xh.reshape(B, D).clone())
    Rr = torch.cat(real)
    train = torch.cat([_clean(ds.train, s) for s in range(0, train_images, B)])[:train_images]
    mu = Rr.double().mean(0).float()
    cen = lambda a: (a - mu).cpu().numpy()
    return [cen(torch.cat(x)) for x in xs], cen(Rr), cen(train)


def test_a_shifted_copy_scores_zero_and_a_permutation_one():
    Qm = pkg_mod("quality")
    ds = _dataset()
    x = torch.cat([_clean(ds.train, s) for s in range(0, 20, B)])  # 20 clean train images
    # a shift of 0.5 per element puts every image 768 = 0.25 D from its own copy: the sets are separable as far as
    # the k-th neighbour radii stay below that.  Among 20 images the 1st and 3rd do (the reference says 0 there,
    # and so must the op); the 5th of the sparsest images does not, and there the op must agree with the reference.
    ks = (1, 3, 5)
    y = x + 0.5
    far = Qm.manifold(x, y, ks=ks)
    print("shifted: %s" % far)
    xc, yc = (t.cpu().numpy() for t in Qm.center(x, y))
    _within(far, _brackets(xc, yc, ks), ks, "shifted")
    want = manifold_ref.manifold(xc, yc, ks)
    for key in KEYS:
        assert want[key][:2] == [0.0, 0.0] and far[key][:2] == [0.0, 0.0], key
    perm = torch.randperm(20, generator=torch.Generator().manual_seed(1)).cuda()
    same = Qm.manifold(x[perm].contiguous(), x, ks=(1, 3, 5))
    print("permuted: %s" % same)
    for key in ("precision", "recall", "coverage"):
        assert same[key] == [1.0, 1.0, 1.0], key
    assert all(v >= 1.0 for v in same["density"]) and far["nonfinite"] == same["nonfinite"] == 0


MK = (1, 3)
OLD_KEYS = ["bandwidth_scales", "images", "nonfinite", "real", "seed", "sigma0", "split", "steps", "train_images"]
OLD_STEP = ["mmd2", "mmd2_at_sigma0", "nn_accuracy", "nn_real", "nn_train"]


@pytest.fixture(scope="module")
def tiny():
    """One report with and one without manifold_k of the tiny network (shared, never modified), and its trainer."""
    tr = _trainer(_net())
    before = (tr.state_dict(), tr.network.iteration, tr.network.adam_updates, tr.network.params.clone())
    return tr, tr.sample_quality(manifold_k=MK), tr.sample_quality(), before


def _strip(res):
    out = {k: v for k, v in res.items() if k != "manifold_k"}
    out["real"] = {k: v for k, v in res["real"].items() if k != "manifold_train"}
    out["steps"] = [{k: v for k, v in s.items() if k != "manifold"} for s in res["steps"]]
    return out


def test_every_manifold_number_matches_a_recomputation(tiny):
    tr, res, _, _ = tiny
    xs, Rr, train = _gather(SEED, _net())
    assert res["manifold_k"] == list(MK) and res["nonfinite"] == 0
    for t, x in enumerate(xs):
        _within(res["steps"][t]["manifold"], _brackets(x, Rr, MK), MK, "step %d" % t)
    _within(res["real"]["manifold_train"], _brackets(Rr, train, MK), MK, "real against train")
    assert tr.sample_quality(manifold_k=MK, train_images=3)["real"]["manifold_train"] is None  # 3 <= max(k)


def test_without_manifold_k_the_report_is_what_it_was(tiny):
    _, res, plain, _ = tiny
    assert sorted(plain) == OLD_KEYS and sorted(plain["real"]) == ["nn_train"]
    assert all(sorted(s) == OLD_STEP for s in plain["steps"])
    assert sorted(res) == sorted(OLD_KEYS + ["manifold_k"]) and sorted(res["real"]) == ["manifold_train", "nn_train"]
    assert all(sorted(s) == sorted(OLD_STEP + ["manifold"]) for s in res["steps"])
    assert _strip(res) == plain


def test_the_report_moves_nothing_and_repeats(tiny):
    tr, res, _, (state, it, adam, params) = tiny
    assert tr.state_dict() == state and (tr.dataset.train_idx, tr.dataset.test_idx) == (0, 0)
    assert (tr.train_offset, tr.test_offset, tr.iteration) == (0, 0, 0)
    assert (tr.network.iteration, tr.network.adam_updates) == (it, adam)
    assert torch.equal(tr.network.params, params)
    assert json.dumps(tr.sample_quality(manifold_k=MK)) == json.dumps(res)
    assert json.loads(json.dumps(res)) == res
    with pytest.raises(ValueError):
        tr.sample_quality(manifold_k=(8,))  # N - 1 = 7 other points
    with pytest.raises(ValueError):
        tr.sample_quality(manifold_k=(0,))
    assert tr.sample_quality(manifold_k=(7,))["manifold_k"] == [7]


def test_quality_k_reaches_sample_quality_jsonl(tmp_path):
    tr = _trainer(_net(), base_dir=str(tmp_path / "on"), quality_frequency=2, quality_k=MK)
    plain = _trainer(_net(), base_dir=str(tmp_path / "off"), quality_frequency=2)
    for _ in range(2):
        tr.step(), plain.step()
    row = json.loads((tmp_path / "on" / "sample_quality.jsonl").read_text().splitlines()[0])
    old = json.loads((tmp_path / "off" / "sample_quality.jsonl").read_text().splitlines()[0])
    assert row["manifold_k"] == list(MK) and all("manifold" in s for s in row["steps"])
    assert row == dict(iteration=2, **tr.sample_quality(manifold_k=MK))
    assert "manifold_k" not in old and _strip(row) == old
    assert torch.equal(tr.network.params, plain.network.params)  # the option changes no training step


def test_the_averaged_weights_carry_it():
    tr = _trainer(_net(), ema_decay=0.99)
    for _ in range(2):
        tr.step()
    avg, live = tr.sample_quality(weights="ema", manifold_k=MK), tr.sample_quality(weights="train", manifold_k=MK)
    assert (avg["weights"], live["weights"]) == ("ema", "train") and avg["manifold_k"] == live["manifold_k"] == list(MK)
    assert all(sorted(s["manifold"]) == ["coverage", "density", "k", "nonfinite", "precision", "recall"]
               for s in avg["steps"])
    assert avg["real"] == live["real"]  # the real side has no weights
    assert _strip(avg) == tr.sample_quality(weights="ema")
