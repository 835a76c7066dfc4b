"""NoisyTrainer.evaluate on the GPU: preset ``tiny`` (B = 4, 32x32x3, T = 3) on DeviceDataset.synthetic(55, ...),
whose 11 test images make two whole windows and the partial one [7, 11), of which rows 8 .. 10 are new.

Every reported number is recomputed here from the specification: the windows, the svae_op_make_batch call under
the key seed ^ eval_seed_xor from offset 0, eps and then the chain noise of every window from one
torch.Generator(device).manual_seed(seed), forward at reg_coeff 1.0 on an identically initialised network, and
x_hat_t scored by tests/metrics_ref.py.  Agreement is within the helper's bound; a mean of at most 11 per-image
values adds (images + 2) 2^-52 of the mean of their magnitudes for its fp64 additions and its division.
"""
import json
import math

import numpy as np
import pytest
import torch

import metrics_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

SEED = 77
B, H, W, C = 4, 32, 32, 3
PER = H * W * C
GROUPS = (B * PER + 3) // 4
WINDOWS = [(0, 4), (4, 4), (7, 3)]  # (start, rows not yet counted) over the 11 test images
L = 2.0


def _net(preset="tiny", seed=0):
    cfg = pkg_mod("config").preset(preset, batch=B, dtype="fp32")
    return pkg_mod("sequential_vae").SequentialVAE(cfg, seed=seed)


def _dataset(n=55):
    return pkg_mod("data").DeviceDataset.synthetic(n, H, W, C, seed=3, device="cuda")


def _trainer(net, ds=None, **kw):
    kw.setdefault("denoise_train", True)
    return pkg_mod("trainer").NoisyTrainer(net, ds if ds is not None else _dataset(), seed=SEED, **kw)


class _Mean:
    """Mean of per-image values with the bound the module docstring states."""

    def __init__(self):
        self.v, self.b = [], []

    def add(self, values, bounds=None):
        self.v += [float(x) for x in values]
        self.b += [0.0] * len(values) if bounds is None else [float(x) for x in bounds]

    def check(self, got, what, extra_rel=0.0):
        n = len(self.v)
        want = math.fsum(self.v) / n
        if math.isinf(want):
            assert got == want, what
            return
        mag = math.fsum(abs(x) for x in self.v) / n
        bound = math.fsum(self.b) / n + (n + 2) * 2.0 ** -52 * mag + extra_rel * abs(want)
        print("%-22s got %.17g want %.17g |diff| %.3e bound %.3e" % (what, got, want, abs(got - want), bound))
        assert abs(got - want) <= bound, what


def _recompute(preset, seed, denoise):
    """{name: _Mean} by the specification, on a network initialised as the evaluated one."""
    L_ = pkg_mod("_lib")
    net, ds = _net(preset), _dataset()
    tr = pkg_mod("trainer").NoisyTrainer  # its constants
    T, Dz = net.cfg.mc_steps, net.cfg.latent_dim
    gen = torch.Generator(device="cuda").manual_seed(seed)
    noise_par = (tr.pepper_prob, tr.salt_prob, tr.gaussian_noise_scale) if denoise else (0.0, 0.0, 0.0)
    m = {k: _Mean() for k in ["elbo", "rec_last"] + ["%s%d" % (q, s) for q in ("mse", "psnr", "ssim") for s in range(T + 1)]
         + ["%s%d" % (q, t) for q in ("recon", "kl") for t in range(T)]}
    for k, (start, fresh) in enumerate(WINDOWS):
        tgt = torch.empty(B, H, W, C, device="cuda")
        inp = torch.empty_like(tgt)
        L_.check(L_.lib().svae_op_make_batch(L_.ptr(ds.test), 1, None, start, B, PER, -1.0, 1.0, *noise_par,
                                             (seed ^ tr.eval_seed_xor) if denoise else 0, k * GROUPS if denoise else 0,
                                             L_.ptr(tgt), L_.ptr(inp), L_.stream_ptr()))
        eps = torch.randn([T, B, Dz], generator=gen, dtype=torch.float32, device="cuda")
        noise = None
        if net.cfg.add_noise_to_chain:
            noise = torch.randn([T, B, H, W, C], generator=gen, dtype=torch.float32, device="cuda")
        net.forward(inp, tgt, eps, 1.0, noise=noise)
        stack = np.stack([inp.cpu().numpy()] + [net.xhat(t).cpu().numpy() for t in range(T)])
        rows, bound = metrics_ref.metrics_ref(stack.reshape(-1, H, W, C), tgt.cpu().numpy(), L)
        rows, bound = rows.reshape(T + 1, B, 4)[:, B - fresh:], bound.reshape(T + 1, B, 4)[:, B - fresh:]
        assert np.all(rows[..., 3] == 0)
        for s in range(T + 1):
            m["mse%d" % s].add(rows[s, :, 0] / PER, bound[s, :, 0] / PER)
            ps = [metrics_ref.psnr_ref(v, PER, L, b) for v, b in zip(rows[s, :, 0], bound[s, :, 0])]
            m["psnr%d" % s].add([p[0] for p in ps], [p[1] for p in ps])
            m["ssim%d" % s].add(rows[s, :, 2], bound[s, :, 2])
        for t in range(T):
            m["recon%d" % t].add(net.copy_out(L_.BUF_REC_IMG, t, B).double().cpu()[B - fresh:])
            m["kl%d" % t].add(net.copy_out(L_.BUF_KL_IMG, t, B).double().cpu()[B - fresh:])
        m["rec_last"].add(net.copy_out(L_.BUF_REC_IMG, T - 1, B).double().cpu()[B - fresh:])
        m["elbo"].add(net.elbo_per_image().cpu()[B - fresh:])
    return m, net.cfg


@pytest.fixture(scope="module")
def tiny_eval():
    """One evaluation of the tiny network's test split (shared, never modified) and its trainer."""
    tr = _trainer(_net())
    before = (tr.state_dict(), tr.network.iteration, tr.network.adam_updates, tr.network.params.clone())
    return tr, tr.evaluate(), before


def _check_against_recomputation(res, preset, seed, denoise):
    m, cfg = _recompute(preset, seed, denoise)
    T = cfg.mc_steps
    assert (res["split"], res["images"], res["seed"]) == ("test", 11, seed)
    assert sorted(res) == ["elbo", "error_per_pixel", "images", "input", "seed", "split", "steps"]
    assert sorted(res["input"]) == ["mse", "psnr", "ssim"] and len(res["steps"]) == T
    for q in ("mse", "psnr", "ssim"):
        m["%s0" % q].check(res["input"][q], "input %s" % q)
        for t in range(T):
            m["%s%d" % (q, t + 1)].check(res["steps"][t][q], "step %d %s" % (t, q))
    for t in range(T):
        assert sorted(res["steps"][t]) == ["kl", "mse", "psnr", "recon", "ssim"]
        m["recon%d" % t].check(res["steps"][t]["recon"], "step %d recon" % t)
        m["kl%d" % t].check(res["steps"][t]["kl"], "step %d kl" % t)
    m["elbo"].check(res["elbo"], "elbo")
    # sum (x_hat_{T-1} - x)^2 / (H W) is C times the last step's mse, exactly as reported
    assert res["error_per_pixel"] == res["steps"][-1]["mse"] * C
    if not cfg.predict_generator_noise:
        # the engine's fp32 mean((mle - target)^2) per image, as trainer.test() reads it: an fp32 reduction over
        # H W C terms, n 2^-24 relative
        rec = m["rec_last"]
        want = math.fsum(rec.v) / len(rec.v) * C
        print("error_per_pixel %.9g, from SVAE_BUF_REC_IMG %.9g" % (res["error_per_pixel"], want))
        assert abs(res["error_per_pixel"] - want) <= PER * 2.0 ** -24 * abs(want)
    return m


def test_every_number_matches_a_recomputation(tiny_eval):
    tr, res, _ = tiny_eval
    _check_against_recomputation(res, "tiny", SEED, True)
    # the corrupted input is the baseline: it is not the clean image
    assert res["input"]["mse"] > 1e-3 and res["input"]["ssim"] < 0.9 and math.isfinite(res["input"]["psnr"])


def test_evaluation_moves_nothing_and_repeats(tiny_eval):
    tr, res, (state, it, adam, params) = tiny_eval
    assert tr.state_dict() == state and (tr.dataset.train_idx, tr.dataset.test_idx) == (0, 0)
    assert (tr.train_offset, tr.test_offset, tr.iteration) == (0, 0, 0)
    assert (tr.network.iteration, tr.network.adam_updates) == (it, adam)
    assert torch.equal(tr.network.params, params)
    assert tr.evaluate() == res
    assert json.loads(json.dumps(res)) == res
    other = tr.evaluate(seed=SEED + 1)
    assert other["seed"] == SEED + 1 and other["input"] != res["input"] and other["steps"] != res["steps"]
    first = tr.evaluate(num_batches=1)
    assert first["images"] == 4 and first["input"] != res["input"]
    assert tr.evaluate(split="train", num_batches=2)["images"] == 8
    with pytest.raises(ValueError):
        tr.evaluate(split="validation")
    with pytest.raises(ValueError):
        tr.evaluate(num_batches=0)
    small = _trainer(tr.network, _dataset(15))  # 12 train / 3 test images
    with pytest.raises(ValueError):
        small.evaluate()
    assert small.evaluate(split="train")["images"] == 12


def test_training_is_bitwise_the_same_with_evaluations_between_steps():
    """The evaluation draws nothing from the network's device Philox counter and moves no cursor: a trainer that
    evaluates before and between its steps ends with the parameters of one that never does."""
    a, b = _trainer(_net()), _trainer(_net())
    a.step(), b.step()
    a.evaluate()
    for k in range(3):
        la, lb = a.step(), b.step()
        assert la == lb, k
        if k < 2:
            a.evaluate(split="train", num_batches=1)
    torch.cuda.synchronize()
    assert torch.equal(a.network.params, b.network.params)
    assert a.state_dict() == b.state_dict()


def test_eval_frequency_writes_evaluation_jsonl(tmp_path):
    tr = _trainer(_net(), base_dir=str(tmp_path), eval_frequency=2)
    plain = _trainer(_net())
    for _ in range(4):
        tr.step(), plain.step()
    lines = (tmp_path / "evaluation.jsonl").read_text().splitlines()
    assert len(lines) == 2
    rows = [json.loads(s) for s in lines]
    assert [r["iteration"] for r in rows] == [2, 4] and rows[0]["steps"] != rows[1]["steps"]
    now = dict(iteration=4, **tr.evaluate())
    assert rows[1] == now
    assert torch.equal(tr.network.params, plain.network.params)  # the option changes no training step
    assert not (tmp_path / "summaries.jsonl").exists()


def test_chain_noise_is_injected_under_tiny_flat():
    """tiny_flat adds noise to the chain: the evaluation injects it after eps from the same generator."""
    tr = _trainer(_net("tiny_flat"))
    assert tr.network.cfg.add_noise_to_chain
    res = tr.evaluate()
    _check_against_recomputation(res, "tiny_flat", SEED, True)
    assert tr.evaluate() == res


def test_without_denoise_train_the_input_is_the_clean_image():
    tr = _trainer(_net(), denoise_train=False)
    res = tr.evaluate(seed=5)
    assert res["input"]["mse"] == 0.0 and res["input"]["psnr"] == math.inf and abs(res["input"]["ssim"] - 1.0) < 1e-12
    _check_against_recomputation(res, "tiny", 5, False)
