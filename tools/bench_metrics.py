"""Image-metric and evaluation measurements; prints one JSON line and writes it to
profiles/image_metrics_bench.json (or --out).

(a) svae_op_image_metrics at CelebA's evaluation shape: the stack [noisy input, x_hat_0 .. x_hat_7] of
    B = 128 images, n = 9 * 128 at 64x64x3, against 128 targets.  One launch per call, event-timed over --iters
    calls, mean us per call per round; with it the fp64 operations the separable formulation needs (counted from
    the shape below) and the bytes it must read once.  --profile-only launches the same calls untimed, for the
    kernel's own time in a kernel trace.
(b) the same four columns by a straightforward torch formulation on the same device and the same fp32 NHWC
    input, in fp64: the five quantities x, y, x^2, y^2, x y as channels of one tensor, two grouped conv2d (1 x 11
    then 11 x 1, valid), the SSIM map and its mean, and the two elementwise sums and the non-finite count.  Timed
    in the same process in alternating rounds; the largest difference between the two results is reported.
(c) NoisyTrainer.evaluate() on a synthetic CelebA-shaped test split of --windows whole windows at the celeba
    preset (B = 128, T = 8), host clock (it ends in its device -> host copy), per window; beside it a bare
    forward(input, target, eps, 1.0) per window, synchronised, in the same rounds.
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"
L = importlib.import_module(PKG + "._lib")
M = importlib.import_module(PKG + ".metrics")
WIN = L.SSIM_WINDOW


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def fp64_ops(n, h, w, c):
    """fp64 operations of the separable formulation per call (an fma counts two): per image and channel the
    horizontal pass makes 5 sums of 11 taps at h (w - 10) places, with 3 products per tap place; the vertical pass
    5 sums of 11 taps at (h - 10)(w - 10) places; about 20 operations for the SSIM quotient per place; 4 per
    element for the two elementwise sums."""
    vh, vw = h - (WIN - 1), w - (WIN - 1)
    per_ch = h * vw * (5 * 2 * WIN + 3 * WIN) + vh * vw * (5 * 2 * WIN + 20)
    return n * (c * per_ch + 4 * h * w * c)


def torch_metrics(x, y, data_range, g):
    """[n, 4] fp64 by torch ops: x [n,H,W,C], y [ny,H,W,C] fp32 NHWC on the device, g the 1-D window (fp64)."""
    n, h, w, c = x.shape
    xd = x.permute(0, 3, 1, 2).double()
    yd = y.permute(0, 3, 1, 2).double().repeat(n // y.shape[0], 1, 1, 1)
    d = xd - yd
    q = torch.cat([xd, yd, xd * xd, yd * yd, xd * yd], 1)  # [n, 5 C, H, W]
    k = 5 * c
    q = F.conv2d(q, g.view(1, 1, 1, WIN).expand(k, 1, 1, WIN), groups=k)
    q = F.conv2d(q, g.view(1, 1, WIN, 1).expand(k, 1, WIN, 1), groups=k)
    mx, my, sxx, syy, sxy = q.split(c, 1)
    c1, c2 = (L.SSIM_K1 * data_range) ** 2, (L.SSIM_K2 * data_range) ** 2
    vx, vy, cxy = sxx - mx * mx, syy - my * my, sxy - mx * my
    ssim = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    bad = (~torch.isfinite(xd)).flatten(1).sum(1) + (~torch.isfinite(yd)).flatten(1).sum(1)
    return torch.stack([(d * d).flatten(1).sum(1), d.abs().flatten(1).sum(1), ssim.flatten(1).mean(1), bad.double()], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="celeba")
    ap.add_argument("--dtype", default="bf16x6")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=4, help="whole test windows of the evaluation leg")
    ap.add_argument("--skip-evaluate", action="store_true", help="legs (a) and (b) only")
    ap.add_argument("--profile-only", action="store_true",
                    help="only launch the op --iters times, nothing timed (for rocprofv3 --kernel-trace --stats -- "
                         "python tools/bench_metrics.py --profile-only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a GPU")
    cfgmod = importlib.import_module(PKG + ".config")
    cfg = cfgmod.preset(a.config, dtype=a.dtype)
    B, T, H, W, C = cfg.batch, cfg.mc_steps, cfg.height, cfg.width, cfg.channels
    lo, hi = (float(v) for v in cfg.range)
    rng = hi - lo
    n = (T + 1) * B
    gen = torch.Generator(device="cuda").manual_seed(0)
    # smooth targets plus noise, and a stack of noisier copies: SSIM well inside (0, 1), as in an evaluation
    yy = torch.linspace(0, 1, H, device="cuda").view(1, H, 1, 1)
    xx = torch.linspace(0, 1, W, device="cuda").view(1, 1, W, 1)
    ab = torch.rand(2, B, 1, 1, C, generator=gen, device="cuda")
    y = (lo + rng * (ab[0] * yy + ab[1] * xx * (1 - ab[0]))
         + 0.1 * rng * (torch.rand(B, H, W, C, generator=gen, device="cuda") - 0.5)).clamp(lo, hi).contiguous()
    x = (y.repeat(T + 1, 1, 1, 1) + 0.2 * rng * (torch.rand(n, H, W, C, generator=gen, device="cuda") - 0.5)
         ).clamp(lo, hi).contiguous()
    out = torch.empty(n, 4, dtype=torch.float64, device="cuda")
    op = lambda: M.image_metrics(x, y, rng, out=out)
    if a.profile_only:
        for _ in range(a.iters):
            op()
        torch.cuda.synchronize()
        return
    k = torch.arange(WIN, dtype=torch.float64, device="cuda") - WIN // 2
    g = torch.exp(-(k * k) / (2.0 * L.SSIM_SIGMA ** 2))
    g = g / g.sum()
    ref = lambda: torch_metrics(x, y, rng, g)
    diff = (op() - ref()).abs().max(0).values.tolist()
    legs = {"op": op, "torch_fp64_separable_conv2d": ref}
    for f in legs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, f in legs.items():
            us[name].append(timed(f, a.iters))
    mean = lambda v: sum(v) / len(v)
    ops, nbytes = fp64_ops(n, H, W, C), 4 * (n + B) * H * W * C
    kernel = {name: dict(us_per_call=round(mean(v), 2), us_rounds=[round(t, 2) for t in v]) for name, v in us.items()}
    kernel["op"].update(fp64_ops_per_call=ops, fp64_gflop_per_s=round(ops / mean(us["op"]) / 1e3, 1),
                        bytes_read_once=nbytes, gb_per_s_on_those_bytes=round(nbytes / mean(us["op"]) / 1e3, 1))
    kernel["op_over_torch"] = round(mean(us["op"]) / mean(us["torch_fp64_separable_conv2d"]), 4)
    kernel["max_abs_difference_per_column"] = diff
    res = dict(tool="bench_metrics", device=torch.cuda.get_device_name(0), shape=dict(n=n, ny=B, h=H, w=W, c=C),
               data_range=rng, iters=a.iters, rounds=a.rounds, kernel=kernel)

    if not a.skip_evaluate:
        SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
        DS = importlib.import_module(PKG + ".data").DeviceDataset
        NT = importlib.import_module(PKG + ".trainer").NoisyTrainer
        net = SV(cfg, seed=0)
        ds = DS.synthetic(5 * a.windows * B, H, W, C, seed=0, range=cfg.range, device="cuda")  # a fifth is the test split
        assert ds.test_size == a.windows * B, ds.test_size
        tr = NT(net, ds, denoise_train=True, seed=0)
        inp, tgt = tr._next(test=True)
        eps = torch.randn(T, B, cfg.latent_dim, device="cuda")

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3  # ms

        def forwards():
            for _ in range(a.windows):
                net.forward(inp, tgt, eps, 1.0)

        tr.evaluate()
        forwards()
        ev_ms, fw_ms = [], []
        for _ in range(a.rounds):
            fw_ms.append(clock(forwards) / a.windows)
            ev_ms.append(clock(tr.evaluate) / a.windows)
        res["evaluate"] = dict(config=a.config, dtype=a.dtype, batch=B, mc_steps=T, windows=a.windows,
                               evaluate_ms_per_window=round(mean(ev_ms), 3),
                               evaluate_ms_rounds=[round(v, 3) for v in ev_ms],
                               forward_ms_per_window=round(mean(fw_ms), 3),
                               forward_ms_rounds=[round(v, 3) for v in fw_ms],
                               evaluate_over_forward=round(mean(ev_ms) / mean(fw_ms), 4))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
