"""Structured-corruption measurements; prints one JSON line and writes it to
profiles/degrade_bench.json (or --out).

At CelebA geometry (64x64x3, B = 128, uint8 dataset), alternating in rounds in this process, event-timed over
windows that walk a dataset larger than one batch:

  degraded      svae_op_make_batch (target only) + svae_op_degrade_batch, every stage on every image (p = 1: blur
                sigma in [0.5, 4], factor 4, 2 boxes) and the reference's pixel noise: what a NoisyTrainer with a
                Degradation enqueues per step
  degraded_half the same at p = 0.5 per stage
  make_batch    the single svae_op_make_batch launch (target + noisy input) a trainer without a Degradation enqueues
  torch         the same corruptions written with torch ops on the clean batch: conv2d blur (per-image kernels,
                replicate padding), avg_pool2d + repeat_interleave, box masks, rand / randn noise, clamp

and the engine's training step (preset celeba, bf16x6, forward + backward_apply on a fixed batch: the step bench.py
times), of which the degraded batch is reported as a share.  The event-timed mean of a leg is bounded below by the
host's enqueue time of its launches (two ctypes calls for `degraded`); no threshold is set on any figure.  Kernel
times come from a trace of one leg: rocprofv3 --kernel-trace --stats -- python tools/bench_degrade.py --profile-case
degraded.
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"
L = importlib.import_module(PKG + "._lib")
DG = importlib.import_module(PKG + ".degrade")
B, H, W, C = 128, 64, 64, 3
PER = H * W * C
NOISE = (0.1, 0.1, 0.1)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def torch_degrade(x, p, gen):
    """x [B,H,W,C] clean, in [-1, 1]: blur, factor-4 box down-sampling, 2 cut-out boxes, each with probability p per
    image, then pepper x0, salt +1, Gaussian 0.1 and the clip."""
    dev = x.device
    u = torch.rand(B, 12, device=dev, generator=gen)
    img = x.permute(0, 3, 1, 2).reshape(1, B * C, H, W)
    sigma = 0.5 + u[:, 0] * 3.5
    k = torch.arange(-12, 13, device=dev, dtype=torch.float32)
    g = torch.exp(-k[None, :] ** 2 / (2 * sigma[:, None] ** 2)) * (k.abs()[None, :] <= torch.ceil(3 * sigma)[:, None])
    g = (g / g.sum(1, keepdim=True)).repeat_interleave(C, 0)
    blurred = F.conv2d(F.pad(img, (12, 12, 0, 0), mode="replicate"), g.view(B * C, 1, 1, 25), groups=B * C)
    blurred = F.conv2d(F.pad(blurred, (0, 0, 12, 12), mode="replicate"), g.view(B * C, 1, 25, 1), groups=B * C)
    img = torch.where((u[:, 1] < p).repeat_interleave(C)[None, :, None, None], blurred, img)
    down = F.avg_pool2d(img, 4).repeat_interleave(4, 2).repeat_interleave(4, 3)
    img = torch.where((u[:, 2] < p).repeat_interleave(C)[None, :, None, None], down, img)
    img = img.view(B, C, H, W)
    yy = torch.arange(H, device=dev)[None, :, None]
    xx = torch.arange(W, device=dev)[None, None, :]
    hit = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
    for q in range(2):
        side = 8 + (u[:, 4 + 4 * q:6 + 4 * q] * 17).long()
        y0 = (u[:, 6 + 4 * q] * (H - side[:, 0] + 1)).long()[:, None, None]
        x0 = (u[:, 7 + 4 * q] * (W - side[:, 1] + 1)).long()[:, None, None]
        hit |= (yy >= y0) & (yy < y0 + side[:, 0, None, None]) & (xx >= x0) & (xx < x0 + side[:, 1, None, None])
    hit &= (u[:, 3] < p)[:, None, None]
    img = torch.where(hit[:, None], torch.zeros((), device=dev), img).permute(0, 2, 3, 1)
    keep = (torch.rand(img.shape, device=dev, generator=gen) >= NOISE[0]).float()
    salt = (torch.rand(img.shape, device=dev, generator=gen) < NOISE[1]).float()
    return (img * keep + salt + NOISE[2] * torch.randn(img.shape, device=dev, generator=gen)).clamp_(-1.0, 1.0)


def batch_legs(nimg=2048):
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (nimg, PER), dtype=torch.uint8, generator=g).cuda()
    tgt = torch.empty(B, H, W, C, device="cuda")
    inp = torch.empty_like(tgt)
    nwin = nimg // B
    groups = (B * PER + 3) // 4
    gen = torch.Generator(device="cuda").manual_seed(0)
    stream = L.stream_ptr()

    def make_batch(i, noisy):
        p, s, sc = NOISE if noisy else (0.0, 0.0, 0.0)
        L.check(L.lib().svae_op_make_batch(L.ptr(u8), 1, None, (i % nwin) * B, B, PER, -1.0, 1.0, p, s, sc, 1,
                                           i * groups, L.ptr(tgt), L.ptr(inp) if noisy else None, stream))

    def degraded(spec):
        def fn(i):
            make_batch(i, False)
            DG.degrade_batch(tgt, spec, -1.0, 1.0, NOISE, 1, i * groups, out=inp)
        return fn

    def torch_leg(i):
        make_batch(i, False)
        torch_degrade(tgt, 1.0, gen)

    full = DG.Degradation(blur=(1.0, 0.5, 4.0), downsample=(1.0, 4), cutout=(1.0, 2, 8, 24, 0.0))
    half = DG.Degradation(blur=(0.5, 0.5, 4.0), downsample=(0.5, 4), cutout=(0.5, 2, 8, 24, 0.0))
    return {"degraded": degraded(full), "degraded_half": degraded(half), "make_batch": lambda i: make_batch(i, True),
            "torch": torch_leg}


def step_ms(steps, warmup, rounds):
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    cfg = cfgmod.preset("celeba", dtype="bf16x6")
    assert (cfg.batch, cfg.height, cfg.width, cfg.channels) == (B, H, W, C)
    net = SV(cfg, seed=0)
    x = (torch.rand(B, H, W, C, device="cuda") * 2 - 1).contiguous()
    it = [0]

    def engine_step():
        it[0] += 1
        net.forward(x, x, None, 1.0 - math.exp(-it[0] / cfg.reg_coeff_rate))
        net.backward_apply(cfg.learning_rate, it[0])

    for _ in range(warmup):
        engine_step()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            engine_step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_bench.json"))
    ap.add_argument("--profile-case", default=None, metavar="LEG",
                    help="only run this leg --iters times, nothing timed (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_degrade needs a GPU")
    legs = batch_legs()
    if a.profile_case:
        for i in range(a.iters):
            legs[a.profile_case](i)
        torch.cuda.synchronize()
        return
    for fn in legs.values():
        for i in range(5):
            fn(i)
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, a.iters))
    med = lambda v: sorted(v)[len(v) // 2]
    res = dict(tool="bench_degrade", device=torch.cuda.get_device_name(0), shape=[B, H, W, C], iters=a.iters,
               timing="device events around --iters enqueues, alternating rounds; bounded below by the host enqueue",
               legs={k: dict(us_per_batch_median=round(med(v), 2), us_per_batch_min=round(min(v), 2),
                             us_rounds=[round(t, 2) for t in v]) for k, v in us.items()})
    steps = step_ms(a.steps, a.warmup, a.rounds)
    res["training_step"] = dict(config="celeba", dtype="bf16x6", ms_per_step_median=round(med(steps), 3),
                                rounds=[round(t, 3) for t in steps])
    for k in ("degraded", "degraded_half", "make_batch"):
        res["legs"][k]["share_of_training_step"] = round(med(us[k]) / 1e3 / med(steps), 5)
    res["degraded_over_make_batch"] = round(med(us["degraded"]) / med(us["make_batch"]), 3)
    res["torch_over_degraded"] = round(med(us["torch"]) / med(us["degraded"]), 3)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
