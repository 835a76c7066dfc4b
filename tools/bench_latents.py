"""Latent-information measurements; prints one JSON line and writes it to
profiles/latent_information_bench.json (or --out).

(a) svae_op_mixture_logdensity with nq = nm = N and latents.segments_for's list (whole code, levels, every single
    dimension): N = 1 152 (nine CelebA windows), 10 000 and 40 520 (CelebA's test split) at the celeba preset's
    Dz = 12, and N = 10 000 at the lsun preset's Dz = 110.  Posteriors as a trained model has them: means N(0, 1),
    sigma log-uniform in [0.05, 1], z one draw from each.  Event-timed, mean us per call per round; with it the
    Gaussian terms and exponentials a call evaluates (counted from the shape) and the launches it makes.
    --profile-only launches the N = 10 000 calls untimed, for the kernel's own time in a kernel trace.
(b) the same table by a torch fp64 formulation on the same inputs: query rows in chunks of about 1 GB of
    [chunk, N, Dz] fp64 terms, torch.logsumexp over the components per single dimension and, after a sum over its
    slice, per group.  Timed in the same process in alternating rounds; the largest difference is reported.
(c) NoisyTrainer.latent_information() on a synthetic CelebA-shaped test split of --windows whole windows at the
    celeba preset (B = 128, T = 8), host clock (it ends in its device -> host copy); beside it the bare
    forward(input, target, eps, 1.0) of those windows, synchronised, in the same rounds.
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"
Lt = importlib.import_module(PKG + ".latents")
CELEBA_TEST = 40520  # the last fifth of 202 599 images
CHUNK_BYTES = 1 << 30


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def inputs(n, dz, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mean = torch.randn(n, dz, generator=gen, device="cuda")
    sigma = torch.exp(torch.rand(n, dz, generator=gen, device="cuda") * math.log(0.05))
    z = mean + sigma * torch.randn(n, dz, generator=gen, device="cuda")
    return z, mean, sigma


def torch_table(z, mu, sigma, segs):
    """[N, n_seg] fp64 by torch ops, no [N, N, Dz] tensor: chunks of query rows."""
    n, dz = z.shape
    md, inv = mu.double()[None], (1.0 / sigma.double())[None]
    cst = (-torch.log(sigma.double()) - 0.5 * math.log(2.0 * math.pi))[None]
    out = torch.empty(n, len(segs), dtype=torch.float64, device=z.device)
    chunk = max(1, CHUNK_BYTES // (8 * n * dz))
    for a in range(0, n, chunk):
        u = (z[a:a + chunk].double()[:, None, :] - md) * inv
        t = cst - 0.5 * u * u  # [chunk, N, Dz]
        single = torch.logsumexp(t, dim=1)
        for i, (_, off, ln) in enumerate(segs):
            out[a:a + chunk, i] = single[:, off] if ln == 1 else torch.logsumexp(t[:, :, off:off + ln].sum(2), dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16x6")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=9, help="whole test windows of the latent_information leg")
    ap.add_argument("--skip-trainer", action="store_true", help="legs (a) and (b) only")
    ap.add_argument("--profile-only", action="store_true",
                    help="only launch the N = 10 000 calls, nothing timed (for rocprofv3 --kernel-trace --stats -- "
                         "python tools/bench_latents.py --profile-only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_information_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latents needs a GPU")
    cfgmod = importlib.import_module(PKG + ".config")
    celeba, lsun = cfgmod.preset("celeba", dtype=a.dtype), cfgmod.preset("lsun", dtype=a.dtype)
    shapes = [("celeba", celeba, 1152), ("celeba", celeba, 10000), ("celeba", celeba, CELEBA_TEST),
              ("lsun", lsun, 10000)]
    mean_of = lambda v: sum(v) / len(v)
    rows = []
    for k, (name, cfg, n) in enumerate(shapes):
        if a.profile_only and n != 10000:
            continue
        segs = Lt.segments_for(cfg)
        dz = cfg.latent_dim
        z, mu, sigma = inputs(n, dz, k)
        out = torch.empty(n, len(segs), dtype=torch.float64, device="cuda")
        op = lambda: Lt.mixture_logdensity(z, mu, sigma, segs, out=out)
        if a.profile_only:
            for _ in range(3):
                op()
            torch.cuda.synchronize()
            continue
        ref = lambda: torch_table(z, mu, sigma, segs)
        got, want = op().clone(), ref()
        diff = float((got - want).abs().max())
        rel = float(((got - want).abs() / want.abs().clamp_min(1.0)).max())
        del want
        legs = {"op": op, "torch_fp64_chunked_logsumexp": ref}
        iters = {}
        for nm_, f in legs.items():  # warm up, and size the timed window to about half a second
            f()
            first = timed(f, 1)
            iters[nm_] = max(1, min(50, int(5e5 / first)))
        us = {nm_: [] for nm_ in legs}
        for _ in range(a.rounds):
            for nm_, f in legs.items():
                us[nm_].append(timed(f, iters[nm_]))
        terms, exps = n * n * sum(s[2] for s in segs), n * n * len(segs)
        t_op, t_ref = mean_of(us["op"]), mean_of(us["torch_fp64_chunked_logsumexp"])
        rows.append(dict(config=name, n=n, dz=dz, segments=len(segs),
                         op=dict(us_per_call=round(t_op, 1), us_rounds=[round(v, 1) for v in us["op"]],
                                 iters=iters["op"], gaussian_terms_per_call=terms, exponentials_per_call=exps,
                                 g_exponentials_per_s=round(exps / t_op / 1e3, 1)),
                         torch_fp64_chunked_logsumexp=dict(us_per_call=round(t_ref, 1),
                                                           us_rounds=[round(v, 1) for v in
                                                                      us["torch_fp64_chunked_logsumexp"]],
                                                           iters=iters["torch_fp64_chunked_logsumexp"],
                                                           query_rows_per_chunk=max(1, CHUNK_BYTES // (8 * n * dz))),
                         op_over_torch=round(t_op / t_ref, 4), max_abs_difference=diff,
                         max_difference_over_max_1_abs=rel))
        print(json.dumps(rows[-1]), flush=True)
    if a.profile_only:
        return
    res = dict(tool="bench_latents", device=torch.cuda.get_device_name(0), rounds=a.rounds, tile=Lt.TILE, op=rows)

    if not a.skip_trainer:
        SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
        DS = importlib.import_module(PKG + ".data").DeviceDataset
        NT = importlib.import_module(PKG + ".trainer").NoisyTrainer
        cfg = celeba
        B, T, H, W, C = cfg.batch, cfg.mc_steps, cfg.height, cfg.width, cfg.channels
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

        rep = tr.latent_information()
        forwards()
        li_ms, fw_ms = [], []
        for _ in range(a.rounds):
            fw_ms.append(clock(forwards))
            li_ms.append(clock(tr.latent_information))
        res["latent_information"] = dict(config="celeba", dtype=a.dtype, batch=B, mc_steps=T, windows=a.windows,
                                         images=rep["images"], latent_information_ms=round(mean_of(li_ms), 3),
                                         latent_information_ms_rounds=[round(v, 3) for v in li_ms],
                                         forwards_ms=round(mean_of(fw_ms), 3),
                                         forwards_ms_rounds=[round(v, 3) for v in fw_ms],
                                         latent_information_over_forwards=round(mean_of(li_ms) / mean_of(fw_ms), 4))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
