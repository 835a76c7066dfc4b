"""JPEG-artefact measurements; prints one JSON line and writes it to profiles/jpeg_bench.json
(or --out).

At CelebA geometry (64x64x3, B = 128), p = 1, quality uniform in 10 .. 90, alternating in rounds in this process,
event-timed:

  jpeg444   one svae_op_jpeg_batch launch, 4:4:4, from a clean fp32 batch into a second tensor
  jpeg420   the same at 4:2:0
  torch     a torch formulation on the same data: levels, YCbCr, unfold to 8 x 8 blocks, two matmuls with the DCT
            matrix, divide by per-image tables, round, multiply, two matmuls back, fold, RGB, dequantise (4:4:4)

The kernel reads and writes the batch once: bytes_moved = 2 * B*H*W*C * 4, reported over the kernel time of a trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_jpeg.py --profile-case jpeg420; pass the figure back with
--kernel-us to have the rate computed) and over the event-timed time, which is bounded below by the host's enqueue.

The training step: --step-processes fresh processes per variant (default 3), alternating, each time
NoisyTrainer.step() of preset celeba (bf16x6, denoise_train, synthetic data) with Degradation(jpeg = (1, 10, 90, 2))
("on") or with the jpeg stage off ("off": the same degrade launch, no jpeg launch); the median of every process and
the range of all rounds are reported.  One variant per process: a first layout that built both trainers in one process timed the
one built second ("off") 0.7 ms a step slower than the first, which processes of their own do not show
(profiles/jpeg_bench_one_process.json).  No threshold is set on any figure.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"
B, H, W, C = 128, 64, 64, 3
PER = H * W * C
BYTES = 2 * B * PER * 4
Q_LO, Q_HI = 10, 90


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def torch_tables(q):
    """[B, 2, 8, 8] float tables of the per-image qualities q [B] (IJG scaling of the Annex K tables)."""
    import torch
    luma = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
    chroma = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
              47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
    base = torch.tensor([luma, chroma], device=q.device).view(1, 2, 8, 8)
    s = torch.where(q < 50, 5000 // q, 200 - 2 * q).view(-1, 1, 1, 1)
    return ((base * s + 50) // 100).clamp(1, 255).float()


def torch_jpeg(x, q, Cm):
    """x [B,H,W,3] in [-1, 1], q [B] int64 qualities, Cm the 8 x 8 DCT matrix: the 4:4:4 round trip."""
    import torch
    T = torch_tables(q)
    T = torch.stack([T[:, 0], T[:, 1], T[:, 1]], 1).view(B, 3, 1, 1, 8, 8)
    L = ((x + 1.0) * 127.5).round().clamp(0, 255)
    R, G, Bl = L[..., 0], L[..., 1], L[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * Bl
    Cb = 128 - 0.168735892 * R - 0.331264108 * G + 0.5 * Bl
    Cr = 128 + 0.5 * R - 0.418687589 * G - 0.081312411 * Bl
    P = torch.stack([Y, Cb, Cr], 1).round().clamp(0, 255) - 128          # [B,3,H,W]
    blk = P.unfold(2, 8, 8).unfold(3, 8, 8)                               # [B,3,H/8,W/8,8,8]
    F = Cm @ blk @ Cm.t()
    Gq = (F / T).round() * T
    g = (Cm.t() @ Gq @ Cm + 128).round().clamp(0, 255)
    P = g.permute(0, 1, 2, 4, 3, 5).reshape(B, 3, H, W)
    Y, Cb, Cr = P[:, 0], P[:, 1] - 128, P[:, 2] - 128
    out = torch.stack([Y + 1.402 * Cr, Y - 0.344136286 * Cb - 0.714136286 * Cr, Y + 1.772 * Cb], -1)
    return out.round().clamp(0, 255) * (2.0 / 255.0) - 1.0


def op_legs():
    import math
    import torch
    DG = importlib.import_module(PKG + ".degrade")
    g = torch.Generator().manual_seed(0)
    # smooth images plus noise: what a codec is meant for (the kernel's time does not depend on the values)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ph = torch.rand(B, 1, 1, C, generator=g) * 6.28
    x = 0.8 * torch.sin(yy[None, :, :, None] / 7 + ph) * torch.cos(xx[None, :, :, None] / 5 + ph)
    x = (x + 0.05 * torch.randn(B, H, W, C, generator=g)).clamp(-1, 1).cuda().contiguous()
    out = torch.empty_like(x)
    Cm = torch.tensor([[(math.sqrt(0.125) if u == 0 else 0.5 * math.cos((2 * k + 1) * u * math.pi / 16))
                        for k in range(8)] for u in range(8)], device="cuda")
    q = torch.randint(Q_LO, Q_HI + 1, (B,), generator=g).cuda()
    s444, s420 = DG.Degradation(jpeg=(1.0, Q_LO, Q_HI, 1)), DG.Degradation(jpeg=(1.0, Q_LO, Q_HI, 2))
    return {"jpeg444": lambda i: DG.jpeg_batch(x, s444, -1.0, 1.0, 1, i * B, out=out),
            "jpeg420": lambda i: DG.jpeg_batch(x, s420, -1.0, 1.0, 1, i * B, out=out),
            "torch": lambda i: torch_jpeg(x, q, Cm)}


def step_case(which, steps, warmup, rounds):
    """ms per NoisyTrainer.step() with the jpeg stage "on" or "off", one round per entry; one JSON line."""
    import torch
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    NT = importlib.import_module(PKG + ".trainer").NoisyTrainer
    DD = importlib.import_module(PKG + ".data").DeviceDataset
    DG = importlib.import_module(PKG + ".degrade")
    cfg = cfgmod.preset("celeba", dtype="bf16x6")
    assert (cfg.batch, cfg.height, cfg.width, cfg.channels) == (B, H, W, C)
    ds = DD.synthetic(8 * B, H, W, C, seed=3, device="cuda")
    deg = DG.Degradation(jpeg=(1.0, Q_LO, Q_HI, 2)) if which == "on" else DG.Degradation()
    t = NT(SV(cfg, seed=0), ds, denoise_train=True, seed=1, degradation=deg)
    for _ in range(warmup):
        t.step()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            t.step()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / steps * 1e3, 4))
    print(json.dumps(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-processes", type=int, default=3)
    ap.add_argument("--kernel-us", type=float, default=None,
                    help="mean kernel time of jpeg_batch_kernel from a rocprofv3 --kernel-trace --stats run of --profile-case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    ap.add_argument("--profile-case", default=None, metavar="LEG",
                    help="only run this leg --iters times, nothing timed (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--step-case", default=None, choices=["on", "off"],
                    help="(internal) one process of the training-step comparison")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg needs a GPU")
    if a.step_case:
        return step_case(a.step_case, a.steps, a.warmup, a.rounds)
    legs = op_legs()
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
    res = dict(tool="bench_jpeg", device=torch.cuda.get_device_name(0), shape=[B, H, W, C], p=1.0, quality=[Q_LO, Q_HI],
               iters=a.iters, bytes_moved=BYTES,
               timing="device events around --iters enqueues, alternating rounds; bounded below by the host enqueue",
               legs={k: dict(us_per_batch_median=round(med(v), 2), us_per_batch_min=round(min(v), 2),
                             us_rounds=[round(t, 2) for t in v]) for k, v in us.items()})
    for k in ("jpeg444", "jpeg420"):
        res["legs"][k]["tb_per_s_event_timed"] = round(BYTES / (med(us[k]) * 1e-6) / 1e12, 4)
    res["torch_over_jpeg444"] = round(med(us["torch"]) / med(us["jpeg444"]), 2)
    if a.kernel_us is not None:
        res["kernel"] = dict(us=a.kernel_us, source="rocprofv3 --kernel-trace --stats, jpeg420 leg",
                             tb_per_s=round(BYTES / (a.kernel_us * 1e-6) / 1e12, 4))
    procs = {"on": [], "off": []}
    for _ in range(a.step_processes):
        for which in procs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-case", which, "--steps", str(a.steps),
                                "--warmup", str(a.warmup), "--rounds", str(a.rounds)], capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit("step process failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
            procs[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
    if a.step_processes:
        flat = {k: [t for p in v for t in p] for k, v in procs.items()}
        res["training_step"] = dict(
            config="celeba", dtype="bf16x6", what="NoisyTrainer.step(), denoise_train, ms per step; one variant per process",
            processes=procs, median_per_process={k: [med(p) for p in v] for k, v in procs.items()},
            on_ms=med(flat["on"]), off_ms=med(flat["off"]),
            range_ms={k: [min(v), max(v)] for k, v in flat.items()},
            on_minus_off_us=round((med(flat["on"]) - med(flat["off"])) * 1e3, 1))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
