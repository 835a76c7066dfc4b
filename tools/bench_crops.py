"""Random-crop measurements; prints one JSON line and writes it to profiles/crops_bench.json (or
--out).

uint8 images of 1024 x 1024 x 3 (--nimg of them), tile 64 x 64, B = 128, three settings:

  plain     s = 1, no symmetry
  mixed     scales {1, 2, 4} with the dihedral group
  s8        s = 8, no symmetry

and per setting two legs, alternating in rounds in this process, event-timed over --iters enqueues at advancing
offsets:

  crop      the single svae_op_crop_batch launch (fp32 target) a NoisyTrainer on a PatchDataset enqueues per step
  torch     the same batch written with torch ops: per-row parameters drawn on the host, per scale an index gather
            of the s h x s w windows, avg_pool2d, per symmetry flip / transpose, dequantise, index_copy_ into the
            batch (the index tensors are uploaded per batch, as a torch data pipeline would)

The event-timed mean of a leg is bounded below by the host's enqueue time of its launches (one ctypes call for
`crop`).  `bytes` are those the crops actually touch: B (s h)(s w) c source bytes read (per row its own scale) plus
B h w c 4 bytes written; `gbps_event` is that over the event time.  Kernel times come from a trace of one leg:
rocprofv3 --kernel-trace --stats -- python tools/bench_crops.py --profile-case mixed; --kernel-us NAME=US,.. records
them in the JSON with the bytes/s they give.

The training step (preset celeba, bf16x6, NoisyTrainer.step() with denoise_train, host clock around --steps steps,
each of which ends in the loss's device -> host copy) is measured in fresh processes, alternating in rounds:

  patches       this tree, PatchDataset over the large images
  plain         this tree, DeviceDataset of 64 x 64 images
  plain_parent  --parent-tree DIR (a built checkout of the parent commit), the same DeviceDataset and step

--step-case CASE runs one such process (with --tree DIR the package is imported from DIR); no threshold is set on
any figure.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "sequential-variational-autoencoder_amd"
B, TILE, C, BIG = 128, 64, 3, 1024
LO, HI = -1.0, 1.0
SETTINGS = {"plain": ((1,), 1), "mixed": ((1, 2, 4), 8), "s8": ((8,), 1)}


def pkg(name):
    return importlib.import_module(PKG + "." + name)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def torch_crops(images, scales, symmetries, rng, out):
    """The torch formulation of one batch into out [B,h,w,c]; parameters from the host generator ``rng``."""
    dev = images.device
    nimg = images.shape[0]
    m = rng.integers(0, nimg, B)
    s = np.asarray(scales)[rng.integers(0, len(scales), B)]
    g = rng.integers(0, symmetries, B)
    y0 = (rng.random(B) * (BIG - s * TILE + 1)).astype(np.int64)
    x0 = (rng.random(B) * (BIG - s * TILE + 1)).astype(np.int64)
    qs = (HI - LO) / 255.0
    for sc in scales:
        rows = np.nonzero(s == sc)[0]
        if rows.size == 0:
            continue
        side = sc * TILE
        idx = torch.from_numpy(np.stack([m[rows], y0[rows], x0[rows]])).to(dev, non_blocking=True)
        ar = torch.arange(side, device=dev)
        win = images[idx[0][:, None, None], (idx[1][:, None] + ar)[:, :, None], (idx[2][:, None] + ar)[:, None, :]]
        x = win.permute(0, 3, 1, 2).to(torch.float32)
        if sc > 1:
            x = F.avg_pool2d(x, sc)
        x = x * qs + LO  # [n, c, h, w]
        gs = g[rows]
        for gv in np.unique(gs):
            sel = np.nonzero(gs == gv)[0]
            part = x[torch.from_numpy(sel).to(dev, non_blocking=True)] if sel.size < rows.size else x
            if gv & 1:
                part = part.flip(3)
            if gv & 2:
                part = part.flip(2)
            if gv & 4:
                part = part.transpose(2, 3)
            out.index_copy_(0, torch.from_numpy(rows[sel]).to(dev, non_blocking=True), part.permute(0, 2, 3, 1).contiguous())
    return s


def crop_legs(nimg, count_bytes=True):
    crops = pkg("crops")
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (nimg, BIG, BIG, C), dtype=torch.uint8, generator=gen).cuda()
    out = torch.empty(B, TILE, TILE, C, device="cuda")
    meta = torch.empty(B, 5, dtype=torch.int32, device="cuda")
    legs, nbytes = {}, {}
    for name, (scales, sym) in SETTINGS.items():
        spec = crops.CropSpec(scales, sym)
        rng = np.random.default_rng(1)
        legs[name + "/crop"] = lambda i, spec=spec: crops.crop_batch(images, (TILE, TILE), spec, B, 1, i * B, (LO, HI),
                                                                     out=out)
        legs[name + "/torch"] = lambda i, scales=scales, sym=sym, rng=rng: torch_crops(images, scales, sym, rng, out)
        # bytes the crops of one batch touch (per row its own scale; the batch at offset 0 stands for the window)
        if not count_bytes:
            continue
        crops.crop_batch(images, (TILE, TILE), spec, B, 1, 0, (LO, HI), out=out, meta=meta)
        s = meta[:, 1].cpu().numpy().astype(np.int64)
        nbytes[name] = int((s * TILE * s * TILE * C).sum() + B * TILE * TILE * C * 4)
    return legs, nbytes


def step_case(case, steps, warmup, rounds, nimg):
    """ms per NoisyTrainer.step() of the celeba preset, one figure per round."""
    cfg = pkg("config").preset("celeba", dtype="bf16x6")
    assert (cfg.batch, cfg.height, cfg.width, cfg.channels) == (B, TILE, TILE, C)
    data = pkg("data")
    gen = torch.Generator().manual_seed(0)
    if case == "patches":
        big = torch.randint(0, 256, (nimg, BIG, BIG, C), dtype=torch.uint8, generator=gen).cuda()
        ds = data.PatchDataset(big[:-1], big[-1:], (TILE, TILE), scales=(1, 2, 4), symmetries=8, eval_crops=B,
                               range=cfg.range)
    else:
        small = torch.randint(0, 256, (2048 + B, TILE, TILE, C), dtype=torch.uint8, generator=gen).cuda()
        ds = data.DeviceDataset(small[:2048], small[2048:], range=cfg.range)
    net = pkg("sequential_vae").SequentialVAE(cfg, seed=0)
    tr = pkg("trainer").NoisyTrainer(net, ds, denoise_train=True, seed=0)
    for _ in range(warmup):
        tr.step()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nimg", type=int, default=16, help="large images held on the device (48 MB at 16)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_bench.json"))
    ap.add_argument("--profile-case", default=None, metavar="SETTING",
                    help="only run this setting's crop leg --iters times, nothing timed (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-us", default=None, metavar="SETTING=US,..",
                    help="kernel times of a trace, recorded with the bytes/s they give")
    ap.add_argument("--step-case", default=None, choices=["patches", "plain"],
                    help="only time the training step of this case in this process and print the rounds as JSON")
    ap.add_argument("--tree", default=ROOT, help="the checkout the package is imported from")
    ap.add_argument("--parent-tree", default=None, metavar="DIR", help="a built checkout of the parent commit")
    ap.add_argument("--step-rounds", type=int, default=3, help="processes per training-step variant")
    ap.add_argument("--no-steps", action="store_true", help="skip the training-step processes")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if not torch.cuda.is_available():
        raise SystemExit("bench_crops needs a GPU")
    if a.step_case:
        print(json.dumps(dict(case=a.step_case, tree=os.path.abspath(a.tree),
                              ms=step_case(a.step_case, a.steps, a.warmup, a.rounds, a.nimg))))
        return
    legs, nbytes = crop_legs(a.nimg, count_bytes=not a.profile_case)
    if a.profile_case:
        for i in range(a.iters):
            legs[a.profile_case + "/crop"](i)
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
    kernel_us = dict((k, float(v)) for k, v in (kv.split("=") for kv in a.kernel_us.split(","))) if a.kernel_us else {}
    res = dict(tool="bench_crops", device=torch.cuda.get_device_name(0), images=[a.nimg, BIG, BIG, C], tile=[TILE, TILE],
               batch=B, iters=a.iters,
               timing="device events around --iters enqueues, alternating rounds; bounded below by the host enqueue",
               settings={})
    for name, (scales, sym) in SETTINGS.items():
        c, t = us[name + "/crop"], us[name + "/torch"]
        row = dict(scales=list(scales), symmetries=sym, bytes_touched=nbytes[name],
                   crop=dict(us_median=round(med(c), 2), us_min=round(min(c), 2), us_rounds=[round(v, 2) for v in c],
                             gbps_event=round(nbytes[name] / med(c) / 1e3, 1)),
                   torch=dict(us_median=round(med(t), 2), us_min=round(min(t), 2), us_rounds=[round(v, 2) for v in t]),
                   torch_over_crop=round(med(t) / med(c), 2))
        if name in kernel_us:
            row["crop"]["kernel_us"] = kernel_us[name]
            row["crop"]["gbps_kernel"] = round(nbytes[name] / kernel_us[name] / 1e3, 1)
        res["settings"][name] = row
    if not a.no_steps:
        variants = [("patches", ROOT), ("plain", ROOT)] + ([("plain_parent", a.parent_tree)] if a.parent_tree else [])
        ms = {k: [] for k, _ in variants}
        for _ in range(a.step_rounds):
            for k, tree in variants:
                cmd = [sys.executable, os.path.abspath(__file__), "--step-case", "patches" if k == "patches" else "plain",
                       "--tree", tree, "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds),
                       "--nimg", str(a.nimg)]
                print("training step: %s" % k, file=sys.stderr, flush=True)
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("step process failed:\n" + r.stderr[-2000:])
                ms[k] += json.loads(r.stdout.strip().splitlines()[-1])["ms"]
        res["training_step"] = dict(
            config="celeba", dtype="bf16x6", denoise_train=True, steps_per_round=a.steps,
            timing="host clock around --steps NoisyTrainer.step() calls, --rounds per process, --step-rounds fresh "
                   "processes per variant, alternating",
            variants={k: dict(ms_per_step_median=round(med(v), 3), ms_per_step_min=round(min(v), 3),
                              ms_per_step_max=round(max(v), 3), rounds=[round(t, 3) for t in v]) for k, v in ms.items()})
        res["training_step"]["patches_over_plain"] = round(med(ms["patches"]) / med(ms["plain"]), 4)
        if a.parent_tree:
            res["training_step"]["plain_over_parent"] = round(med(ms["plain"]) / med(ms["plain_parent"]), 4)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
