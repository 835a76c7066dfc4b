"""Polyak-averaging measurements; prints one JSON line and writes it to profiles/ema_bench.json
(or --out).

The kernel, over the live region of preset celeba's flat parameter buffer (n_live floats), alternating in rounds in
this process, event-timed around --iters enqueues (each launch runs far longer than its enqueue, so the device
time dominates):

  svae_op_ema   one launch of csrc/ema.hip: e -= omd * (e - w)
  torch_lerp    ema.lerp_(params, omd) on the same tensors

The kernel reads both streams and writes one: bytes_moved = 12 * n_live, reported as TB/s against the 6.29 TB/s a
float4 copy reaches on this chip.  A kernel time from a trace (rocprofv3 --kernel-trace --stats -- python
tools/bench_ema.py --profile-case svae_op_ema) can be passed back with --kernel-us.

The training step: --step-processes fresh processes per variant (default 3), alternating, each timing
NoisyTrainer.step() of preset celeba (bf16x6, denoise_train, synthetic data): "on" with ema_decay = 0.999, "off"
without, and with --parent-tree DIR "parent": the same step from a built checkout of the commit before averaging
existed (its own package and library; this file only supplies the loop).  The median of every process and the
range of all rounds are reported; no threshold is set on any figure.
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
COPY_TBS = 6.29  # float4 copy, measured on this chip
OMD = 1.0 - 0.999


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def op_legs():
    import torch
    L = importlib.import_module(PKG + "._lib")
    W = importlib.import_module(PKG + ".weights")
    cfg = importlib.import_module(PKG + ".config").preset("celeba")
    _, n_total, n_live = W.param_table(cfg)
    g = torch.Generator().manual_seed(0)
    w = torch.randn(n_live, generator=g).cuda()
    e = (w + 0.01 * torch.randn(n_live, generator=g).cuda()).contiguous()
    lib, s = L.lib(), L.stream_ptr()

    def op():
        L.check(lib.svae_op_ema(L.ptr(e), L.ptr(w), n_live, OMD, s))

    return n_total, n_live, {"svae_op_ema": op, "torch_lerp": lambda: e.lerp_(w, OMD)}


def step_case(which, steps, warmup, rounds, tree=None):
    """ms per NoisyTrainer.step() with averaging "on" or "off", one round per entry; one JSON line.  ``tree``: import
    the package from that checkout instead of this one."""
    import torch
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    NT = importlib.import_module(PKG + ".trainer").NoisyTrainer
    DD = importlib.import_module(PKG + ".data").DeviceDataset
    cfg = cfgmod.preset("celeba", dtype="bf16x6")
    ds = DD.synthetic(8 * cfg.batch, cfg.height, cfg.width, cfg.channels, seed=3, device="cuda")
    kw = dict(ema_decay=0.999) if which == "on" else {}  # "off" passes nothing: a tree without the option runs it
    t = NT(SV(cfg, seed=0), ds, denoise_train=True, seed=1, **kw)
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-processes", type=int, default=3)
    ap.add_argument("--parent-tree", default=None,
                    help="a built checkout of the commit before averaging: adds the 'parent' step variant")
    ap.add_argument("--tree", default=None, help="(internal) the checkout a --step-case process imports")
    ap.add_argument("--kernel-us", type=float, default=None,
                    help="mean kernel time of ema_kernel from a rocprofv3 --kernel-trace --stats run of --profile-case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    ap.add_argument("--profile-case", default=None, metavar="LEG",
                    help="only run this leg --iters times, nothing timed (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--step-case", default=None, choices=["on", "off"],
                    help="(internal) one process of the training-step comparison")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema needs a GPU")
    if a.step_case:
        return step_case(a.step_case, a.steps, a.warmup, a.rounds, a.tree)
    n_total, n_live, legs = op_legs()
    if a.profile_case:
        for _ in range(a.iters):
            legs[a.profile_case]()
        torch.cuda.synchronize()
        return
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, a.iters))
    med = lambda v: sorted(v)[len(v) // 2]
    nbytes = 12 * n_live
    res = dict(tool="bench_ema", device=torch.cuda.get_device_name(0), config="celeba", n_total=n_total, n_live=n_live,
               omd=OMD, iters=a.iters, bytes_moved=nbytes, copy_rate_tb_per_s=COPY_TBS,
               timing="device events around --iters enqueues, alternating rounds",
               legs={k: dict(us_median=round(med(v), 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                             us_rounds=[round(t, 2) for t in v],
                             tb_per_s=round(nbytes / (med(v) * 1e-6) / 1e12, 3),
                             of_copy_rate=round(nbytes / (med(v) * 1e-6) / 1e12 / COPY_TBS, 3))
                     for k, v in us.items()})
    res["torch_over_op"] = round(med(us["torch_lerp"]) / med(us["svae_op_ema"]), 3)
    if a.kernel_us is not None:
        res["kernel"] = dict(us=a.kernel_us, source="rocprofv3 --kernel-trace --stats, svae_op_ema leg",
                             tb_per_s=round(nbytes / (a.kernel_us * 1e-6) / 1e12, 3))
    variants = ["on", "off"] + (["parent"] if a.parent_tree else [])
    procs = {k: [] for k in variants}
    for _ in range(a.step_processes):
        for which in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--step-case", "off" if which == "parent" else which,
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
            if which == "parent":
                cmd += ["--tree", a.parent_tree]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit("step process failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
            procs[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
    if a.step_processes:
        flat = {k: [t for p in v for t in p] for k, v in procs.items()}
        step = dict(config="celeba", dtype="bf16x6",
                    what="NoisyTrainer.step(), denoise_train, ms per step; one variant per process",
                    processes=procs, median_per_process={k: [med(p) for p in v] for k, v in procs.items()},
                    median_ms={k: med(v) for k, v in flat.items()},
                    range_ms={k: [min(v), max(v)] for k, v in flat.items()},
                    on_minus_off_us=round((med(flat["on"]) - med(flat["off"])) * 1e3, 1))
        if a.parent_tree:
            step["off_minus_parent_us"] = round((med(flat["off"]) - med(flat["parent"])) * 1e3, 1)
        res["training_step"] = step
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
