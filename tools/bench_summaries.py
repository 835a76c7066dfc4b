"""Training-summary measurements; prints one JSON line and writes it to
profiles/summaries_bench.json (or --out).

(a) svae_op_tensor_stats over the celeba parameter table (n_total floats, one segment per tensor) on the
    parameters (no clamp) and on the gradients of a real step (clamp 10): event-timed mean us per call (two
    launches) and bytes/s on the bytes the op must read (4 n_total), against the measured float4 copy rate
    of the device (6.29 TB/s; a copy moves two bytes per byte read, this op reads only).  --profile-only
    launches the same calls untimed, for the per-kernel times of a kernel trace.
(b) the same quantities with torch on the device, timed in the same process in alternating rounds:
    torch._foreach_norm over the per-tensor views for the weight norms; for the gradients a clamp into a
    scratch array, torch._foreach_norm over its views, and whole-array passes for the clipped count, the
    non-finite count and max |g| (per group they would cost more; per tensor, far more).  fp32
    accumulation, not the op's fp64.
(c) a whole ``SequentialVAE.summaries()`` call at celeba, B = 128, T = 8 (it ends in its device -> host
    copy): host clock.
(d) ``train()`` steps of the same network timed in the same rounds, and the share a summary every
    10 steps adds: summaries / (10 x step).
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
L = importlib.import_module(PKG + "._lib")
COPY_TBS = 6.29  # float4 copy, measured on the MI355X


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def row(us, nbytes):
    m = sum(us) / len(us)
    return dict(us_per_call=round(m, 2), us_rounds=[round(v, 2) for v in us], bytes_read=nbytes,
                tb_per_s=round(nbytes / m / 1e6, 3), share_of_copy_rate=round(nbytes / m / 1e6 / COPY_TBS, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="celeba")
    ap.add_argument("--dtype", default="bf16x6")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-only", action="store_true",
                    help="only launch the op --iters times on the parameters and on the gradients, nothing timed "
                         "(for rocprofv3 --kernel-trace --stats -- python tools/bench_summaries.py --profile-only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summaries_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_summaries needs a GPU")
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    cfg = cfgmod.preset(a.config, dtype=a.dtype)
    net = SV(cfg, seed=0)
    x = (torch.rand(cfg.batch, cfg.height, cfg.width, cfg.channels, device="cuda") * 2 - 1).contiguous()
    for _ in range(a.warmup):
        net.train(x, x)
    net.summaries()
    sm = net._summaries
    plan, clip = sm.p_table, float(cfg.clip_grad_value)
    out = torch.empty(plan.n_seg * 8, dtype=torch.float64, device="cuda")
    s = L.stream_ptr()

    def op(buf, c):
        L.check(L.lib().svae_op_tensor_stats(L.ptr(buf), L.ptr(plan.table), plan.n_seg, plan.n_chunks, c,
                                             L.ptr(sm.partials), L.ptr(out), s))

    if a.profile_only:
        for _ in range(a.iters):
            op(net.params, math.inf)
            op(net.grads, clip)
        torch.cuda.synchronize()
        return
    tab = sorted(net.table, key=lambda p: p["offset"])
    views = lambda buf: [buf[p["offset"]:p["offset"] + p["size"]] for p in tab]
    pviews, scratch = views(net.params), torch.empty_like(net.grads)
    sviews = views(scratch)

    def torch_weights():
        return torch._foreach_norm(pviews)

    def torch_grads():
        g = net.grads
        torch.clamp(g, -clip, clip, out=scratch)
        norms = torch._foreach_norm(sviews)
        a_ = g.abs()
        return norms, (a_ > clip).sum(), (~torch.isfinite(g)).sum(), a_.max()

    legs = {
        "op_params": lambda: op(net.params, math.inf),
        "op_grads_clip": lambda: op(net.grads, clip),
        "torch_params_foreach_norm": torch_weights,
        "torch_grads_clamp_norm_counts_max": torch_grads,
    }
    for f in legs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():
            us[k].append(timed(f, a.iters))
    nbytes = 4 * net.n_total
    kernel = {k: row(v, nbytes) for k, v in us.items()}
    kernel["op_over_torch_params"] = round(kernel["op_params"]["us_per_call"] /
                                           kernel["torch_params_foreach_norm"]["us_per_call"], 4)
    kernel["op_over_torch_grads"] = round(kernel["op_grads_clip"]["us_per_call"] /
                                          kernel["torch_grads_clamp_norm_counts_max"]["us_per_call"], 4)

    def clock(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3  # ms

    call_ms, step_ms = [], []
    for _ in range(a.rounds):
        step_ms.append(clock(lambda: net.train(x, x), a.steps))
        call_ms.append(clock(net.summaries, a.steps))
    mean = lambda v: sum(v) / len(v)
    whole = dict(config=a.config, dtype=a.dtype, batch=cfg.batch, mc_steps=cfg.mc_steps,
                 summaries_us_per_call=round(mean(call_ms) * 1e3, 1), summaries_us_rounds=[round(v * 1e3, 1) for v in call_ms],
                 train_step_ms=round(mean(step_ms), 3), train_step_ms_rounds=[round(v, 3) for v in step_ms],
                 summary_freq=10, share_of_step_at_freq_10=round(mean(call_ms) / (10 * mean(step_ms)), 5))
    res = dict(tool="bench_summaries", device=torch.cuda.get_device_name(0), copy_rate_tb_per_s=COPY_TBS,
               n_total=net.n_total, n_tensors=plan.n_seg, n_chunks=plan.n_chunks, chunk=L.STATS_CHUNK,
               iters=a.iters, rounds=a.rounds, kernel=kernel, summaries_call=whole)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
