"""Throughput bench of the Sequential-VAE training step on MI355X.

Metric (BASELINE.json): images/sec + ELBO/img, CelebA 64x64 seq-VAE fwd+bwd at N GPUs.
A step = forward of the unrolled 8-step chain + backward + (N>1: one RCCL all-reduce
of the flat gradient over xGMI) + clip/Adam, on one synthetic [B,64,64,3] batch per
GPU (B=128, weak scaling).  Inputs are resident in HBM before the timed region.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config celeba] [--dump-outputs DIR] [--full]
N>1 is launched by the driver via torch.distributed.run (one rank per GPU).

A plain run does what `value` needs and nothing else: set-up, warm-up, the K timed steps (with the
dominant kernel's event probe inside them, as always), the outputs if --dump-outputs is given, and the
result line.  --full adds every other leg after the timed region: the secondary-kernel probe and its
isolated launches, the other precision modes (bf16_value / parity_value, fp32_value), the fp32 step's
dominant-kernel timing, and the CPU baseline; --no-secondary, --no-cpu-baseline, --no-fp32 and
--no-fp32-mode trim it.
"""
import argparse
import ctypes
import importlib
import json
import math
import os
import sys
import time

# Hardware queues per process, before anything initialises HIP: the engine's three streams plus RCCL's own
# (N > 1) share HIP's default 4 queues, and streams sharing a queue serialise.  Measured with an RCCL process
# group in the process (tools/dist_overhead.py, profiles/r06_d_overhead.txt): 19.30 ms/step at 4 queues,
# 15.48 at 8 (15.54 / 15.50 without a process group: N = 1 is unaffected).  At least 8: the GPU boxes export 4
try:
    _hwq = int(os.environ.get("GPU_MAX_HW_QUEUES", "0"))
except ValueError:
    _hwq = 0
if _hwq < 8:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (no 2:1 sparsity)
# dominant kernel of both steps (profiles/r05_f6_kernel_stats.txt, r05_fbf_kernel_stats.txt: the largest
# total time): the wave-split halo gather gather_x3_kernel (csrc/halo_x3.hip; every forward / input-gradient
# conv with >= 1 channel chunk on the main stream, the critical path) -- on scaled fp16 hi/lo planes in the
# split mode, bf16 in the bf16 mode.  The stride-1 halo weight-GEMM (side stream, wgrad_halo2_kernel) is
# reported as the secondary entry.
DOMINANT_KID = "KID_HALO_X3"
DOMINANT_KID_SPLIT = "KID_HALO_X3"
SECONDARY_KID = "KID_WHALO2_S1"
# PMC summaries (tools/pmc_traffic.py: FETCH_SIZE / WRITE_SIZE passes of the same bench command, calibrated
# FETCH rules) per workload; a workload never borrows another's traffic (LSUN read CelebA's)
PMC_FILES = {
    "celeba/bf16": ["profiles/r05_gbf_pmc_traffic.json", "profiles/r05_fbf_pmc_traffic.json"],
    "celeba/bf16x6": ["profiles/r06_h_pmc_traffic.json", "profiles/r06_g_pmc_traffic.json"],
    "lsun/bf16": ["profiles/r04_final_lsun_pmc_traffic.json", "profiles/r04_v1_lsun_pmc_traffic.json"],
    "lsun/bf16x6": ["profiles/r05_fl6_pmc_traffic.json"],
    "c_pixelvae/bf16": ["profiles/r04_final_pv_pmc_traffic.json", "profiles/r04_v1_pv_pmc_traffic.json"],
    "c_pixelvae/bf16x6": ["profiles/r06_gpv_pmc_traffic.json", "profiles/r05_gpv_pmc_traffic.json"],
}


# metric / workload per preset (BASELINE.json configs[1] is the headline: CelebA B=128)
METRIC = {
    "celeba": ("images/sec (CelebA 64x64 seq-VAE fwd+bwd+Adam step)",
               "CelebA 64x64 default seq-VAE (c_inhomog), T=8 chain, fwd+bwd+clip+Adam"),
    "lsun": ("images/sec (LSUN-bedroom 64x64 seq-VAE fwd+bwd+Adam step)",
             "LSUN-bedroom 64x64 seq-VAE (sequential_vae_lsun, latent 110), T=8 chain, fwd+bwd+clip+Adam"),
    "mnist_1step": ("images/sec (MNIST 32x32 1-step seq-VAE fwd+bwd+Adam step)",
                    "MNIST 1-step seq-VAE (m_* geometry, latent 24), fwd+bwd+clip+Adam"),
    "c_pixelvae": ("images/sec (CelebA 64x64 seq-VAE + PixelCNN++ decoder, c_pixelvae, fwd+bwd+Adam step)",
                   "c_pixelvae (sequential_vae.py:529-543): T=2 shared theta/phi, step 0 ladder, step 1 PixelCNN++ "
                   "head (nr_resnet 3, 160 filters, 10 mixtures, dropout 0.3), fwd+bwd+clip+Adam+EMA"),
}


def conv_flops_per_img(cfg):
    """Algorithmic fwd MACs per image of the executed graph (SURVEY §8a totals), x3 for
    fwd+dgrad+wgrad, x2 FLOP/MAC."""
    F, S, L, T = cfg.filter_sizes, cfg.image_sizes, cfg.levels, cfg.mc_steps
    C = cfg.channels

    def conv(cin, cout, hout):
        return 16 * cin * cout * hout * hout

    def convt(cin, cout, hin, s):
        return 16 * cin * cout * hin * hin  # every input pixel scatters to 16 taps (4x4 kernel)

    inf = 0
    cin = F[0]
    for lvl in range(L - 1):
        inf += conv(cin, F[lvl + 1], S[lvl + 1]) + conv(F[lvl + 1], F[lvl + 1], S[lvl + 1])
        inf += 2 * S[lvl + 1] ** 2 * F[lvl + 1] * cfg.latent_dims[lvl]
        cin = F[lvl + 1]
    inf += 2 * S[L - 1] ** 2 * F[L - 1] * cfg.latent_dims[L - 1]
    enc = 0
    cin = F[0]
    for lvl in range(L - 1):
        enc += conv(cin, F[lvl + 1], S[lvl + 1]) + conv(F[lvl + 1], F[lvl + 1], S[lvl + 1])
        cin = F[lvl + 1]
    enc += conv(F[L - 1], F[L - 1], S[L]) + S[L] ** 2 * F[L - 1] * F[L]
    dec = 0
    split = sum(cfg.latent_dims[i] * S[i + 1] ** 2 * F[i + 1] for i in range(L - 1)) + cfg.latent_dims[L - 1] * F[L + 1]
    cin = F[L]
    for lvl in range(L - 2, -1, -1):
        dec += convt(cin, F[lvl + 1], S[lvl + 2], 2) + convt(2 * F[lvl + 1], F[lvl + 1], S[lvl + 1], 1)
        cin = F[lvl + 1]
    out0 = convt(F[1], C, S[1], 2)
    ratio = convt(F[1], 1, S[1], 2)
    top0 = F[L + 1] * S[L] ** 2 * F[L]
    top = (F[L + 1] + F[L]) * S[L] ** 2 * F[L]
    macs = T * (inf + dec + split + out0) + (T - 1) * (enc + ratio) + top0 + (T - 1) * top
    return 3 * 2 * macs


def dominant_kernel_shape(cfg):
    """Decoder level-0 stride-1 conv-T (32x32, 2F1->F1): the largest single launch of
    the forward (37% of MACs are the three decoder s1 layers)."""
    F, S = cfg.filter_sizes, cfg.image_sizes
    return dict(n=cfg.batch, h=S[1], cin=2 * F[1], cout=F[1], stride=1, transpose=1)


def time_dominant_kernel(L, shape, iters=50):
    """Average duration of the dominant kernel launch (HIP events on the launch stream)."""
    n, h, cin, cout = shape["n"], shape["h"], shape["cin"], shape["cout"]
    x = torch.randn(n, h, h, cin, device="cuda")
    w = torch.randn(4, 4, cout, cin, device="cuda") * 0.02
    y = torch.empty(n, h, h, cout, device="cuda")
    st = L.stream_ptr()
    for _ in range(5):
        L.check(L.lib().svae_op_conv(L.ptr(x), n, h, cin, L.ptr(w), cout, 1, 1, L.ptr(y), st))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        L.check(L.lib().svae_op_conv(L.ptr(x), n, h, cin, L.ptr(w), cout, 1, 1, L.ptr(y), st))
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) / 1000.0 / iters
    flops = 2.0 * n * h * h * cout * 16 * cin
    return sec, flops


def isolated_wgrad(L, cfg, iters=20):
    """The dominant kernel's launches of one step, each timed alone on an idle GPU (HIP events,
    svae_op_wgrad_bf16 with the step's operand storage): the stride-1 halo weight-GEMMs of the
    decoder s1 conv-Ts (dY bf16, input = the fp32 concat), the encoder b convs (both bf16) and the
    T-batched recognition b convs (both bf16; one launch of T*B images).  In the step these run on
    the side stream concurrently with the main stream's kernels, which is why the live average is
    higher: this separates the kernel's own speed from that sharing."""
    F, S, T, B = cfg.filter_sizes, cfg.image_sizes, cfg.mc_steps, cfg.batch
    shapes = []  # (n, h, cin, cout, transpose, x_bf16, dy_bf16, launches per step)
    for lvl in range(cfg.levels - 1):
        Fl, h = F[lvl + 1], S[lvl + 1]
        shapes.append((B, h, 2 * Fl, Fl, 1, 0, 1, T))
        shapes.append((B, h, Fl, Fl, 0, 1, 1, T - 1))
        shapes.append((T * B, h, Fl, Fl, 0, 1, 1, 1))
    scratch = torch.empty(64 << 20, device="cuda")
    tot_t = tot_f = 0.0
    n_launch = 0
    for (n, h, cin, cout, tr, xb, db, cnt) in shapes:
        if cnt < 1:
            continue
        x = torch.randn(n, h, h, cin, device="cuda").to(torch.bfloat16 if xb else torch.float32)
        dy = (torch.randn(n, h, h, cout, device="cuda") * 0.1).to(torch.bfloat16 if db else torch.float32)
        dw = torch.empty(16 * cin * cout, device="cuda")
        path = 2 | (16 if xb else 0) | (32 if db else 0)
        args = (ctypes.c_void_p(x.data_ptr()), n, h, cin, ctypes.c_void_p(dy.data_ptr()), cout, 1, tr, path,
                L.ptr(dw), L.ptr(scratch), scratch.numel() * 4, L.stream_ptr())
        L.check(L.lib().svae_op_wgrad_bf16(*args))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            L.lib().svae_op_wgrad_bf16(*args)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters  # kernel + its split reduce, as launched by the engine
        tot_t += us * cnt
        tot_f += 2.0 * 16 * cin * cout * n * h * h * cnt
        n_launch += cnt
    ach = tot_f / (tot_t * 1e-6) / 1e12
    return dict(achieved=round(ach, 3), frac=round(ach / BF16_MFMA_PEAK_TFLOPS, 5),
                avg_launch_us=round(tot_t / n_launch, 2), launches=n_launch,
                method="each of the step's launches alone on the idle GPU (svae_op_wgrad_bf16, split reduce "
                       "included), same shapes and operand storage; the live figure above is the in-step one")


def pmc_traffic(kernel, key="celeba/bf16"):
    """HBM bytes per launch of `kernel` (a family: every template instance whose name starts with
    the kernel's base name, weighted by dispatch count) from the committed PMC summary of this
    workload (`key` = config/dtype; tools/pmc_traffic.py: separate FETCH_SIZE / WRITE_SIZE rocprofv3
    passes of the bench command, the gfx950 FETCH correction per kernel as recorded there), or
    (None, None) when that workload has none."""
    bases = [k.strip().split("<")[0].split(" ")[0] for k in kernel.split(" + ")]  # "a + b": both families
    paths = [os.path.join(ROOT, p) for p in PMC_FILES.get(key, [])]
    for path in paths:
        try:
            with open(path) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        tot = n = 0
        for k, v in d.get("kernels", {}).items():
            if "wgrad_halo2_kernel" in bases and "<" in k:  # the stride-1 instances (last template argument S)
                targs = k[k.index("<") + 1:k.rindex(">")].split(",")
                if len(targs) >= 10 and targs[9].strip() != "1":
                    continue
            if k.split("<")[0] in bases and v.get("hbm_bytes_per_launch"):
                tot += v["hbm_bytes_per_launch"] * v["dispatches_fetch_pass"]
                n += v["dispatches_fetch_pass"]
        if n:
            return float(tot) / n, os.path.relpath(path, ROOT)
    return None, None


DUMP_BUDGET = 64 << 20  # bytes of --dump-outputs, all files together


def dump_outputs(dirname, arrays, seed=0):
    """--dump-outputs: write each array of `arrays` (name -> ndarray) as <dirname>/<name>.npy, float64 where it
    is float64 and float32 otherwise, DUMP_BUDGET bytes at the most in all.  Arrays are taken smallest first and
    each may use an equal share of what is left, so small ones are whole; a larger one becomes a 1-D sample of
    its flattened elements at fixed indices (sorted draws of default_rng(seed): the same for every run and
    build of the same shapes)."""
    os.makedirs(dirname, exist_ok=True)
    left = DUMP_BUDGET - 1024 * len(arrays)  # the .npy headers
    todo = sorted(arrays.items(), key=lambda kv: kv[1].size * kv[1].dtype.itemsize)
    for i, (name, a) in enumerate(todo):
        a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
        cap = left // (len(todo) - i) // a.dtype.itemsize
        if a.size > cap:
            idx = np.unique(np.random.default_rng(seed).integers(0, a.size, cap))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)
        left -= a.size * a.dtype.itemsize


def _cpu_threads():
    """Host threads for the CPU baseline: the physical cores this process may use, capped by the
    box's CPU share (OMP_NUM_THREADS, set to 16 on the GPU boxes)."""
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or os.cpu_count() or 1
    except ImportError:
        phys = os.cpu_count() or 1
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else phys
    n = min(phys, avail)
    share = os.environ.get("OMP_NUM_THREADS")
    if share and share.isdigit() and int(share) > 0:
        n = min(n, int(share))
    return max(1, n), phys, avail


def cpu_baseline(cfg, cfgname, target_sec=20.0, max_steps=3):
    """PyTorch-CPU fp32 restatement of the same graph (oracle/torch_twin.py) at the workload's
    own batch (B=128 for CelebA, T=8), fwd+bwd, on a bounded sample of steps."""
    from oracle import spec, torch_twin
    threads, phys, avail = _cpu_threads()
    torch.set_num_threads(threads)
    B = cfg.batch
    cd = spec.make_config(cfgname, batch=B)
    _, struct, params = spec.init_params(cd, seed=0, dtype=np.float32)
    x, tgt, eps = spec.make_inputs(cd, batch=B)
    tw = torch_twin.Twin(cd, struct, params, dtype=torch.float32)
    # warm-up (oneDNN primitive creation) on a small slice of the same batch
    cw = spec.make_config(cfgname, batch=8)
    torch_twin.Twin(cw, struct, params, dtype=torch.float32).step(x[:8], tgt[:8], eps[:, :8], 1.0)
    t0 = time.time()
    n = 0
    while n < max_steps and (n == 0 or (time.time() - t0) < target_sec):
        tw.step(x, tgt, eps, 1.0)
        n += 1
    dt = (time.time() - t0) / n
    return dict(value=B / dt, unit="images/sec", cores=threads, kind="port",
                sample="%d fwd+bwd step(s) of the full B=%d %s batch (T=%d) with oracle/torch_twin.py fp32 on "
                       "%d threads (host: %d physical cores, %d in this process's affinity; the box's CPU share "
                       "OMP_NUM_THREADS=%s)" % (n, B, cfgname, cd["mc_steps"], threads, phys, avail,
                                                os.environ.get("OMP_NUM_THREADS", "unset")))


def mode_throughput(cfg, SV, dtype, steps=10, warmup=3, probe_kid=None, probe_launches=96):
    """images/sec of the same training step in another precision mode: "fp32" (fp32 MFMA) or
    "bf16x6" (split-bf16 MFMA, the fp32-accurate mode held to the fp32 parity bounds in
    tests/test_headline_gpu.py).  probe_kid: the first probe_launches launches of that kernel family
    inside the timed steps are bracketed by HIP event pairs (svae_probe_begin); returns
    (images/s, ms/step, probe dict or None)."""
    from dataclasses import replace
    L = importlib.import_module(PKG + "._lib")
    c32 = replace(cfg, dtype=dtype)
    net = SV(c32, seed=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    lo, hi = c32.range
    x = (torch.rand(c32.batch, c32.height, c32.width, c32.channels, device="cuda", generator=g) * (hi - lo) + lo)
    for it in range(1, warmup + steps + 1):
        if it == warmup + 1:
            torch.cuda.synchronize()
            if probe_kid is not None:
                L.check(L.lib().svae_probe_begin(net.ctx, probe_kid, probe_launches), net.ctx)
            t0 = time.perf_counter()
        net.forward(x, x, None, 1.0 - math.exp(-it / c32.reg_coeff_rate))
        net.backward_apply(c32.learning_rate, it)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    probe = None
    if probe_kid is not None:
        n, nt = ctypes.c_int64(), ctypes.c_int64()
        fl, ms_k = ctypes.c_double(), ctypes.c_double()
        L.check(L.lib().svae_probe_end(net.ctx, ctypes.byref(n), ctypes.byref(nt), ctypes.byref(fl),
                                       ctypes.byref(ms_k)), net.ctx)
        if nt.value > 0:
            probe = dict(kernel=L.lib().svae_kernel_name(probe_kid).decode(), launches_per_step=n.value / steps,
                         timed=nt.value, flops=fl.value, ms=ms_k.value)
    net.close()
    return c32.batch * steps / dt, dt / steps * 1e3, probe


def _pv_throughput(PV, B, dtype, steps, warmup, probe_cap):
    """Time `steps` c_pixelvae training steps in `dtype` (the head in its split mode for "bf16x6" / "fp32",
    bf16 MFMA for "bf16"): (images/sec, ms/step, forward-conv probe, elbo, head conv FLOPs per step, pv)."""
    pv = PV("c_pixelvae", batch_size=B, dtype=dtype)
    c = pv.cfg
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    x = (torch.rand(B, c.height, c.width, c.channels, device="cuda", generator=g) * 2 - 1).contiguous()
    for _ in range(warmup):
        pv.train(x, x)
    torch.cuda.synchronize()
    pv.head.probe, pv.head.probe_cap = [], probe_cap
    pv.head.conv_flops = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        pv.train(x, x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    probe, pv.head.probe = pv.head.probe, None
    head_flops = 3.0 * pv.head.conv_flops / steps  # forward + input gradient + weight gradient
    return B * steps / dt, dt / steps * 1e3, probe, pv.loss_value(), head_flops, pv, x


def _pv_roofline(probe, planes, head_flops, vae_flops, ms, key):
    """The head's forward convolutions (event pairs around each probed launch): algorithmic FLOPs per
    second; in the split mode one algorithmic conv is 3 fp16 plane products in one launch (issued = 3 x achieved;
    6 bf16 ones where channels % 8 != 0)."""
    pflops = sum(f for f, _, _, _ in probe)
    iflops = sum(f * k for f, _, _, k in probe)  # the MFMA work the plane products really run
    pms = sum(e0.elapsed_time(e1) for _, e0, e1, _ in probe)
    if pms <= 0:
        return None
    ach = pflops / (pms / 1e3) / 1e12
    kern = "pc_conv3r_kernel + pc_conv3_kernel + pc_conv2_kernel"
    traffic, tsrc = pmc_traffic(kern, key)
    return {"bound": "mfma", "achieved": round(ach, 3), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / BF16_MFMA_PEAK_TFLOPS, 5), "traffic": traffic, "traffic_source": tsrc,
            "traffic_unit": "HBM bytes per launch (PMC, family average)",
            "kernel": kern + " (PixelCNN++ head forward convolutions, all instances%s)"
                      % (", split mode: 3 fp16 plane products per conv (6 bf16 ones where channels % 8 != 0)"
                         if planes > 1 else ""),
            "issued": round(ach * iflops / pflops, 3), "frac_issued": round(ach * iflops / pflops / BF16_MFMA_PEAK_TFLOPS, 5),
            "timed_convs": len(probe), "avg_conv_us": round(pms * 1e3 / max(1, len(probe)), 2),
            "step_achieved_tflops": round((head_flops + vae_flops) / (ms / 1e3) / 1e12, 3),
            "step_achieved_method": "estimated: head FLOPs = 3 x forward convolution FLOPs"}


def pixelvae_cpu_baseline(pv, x, c, nb):
    """The same c_pixelvae training step (both chain steps, the head's training pass WITH dropout 0.3, the
    mixture draw, highway, 16 MSE + KL, backward through everything) in fp32 torch on the host cores:
    oracle/pixelvae.py at dtype float32 -- the fp32 counterpart of the fp32-grade split step, on a batch
    sample of nb images (the timing is per image; one untimed step first, then steps until >= 10 s)."""
    from oracle import pcnn as opc, pixelvae as opv, spec as ospec_mod
    threads, phys, avail = _cpu_threads()
    torch.set_num_threads(threads)
    cd = ospec_mod.make_config("celeba", batch=nb, mc_steps=2, latent_dims=list(c.latent_dims),
                               filter_sizes=list(c.filter_sizes), latent_mean_clip=c.latent_mean_clip,
                               min_highway=c.min_highway, max_highway=c.max_highway, regularized_steps=(0,),
                               first_step_loss_coeff=c.first_step_loss_coeff)
    cd["share_theta"] = cd["share_phi"] = True
    hs = opc.make_spec(H=64, W=64, K=c.latent_dim)
    rng = np.random.default_rng(7)
    xs = x[:nb].cpu().numpy()
    eps = rng.standard_normal((2, nb, c.latent_dim)).astype(np.float32)
    um = rng.uniform(1e-5, 1 - 1e-5, (nb, 64, 64, hs["M"])).astype(np.float32)
    ul = rng.uniform(1e-5, 1 - 1e-5, (nb, 64, 64, 3)).astype(np.float32)
    keep = 0.7  # dropout_p 0.3 (pixelvae.py:54-63) in every gated resnet: one keep-mask per resnet, in call order
    R, F = hs["R"], hs["F"]
    res = [64] * (2 * R) + [32] * (2 * R) + [16] * (2 * R) + [16] * (2 * R) + [32] * (2 * R + 2) + [64] * (2 * R + 2)
    masks = [(rng.uniform(size=(nb, r, r, F)) < keep).astype(np.float32) / keep for r in res]
    pub, hp = pv.vae.param_dict(), pv.head.params()
    run = lambda: opv.forward_backward(cd, pub, hs, hp, xs, xs, eps, 1.0, um, ul, masks, bf16_head=False,
                                       dtype=torch.float32)
    run()
    n, t0 = 0, time.perf_counter()
    while True:
        run()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= 10.0 or n >= 20:
            break
    return dict(value=round(nb * n / dt, 4), unit="images/sec", cores=threads, kind="port",
                sample="%d fwd+bwd steps of %d images of the c_pixelvae chain (oracle/pixelvae.py in fp32 torch CPU, "
                       "dropout 0.3 on, 1 untimed step first) on %d threads (host: %d physical cores)"
                       % (n, nb, threads, phys))


def run_pixelvae(args, cfgmod):
    """BASELINE configs[4] (CelebA + pixel_cnn decoder, 1 GPU): the c_pixelvae training step
    (pixelvae.PixelVAE.train: engine forward, head training pass with dropout, sampler + highway,
    both backwards, Adam + Polyak EMA) on a synthetic batch resident in HBM.  `value` is the
    --dtype step (default bf16x6: the engine's split mode and the head's 3-plane split mode, the
    fp32-grade step of tests/test_pixelvae_gpu.py); the bf16 step is reported beside it.  The
    roofline entry is the head's forward convolution kernels (pc_conv3_kernel for the stride-1 halo
    convs, pc_conv2_kernel for the rest: every forward convolution of the head, timed live by event
    pairs around its first --probe-launches convolutions inside the timed region).  The per-step head
    FLOPs (and so step_achieved_tflops) are ESTIMATED as 3x the forward convolution FLOPs (forward +
    input gradient + weight gradient); only the forward launches are timed."""
    PV = importlib.import_module(PKG + ".pixelvae").PixelVAE
    torch.manual_seed(1234)  # the sampler's uniforms and the dropout seeds come from torch's generators
    B = args.batch or 128
    dtype = args.dtype
    cap = args.probe_launches or 96
    value, ms, probe, elbo, head_flops, pv, x = _pv_throughput(PV, B, dtype, args.steps, args.warmup, cap)
    c = pv.cfg
    planes = pv.head.planes
    if args.dump_outputs:  # the last timed step: its loss and reconstruction, the parameters it left
        dump_outputs(args.dump_outputs, {
            "loss": np.array([pv.loss_value()], np.float64), "xhat": pv.xhat(pv.e).cpu().numpy(),
            "params": pv.vae.params.cpu().numpy(), "head_params": pv.head.P.cpu().numpy()})
    vae_flops = conv_flops_per_img(c) * B  # the engine's part (both steps' recognition + step 0 ladder)
    alt = "bf16" if dtype != "bf16" else "bf16x6"
    alt_value = alt_ms = alt_roof = None
    if not args.no_secondary:
        pv.close()
        del pv
        torch.cuda.empty_cache()
        av, am, ap_, _, ahf, apv, _ = _pv_throughput(PV, B, alt, args.parity_steps, 2, cap)
        alt_value, alt_ms = av, am
        alt_roof = _pv_roofline(ap_, apv.head.planes, ahf, vae_flops, am, "c_pixelvae/" + alt)
        apv.close()
        del apv
        torch.cuda.empty_cache()
        pv = PV("c_pixelvae", batch_size=B, dtype=dtype)  # (for the CPU baseline's parameters)
    parity = dtype != "bf16"
    line = {
        "metric": METRIC["c_pixelvae"][0], "value": round(value, 2), "unit": "images/sec", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": dtype + (" engine, split head (scaled fp16 hi/lo planes: 3 fp16-MFMA products per GEMM)" if planes > 1
                          else " engine, bf16-MFMA head"),
        "data": "synthetic U[-1,1] NHWC batch, target=input, eps / sampler uniforms / dropout masks on device",
        "config": {"workload": METRIC["c_pixelvae"][1], "model": "c_pixelvae", "global_batch": B, "per_gpu_batch": B,
                   "image": [c.height, c.width, c.channels], "mc_steps": c.mc_steps, "parallelism": "dp1"},
        "elbo_per_img": round(elbo, 5),
        "full": args.full, "dump_outputs": args.dump_outputs,
        "parity": parity,
        "parity_value": round(value, 2) if parity else (None if alt_value is None else round(alt_value, 2)),
        "parity_ms_per_step": round(ms, 3) if parity else (None if alt_ms is None else round(alt_ms, 3)),
        "parity_dtype": dtype if parity else (alt if alt_value is not None else None),
        "parity_roofline": None if parity else alt_roof,
        "bf16_value": None if alt != "bf16" or alt_value is None else round(alt_value, 2),
        "bf16_ms_per_step": None if alt != "bf16" or alt_ms is None else round(alt_ms, 3),
        "bf16_roofline": alt_roof if alt == "bf16" else None,
        "head_conv_tflop_per_step": round(head_flops / 1e12, 3),
        "head_conv_tflop_method": "estimated: 3 x the counted forward convolution FLOPs (fwd + dgrad + wgrad)",
        "roofline": _pv_roofline(probe, planes, head_flops, vae_flops, ms, "c_pixelvae/" + dtype),
        "cpu_baseline": None,
    }
    if not args.no_cpu_baseline:
        line["cpu_baseline"] = pixelvae_cpu_baseline(pv, x, c, args.cpu_batch)
    print(json.dumps(line), flush=True)
    pv.close()


def _spawn_ranks(n):
    """--gpus N without a torch.distributed launcher: start N ranks as child processes (nothing
    here has touched the GPU yet) and exit with their status."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--warmup-seconds", type=float, default=1.0,
                    help="after the --warmup steps, more untimed steps until this much warm-up has run (0: off); "
                         "--steps and what is timed are unchanged")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run every other leg (secondary-kernel probe, other precision "
                         "modes, the fp32 step's dominant-kernel timing, CPU baseline); a plain run has none of them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (loss, per-step statistics, "
                         "per-image ELBO, the final reconstruction, the updated parameters) as DIR/<name>.npy, 64 MB "
                         "at the most (a fixed sample of a larger array).  The step count must not depend on the "
                         "clock, so the time-based warm-up is off: exactly --warmup steps run before the timed ones")
    ap.add_argument("--config", default="celeba")
    ap.add_argument("--batch", type=int, default=None)
    # bf16x6 (split-bf16 MFMA, held to the fp32 parity bounds in tests/test_headline_gpu.py) is the
    # headline: `value` is a parity-grade step.  The plain bf16 step is reported beside it (bf16_value)
    ap.add_argument("--dtype", default="bf16x6", choices=["bf16", "fp32", "bf16x6"])
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="N>1 process group: nccl (= RCCL, one rank per GPU; the default) or gloo (a CPU test of the "
                         "multi-rank path, e.g. several ranks sharing one GPU, where RCCL refuses)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip every leg after the timed region (secondary kernel probe, other precision modes)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=8, help="c_pixelvae: images per CPU-baseline step (a sample)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N>1: one all-reduce after the backward instead of per-step buckets during it")
    ap.add_argument("--no-fp32", action="store_true",
                    help="skip the other-mode throughputs (bf16_value / parity_value, fp32_value)")
    ap.add_argument("--no-fp32-mode", action="store_true",
                    help="skip only the fp32-MFMA throughput (fp32_value)")
    ap.add_argument("--parity-steps", type=int, default=10, help="timed steps of the other-mode throughputs")
    ap.add_argument("--probe-launches", type=int, default=96,
                    help="dominant-kernel launches timed with HIP event pairs inside the timed region (the first N; "
                         "0 = every launch). Each pair is two event records on the kernel's stream, so timing all "
                         "~1000 launches of a 20-step run costs the step itself ~2 %%")
    return ap


def init_distributed(args, world, local):
    """The N>1 process group: RCCL (backend "nccl", one rank per GPU) unless --dist-backend gloo;
    returns torch.distributed, or None at N=1."""
    if world <= 1:
        return None
    import torch.distributed as dist
    if args.dist_backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group("gloo")
    return dist


def main():
    args = make_parser().parse_args()
    if not args.full:  # a plain run: the timed steps and nothing after them
        args.no_secondary = args.no_cpu_baseline = True
    if args.dump_outputs:  # the same steps on the same inputs in every run
        args.warmup_seconds = 0.0

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(_spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d (launch one rank per GPU)" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()  # (does not initialise the GPU)
    if args.dist_backend == "nccl" and world > 1 and local >= ndev:
        sys.exit("bench.py: rank %d has no GPU of its own (%d visible); RCCL needs one rank per GPU "
                 "(--dist-backend gloo tests the multi-rank path on fewer GPUs)" % (local, ndev))
    local = local % max(1, ndev)
    torch.cuda.set_device(local)
    if os.environ.get("SVAE_BENCH_STREAM") == "1":  # A/B: run on a non-default torch stream
        torch.cuda.set_stream(torch.cuda.Stream(local))
    dist = init_distributed(args, world, local)

    cfgmod = importlib.import_module(PKG + ".config")
    if args.config == "c_pixelvae":
        if world != 1:
            sys.exit("bench.py: --config c_pixelvae is the 1-GPU configuration (BASELINE configs[4])")
        run_pixelvae(args, cfgmod)
        return
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    par = importlib.import_module(PKG + ".parallel")
    L = importlib.import_module(PKG + "._lib")
    over = {"dtype": args.dtype}
    if args.batch:
        over["batch"] = args.batch
    cfg = cfgmod.preset(args.config, **over)
    cfgname = cfgmod.NETNAMES.get(args.config, args.config)
    B = cfg.batch
    overlap = world > 1 and not args.no_overlap
    hook = par.allreduce_hook(dist) if world > 1 and not overlap else None
    net = SV(cfg, seed=0, grad_hook=hook)
    if overlap:  # per-step gradient buckets all-reduced (RCCL) while the earlier steps' backward runs
        net.enable_overlapped_allreduce(dist)

    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + rank)
    lo, hi = cfg.range
    x = (torch.rand(B, cfg.height, cfg.width, cfg.channels, device="cuda", generator=g) * (hi - lo) + lo).contiguous()
    tgt = x

    def step(it):
        reg = 1.0 - math.exp(-it / cfg.reg_coeff_rate)
        net.forward(x, tgt, None, reg)
        net.backward_apply(cfg.learning_rate, it)  # backward + clip/Adam per chain-step bucket

    probe_kid = getattr(L, DOMINANT_KID if args.dtype == "bf16" else DOMINANT_KID_SPLIT) if args.dtype in ("bf16", "bf16x6") else None
    it = 0
    tw = time.perf_counter()
    for _ in range(args.warmup):
        it += 1
        step(it)
    torch.cuda.synchronize()
    # time-based warm-up: keep stepping until --warmup-seconds of warm-up have run, so the
    # clock and caches settle before the timed region; every rank runs the same count (each step all-reduces)
    # (rounds of steps sized from the last round's per-step time -- the first steps run slower -- until the
    # target is reached; each round's count is the MAX over ranks)
    per = (time.perf_counter() - tw) / max(1, args.warmup)
    extra = 0
    for _round in range(8):
        wdt = time.perf_counter() - tw
        need = max(0, int(math.ceil((args.warmup_seconds - wdt) / max(per, 1e-4)))) if args.warmup_seconds > 0 else 0
        if dist:
            te = torch.tensor([need], device="cuda", dtype=torch.int64)
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            need = int(te.item())
        if need == 0:
            break
        t0r = time.perf_counter()
        for _ in range(need):
            it += 1
            step(it)
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0r) / need
        extra += need
    warm_s = time.perf_counter() - tw
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    if probe_kid is not None and rank == 0:  # event pairs around every launch of the dominant kernel
        cap = args.probe_launches if args.probe_launches > 0 else 400 * args.steps
        L.check(L.lib().svae_probe_begin(net.ctx, probe_kid, cap), net.ctx)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        it += 1
        step(it)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:  # the last timed step, before any later leg steps again
        dump_outputs(args.dump_outputs, {
            "loss": np.array([net.loss_value()], np.float64), "step_stats": net.step_stats().cpu().numpy(),
            "elbo_per_image": net.elbo_per_image().cpu().numpy(), "xhat": net.xhat(-1).cpu().numpy(),
            "params": net.params.cpu().numpy()})
    probe = None
    if probe_kid is not None and rank == 0:
        n, nt = ctypes.c_int64(), ctypes.c_int64()
        fl, ms_k = ctypes.c_double(), ctypes.c_double()
        L.check(L.lib().svae_probe_end(net.ctx, ctypes.byref(n), ctypes.byref(nt), ctypes.byref(fl),
                                       ctypes.byref(ms_k)), net.ctx)
        probe = dict(kernel=L.lib().svae_kernel_name(probe_kid).decode(), launches=n.value, timed=nt.value,
                     flops=fl.value, ms=ms_k.value)
    probe2 = None
    if probe_kid is not None and rank == 0 and world == 1 and not args.no_secondary:
        # secondary kernel (the side stream's weight-GEMM): two more steps with its launches timed,
        # after the timed region (not part of `value`)
        kid2 = getattr(L, SECONDARY_KID)
        L.check(L.lib().svae_probe_begin(net.ctx, kid2, args.probe_launches or 96), net.ctx)
        for _ in range(2):
            it += 1
            step(it)
        torch.cuda.synchronize()
        n, nt = ctypes.c_int64(), ctypes.c_int64()
        fl, ms_k = ctypes.c_double(), ctypes.c_double()
        L.check(L.lib().svae_probe_end(net.ctx, ctypes.byref(n), ctypes.byref(nt), ctypes.byref(fl),
                                       ctypes.byref(ms_k)), net.ctx)
        if nt.value > 0:
            ach2 = fl.value / (ms_k.value / 1e3) / 1e12
            tr2, tsrc2 = pmc_traffic(L.lib().svae_kernel_name(kid2).decode(), args.config + "/" + args.dtype)
            probe2 = dict(kernel=L.lib().svae_kernel_name(kid2).decode(), achieved=round(ach2, 3),
                          frac=round(ach2 / BF16_MFMA_PEAK_TFLOPS, 5), launches_per_step=n.value / 2,
                          avg_launch_us=round(ms_k.value * 1e3 / nt.value, 2), timed_launches=nt.value,
                          flops_per_launch=round(fl.value / nt.value), traffic=tr2, traffic_source=tsrc2,
                          method="2 steps after the timed region, HIP event pairs on the side stream")
    elbo = net.loss_value()
    if dist:
        t = torch.tensor([elapsed], device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        e = torch.tensor([elbo], device="cuda", dtype=torch.float64)
        dist.all_reduce(e, op=dist.ReduceOp.SUM)
        elbo = float(e.item()) / world

    ms = elapsed / args.steps * 1000.0
    value = world * B * args.steps / elapsed
    flops_img = conv_flops_per_img(cfg)

    roof = None
    cpu = None
    nprod = 3 if args.dtype == "bf16x6" else 1  # MFMAs issued per useful one (fp16 hi/lo planes: three products)
    if rank == 0 and probe is not None and probe["timed"] > 0:
        # dominant kernel, timed live in the timed region: sum of per-launch algorithmic FLOPs
        # (2*taps*M*N*pixels) / sum of per-launch event durations
        ach = probe["flops"] / (probe["ms"] / 1e3) / 1e12
        avg_us = probe["ms"] * 1e3 / probe["timed"]
        traffic, tsrc = pmc_traffic(probe["kernel"], args.config + "/" + args.dtype)
        roof = dict(bound="mfma", achieved=round(ach, 3), peak=BF16_MFMA_PEAK_TFLOPS, unit="TFLOP/s",
                    frac=round(ach / BF16_MFMA_PEAK_TFLOPS, 5), traffic=traffic,
                    kernel=probe["kernel"] + (" (scaled fp16 hi/lo planes: 3 MFMAs per fragment pair)" if nprod > 1 else ""),
                    launches_per_step=probe["launches"] / args.steps,
                    avg_launch_us=round(avg_us, 2), timed_launches=probe["timed"],
                    flops_per_launch=round(probe["flops"] / probe["timed"]),
                    traffic_source=tsrc,
                    step_achieved_tflops=round(flops_img * value / world / 1e12, 3),
                    step_frac=round(flops_img * value / world / 1e12 / BF16_MFMA_PEAK_TFLOPS, 5))
        if nprod > 1:  # the MFMA work the plane products really run
            roof["issued"] = round(nprod * ach, 3)
            roof["frac_issued"] = round(nprod * ach / BF16_MFMA_PEAK_TFLOPS, 5)
    elif rank == 0 and args.full:
        shape = dominant_kernel_shape(cfg)
        sec, kflops = time_dominant_kernel(L, shape)
        ach = kflops / sec / 1e12
        roof = dict(bound="mfma", achieved=round(ach, 3), peak=FP32_MFMA_PEAK_TFLOPS, unit="TFLOP/s",
                    frac=round(ach / FP32_MFMA_PEAK_TFLOPS, 4), traffic=None,
                    kernel="igemm_fwd_kernel<256,32,4,1,NK> decoder level-0 conv-T s1 %s" % (
                        "x".join(str(shape[k]) for k in ("n", "h", "cin", "cout"))),
                    kernel_us=round(sec * 1e6, 2),
                    step_achieved_tflops=round(flops_img * value / world / 1e12, 3))
    if rank == 0 and roof is not None and probe2 is not None:
        probe2["isolated"] = isolated_wgrad(L, cfg) if args.dtype == "bf16" else None
        roof["secondary"] = probe2
    fp32_value = fp32_ms = alt_value = alt_ms = alt_roof = None
    alt = "bf16" if args.dtype == "bf16x6" else "bf16x6"  # the other bf16-MFMA mode, timed after the region
    if world == 1 and args.dtype in ("bf16", "bf16x6") and not args.no_fp32 and not args.no_secondary:
        net.close()
        alt_value, alt_ms, alt_probe = mode_throughput(cfg, SV, alt, steps=args.parity_steps,
                                                       probe_kid=getattr(L, DOMINANT_KID if alt == "bf16" else DOMINANT_KID_SPLIT),
                                                       probe_launches=args.probe_launches or 96)
        if alt_probe is not None:  # useful (algorithmic) and, for bf16x6, issued (3 products) MFMA rates
            use = alt_probe["flops"] / (alt_probe["ms"] / 1e3) / 1e12
            k = 3 if alt == "bf16x6" else 1
            tr_a, tsrc_a = pmc_traffic(alt_probe["kernel"], args.config + "/" + alt)
            alt_roof = {"bound": "mfma", "kernel": alt_probe["kernel"],
                        "achieved": round(use, 3), "issued": round(k * use, 3), "peak": BF16_MFMA_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": round(use / BF16_MFMA_PEAK_TFLOPS, 5),
                        "frac_issued": round(k * use / BF16_MFMA_PEAK_TFLOPS, 5),
                        "launches_per_step": alt_probe["launches_per_step"], "timed_launches": alt_probe["timed"],
                        "avg_launch_us": round(alt_probe["ms"] * 1e3 / alt_probe["timed"], 2),
                        "flops_per_launch": round(alt_probe["flops"] / alt_probe["timed"]),
                        "traffic": tr_a, "traffic_source": tsrc_a,
                        "step_achieved_tflops": round(flops_img * alt_value / 1e12, 3),
                        "step_frac": round(flops_img * alt_value / 1e12 / BF16_MFMA_PEAK_TFLOPS, 5)}
        if not args.no_fp32_mode:
            fp32_value, fp32_ms, _ = mode_throughput(cfg, SV, "fp32", steps=args.parity_steps)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(cfg, cfgname)
    if rank == 0:
        line = {
            "metric": METRIC[cfgname][0],
            "value": round(value, 2),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "warmup_extra_steps": extra,
            "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")),
            "warmup_s": round(warm_s, 3),
            "ms_per_step": round(ms, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic U[-1,1] NHWC batch, target=input, eps on-device Philox; deterministic splitmix64 init",
            "config": {"workload": METRIC[cfgname][1],
                       "model": args.config, "global_batch": B * world, "per_gpu_batch": B,
                       "image": [cfg.height, cfg.width, cfg.channels], "mc_steps": cfg.mc_steps,
                       "parallelism": "dp%d" % world,
                       "grad_allreduce": ("per-step buckets overlapped with the backward" if overlap else "one call after the backward") if world > 1 else None},
            "elbo_per_img": round(elbo, 5),
            "full": args.full,
            "dump_outputs": args.dump_outputs,
            # bf16x6 and fp32 are held to the fp32 parity bounds (tests/test_headline_gpu.py); plain bf16
            # operands are not (x_hat_7 / gradients decorrelate from float64 at T=8): bf16 is labelled
            "parity": args.dtype != "bf16",
            "bf16_value": None if alt_value is None or alt != "bf16" else round(alt_value, 2),
            "bf16_ms_per_step": None if alt_ms is None or alt != "bf16" else round(alt_ms, 3),
            "bf16_parity": False if alt == "bf16" and alt_value is not None else None,
            "bf16_roofline": alt_roof if alt == "bf16" else None,
            "parity_value": round(value, 2) if args.dtype != "bf16" else (None if alt_value is None else round(alt_value, 2)),
            "parity_ms_per_step": round(ms, 3) if args.dtype != "bf16" else (None if alt_ms is None else round(alt_ms, 3)),
            "parity_dtype": args.dtype if args.dtype != "bf16" else ("bf16x6" if alt_value is not None else None),
            "parity_roofline": alt_roof if alt == "bf16x6" else None,
            "fp32_value": None if fp32_value is None else round(fp32_value, 2),
            "fp32_ms_per_step": None if fp32_ms is None else round(fp32_ms, 3),
            "flops_per_img": flops_img,
            "roofline": roof,
            "cpu_baseline": cpu,
        }
        print(json.dumps(line), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
