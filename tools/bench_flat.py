"""Flat-generator measurements (DESIGN.md "Flat generator"); prints one JSON line and writes it to
profiles/flat_bench.json (or --out).

(a) every layer shape of the C = 3 flat stack at B = 128, 64x64: event-timed mean of svae_op_flat_conv /
    _dgrad / _wgrad against the same shape through the general fp32 path (svae_op_conv / _conv_dgrad /
    _conv_wgrad at stride 1) where that path computes the shape, alternating the two in rounds.  The
    forward asks the path (svae_op_conv returns an error for cout % 4).  The other two entry points
    return 0 for every shape, so the rule is the one their kernels set (PARENT_RULE below), and each
    compared result is checked against the flat op's (parent_max_rel_diff);
(b) c_infusion_test at B = 128, T = 8, bf16x6: images/s over the timed steps, the flat family's launches
    per step (counted from the schedule) and its fp32 TF/s against the 157 TF matrix peak on useful and
    on issued (padded) FLOPs, over the family's isolated kernel time from (a).  That time is a LOWER
    bound of the family's time in the step: the forward ops are timed as the step runs them (fused
    BN + lrelu input, statistics partials and their finish), but the gradient ops read raw tensors,
    where the step forms d pre from two tensors while staging, writes fp64 partials and adds the
    statistics-finish and bias-sum launches.
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"
L = importlib.import_module(PKG + "._lib")
PEAK_TF = 157.3


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


# Which shapes the general fp32 path computes, read from its kernels (the entry points do not check):
#   dgrad  cin % 4 != 0 goes to the small-N gather, which accumulates 4 outputs at most (misc.hip
#          gconv_smalln_kernel): cin <= 4 or cin % 4 == 0
#   wgrad  wgrad_kernel stages dy with 16-byte loads along cout whatever cout is (gemm.hip): cout % 4 == 0,
#          otherwise the loads are misaligned and run past the tensor's last row
PARENT_RULE = {"dgrad": lambda cin, cout: cin <= 4 or cin % 4 == 0,
               "wgrad": lambda cin, cout: cout % 4 == 0}


def ab(flat, parent, iters, rounds, ok):
    """mean us of both, alternating rounds after a warm-up of each; parent None where the general path does
    not take the shape (ok False)"""
    for _ in range(3):
        flat()
        if ok:
            parent()
    torch.cuda.synchronize()
    tf, tp = [], []
    for _ in range(rounds):
        tf.append(timed(flat, iters))
        if ok:
            tp.append(timed(parent, iters))
    return sum(tf) / len(tf), (sum(tp) / len(tp) if ok else None)


def layer_shapes(n, h, sizes, iters, rounds):
    lib = L.lib()
    out = []
    scratch = torch.empty(64 << 20, device="cuda")
    for cin, cout in zip(sizes[:-1], sizes[1:]):
        x = torch.randn(n, h, h, cin, device="cuda")
        w = torch.randn(4, 4, cin, cout, device="cuda") * 0.05
        dy = torch.randn(n, h, h, cout, device="cuda")
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        s = L.stream_ptr()
        nb = scratch.numel() * 4
        chk = lambda rc: L.check(rc)
        y2, dx2, dw2 = torch.zeros_like(y), torch.zeros_like(dx), torch.zeros_like(dw)
        mean, inv, beta = torch.zeros(cin, device="cuda"), torch.ones(cin, device="cuda"), torch.zeros(cin, device="cuda")
        stats = torch.empty(2 * cout, device="cuda")
        ops = {
            "conv": (lambda: chk(lib.svae_op_flat_conv(L.ptr(x), n, h, cin, L.ptr(w), cout, None, None, None, L.ptr(y), None, s)),
                     lambda: chk(lib.svae_op_conv(L.ptr(x), n, h, cin, L.ptr(w), cout, 1, 0, L.ptr(y2), s)), y, y2),
            "dgrad": (lambda: chk(lib.svae_op_flat_dgrad(L.ptr(dy), n, h, cin, L.ptr(w), cout, L.ptr(dx), s)),
                      lambda: chk(lib.svae_op_conv_dgrad(L.ptr(dy), n, h, cin, L.ptr(w), cout, 1, 0, L.ptr(dx2), s)), dx, dx2),
            "wgrad": (lambda: chk(lib.svae_op_flat_wgrad(L.ptr(x), n, h, cin, L.ptr(dy), cout, L.ptr(dw), L.ptr(scratch), nb, s)),
                      lambda: chk(lib.svae_op_conv_wgrad(L.ptr(x), n, h, cin, L.ptr(dy), cout, 1, 0, L.ptr(dw2), L.ptr(scratch), nb, s)), dw, dw2),
        }
        # the forward as the step launches it: BN + lrelu on the load (layers >= 1), statistics partials + finish
        # (every layer but the output conv)
        in_step = lambda: chk(lib.svae_op_flat_conv(L.ptr(x), n, h, cin, L.ptr(w), cout, L.ptr(mean), L.ptr(inv),
                                                    L.ptr(beta), L.ptr(y), L.ptr(stats), s))
        P = n * h * h
        pad = lambda c: 16 if c <= 16 else 32
        row = dict(cin=cin, cout=cout, useful_gflop=2.0 * 16 * cin * cout * P / 1e9,
                   issued_gflop=dict(conv=2.0 * 16 * cin * pad(cout) * P / 1e9, dgrad=2.0 * 16 * cout * pad(cin) * P / 1e9,
                                     wgrad=2.0 * 16 * cin * pad(cout) * P / 1e9))
        for k, (f, p, got, got2) in ops.items():
            if k == "conv":  # the path is asked: an error return (before any launch) = not accepted
                parent_ok = lib.svae_op_conv(L.ptr(x), n, h, cin, L.ptr(w), cout, 1, 0, L.ptr(y2), s) == 0
            else:
                parent_ok = PARENT_RULE[k](cin, cout)
            tf_, tp_ = ab(f, p, iters, rounds, parent_ok)
            row[k] = dict(flat_us=round(tf_, 2), parent_accepts=parent_ok,
                          parent_us=None if tp_ is None else round(tp_, 2),
                          parent_over_flat=None if tp_ is None else round(tp_ / tf_, 3),
                          parent_max_rel_diff=(float("%.3g" % ((got - got2).abs().max() / got.abs().max()).item())
                                               if parent_ok else None),
                          flat_tflops_useful=round(row["useful_gflop"] / tf_ * 1e3, 3))
        for _ in range(3):
            in_step()
        torch.cuda.synchronize()
        row["conv"]["flat_in_step_us"] = round(sum(timed(in_step, iters) for _ in range(rounds)) / rounds, 2)
        out.append(row)
    return out


def chain(batch, steps, warmup, dtype):
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    cfg = cfgmod.preset("c_infusion_test", batch=batch, dtype=dtype)
    net = SV(cfg, seed=0)
    x = torch.rand(batch, cfg.height, cfg.width, cfg.channels, device="cuda") * 2 - 1
    for _ in range(warmup):
        net.train(x, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net.forward(x, x, None, 0.5)
        net.backward_apply(cfg.learning_rate)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nl, T = cfg.flat_conv_layers, cfg.mc_steps
    # per flat step: forward nl convs + (nl - 1) statistics finishes; backward per layer wgrad + slab sum + dgrad,
    # (nl - 1) BN-sum finishes, the bias column sums + their finish
    fwd, bwd = nl + (nl - 1), 3 * nl + (nl - 1) + 2
    return dict(config="c_infusion_test", batch=batch, mc_steps=T, dtype=dtype, steps=steps,
                images_per_s=round(batch * steps / dt, 1), step_ms=round(dt / steps * 1e3, 3),
                flat_launches_per_step=dict(forward=(T - 1) * fwd, backward=(T - 1) * bwd,
                                            method="counted from the schedule (flat.hip launches + sd_stat_fin), "
                                                   "output_fwd / output_bwd / chain_noise / loss_reduce not included"),
                total_launches_per_step=None,
                total_launches_note="not measured: the engine's probe counts one kernel family, not a step"), cfg


def profile_steps(batch, steps):
    """Steps of c_infusion_test for a kernel trace (rocprofv3 --kernel-trace -- python tools/bench_flat.py
    --profile-steps N, then tools/prof_launches.py on the database): backward and the Adam update as two
    calls, so that one adam_kernel launch ends each step, which is how prof_launches.py delimits steps."""
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    cfg = cfgmod.preset("c_infusion_test", batch=batch, dtype="bf16x6")
    net = SV(cfg, seed=0)
    x = torch.rand(batch, cfg.height, cfg.width, cfg.channels, device="cuda") * 2 - 1
    for _ in range(steps):
        net.forward(x, x, None, 0.5)
        net.backward()
        net.apply_gradients(cfg.learning_rate)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_bench.json"))
    ap.add_argument("--profile-steps", type=int, default=0, help="only run this many steps (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flat needs a GPU")
    if a.profile_steps:
        profile_steps(a.batch, a.profile_steps)
        return
    layers = layer_shapes(a.batch, a.size, [3, 6, 12, 24, 12, 6, 3], a.iters, a.rounds)
    ch, cfg = chain(a.batch, a.steps, a.warmup, "bf16x6")
    T = cfg.mc_steps
    fam_us = sum(r["conv"]["flat_in_step_us"] + r["dgrad"]["flat_us"] + r["wgrad"]["flat_us"] for r in layers) * (T - 1)
    useful = 3 * sum(r["useful_gflop"] for r in layers) * (T - 1)
    issued = sum(sum(r["issued_gflop"].values()) for r in layers) * (T - 1)
    ch["flat_family"] = dict(isolated_ms_per_step=round(fam_us / 1e3, 3), useful_gflop_per_step=round(useful, 2),
                             issued_gflop_per_step=round(issued, 2),
                             tflops_useful=round(useful / fam_us * 1e3, 2),
                             tflops_issued=round(issued / fam_us * 1e3, 2),
                             share_of_fp32_matrix_peak_useful=round(useful / fam_us * 1e3 / PEAK_TF, 4),
                             share_of_fp32_matrix_peak_issued=round(issued / fam_us * 1e3 / PEAK_TF, 4),
                             method="FLOPs from shapes over the family's ops timed alone on an idle GPU (part a): the "
                                    "forward as the step launches it (fused input, statistics + finish), the two "
                                    "gradients on raw tensors without the step's d-pre staging, partials and their "
                                    "finish launches -- a lower bound of the family's time in the step, so the "
                                    "TF/s and shares are upper bounds")
    res = dict(tool="bench_flat", device=torch.cuda.get_device_name(0), layers=layers, chain=ch)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
