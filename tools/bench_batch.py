"""Batch-pipeline measurements; prints one JSON line and writes it to
profiles/batch_pipeline.json (or --out).

(a) svae_op_make_batch alone at 64x64x3, B = 128 and 256, uint8 and fp32 sources, both outputs, at the
    reference's noise constants: event-timed mean us per launch over windows that walk a dataset larger
    than one batch, and GB/s on the bytes the contract moves (source row + two fp32 outputs per element),
    against the measured float4 copy rate of the device (6.29 TB/s).
(b) the normals' maximum deviation from the float64 restatement (tests/batch_ref.py) over 2^20 draws: the
    figure tests/test_make_batch_gpu.py takes its bound from.
(c) preset celeba, bf16x6: `trainer.step()` with denoise_train off and on (each step returns its loss, so
    each ends in a device synchronise), and the same two without the loss fetch -- make_batch + forward +
    backward_apply, the step bench.py times -- next to that plain step on a fixed batch, all alternating
    in rounds in this process.
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "sequential-variational-autoencoder_amd"
L = importlib.import_module(PKG + "._lib")
COPY_TBS = 6.29  # float4 copy, measured on the MI355X


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def kernel_rows(iters, rounds, nimg=2048, only=None):
    """only = (B, source, outputs): that configuration alone, `iters` launches, nothing timed here (for
    rocprofv3 --kernel-trace --stats -- python tools/bench_batch.py --profile-case 128:uint8:target+input:
    the event-timed mean below has a floor of one host enqueue, ~8 us through ctypes)."""
    out = []
    per = 64 * 64 * 3
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (nimg, per), dtype=torch.uint8, generator=g).cuda()
    f32 = (u8.float() / 127.5 - 1.0).contiguous()
    for B in (128, 256):
        tgt, inp = torch.empty(B, per, device="cuda"), torch.empty(B, per, device="cuda")
        nwin = nimg // B
        for name, data in (("uint8", u8), ("fp32", f32)):
            for mode, (p, s, sc, want_in) in (("target+input", (0.1, 0.1, 0.1, True)), ("target only", (0.0, 0.0, 0.0, False))):
                def fn(i):
                    L.check(L.lib().svae_op_make_batch(L.ptr(data), 1 if data.dtype == torch.uint8 else 0, None,
                                                       (i % nwin) * B, B, per, -1.0, 1.0, p, s, sc, 1, i * (B * per // 4),
                                                       L.ptr(tgt), L.ptr(inp) if want_in else None, L.stream_ptr()))
                if only is not None:
                    if only == (B, name, mode):
                        for i in range(iters):
                            fn(i)
                        torch.cuda.synchronize()
                    continue
                for i in range(5):
                    fn(i)
                torch.cuda.synchronize()
                us = [timed(fn, iters) for _ in range(rounds)]
                nbytes = B * per * (data.element_size() + (8 if want_in else 4))
                m = sum(us) / len(us)
                out.append(dict(batch=B, source=name, outputs=mode, us_per_launch=round(m, 2),
                                us_rounds=[round(v, 2) for v in us], bytes=nbytes, gb_per_s=round(nbytes / m / 1e3, 1),
                                share_of_copy_rate=round(nbytes / m / 1e6 / COPY_TBS, 4)))
    return out


def normal_deviation():
    import batch_ref
    n = 1 << 20
    x = torch.zeros(1, n, device="cuda")
    out = torch.empty_like(x)
    seed, off = 0x0123456789ABCDEF, 2 ** 32 - 1000
    L.check(L.lib().svae_op_make_batch(L.ptr(x), 0, None, 0, 1, n, -1e30, 1e30, 0.0, 0.0, 1.0, seed, off, None,
                                       L.ptr(out), L.stream_ptr()))
    ref = batch_ref.normals(n, seed, off)
    d = np.abs(out.cpu().numpy().ravel().astype(np.float64) - ref)
    return dict(draws=n, max_abs_dev=float("%.4g" % d.max()), mean_abs_dev=float("%.4g" % d.mean()),
                max_abs_normal=float("%.4g" % np.abs(ref).max()))


def trainer_rows(steps, warmup, rounds):
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    DS = importlib.import_module(PKG + ".data").DeviceDataset
    NT = importlib.import_module(PKG + ".trainer").NoisyTrainer
    cfg = cfgmod.preset("celeba", dtype="bf16x6")
    B = cfg.batch
    ds = DS.synthetic(8 * B, cfg.height, cfg.width, cfg.channels, seed=0, test_fraction=0.25, device="cuda")
    net = SV(cfg, seed=0)
    tr = {False: NT(net, ds, denoise_train=False), True: NT(net, ds, denoise_train=True)}
    x = (torch.rand(B, cfg.height, cfg.width, cfg.channels, device="cuda") * 2 - 1).contiguous()
    it = [0]

    def engine_step(inp, tgt):
        it[0] += 1
        net.forward(inp, tgt, None, 1.0 - math.exp(-it[0] / cfg.reg_coeff_rate))
        net.backward_apply(cfg.learning_rate, it[0])

    legs = {
        "plain_step_fixed_batch": lambda: engine_step(x, x),                      # what bench.py times
        "pipeline_step_denoise_off": lambda: engine_step(*tr[False]._next()),     # + make_batch, no loss fetch
        "pipeline_step_denoise_on": lambda: engine_step(*tr[True]._next()),
        "trainer_step_denoise_off": lambda: tr[False].step(),                     # returns the loss: one sync per step
        "trainer_step_denoise_on": lambda: tr[True].step(),
    }
    for f in legs.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    res = {k: dict(ms_per_step=round(sum(v) / len(v), 3), rounds=[round(a, 3) for a in v]) for k, v in ms.items()}
    base = res["plain_step_fixed_batch"]["ms_per_step"]
    for k in res:
        res[k]["over_plain_step"] = round(res[k]["ms_per_step"] / base, 4)
    res["on_over_off_trainer"] = round(res["trainer_step_denoise_on"]["ms_per_step"] /
                                       res["trainer_step_denoise_off"]["ms_per_step"], 4)
    res["on_over_off_pipeline"] = round(res["pipeline_step_denoise_on"]["ms_per_step"] /
                                        res["pipeline_step_denoise_off"]["ms_per_step"], 4)
    return dict(config="celeba", dtype="bf16x6", batch=B, steps=steps, warmup=warmup, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_pipeline.json"))
    ap.add_argument("--profile-case", default=None, metavar="B:SOURCE:OUTPUTS",
                    help="only launch this kernel configuration --iters times (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch needs a GPU")
    if a.profile_case:
        b, src, mode = a.profile_case.split(":")
        kernel_rows(a.iters, a.rounds, only=(int(b), src, mode))
        return
    res = dict(tool="bench_batch", device=torch.cuda.get_device_name(0), copy_rate_tb_per_s=COPY_TBS,
               kernel=kernel_rows(a.iters, a.rounds), normals=normal_deviation())
    if not a.no_trainer:
        res["trainer"] = trainer_rows(a.steps, a.warmup, a.rounds)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
