"""Power-spectrum measurements; prints one JSON line and writes it to
profiles/spectrum_bench.json (or --out).

(a) svae_op_power_spectrum at CelebA's report shape: the stack [input, x_hat_0 .. x_hat_7, one more slot] of
    B = 128 images, n = (T + 2) * 128 at 64x64x3, against 128 targets, both planes.  One launch per call,
    event-timed over --iters calls, us per call per round and their median; with it the fp64 operations the stated
    order needs (counted from the shape below; none of them fused) and the bytes it must read once.
    --profile-only launches the same calls untimed, for the kernel's own time in a kernel trace.
(b) the same table by a straightforward torch formulation on the same device and the same fp32 NHWC input, in
    fp64: window, torch.fft.rfft2, abs()^2 times the multiplicity, index_add_ over the same bin table (the skipped
    entries into a spare bin), for the images and for their differences.  Timed in the same process in alternating
    rounds; the largest relative difference between the two results is reported.
(c) NoisyTrainer.spectrum() on a synthetic CelebA-shaped test split of --windows whole windows at the celeba
    preset (B = 128, T = 8), host clock (it ends in its device -> host copy), per window; beside it the forwards
    and generate calls it contains (one of each per window), synchronised, in the same rounds.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"
S = importlib.import_module(PKG + ".spectra")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def fp64_ops(n, h, w, c, n_bins, planes=2):
    """fp64 operations of the stated order per call (each product, sum and difference counts one; nothing is
    fused): per image, channel and plane 2 products per pixel for the window (3 operations in the difference plane),
    4 per (row, column, tap) of the row pass, 8 per (row, column, tap) of the column pass, 4 per spectrum entry for
    the power and one add per entry and per (column, bin) for the bins."""
    wu = w // 2 + 1
    per_plane = 2 * h * w + 4 * h * wu * w + 8 * h * wu * h + 4 * h * wu + h * wu + wu * n_bins
    return n * c * (planes * per_plane + (planes - 1) * h * w)


def torch_spectrum(x, y, win2d, mult, index, n_bins):
    """[n, c, 2, n_bins] fp64 by torch ops: x [n,H,W,C], y [ny,H,W,C] fp32 NHWC on the device."""
    n, h, w, c = x.shape
    xd = x.permute(0, 3, 1, 2).double()
    yd = y.permute(0, 3, 1, 2).double().repeat(n // y.shape[0], 1, 1, 1)
    planes = torch.stack([xd, xd - yd], 2) * win2d                    # [n, c, 2, h, w]
    p = (torch.fft.rfft2(planes).abs() ** 2 * mult).flatten(3)          # [n, c, 2, h * wu]
    out = torch.zeros(n, c, 2, n_bins + 1, dtype=torch.float64, device=x.device)
    out.index_add_(3, index, p)
    return out[..., :n_bins]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="celeba")
    ap.add_argument("--dtype", default="bf16x6")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", type=int, default=4, help="whole test windows of the report leg")
    ap.add_argument("--skip-report", action="store_true", help="legs (a) and (b) only")
    ap.add_argument("--profile-only", action="store_true",
                    help="only launch the op --iters times, nothing timed (for rocprofv3 --kernel-trace --stats -- "
                         "python tools/bench_spectrum.py --profile-only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectrum needs a GPU")
    cfgmod = importlib.import_module(PKG + ".config")
    cfg = cfgmod.preset(a.config, dtype=a.dtype)
    B, T, H, W, C = cfg.batch, cfg.mc_steps, cfg.height, cfg.width, cfg.channels
    lo, hi = (float(v) for v in cfg.range)
    rng = hi - lo
    n = (T + 2) * B
    gen = torch.Generator(device="cuda").manual_seed(0)
    # smooth targets plus noise, and a stack of noisier copies, as in a report
    yy = torch.linspace(0, 1, H, device="cuda").view(1, H, 1, 1)
    xx = torch.linspace(0, 1, W, device="cuda").view(1, 1, W, 1)
    ab = torch.rand(2, B, 1, 1, C, generator=gen, device="cuda")
    y = (lo + rng * (ab[0] * yy + ab[1] * xx * (1 - ab[0]))
         + 0.1 * rng * (torch.rand(B, H, W, C, generator=gen, device="cuda") - 0.5)).clamp(lo, hi).contiguous()
    x = (y.repeat(T + 2, 1, 1, 1) + 0.2 * rng * (torch.rand(n, H, W, C, generator=gen, device="cuda") - 0.5)
         ).clamp(lo, hi).contiguous()
    win_y, win_x, _, _, table, n_bins, _ = S.device_tables(H, W, "hann", x.device)
    out = torch.empty(n, C, 2, n_bins, dtype=torch.float64, device="cuda")
    op = lambda: S.power_spectrum(x, y, out=out)
    if a.profile_only:
        for _ in range(a.iters):
            op()
        torch.cuda.synchronize()
        return
    win2d = win_y.view(H, 1) * win_x.view(1, W)
    mult = torch.from_numpy(S.multiplicity(W)).to(x.device)
    index = torch.where(table >= 0, table, torch.full_like(table, n_bins)).flatten().long()
    ref = lambda: torch_spectrum(x, y, win2d, mult, index, n_bins)
    got, want = op().clone(), ref()
    diff = float(((got - want).abs() / want.abs().amax((2, 3), keepdim=True)).max())
    legs = {"op": op, "torch_fp64_rfft2_index_add": ref}
    for f in legs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, f in legs.items():
            us[name].append(timed(f, a.iters))
    med = statistics.median
    ops, nbytes = fp64_ops(n, H, W, C, n_bins), 4 * (n + B) * H * W * C
    kernel = {name: dict(us_per_call_median=round(med(v), 2), us_rounds=[round(t, 2) for t in v]) for name, v in us.items()}
    kernel["op"].update(fp64_ops_per_call=ops, fp64_gop_per_s=round(ops / med(us["op"]) / 1e3, 1),
                        bytes_read_once=nbytes, gb_per_s_on_those_bytes=round(nbytes / med(us["op"]) / 1e3, 1),
                        blocks=n * C)
    kernel["op_over_torch"] = round(med(us["op"]) / med(us["torch_fp64_rfft2_index_add"]), 4)
    kernel["max_difference_over_largest_value_of_the_row"] = diff
    res = dict(tool="bench_spectrum", device=torch.cuda.get_device_name(0),
               shape=dict(n=n, ny=B, h=H, w=W, c=C, n_bins=n_bins), window="hann", iters=a.iters, rounds=a.rounds,
               kernel=kernel)

    if not a.skip_report:
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

        def contained():
            for _ in range(a.windows):
                net.forward(inp, tgt, eps, 1.0)
            for _ in range(a.windows):
                net.generate(eps)

        tr.spectrum()
        contained()
        sp_ms, fw_ms = [], []
        for _ in range(a.rounds):
            fw_ms.append(clock(contained) / a.windows)
            sp_ms.append(clock(tr.spectrum) / a.windows)
        res["spectrum"] = dict(config=a.config, dtype=a.dtype, batch=B, mc_steps=T, windows=a.windows,
                               spectrum_ms_per_window_median=round(med(sp_ms), 3),
                               spectrum_ms_rounds=[round(v, 3) for v in sp_ms],
                               forward_and_generate_ms_per_window_median=round(med(fw_ms), 3),
                               forward_and_generate_ms_rounds=[round(v, 3) for v in fw_ms],
                               spectrum_over_contained=round(med(sp_ms) / med(fw_ms), 4))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
