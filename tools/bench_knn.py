"""k-NN manifold measurements; prints one JSON line and writes it to profiles/manifold_bench.json (or
--out).  Modelled on tools/bench_quality.py.

(a) svae_op_pairwise_knn with one group, n = m, k = 5 and two radii per column (the columns' own 3rd and 5th
    neighbour radii), at (n, d) = (1 152, 12 288), (10 000, 12 288) and (10 000, 3 072).  Rows N(0, 1) / 2 as centred
    images are.  Event-timed, mean us per call per round, against
      - svae_op_pairwise_stats on the same inputs with the nearest neighbour only: the same norms and tile, so the
        difference is the cost of the new epilogue;
      - a torch fp32 formulation: row chunks of about 1 GB of [chunk, m] fp32, x @ y.T, the norms, clamp,
        topk(k, largest=False), the comparison with the radii and the sum.
    timed in the same process in alternating rounds.  --skip-op leaves this leg out.
(b) NoisyTrainer.sample_quality(manifold_k=(3, 5)) against the same call without manifold_k on a synthetic
    CelebA-shaped test split of --windows whole windows at the celeba preset (B = 128, T = 8), host clock (it ends
    in its device -> host copy), in alternating rounds.  --skip-trainer leaves this leg out.
Run it in several processes (--out each) for the round-to-round and process-to-process spread.
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
Q = importlib.import_module(PKG + ".quality")
CHUNK_BYTES = 1 << 30
K, RADII_K = 5, (3, 5)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def torch_knn(x, y, k, radii):
    """(knn_d2 [n, k], inside [n, n_radii]) by torch fp32 ops, no [n, m] tensor beyond a chunk of rows."""
    n, m = x.shape[0], y.shape[0]
    a, b = x.square().sum(1), y.square().sum(1)
    r32 = radii.float()
    knn = torch.empty(n, k, dtype=torch.float32, device=x.device)
    inside = torch.empty(n, radii.shape[1], dtype=torch.int64, device=x.device)
    chunk = max(1, CHUNK_BYTES // (4 * m))
    for s in range(0, n, chunk):
        d2 = (a[s:s + chunk, None] + b[None, :] - 2.0 * (x[s:s + chunk] @ y.t())).clamp_min_(0.0)
        knn[s:s + chunk] = d2.topk(k, dim=1, largest=False).values
        for c in range(radii.shape[1]):
            inside[s:s + chunk, c] = (d2 <= r32[None, :, c]).sum(1)
    return knn, inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16x6")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=78, help="whole test windows of the sample_quality leg")
    ap.add_argument("--skip-op", action="store_true", help="leg (b) only")
    ap.add_argument("--skip-trainer", action="store_true", help="leg (a) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manifold_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn needs a GPU")
    mean_of = lambda v: sum(v) / len(v)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = dict(tool="bench_knn", device=torch.cuda.get_device_name(0), rounds=a.rounds, k=K, radii_k=list(RADII_K),
               argv=sys.argv[1:])
    rows = []
    for n, d in () if a.skip_op else ((1152, 12288), (10000, 12288), (10000, 3072)):
        x = torch.randn(n, d, generator=gen, device="cuda") * 0.5
        y = torch.randn(n, d, generator=gen, device="cuda") * 0.5
        radii, _ = Q.self_radii(y, RADII_K)
        out = {"knn_d2": torch.empty(n, 1, K, dtype=torch.float64, device="cuda"),
               "inside": torch.empty(n, 1, len(RADII_K), dtype=torch.int64, device="cuda"),
               "nonfinite": torch.empty(n, 1, dtype=torch.int64, device="cuda")}
        nn_out = {"nn_d2": torch.empty(n, 1, dtype=torch.float64, device="cuda"),
                  "nn_idx": torch.empty(n, 1, dtype=torch.int64, device="cuda")}
        legs = {"op": lambda: Q.knn_stats(x, [y], K, radii=[radii], out=out),
                "pairwise_stats_nn_only": lambda: Q.pairwise_stats(x, [y], [], out=nn_out, ksum=False),
                "torch_fp32_chunked": lambda: torch_knn(x, y, K, radii)}
        gk, gi, gb = legs["op"]()
        wk, wi = legs["torch_fp32_chunked"]()
        _, nd, _ = legs["pairwise_stats_nn_only"]()
        diff = dict(knn_d2_max_abs=float((gk[:, 0] - wk.double()).abs().max()),
                    inside_differ=int((gi[:, 0] != wi).sum()), inside_total=int(gi.sum()),
                    first_neighbour_is_nn_d2=bool(torch.equal(gk[:, 0, 0], nd[:, 0])), nonfinite=int(gb.sum()))
        del wk, wi
        iters = {}
        for name, f in legs.items():  # warm up, and size the timed window to about half a second
            f()
            iters[name] = max(1, min(50, int(5e5 / timed(f, 1))))
        us = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, f in legs.items():
                us[name].append(timed(f, iters[name]))
        t = {name: mean_of(v) for name, v in us.items()}
        flop = 2.0 * n * n * d
        row = dict(n=n, m=n, d=d)
        for name in legs:
            row[name] = dict(us_per_call=round(t[name], 1), us_rounds=[round(v, 1) for v in us[name]],
                             iters=iters[name], inner_product_tflops=round(flop / t[name] / 1e6, 1))
        row.update(op_over_pairwise_stats=round(t["op"] / t["pairwise_stats_nn_only"], 4),
                   op_over_torch=round(t["op"] / t["torch_fp32_chunked"], 4), op_against_torch=diff)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y
    if rows:
        res["op"] = rows

    if not a.skip_trainer:
        cfgmod = importlib.import_module(PKG + ".config")
        SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
        DS = importlib.import_module(PKG + ".data").DeviceDataset
        NT = importlib.import_module(PKG + ".trainer").NoisyTrainer
        cfg = cfgmod.preset("celeba", dtype=a.dtype)
        B, T = cfg.batch, cfg.mc_steps
        net = SV(cfg, seed=0)
        ds = DS.synthetic(5 * a.windows * B, cfg.height, cfg.width, cfg.channels, seed=0, range=cfg.range,
                          device="cuda")  # a fifth is the test split
        assert ds.test_size == a.windows * B, ds.test_size
        tr = NT(net, ds, seed=0)

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3  # ms

        with_k = lambda: tr.sample_quality(manifold_k=RADII_K)
        rep = with_k()
        tr.sample_quality()
        plain_ms, man_ms = [], []
        for _ in range(a.rounds):
            plain_ms.append(clock(tr.sample_quality))
            man_ms.append(clock(with_k))
        res["sample_quality"] = dict(config="celeba", dtype=a.dtype, batch=B, mc_steps=T, windows=a.windows,
                                     images=rep["images"], train_images=rep["train_images"],
                                     manifold_k=rep["manifold_k"],
                                     plain_ms=round(mean_of(plain_ms), 1), plain_ms_rounds=[round(v, 1) for v in plain_ms],
                                     with_manifold_ms=round(mean_of(man_ms), 1),
                                     with_manifold_ms_rounds=[round(v, 1) for v in man_ms],
                                     with_over_plain=round(mean_of(man_ms) / mean_of(plain_ms), 3),
                                     untrained_report=dict(steps=[s["manifold"] for s in rep["steps"]],
                                                           real_against_train=rep["real"]["manifold_train"]))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
