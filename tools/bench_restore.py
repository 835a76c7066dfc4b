"""Whole-image restoration measurements; prints one JSON line and writes it to
profiles/restore_bench.json (or --out).

One 1024 x 1024 x 3 uint8 image, tile 64, stride 32 (31 x 31 = 961 tiles, none clamped), alternating in rounds in
this process, event-timed:

  extract        svae_op_extract_tiles of all 961 tiles (uint8 -> fp32)
  blend_1        svae_op_blend_tiles of one set of tiles into uint8
  blend_8        the same for nstack = 8 (the chain steps of a steps="all" restoration)
  torch_extract  the same tiles with torch: dequantise, a strided view (unfold), one contiguous copy
  torch_blend_1  the same image with torch: tiles times the window, fold, the window folded as well, divide,
  torch_blend_8  where(known), quantise (fold sums in an order of its own: equal within rounding, not bitwise)

and SequentialVAE.restore of that image on the celeba preset (B = 128, bf16x6: 8 windows) against the 8 forwards
it contains, host-timed around a device synchronise.  The event-timed mean of a leg is bounded below by the host's
enqueue time of its launches (one ctypes call for the ops); no threshold is set on any figure.  Kernel times come
from a trace of one leg: rocprofv3 --kernel-trace --stats -- python tools/bench_restore.py --profile-case extract.
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "sequential-variational-autoencoder_amd"
R = importlib.import_module(PKG + ".restore")
SIDE, C, TILE, STRIDE = 1024, 3, 64, 32
LO, HI = -1.0, 1.0


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def op_legs():
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (1, SIDE, SIDE, C), dtype=torch.uint8, generator=g).cuda()
    known = (torch.rand(1, SIDE, SIDE, generator=g) < 0.25).to(torch.uint8).cuda()
    grid = R.TileGrid(1, SIDE, SIDE, C, TILE, TILE, STRIDE, STRIDE)
    k = grid.ky
    assert grid.n_tiles == 961 and int(grid.ox[-1]) == (k - 1) * STRIDE
    tiles = torch.empty(8, grid.n_tiles, TILE, TILE, C, device="cuda")
    R.extract_tiles(img, grid, out=tiles[0])
    for s in range(1, 8):
        tiles[s] = tiles[0] * (1 - 0.05 * s)
    out8 = torch.empty(8, 1, SIDE, SIDE, C, dtype=torch.uint8, device="cuda")
    scratch = torch.empty_like(tiles[0])
    win = torch.from_numpy(grid.weight()).float().cuda()                        # [64, 64]
    win_cols = win.reshape(1, 1, TILE * TILE, 1).expand(1, 1, TILE * TILE, k * k).reshape(1, TILE * TILE, k * k)

    def blend(n):
        return lambda i: R.blend_tiles(tiles, grid, nstack=n, source=img, known=known, range=(LO, HI), out_u8=out8[:n])

    def torch_extract(i):
        x = LO + img.float() * ((HI - LO) / 255.0)
        v = x[0].unfold(0, TILE, STRIDE).unfold(1, TILE, STRIDE)                # [k, k, C, 64, 64]
        return v.permute(0, 1, 3, 4, 2).reshape(k * k, TILE, TILE, C).contiguous()

    def torch_blend(n):
        def fn(i):
            t = tiles[:n].view(n, k * k, TILE, TILE, C) * win[None, None, :, :, None]
            cols = t.permute(0, 4, 2, 3, 1).reshape(n, C * TILE * TILE, k * k)
            acc = F.fold(cols, (SIDE, SIDE), TILE, stride=STRIDE)               # [n, C, H, W]
            wgt = F.fold(win_cols, (SIDE, SIDE), TILE, stride=STRIDE)           # [1, 1, H, W]
            v = (acc / wgt).permute(0, 2, 3, 1)
            src = LO + img.float() * ((HI - LO) / 255.0)
            v = torch.where(known[:, :, :, None] != 0, src, v)
            return ((v - LO) * (255.0 / (HI - LO))).round_().clamp_(0, 255).to(torch.uint8)
        return fn

    legs = {"extract": lambda i: R.extract_tiles(img, grid, out=scratch), "blend_1": blend(1), "blend_8": blend(8),
            "torch_extract": torch_extract, "torch_blend_1": torch_blend(1), "torch_blend_8": torch_blend(8)}
    # the torch formulation is the same result within rounding (fold adds in fp32 in an order of its own)
    assert (torch_extract(0) - tiles[0]).abs().max().item() <= 1e-6
    blend(8)(0)
    diff = (torch_blend(8)(0)[:, None].int() - out8.int()).abs().max().item()
    assert diff <= 1, diff
    tile_bytes = grid.n_tiles * TILE * TILE * C * 4
    image_bytes = SIDE * SIDE * C
    moved = {"extract": image_bytes + tile_bytes, "blend_1": tile_bytes + 2 * image_bytes + SIDE * SIDE,
             "blend_8": 8 * (tile_bytes + image_bytes) + image_bytes + SIDE * SIDE}
    return legs, moved


def restore_ms(rounds):
    """(whole restore, the 8 forwards it contains) in ms per image, per round."""
    cfgmod = importlib.import_module(PKG + ".config")
    SV = importlib.import_module(PKG + ".sequential_vae").SequentialVAE
    cfg = cfgmod.preset("celeba", dtype="bf16x6")
    assert (cfg.batch, cfg.height, cfg.width, cfg.channels) == (128, TILE, TILE, C)
    net = SV(cfg, seed=0)
    img = torch.randint(0, 256, (1, SIDE, SIDE, C), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    x = (torch.rand(128, TILE, TILE, C, device="cuda") * 2 - 1).contiguous()
    eps = torch.zeros(cfg.mc_steps, 128, cfg.latent_dim, device="cuda")
    nwin = len(R.windows(961, 128))

    def whole():
        net.restore(img, stride=STRIDE)

    def forwards():
        for _ in range(nwin):
            net.forward(x, x, eps, 1.0)

    out = {"restore": [], "forwards": []}
    for fn in (whole, forwards):
        fn()
    for _ in range(rounds):
        for name, fn in (("restore", whole), ("forwards", forwards)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / 3 * 1e3)
    return out, nwin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_bench.json"))
    ap.add_argument("--ops-only", action="store_true", help="skip the whole-restore legs")
    ap.add_argument("--profile-case", default=None, metavar="LEG",
                    help="only run this leg --iters times, nothing timed (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore needs a GPU")
    legs, moved = op_legs()
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
    res = dict(tool="bench_restore", device=torch.cuda.get_device_name(0), image=[SIDE, SIDE, C], tile=TILE,
               stride=STRIDE, tiles=961, iters=a.iters,
               timing="device events around --iters enqueues, alternating rounds; bounded below by the host enqueue",
               legs={k: dict(us_median=round(med(v), 2), us_min=round(min(v), 2), us_rounds=[round(t, 2) for t in v])
                     for k, v in us.items()})
    for k, b in moved.items():
        res["legs"][k]["bytes_moved"] = b
        res["legs"][k]["gb_per_s_event_timed"] = round(b / med(us[k]) / 1e3, 1)
    for k in ("extract", "blend_1", "blend_8"):
        res["torch_over_" + k] = round(med(us["torch_" + k]) / med(us[k]), 2)
    ms, nwin = (None, 0) if a.ops_only else restore_ms(a.rounds)
    if ms is not None:
        res["restore"] = dict(config="celeba", dtype="bf16x6", batch=128, windows=nwin,
                              ms_per_image_median=round(med(ms["restore"]), 3),
                              forwards_ms_median=round(med(ms["forwards"]), 3),
                              restore_rounds=[round(t, 3) for t in ms["restore"]],
                              forwards_rounds=[round(t, 3) for t in ms["forwards"]],
                              around_the_forwards_ms=round(med(ms["restore"]) - med(ms["forwards"]), 3))
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
