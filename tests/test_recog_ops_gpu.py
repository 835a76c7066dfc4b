"""Recognition-heads, latent and split-latent kernels (csrc/misc.hip) through svae_op_heads_fwd / _latent_fwd /
_latent_bwd / _heads_bwd / _splitfc / _splitfc_bwd against the float64 restatements of tests/recog_ref.py
(held to the oracle's own ops by tests/test_recog_ref.py), at the smallest shapes that reach every kernel,
every dispatch rule and every tail.  Each case asserts which kernel ran, runs twice (bitwise equal: the
kernels promise fixed summation orders) and leaves a sentinel around everything it may write.

Bounds: those of tests/test_ops_gpu.py and tests/test_flat_ops_gpu.py, max|err| <= tol * (1 + max|ref|) with
tol 2e-5 for forwards and input gradients and 5e-5 for sums over the batch (dW, db, dbeta).  Plain fp32
arithmetic (the same restatements on torch CPU float32) on exactly these cases, worst case per quantity on
that scale (MEASURED_F32 below):
  heads forward   mean 3.7e-7, stddev 4.7e-7                                    -> 2e-5 (the project's)
  latent forward  mu 1.4e-7, sig 8.2e-8, z 2.0e-7, kl_img 2.1e-7               -> 2e-5
  latent backward dhead 7.0e-8                                                 -> 2e-5
  heads backward  dx 1.4e-7                                                    -> 2e-5
                  dwm 6.4e-7, dws 5.6e-7, dbm 1.4e-7, dbs 1.4e-7               -> 5e-5
  split FC        out 2.1e-7, mean 9.8e-8, invstd 1.2e-7, dz 4.5e-7            -> 2e-5
                  dw 4.2e-7, dbeta 1.1e-7                                      -> 5e-5
Every figure is at least 10x under its bound, so the project's bounds stand for every quantity and none is
widened: only a wrong column, split, row tail or summation can exceed them.

Split FC: the backward takes lrelu' from a recomputed fp32 pre-activation, so the seeds (SFC_SEED, found on
the CPU) are those at which, in the float64 reference alone, no element has |xhat + beta| < 2e-5 (ten
times the fp32 error of a K <= 32 dot product of these magnitudes); the test asserts it before the kernel
runs, and no element is excluded from any comparison."""
import ctypes

import numpy as np
import pytest
import torch

import recog_ref as R
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

FWD_TOL, SUM_TOL = 2e-5, 5e-5
# worst |fp32 CPU - fp64| / (1 + max|ref|) per quantity over the cases below
MEASURED_F32 = {
    "head_mean": 3.7e-07, "head_std": 4.7e-07,
    "mu": 1.4e-07, "sig": 8.2e-08, "z": 2.0e-07, "kl_img": 2.1e-07, "dhead": 7.0e-08,
    "heads_dx": 1.4e-07, "heads_dwm": 6.4e-07, "heads_dws": 5.6e-07, "heads_dbm": 1.4e-07, "heads_dbs": 1.4e-07,
    "sfc_out": 2.1e-07, "sfc_mean": 9.8e-08, "sfc_invstd": 1.2e-07, "sfc_dz": 4.5e-07, "sfc_dw": 4.2e-07,
    "sfc_dbeta": 1.1e-07,
}
SENT = 777.0
NARROW, TILE, SKINNY = 0, 1, 2          # SVAE_HEADS_FWD_*
ROWGROUP, PLAIN, BTILE = 0, 1, 2        # SVAE_HEADS_BWD_*
CLIP, PRIOR = 1.0, 0.5


def _lib():
    return pkg_mod("_lib")


def _u(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).uniform(-1, 1, size=shape) * scale).astype(np.float32))


def _tol(name, base):
    """The project's bound, unless 10x the measured fp32 error is larger (it never is, see the docstring)."""
    return max(base, 10 * MEASURED_F32[name])


def _close(name, got, ref, base):
    got = got.double().cpu() if isinstance(got, torch.Tensor) else got
    err, scale = (got - ref).abs().max().item(), 1 + ref.abs().max().item()
    tol = _tol(name, base)
    print("%-9s max|err| / (1 + max|ref|) = %.3e   (bound %.1e)" % (name, err / scale, tol))
    assert err <= tol * scale, (name, err, scale)


# ------------------------------------------------------------------------------------------------ heads
# (B, K, D, variant, options)
HEADS_FWD = [
    (7, 4, 1, NARROW, dict(nsplit_extra=2)),            # nsplit larger than heads_splits(K)
    (9, 2560, 2, NARROW, dict(groups=3)),               # two splits, the second partial
    (8, 2048, 3, NARROW, {}),
    (33, 6144, 4, NARROW, {}),
    (70, 2088, 5, TILE, dict(coff=3, dz=12)),           # K % 32 != 0, B % 64 != 0; pcols = 2 Dz > 2 D
    (64, 2048, 8, TILE, {}),
    (5, 96, 9, TILE, dict(groups=3)),
    (256, 4096, 30, TILE, {}),
    (3, 40, 32, TILE, {}),
    (6, 2050, 3, SKINNY, {}),                           # K % 4 != 0
    (8, 2048, 3, SKINNY, dict(misalign=1)),             # wm one float off a 16-byte boundary
    (9, 2560, 2, SKINNY, dict(misalign=1, coff=1, dz=4, groups=2)),
]
HEADS_BWD = [
    (32, 100, 3, ROWGROUP, {}),                         # K % 64 != 0
    (128, 2048, 4, ROWGROUP, {}),
    (64, 200, 5, ROWGROUP, dict(coff=2, dz=9)),
    (32, 64, 8, ROWGROUP, dict(groups=3)),
    (7, 300, 2, PLAIN, dict(groups=3)),
    (33, 257, 6, PLAIN, dict(coff=1, dz=8)),
    (70, 2088, 9, BTILE, dict(coff=4, dz=13)),
    (256, 4096, 30, BTILE, {}),
    (5, 40, 32, BTILE, dict(groups=3)),
]


def _hid(c):
    return "B%d-K%d-D%d-%s" % (c[0], c[1], c[2], "-".join("%s%s" % kv for kv in sorted(c[4].items())) or "plain")


def heads_inputs(B, K, D, groups, seed):
    """x uniform(-1, 1); weights scaled by 3 / sqrt(K): the head sums have unit deviation (within +-4)."""
    a = 3.0 / np.sqrt(K)
    return _u((groups, B, K), seed), _u((groups, K, D), seed + 1, a), _u((groups, K, D), seed + 2, a)


def heads_fwd_ref(x, wm, ws):
    return dict(zip(("head_mean", "head_std"), R.heads(x, wm, ws)))


def heads_bwd_inputs(B, K, D, groups, dz, accumulate, seed):
    x, wm, ws = heads_inputs(B, K, D, groups, seed)
    return x, wm, ws, _u((groups, B, 2 * dz), seed + 3), (_u((groups, B, K), seed + 4) if accumulate else None)


def heads_bwd_ref(x, wm, ws, dhead, dx0, D, coff):
    dm, ds = R.head_cols(dhead, D, coff)
    return dict(zip(("heads_dx", "heads_dwm", "heads_dws", "heads_dbm", "heads_dbs"),
                    R.heads_bwd(x, wm, ws, dm, ds, dx0)))


def _wbuf(w, w_gs, mis):
    """The groups' [K, D] weights w_gs elements apart in a sentinel buffer, `mis` floats off its start."""
    g = w.shape[0]
    buf = torch.full((g * w_gs + mis,), SENT, device="cuda")
    v = buf[mis:]
    v.view(g, w_gs)[:, :w[0].numel()] = w.reshape(g, -1).cuda()
    assert v.data_ptr() % 16 == (4 * mis) % 16
    return buf, v


@pytest.mark.parametrize("case", HEADS_FWD, ids=_hid)
def test_heads_fwd(case):
    B, K, D, want, o = case
    groups, coff, dz, mis = o.get("groups", 1), o.get("coff", 0), o.get("dz", D), o.get("misalign", 0)
    L = _lib()
    hs = L.lib().svae_op_heads_splits(K)
    assert hs == -(-K // 2048)
    nsplit, pcols = hs + o.get("nsplit_extra", 0), 2 * dz
    x, wm, ws = heads_inputs(B, K, D, groups, 100)
    ref = heads_fwd_ref(x.double(), wm.double(), ws.double())
    w_gs = (K * D + 3) // 4 * 4 + 4
    xd = x.cuda()
    (_, wmd), (_, wsd) = _wbuf(wm, w_gs, mis), _wbuf(ws, w_gs, 0)

    def run():
        part = torch.full((groups, nsplit, B, pcols), SENT, device="cuda")
        var = ctypes.c_int32(-1)
        L.check(L.lib().svae_op_heads_fwd(L.ptr(xd), B, K, L.ptr(wmd), L.ptr(wsd), w_gs, D, L.ptr(part), nsplit, pcols,
                                          coff, groups, ctypes.byref(var), L.stream_ptr()))
        torch.cuda.synchronize()
        return part, var.value

    part, var = run()
    assert var == want
    own = torch.zeros(nsplit, pcols, dtype=torch.bool)
    own[:hs, coff:coff + D] = True
    own[:hs, dz + coff:dz + coff + D] = True
    p = part.cpu().permute(0, 2, 1, 3)  # [g, B, nsplit, pcols]
    assert (p[:, :, ~own] == SENT).all(), "wrote outside the level's own columns and splits"
    s = p[:, :, :hs].double().sum(2)
    m, sd = R.head_cols(s, D, coff)
    _close("head_mean", m, ref["head_mean"], FWD_TOL)
    _close("head_std", sd, ref["head_std"], FWD_TOL)
    part2, _ = run()
    assert torch.equal(part, part2)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", HEADS_BWD, ids=_hid)
def test_heads_bwd(case, accumulate):
    B, K, D, want, o = case
    groups, coff, dz = o.get("groups", 1), o.get("coff", 0), o.get("dz", D)
    L = _lib()
    x, wm, ws, dhead, dx0 = heads_bwd_inputs(B, K, D, groups, dz, accumulate, 200)
    ref = heads_bwd_ref(x.double(), wm.double(), ws.double(), dhead.double(), None if dx0 is None else dx0.double(),
                        D, coff)
    w_gs = (K * D + 3) // 4 * 4 + 4
    xd, dhd = x.cuda(), dhead.cuda()
    (_, wmd), (_, wsd) = _wbuf(wm, w_gs, 0), _wbuf(ws, w_gs, 0)

    def run():
        dx = dx0.cuda() if accumulate else torch.full((groups, B, K), SENT, device="cuda")
        outs = [torch.full((groups, w_gs), SENT, device="cuda") for _ in range(4)]
        var = ctypes.c_int32(-1)
        L.check(L.lib().svae_op_heads_bwd(L.ptr(xd), L.ptr(dx), B, K, L.ptr(wmd), L.ptr(wsd), w_gs, D, L.ptr(dhd),
                                          2 * dz, coff, *[L.ptr(t) for t in outs], accumulate, groups,
                                          ctypes.byref(var), L.stream_ptr()))
        torch.cuda.synchronize()
        return [dx] + outs, var.value

    got, var = run()
    assert var == want
    dx, dwm, dws, dbm, dbs = got
    _close("heads_dx", dx, ref["heads_dx"], FWD_TOL)
    for name, t, n in (("heads_dwm", dwm, K * D), ("heads_dws", dws, K * D), ("heads_dbm", dbm, D),
                       ("heads_dbs", dbs, D)):
        assert (t[:, n:] == SENT).all(), name + ": wrote past the group's own elements"
        _close(name, t[:, :n].reshape(ref[name].shape), ref[name], SUM_TOL)
    got2, _ = run()
    assert all(torch.equal(a, b) for a, b in zip(got, got2))


# ------------------------------------------------------------------------------------------------ latent
LATENT_DIMS = [(1,), (2, 3, 4), (25, 25, 25, 25), (32, 32, 32, 32, 1), (32,) * 8]  # Dz 1, 9, 100, 129, 256
LATENT_B = [1, 5, 130]
LATENT_NSPLIT = [1, 3, 32, 33, 70]
GROUPS = 2
BIAS_GAP = 3  # floats between the levels' bias tensors (NaN there: a wrong level lookup reads one)


def _on_clip(B, Dz):
    """(group, row, column, sign): means put exactly on the clip bounds."""
    return sorted({(0, 0, 0, 1.0), (1, B - 1, Dz - 1, -1.0), (0, B // 2, Dz // 2, 1.0), (1, B // 3, Dz // 4, -1.0)})


def latent_fwd_inputs(dims, B, nsplit, seed):
    """Partials whose sums have deviation ~1.2 (pre-sigmoid sums within +-4, sig away from 0), mean biases
    that are exact in binary so that a few means can sit exactly on +-clip."""
    Dz = sum(dims)
    part = _u((GROUPS, nsplit, B, 2 * Dz), seed, 2.0 / np.sqrt(nsplit))
    bm = torch.round(_u((GROUPS, Dz), seed + 1, 0.5) * 64) / 64
    bs, eps = _u((GROUPS, Dz), seed + 2, 0.5), _u((GROUPS, B, Dz), seed + 3)
    for g, n, c, sgn in _on_clip(B, Dz):
        part[g, :, n, c] = 0.0
        part[g, 0, n, c] = sgn * CLIP - bm[g, c]
    return part, bm, bs, eps


def _gapped(bias, dims):
    """[groups][Dz] biases in the entry point's layout: level l starts BIAS_GAP floats after level l - 1 ends."""
    out = torch.full((bias.shape[0], sum(dims) + len(dims) * BIAS_GAP), float("nan"))
    o = 0
    for l, d in enumerate(dims):
        out[:, o + l * BIAS_GAP:o + l * BIAS_GAP + d] = bias[:, o:o + d]
        o += d
    return out.cuda()


def latent_fwd_ref(part, bm, bs, eps, uniform):
    return dict(zip(("mu", "sig", "z", "kl_img"), R.latent_fwd(part, bm, bs, eps, CLIP, PRIOR, uniform)))


def latent_bwd_inputs(dims, B, seed):
    Dz = sum(dims)
    mu, sig = _u((GROUPS, B, Dz), seed, 2.0), torch.sigmoid(_u((GROUPS, B, Dz), seed + 1, 4.0))
    for g, n, c, sgn in _on_clip(B, Dz):
        mu[g, n, c] = sgn * CLIP
    return mu, sig, _u((GROUPS, B, Dz), seed + 2), _u((GROUPS, B, Dz), seed + 3), torch.tensor([0.37, 1.3])


def latent_bwd_ref(mu, sig, eps, dz, kc, uniform):
    return {"dhead": R.latent_bwd(mu, sig, eps, dz, kc, CLIP, PRIOR, uniform)}


def _lid(v):
    return "Dz%d" % sum(v) if isinstance(v, tuple) else None


@pytest.mark.parametrize("B", LATENT_B)
@pytest.mark.parametrize("dims", LATENT_DIMS, ids=_lid)
def test_latent_fwd(dims, B):
    L = _lib()
    Dz = sum(dims)
    cdims = (ctypes.c_int32 * len(dims))(*dims)
    for nsplit in LATENT_NSPLIT:
        part, bm, bs, eps = latent_fwd_inputs(dims, B, nsplit, 300 + nsplit)
        pd, bmd, bsd, ed = part.cuda(), _gapped(bm, dims), _gapped(bs, dims), eps.cuda()
        for uniform in (0, 1):
            ref = latent_fwd_ref(part.double(), bm.double(), bs.double(), eps.double(), uniform)
            outside = (ref["mu"].abs() > CLIP).double().mean().item()
            assert outside >= 0.05 or B * Dz < 20, outside

            def run():
                outs = [torch.full((GROUPS, B, Dz), SENT, device="cuda") for _ in range(3)]
                outs.append(torch.full((GROUPS, B), SENT, device="cuda"))
                L.check(L.lib().svae_op_latent_fwd(L.ptr(pd), nsplit, B, len(dims), cdims, L.ptr(bmd), L.ptr(bsd),
                                                   BIAS_GAP, CLIP, PRIOR, uniform, L.ptr(ed),
                                                   *[L.ptr(t) for t in outs], GROUPS, L.stream_ptr()))
                torch.cuda.synchronize()
                return outs

            got = run()
            print("Dz %d B %d nsplit %d uniform %d (%.0f%% of the means outside the clip)"
                  % (Dz, B, nsplit, uniform, 100 * outside))
            for name, t in zip(("mu", "sig", "z", "kl_img"), got):
                _close(name, t, ref[name], FWD_TOL)
            for g, n, c, sgn in _on_clip(B, Dz):  # exactly on the bound, in the kernel as in the reference
                assert got[0][g, n, c].item() == sgn * CLIP == ref["mu"][g, n, c].item()
            assert all(torch.equal(a, b) for a, b in zip(got, run()))


@pytest.mark.parametrize("B", LATENT_B)
@pytest.mark.parametrize("dims", LATENT_DIMS, ids=_lid)
def test_latent_bwd(dims, B):
    L = _lib()
    Dz = sum(dims)
    mu, sig, eps, dz, kc = latent_bwd_inputs(dims, B, 400)
    dev = [t.cuda() for t in (mu, sig, eps, dz, kc)]
    assert (mu.abs() > CLIP).double().mean().item() >= 0.05 or B * Dz < 20
    for uniform in (0, 1):
        ref = latent_bwd_ref(mu.double(), sig.double(), eps.double(), dz.double(), kc.double(), uniform)["dhead"]

        def run():
            dhead = torch.full((GROUPS, B, 2 * Dz), SENT, device="cuda")
            L.check(L.lib().svae_op_latent_bwd(*[L.ptr(t) for t in dev[:4]], B, Dz, L.ptr(dev[4]), PRIOR, uniform, CLIP,
                                               L.ptr(dhead), GROUPS, L.stream_ptr()))
            torch.cuda.synchronize()
            return dhead

        dhead = run()
        print("Dz %d B %d uniform %d" % (Dz, B, uniform))
        _close("dhead", dhead[..., :Dz], ref[..., :Dz], FWD_TOL)   # d raw mean
        _close("dhead", dhead[..., Dz:], ref[..., Dz:], FWD_TOL)   # d pre-sigmoid
        dm = dhead[..., :Dz].cpu()
        assert (dm[mu.abs() > CLIP] == 0).all()
        for g, n, c, _ in _on_clip(B, Dz):  # the gradient passes on the bound (tf.clip_by_value, torch.clamp)
            assert dm[g, n, c].item() != 0 and ref[g, n, c].item() != 0
        assert torch.equal(dhead, run())


# ------------------------------------------------------------------------------------------------ split FC
# (B, K, J, F)
SFC = [(4, 2, 96, 24), (7, 3, 200, 8), (32, 4, 64, 64), (8, 5, 130, 13), (16, 8, 256, 16),
       (4, 30, 96, 24),       # B < 4 KM: the dps tile doubles as the dW reduction buffer
       (128, 9, 100, 10),
       (256, 30, 128, 32)]    # ~100 KB of LDS
# seeds at which no |xhat + beta| of the float64 reference is under 2e-5 (searched on the CPU from 500 up)
SFC_SEED = {(4, 2, 96, 24): 500, (7, 3, 200, 8): 500, (32, 4, 64, 64): 500, (8, 5, 130, 13): 500,
            (16, 8, 256, 16): 500, (4, 30, 96, 24): 500, (128, 9, 100, 10): 500, (256, 30, 128, 32): 520}
KINK = 2e-5
ZOFF, ZPAD = 3, 2


def sfc_geom(B, K, J, F):
    ldz, ldo = ZOFF + K + ZPAD, F + 3
    o_n = (J // F) * ldo + 2
    return ldz, ldo, o_n


def sfc_inputs(B, K, J, F, seed):
    ldz, ldo, o_n = sfc_geom(B, K, J, F)
    return (_u((B, ldz), seed), _u((K, J), seed + 1), _u((J,), seed + 2, 0.5), _u((B * o_n,), seed + 3),
            _u((B, ldz), seed + 4))


def sfc_ref(B, K, J, F, z, w, beta, doutbuf):
    _, ldo, o_n = sfc_geom(B, K, J, F)
    out, mean, inv, y = R.splitfc(z, ZOFF, K, w, beta)
    dout = doutbuf[R.splitfc_offsets(B, J, F, ldo, o_n)]
    dw, dbeta, dzl = R.splitfc_bwd(z, ZOFF, K, w, beta, dout)
    return {"sfc_out": out, "sfc_mean": mean, "sfc_invstd": inv, "sfc_dw": dw, "sfc_dbeta": dbeta, "sfc_dz": dzl,
            "y": y}


def _sfc_fwd(L, zd, wd, bd, B, K, J, F, nt=1, strides=(0, 0, 0, 0)):
    ldz, ldo, o_n = sfc_geom(B, K, J, F)
    mean, inv = (torch.full((nt, J), SENT, device="cuda") for _ in range(2))
    out = torch.full((nt, B * o_n), SENT, device="cuda")
    L.check(L.lib().svae_op_splitfc(L.ptr(zd), ldz, ZOFF, B, K, L.ptr(wd), L.ptr(bd), J, F, ldo, o_n, L.ptr(mean),
                                    L.ptr(inv), L.ptr(out), nt, *strides, L.stream_ptr()))
    torch.cuda.synchronize()
    return out, mean, inv


@pytest.mark.parametrize("case", SFC, ids=lambda c: "B%d-K%d-J%d-F%d" % c)
def test_splitfc_fwd_bwd(case):
    B, K, J, F = case
    L = _lib()
    ldz, ldo, o_n = sfc_geom(B, K, J, F)
    z, w, beta, doutbuf, dz0 = sfc_inputs(B, K, J, F, SFC_SEED[case])
    ref = sfc_ref(B, K, J, F, z.double(), w.double(), beta.double(), doutbuf.double())
    assert ref["y"].abs().min().item() >= KINK, "seed puts a reference element on the lrelu kink"
    off = R.splitfc_offsets(B, J, F, ldo, o_n)
    own = torch.zeros(B * o_n, dtype=torch.bool)
    own[off.reshape(-1)] = True
    zd, wd, bd, dod = z.cuda(), w.cuda(), beta.cuda(), doutbuf.cuda()
    scratch = torch.empty(-(-J // 64) * B * K, device="cuda")

    def run():
        out, mean, inv = _sfc_fwd(L, zd, wd, bd, B, K, J, F)
        dw, dbeta = torch.full((K, J), SENT, device="cuda"), torch.full((J,), SENT, device="cuda")
        dz = dz0.cuda()
        L.check(L.lib().svae_op_splitfc_bwd(L.ptr(zd), ldz, ZOFF, B, K, L.ptr(wd), L.ptr(bd), J, F, ldo, o_n,
                                            L.ptr(mean), L.ptr(inv), L.ptr(dod), L.ptr(dw), L.ptr(dbeta), L.ptr(dz),
                                            L.ptr(scratch), scratch.numel() * 4, L.stream_ptr()))
        torch.cuda.synchronize()
        return out[0], mean[0], inv[0], dw, dbeta, dz

    got = run()
    out, mean, inv, dw, dbeta, dz = (t.cpu() for t in got)
    assert (out[~own] == SENT).all(), "wrote outside the level's place in the concat buffer"
    _close("sfc_out", out[off], ref["sfc_out"], FWD_TOL)
    _close("sfc_mean", mean, ref["sfc_mean"], FWD_TOL)
    _close("sfc_invstd", inv, ref["sfc_invstd"], FWD_TOL)
    _close("sfc_dw", dw, ref["sfc_dw"], SUM_TOL)
    _close("sfc_dbeta", dbeta, ref["sfc_dbeta"], SUM_TOL)
    want_dz = dz0.double()
    want_dz[:, ZOFF:ZOFF + K] += ref["sfc_dz"]
    lvl = torch.zeros(ldz, dtype=torch.bool)
    lvl[ZOFF:ZOFF + K] = True
    assert torch.equal(dz[:, ~lvl], dz0[:, ~lvl]), "dz changed outside the level's columns"
    _close("sfc_dz", dz, want_dz, FWD_TOL)
    assert all(torch.equal(a, b) for a, b in zip(got, run()))


@pytest.mark.parametrize("case", [SFC[1], SFC[3], SFC[6]], ids=lambda c: "B%d-K%d-J%d-F%d" % c)
def test_splitfc_steps_launch_is_bitwise_the_single_launches(case):
    """nt = 3 through splitfc_fwd_steps (grid.y = step) against three splitfc_fwd launches."""
    B, K, J, F = case
    L = _lib()
    ldz, _, o_n = sfc_geom(B, K, J, F)
    nt = 3
    z, w, beta = _u((nt, B, ldz), 600), _u((nt, K, J), 601), _u((nt, J), 602, 0.5)
    zd, wd, bd = z.cuda(), w.cuda(), beta.cuda()
    out, mean, inv = _sfc_fwd(L, zd, wd, bd, B, K, J, F, nt, (B * ldz, K * J, J, B * o_n))
    assert not (mean == SENT).any()
    for i in range(nt):
        o1, m1, i1 = _sfc_fwd(L, zd[i], wd[i], bd[i], B, K, J, F)
        assert torch.equal(o1[0], out[i]) and torch.equal(m1[0], mean[i]) and torch.equal(i1[0], inv[i])
        ref = R.splitfc(z[i].double(), ZOFF, K, w[i].double(), beta[i].double())
        _close("sfc_mean", mean[i], ref[1], FWD_TOL)


# ------------------------------------------------------------------------------------------------ rejections
EBADARG = -2


def _t(n=64):
    return torch.zeros(n, device="cuda")


def test_heads_splits_is_the_chunk_count():
    lib = _lib().lib()
    assert [lib.svae_op_heads_splits(k) for k in (1, 2048, 2049, 65536)] == [1, 1, 2, 32]
    assert lib.svae_op_heads_splits(0) == EBADARG


def _reject(fn, args, bad):
    """The good call returns 0; with one argument replaced it returns SVAE_EBADARG (and launches nothing)."""
    L = _lib()
    assert getattr(L.lib(), fn)(*args.values()) == 0
    args = dict(args)
    assert set(bad) <= set(args)
    args.update(bad)
    assert getattr(L.lib(), fn)(*args.values()) == EBADARG
    torch.cuda.synchronize()


def _p(n=64, fill=0.0):
    """Device pointer of a fresh buffer (kept alive by the returned object's owner list)."""
    t = torch.full((n,), fill, device="cuda")
    _KEEP.append(t)
    return _lib().ptr(t)


_KEEP = []


@pytest.fixture(autouse=True)
def _drop_buffers():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


@pytest.mark.parametrize("bad", [dict(x=None), dict(part=None), dict(b=0), dict(k=-1), dict(d=0), dict(d=33, pcols=66),
                                 dict(groups=0), dict(k=2049, nsplit=1), dict(coff=1), dict(pcols=5)], ids=str)
def test_heads_fwd_rejects(bad):
    """null, non-positive, d > 32, nsplit < heads_splits(k), columns that do not fit pcols / 2."""
    L = _lib()
    _reject("svae_op_heads_fwd", dict(x=_p(4096), b=2, k=4, wm=_p(), ws=_p(), w_gs=0, d=2, part=_p(), nsplit=1, pcols=4,
                                      coff=0, groups=1, variant=None, stream=L.stream_ptr()), bad)


@pytest.mark.parametrize("bad", [dict(dx=None), dict(dbs=None), dict(b=0), dict(k=0), dict(d=33, dcols=66),
                                 dict(groups=-1), dict(coff=1)], ids=str)
def test_heads_bwd_rejects(bad):
    L = _lib()
    _reject("svae_op_heads_bwd", dict(x=_p(), dx=_p(), b=2, k=4, wm=_p(), ws=_p(), w_gs=0, d=2, dhead=_p(), dcols=4,
                                      coff=0, dwm=_p(), dws=_p(), dbm=_p(), dbs=_p(), accumulate=0, groups=1,
                                      variant=None, stream=L.stream_ptr()), bad)


def _dims(*v):
    return (ctypes.c_int32 * 8)(*v)


@pytest.mark.parametrize("bad", [dict(part=None), dict(kl_img=None), dict(nsplit=0), dict(b=0), dict(levels=0),
                                 dict(levels=9), dict(dims=_dims(*[33] * 8), levels=8), dict(dims=_dims(0, 1)),
                                 dict(groups=0), dict(bias_gap=-1)], ids=lambda b: "-".join(b))
def test_latent_fwd_rejects(bad):
    """Dz = 8 x 33 = 264 > 256 is the documented limit; the rest are null or non-positive arguments."""
    L = _lib()
    _reject("svae_op_latent_fwd", dict(part=_p(4096), nsplit=1, b=2, levels=2, dims=_dims(1, 2), bm=_p(), bs=_p(),
                                       bias_gap=0, clip=CLIP, prior=PRIOR, uniform=0, eps=_p(), mu=_p(), sig=_p(),
                                       z=_p(), kl_img=_p(), groups=1, stream=L.stream_ptr()), bad)


@pytest.mark.parametrize("bad", [dict(mu=None), dict(dhead=None), dict(b=0), dict(Dz=0), dict(Dz=257), dict(groups=0)],
                         ids=str)
def test_latent_bwd_rejects(bad):
    L = _lib()
    _reject("svae_op_latent_bwd", dict(mu=_p(), sig=_p(fill=0.5), eps=_p(), dz=_p(), b=2, Dz=3, kl_coef=_p(),
                                       prior=PRIOR, uniform=0, clip=CLIP, dhead=_p(), groups=1,
                                       stream=L.stream_ptr()), bad)


def _sfc_good(L):
    z = torch.arange(64.0, device="cuda") % 7  # (a batch with some variance: any finite input does)
    _KEEP.append(z)
    return dict(z=L.ptr(z), ldz=4, zoff=1, b=2, k=3, w=_p(fill=0.5), beta=_p(), j=8, f=4, ldo=4, o_n=8, mean=_p(),
                invstd=_p())


@pytest.mark.parametrize("bad", [dict(z=None), dict(out=None), dict(b=0), dict(k=0), dict(k=33, ldz=40), dict(j=0),
                                 dict(f=0), dict(nt=0), dict(nt=17), dict(ldz=3)], ids=str)
def test_splitfc_rejects(bad):
    L = _lib()
    a = _sfc_good(L)
    a.update(out=_p(), nt=1, z_ts=0, w_ts=0, bn_ts=0, out_ts=0, stream=L.stream_ptr())
    _reject("svae_op_splitfc", a, bad)


@pytest.mark.parametrize("bad", [dict(dout=None), dict(scratch=None), dict(b=0), dict(k=33, ldz=40), dict(j=-1),
                                 dict(scratch_bytes=2 * 3 * 4 - 1)], ids=str)
def test_splitfc_bwd_rejects(bad):
    L = _lib()
    a = _sfc_good(L)
    a.update(mean=_p(), invstd=_p(fill=1.0), dout=_p(), dw=_p(), dbeta=_p(), dz=_p(), scratch=_p(),
             scratch_bytes=2 * 3 * 4, stream=L.stream_ptr())
    _reject("svae_op_splitfc_bwd", a, bad)
