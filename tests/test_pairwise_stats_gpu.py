"""svae_op_pairwise_stats on the GPU against tests/quality_ref.py (numpy float64, the direct form sum (x - y)^2).

Bounds (derived from the op's stated numerics, not tuned).  The op forms d2 = a_i + b_j - 2 g_ij with g the fp32
inner product on the fp32 MFMA (exact products, a chain of d fp32 additions: relative to sum_k |x_ik y_jk| its error
is at most gamma_d <= (d + 2) u, u = 2^-24, and the factor 2 doubles it) and a, b the squared norms in fp64 (the
combination and the norms: a few 2^-53 of a_i + b_j).  So per pair

    tau_ij = 2 (d + 2) u sum_k |x_ik y_jk| + 4 2^-53 (a_i + b_j)

and   |nn_d2 - ref| <= tau of the reference minimiser,
      nn_idx names an admitted column whose reference d2 <= reference minimum + 2 max_j tau_ij,
      |ksum - ref| <= sum_j k_ij (exp(tau_ij inv_two_sigma2) - 1) + 1e-12 ref      (fp64 exp and summation).
Every case prints its error over the bound.  gamma_d is the worst case: no input may exceed it.

Shapes (n, [m_g], d), with R, C, K the op's exported tiles: (1, [1], 1), (5, [3, 4], 7), (R - 1, [C + 1], K + 1),
(R + 1, [C - 1, 1, C + 3], K - 1), (2 R + 1, [2 C + 1, C], 48), (70, [70 self, 33], 3072), (40, [40 self], 12288);
and the two sides of the op's grid threshold: below FILL = 256 blocks of R x C it takes row tiles of 32, from there on
of R, so (R + 1, [126 C + 5], K + 1) (2 x 127 blocks: the small row tile, as every shape above) and (R + 1,
[127 C + 1], K + 1) (2 x 128 blocks: the R-row tile), whose row slices (small grids) must give the full call's bytes.
Each runs with 1, 5 and 8 bandwidths spanning sigma^2 = 1e-2 .. 1e2 times the mean d2 and with ksum only, the
nearest neighbour only, and both.  Inputs have leading dimensions above d with NaN in the gaps, bases off 16-byte
alignment and NaN / 1e30 guard bands; every output sits between sentinel rows.  Data: N(0, 1) rows; row 0 of every
group without the offset is x's row 0 (d2 = 0 after the clamp), its row 1 is x's row 1 with one element moved by
2^-10; "far": the last group is offset by +8 in every element (large norms); "near": x and every group are offset by
+8 (large norms, small differences: the cancellation case).
"""
import ctypes

import numpy as np
import pytest
import torch

import quality_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

R, C, K = 128, 128, 32  # SVAE_PAIRWISE_TILE_ROWS, _COLS, _K: asserted below
GUARD = 256
SENTINEL = -12345.678
U = 2.0 ** -24
# (n, [m_g], d, self group, offset)
SHAPES = [(1, (1,), 1, None, None), (5, (3, 4), 7, None, None), (R - 1, (C + 1,), K + 1, None, None),
          (R + 1, (C - 1, 1, C + 3), K - 1, None, "far"), (2 * R + 1, (2 * C + 1, C), 48, None, "near"),
          (70, (70, 33), 3072, 0, "far"), (40, (40,), 12288, 0, "near"),
          (R + 1, (126 * C + 5,), K + 1, None, None), (R + 1, (127 * C + 1,), K + 1, None, None)]
IDS = ["%dx%sx%d" % (n, "+".join(map(str, m)), d) for n, m, d, _, _ in SHAPES]
N_BW = [1, 5, 8]
MODES = ["ksum", "nn", "both"]


def _data(n, ms, d, self_group, offset):
    rng = np.random.default_rng(1000003 * n + 1009 * sum(ms) + d)
    x = rng.normal(0, 1, (n, d)).astype(np.float32)
    groups = []
    for g, m in enumerate(ms):
        if g == self_group:
            groups.append(x)
            continue
        y = rng.normal(0, 1, (m, d)).astype(np.float32)
        if not (offset == "far" and g == len(ms) - 1):
            y[0] = x[0]
            if m > 1 and n > 1:
                y[1] = x[1]
                y[1, 0] += np.float32(2.0 ** -10)
        groups.append(y)
    if offset == "far":
        groups[-1] = groups[-1] + np.float32(8.0)
    if offset == "near":  # in place: the self group stays x itself
        x += np.float32(8.0)
        for g, y in enumerate(groups):
            if g != self_group:
                y += np.float32(8.0)
    return x, groups


def _device(a, ld, shift):
    """a [n, d] on the device with rows ld floats apart (NaN in the gaps), between guard bands of NaN / 1e30, the
    base ``shift`` floats off 16-byte alignment.  Returns (view, buffer, host image of the buffer)."""
    n, d = a.shape
    body = np.full((n, ld), np.nan, np.float32)
    body[:, :d] = a
    host = np.empty(GUARD + shift + n * ld + GUARD, np.float32)
    host[0::2], host[1::2] = np.nan, 1e30
    host[GUARD + shift:GUARD + shift + n * ld] = body.ravel()
    buf = torch.from_numpy(host.copy()).cuda()
    view = buf[GUARD + shift:].as_strided((n, d), (ld, 1))
    assert (view.data_ptr() % 16 == 0) == (shift % 4 == 0)
    return view, buf, host


def _run(xd, gd, bw, self_group, mode="both", extra=2):
    """The op through quality.pairwise_stats into outputs with sentinel rows around them; numpy arrays or None."""
    Qm = pkg_mod("quality")
    n, G, nb = xd.shape[0], len(gd), len(bw)
    bufs = {"ksum": torch.full((extra + n + extra, G, max(nb, 1)), SENTINEL, dtype=torch.float64, device="cuda"),
            "nn_d2": torch.full((extra + n + extra, G), SENTINEL, dtype=torch.float64, device="cuda"),
            "nn_idx": torch.full((extra + n + extra, G), -777, dtype=torch.int64, device="cuda")}
    got = Qm.pairwise_stats(xd, gd, bw, self_group=self_group, out={k: v[extra:] for k, v in bufs.items()},
                            ksum=mode != "nn", nn=mode != "ksum")
    res = []
    for key, t, sent in zip(("ksum", "nn_d2", "nn_idx"), got, (SENTINEL, SENTINEL, -777)):
        host = bufs[key].cpu().numpy()
        if t is None:
            assert np.all(host == sent)  # a skipped part writes nothing
            res.append(None)
            continue
        assert t.data_ptr() == bufs[key][extra].data_ptr()
        flat = host.reshape(-1)
        used = t.numel()
        lead = extra * host[0].size
        assert np.all(flat[:lead] == sent) and np.all(flat[lead + used:] == sent)
        res.append(flat[lead:lead + used].reshape(tuple(t.shape)).copy())
    return res


def _bandwidths(mean_d2, nb):
    return [mean_d2] if nb == 1 else list(mean_d2 * np.logspace(-2, 2, nb))


@pytest.fixture(scope="module")
def cases():
    """Per shape: host data, device views (shared, never modified), the reference d2 and tau per group."""
    L = pkg_mod("_lib")
    assert (L.PAIRWISE_TILE_ROWS, L.PAIRWISE_TILE_COLS, L.PAIRWISE_TILE_K) == (R, C, K)
    assert (L.PAIRWISE_MAX_GROUPS, L.PAIRWISE_MAX_BW) == (4, 8)
    out = {}
    for sid, (n, ms, d, sg, offset) in zip(IDS, SHAPES):
        x, groups = _data(n, ms, d, sg, offset)
        xd, xbuf, xhost = _device(x, d + 3, 1)
        gd, keep = [], [(xbuf, xhost)]
        for g, y in enumerate(groups):
            if g == sg:
                gd.append(xd)
                continue
            yd, ybuf, yhost = _device(y, d + 5, 2 + g % 2)
            gd.append(yd)
            keep.append((ybuf, yhost))
        x64 = x.astype(np.float64)
        d2s, taus, oks = [], [], []
        for g, y in enumerate(groups):
            y64 = y.astype(np.float64)
            d2s.append(quality_ref.sqdist(x, y))
            a, b = np.square(x64).sum(1), np.square(y64).sum(1)
            taus.append(2.0 * (d + 2) * U * (np.abs(x64) @ np.abs(y64).T) + 4.0 * 2.0 ** -53 * (a[:, None] + b[None, :]))
            ok = np.ones(d2s[-1].shape, bool)
            if g == sg:
                ok[np.arange(n), np.arange(n)] = False
            oks.append(ok)
        mean_d2 = float(np.mean(np.concatenate([v.ravel() for v in d2s])))
        mean_d2 = mean_d2 if mean_d2 > 0 else 1.0
        out[sid] = dict(x=x, groups=groups, xd=xd, gd=gd, keep=keep, d2=d2s, tau=taus, ok=oks, mean_d2=mean_d2, sg=sg,
                        runs={})
    yield out
    for k in out.values():  # the inputs and their bands are untouched by every call of the module
        for buf, host in k["keep"]:
            assert np.array_equal(buf.cpu().numpy(), host, equal_nan=True)


def _result(k, nb, mode):
    key = (nb, mode)
    if key not in k["runs"]:
        k["runs"][key] = _run(k["xd"], k["gd"], _bandwidths(k["mean_d2"], nb), k["sg"], mode)
    return k["runs"][key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nb", N_BW)
@pytest.mark.parametrize("sid", IDS)
def test_matches_the_reference(cases, sid, nb, mode):
    k = cases[sid]
    bw = _bandwidths(k["mean_d2"], nb)
    ksum, nn_d2, nn_idx = _result(k, nb, mode)
    assert (ksum is None) == (mode == "nn") and (nn_d2 is None) == (mode == "ksum") == (nn_idx is None)
    n = k["x"].shape[0]
    worst_k = worst_d = 0.0
    for g, (d2, tau, ok) in enumerate(zip(k["d2"], k["tau"], k["ok"])):
        if ksum is not None:
            for l, s2 in enumerate(bw):
                inv = 0.5 / s2
                kij = np.where(ok, np.exp(-d2 * inv), 0.0)
                want = kij.sum(1)
                bound = (kij * np.expm1(tau * inv)).sum(1) + 1e-12 * want
                err = np.abs(ksum[:, g, l] - want)
                assert np.all(np.isfinite(ksum[:, g, l]))
                worst_k = max(worst_k, float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0)
                assert np.all(err <= bound), (g, l, float(err.max()))
        if nn_d2 is not None:
            masked = np.where(ok, d2, np.inf)
            has = ok.any(1)
            assert np.all(nn_idx[~has, g] == -1) and np.all(nn_d2[~has, g] == np.inf)
            rows = np.flatnonzero(has)
            if rows.size:
                jref = masked[rows].argmin(1)
                ref_min = masked[rows, jref]
                bound = tau[rows, jref]
                err = np.abs(nn_d2[rows, g] - ref_min)
                assert np.all(nn_d2[rows, g] >= 0.0)  # clamped
                worst_d = max(worst_d, float((err / bound).max()))
                assert np.all(err <= bound), (g, float(err.max()))
                j = nn_idx[rows, g]
                assert np.all((j >= 0) & (j < d2.shape[1])) and np.all(ok[rows, j])
                slack = 2.0 * np.where(ok, tau, 0.0)[rows].max(1)
                assert np.all(d2[rows, j] <= ref_min + slack), g
    print("%s, %d bandwidths, %s: max error / bound: ksum %.3e, nn_d2 %.3e" % (sid, nb, mode, worst_k, worst_d))
    if mode != "both":  # a part computed alone has the bytes it has beside the other
        both = _result(k, nb, "both")
        for a, b in zip((ksum, nn_d2, nn_idx), both):
            assert a is None or a.tobytes() == b.tobytes()


@pytest.mark.parametrize("sid", [IDS[1], IDS[3], IDS[5]])
def test_duplicates_and_near_duplicates(cases, sid):
    """x's row 0 sits in the groups without offset: the computed d2 is clamped at 0 from below and within tau of
    0; row 1 against its copy moved by 2^-10 in one element stays within tau of 2^-20."""
    k = cases[sid]
    _, nn_d2, _ = _result(k, 5, "both")
    for g, (d2, tau) in enumerate(zip(k["d2"], k["tau"])):
        if g == k["sg"] or d2[0, 0] != 0.0:
            continue
        assert 0.0 <= nn_d2[0, g] <= tau[0, 0]
        if d2.shape[1] > 1:
            assert d2[1, 1] == 2.0 ** -20 and abs(nn_d2[1, g] - d2[1, 1]) <= tau[1, 1]


@pytest.mark.parametrize("sid", [IDS[1], IDS[4], IDS[5], IDS[7], IDS[8]])
def test_two_calls_and_a_slice_of_the_rows_give_the_same_bytes(cases, sid):
    k = cases[sid]
    bw = _bandwidths(k["mean_d2"], 5)
    full = _result(k, 5, "both")
    again = _run(k["xd"], k["gd"], bw, k["sg"])
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()
    # row independence, without self exclusion: rows [3, 3 + r) alone, from a dense aligned copy as well
    n = k["x"].shape[0]
    free = _run(k["xd"], k["gd"], bw, None)
    for a, b in ((3, 4), (3, min(n, 3 + 66)), (3, n)):
        part = _run(k["xd"][a:b], k["gd"], bw, None)
        for p, f in zip(part, free):
            assert p.tobytes() == f[a:b].tobytes(), (a, b)
    dense = _run(torch.from_numpy(k["x"][3:]).cuda(), [torch.from_numpy(y).cuda() for y in k["groups"]], bw, None)
    for p, f in zip(dense, free):
        assert p.tobytes() == f[3:].tobytes()


def test_a_nan_spoils_only_the_rows_and_columns_that_read_it(cases):
    k = cases[IDS[1]]  # (5, [3, 4], 7)
    bw = _bandwidths(k["mean_d2"], 5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    base = _run(dev(k["x"]), [dev(y) for y in k["groups"]], bw, None)
    for bad in (np.nan, np.inf):
        x = k["x"].copy()
        x[2, 4] = bad
        got = _run(dev(x), [dev(y) for y in k["groups"]], bw, None)
        assert not np.any(np.isfinite(got[0][2])) and not np.any(np.isfinite(got[1][2]))
        rest = [0, 1, 3, 4]
        for a, b in zip(got, base):
            assert a[rest].tobytes() == b[rest].tobytes()
        y1 = k["groups"][1].copy()
        y1[3, 0] = bad
        got = _run(dev(k["x"]), [dev(k["groups"][0]), dev(y1)], bw, None)
        assert not np.any(np.isfinite(got[0][:, 1]))  # every row's sum over group 1 reads column 3
        assert not np.any(np.isfinite(got[1][:, 1]))
        for a, b in zip(got, base):
            assert a[:, 0].tobytes() == b[:, 0].tobytes()


def test_bad_arguments_return_their_code_without_a_launch(cases):
    L = pkg_mod("_lib")
    k = cases[IDS[1]]
    x = torch.from_numpy(k["x"]).cuda()
    ys = [torch.from_numpy(y).cuda() for y in k["groups"]]
    n, d = x.shape
    ksum = torch.full((n, 2, 2), SENTINEL, dtype=torch.float64, device="cuda")
    nd = torch.full((n, 2), SENTINEL, dtype=torch.float64, device="cuda")
    ni = torch.full((n, 2), -777, dtype=torch.int64, device="cuda")
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)
    f64s = lambda *v: (ctypes.c_double * len(v))(*v)
    ptrs = lambda *t: (ctypes.c_void_p * len(t))(*[None if v is None else v.data_ptr() for v in t])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = L.lib()
    need = lib.svae_op_pairwise_scratch_bytes(n, i64s(3, 4), 2, 2)
    assert need > 0
    scratch = torch.zeros(max(need, 1 << 16), dtype=torch.uint8, device="cuda")
    ok = dict(x=p(x), n=n, ldx=d, y=ptrs(*ys), m=i64s(3, 4), ldy=i64s(d, d), n_groups=2, d=d, self_group=-1,
              inv=f64s(0.5, 0.01), n_bw=2, ksum=p(ksum), nn_d2=p(nd), nn_idx=p(ni), scratch=p(scratch))
    order = ["x", "n", "ldx", "y", "m", "ldy", "n_groups", "d", "self_group", "inv", "n_bw", "ksum", "nn_d2", "nn_idx",
             "scratch"]

    def rc(**over):
        a = dict(ok, **over)
        return lib.svae_op_pairwise_stats(*[a[name] for name in order], L.stream_ptr())

    EBADCONFIG, EBADARG = -1, -2
    five = dict(y=ptrs(*([ys[0]] * 5)), m=i64s(*([3] * 5)), ldy=i64s(*([d] * 5)), n_groups=5)
    for over in (dict(x=None), dict(y=None), dict(m=None), dict(ldy=None), dict(y=ptrs(ys[0], None)), dict(inv=None),
                 dict(scratch=None), dict(n=0), dict(n=-3), dict(d=0), dict(n_groups=0), dict(m=i64s(3, 0)),
                 dict(m=i64s(-1, 4)), dict(ldx=d - 1), dict(ldy=i64s(d, d - 1)), dict(n_bw=-1),
                 dict(n_bw=0), dict(n_bw=2, ksum=None, nn_d2=None, nn_idx=None), dict(nn_d2=None), dict(nn_idx=None),
                 dict(inv=f64s(0.5, 0.0)), dict(inv=f64s(-1.0, 0.5)), dict(inv=f64s(float("nan"), 0.5)),
                 dict(inv=f64s(0.5, float("inf"))), dict(self_group=2), dict(self_group=0),  # x != y[0], n != m[0]
                 dict(self_group=1, y=ptrs(ys[0], x), m=i64s(3, 4))):                          # x == y[1], n != m[1]
        assert rc(**over) == EBADARG, over
        assert b"pairwise_stats" in lib.svae_last_error(None)
    for over in (five, dict(inv=f64s(*([0.5] * 9)), n_bw=9)):
        assert rc(**over) == EBADCONFIG, over
    assert lib.svae_op_pairwise_scratch_bytes(n, i64s(3, 4), 5, 2) == -1
    torch.cuda.synchronize()
    assert torch.all(ksum == SENTINEL) and torch.all(nd == SENTINEL) and torch.all(ni == -777)
    assert rc() == 0  # the same arguments, unspoilt, run
    torch.cuda.synchronize()
    want_k, want_d, want_i, _ = quality_ref.pairwise_stats(k["x"], k["groups"], [1.0, 50.0])
    np.testing.assert_allclose(ksum.cpu().numpy(), want_k, rtol=1e-4)
    np.testing.assert_allclose(nd.cpu().numpy(), want_d, rtol=1e-4, atol=1e-5)
    # the Python wrapper refuses what the op cannot take
    Qm = pkg_mod("quality")
    with pytest.raises(ValueError):
        Qm.pairwise_stats(x.double(), ys, [1.0])
    with pytest.raises(ValueError):
        Qm.pairwise_stats(x.t(), ys, [1.0])
    with pytest.raises(ValueError):
        Qm.pairwise_stats(x, [ys[0][:, :d - 1]], [1.0])
    with pytest.raises(RuntimeError, match="pairwise_stats"):
        Qm.pairwise_stats(x, ys, [-1.0])
    with pytest.raises(RuntimeError, match="pairwise_stats"):
        Qm.pairwise_stats(x, ys, [1.0], self_group=0)
