"""svae_op_pairwise_knn on the GPU against tests/manifold_ref.py (numpy float64, the direct form sum (x - y)^2).

Bounds (derived from the op's stated numerics, not tuned).  The op's d2 is svae_op_pairwise_stats' own, so per pair
it is within

    tau_ij = 2 (d + 2) u sum_k |x_ik y_jk| + 4 2^-53 (a_i + b_j)          (u = 2^-24)

of the reference (tests/test_pairwise_stats_gpu.py derives it).  From that:
  * an order statistic is 1-Lipschitz in the max norm, and only columns that can reach the s-th place matter:
    |knn_d2[i][g][s] - ref_s| <= max tau_ij over the admitted columns whose reference d2 <= ref_s + 2 max_j tau_ij;
  * a count is bracketed by the pairs the reference decides:
    #{ref d2 <= r^2 - tau} <= inside <= #{ref d2 <= r^2 + tau};
  * an interval that wide could hide a failure, so the share of undecided (pair, radius) entries, |ref d2 - r^2| <=
    tau, is capped from the reference alone: 0.1 % for d <= 48, 1 % for d = 3072, 5 % for d = 12288 without offset.
    (12288 "near", large norms and small differences, leaves nearly every pair undecided: it is kept for knn_d2 only.)
Every case prints its error over the bound.

Radii: per group [m_g][4] squared radii, the reference distance of each of the group's own points to its k-th nearest
other point times 1.02 (the factor keeps the group's own pairs off the boundary) for k = 1, 3, 5, NaN where the
group has no more than k points (a NaN radius admits nothing), and one column of +inf (admits every finite d2).
n_radii = 1 takes the first column.  The k-th radii of the two large groups come from a chunked float64 Gram form
(they are inputs of the test, not expectations).

Shapes (n, [m_g], d), with R, C, K the op's exported tiles: (1, [1], 1), (5, [3, 4], 7), (R - 1, [C + 1], K + 1),
(R + 1, [C - 1, 1, C + 3], K - 1) "far", (2 R + 1, [2 C + 1, C], 48) "near", (70, [70 self, 33], 3072),
(40, [40 self], 12288), the same "near", and the two sides of the grid threshold (below FILL = 256 blocks of R x C
the op takes row tiles of 32): (R + 1, [126 C + 5], K + 1) and (R + 1, [127 C + 1], K + 1).  Each runs with k in
{1, 3, 8} and n_radii in {0, 1, 4}, and with the counts alone (k = 0).  Inputs have leading dimensions above d with
NaN in the gaps, bases off 16-byte alignment and NaN / 1e30 guard bands; every output sits between sentinel rows; the
inputs are compared with their host images at module teardown.  The data are test_pairwise_stats_gpu.py's.
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
ISENT = -777
U = 2.0 ** -24
KMAX, RMAX = 8, 4  # SVAE_KNN_MAX_K, _MAX_RADII: asserted below
RADII_K = (1, 3, 5)
# (n, [m_g], d, self group, offset)
SHAPES = [(1, (1,), 1, None, None), (5, (3, 4), 7, None, None), (R - 1, (C + 1,), K + 1, None, None),
          (R + 1, (C - 1, 1, C + 3), K - 1, None, "far"), (2 * R + 1, (2 * C + 1, C), 48, None, "near"),
          (70, (70, 33), 3072, 0, None), (40, (40,), 12288, 0, None), (40, (40,), 12288, 0, "near"),
          (R + 1, (126 * C + 5,), K + 1, None, None), (R + 1, (127 * C + 1,), K + 1, None, None)]
IDS = ["%dx%sx%d%s" % (n, "+".join(map(str, m)), d, "-" + o if o else "") for n, m, d, _, o in SHAPES]
COUNTED = [sid for sid, s in zip(IDS, SHAPES) if not (s[2] == 12288 and s[4] == "near")]
KS = [1, 3, 8]
NRS = [0, 1, 4]


def _cap(d):
    return 0.001 if d <= 48 else 0.01 if d == 3072 else 0.05


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


def _self_radii(y):
    """[m, 4] float64: 1.02 times the squared distance to the k-th nearest other point for k in RADII_K (NaN where
    m <= k), then +inf."""
    m = y.shape[0]
    out = np.full((m, RMAX), np.nan)
    out[:, 3] = np.inf
    cols = [k - 1 for k in RADII_K if m > k]
    if not cols:
        return out
    y64 = y.astype(np.float64)
    for r0 in range(0, m, 1024):
        r1 = min(m, r0 + 1024)
        if m <= 1024:
            d2 = quality_ref.sqdist(y[r0:r1], y)
        else:
            nrm = np.square(y64).sum(1)
            d2 = np.maximum(nrm[r0:r1, None] + nrm[None, :] - 2.0 * (y64[r0:r1] @ y64.T), 0.0)
        d2[np.arange(r1 - r0), np.arange(r0, r1)] = np.inf
        near = np.sort(np.partition(d2, cols[-1], axis=1)[:, :cols[-1] + 1], 1)  # the cols[-1] + 1 smallest, in order
        out[r0:r1, :len(cols)] = 1.02 * near[:, cols]
    return out


def _run(xd, gd, k, radii, self_group, extra=2):
    """The op through quality.knn_stats into outputs with sentinel rows around them: (knn_d2, inside, nonfinite) as
    numpy arrays, None for a skipped part."""
    Qm = pkg_mod("quality")
    n, G = xd.shape[0], len(gd)
    nr = 0 if radii is None else max(r.shape[1] for r in radii if r is not None)
    bufs = {"knn_d2": torch.full((extra + n + extra, G, max(k, 1)), SENTINEL, dtype=torch.float64, device="cuda"),
            "inside": torch.full((extra + n + extra, G, max(nr, 1)), ISENT, dtype=torch.int64, device="cuda"),
            "nonfinite": torch.full((extra + n + extra, G), ISENT, dtype=torch.int64, device="cuda")}
    got = Qm.knn_stats(xd, gd, k, radii=radii, self_group=self_group, out={k_: v[extra:] for k_, v in bufs.items()})
    res = []
    for key, t, sent in zip(("knn_d2", "inside", "nonfinite"), got, (SENTINEL, ISENT, ISENT)):
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


@pytest.fixture(scope="module")
def cases():
    """Per shape: host data, device views and radii (shared, never modified) and, per group, what the reference
    says: the 8 smallest admitted d2 and their bounds, the count brackets and the undecided share."""
    L = pkg_mod("_lib")
    assert (L.PAIRWISE_TILE_ROWS, L.PAIRWISE_TILE_COLS, L.PAIRWISE_TILE_K) == (R, C, K)
    assert (L.PAIRWISE_MAX_GROUPS, L.KNN_MAX_K, L.KNN_MAX_RADII) == (4, KMAX, RMAX)
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
        radii = [_self_radii(y) for y in groups]
        rd4 = [torch.from_numpy(r).cuda() for r in radii]
        rd1 = [torch.from_numpy(np.ascontiguousarray(r[:, :1])).cuda() for r in radii]
        keep += [(t, r) for t, r in zip(rd4, radii)] + [(t, r[:, :1]) for t, r in zip(rd1, radii)]
        ref = []
        undecided = entries = 0
        for g, y in enumerate(groups):
            y64 = y.astype(np.float64)
            d2 = quality_ref.sqdist(x, y)
            a, b = np.square(x64).sum(1), np.square(y64).sum(1)
            tau = 2.0 * (d + 2) * U * (np.abs(x64) @ np.abs(y64).T) + 4.0 * 2.0 ** -53 * (a[:, None] + b[None, :])
            ok = np.ones(d2.shape, bool)
            if g == sg:
                ok[np.arange(n), np.arange(n)] = False
            masked = np.where(ok, d2, np.inf)
            top = np.full((n, KMAX), np.inf)
            s = np.sort(masked, 1)[:, :KMAX]
            top[:, :s.shape[1]] = s
            tmax = np.where(ok, tau, 0.0).max(1)
            bound = np.zeros((n, KMAX))
            for s_ in range(KMAX):
                cand = ok & (d2 <= (top[:, s_] + 2.0 * tmax)[:, None])
                bound[:, s_] = np.where(cand, tau, 0.0).max(1)
            r = radii[g]
            with np.errstate(invalid="ignore"):
                lo = (ok[:, :, None] & (d2[:, :, None] <= r[None] - tau[:, :, None])).sum(1)
                hi = (ok[:, :, None] & (d2[:, :, None] <= r[None] + tau[:, :, None])).sum(1)
                fin = np.isfinite(r)
                undecided += int((ok[:, :, None] & fin[None] & (np.abs(d2[:, :, None] - r[None]) <= tau[:, :, None])).sum())
            entries += int((ok[:, :, None] & fin[None]).sum())
            ref.append(dict(top=top, bound=bound, lo=lo, hi=hi, admitted=ok.sum(1)))
        out[sid] = dict(x=x, groups=groups, xd=xd, gd=gd, keep=keep, radii=radii, rd={0: None, 1: rd1, 4: rd4}, ref=ref,
                        sg=sg, d=d, share=undecided / max(entries, 1), runs={})
    yield out
    for k in out.values():  # the inputs and their bands are untouched by every call of the module
        for buf, host in k["keep"]:
            assert np.array_equal(buf.cpu().numpy(), host, equal_nan=True)


def _result(c, k, nr):
    key = (k, nr)
    if key not in c["runs"]:
        c["runs"][key] = _run(c["xd"], c["gd"], k, c["rd"][nr], c["sg"])
    return c["runs"][key]


def _check_knn(c, knn, k):
    worst = 0.0
    for g, ref in enumerate(c["ref"]):
        want, bound = ref["top"][:, :k], ref["bound"][:, :k]
        got = knn[:, g]
        none = np.isinf(want)
        assert np.all(got[none] == np.inf)  # fewer than k admitted columns: padded
        assert np.all(np.isfinite(got[~none])) and np.all(got[~none] >= 0.0)  # clamped
        assert np.all(got[:, 1:] >= got[:, :-1])  # ascending
        err = np.abs(got[~none] - want[~none])
        if err.size:
            worst = max(worst, float((err / np.maximum(bound[~none], 1e-300)).max()) if err.max() > 0 else 0.0)
            assert np.all(err <= bound[~none]), (g, float(err.max()))
    return worst


def _check_inside(c, inside, nr):
    width = tight = 0
    for g, ref in enumerate(c["ref"]):
        lo, hi, got = ref["lo"][:, :nr], ref["hi"][:, :nr], inside[:, g]
        assert np.all((lo <= got) & (got <= hi)), g
        width += int((hi - lo).sum())
        tight += int(lo.sum())
        if nr == RMAX:  # the +inf column counts every admitted pair (no NaN among the data)
            assert np.array_equal(got[:, 3], ref["admitted"])
    return width, tight


@pytest.mark.parametrize("nr", NRS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sid", IDS)
def test_matches_the_reference(cases, sid, k, nr):
    c = cases[sid]
    knn, inside, bad = _result(c, k, nr)
    assert knn.shape == (c["x"].shape[0], len(c["groups"]), k) and (inside is None) == (nr == 0)
    assert not bad.any()
    worst = _check_knn(c, knn, k)
    msg = "%s, k = %d, %d radii: knn_d2 max error / bound %.3e" % (sid, k, nr, worst)
    if inside is not None and sid in COUNTED:
        print("%s: undecided share %.4f %% (cap %.2f %%)" % (sid, 100 * c["share"], 100 * _cap(c["d"])))
        assert c["share"] <= _cap(c["d"])
        width, tight = _check_inside(c, inside, nr)
        msg += "; inside within brackets of total width %d around %d decided" % (width, tight)
    print(msg)
    # a part computed alone has the bytes it has beside the other
    assert knn.tobytes() == _result(c, k, 4)[0].tobytes() == _result(c, k, 0)[0].tobytes()
    assert bad.tobytes() == _result(c, k, 4)[2].tobytes()


@pytest.mark.parametrize("nr", [1, 4])
@pytest.mark.parametrize("sid", IDS)
def test_the_counts_alone(cases, sid, nr):
    c = cases[sid]
    knn, inside, bad = _result(c, 0, nr)
    assert knn is None and not bad.any()
    if sid in COUNTED:
        assert c["share"] <= _cap(c["d"])
        print("%s, %d radii alone: brackets of total width %d around %d decided" % ((sid, nr) + _check_inside(c, inside, nr)))
    for k in (3, 8):
        assert inside.tobytes() == _result(c, k, nr)[1].tobytes()
    assert inside.tobytes() == np.ascontiguousarray(_result(c, 3, 4)[1][:, :, :nr]).tobytes()


@pytest.mark.parametrize("sid", IDS)
def test_the_first_neighbour_is_pairwise_stats_nearest(cases, sid):
    """The two ops compute one distance: knn_d2[:, g, 0] has the bytes of nn_d2[:, g]."""
    c = cases[sid]
    _, nn_d2, _ = pkg_mod("quality").pairwise_stats(c["xd"], c["gd"], [], self_group=c["sg"], ksum=False)
    want = nn_d2.cpu().numpy()
    for k in KS:
        got = _result(c, k, 0)[0]
        assert np.ascontiguousarray(got[:, :, 0]).tobytes() == want.tobytes(), k


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("sid", [IDS[5], IDS[6]])
def test_a_set_against_its_own_radii_counts_its_own_lists(cases, sid, k):
    """x = y as the self group with radii the op's own knn_d2[:, 0, k - 1]: d2 is bitwise symmetric, so column j's
    ball holds exactly the rows whose distance is in j's own list up to its k-th value."""
    c = cases[sid]
    n = c["x"].shape[0]
    knn = _result(c, k, 0)[0][:, 0]
    rad = torch.from_numpy(np.ascontiguousarray(knn[:, k - 1:k])).cuda()
    _, inside, bad = _run(c["xd"], [c["xd"]], 0, [rad], 0)
    want = int((knn <= knn[:, k - 1:k]).sum())
    assert int(inside.sum()) == want and not bad.any()
    if np.all(np.diff(knn, axis=1) > 0.0):  # no ties in any list
        assert want == k * n


@pytest.mark.parametrize("sid", [IDS[1], IDS[4], IDS[5], IDS[8], IDS[9]])
def test_two_calls_and_a_slice_of_the_rows_give_the_same_bytes(cases, sid):
    c = cases[sid]
    full = _result(c, 3, 4)
    again = _run(c["xd"], c["gd"], 3, c["rd"][4], c["sg"])
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()
    # row independence, without self exclusion: rows [3, 3 + r) alone, from a dense aligned copy as well
    n = c["x"].shape[0]
    free = _run(c["xd"], c["gd"], 3, c["rd"][4], None)
    for a, b in ((3, 4), (3, min(n, 3 + 66)), (3, n)):
        part = _run(c["xd"][a:b], c["gd"], 3, c["rd"][4], None)
        for p, f in zip(part, free):
            assert p.tobytes() == f[a:b].tobytes(), (a, b)
    dense = _run(torch.from_numpy(c["x"][3:]).cuda(), [torch.from_numpy(y).cuda() for y in c["groups"]], 3, c["rd"][4],
                 None)
    for p, f in zip(dense, free):
        assert p.tobytes() == f[3:].tobytes()


def test_a_nan_is_counted_and_enters_nothing_else(cases):
    c = cases[IDS[1]]  # (5, [3, 4], 7)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rd = c["rd"][4]
    base = _run(dev(c["x"]), [dev(y) for y in c["groups"]], 3, rd, None)
    assert not base[2].any()
    for badv in (np.nan, np.inf):
        x = c["x"].copy()
        x[2, 4] = badv
        knn, inside, bad = _run(dev(x), [dev(y) for y in c["groups"]], 3, rd, None)
        assert np.array_equal(bad[2], [3, 4]) and np.all(knn[2] == np.inf) and np.all(inside[2] == 0)
        rest = [0, 1, 3, 4]
        for a, b in zip((knn, inside, bad), base):
            assert a[rest].tobytes() == b[rest].tobytes()
        y1 = c["groups"][1].copy()
        y1[3, 0] = badv
        knn, inside, bad = _run(dev(c["x"]), [dev(c["groups"][0]), dev(y1)], 3, rd, None)
        assert np.all(bad[:, 1] == 1) and not bad[:, 0].any()
        for a, b in zip((knn, inside), base):
            assert a[:, 0].tobytes() == b[:, 0].tobytes()
        # nothing else changes beyond the removal of that column
        cut = [0, 1, 2]
        want = _run(dev(c["x"]), [dev(c["groups"][0]), dev(c["groups"][1][cut])], 3, [rd[0], rd[1][cut].contiguous()],
                    None)
        assert knn[:, 1].tobytes() == want[0][:, 1].tobytes() and inside[:, 1].tobytes() == want[1][:, 1].tobytes()


def test_bad_arguments_return_their_code_without_a_launch(cases):
    L = pkg_mod("_lib")
    c = cases[IDS[1]]
    x = torch.from_numpy(c["x"]).cuda()
    ys = [torch.from_numpy(y).cuda() for y in c["groups"]]
    rs = [torch.from_numpy(np.ascontiguousarray(r[:, :2])).cuda() for r in c["radii"]]
    n, d = x.shape
    knn = torch.full((n, 2, 3), SENTINEL, dtype=torch.float64, device="cuda")
    ins = torch.full((n, 2, 2), ISENT, dtype=torch.int64, device="cuda")
    nf = torch.full((n, 2), ISENT, dtype=torch.int64, device="cuda")
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)
    ptrs = lambda *t: (ctypes.c_void_p * len(t))(*[None if v is None else v.data_ptr() for v in t])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = L.lib()
    need = lib.svae_op_knn_scratch_bytes(n, i64s(3, 4), 2, 3, 2)
    assert need > 0
    scratch = torch.zeros(max(need, 1 << 16), dtype=torch.uint8, device="cuda")
    ok = dict(x=p(x), n=n, ldx=d, y=ptrs(*ys), m=i64s(3, 4), ldy=i64s(d, d), n_groups=2, d=d, self_group=-1, k=3,
              knn_d2=p(knn), radius2=ptrs(*rs), n_radii=2, inside=p(ins), nonfinite=p(nf), scratch=p(scratch))
    order = ["x", "n", "ldx", "y", "m", "ldy", "n_groups", "d", "self_group", "k", "knn_d2", "radius2", "n_radii",
             "inside", "nonfinite", "scratch"]

    def rc(**over):
        a = dict(ok, **over)
        return lib.svae_op_pairwise_knn(*[a[name] for name in order], L.stream_ptr())

    EBADCONFIG, EBADARG = -1, -2
    five = dict(y=ptrs(*([ys[0]] * 5)), m=i64s(*([3] * 5)), ldy=i64s(*([d] * 5)), n_groups=5,
                radius2=ptrs(*([rs[0]] * 5)))
    for over in (dict(x=None), dict(y=None), dict(m=None), dict(ldy=None), dict(y=ptrs(ys[0], None)),
                 dict(scratch=None), dict(n=0), dict(n=-3), dict(d=0), dict(n_groups=0), dict(m=i64s(3, 0)),
                 dict(m=i64s(-1, 4)), dict(ldx=d - 1), dict(ldy=i64s(d, d - 1)), dict(k=-1), dict(n_radii=-1),
                 dict(k=0), dict(knn_d2=None), dict(n_radii=0), dict(inside=None), dict(radius2=None),
                 dict(k=0, knn_d2=None, n_radii=0, inside=None), dict(self_group=2), dict(self_group=0),
                 dict(self_group=1, y=ptrs(ys[0], x), m=i64s(3, 4))):
        assert rc(**over) == EBADARG, over
        assert lib.svae_last_error(None).startswith(b"pairwise_knn:")
    for over in (five, dict(k=KMAX + 1), dict(n_radii=RMAX + 1)):
        assert rc(**over) == EBADCONFIG, over
        assert lib.svae_last_error(None).startswith(b"pairwise_knn:")
    for bad in ((n, i64s(3, 4), 5, 3, 2), (n, i64s(3, 4), 2, KMAX + 1, 2), (n, i64s(3, 4), 2, 3, RMAX + 1),
                (n, i64s(3, 4), 2, -1, 2), (n, i64s(3, 4), 2, 0, 0), (0, i64s(3, 4), 2, 3, 2), (n, i64s(3, 0), 2, 3, 2),
                (n, None, 2, 3, 2)):
        assert lib.svae_op_knn_scratch_bytes(*bad) == -1, bad
    torch.cuda.synchronize()
    assert torch.all(knn == SENTINEL) and torch.all(ins == ISENT) and torch.all(nf == ISENT)
    assert rc() == 0  # the same arguments, unspoilt, run
    assert rc(nonfinite=None, radius2=ptrs(rs[0], None)) == 0  # nonfinite and a group's radii are optional
    torch.cuda.synchronize()
    import manifold_ref
    want_k, want_i, want_b, _ = manifold_ref.knn_stats(c["x"], c["groups"], 3, radii=[c["radii"][0][:, :2], None])
    np.testing.assert_allclose(knn.cpu().numpy(), want_k, rtol=1e-4, atol=1e-5)
    assert np.array_equal(ins.cpu().numpy(), want_i) and np.array_equal(nf.cpu().numpy(), want_b)
    # the Python wrapper refuses what the op cannot take
    Qm = pkg_mod("quality")
    with pytest.raises(ValueError):
        Qm.knn_stats(x.double(), ys, 3)
    with pytest.raises(ValueError):
        Qm.knn_stats(x.t(), ys, 3)
    with pytest.raises(ValueError):
        Qm.knn_stats(x, [ys[0][:, :d - 1]], 3)
    with pytest.raises(ValueError):
        Qm.knn_stats(x, ys, 3, radii=[rs[0]])  # one entry per group
    with pytest.raises(ValueError):
        Qm.knn_stats(x, ys, 3, radii=[rs[0].float(), None])
    with pytest.raises(ValueError):
        Qm.knn_stats(x, ys, 3, radii=[rs[1], rs[0]])  # rows do not match the groups
    with pytest.raises(ValueError):
        Qm.knn_stats(x, ys, 3, radii=[rs[0], rs[1][:, :1].contiguous()])  # two widths
    with pytest.raises(RuntimeError, match="pairwise_knn"):
        Qm.knn_stats(x, ys, KMAX + 1)
    with pytest.raises(RuntimeError, match="pairwise_knn"):
        Qm.knn_stats(x, ys, 0)
    with pytest.raises(RuntimeError, match="pairwise_knn"):
        Qm.knn_stats(x, ys, 3, self_group=0)


def test_first_check_names_its_op(built_lib):
    L = pkg_mod("_lib")
    P = ctypes.c_void_p(0x1000)  # never read
    for symbol in ("svae_op_knn_scratch_bytes", "svae_op_pairwise_knn"):
        assert symbol in L.EXPORTED
    assert L.lib().svae_op_pairwise_knn(None, 8, 4, None, None, None, 1, 4, -1, 1, P, None, 0, None, None, P,
                                        None) == -2
    assert L.lib().svae_last_error(None).startswith(b"pairwise_knn:")
