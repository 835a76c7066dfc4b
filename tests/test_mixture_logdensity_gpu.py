"""svae_op_mixture_logdensity on the GPU against tests/latent_ref.py (numpy float64, two passes).

Bound: |got - ref| <= 1e-9 + 1e-12 |ref|.  It is a rounding bound: every exponent is a sum of d terms of a few fp64
operations each, (d + 3) 2^-53 relative, and the sum over the components adds nm 2^-53; a streaming and a two-pass
fp64 evaluation of these input families agree to a few 1e-16 relative (the hopeless queries have |ref| near 1e7),
three orders and more inside it; every case prints its error over the bound.

Shapes (nq, nm, d), with TILE the kernel's component tile: every (nq, nm) of (1, 1), (5, 1), (7, TILE - 1),
(33, TILE), (16, TILE + 1), (64, 2 TILE + 1), (257, 130) and every d of 1, 3, 12, 110, 256, d = 256 with nm > TILE.
Each runs with the whole / levels / single-dimensions list, the same list reversed and a list of overlapping odd
segments.  z, mu and sigma have leading dimensions above d with NaN in the gap, bases off 16-byte alignment and
guard bands of NaN / 1e30 around them; out has sentinel rows before and after.  sigma is log-uniform in
[1e-3, 1]; the first min(nq, nm) queries are draws from their own component, the rest N(0, 4): near and hopeless
queries both occur.
"""
import ctypes

import numpy as np
import pytest
import torch

import latent_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

TILE = 16  # SVAE_LATENTS_TILE, asserted below
GUARD = 256
SENTINEL = -12345.678
SHAPES = [(1, 1, 1), (5, 1, 3), (7, TILE - 1, 12), (33, TILE, 110), (16, TILE + 1, 256), (64, 2 * TILE + 1, 12),
          (257, 130, 110)]
LEVELS = {1: [1], 3: [2, 1], 12: [3, 3, 3, 3], 110: [20, 30, 30, 30], 256: [64, 64, 64, 64]}
KINDS = ["report", "reversed", "overlapping"]


def _segments(d, kind):
    if kind == "overlapping":
        segs = [(0, d), (d // 3, max(1, d // 2)), (d - 1, 1), (0, 1), (d // 2, d - d // 2), (0, d)]
        segs += [(1, min(d - 1, 5)), (d - min(d, 7), min(d, 7)), (min(d - 1, 2), 1)] if d > 1 else []
        return segs
    segs = [(o, n) for _, o, n in latent_ref.segments_for(LEVELS[d])]
    return segs[::-1] if kind == "reversed" else segs


def _data(nq, nm, d):
    rng = np.random.default_rng(100000 * nq + 1000 * nm + d)
    mu = rng.normal(0, 1, (nm, d)).astype(np.float32)
    sigma = np.exp(rng.uniform(np.log(1e-3), 0.0, (nm, d))).astype(np.float32)
    z = rng.normal(0, 2, (nq, d)).astype(np.float32)
    k = min(nq, nm)
    z[:k] = (mu[:k] + sigma[:k] * rng.normal(0, 1, (k, d))).astype(np.float32)
    return z, mu, sigma


def _device(a, ld, shift):
    """a [n, d] on the device with rows ld floats apart (NaN in the gaps), between guard bands of NaN / 1e30,
    the base ``shift`` floats off 16-byte alignment.  Returns (view, buffer, host image of the buffer)."""
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


def _run(zd, md, sd, segs, extra=2):
    """The op through latents.mixture_logdensity into an out with sentinel rows around it; numpy [nq, n_seg]."""
    Lt = pkg_mod("latents")
    nq, ns = zd.shape[0], len(segs)
    out = torch.full((extra + nq + extra, ns), SENTINEL, dtype=torch.float64, device="cuda")
    got = Lt.mixture_logdensity(zd, md, sd, segs, out=out[extra:])
    assert got.shape == (nq, ns) and got.data_ptr() == out[extra].data_ptr()
    host = out.cpu().numpy()
    assert np.all(host[:extra] == SENTINEL) and np.all(host[extra + nq:] == SENTINEL)
    return host[extra:extra + nq].copy()


@pytest.fixture(scope="module")
def cases():
    """Per shape: host data, device views (shared, never modified) and, per kind of list, segments, reference
    and device result."""
    assert pkg_mod("_lib").LATENTS_TILE == TILE and pkg_mod("latents").TILE == TILE
    out = {}
    for nq, nm, d in SHAPES:
        z, mu, sigma = _data(nq, nm, d)
        zd, zbuf, zhost = _device(z, d + 3, 1)
        md, mbuf, mhost = _device(mu, d + 5, 3)
        sd, sbuf, shost = _device(sigma, d + 5, 2)
        k = dict(z=z, mu=mu, sigma=sigma, zd=zd, md=md, sd=sd, keep=(zbuf, mbuf, sbuf))
        for kind in KINDS:
            segs = _segments(d, kind)
            k[kind] = dict(segs=segs, want=latent_ref.mixture_logdensity(z, mu, sigma, segs),
                           got=_run(zd, md, sd, segs))
        for buf, host in ((zbuf, zhost), (mbuf, mhost), (sbuf, shost)):  # the inputs and their bands are untouched
            assert np.array_equal(buf.cpu().numpy(), host, equal_nan=True)
        out[(nq, nm, d)] = k
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_the_reference(cases, shape, kind):
    k = cases[shape][kind]
    got, want = k["got"], k["want"]
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    err = np.abs(got - want)
    bound = 1e-9 + 1e-12 * np.abs(want)
    print("%s %s: %d segments, max |got - ref| %.3e, max of error / bound %.3e, ref in [%.3e, %.3e]" % (
        shape, kind, len(k["segs"]), err.max(), (err / bound).max(), want.min(), want.max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_column_does_not_depend_on_its_company(cases, shape):
    """Bitwise: the reversed list's columns are the report list's reversed; equal segments of one list give equal
    columns; a segment asked for alone gives its column."""
    k = cases[shape]
    assert k["reversed"]["got"][:, ::-1].tobytes() == k["report"]["got"].tobytes()
    ov = k["overlapping"]
    assert ov["got"][:, 0].tobytes() == ov["got"][:, 5].tobytes() == k["report"]["got"][:, 0].tobytes()
    for col in (1, len(ov["segs"]) - 1):
        alone = _run(k["zd"], k["md"], k["sd"], [ov["segs"][col]])
        assert alone[:, 0].tobytes() == ov["got"][:, col].tobytes(), col


@pytest.mark.parametrize("shape", [(16, TILE + 1, 256), (64, 2 * TILE + 1, 12), (257, 130, 110)])
def test_two_calls_and_a_slice_of_the_queries_give_the_same_bytes(cases, shape):
    k = cases[shape]
    segs, full = k["report"]["segs"], k["report"]["got"]
    assert _run(k["zd"], k["md"], k["sd"], segs).tobytes() == full.tobytes()
    nq = shape[0]
    for a, b in ((0, 1), (nq // 3, nq // 3 + 5), (nq - 3, nq)):
        part = _run(k["zd"][a:b], k["md"], k["sd"], segs)
        assert part.tobytes() == full[a:b].tobytes(), (a, b)
    # aligned, dense inputs: the same values
    dense = _run(torch.from_numpy(k["z"]).cuda(), torch.from_numpy(k["mu"]).cuda(), torch.from_numpy(k["sigma"]).cuda(),
                 segs)
    assert dense.tobytes() == full.tobytes()


def test_a_bad_sigma_spoils_only_the_rows_that_read_it(cases):
    """sigma <= 0 or NaN in one dimension of one component: every segment holding that dimension is non-finite,
    the other segments keep their bytes."""
    k = cases[(64, 2 * TILE + 1, 12)]
    segs, full = k["report"]["segs"], k["report"]["got"]
    for bad in (0.0, -1.0, np.nan):
        sigma = k["sigma"].copy()
        sigma[20, 7] = bad
        got = _run(torch.from_numpy(k["z"]).cuda(), torch.from_numpy(k["mu"]).cuda(), torch.from_numpy(sigma).cuda(),
                   segs)
        holds = np.array([o <= 7 < o + n for o, n in segs])
        assert not np.any(np.isfinite(got[:, holds])), bad
        assert got[:, ~holds].tobytes() == full[:, ~holds].tobytes(), bad


def test_bad_arguments_return_their_code_without_a_launch(cases):
    L, Lt = pkg_mod("_lib"), pkg_mod("latents")
    k = cases[(7, TILE - 1, 12)]
    z, mu, sg = (torch.from_numpy(k[n]).cuda() for n in ("z", "mu", "sigma"))
    out = torch.full((7, 2), SENTINEL, dtype=torch.float64, device="cuda")
    fn = L.lib().svae_op_mixture_logdensity
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    seg = lambda *v: (ctypes.c_int32 * len(v))(*v)
    ok = dict(z=p(z), nq=7, ldz=12, mu=p(mu), sigma=p(sg), nm=TILE - 1, ldm=12, d=12, seg=seg(0, 12, 3, 2), n_seg=2,
              out=p(out))
    order = ["z", "nq", "ldz", "mu", "sigma", "nm", "ldm", "d", "seg", "n_seg", "out"]

    def rc(**over):
        a = dict(ok, **over)
        return fn(*[a[n] for n in order], L.stream_ptr())

    EBADCONFIG, EBADARG = -1, -2
    for over in (dict(z=None), dict(mu=None), dict(sigma=None), dict(seg=None), dict(out=None), dict(nq=0), dict(nq=-1),
                 dict(nm=0), dict(d=0), dict(n_seg=0), dict(n_seg=-2), dict(ldz=11), dict(ldm=11),
                 dict(seg=seg(0, 13, 3, 2)), dict(seg=seg(0, 12, -1, 2)), dict(seg=seg(0, 12, 3, 0)),
                 dict(seg=seg(0, 12, 12, 1)), dict(seg=seg(0, 12, 11, 2))):
        assert rc(**over) == EBADARG, over
        assert b"mixture_logdensity" in L.lib().svae_last_error(None)
    big = seg(*([0, 1] * (L.LATENTS_MAX_SEGMENTS + 1)))
    for over in (dict(d=L.LATENTS_MAX_DIM + 1, ldz=400, ldm=400), dict(seg=big, n_seg=L.LATENTS_MAX_SEGMENTS + 1)):
        assert rc(**over) == EBADCONFIG, over
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
    assert rc() == 0  # the same arguments, unspoilt, run
    torch.cuda.synchronize()
    want = latent_ref.mixture_logdensity(k["z"], k["mu"], k["sigma"], [(0, 12), (3, 2)])
    assert np.all(np.abs(out.cpu().numpy() - want) <= 1e-9 + 1e-12 * np.abs(want))
    # the Python wrapper refuses what the op cannot take
    with pytest.raises(ValueError):
        Lt.mixture_logdensity(z.double(), mu, sg, [(0, 12)])
    with pytest.raises(ValueError):
        Lt.mixture_logdensity(z, mu, sg[:, :11], [(0, 11)])
    with pytest.raises(ValueError):
        Lt.mixture_logdensity(z.t(), mu, sg, [(0, 12)])
    with pytest.raises(RuntimeError, match="mixture_logdensity"):
        Lt.mixture_logdensity(z, mu, sg, [(5, 8)])
