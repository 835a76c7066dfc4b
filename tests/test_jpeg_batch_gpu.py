"""svae_op_jpeg_batch (csrc/jpeg.hip) against its numpy restatement (tests/jpeg_ref.py).

Every stage of the contract is integer draws, fp32 operations rounded one by one in a stated order, correctly rounded
divisions and rintf, so the kernel's output and qualities are bitwise the restatement's fp32 mode: no tolerance.
(tests/test_jpeg_ref.py shows why none would do: quantiser ties make the fp32 and fp64 modes differ in whole blocks.)

The seed is chosen (with the restatement, on the CPU; test_seeds_exercise_both_sides_of_every_gate) so that at
p = 0.5 the gate both fires and does not fire within each batch."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_ref as jr
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
OFFSET = 2 ** 32 - 2  # the image counter carries into c1 inside a batch of three
SEED = 1
GUARD = 64

SHAPES = [
    (3, 8, 8, 1),      # one block
    (3, 13, 21, 3),    # partial blocks on both axes, an odd chroma plane under 4:2:0, rows that are no multiple of 4
    (3, 28, 28, 1),    # MNIST: four tiles an image, the last ones partial
    (2, 16, 24, 3),    # exact multiples of 16 and of 8
    (2, 64, 64, 3),    # CelebA geometry
    (2, 9, 600, 3),    # a wide image: 38 tiles a row, the last one partial
]
# name: (p, q_lo, q_hi)
QUALITIES = {"q5_95": (0.5, 5, 95), "q1": (1.0, 1, 1), "q50": (1.0, 50, 50), "q100": (1.0, 100, 100)}


def _batch(shape):
    """Smooth waves plus noise over the whole range, a few pixels at the ends of it."""
    n, h, w, c = shape
    rng = np.random.default_rng(sum(shape))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    x = np.empty(shape)
    for b in range(n):
        for ch in range(c):
            fy, fx, ph = rng.uniform(0.3, 3.0), rng.uniform(0.3, 3.0), rng.uniform(0, 6.28)
            x[b, :, :, ch] = 0.8 * np.sin(fy * yy / 4 + ph) * np.cos(fx * xx / 4 + ch)
    x += rng.normal(0, 0.08, size=shape)
    x = np.clip(x, LO, HI)
    flat = x.reshape(-1)
    flat[rng.integers(0, flat.size, size=8)] = LO
    flat[rng.integers(0, flat.size, size=8)] = HI
    return x.astype(np.float32)


def _c_spec(p, q_lo, q_hi, sub):
    return pkg_mod("_lib").SvaeJpegSpec(p, q_lo, q_hi, sub)


def _run(x, spec, seed=SEED, offset=OFFSET, want_quality=True, misalign_in=False, misalign_out=False, inplace=False,
         lo=LO, hi=HI):
    """One launch; (out, quality) as numpy.  Outputs sit between guard bands that must survive; misalign_*: the
    tensor starts 4 bytes past a 16-byte boundary.  inplace: out is the source itself (guarded alike)."""
    L = pkg_mod("_lib")
    n, h, w, c = x.shape
    sh_in, sh_out = (1 if misalign_in else 0), (1 if misalign_out else 0)
    if inplace:
        sh_out = sh_in
    out = torch.full((x.size + 2 * GUARD + 1,), float("nan"), device="cuda")
    dst = out[GUARD + sh_out:GUARD + sh_out + x.size]
    if inplace:
        src = dst
    else:
        src = torch.empty(x.size + 1, device="cuda")[sh_in:][:x.size]
    src.copy_(torch.from_numpy(x).reshape(-1))
    assert src.data_ptr() % 16 == 4 * sh_in and dst.data_ptr() % 16 == 4 * sh_out
    qbuf = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    qv = qbuf[GUARD:GUARD + n]
    L.check(L.lib().svae_op_jpeg_batch(L.ptr(src), n, h, w, c, lo, hi, _c_spec(*spec), seed, offset, L.ptr(dst),
                                       L.ptr(qv) if want_quality else None, L.stream_ptr()))
    torch.cuda.synchronize()
    if not inplace:
        assert np.array_equal(src.cpu().numpy().view(np.int32), x.reshape(-1).view(np.int32)), "wrote the source"
    out, qbuf = out.cpu().numpy(), qbuf.cpu().numpy()
    lo_, hi_ = GUARD + sh_out, GUARD + sh_out + x.size
    assert np.isnan(out[:lo_]).all() and np.isnan(out[hi_:]).all(), "wrote outside out"
    assert (qbuf[:GUARD] == -7).all() and (qbuf[GUARD + n:] == -7).all(), "wrote outside quality"
    if not want_quality:
        assert (qbuf == -7).all()
    return out[lo_:hi_].reshape(x.shape), qbuf[GUARD:GUARD + n]


def _bitwise(got, ref):
    np.testing.assert_array_equal(got.view(np.int32), np.asarray(ref).astype(np.float32).view(np.int32))


@pytest.fixture(scope="module")
def refs():
    """(shape, quality name, subsample) -> the restatement's fp32 mode, computed once."""
    cache = {}

    def get(shape, name, sub):
        key = (shape, name, sub if shape[3] == 3 else 1)
        if key not in cache:
            p, q_lo, q_hi = QUALITIES[name]
            cache[key] = jr.jpeg_batch(_batch(shape), p, q_lo, q_hi, sub, LO, HI, SEED, OFFSET, "fp32")
        return cache[key]
    return get


@pytest.mark.parametrize("shape", SHAPES)
def test_seeds_exercise_both_sides_of_every_gate(shape):
    q = jr.draws(shape[0], 0.5, 5, 95, SEED, OFFSET)
    assert {bool(v) for v in q} == {False, True}
    assert all(5 <= v <= 95 for v in q if v)
    assert OFFSET + shape[0] > 2 ** 32 or shape[0] == 2  # the counter carries inside the batches of three


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("name", sorted(QUALITIES))
@pytest.mark.parametrize("shape", SHAPES)
def test_output_and_quality_are_bitwise_the_restatement(shape, name, sub, refs):
    ref = refs(shape, name, sub)
    x = _batch(shape)
    out, quality = _run(x, QUALITIES[name] + (sub,))
    np.testing.assert_array_equal(quality, ref["quality"])
    _bitwise(out, ref["out"])
    for b in range(shape[0]):
        if quality[b] == 0:
            np.testing.assert_array_equal(out[b].view(np.int32), x[b].view(np.int32))
        else:
            assert not np.array_equal(out[b], x[b])


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_in_place_equals_out_of_place(shape, sub, refs):
    ref = refs(shape, "q5_95", sub)
    for mis in (False, True):
        out, quality = _run(_batch(shape), QUALITIES["q5_95"] + (sub,), inplace=True, misalign_in=mis)
        np.testing.assert_array_equal(quality, ref["quality"])
        _bitwise(out, ref["out"])


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_unaligned_in_and_out_take_the_scalar_paths(shape, sub, refs):
    ref = refs(shape, "q5_95", sub)
    for mi, mo in ((True, False), (False, True), (True, True)):
        out, quality = _run(_batch(shape), QUALITIES["q5_95"] + (sub,), misalign_in=mi, misalign_out=mo)
        np.testing.assert_array_equal(quality, ref["quality"])
        _bitwise(out, ref["out"])


def test_two_calls_and_a_null_quality_give_the_same_bytes():
    shape = (2, 64, 64, 3)
    x, spec = _batch(shape), (0.5, 5, 95, 2)
    a, qa = _run(x, spec)
    b, qb = _run(x, spec)
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    np.testing.assert_array_equal(qa, qb)
    c, _ = _run(x, spec, want_quality=False)
    np.testing.assert_array_equal(a.view(np.int32), c.view(np.int32))
    d, qd = _run(x, spec, seed=SEED + 1)
    assert not np.array_equal(qa, qd)


def test_images_draw_by_their_counter_not_by_the_launch():
    """Image b of a call at offset o is image 0 of a call at offset o + b: a batch cut in two with the offset
    advanced gives the same rows."""
    shape = (3, 13, 21, 3)
    x, spec = _batch(shape), (0.5, 5, 95, 2)
    whole, qw = _run(x, spec, offset=OFFSET)
    head, qh = _run(x[:1], spec, offset=OFFSET)
    tail, qt = _run(x[1:], spec, offset=OFFSET + 1)
    np.testing.assert_array_equal(np.concatenate([head, tail]).view(np.int32), whole.view(np.int32))
    np.testing.assert_array_equal(np.concatenate([qh, qt]), qw)


def test_other_ranges_and_the_python_wrapper():
    """lo = 0, hi = 255 (levels as they are) and lo = 0, hi = 1; degrade.jpeg_batch in place and into out."""
    D = pkg_mod("degrade")
    shape = (2, 16, 24, 3)
    for lo, hi in ((0.0, 255.0), (0.0, 1.0)):
        x = ((_batch(shape) - LO) * np.float32((hi - lo) / (HI - LO)) + np.float32(lo)).astype(np.float32)
        ref = jr.jpeg_batch(x, 1.0, 30, 30, 2, lo, hi, 5, 9, "fp32")
        out, _ = _run(x, (1.0, 30, 30, 2), seed=5, offset=9, lo=lo, hi=hi)
        _bitwise(out, ref["out"])
    deg = D.Degradation(jpeg=(1.0, 30, 30))
    assert deg.jpeg == (1.0, 30, 30, 2)
    t = torch.from_numpy(x).cuda()
    quality = torch.zeros(2, dtype=torch.int32, device="cuda")
    other = D.jpeg_batch(t, deg, 0.0, 1.0, 5, 9, out=torch.empty_like(t), quality=quality)
    assert torch.equal(t.cpu(), torch.from_numpy(x)) and quality.tolist() == [30, 30]
    same = D.jpeg_batch(t, deg, 0.0, 1.0, 5, 9)
    assert same is t and torch.equal(t, other)
    _bitwise(t.cpu().numpy(), ref["out"])


def _bad_cases():
    ok = dict(n=2, h=8, w=8, c=3, lo=LO, hi=HI, spec=(0.5, 5, 95, 2), null=())
    def case(**kw):
        d = dict(ok)
        d.update(kw)
        return d
    nan = float("nan")
    return {
        "null_in": case(null=("in",)), "null_out": case(null=("out",)), "null_spec": case(null=("spec",)),
        "n0": case(n=0), "h0": case(h=0), "w_negative": case(w=-1),
        "c0": case(c=0), "c2": case(c=2), "c4": case(c=4),
        "p_above_1": case(spec=(1.5, 5, 95, 2)), "p_negative": case(spec=(-0.1, 5, 95, 2)),
        "p_nan": case(spec=(nan, 5, 95, 2)),
        "q_lo_0": case(spec=(0.5, 0, 95, 2)), "q_hi_101": case(spec=(0.5, 5, 101, 2)),
        "q_lo_above_hi": case(spec=(0.5, 60, 50, 2)),
        "subsample_0": case(spec=(0.5, 5, 95, 0)), "subsample_3": case(spec=(0.5, 5, 95, 3)),
        "lo_equals_hi": case(lo=1.0, hi=1.0), "lo_above_hi": case(lo=1.0, hi=-1.0),
    }


@pytest.mark.parametrize("name", sorted(_bad_cases()))
def test_bad_arguments_return_ebadarg_and_launch_nothing(name):
    L = pkg_mod("_lib")
    k = _bad_cases()[name]
    n, h, w, c = 2, 8, 8, 3
    src = torch.rand(n * h * w * c, device="cuda") * 2 - 1
    out = torch.full((n * h * w * c,), float("nan"), device="cuda")
    quality = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    before = src.clone()

    def call(kk):
        return L.lib().svae_op_jpeg_batch(
            None if "in" in kk["null"] else L.ptr(src), kk["n"], kk["h"], kk["w"], kk["c"], kk["lo"], kk["hi"],
            None if "spec" in kk["null"] else ctypes.byref(_c_spec(*kk["spec"])), 1, 0,
            None if "out" in kk["null"] else L.ptr(out), L.ptr(quality), L.stream_ptr())
    assert call(k) == -2, name
    assert b"jpeg_batch" in L.lib().svae_last_error(None)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (quality == -7).all() and torch.equal(src, before)


def test_the_unchanged_valid_call_succeeds():
    """The arguments every bad case varies are accepted as they are, and an image above 2^31 - 1 elements is a
    configuration error, not a bad argument."""
    L = pkg_mod("_lib")
    x = _batch((2, 8, 8, 3))
    out, quality = _run(x, (0.5, 5, 95, 2), seed=1, offset=0)
    assert np.isfinite(out).all() and ((quality == 0) | ((quality >= 5) & (quality <= 95))).all()
    t = torch.zeros(4, device="cuda")
    rc = L.lib().svae_op_jpeg_batch(L.ptr(t), 1, 65536, 32768, 1, LO, HI, ctypes.byref(_c_spec(0.5, 5, 95, 2)), 1, 0,
                                    L.ptr(t), None, L.stream_ptr())
    assert rc != 0 and rc != -2 and b"jpeg_batch" in L.lib().svae_last_error(None)
    torch.cuda.synchronize()
    assert (t == 0).all()
