"""svae_op_degrade_batch (csrc/degrade.hip) against its numpy restatement (tests/degrade_ref.py).

Without blur every stage is integer draws, exact copies, sequential fp32 block sums and one division, and (with
gaussian_scale = 0) the masks of the pixel noise: the kernel's input and mask are bitwise the restatement's fp32
mode.  The Gaussian pixel noise uses the device's fast fp32 transcendentals, so it is held bitwise to
svae_op_make_batch itself applied in place to the restatement's batch before the pixel noise.

With blur the kernel is compared to the fp64 truth.  The bound is 4 x the largest deviation of the restatement's
own fp32 mode from its fp64 mode on the same inputs (the factor covers expf and summation-order differences between
device and numpy); where the Gaussian pixel noise is on as well, the normals' bound of tests/test_make_batch_gpu.py
times the scale is added (clipping is 1-Lipschitz).

The seeds are chosen (with the restatement, on the CPU; test_seeds_exercise_both_sides_of_every_gate) so that
within each batch every gate both fires and does not fire."""
import ctypes

import numpy as np
import pytest
import torch

import degrade_ref as dr
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

NORMAL_BOUND = 4 * 1.9405e-6  # tests/test_make_batch_gpu.py: max |device normal - float64 restatement|, x 4
LO, HI = -1.0, 1.0
OFFSET = 2 ** 32 - 2  # the image counter carries into c1 inside the batch

# shape: the seed under which every gate fires and does not fire within the batch at p = 0.5
SHAPES = {
    (2, 7, 9, 3): 22,       # odd sizes, partial down-sample blocks, groups straddling pixels, rows and images, r = 12 > h
    (3, 28, 28, 1): 1,     # MNIST, one channel: two bands of 16 rows
    (2, 64, 64, 3): 22,     # CelebA geometry: band borders and halos
    (2, 9, 90, 3): 22,      # a band of 8 rows with 12 halo rows does not fit 64 KB: the global-memory kernel
}
ALL = dr.Spec(0.5, 0.4, 4.0, 0.5, 4, 0.5, 3, 2, 12, 0.25, 0.0, 0.0, 0.0)
STAGES = {
    "down": ALL._replace(p_blur=0.0, p_cut=0.0),
    "cut": ALL._replace(p_blur=0.0, p_down=0.0),
    "noise": dr.IDENTITY._replace(pepper_prob=0.3, salt_prob=0.2),
    "down_cut_noise": ALL._replace(p_blur=0.0, pepper_prob=0.3, salt_prob=0.2),
}


def _seed(shape):
    return SHAPES[shape]


def _target(shape):
    return np.random.default_rng(sum(shape)).uniform(-1, 1, size=shape).astype(np.float32)


def _c_spec(spec):
    return pkg_mod("_lib").SvaeDegradeSpec(*spec)


GUARD = 64


def _run(x, spec, seed, offset=OFFSET, want_mask=True, misalign_in=False, misalign_out=False, lo=LO, hi=HI):
    """One launch; (input, mask) as numpy.  Outputs sit between NaN guard bands that must survive; misalign_*: the
    tensor starts 4 bytes past a 16-byte boundary."""
    L = pkg_mod("_lib")
    n, h, w, c = x.shape
    src = torch.empty(x.size + 1, device="cuda")[1 if misalign_in else 0:][:x.size]
    src.copy_(torch.from_numpy(x).reshape(-1))
    assert src.data_ptr() % 16 == (4 if misalign_in else 0)
    sh = 1 if misalign_out else 0
    out = torch.full((x.size + 2 * GUARD + 1,), float("nan"), device="cuda")
    msk = torch.full((n * h * w + 2 * GUARD,), float("nan"), device="cuda")
    inp = out[GUARD + sh:GUARD + sh + x.size]
    mk = msk[GUARD:GUARD + n * h * w]
    assert inp.data_ptr() % 16 == 4 * sh
    L.check(L.lib().svae_op_degrade_batch(L.ptr(src), n, h, w, c, lo, hi, _c_spec(spec), seed, offset, L.ptr(inp),
                                          L.ptr(mk) if want_mask else None, L.stream_ptr()))
    torch.cuda.synchronize()
    out, msk = out.cpu().numpy(), msk.cpu().numpy()
    assert np.isnan(out[:GUARD + sh]).all() and np.isnan(out[GUARD + sh + x.size:]).all(), "wrote outside input"
    assert np.isnan(msk[:GUARD]).all() and np.isnan(msk[GUARD + n * h * w:]).all(), "wrote outside mask"
    if not want_mask:
        assert np.isnan(msk).all()
    return out[GUARD + sh:GUARD + sh + x.size].reshape(x.shape), msk[GUARD:GUARD + n * h * w].reshape(n, h, w)


def _bitwise(got, ref):
    np.testing.assert_array_equal(got.view(np.int32), np.asarray(ref).astype(np.float32).view(np.int32))


def _make_batch_in_place(x, noise, seed, offset):
    """svae_op_make_batch's corruption of the float32 batch x, in place on the device."""
    L = pkg_mod("_lib")
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n = x.shape[0]
    L.check(L.lib().svae_op_make_batch(L.ptr(d), 0, None, 0, n, x.size // n, LO, HI, *noise, seed, offset, None,
                                       L.ptr(d), L.stream_ptr()))
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.fixture(scope="module")
def refs():
    """(shape, stage) -> the restatement's fp32 mode, computed once."""
    cache = {}

    def get(shape, name):
        if (shape, name) not in cache:
            cache[shape, name] = dr.degrade(_target(shape), STAGES[name], LO, HI, _seed(shape), OFFSET, "fp32")
        return cache[shape, name]
    return get


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_seeds_exercise_both_sides_of_every_gate(shape):
    seed = _seed(shape)
    n, h, w, _ = shape
    d = dr.draws(n, h, w, ALL, seed, OFFSET)
    for g in ("blur", "down", "cut"):
        assert {bool(x[g]) for x in d} == {False, True}, g
    assert max(x["r"] for x in d) >= 1


@pytest.mark.parametrize("name", sorted(STAGES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stages_without_blur_are_bitwise(shape, name, refs):
    ref = refs(shape, name)
    inp, mask = _run(_target(shape), STAGES[name], _seed(shape))
    _bitwise(inp, ref["input"])
    _bitwise(mask, ref["mask"])
    if "cut" in name:
        assert 0 < ref["mask"].mean() < 1
    if name != "noise":
        assert not np.array_equal(ref["structured"], _target(shape))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_unaligned_target_and_input_take_the_scalar_paths(shape, refs):
    ref = refs(shape, "down_cut_noise")
    for mi, mo in ((True, False), (False, True), (True, True)):
        inp, mask = _run(_target(shape), STAGES["down_cut_noise"], _seed(shape), misalign_in=mi, misalign_out=mo)
        _bitwise(inp, ref["input"])
        _bitwise(mask, ref["mask"])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_identity_and_gaussian_noise_are_make_batch(shape, refs):
    x = _target(shape)
    noise = (0.1, 0.1, 0.1)
    seed = _seed(shape)
    # the identity spec: bitwise svae_op_make_batch's input for the same noise, seed and offset
    spec = dr.IDENTITY._replace(pepper_prob=noise[0], salt_prob=noise[1], gaussian_scale=noise[2])
    inp, mask = _run(x, spec, seed)
    _bitwise(inp, _make_batch_in_place(x, noise, seed, OFFSET))
    assert not mask.any()
    # all stages but blur, with the Gaussian noise: svae_op_make_batch on the restatement's structured batch
    spec = STAGES["down_cut_noise"]._replace(pepper_prob=noise[0], salt_prob=noise[1], gaussian_scale=noise[2])
    inp, mask = _run(x, spec, seed)
    ref = refs(shape, "down_cut_noise")
    _bitwise(inp, _make_batch_in_place(ref["structured"], noise, seed, OFFSET))
    _bitwise(mask, ref["mask"])


@pytest.mark.parametrize("noise", [(0.0, 0.0, 0.0), (0.3, 0.2, 0.0), (0.1, 0.1, 0.1)])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_blur_against_the_fp64_truth(shape, noise):
    x = _target(shape)
    seed = _seed(shape)
    # every stage at p = 0.5, and the blur alone on every image at the widest radius (r = 12: wider than 7 x 9)
    for spec in (ALL, ALL._replace(p_blur=1.0, sigma_lo=3.9, p_down=0.0, p_cut=0.0)):
        spec = spec._replace(pepper_prob=noise[0], salt_prob=noise[1], gaussian_scale=noise[2])
        truth = dr.degrade(x, spec, LO, HI, seed, OFFSET, "fp64")
        own = dr.degrade(x, spec, LO, HI, seed, OFFSET, "fp32")
        radii = [d["r"] for d in truth["draws"]]
        assert max(radii) >= 1 and (spec.p_blur < 1.0 or set(radii) == {12})
        self_dev = float(np.abs(own["input"] - truth["input"]).max())
        inp, mask = _run(x, spec, seed)
        dev = float(np.abs(inp.astype(np.float64) - truth["input"]).max())
        bound = 4 * self_dev + NORMAL_BOUND * noise[2]
        print("%s p_blur %.1f noise %s: device - fp64 %.3e, fp32 mode - fp64 %.3e, bound %.3e"
              % (shape, spec.p_blur, noise, dev, self_dev, bound))
        assert self_dev > 0 and dev <= bound
        _bitwise(mask, truth["mask"])


def test_two_calls_and_a_null_mask_give_the_same_bytes():
    shape = (2, 64, 64, 3)
    x, seed = _target(shape), _seed(shape)
    spec = ALL._replace(pepper_prob=0.1, salt_prob=0.1, gaussian_scale=0.1)
    a, ma = _run(x, spec, seed)
    b, mb = _run(x, spec, seed)
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    np.testing.assert_array_equal(ma, mb)
    c, _ = _run(x, spec, seed, want_mask=False)
    np.testing.assert_array_equal(a.view(np.int32), c.view(np.int32))
    d, _ = _run(x, spec, seed + 1)
    assert not np.array_equal(a, d)


def test_images_draw_by_their_counter_not_by_the_launch():
    """Image b of a call at offset o is image 0 of a call at offset o + b: the same structural draws (the pixel noise
    is off, its groups are counted from the batch's first element)."""
    shape = (3, 28, 28, 1)
    x, seed = _target(shape), _seed(shape)
    spec = ALL._replace(p_blur=1.0, p_down=1.0, p_cut=1.0)
    whole, mw = _run(x, spec, seed, offset=7)
    for b in range(3):
        one, m1 = _run(x[b:b + 1], spec, seed, offset=7 + b)
        np.testing.assert_array_equal(one.view(np.int32), whole[b:b + 1].view(np.int32))
        np.testing.assert_array_equal(m1, mw[b:b + 1])


def test_global_memory_kernel_is_bitwise_the_band_kernel(refs):
    """At 90 x 3 columns a band of 8 rows fits the LDS without halo rows and not with the 12 of sigma_hi = 4.
    p_blur = 2^-32 (thr = 1) sizes the halos without ever firing here, so the same stages run in global memory:
    bitwise the restatement, which tests/test_stages_without_blur_are_bitwise holds the band kernel to."""
    shape = (2, 9, 90, 3)
    x, seed = _target(shape), _seed(shape)
    spec = STAGES["down_cut_noise"]._replace(p_blur=2.0 ** -32)
    assert dr.threshold(spec.p_blur) == 1 and spec.sigma_hi == 4.0
    assert not any(d["blur"] for d in dr.draws(2, 9, 90, spec, seed, OFFSET))
    assert 4 * (64 + 2 * (8 + 24) * 270) > 65536 >= 4 * (64 + 2 * 8 * 270)
    ref = refs(shape, "down_cut_noise")
    for mis in (False, True):
        inp, mask = _run(x, spec, seed, misalign_in=mis, misalign_out=mis)
        _bitwise(inp, ref["input"])
        _bitwise(mask, ref["mask"])


def _bad_cases():
    ok = dict(n=2, h=8, w=8, c=3, lo=LO, hi=HI, spec=ALL, inplace=False, null=())
    def case(**kw):
        d = dict(ok)
        d.update(kw)
        return d
    nan = float("nan")
    return {
        "null_target": case(null=("target",)), "null_input": case(null=("input",)), "null_spec": case(null=("spec",)),
        "in_place": case(inplace=True),
        "n0": case(n=0), "h0": case(h=0), "w_negative": case(w=-1), "c0": case(c=0),
        "fewer_than_4_elements": case(h=1, w=1, c=3),
        "p_blur_above_1": case(spec=ALL._replace(p_blur=1.5)), "p_down_negative": case(spec=ALL._replace(p_down=-0.1)),
        "p_cut_nan": case(spec=ALL._replace(p_cut=nan)), "pepper_above_1": case(spec=ALL._replace(pepper_prob=2.0)),
        "salt_negative": case(spec=ALL._replace(salt_prob=-1.0)),
        "sigma_lo_negative": case(spec=ALL._replace(sigma_lo=-0.5)),
        "sigma_lo_above_hi": case(spec=ALL._replace(sigma_lo=2.0, sigma_hi=1.0)),
        "sigma_hi_above_4": case(spec=ALL._replace(sigma_hi=4.5)),
        "factor_3": case(spec=ALL._replace(factor=3)), "factor_0": case(spec=ALL._replace(factor=0)),
        "factor_16": case(spec=ALL._replace(factor=16)),
        "boxes_5": case(spec=ALL._replace(boxes=5)), "boxes_negative": case(spec=ALL._replace(boxes=-1)),
        "min_side_0": case(spec=ALL._replace(min_side=0)),
        "min_side_above_max": case(spec=ALL._replace(min_side=5, max_side=4)),
        "negative_gaussian_scale": case(spec=ALL._replace(gaussian_scale=-0.1)),
        "lo_above_hi": case(lo=1.0, hi=-1.0),
    }


@pytest.mark.parametrize("name", sorted(_bad_cases()))
def test_bad_arguments_return_ebadarg_and_launch_nothing(name):
    L = pkg_mod("_lib")
    k = _bad_cases()[name]
    n, h, w, c = 2, 8, 8, 3
    src = torch.rand(n * h * w * c, device="cuda")
    out = torch.full((n * h * w * c,), float("nan"), device="cuda")
    mask = torch.full((n * h * w,), float("nan"), device="cuda")
    before = src.clone()
    spec = _c_spec(k["spec"])
    rc = L.lib().svae_op_degrade_batch(
        None if "target" in k["null"] else L.ptr(src), k["n"], k["h"], k["w"], k["c"], k["lo"], k["hi"],
        None if "spec" in k["null"] else ctypes.byref(spec), 1, 0,
        None if "input" in k["null"] else (L.ptr(src) if k["inplace"] else L.ptr(out)), L.ptr(mask), L.stream_ptr())
    assert rc == -2, name
    assert b"degrade_batch" in L.lib().svae_last_error(None)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(mask).all() and torch.equal(src, before)


def test_the_unchanged_valid_call_succeeds():
    """The arguments every bad case varies are accepted as they are."""
    x = _target((2, 8, 8, 3))
    inp, mask = _run(x, ALL, 1, offset=0)
    assert np.isfinite(inp).all() and set(np.unique(mask)) <= {0.0, 1.0}
