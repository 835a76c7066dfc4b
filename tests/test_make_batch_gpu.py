"""svae_op_make_batch (csrc/batch.hip) against its numpy restatement (tests/batch_ref.py).

Masks and dequantisation (gaussian_scale = 0): the input is bitwise the restatement rounded to float32
(target * keep and + salt are exact in float64 for these inputs, so that rounding is the kernel's one);
the uint8 target is within 4 * 2^-24 * max(|lo|, |hi|, 1) of the float64 value (one fp32 multiply, one
fp32 add, one rounded constant).

Normals: the kernel's N(0,1) use the fp32 fast transcendentals (__logf, __cosf, __sinf), the restatement
float64 ones on the same float32 u and angle.  Measured on an MI355X over 2^20 draws: max |device -
restatement| = NORMAL_DEV_MEASURED (profiles/batch_pipeline.json).  The bound is 4 x that
(the spread of the fp32 transcendental path between ROCm builds) and may not exceed 1e-4; a wrong
word-to-lane mapping is off by order 1."""
import numpy as np
import pytest
import torch

import batch_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

NORMAL_DEV_MEASURED = 1.9405e-6  # MI355X, ROCm 7, 2^20 draws, max |n| 5.36 (tools/bench_batch.py "normals")
NORMAL_BOUND = 4 * NORMAL_DEV_MEASURED
SEED = 0x0123456789ABCDEF


def _run(data, idx, start, n, lo, hi, pepper, salt, scale, seed=SEED, offset=0, want_target=True, want_input=True,
         inplace=False, misalign=False):
    """One launch; returns (target, input) as numpy [n, per_image] (None where not requested)."""
    L = pkg_mod("_lib")
    d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    per = int(np.prod(d.shape[1:]))
    di = None if idx is None else torch.tensor(idx, dtype=torch.int32, device="cuda")

    def out():
        if not misalign:
            return torch.full((n, per), float("nan"), device="cuda")
        return torch.full((n * per + 1,), float("nan"), device="cuda")[1:].view(n, per)  # 4-byte aligned only
    tgt = out() if want_target else None
    inp = d if inplace else (out() if want_input else None)
    L.check(L.lib().svae_op_make_batch(L.ptr(d), 1 if d.dtype == torch.uint8 else 0, L.ptr(di), start, n, per, lo, hi,
                                       pepper, salt, scale, seed, offset, L.ptr(tgt), L.ptr(inp), L.stream_ptr()))
    torch.cuda.synchronize()
    return (None if tgt is None else tgt.cpu().numpy()), (None if inp is None else inp.cpu().numpy().reshape(n, per))


def _data(N, per, u8, seed):
    r = np.random.default_rng(seed)
    if u8:
        return r.integers(0, 256, size=(N, per), dtype=np.uint8)
    return r.uniform(-1, 1, size=(N, per)).astype(np.float32)


def _bitwise(got, ref64):
    np.testing.assert_array_equal(got.view(np.int32), ref64.astype(np.float32).view(np.int32))


# name: (N, n, per_image, u8, idx, start, offset, misaligned outputs)
MASK_CASES = {
    # a: groups straddle images, a partial last group, repeated and unordered rows (scalar uint8 path)
    "a_u8_idx_75": (4, 3, 75, True, [2, 0, 2], 0, 0, False),
    # b: the 16-byte fp32 path with a start
    "b_f32_3072_start1": (6, 4, 3072, False, None, 1, 0, False),
    # c: per_image % 4 == 2: the scalar fp32 path over several blocks, the last one partial
    "c_f32_1030": (2, 2, 1030, False, None, 0, 0, False),
    # e: the counter carries into c1 inside the launch
    "e_f32_carry": (2, 2, 1030, False, None, 0, 2 ** 32 - 3, False),
    # the paths the alignment selects: uint8 through LDS tiles (3 whole tiles; one partial tile; 3 tiles + 48),
    # fp32 with a partial last group, fp32 and uint8 rows whose outputs are only 4-byte aligned, gathered rows
    "u8_tiles_3072": (5, 4, 3072, True, [4, 1, 0, 1], 0, 7, False),
    "u8_partial_tile_48": (6, 5, 48, True, None, 1, 0, False),
    "u8_tiles_4112": (3, 3, 4112, True, None, 0, 0, False),
    "f32_tail_1031": (3, 3, 1031, False, [1, 2, 0], 0, 0, False),
    "f32_misaligned_out": (3, 2, 64, False, None, 1, 0, True),
    "u8_misaligned_out": (3, 2, 64, True, None, 1, 0, True),
    "f32_idx_vec": (5, 3, 256, False, [4, 4, 0], 0, 2 ** 40, False),
}


@pytest.mark.parametrize("name", sorted(MASK_CASES))
@pytest.mark.parametrize("rng", [(-1.0, 1.0), (0.0, 1.0)])
def test_masks_and_dequantisation(name, rng):
    N, n, per, u8, idx, start, offset, mis = MASK_CASES[name]
    lo, hi = rng
    data = _data(N, per, u8, seed=len(name))
    ref = batch_ref.make_batch(data, idx, start, n, lo, hi, 0.3, 0.2, 0.0, SEED, offset)
    tgt, inp = _run(data, idx, start, n, lo, hi, 0.3, 0.2, 0.0, offset=offset, misalign=mis)
    _bitwise(inp, ref["input"])
    if u8:
        err = np.abs(tgt.astype(np.float64) - ref["target64"]).max()
        print("uint8 target: max |err| %.3e (bound %.3e)" % (err, 4 * 2.0 ** -24 * max(abs(lo), abs(hi), 1.0)))
        assert err <= 4 * 2.0 ** -24 * max(abs(lo), abs(hi), 1.0)
        _bitwise(tgt, ref["target"].astype(np.float64))  # and exactly the separately rounded multiply and add
    else:
        _bitwise(tgt, ref["target64"])
    frac = np.mean(ref["unclipped"] != ref["target"].astype(np.float64))
    assert 0.3 < frac < 0.6, frac  # the masks are live: about 1 - 0.7 * 0.8 of the elements change


def test_outputs_are_optional_and_in_place():
    """Case d: in place on fp32 data (apply_noise on a given batch), and either output alone."""
    data = _data(4, 3072, False, seed=3)
    ref = batch_ref.make_batch(data, None, 0, 4, -1.0, 1.0, 0.3, 0.2, 0.0, SEED, 11)
    _, inp = _run(data, None, 0, 4, -1.0, 1.0, 0.3, 0.2, 0.0, offset=11, want_target=False, inplace=True)
    _bitwise(inp, ref["input"])
    tgt, inp = _run(data, None, 0, 4, -1.0, 1.0, 0.3, 0.2, 0.0, offset=11, want_target=True, inplace=True)
    _bitwise(inp, ref["input"])
    _bitwise(tgt, ref["target64"])
    data = _data(3, 77, False, seed=4)  # the scalar path in place
    ref = batch_ref.make_batch(data, None, 0, 3, -1.0, 1.0, 0.3, 0.2, 0.0, SEED, 0)
    _bitwise(_run(data, None, 0, 3, -1.0, 1.0, 0.3, 0.2, 0.0, want_target=False, inplace=True)[1], ref["input"])
    tgt, inp = _run(data, None, 0, 3, -1.0, 1.0, 0.3, 0.2, 0.0, want_input=False)
    assert inp is None
    _bitwise(tgt, ref["target64"])
    tgt, inp = _run(data, None, 0, 3, -1.0, 1.0, 0.3, 0.2, 0.0, want_target=False)
    assert tgt is None
    _bitwise(inp, ref["input"])
    # probabilities 0 and 1: nothing / everything peppered and salted
    _, inp = _run(data, None, 0, 3, -1.0, 1.0, 0.0, 0.0, 0.0, want_target=False)
    _bitwise(inp, data.astype(np.float64))
    _, inp = _run(data, None, 0, 3, -1.0, 1.0, 1.0, 1.0, 0.0, want_target=False)
    assert np.mean(inp == 1.0) > 0.999


def test_in_place_with_a_gather_is_refused():
    L = pkg_mod("_lib")
    d = torch.zeros(4, 8, device="cuda")
    rc = L.lib().svae_op_make_batch(L.ptr(d), 0, None, 1, 2, 8, -1.0, 1.0, 0.1, 0.1, 0.1, 1, 0, None, L.ptr(d),
                                    L.stream_ptr())
    assert rc == -2 and b"in place" in L.lib().svae_last_error(None)


@pytest.fixture(scope="module")
def normal_dev():
    """max |device - float64 restatement| over 2^20 normals: x = 0, no masks, scale 1, range +-1e30."""
    n = 1 << 20
    data = np.zeros((1, n), np.float32)
    _, inp = _run(data, None, 0, 1, -1e30, 1e30, 0.0, 0.0, 1.0, offset=2 ** 32 - 1000, want_target=False)
    ref = batch_ref.normals(n, SEED, 2 ** 32 - 1000)
    dev = float(np.abs(inp.ravel().astype(np.float64) - ref).max())
    print("normals: max |device - restatement| = %.4e over 2^20 draws (max |n| %.3f)" % (dev, np.abs(ref).max()))
    return dev


def test_normals(normal_dev):
    assert NORMAL_BOUND <= 1e-4
    assert normal_dev <= NORMAL_BOUND, normal_dev


def test_geometry_independence():
    """One call over 4 rows of 75 against two calls of 2 rows with the offset advanced by ceil(150 / 4): equal
    on the elements whose groups coincide.  Those are the first call's 150 (its partial last group
    included); 150 % 4 = 2, so the second call starts a fresh group where the one call is mid-group, and it
    is held to its own restatement at the advanced offset instead.  The same call twice is bitwise equal."""
    args = (-1.0, 1.0, 0.1, 0.1, 0.1)
    for u8 in (False, True):
        data = _data(4, 75, u8, seed=9)
        _, one = _run(data, None, 0, 4, *args, offset=100)
        _, again = _run(data, None, 0, 4, *args, offset=100)
        np.testing.assert_array_equal(one.view(np.int32), again.view(np.int32))
        _, first = _run(data, None, 0, 2, *args, offset=100)
        _, second = _run(data, None, 2, 2, *args, offset=100 + (150 + 3) // 4)
        np.testing.assert_array_equal(first.view(np.int32), one[:2].view(np.int32))
        r2 = batch_ref.make_batch(data, None, 2, 2, *args, SEED, 100 + 38)
        assert np.abs(second.astype(np.float64) - r2["input"]).max() <= NORMAL_BOUND * 0.1
    # rows of 76 (a multiple of 4): every group of the split calls coincides with the one call's
    data = _data(4, 76, False, seed=10)
    _, one = _run(data, None, 0, 4, *args, offset=5)
    _, first = _run(data, None, 0, 2, *args, offset=5)
    _, second = _run(data, None, 2, 2, *args, offset=5 + 38)
    np.testing.assert_array_equal(np.concatenate([first, second]).view(np.int32), one.view(np.int32))


def test_full_mix_at_the_reference_constants():
    """0.1 / 0.1 / 0.1 on (-1, 1), case b: within the normals' bound x 0.1 of the restatement.  No element
    is excepted: clipping is 1-Lipschitz, so an element whose unclipped value lies next to +-1 and is
    clipped on one side only still differs by no more than the unclipped values do."""
    N, n, per, u8, idx, start, offset, _ = MASK_CASES["b_f32_3072_start1"]
    data = _data(N, per, u8, seed=21)
    ref = batch_ref.make_batch(data, idx, start, n, -1.0, 1.0, 0.1, 0.1, 0.1, SEED, 12345)
    tgt, inp = _run(data, idx, start, n, -1.0, 1.0, 0.1, 0.1, 0.1, offset=12345)
    _bitwise(tgt, ref["target64"])
    bound = NORMAL_BOUND * 0.1
    err = np.abs(inp.astype(np.float64) - ref["input"])
    print("full mix: max err %.3e (bound %.3e)" % (err.max(), bound))
    assert err.max() <= bound
    assert 0.03 < np.mean(inp == 1.0) < 0.25 and np.mean(inp == -1.0) < 0.1
