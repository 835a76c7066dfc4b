"""svae_op_ema (csrc/ema.hip) on the GPU against tests/ema_ref.py: bitwise.

The kernel takes 16-byte accesses from the first 16-byte boundary of ``ema`` (on ``w`` too when it is aligned
there) and goes element by element before and after, over a grid of at most 4096 blocks of 256 lanes with two
16-byte groups per lane and sweep.  The cases walk every one of those paths: lengths below, at and above a group,
each pointer on and one element off a 16-byte boundary, and one length past a full sweep of the largest grid."""
import numpy as np
import pytest
import torch

import ema_ref as er
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

SWEEP = 4096 * 256 * 2 * 4  # elements the largest grid covers in one sweep
OMDS = [2.0 ** -10, 0.1, 1.0]


def _op(e, w, omd):
    L = pkg_mod("_lib")
    return L.lib().svae_op_ema(L.ptr(e), L.ptr(w), e.numel(), float(np.float32(omd)), L.stream_ptr())


def _pair(n, off_e, off_w, seed=0):
    """(e, w) device views of n floats whose first element is off_e / off_w elements past a 16-byte boundary, and
    the host copies."""
    rng = np.random.default_rng(seed + 17 * n)
    he = rng.standard_normal(n).astype(np.float32)
    hw = (he + rng.standard_normal(n).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    be = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    bw = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    assert be.data_ptr() % 16 == 0 and bw.data_ptr() % 16 == 0
    e, w = be[off_e:off_e + n], bw[off_w:off_w + n]
    e.copy_(torch.from_numpy(he))
    w.copy_(torch.from_numpy(hw))
    return e, w, he, hw, be, bw


def _same_bits(got, want):
    np.testing.assert_array_equal(np.asarray(got).view(np.int32), np.asarray(want).view(np.int32))


@pytest.mark.parametrize("off_w", [0, 1])
@pytest.mark.parametrize("off_e", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023])
def test_small_lengths_and_alignments(n, off_e, off_w):
    for omd in OMDS:
        e, w, he, hw, be, bw = _pair(n, off_e, off_w)
        assert _op(e, w, omd) == 0
        _same_bits(e.cpu().numpy(), er.update(he, hw, np.float32(omd)))
        _same_bits(w.cpu().numpy(), hw)
        # nothing outside [0, n) is written
        assert float(be[:off_e].abs().sum()) == 0.0 and float(be[off_e + n:].abs().sum()) == 0.0


@pytest.mark.parametrize("off_e,off_w", [(0, 0), (1, 0)])
def test_past_a_full_sweep_of_the_largest_grid(off_e, off_w):
    """Grid-stride: the second sweep, a ragged last group and a scalar tail (33.6 MB per buffer)."""
    n = SWEEP + 4 * 700 + 3
    e, w, he, hw, be, bw = _pair(n, off_e, off_w)
    assert _op(e, w, 0.1) == 0
    _same_bits(e.cpu().numpy(), er.update(he, hw, np.float32(0.1)))
    assert float(be[off_e + n:].abs().sum()) == 0.0


def test_nonfinite_propagates_as_the_formula_says():
    n = 1023
    e, w, he, hw, _, _ = _pair(n, 0, 0)
    for i, v in [(0, np.nan), (5, np.inf), (6, -np.inf), (1022, np.nan), (513, np.inf)]:
        hw[i] = v
    he[7] = np.inf
    hw[7] = np.inf  # inf - inf
    e.copy_(torch.from_numpy(he))
    w.copy_(torch.from_numpy(hw))
    assert _op(e, w, 0.1) == 0
    got, want = e.cpu().numpy(), er.update(he, hw, np.float32(0.1))
    nan = np.isnan(want)
    assert sorted(np.flatnonzero(nan)) == [0, 7, 1022]
    np.testing.assert_array_equal(np.isnan(got), nan)  # a NaN's payload is the hardware's own
    _same_bits(got[~nan], want[~nan])
    assert got[5] == np.inf and got[6] == -np.inf and got[513] == np.inf  # the average follows the weight


def test_omd_zero_makes_no_change_and_repeats_are_identical():
    e, w, he, hw, _, _ = _pair(1023, 1, 0)
    assert _op(e, w, 0.0) == 0
    _same_bits(e.cpu().numpy(), he)
    outs = []
    for _ in range(2):
        e.copy_(torch.from_numpy(he))
        assert _op(e, w, 2.0 ** -10) == 0
        outs.append(e.cpu().numpy())
    _same_bits(outs[0], outs[1])
    # omd = 1 moves the average onto the weights up to the roundings of the formula
    e.copy_(torch.from_numpy(he))
    assert _op(e, w, 1.0) == 0
    _same_bits(e.cpu().numpy(), er.update(he, hw, np.float32(1.0)))


def test_bad_arguments():
    L = pkg_mod("_lib")
    lib = L.lib()
    e, w, he, _, _, _ = _pair(16, 0, 0)
    s = L.stream_ptr()
    assert lib.svae_op_ema(None, L.ptr(w), 16, 0.5, s) == -2
    assert lib.svae_op_ema(L.ptr(e), None, 16, 0.5, s) == -2
    assert lib.svae_op_ema(L.ptr(e), L.ptr(w), 0, 0.5, s) == -2
    assert lib.svae_op_ema(L.ptr(e), L.ptr(w), -4, 0.5, s) == -2
    for omd in (-0.25, 1.5, float("nan"), float("inf")):
        assert lib.svae_op_ema(L.ptr(e), L.ptr(w), 16, omd, s) == -2
        assert b"omd" in lib.svae_last_error(None)
    _same_bits(e.cpu().numpy(), he)
