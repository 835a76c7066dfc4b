"""svae_op_tensor_stats on the GPU against tests/stats_ref.py (float64, exactly rounded sums).

One array of about 300 k floats: the segment lengths {0, 1, 3, 4, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1,
3 CHUNK + 5}, two segments at each offset residue 1, 2, 3 mod 4, two adjacent segments that share a 16-byte
group, gaps between segments and a guard band on both sides of the array, all filled with NaN and 1e30: a read
outside a segment would show in its row.  Bound per sum (derived in stats_ref): n 2^-52 sum |term|; counts and
the maximum are exact.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import stats_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

GUARD = 256       # floats before and after the array (a multiple of 4: the array stays 16-byte aligned)
SENTINEL = -12345.678
EXTRA_ROWS = 3


def _layout():
    C = pkg_mod("_lib").STATS_CHUNK
    segs = []  # (offset, length)
    pos = 0

    def add(length, gap, residue=None):
        nonlocal pos
        pos += gap
        if residue is not None:
            pos += (residue - pos) % 4
        segs.append((pos, length))
        pos += length

    for n, g in zip([0, 1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5], [4, 0, 2, 64, 1, 7, 0, 70, 3, 6, 9]):
        add(n, g)
    for r in (1, 2, 3):  # two segments at every misaligned residue: one over several chunks, one short
        add(2 * C + 7, 5, r)
        add(37, 11, r)
    add(4 * 50 + 2, 8, 0)   # ends in the middle of a 16-byte group ...
    add(9, 0)               # ... which the next segment shares
    add(5 * C + 3, 13, 0)   # a long aligned one: interior chunks are whole groups
    return segs, pos + 16


@pytest.fixture(scope="module")
def case():
    """The array (host, with gaps filled), its segments, the device plan and scratch."""
    S = pkg_mod("summaries")
    segs, n = _layout()
    assert 250_000 < n < 350_000
    offsets, lengths = [o for o, _ in segs], [m for _, m in segs]
    rng = np.random.default_rng(11)
    x = np.empty(n, dtype=np.float32)
    x[0::2], x[1::2] = np.nan, 1e30  # the gaps
    for o, m in segs:
        x[o:o + m] = (rng.standard_normal(m) * 8.0).astype(np.float32)  # about a fifth beyond +-10
    table, n_chunks = S.stats_plan(offsets, lengths)
    return dict(x=x, offsets=offsets, lengths=lengths, n_seg=len(segs), n_chunks=n_chunks,
                table=torch.from_numpy(table).cuda(),
                partials=torch.empty(max(1, n_chunks) * 8, dtype=torch.float64, device="cuda"))


def _device(x, shift=0):
    """x on the device between two guard bands of NaN / 1e30; shift moves it off 16-byte alignment."""
    buf = torch.empty(GUARD + shift + x.size + GUARD, dtype=torch.float32)
    buf[0::2], buf[1::2] = float("nan"), 1e30
    buf[GUARD + shift:GUARD + shift + x.size] = torch.from_numpy(x)
    buf = buf.cuda()
    view = buf[GUARD + shift:GUARD + shift + x.size]
    assert (view.data_ptr() % 16 == 0) == (shift % 4 == 0)
    return view


def _run(case, xd, c):
    L = pkg_mod("_lib")
    out = torch.full(((case["n_seg"] + EXTRA_ROWS), 8), SENTINEL, dtype=torch.float64, device="cuda")
    L.check(L.lib().svae_op_tensor_stats(L.ptr(xd), L.ptr(case["table"]), case["n_seg"], case["n_chunks"], c,
                                         L.ptr(case["partials"]), L.ptr(out), L.stream_ptr()))
    got = out.cpu().numpy()
    assert np.all(got[case["n_seg"]:] == SENTINEL)  # rows past n_seg are not touched
    return got[:case["n_seg"]]


@pytest.fixture(scope="module")
def clean(case):
    """Device results of the clean array for the three clamps (computed once, shared, never modified)."""
    xd = _device(case["x"])
    return {c: _run(case, xd, c) for c in (math.inf, 10.0, 0.0)}


@pytest.mark.parametrize("c", [math.inf, 10.0, 0.0])
def test_columns_match_the_reference(case, clean, c):
    want, bound = stats_ref.stats_ref(case["x"], case["offsets"], case["lengths"], c)
    got = clean[c]
    stats_ref.assert_rows(got, want, bound, "c = %r" % c)
    assert np.all(got[:, 7] == 0.0) and np.all(got[:, 6] == 0.0)
    assert np.all(got[0] == 0.0)  # the empty segment's row
    if c == 10.0:
        assert got[:, 5].sum() > 0.1 * sum(case["lengths"])  # the clamp matters in this data
    if c == 0.0:
        assert np.all(got[:, 1:4] == 0.0) and np.all(got[1:, 5] == got[1:, 0])


def test_non_finite_elements_are_counted_and_ignored(case):
    x = case["x"].copy()
    C = pkg_mod("_lib").STATS_CHUNK
    planted = {}
    for s, where in ((7, [0, 5, C - 2]), (10, [3, C, 2 * C + 1, 3 * C + 4]), (12, [36])):
        o, m = case["offsets"][s], case["lengths"][s]
        assert all(w < m for w in where)
        for i, w in enumerate(where):
            x[o + w] = (np.nan, np.inf, -np.inf)[i % 3]
        planted[s] = len(where)
    for c in (math.inf, 10.0):
        got = _run(case, _device(x), c)
        want, bound = stats_ref.stats_ref(x, case["offsets"], case["lengths"], c)
        stats_ref.assert_rows(got, want, bound, "planted, c = %r" % c)
        for s in range(case["n_seg"]):
            assert got[s, 6] == planted.get(s, 0)
            assert got[s, 0] == case["lengths"][s] - planted.get(s, 0)
        assert np.all(np.isfinite(got))


def test_nothing_outside_a_segment_is_read(case, clean):
    """The gaps and guard bands hold NaN and 1e30 in `clean`; with zeros there instead every row keeps its bytes."""
    x = np.zeros_like(case["x"])
    for o, m in zip(case["offsets"], case["lengths"]):
        x[o:o + m] = case["x"][o:o + m]
    buf = torch.zeros(GUARD + x.size + GUARD, dtype=torch.float32)
    buf[GUARD:GUARD + x.size] = torch.from_numpy(x)
    xd = buf.cuda()[GUARD:GUARD + x.size]
    for c in (math.inf, 10.0):
        assert _run(case, xd, c).tobytes() == clean[c].tobytes()


def test_two_calls_give_identical_bytes(case, clean):
    xd = _device(case["x"])
    for c in (math.inf, 10.0, 0.0):
        assert _run(case, xd, c).tobytes() == clean[c].tobytes()


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_result_does_not_depend_on_the_address(case, clean, shift):
    """x off 16-byte alignment takes 4-byte loads throughout: the same sums in the same order."""
    xd = _device(case["x"], shift)
    assert _run(case, xd, 10.0).tobytes() == clean[10.0].tobytes()


def test_stream_and_empty_plans(case):
    """On a side stream; a plan of empty segments launches the finish kernel alone and writes zero rows."""
    L, S = pkg_mod("_lib"), pkg_mod("summaries")
    table, n_chunks = S.stats_plan([3, 3, 9], [0, 0, 0])
    assert n_chunks == 0
    xd = _device(case["x"])
    out = torch.full((4, 8), SENTINEL, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        L.check(L.lib().svae_op_tensor_stats(L.ptr(xd), L.ptr(torch.from_numpy(table).cuda()), 3, 0, 1.0,
                                             L.ptr(case["partials"]), L.ptr(out), L.stream_ptr(s)))
    s.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:3] == 0.0) and np.all(got[3] == SENTINEL)


def test_bad_arguments(case):
    L = pkg_mod("_lib")
    lib = L.lib()
    xd = _device(case["x"])
    out = torch.zeros(case["n_seg"], 8, dtype=torch.float64, device="cuda")
    good = [L.ptr(xd), L.ptr(case["table"]), case["n_seg"], case["n_chunks"], 10.0, L.ptr(case["partials"]),
            L.ptr(out), L.stream_ptr()]
    assert lib.svae_op_tensor_stats(*good) == 0
    for i, bad in [(0, None), (1, None), (5, None), (6, None), (2, -1), (3, -1), (4, -0.5), (4, float("nan"))]:
        args = list(good)
        args[i] = bad
        assert lib.svae_op_tensor_stats(*args) == -2, i
        assert b"tensor_stats" in lib.svae_last_error(None)
    torch.cuda.synchronize()
