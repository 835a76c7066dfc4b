"""svae_op_image_metrics on the GPU against tests/metrics_ref.py (float64, direct windowed sums), within the
bound derived there.

Shapes: 11x11x1 (a single window), 12x13x3 (non-square, interleaved channels), 32x32x1, 64x64x3, and with T the
kernel's tile, valid regions of (T - 1) x (2T - 1), T x 2T and (T + 1) x (2T + 1) positions.  Every shape runs
with n = 1 and with n = 6 against ny = 2 (image i against target i % 2); the six images are smooth plus noise
in [-1, 1], with image 3 constant against a constant target 1 and image 4 equal to its target 0.  x, y and out
sit between guard bands of NaN and 1e30, out has sentinel rows past n: a stray read would show in a row, a
stray write in the bands.
"""
import numpy as np
import pytest
import torch

import metrics_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

GUARD = 256        # floats (a multiple of 4: the arrays stay 16-byte aligned)
SENTINEL = -12345.678
EXTRA_ROWS = 3
TILE = 16          # SVAE_METRICS_TILE, asserted below
SHAPES = [(11, 11, 1), (12, 13, 3), (32, 32, 1), (64, 64, 3),
          (TILE + 9, 2 * TILE + 9, 2), (TILE + 10, 2 * TILE + 10, 2), (TILE + 11, 2 * TILE + 11, 2)]
L = 2.0


def _smooth(rng, n, h, w, c):
    yy = np.linspace(0, 1, h).reshape(1, h, 1, 1)
    xx = np.linspace(0, 1, w).reshape(1, 1, w, 1)
    a, b = rng.uniform(-1, 1, (2, n, 1, 1, c))
    return 0.6 * (a * np.cos(3 * yy + b) + b * np.sin(4 * xx * (1 + a)))


def _data(h, w, c):
    """x [6,h,w,c], y [2,h,w,c] float32 in [-1, 1]: x is its target plus noise, so SSIM is well inside (0, 1)."""
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    y = np.clip(_smooth(rng, 2, h, w, c) + 0.2 * rng.uniform(-1, 1, (2, h, w, c)), -1, 1).astype(np.float32)
    x = np.clip(y[np.arange(6) % 2] + 0.3 * rng.uniform(-1, 1, (6, h, w, c)), -1, 1).astype(np.float32)
    y[1] = -0.5          # a constant target ...
    x[3] = 0.25          # ... and a constant image against it (x[1], x[5]: noisy images against a constant)
    x[4] = y[0]          # an identical pair
    return x, y


def _device(a, shift=0):
    """a on the device between two guard bands of NaN / 1e30; shift moves it off 16-byte alignment."""
    flat = torch.from_numpy(a).reshape(-1)
    buf = torch.empty(GUARD + shift + flat.numel() + GUARD, dtype=torch.float32)
    buf[0::2], buf[1::2] = float("nan"), 1e30
    buf[GUARD + shift:GUARD + shift + flat.numel()] = flat
    buf = buf.cuda()
    view = buf[GUARD + shift:GUARD + shift + flat.numel()].view(a.shape)
    assert (view.data_ptr() % 16 == 0) == (shift % 4 == 0)
    return view, buf


def _run(xd, yd, data_range=L):
    """The op on device views; checks the bands of out and returns the n rows as numpy."""
    M = pkg_mod("metrics")
    n = xd.shape[0]
    out = torch.full((1 + n + EXTRA_ROWS, 4), SENTINEL, dtype=torch.float64, device="cuda")
    got = M.image_metrics(xd, yd, data_range, out=out[1:])
    assert got.shape == (n, 4) and got.data_ptr() == out[1].data_ptr()
    host = out.cpu().numpy()
    assert np.all(host[0] == SENTINEL) and np.all(host[1 + n:] == SENTINEL)  # nothing outside the n rows is written
    return host[1:1 + n].copy()


@pytest.fixture(scope="module")
def cases():
    """Per shape: the host data, the reference with its bound, and the batched device result (computed once,
    shared, never modified)."""
    assert pkg_mod("_lib").METRICS_TILE == TILE
    out = {}
    for h, w, c in SHAPES:
        x, y = _data(h, w, c)
        want, bound = metrics_ref.metrics_ref(x, y, L)
        xd, xbuf = _device(x)
        yd, ybuf = _device(y)
        got = _run(xd, yd)
        for buf, a in ((xbuf, x), (ybuf, y)):  # the inputs and their bands are untouched
            host = buf.cpu().numpy()
            assert np.array_equal(host[GUARD:GUARD + a.size], a.ravel())
            assert np.all(np.isnan(host[:GUARD:2])) and np.all(host[1:GUARD:2] == np.float32(1e30))
        out[(h, w, c)] = dict(x=x, y=y, want=want, bound=bound, got=got)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_batched_call_matches_the_reference(cases, shape):
    k = cases[shape]
    err = np.abs(k["got"] - k["want"])
    print("%s: max error sse %.3e sae %.3e ssim %.3e; ssim bound %.3e .. %.3e" % (
        shape, err[:, 0].max(), err[:, 1].max(), err[:, 2].max(), k["bound"][:, 2].min(), k["bound"][:, 2].max()))
    metrics_ref.assert_rows(k["got"], k["want"], k["bound"], str(shape))
    assert np.all(k["got"][4, :2] == 0.0)                     # the identical pair: exactly zero error
    assert abs(k["got"][4, 2] - 1.0) <= k["bound"][4, 2]
    a, b, c1 = 0.25, -0.5, (0.01 * L) ** 2                    # the constant pair: the closed form
    assert abs(k["got"][3, 2] - (2 * a * b + c1) / (a * a + b * b + c1)) <= k["bound"][3, 2]
    assert np.all(k["got"][:, 3] == 0.0)
    assert np.all(k["bound"][:, 2] < 1e-9)                    # the bound is a rounding bound, not a tolerance


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_equal_the_single_image_calls_bit_for_bit(cases, shape):
    """n = 1: row i of the batched call depends on image i and target i % ny only."""
    k = cases[shape]
    for i in range(6):
        xd, _ = _device(k["x"][i:i + 1])
        yd, _ = _device(k["y"][i % 2:i % 2 + 1])
        one = _run(xd, yd)
        assert one.tobytes() == k["got"][i:i + 1].tobytes(), i
    metrics_ref.assert_rows(one, k["want"][5:6], k["bound"][5:6], "n = 1, %s" % (shape,))


@pytest.mark.parametrize("shape", [(12, 13, 3), (64, 64, 3), (TILE + 11, 2 * TILE + 11, 2)])
def test_two_calls_and_any_alignment_give_the_same_bytes(cases, shape):
    """Off 16-byte alignment the elementwise pass takes 4-byte loads: the same values in the same order."""
    k = cases[shape]
    xd, _ = _device(k["x"])
    yd, _ = _device(k["y"])
    assert _run(xd, yd).tobytes() == k["got"].tobytes()
    for sx, sy in ((1, 0), (0, 2), (3, 1)):
        xs, _ = _device(k["x"], sx)
        ys, _ = _device(k["y"], sy)
        assert _run(xs, ys).tobytes() == k["got"].tobytes(), (sx, sy)


def test_a_nan_is_counted_and_leaves_the_other_rows_intact(cases):
    k = cases[(12, 13, 3)]
    x = k["x"].copy()
    x[2, 5, 7, 1] = np.nan
    xd, _ = _device(x)
    yd, _ = _device(k["y"])
    got = _run(xd, yd)
    want, bound = metrics_ref.metrics_ref(x, k["y"], L)
    assert got[:, 3].tolist() == [0, 0, 1, 0, 0, 0]
    metrics_ref.assert_rows(got, want, bound, "one NaN")
    keep = [0, 1, 3, 4, 5]
    assert got[keep].tobytes() == k["got"][keep].tobytes()
    y = k["y"].copy()
    y[1, 0, 0, 0] = np.inf  # in a target: every image scored against it reports it
    yd, _ = _device(y)
    got = _run(xd, yd)
    assert got[:, 3].tolist() == [0, 1, 1, 1, 0, 1]
    assert got[[0, 4]].tobytes() == k["got"][[0, 4]].tobytes()


def test_stack_input_data_range_and_a_side_stream(cases):
    """x as [k,B,H,W,C] is the same launch; data_range enters C1 and C2 only; the launch follows its stream."""
    M = pkg_mod("metrics")
    k = cases[(32, 32, 1)]
    xd, _ = _device(k["x"])
    yd, _ = _device(k["y"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = M.image_metrics(xd.view(3, 2, 32, 32, 1), yd, L)
    s.synchronize()
    assert got.shape == (6, 4) and got.cpu().numpy().tobytes() == k["got"].tobytes()
    want, bound = metrics_ref.metrics_ref(k["x"], k["y"], 1.0)
    got1 = _run(xd, yd, 1.0)
    metrics_ref.assert_rows(got1, want, bound, "data_range 1")
    assert np.array_equal(got1[:, :2], k["got"][:, :2]) and not np.array_equal(got1[:3, 2], k["got"][:3, 2])
    with pytest.raises(ValueError):
        M.image_metrics(xd, yd[:, :31], L)
    with pytest.raises(RuntimeError, match="image_metrics"):
        M.image_metrics(xd[:5], yd, L)
