"""svae_op_power_spectrum on the GPU against tests/spectrum_ref.py, bit for bit.

The restatement performs the op's operations in the op's order, each rounded once, so the comparison is of bytes, not
within a tolerance.  Shapes (n, ny, h, w, c): odd sizes without a Nyquist column, the stack rule with the Nyquist
multiplicity, h != w, 28 x 28, the presets' 64 x 64 x 3 and one image at SVAE_SPECTRUM_MAX_DIM square.  out sits
between guard bands of NaN and nonfinite between sentinels; x and y sit between bands of NaN and 1e30, so a stray
read shows in a row and a stray write in a band.
"""
import ctypes

import numpy as np
import pytest
import torch

import spectrum_ref
from conftest import pkg_mod

pytestmark = pytest.mark.gpu

GUARD = 256  # floats / doubles (a multiple of 4: the arrays stay 16-byte aligned)
SENTINEL = -12345.678
MAX_DIM = 96  # SVAE_SPECTRUM_MAX_DIM, asserted below
SHAPES = [(5, 5, 7, 9, 3), (6, 2, 8, 8, 1), (3, 3, 12, 5, 3), (4, 2, 28, 28, 1), (2, 1, 64, 64, 3),
          (1, 1, MAX_DIM, MAX_DIM, 1)]


def _tables(h, w, kind="hann"):
    S = pkg_mod("spectra")
    table, n_bins, _ = S.radial_bins(h, w)
    return dict(win_y=S.window(h, kind), win_x=S.window(w, kind), tw_y=S.twiddles(h), tw_x=S.twiddles(w), table=table,
                n_bins=n_bins)


def _data(n, ny, h, w, c):
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    y = rng.normal(0, 0.5, (ny, h, w, c)).astype(np.float32)
    x = (y[np.arange(n) % ny] + rng.normal(0, 0.2, (n, h, w, c))).astype(np.float32)
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
    return view


def _run(xd, yd, t, fill=float("nan")):
    """The op on device views with the tables t; checks the bands and returns (out [n,c,2,n_bins], nonfinite [n,c])."""
    L = pkg_mod("_lib")
    n, h, w, c = xd.shape
    nb = t["n_bins"]
    size = n * c * 2 * nb
    out = torch.full((GUARD + size + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    out[GUARD:GUARD + size] = fill
    bad = torch.full((1 + n * c + 1,), -7, dtype=torch.int64, device="cuda")
    dev = {k: torch.from_numpy(np.ascontiguousarray(t[k])).cuda() for k in ("win_y", "win_x", "tw_y", "tw_x", "table")}
    assert dev["table"].dtype == torch.int32 and dev["tw_x"].shape == (w, 2)
    L.check(L.lib().svae_op_power_spectrum(
        L.ptr(xd), n, L.ptr(yd), n if yd is None else yd.shape[0], h, w, c, L.ptr(dev["win_y"]), L.ptr(dev["win_x"]),
        L.ptr(dev["tw_y"]), L.ptr(dev["tw_x"]), L.ptr(dev["table"]), nb, L.ptr(out[GUARD:]), L.ptr(bad[1:]),
        L.stream_ptr()))
    host, hbad = out.cpu().numpy(), bad.cpu().numpy()
    assert np.all(np.isnan(host[:GUARD])) and np.all(np.isnan(host[GUARD + size:]))  # nothing outside is written
    assert hbad[0] == -7 and hbad[-1] == -7
    return host[GUARD:GUARD + size].reshape(n, c, 2, nb).copy(), hbad[1:-1].reshape(n, c).copy()


def _ref(x, y, t):
    return spectrum_ref.power_spectrum_ref(x, y, t["win_y"], t["win_x"], t["tw_y"], t["tw_x"], t["table"], t["n_bins"])


@pytest.fixture(scope="module")
def cases():
    """Per shape: the host data, the tables, the reference and the device result (computed once, shared, never
    modified)."""
    assert pkg_mod("_lib").SPECTRUM_MAX_DIM == MAX_DIM
    out = {}
    for shape in SHAPES:
        n, ny, h, w, c = shape
        x, y = _data(n, ny, h, w, c)
        t = _tables(h, w)
        want, wbad = _ref(x, y, t)
        got, bad = _run(_device(x), _device(y), t)
        out[shape] = dict(x=x, y=y, t=t, want=want, wbad=wbad, got=got, bad=bad)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_op_equals_the_restatement_bit_for_bit(cases, shape):
    k = cases[shape]
    rel = np.abs(k["got"] - k["want"]).max() / np.abs(k["want"]).max()
    print("%s: largest difference %.2e of the largest value" % (shape, rel))
    assert np.all(np.isfinite(k["got"])) and np.all(k["got"] >= 0.0)
    assert k["got"].tobytes() == k["want"].tobytes()
    assert np.all(k["bad"] == 0) and np.array_equal(k["bad"], k["wbad"])


@pytest.mark.parametrize("shape", SHAPES[:5])
def test_rows_do_not_depend_on_the_batch_and_two_calls_agree(cases, shape):
    """Row (i, k) depends on image i and its partner only: single-image calls give the batched rows; a second
    batched call gives the same bytes."""
    k = cases[shape]
    n, ny = shape[:2]
    again, _ = _run(_device(k["x"]), _device(k["y"]), k["t"])
    assert again.tobytes() == k["got"].tobytes()
    for i in (0, n - 1):
        one, _ = _run(_device(k["x"][i:i + 1]), _device(k["y"][i % ny:i % ny + 1]), k["t"])
        assert one.tobytes() == k["got"][i:i + 1].tobytes(), i


@pytest.mark.parametrize("shape", [(5, 5, 7, 9, 3), (6, 2, 8, 8, 1), (2, 1, 64, 64, 3)])
def test_any_alignment_gives_the_same_bytes(cases, shape):
    """Off a 16-byte boundary the images are loaded element by element: the same values in the same order."""
    k = cases[shape]
    for sx, sy in ((1, 0), (0, 2), (3, 1)):
        got, bad = _run(_device(k["x"], sx), _device(k["y"], sy), k["t"])
        assert got.tobytes() == k["got"].tobytes(), (sx, sy)
        assert np.all(bad == 0)


def test_inputs_spanning_twenty_powers_of_e():
    n, ny, h, w, c = 4, 2, 12, 10, 3
    rng = np.random.default_rng(5)
    mag = lambda *s: (np.exp(rng.uniform(-10, 10, s)) * rng.choice([-1.0, 1.0], s)).astype(np.float32)
    x, y = mag(n, h, w, c), mag(ny, h, w, c)
    for kind in ("hann", "none"):
        t = _tables(h, w, kind)
        want, _ = _ref(x, y, t)
        got, bad = _run(_device(x), _device(y), t)
        assert got.tobytes() == want.tobytes() and np.all(bad == 0), kind


def test_without_y_plane_one_is_not_touched(cases):
    shape = (5, 5, 7, 9, 3)
    k = cases[shape]
    got, bad = _run(_device(k["x"]), None, k["t"], fill=SENTINEL)
    assert got[:, :, 0].tobytes() == k["got"][:, :, 0].tobytes()
    assert np.all(got[:, :, 1] == SENTINEL)
    assert np.all(bad == 0)


def test_skipped_entries_and_an_empty_bin(cases):
    """-1 and out-of-range entries are left out, a bin no entry maps to is written 0, a coarser table sums alike."""
    shape = (4, 2, 28, 28, 1)
    k = cases[shape]
    t = dict(k["t"])
    table = t["table"].copy()
    table[table == 3] = -1          # an annulus dropped: bin 3 is empty
    table[5, 2] = 9999              # outside [0, n_bins): skipped like -1
    table[table >= 10] += 2         # bins 10 and 11 are empty too
    t["table"], t["n_bins"] = table, t["n_bins"] + 2
    want, _ = _ref(k["x"], k["y"], t)
    got, _ = _run(_device(k["x"]), _device(k["y"]), t, fill=SENTINEL)
    assert got.tobytes() == want.tobytes()
    assert np.all(got[..., [3, 10, 11]] == 0.0) and np.all(got[..., [0, 1, 2, 4, 9, 12]] > 0.0)
    assert np.array_equal(got[..., 12:], k["got"][..., 10:])  # the untouched annuli keep their bytes


def test_a_nan_is_counted_and_leaves_the_other_rows_intact(cases):
    shape = (5, 5, 7, 9, 3)
    k = cases[shape]
    x = k["x"].copy()
    x[2, 5, 7, 1] = np.nan
    x[2, 0, 0, 1] = np.inf
    got, bad = _run(_device(x), _device(k["y"]), k["t"])
    want_bad = np.zeros((5, 3), dtype=np.int64)
    want_bad[2, 1] = 2
    assert np.array_equal(bad, want_bad)
    assert not np.any(np.isfinite(got[2, 1]))           # both planes of the row that read it
    keep = np.ones((5, 3), dtype=bool)
    keep[2, 1] = False
    assert got[keep].tobytes() == k["got"][keep].tobytes()
    y = k["y"].copy()
    y[4, 3, 3, 0] = -np.inf                             # in a partner: plane 1 only
    got, bad = _run(_device(k["x"]), _device(y), k["t"])
    want_bad[:] = 0
    want_bad[4, 0] = 1
    assert np.array_equal(bad, want_bad)
    assert got[4, 0, 0].tobytes() == k["got"][4, 0, 0].tobytes() and not np.any(np.isfinite(got[4, 0, 1]))


def test_identical_images_give_an_error_plane_of_exactly_zero(cases):
    shape = (6, 2, 8, 8, 1)
    k = cases[shape]
    x = np.concatenate([k["y"]] * 3)
    got, _ = _run(_device(x), _device(k["y"]), k["t"])
    assert np.all(got[:, :, 1] == 0.0) and not np.any(np.signbit(got[:, :, 1]))
    assert np.all(got[:, :, 0].sum(-1) > 0.0)
    assert got[:2, :, 0].tobytes() == got[2:4, :, 0].tobytes()


def test_wrapper_stack_input_window_and_a_side_stream(cases):
    """spectra.power_spectrum: x as [k,B,H,W,C] is the same launch, its cached tables are the module's, the launch
    follows its stream, and bad arguments raise."""
    S = pkg_mod("spectra")
    shape = (6, 2, 8, 8, 1)
    k = cases[shape]
    xd, yd = _device(k["x"]), _device(k["y"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    bad = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(s):
        got = S.power_spectrum(xd.view(3, 2, 8, 8, 1), yd, nonfinite=bad)
    s.synchronize()
    assert got.shape == (6, 1, 2, 5) and got.cpu().numpy().tobytes() == k["got"].tobytes()
    assert bad.tolist() == [0] * 6
    alone = S.power_spectrum(xd)                       # y = None: plane 1 of a fresh result reads 0
    assert alone[:, :, 0].cpu().numpy().tobytes() == k["got"][:, :, 0].tobytes()
    assert torch.all(alone[:, :, 1] == 0.0)
    want, _ = _ref(k["x"], k["y"], _tables(8, 8, "none"))
    assert S.power_spectrum(xd, yd, window="none").cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        S.power_spectrum(xd, yd[:, :7])
    with pytest.raises(ValueError):
        S.power_spectrum(xd, yd, window="hamming")
    with pytest.raises(RuntimeError, match="power_spectrum"):
        S.power_spectrum(xd[:5], yd)
    big = torch.zeros(1, pkg_mod("_lib").SPECTRUM_MAX_DIM + 2, 8, 1, device="cuda")
    with pytest.raises(RuntimeError, match="power_spectrum"):
        S.power_spectrum(big)
