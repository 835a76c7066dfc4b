"""CPU checks of the batch pipeline: the Philox restatement against the Random123 known answers, the new
entry point's export and argument checks (pure host code), the dataset cursor and the canvases."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import batch_ref
from conftest import ROOT, pkg_mod


# ---------------------------------------------------------------------------------- the restatement
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    out = batch_ref.philox4x32_10(*[np.array([c], np.uint64) for c in ctr], *key)
    assert " ".join("%08x" % int(w[0]) for w in out) == want


def test_restatement_counter_layout():
    """Element e draws from group e // 4 at counter offset + group, the carry reaching c1; streams differ."""
    off = 2 ** 32 - 3
    w = batch_ref.words(32, seed=0x123456789ABCDEF, offset=off, stream=1)
    for g in (0, 2, 3, 7):  # groups 3.. have c1 = 1
        ctr = off + g
        one = batch_ref.philox4x32_10(np.uint64(ctr & 0xFFFFFFFF), np.uint64(ctr >> 32), np.uint64(1), np.uint64(0),
                                      0x89ABCDEF, 0x01234567)
        assert [int(x) for x in one] == [int(x) for x in w[4 * g:4 * g + 4]]
    assert not np.array_equal(w, batch_ref.words(32, 0x123456789ABCDEF, off, 2))
    assert batch_ref.threshold(0.0) == 0 and batch_ref.threshold(1.0) == 2 ** 32 - 1
    assert batch_ref.threshold(0.5) == 2 ** 31
    assert batch_ref.threshold(0.1) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32))


def test_restatement_statistics():
    """The restated corruption has the stated rates and unit-variance normals (a wrong comparison
    direction or word-to-lane mapping shows here before any GPU run)."""
    n = 1 << 16
    x = np.full((1, n), 0.25, np.float32)
    r = batch_ref.make_batch(x, None, 0, 1, -1.0, 1.0, 0.1, 0.2, 0.0, seed=5, offset=0)
    v = r["unclipped"].ravel()
    pepper = np.mean((v == 0.0) | (v == 1.0))
    salt = np.mean(v >= 1.0)
    assert abs(pepper - 0.1) < 0.01 and abs(salt - 0.2) < 0.01
    z = batch_ref.normals(n, seed=5, offset=0)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert abs(np.corrcoef(z[0::4], z[1::4])[0, 1]) < 0.03


# ---------------------------------------------------------------------------------- the library
def test_library_exports_make_batch(built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "svae_op_make_batch")
    assert "svae_op_make_batch" in pkg_mod("_lib").EXPORTED
    assert pkg_mod("_lib").lib().svae_op_make_batch.argtypes is not None


GOOD = dict(data=0x1000, u8=0, idx=None, start=0, n=2, per=8, lo=-1.0, hi=1.0, pepper=0.1, salt=0.1, scale=0.1,
            target=0x2000, inp=0x3000)
BAD = [("null data", dict(data=None)), ("both null", dict(target=None, inp=None)),
       ("positive", dict(n=0)), ("positive", dict(n=-3)), ("positive", dict(per=0)),
       ("probability", dict(pepper=-0.01)), ("probability", dict(pepper=1.5)), ("probability", dict(salt=1.01)),
       ("probability", dict(salt=float("nan"))), ("negative", dict(scale=-1.0)), ("lo > hi", dict(lo=1.0, hi=-1.0))]


@pytest.mark.parametrize("msg,over", BAD)
def test_make_batch_rejects_bad_arguments(built_lib, msg, over):
    """Every check runs before any HIP call: fake non-null pointers are never dereferenced."""
    L = pkg_mod("_lib")
    a = dict(GOOD, **over)
    rc = L.lib().svae_op_make_batch(a["data"], a["u8"], a["idx"], a["start"], a["n"], a["per"], a["lo"], a["hi"],
                                    a["pepper"], a["salt"], a["scale"], 1, 0, a["target"], a["inp"], None)
    assert rc == -2
    err = L.lib().svae_last_error(None).decode()
    assert err.startswith("make_batch") and msg in err, err


# ---------------------------------------------------------------------------------- dataset
def _ds(n_train, n_test=8, rng=(-1.0, 1.0), dtype=torch.uint8):
    D = pkg_mod("data").DeviceDataset
    mk = lambda n: (torch.arange(n * 2 * 2 * 1).reshape(n, 2, 2, 1) % 251).to(dtype)
    return D(mk(n_train), mk(n_test), range=rng, name="t")


@pytest.mark.parametrize("size,want", [(12, [(0, 4), (4, 4), (8, 4), (0, 4)]), (10, [(0, 4), (4, 4), (0, 4)])])
def test_cursor_follows_the_reference_rule(size, want):
    ds = _ds(size, size)
    assert [ds.next_batch(4) for _ in want] == want
    assert [ds.next_test_batch(4) for _ in want] == want
    assert ds.state_dict() == {"train_idx": want[-1][0] + 4, "test_idx": want[-1][0] + 4}
    with pytest.raises(ValueError):
        ds.next_batch(size + 1)


def test_from_array_split_and_display():
    D = pkg_mod("data").DeviceDataset
    arr = np.arange(10 * 2 * 2 * 3, dtype=np.uint8).reshape(10, 2, 2, 3)
    ds = D.from_array(arr, range=(0.0, 1.0))
    assert (ds.train_size, ds.test_size, ds.data_dims) == (8, 2, [2, 2, 3])
    np.testing.assert_array_equal(ds.rows((2, 3)).numpy(), arr[2:5])
    np.testing.assert_array_equal(ds.rows((1, 1), test=True).numpy(), arr[9:10])
    x = np.array([-1.5, -1.0, 0.0, 0.5, 1.0, 2.0])
    np.testing.assert_allclose(ds.display(x), [0, 0, 0, 0.5, 1, 1])
    np.testing.assert_allclose(_ds(4).display(x), [0, 0, 0.5, 0.75, 1, 1])
    np.testing.assert_allclose(_ds(4).display(torch.tensor(x)).numpy(), [0, 0, 0.5, 0.75, 1, 1])
    s = D.synthetic(20, 4, 4, 3, seed=1, test_fraction=0.4)
    assert (s.train_size, s.test_size, s.train.dtype) == (12, 8, torch.uint8)
    assert torch.equal(s.train, D.synthetic(20, 4, 4, 3, seed=1, test_fraction=0.4).train)


# ---------------------------------------------------------------------------------- canvases
def _imgs(base, C=1):
    """2 images of 4x4xC, image b filled with base + b / 10."""
    return np.stack([np.full((4, 4, C), base + b / 10.0) for b in range(2)])


@pytest.mark.parametrize("C,border_value", [(1, 0.0), (3, 1.0)])
def test_reconstruction_canvas_cells(C, border_value):
    cv = pkg_mod("canvas")
    o, nz, r = _imgs(0.1, C), _imgs(0.3, C), _imgs(0.5, C)
    c = cv.reconstruction_canvas(o, nz, r)
    assert c.shape == (2 * 4, 3 * 4 + 2 * 10, C)
    for b in range(2):
        rows = slice(4 * b, 4 * b + 4)
        np.testing.assert_array_equal(c[rows, 0:4], o[b])
        np.testing.assert_array_equal(c[rows, 14:18], nz[b])
        np.testing.assert_array_equal(c[rows, 28:32], r[b])
    assert np.all(c[:, 4:14] == border_value) and np.all(c[:, 18:28] == border_value)


def test_chain_canvas_cells():
    cv = pkg_mod("canvas")
    start, m, s = _imgs(0.1), [_imgs(0.2), _imgs(0.3)], [_imgs(0.6), _imgs(0.7)]
    c = cv.chain_canvas(start, m)  # T = 2, no chain noise
    assert c.shape == (2 * 4, 3 * 4, 1)
    for b in range(2):
        for k, col in enumerate([start] + m):
            np.testing.assert_array_equal(c[4 * b:4 * b + 4, 4 * k:4 * k + 4], col[b])
    c = cv.chain_canvas(start, m, s)  # chain noise: MLEs above samples
    assert c.shape == (2 * 2 * 4, 3 * 4, 1)
    for b in range(2):
        np.testing.assert_array_equal(c[8 * b:8 * b + 4, 0:4], start[b])
        assert np.all(c[8 * b + 4:8 * b + 8, 0:4] == 0.0)
        for t in range(2):
            np.testing.assert_array_equal(c[8 * b:8 * b + 4, 4 * (t + 1):4 * (t + 2)], m[t][b])
            np.testing.assert_array_equal(c[8 * b + 4:8 * b + 8, 4 * (t + 1):4 * (t + 2)], s[t][b])


def test_save_canvas_writes_a_file(tmp_path):
    cv = pkg_mod("canvas")
    for C in (1, 3):
        p = cv.save_canvas(np.full((4, 6, C), 0.5), str(tmp_path / "a" / "b"), "x%d" % C)
        assert os.path.exists(p) and os.path.splitext(p)[1] in (".png", ".npy")


def test_train_tool_refuses_an_existing_model_directory(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("svae_train_tool", os.path.join(ROOT, "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = tmp_path / "tiny_v1"
    assert tool.model_dir_error(str(base), True) and tool.model_dir_error(str(base), False) is None
    base.mkdir()
    assert tool.model_dir_error(str(base), False) and tool.model_dir_error(str(base), True) is None
    rc = tool.main(["--netname", "tiny", "--synthetic", "20", "--models_dir", str(tmp_path)])
    assert rc == 1 and "already exists" in capsys.readouterr().out
