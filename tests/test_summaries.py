"""CPU checks of the training summaries: the host plan of svae_op_tensor_stats (pure host, through ctypes), the
scalar names a configuration produces, and the ABI list."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg_mod

I64P = ctypes.POINTER(ctypes.c_int64)


def _chunk():
    L = pkg_mod("_lib")
    txt = open(os.path.join(ROOT, "include", "svae_hip.h")).read()
    assert int(re.search(r"#define SVAE_STATS_CHUNK (\d+)", txt).group(1)) == L.STATS_CHUNK
    return L.STATS_CHUNK


def _segments():
    """The lengths the issue names, in this order, with gaps of 0 .. 70 elements between them (so the offsets
    take every residue mod 4)."""
    C = _chunk()
    lengths = [0, 1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5]
    gaps = [5, 0, 2, 64, 1, 7, 0, 70, 3, 6, 9]
    offsets, pos = [], 0
    for n, g in zip(lengths, gaps):
        pos += g
        offsets.append(pos)
        pos += n
    return offsets, lengths


def _plan(offsets, lengths, cap=None, table=True):
    lib = pkg_mod("_lib").lib()
    off, ln = np.asarray(offsets, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    n = len(offsets)
    count = lib.svae_op_stats_plan(off.ctypes.data_as(I64P), ln.ctypes.data_as(I64P), n, None, 0)
    if not table or count < 0:
        return count, None
    cap = n + 1 + 2 * count if cap is None else cap
    tab = np.full(max(cap, 1), -7, dtype=np.int64)
    rc = lib.svae_op_stats_plan(off.ctypes.data_as(I64P), ln.ctypes.data_as(I64P), n, tab.ctypes.data_as(I64P), cap)
    return rc, tab


def test_plan_covers_every_segment_once_in_order(built_lib):
    C = _chunk()
    offsets, lengths = _segments()
    n = len(offsets)
    count, _ = _plan(offsets, lengths, table=False)
    rc, tab = _plan(offsets, lengths)
    assert rc == count > 0
    first = tab[:n + 1]
    assert first[0] == 0 and first[n] == count and np.all(np.diff(first) >= 0)
    begin = tab[n + 1::2][:count]
    word = tab[n + 2::2][:count]
    seg, length = word >> 32, word & 0xFFFFFFFF
    assert tab.size == n + 1 + 2 * count
    for s in range(n):
        k0, k1 = first[s], first[s + 1]
        if lengths[s] == 0:
            assert k0 == k1  # the empty segment has no chunk
            continue
        assert k1 > k0 and np.all(seg[k0:k1] == s)
        assert np.all(length[k0:k1] >= 1) and np.all(length[k0:k1] <= C)  # no chunk exceeds CHUNK
        # covered exactly once and in order: every chunk starts where the one before ended
        assert begin[k0] == offsets[s]
        assert np.all(begin[k0 + 1:k1] == begin[k0:k1 - 1] + length[k0:k1 - 1])
        assert begin[k1 - 1] + length[k1 - 1] == offsets[s] + lengths[s]  # and none crosses the segment's end
        # the cuts lie at (offset & ~3) + k * CHUNK: 16-byte groups are never split between chunks
        assert np.all((begin[k0 + 1:k1] - (offsets[s] & ~3)) % C == 0)
    assert seg.tolist() == sorted(seg.tolist())


def test_plan_chunk_counts_at_the_thresholds(built_lib):
    C = _chunk()
    for off, n, want in [(0, C - 1, 1), (0, C, 1), (0, C + 1, 2), (0, 3 * C + 5, 4), (1, C - 1, 1), (1, C, 2),
                         (3, 1, 1), (3, 2, 1), (8, 0, 0)]:
        assert _plan([off], [n], table=False)[0] == want, (off, n)
    assert _plan([], [], table=False)[0] == 0


def test_plan_refuses_a_small_table_and_bad_segments(built_lib):
    L = pkg_mod("_lib")
    offsets, lengths = _segments()
    count, _ = _plan(offsets, lengths, table=False)
    need = len(offsets) + 1 + 2 * count
    rc, tab = _plan(offsets, lengths, cap=need - 1)
    assert rc == -2  # SVAE_EBADARG
    msg = L.lib().svae_last_error(None).decode()
    assert str(need - 1) in msg and str(need) in msg
    assert np.all(tab == -7)  # nothing written
    for off, ln in [([4, 0], [2, 2]), ([0, 3], [4, 2]), ([-1], [2]), ([0], [-2])]:
        assert _plan(off, ln, table=False)[0] == -2, (off, ln)


def test_python_plan_wrapper(built_lib):
    S = pkg_mod("summaries")
    offsets, lengths = _segments()
    rc, tab = _plan(offsets, lengths)
    table, n_chunks = S.stats_plan(offsets, lengths)
    assert n_chunks == rc and np.array_equal(table, tab)


def _step_names(t, imp=False):
    names = ["reconstruction_loss_step_%d" % t, "regularization_loss_step_%d" % t,
             "latent_mean_avg_magnitude_step_%d" % t, "latent_mean_avg_step_%d" % t, "latent_stddev_avg_step_%d" % t,
             "training_stddev_avg_magnitude_step_%d" % t]
    return names + (["improvement_maximization_loss_step_%d" % t] if imp and t >= 1 else [])


NORMS = ["theta_weights_norm", "phi_weights_norm", "theta_elbo_grads_norm", "phi_elbo_grads_norm",
         "theta_elbo_update_ratio", "phi_elbo_update_ratio"]
DEBUG = ["debug/theta_grads_clipped_fraction", "debug/phi_grads_clipped_fraction", "debug/theta_grads_max_abs",
         "debug/phi_grads_max_abs", "debug/grads_nonfinite", "debug/weights_nonfinite"]
TINY = ["loss",
        "reconstruction_loss_step_0", "regularization_loss_step_0", "latent_mean_avg_magnitude_step_0",
        "latent_mean_avg_step_0", "latent_stddev_avg_step_0", "training_stddev_avg_magnitude_step_0",
        "reconstruction_loss_step_1", "regularization_loss_step_1", "latent_mean_avg_magnitude_step_1",
        "latent_mean_avg_step_1", "latent_stddev_avg_step_1", "training_stddev_avg_magnitude_step_1",
        "reconstruction_loss_step_2", "regularization_loss_step_2", "latent_mean_avg_magnitude_step_2",
        "latent_mean_avg_step_2", "latent_stddev_avg_step_2", "training_stddev_avg_magnitude_step_2"] + NORMS + DEBUG


def test_summary_names():
    S, preset = pkg_mod("summaries"), pkg_mod("config").preset
    assert S.summary_names(preset("tiny")) == TINY
    # chain noise with a predicted stddev changes values, not names
    assert S.summary_names(preset("tiny", add_noise_to_chain=True, predict_generator_noise=True)) == TINY
    imp = S.summary_names(preset("tiny", add_improvement_maximization_loss=True))
    assert imp == (["loss"] + _step_names(0, True) + _step_names(1, True) + _step_names(2, True) + NORMS +
                   ["phi_latent_pred_grads_norm", "phi_latent_pred_update_ratio"] + DEBUG)
    assert [n for n in imp if n.startswith("improvement")] == ["improvement_maximization_loss_step_1",
                                                               "improvement_maximization_loss_step_2"]
    for cfg in (preset("tiny"), preset("celeba", add_noise_to_chain=True, predict_generator_noise=True),
                preset("c_homog_imp_max_var_pred")):
        names = S.summary_names(cfg)
        assert len(names) == len(set(names))
        assert not [n for n in names if "resnet_gate" in n or n.startswith("classic_")]
    assert len(S.summary_names(preset("celeba"))) == 1 + 6 * 8 + 6 + 6


def test_entry_points_are_exported(built_lib):
    L = pkg_mod("_lib")
    assert "svae_op_tensor_stats" in L.EXPORTED and "svae_op_stats_plan" in L.EXPORTED
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "svae_op_tensor_stats") and hasattr(lib, "svae_op_stats_plan")


def test_tensor_stats_rejects_bad_arguments_without_a_gpu(built_lib):
    """Argument checks come before any launch, so they hold on a machine without a device."""
    lib = pkg_mod("_lib").lib()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused
    inf = float("inf")
    assert lib.svae_op_tensor_stats(None, p, 1, 1, inf, p, p, None) == -2
    assert lib.svae_op_tensor_stats(p, None, 1, 1, inf, p, p, None) == -2
    assert lib.svae_op_tensor_stats(p, p, 1, 1, inf, None, p, None) == -2
    assert lib.svae_op_tensor_stats(p, p, 1, 1, inf, p, None, None) == -2
    assert lib.svae_op_tensor_stats(p, p, -1, 1, inf, p, p, None) == -2
    assert lib.svae_op_tensor_stats(p, p, 1, -1, inf, p, p, None) == -2
    assert lib.svae_op_tensor_stats(p, p, 1, 1, -1.0, p, p, None) == -2
    assert lib.svae_op_tensor_stats(p, p, 1, 1, float("nan"), p, p, None) == -2


def test_reference_columns():
    """tests/stats_ref.py on a case small enough to state by hand."""
    import stats_ref
    x = np.array([1.0, -3.0, np.nan, 12.0, np.inf, -0.5, 99.0], dtype=np.float32)
    rows, bound = stats_ref.stats_ref(x, [0, 6], [6, 0], 10.0)
    assert rows[0].tolist() == [4.0, 1.0 - 3.0 + 10.0 - 0.5, 14.5, 1.0 + 9.0 + 100.0 + 0.25, 12.0, 1.0, 2.0, 0.0]
    assert rows[1].tolist() == [0.0] * 8 and bound[1].tolist() == [0.0] * 8
    assert bound[0, 0] == bound[0, 4] == bound[0, 5] == bound[0, 6] == 0.0 and bound[0, 1] == 4 * 2.0 ** -52 * 14.5
