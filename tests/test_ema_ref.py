"""CPU checks of tests/ema_ref.py (the restatement the GPU tests hold svae_op_ema and the trainer to) and of the new
entry points' ctypes signatures."""
import ctypes

import numpy as np

import ema_ref as er
from conftest import pkg_mod


def test_warmup_schedule():
    # min(decay, (1 + n) / (10 + n)): TF's num_updates rule
    assert er.decay_t(0.999, 0) == 0.1
    assert er.decay_t(0.999, 1) == 2.0 / 11.0
    assert er.decay_t(0.999, 9) == 10.0 / 19.0
    assert er.decay_t(0.999, 10 ** 6) == 0.999
    # the cross-over: (1 + n) / (10 + n) reaches 0.999 at n = 8990
    assert er.decay_t(0.999, 8989) < 0.999 and er.decay_t(0.999, 8991) == 0.999
    assert er.decay_t(0.05, 0) == 0.05  # a decay below the ramp is never raised
    assert er.omd(0.999, 0) == np.float32(0.9) and er.omd(0.999, 0).dtype == np.float32
    assert er.omd(0.999, 10 ** 6) == np.float32(1.0 - 0.999)


def test_schedule_without_warmup_and_with_every():
    assert er.decay_t(0.999, 0, warmup=False) == 0.999
    assert er.omd(0.999, 0, warmup=False) == np.float32(1.0 - 0.999)
    assert er.omd(0.999, 0, warmup=False, every=3) == np.float32(1.0 - 0.999 ** 3)
    assert er.omd(0.999, 1, warmup=True, every=3) == np.float32(1.0 - (2.0 / 11.0) ** 3)
    # every = 3 averages steps 3 and 6 of 1 .. 7, each as one update of the count
    w = [np.full(8, float(k), np.float32) for k in range(1, 8)]
    e, n = er.track(np.zeros(8, np.float32), w, 6, 0.5, warmup=False, every=3)
    assert n == 2
    want = er.update(er.update(np.zeros(6, np.float32), w[2][:6], er.omd(0.5, 0, False, 3)), w[5][:6],
                     er.omd(0.5, 1, False, 3))
    np.testing.assert_array_equal(e[:6], want)
    np.testing.assert_array_equal(e[6:], 0.0)  # the dead tail never moves


def test_restatement_against_fp64():
    """Three fp32 roundings: the difference (its error is scaled by omd), the product, the result; half an ulp
    each, here bounded by one."""
    rng = np.random.default_rng(0)
    e = rng.standard_normal(1 << 16).astype(np.float32)
    w = (e + rng.standard_normal(e.size).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 1, e.size)
         ).astype(np.float32)
    u = 2.0 ** -23  # one ulp, relative
    for omd in (np.float32(2.0 ** -10), np.float32(0.1), np.float32(1.0)):
        got = er.update(e, w, omd).astype(np.float64)
        d = e.astype(np.float64) - w.astype(np.float64)
        p = float(omd) * d
        exact = e.astype(np.float64) - p
        bound = u * (float(omd) * np.abs(d) + np.abs(p) + np.abs(exact)) + 1e-45
        assert (np.abs(got - exact) <= bound).all()
    # omd = 1 on well-separated values returns w up to those roundings, omd = 0 returns e exactly
    np.testing.assert_array_equal(er.update(e, w, np.float32(0.0)), e)
    np.testing.assert_array_equal(er.update(e, e, np.float32(0.3)), e)


def test_restatement_propagates_nonfinite():
    e = np.array([1.0, 1.0, 1.0, np.inf, 2.0], np.float32)
    w = np.array([np.nan, np.inf, -np.inf, np.inf, 3.0], np.float32)
    r = er.update(e, w, np.float32(0.5))
    assert np.isnan(r[0]) and r[1] == np.inf and r[2] == -np.inf and np.isnan(r[3]) and r[4] == 2.5


def test_signatures_load(built_lib):
    L = pkg_mod("_lib")
    lib = L._load(built_lib)
    vp, f32, i64, i32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64, ctypes.c_int32
    assert lib.svae_op_ema.argtypes == [vp, vp, i64, f32, vp] and lib.svae_op_ema.restype == i32
    assert lib.svae_set_ema.argtypes == [vp, vp, f32] and lib.svae_set_ema.restype == i32
    assert {"svae_op_ema", "svae_set_ema"} <= set(L.EXPORTED)
    # the host-side argument checks run before any device call
    assert lib.svae_op_ema(None, None, 4, 0.5, None) == -2
    assert b"null" in lib.svae_last_error(None)
    assert lib.svae_set_ema(None, None, 0.5) == -2
