"""The context-free entry points (svae_op_make_batch ... svae_op_ema): one call each that fails at the op's first
argument check.  The check runs on the host before any device call, so the pointers are never read and no GPU is
needed; the code and the prefix of svae_last_error(NULL) show that the symbol is bound to that op's own checks.
"""
import ctypes

import pytest

from conftest import pkg_mod

EBADARG = -2
P = ctypes.c_void_p(0x1000)  # never read

# (symbol, arguments with the first-checked one bad, prefix of the message)
CASES = [
    ("svae_op_make_batch", (None, 1, None, 0, 4, 16, 0.0, 1.0, 0.0, 0.0, 0.0, 1, 0, P, P, None), b"make_batch:"),
    ("svae_op_degrade_batch", (None, 4, 8, 8, 3, 0.0, 1.0, None, 1, 0, P, None, None), b"degrade_batch:"),
    ("svae_op_crop_batch", (None, 1, 2, 32, 32, 3, 8, 8, None, None, 1, 0, 4, 0.0, 1.0, P, None, None, None),
     b"crop_batch:"),
    ("svae_op_jpeg_batch", (None, 4, 16, 16, 3, 0.0, 1.0, None, 1, 0, P, None, None), b"jpeg_batch:"),
    ("svae_op_extract_tiles", (None, 1, 2, 32, 32, 3, 8, 8, 4, 4, 0.0, 1.0, 0, 1, P, None), b"extract_tiles:"),
    ("svae_op_blend_tiles", (None, 1, 0, 2, 32, 32, 3, 8, 8, 4, 4, None, 0, None, 0.0, 1.0, P, None, None),
     b"blend_tiles:"),
    ("svae_op_stats_plan", (None, None, -1, None, 0), b"stats_plan:"),
    ("svae_op_tensor_stats", (None, P, 1, 1, 1.0, P, P, None), b"tensor_stats:"),
    ("svae_op_image_metrics", (None, 4, P, 2, 16, 16, 3, 1.0, P, None), b"image_metrics:"),
    ("svae_op_mixture_logdensity", (None, 8, 4, P, P, 8, 4, 4, None, 1, P, None), b"mixture_logdensity:"),
    ("svae_op_pairwise_stats", (None, 8, 4, None, None, None, 1, 4, -1, None, 0, None, P, P, P, None),
     b"pairwise_stats:"),
    ("svae_op_power_spectrum", (None, 4, P, 2, 8, 8, 3, P, P, P, P, P, 5, P, None, None), b"power_spectrum:"),
    ("svae_op_ema", (None, P, 16, 0.5, None), b"ema:"),
]


@pytest.mark.parametrize("symbol,args,prefix", CASES, ids=[c[0] for c in CASES])
def test_first_check_names_its_op(built_lib, symbol, args, prefix):
    L = pkg_mod("_lib")
    assert symbol in L.EXPORTED
    assert getattr(L.lib(), symbol)(*args) == EBADARG
    assert L.lib().svae_last_error(None).startswith(prefix)


def test_pairwise_scratch_bytes_refuses_a_bad_shape(built_lib):
    L = pkg_mod("_lib")
    m = (ctypes.c_int64 * 1)(8)
    fn = L.lib().svae_op_pairwise_scratch_bytes
    assert fn(0, m, 1, 0) == -1      # no rows
    assert fn(8, None, 1, 0) == -1   # no group sizes
    assert fn(8, m, 1, 0) > 0
