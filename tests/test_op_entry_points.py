"""The context-free entry points (svae_op_make_batch ... svae_op_sqdiff_img): one call each that fails at the op's first
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
    ("svae_op_gconv_variant", (16, 16, 4, 1, 2, 8, 8, None), b"gconv_variant:"),
    ("svae_op_gconv_last_kernel", (None,), b"gconv_last_kernel:"),
    ("svae_op_gconv_smalln", (None, 2, 4, 4, 16, P, 3, None, 0, None, None, 1, 2, 0, P, None, None), b"gconv_smalln:"),
    ("svae_op_output_convt", (None, 2, 4, 16, P, None, P, None, 3, 0, P, None, P, None, 0, None, None),
     b"output_convt:"),
    ("svae_op_output_fwd", (None, 2, 4, 4, 3, None, P, 0.0, 1.0, 0.1, 0.9, P, P, P, P, P, None), b"output_fwd:"),
    ("svae_op_output_bwd", (None, 2, 4, 4, 3, None, P, P, 0.0, 1.0, 0.1, 0.9, 1.0, None, P, None, P, None, P, 4096,
                            None), b"output_bwd:"),
    ("svae_op_sd_layer", (None, 3, 0, 2, 4, 4, 3, P, 5, P, P, P, P, P, P, 4096, None), b"sd_layer:"),
    ("svae_op_sd_layer_bwd", (None, P, P, P, P, P, 3, 0, 2, 4, 4, 3, P, 5, 0, P, P, P, P, 3, P, 1 << 20, None),
     b"sd_layer_bwd:"),
    ("svae_op_sd_head_fwd", (None, 5, P, P, 1.0, P, P, P, 0.5, 2, 4, 4, 3, P, P, P, None), b"sd_head_fwd:"),
    ("svae_op_sd_head_bwd", (None, 5, P, P, 1.0, P, P, P, 0.5, 1.0, None, 2, 4, 4, 3, P, P, P, P, P, 4096, None),
     b"sd_head_bwd:"),
    ("svae_op_chain_noise", (None, P, 0.5, 16, P, None), b"chain_noise:"),
    ("svae_op_imp_seed", (None, None, None, None, 0.5, 16, P, None), b"imp_seed:"),
    ("svae_op_sqdiff_img", (None, P, 2, 16, P, None), b"sqdiff_img:"),
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


def test_output_convt_refuses_an_unknown_mode_and_a_missing_bf16_table(built_lib):
    L = pkg_mod("_lib")
    fn = L.lib().svae_op_output_convt
    assert fn(P, 2, 4, 16, P, None, P, None, 3, 3, P, P, P, None, 0, None, None) == EBADARG
    assert L.lib().svae_last_error(None).startswith(b"output_convt: mode")
    for mode in (1, 2):   # the bf16 modes pack into wpack_h
        assert fn(P, 2, 4, 16, P, None, P, None, 3, mode, P, None, P, None, 0, None, None) == EBADARG
        assert b"wpack_h" in L.lib().svae_last_error(None)
    # f1 % 4 == 0 reads 16-byte vectors
    assert fn(ctypes.c_void_p(0x1004), 2, 4, 16, P, None, P, None, 3, 0, P, None, P, None, 0, None, None) == EBADARG
    assert b"16-byte" in L.lib().svae_last_error(None)


def test_sd_entry_points_refuse_a_height_that_is_no_multiple_of_4(built_lib):
    """sd_conv_wgrad covers h / 4 row blocks per image: both layer entry points refuse other heights (make_geo cannot
    let one through: levels >= 2 makes every image size a multiple of 4, and it checks predict_generator_noise again)."""
    L = pkg_mod("_lib")
    assert L.lib().svae_op_sd_layer(P, 3, 0, 2, 6, 8, 3, P, 5, P, P, P, P, P, P, 1 << 20, None) == EBADARG
    assert b"multiple of 4" in L.lib().svae_last_error(None)
    assert L.lib().svae_op_sd_layer_bwd(P, P, P, P, P, P, 3, 0, 2, 6, 8, 3, P, 5, 0, P, P, P, P, 3, P, 1 << 20,
                                        None) == EBADARG
    assert b"multiple of 4" in L.lib().svae_last_error(None)
