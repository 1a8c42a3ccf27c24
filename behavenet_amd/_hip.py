"""ctypes binding of libbehavenet_hip.so (include/behavenet_hip.h).

This module is the only place where Python touches the C ABI.  It hands over raw device
pointers (``tensor.data_ptr()``) and the current HIP stream; PyTorch is used for device memory
and streams only.  There is NO fallback: if the library is missing, or a tensor is not a
contiguous fp32 device tensor, the call raises.
"""

import ctypes
import os

import numpy as np
import torch

_LIB_NAME = 'libbehavenet_hip.so'
# BN_HIP_LIB: an alternative build of the same ABI (tools/build_variant.sh, A/B of two whole libraries)
_LIB_PATH = os.environ.get('BN_HIP_LIB') or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)
_lib = None

ACT_NONE, ACT_LRELU, ACT_SIGMOID = 0, 1, 2

PROF_NONE, PROF_CONV_FWD, PROF_CONV_BWD_D, PROF_CONV_BWD_W = 0, 1, 2, 3
PROF_CONVT_FWD, PROF_CONVT_BWD_D, PROF_CONVT_BWD_W, PROF_ADAM = 4, 5, 6, 7
PROF_LINEAR_FWD, PROF_LINEAR_BWD = 8, 9

_c_int, _c_float, _c_size_t, _c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

_CONV_GEOM = [_c_int] * 12
_ACT_WS = [_c_int, _c_float, _c_void_p, _c_size_t, _c_void_p]   # act, slope, ws, ws_bytes, stream

OP_CONV_FWD, OP_CONV_BWD_D, OP_CONV_BWD_W = 1, 2, 3
OP_CONVT_FWD, OP_CONVT_BWD_D, OP_CONVT_BWD_W = 4, 5, 6

# name -> (restype, argtypes); mirrors include/behavenet_hip.h one to one
SIGNATURES = {
    'bn_version': (_c_int, []),
    'bn_build_arch': (ctypes.c_char_p, []),
    'bn_error_string': (ctypes.c_char_p, [_c_int]),
    'bn_set_force_generic': (_c_int, [_c_int]),
    'bn_set_bigk1_block_bytes': (_c_size_t, [_c_size_t]),
    'bn_conv_ws_bytes': (_c_size_t, [_c_int] + _CONV_GEOM),
    'bn_conv_taps_bytes': (_c_size_t, [_c_int] + _CONV_GEOM),
    'bn_conv_taps_pad': (_c_int, [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    'bn_conv2d_fwd': (_c_int, [_c_void_p] * 5 + _CONV_GEOM + _ACT_WS),
    'bn_conv2d_fwd_u8_ws_bytes': (_c_size_t, _CONV_GEOM + [_c_int]),
    'bn_conv2d_fwd_u8': (_c_int, [_c_void_p] * 4 + _CONV_GEOM + _ACT_WS),
    'bn_conv2d_bwd_data': (_c_int, [_c_void_p] * 5 + _CONV_GEOM + _ACT_WS),
    'bn_conv2d_bwd_weight': (
        _c_int, [_c_void_p] * 4 + _CONV_GEOM + [_c_int, _c_void_p, _c_size_t, _c_void_p]),
    'bn_convT2d_fwd': (_c_int, [_c_void_p] * 5 + _CONV_GEOM + _ACT_WS),
    'bn_convT2d_bwd_data': (_c_int, [_c_void_p] * 5 + _CONV_GEOM + _ACT_WS),
    'bn_convT2d_bwd_weight': (
        _c_int, [_c_void_p] * 4 + _CONV_GEOM + [_c_int, _c_void_p, _c_size_t, _c_void_p]),
    'bn_batchnorm_ws_bytes': (_c_size_t, [_c_int, _c_int]),
    'bn_batchnorm_stats': (_c_int, [_c_void_p] * 3 + [_c_int] * 3 + [_c_void_p, _c_size_t, _c_void_p]),
    'bn_batchnorm_finalize': (_c_int, [_c_void_p] * 5 + [_c_int] + [_c_float] * 3 + [_c_void_p]),
    'bn_batchnorm_act_fwd': (_c_int, [_c_void_p] * 6 + [_c_int] * 4 + [_c_float, _c_void_p]),
    'bn_batchnorm_train_fwd_chunks': (
        _c_int, [_c_void_p] * 11 + [_c_int] * 3 + [_c_float, _c_int, _c_float, _c_void_p, _c_size_t,
                                                  _c_void_p]),
    'bn_batchnorm_act_bwd_chunks': (
        _c_int, [_c_void_p] * 10 + [_c_int, _c_void_p] + [_c_int] * 4 + [_c_float, _c_void_p, _c_size_t,
                                                                        _c_void_p]),
    'bn_batchnorm_act_bwd': (
        _c_int, [_c_void_p] * 9 + [_c_int] * 6 + [_c_float, _c_void_p, _c_size_t, _c_void_p]),
    'bn_batchnorm_moment': (_c_int, [_c_void_p] * 3 + [_c_int] * 3 + [_c_void_p, _c_size_t, _c_void_p]),
    'bn_batchnorm_bwd_reduce': (
        _c_int, [_c_void_p] * 7 + [_c_int] * 4 + [_c_float, _c_void_p, _c_size_t, _c_void_p]),
    'bn_batchnorm_bwd_apply': (
        _c_int, [_c_void_p] * 9 + [_c_int] * 3 + [_c_float, _c_int, _c_float, _c_void_p]),
    'bn_maxpool2d_fwd': (_c_int, [_c_void_p] * 3 + [_c_int] * 9 + [_c_void_p]),
    'bn_maxpool2d_bwd': (_c_int, [_c_void_p] * 3 + [_c_int] * 9 + [_c_void_p]),
    'bn_maxpool2d_act_fwd': (_c_int, [_c_void_p] * 3 + [_c_int] * 4 + [ctypes.c_float, _c_void_p]),
    'bn_conv2d_pool2_act_fwd': (_c_int, [_c_void_p] * 5 + _CONV_GEOM + [_c_int, _c_float, _c_void_p]),
    'bn_conv2d_pool2_act_ok': (_c_int, _CONV_GEOM),
    'bn_conv2d_pool2_bwd_weight_ws_bytes': (_c_size_t, _CONV_GEOM),
    'bn_conv2d_pool2_bwd_weight': (
        _c_int, [_c_void_p] * 6 + _CONV_GEOM + [_c_int, _c_float, _c_int, _c_void_p, _c_size_t, _c_void_p]),
    'bn_maxpool2d_act_bwd': (_c_int, [_c_void_p] * 4 + [_c_int] * 4 + [ctypes.c_float, _c_void_p]),
    'bn_maxunpool2d_fwd': (_c_int, [_c_void_p] * 3 + [_c_int] * 3 + [_c_void_p]),
    'bn_maxunpool2d_fwd_k2': (_c_int, [_c_void_p] * 3 + [_c_int] * 3 + [_c_void_p]),
    'bn_maxunpool2d_bwd': (_c_int, [_c_void_p] * 3 + [_c_int] * 3 + [_c_void_p]),
    'bn_act_fwd': (_c_int, [_c_void_p] * 2 + [_c_size_t, _c_int, _c_float, _c_void_p]),
    'bn_act_bwd': (_c_int, [_c_void_p] * 3 + [_c_size_t, _c_int, _c_float, _c_void_p]),
    'bn_linear_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_linear_fwd': (_c_int, [_c_void_p] * 4 + [_c_int] * 3 + [_c_void_p, _c_size_t, _c_void_p]),
    'bn_linear_bwd': (
        _c_int, [_c_void_p] * 5 + [_c_int, _c_float, _c_void_p, _c_void_p, _c_int] +
        [_c_int] * 3 + [_c_void_p, _c_size_t, _c_void_p]),
    'bn_sqerr_frame_sums': (_c_int, [_c_void_p] * 4 + [_c_int, _c_size_t, _c_void_p]),
    'bn_sqerr_bwd': (_c_int, [_c_void_p] * 4 + [_c_size_t, _c_float, _c_void_p, _c_void_p]),
    'bn_convT2d_fwd_sqerr_parts': (_c_int, _CONV_GEOM),
    'bn_convT2d_fwd_sqerr_ws_bytes': (_c_size_t, _CONV_GEOM + [_c_int]),
    'bn_convT2d_fwd_sqerr': (
        _c_int, [_c_void_p] * 8 + _CONV_GEOM + [_c_int, _c_float, _c_void_p, _c_size_t, _c_void_p]),
    'bn_scale_frames': (_c_int, [_c_void_p] * 4 + [_c_int, _c_size_t, _c_void_p]),
    'bn_reduce_sum': (_c_int, [_c_void_p] * 2 + [_c_size_t, _c_float, _c_void_p]),
    'bn_reparam_fwd': (_c_int, [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_kl_rows': (_c_int, [_c_void_p] * 3 + [_c_int, _c_int, _c_void_p]),
    'bn_reparam_bwd': (_c_int, [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_kl_bwd': (_c_int, [_c_void_p] * 4 + [_c_size_t, _c_float, _c_void_p, _c_void_p]),
    'bn_decomposed_kl_fwd': (_c_int, [_c_void_p] * 7 + [_c_int, _c_int, _c_void_p]),
    'bn_decomposed_kl_bwd': (_c_int, [_c_void_p] * 9 + [_c_int, _c_int, _c_void_p]),
    'bn_psvae_head_fwd': (_c_int, [_c_void_p] * 14 + [_c_int] * 3 + [_c_void_p]),
    'bn_psvae_head_combine': (
        _c_int, [_c_void_p] * 4 + [_c_int] + [_c_float] * 3 + [_c_int] + [_c_void_p] * 3),
    'bn_psvae_head_bwd': (
        _c_int, [_c_void_p] * 3 + [_c_int] + [_c_void_p] * 10 + [_c_float] + [_c_void_p] * 5 +
        [_c_int] * 4 + [_c_void_p]),
    'bn_adam_amsgrad_step': (
        _c_int, [_c_void_p] * 5 + [_c_size_t] + [_c_float] * 5 + [_c_int, _c_void_p]),
    'bn_conv2d_first_bf16_ok': (_c_int, _CONV_GEOM),
    'bn_conv2d_bf16_ok': (_c_int, _CONV_GEOM),
    'bn_conv_pack_w_bf16_bytes': (_c_size_t, [_c_int] * 4),
    'bn_conv_pack_w_bf16': (_c_int, [_c_void_p] * 2 + [_c_int] * 4 + [_c_void_p]),
    'bn_conv2d_first_bf16': (
        _c_int, [_c_void_p, _c_int] + [_c_void_p] * 3 + _CONV_GEOM + [_c_int, _c_float, _c_void_p]),
    'bn_conv2d_fwd_bf16': (
        _c_int, [_c_void_p] * 4 + [_c_int] + _CONV_GEOM + [_c_int, _c_float, _c_void_p]),
    'bn_convT2d_bf16_ok': (_c_int, _CONV_GEOM),
    'bn_convT2d_last_bf16_ok': (_c_int, _CONV_GEOM),
    'bn_convT_pack_w_bf16_bytes': (_c_size_t, [_c_int] * 4),
    'bn_convT_pack_w_bf16': (_c_int, [_c_void_p] * 2 + [_c_int] * 4 + [_c_void_p]),
    'bn_to_nhwc_bf16': (_c_int, [_c_void_p] * 2 + [_c_int] * 4 + [_c_void_p]),
    'bn_convT2d_fwd_bf16': (
        _c_int, [_c_void_p] * 4 + [_c_int] + _CONV_GEOM + [_c_int, _c_float, _c_void_p]),
    'bn_convT2d_last_bf16': (
        _c_int, [_c_void_p] * 4 + _CONV_GEOM + [_c_int, _c_float, _c_void_p]),
    'bn_convT2d_last_bf16_sqerr_ws_bytes': (_c_size_t, _CONV_GEOM),
    'bn_convT2d_last_bf16_sqerr': (
        _c_int, [_c_void_p] * 4 + [_c_int] + [_c_void_p] * 2 + _CONV_GEOM +
        [_c_int, _c_float, _c_float, _c_void_p, _c_size_t, _c_void_p]),
    'bn_convT2d_last_bf16_u8': (
        _c_int, [_c_void_p] * 4 + _CONV_GEOM + [_c_int, _c_float, _c_void_p]),
    'bn_frame_sq_err_ws_bytes': (_c_size_t, [_c_int, _c_size_t]),
    'bn_frame_sq_err': (
        _c_int, [_c_void_p] * 2 + [_c_int] + [_c_void_p] * 2 + [_c_int, _c_size_t, _c_float, _c_void_p, _c_size_t,
                                                                 _c_void_p]),
    'bn_pixel_stats_ws_bytes': (_c_size_t, [_c_int, _c_size_t]),
    'bn_pixel_stats_accum': (
        _c_int, [_c_void_p] * 2 + [_c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_size_t, _c_void_p, _c_size_t,
                                   _c_void_p]),
    'bn_u8_to_unit_float': (_c_int, [_c_void_p] * 2 + [_c_size_t, _c_void_p]),
    'bn_unit_float_to_u8': (_c_int, [_c_void_p] * 2 + [_c_size_t, _c_void_p]),
    'bn_cond_encoder_input': (_c_int, [_c_void_p, _c_int, _c_void_p] + [_c_int] * 6 + [_c_void_p, _c_void_p]),
    'bn_frame_mosaic_u8': (_c_int, [_c_void_p] + [_c_int] * 10 + [_c_void_p] + [_c_int] * 3 + [_c_void_p, _c_void_p]),
    'bn_frame_mosaic_ch_u8': (_c_int, [_c_void_p] + [_c_int] * 11 + [_c_void_p] + [_c_int] * 3
                              + [_c_void_p, _c_void_p]),
    'bn_stamp_boxes_u8': (_c_int, [_c_void_p] + [_c_int] * 5 + [_c_void_p] + [_c_int] * 5 + [_c_void_p]),
    'bn_recon_panels_u8': (_c_int, [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p] + [_c_int] * 6
                           + [_c_void_p, _c_size_t, _c_void_p]),
    'bn_column_select_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_column_count': (_c_int, [_c_void_p] + [_c_int] * 3 + [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    'bn_column_select': (_c_int, [_c_void_p] + [_c_int] * 3 + [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_size_t,
                                                                _c_void_p]),
    'bn_segment_label_sums_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_segment_label_sums': (_c_int, [_c_void_p, _c_int] * 3 + [_c_void_p] + [_c_int] * 3
                              + [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    'bn_segment_gram_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_segment_gram': (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p] + [_c_int] * 3
                        + [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    'bn_softmax_cv_lossgrad_ws_bytes': (_c_size_t, [_c_int] * 4),
    'bn_softmax_cv_lossgrad': (_c_int, [_c_void_p, _c_int] + [_c_void_p] * 4 + [_c_int] * 4
                               + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_softmax_cv_score_ws_bytes': (_c_size_t, [_c_int] * 4),
    'bn_softmax_cv_score': (_c_int, [_c_void_p, _c_int] + [_c_void_p] * 4 + [_c_int] * 4
                            + [_c_void_p] * 2 + [_c_size_t, _c_void_p]),
    'bn_arhmm_loglik_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_arhmm_loglik': (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p] + [_c_int] * 5
                        + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_hmm_forward_backward_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_hmm_forward_backward': (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 3 + [_c_void_p, _c_void_p, _c_int]
                                + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_arhmm_moments_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_arhmm_moments': (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p] + [_c_int] * 5
                         + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_hmm_viterbi_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_hmm_viterbi': (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 3 + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_arhmm_grid_loglik_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_arhmm_grid_loglik': (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p] + [_c_int] * 5
                             + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_arhmm_grid_moments_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_arhmm_grid_moments': (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p] + [_c_int] * 5
                              + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_hmm_grid_forward_backward_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_hmm_grid_forward_backward': (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 5 + [_c_void_p] * 3 + [_c_int] * 4
                                     + [_c_void_p, _c_void_p, _c_int] + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_hmm_grid_viterbi_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_hmm_grid_viterbi': (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 5 + [_c_void_p] * 3 + [_c_int] * 4
                            + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_arhmm_sample_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_arhmm_sample': (_c_int, [_c_void_p] * 5 + [_c_int] * 5 + [_c_void_p] * 4 + [_c_int] + [_c_void_p] * 3
                        + [_c_size_t, _c_void_p]),
    'bn_hmm_predictive_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_hmm_predictive': (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 3 + [_c_void_p] * 4 + [_c_size_t, _c_void_p]),
    'bn_arhmm_predict_ws_bytes': (_c_size_t, [_c_int] * 5),
    'bn_arhmm_predict': (_c_int, [_c_void_p, _c_int, _c_void_p] + [_c_int] * 5 + [_c_void_p] * 4
                         + [_c_size_t, _c_void_p]),
    'bn_arhmm_forecast_sums_ws_bytes': (_c_size_t, [_c_int] * 6),
    'bn_arhmm_forecast_sums': (_c_int, [_c_void_p, _c_int, _c_void_p] + [_c_int] * 6 + [_c_void_p] * 4
                               + [_c_size_t, _c_void_p]),
    'bn_state_runs_ws_bytes': (_c_size_t, [_c_int] * 3),
    'bn_state_runs': (_c_int, [_c_void_p, _c_void_p] + [_c_int] * 3 + [_c_void_p, ctypes.c_longlong] + [_c_void_p] * 5
                      + [_c_size_t, _c_void_p]),
    'bn_prof_select': (_c_int, [_c_int] * 3),
    'bn_prof_select_nth': (_c_int, [_c_int] * 4),
    'bn_prof_read': (_c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]),
    'bn_prof_read_main': (_c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]),
    'bn_prof_set_bracket': (_c_int, [_c_int]),
    'bn_prof_kernel_name': (ctypes.c_char_p, []),
    'bn_prof_dispatch_overhead_us': (ctypes.c_double, [_c_int, _c_void_p]),
}


class HipLibraryError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def load(required=True):
    """Load the shared library (once).  Raises if it is missing and ``required``."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        if required:
            raise HipLibraryError(
                '%s not found next to the package (%s). Build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` or '
                '`make -C behavenet_amd/csrc`. There is no CPU fallback.' % (_LIB_NAME, _LIB_PATH))
        return None
    lib = ctypes.CDLL(_LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = load().bn_error_string(int(rc))
        raise HipLibraryError('%s failed: %s (code %d)' % (what, msg.decode() if msg else '?', rc))


def _ptr(t, name, dtype=torch.float32, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise HipLibraryError('%s: tensor is None' % name)
    if not t.is_cuda:
        raise HipLibraryError(
            '%s: expected a tensor on the GPU, got device %s (the HIP path has no CPU fallback)'
            % (name, t.device))
    if t.dtype != dtype:
        raise HipLibraryError('%s: expected dtype %s, got %s' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise HipLibraryError('%s: tensor must be contiguous' % name)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------
# convolution roles.  geom = (N, C, H, W, K, R, S, stride, pad_t, pad_l, P, Q) for conv and
# (N, Ci, Hi, Wi, Co, R, S, stride, crop_t, crop_l, Ho, Wo) for convT -- the header's order.
# ------------------------------------------------------------------------------------------
_ws_cache = {}


def _arena(device, nbytes, tag=None):
    """Pointer to at least ``nbytes`` of scratch on ``device``: a grow-only arena per (device,
    stream, tag) -- kernels on different streams may run concurrently -- or, while a HIP graph is
    being recorded, a block of the GRAPH's memory pool for this call only (freed right away: the
    pool re-issues it within the recording in stream order and keeps it reserved for the replays).
    A recording's block must never enter the cache: an arena cached from one graph's pool outlives
    the pool, and the next recording (another pool) would be handed memory that went back to the
    driver with the first graph (round 5: "write access to a read-only page" in the third recording
    of a process)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device).data_ptr()
    key = (device, torch.cuda.current_stream(device).cuda_stream) + ((tag,) if tag else ())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        with torch.cuda.stream(torch.cuda.current_stream(device)):
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf.data_ptr()


def _workspace(op, geom, device):
    """(pointer, nbytes) of the grow-only scratch arena of `device` sized for this call."""
    if torch.device(device).type != 'cuda':
        raise HipLibraryError(
            'expected tensors on the GPU, got device %s (the HIP path has no CPU fallback)' % device)
    nbytes = load().bn_conv_ws_bytes(op, *geom)
    if nbytes == 0:
        return None, 0
    return _arena(device, nbytes), nbytes


_taps_bytes = {}
_generic_epoch = 0      # set_force_generic() changes what the dispatch pads


def conv_taps_bytes(op, geom):
    """Bytes of the 5x5 copy of a small-kernel layer's taps if `op` pads them, else 0 (bn_conv_taps_bytes)."""
    key = (_generic_epoch, op) + tuple(geom)
    v = _taps_bytes.get(key)
    if v is None:
        v = _taps_bytes[key] = int(load().bn_conv_taps_bytes(op, *geom))
    return v


def conv_taps_pad(jobs, device):
    """jobs = [(op, geom, w)] -> [w5]: the 5x5 copies of the layers' taps, all in ONE launch (bn_conv_taps_pad).
    The copies are slices of one fresh buffer; pass them to the forward / data-gradient wrappers as ``w5=``."""
    n = len(jobs)
    if n == 0:
        return []
    sizes = [(conv_taps_bytes(op, geom) // 4 + 63) // 64 * 64 for op, geom, _ in jobs]
    if min(sizes) == 0:
        raise HipLibraryError('conv_taps_pad: a layer whose op does not pad its taps')
    buf = torch.empty(sum(sizes), dtype=torch.float32, device=device)
    out, o = [], 0
    for sz in sizes:
        out.append(buf[o:o + sz])
        o += sz
    wp = (ctypes.c_void_p * n)(*[_ptr(w, 'w') for _, _, w in jobs])
    w5p = (ctypes.c_void_p * n)(*[t.data_ptr() for t in out])
    flat = []
    for op, geom, _ in jobs:
        flat.append(op)
        flat.extend(int(v) for v in geom)
    geoms = (ctypes.c_int * (13 * n))(*flat)
    _check(load().bn_conv_taps_pad(n, wp, w5p, geoms, _stream()), 'bn_conv_taps_pad')
    return out


def conv2d_fwd(x, w, b, geom, act, slope, w5=None):
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    y = torch.empty((N, K, P, Q), dtype=torch.float32, device=x.device)
    ws, nb = _workspace(OP_CONV_FWD, geom, x.device)
    _check(load().bn_conv2d_fwd(
        _ptr(x, 'x'), _ptr(w, 'w'), _ptr(w5, 'w5', allow_none=True), _ptr(b, 'b', allow_none=True), _ptr(y, 'y'),
        *geom, act, slope, ws, nb, _stream()), 'bn_conv2d_fwd')
    return y


def conv2d_fwd_u8(x_u8, w, b, geom, act, slope):
    """First encoder layer from uint8 frames (value / 255 fused into the patch load)."""
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    y = torch.empty((N, K, P, Q), dtype=torch.float32, device=x_u8.device)
    lib = load()
    nbytes = lib.bn_conv2d_fwd_u8_ws_bytes(*geom, act)
    ws = None
    if nbytes:
        ws = _arena(x_u8.device, nbytes, 'fwd_u8')
    _check(lib.bn_conv2d_fwd_u8(
        _ptr(x_u8, 'x', dtype=torch.uint8), _ptr(w, 'w'), _ptr(b, 'b', allow_none=True),
        _ptr(y, 'y'), *geom, act, slope, ws, nbytes, _stream()), 'bn_conv2d_fwd_u8')
    return y


def conv2d_bwd_data(dy, w, geom, dact_src, dact, slope, w5=None):
    N, C, H, W = geom[:4]
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    ws, nb = _workspace(OP_CONV_BWD_D, geom, dy.device)
    _check(load().bn_conv2d_bwd_data(
        _ptr(dy, 'dy'), _ptr(w, 'w'), _ptr(w5, 'w5', allow_none=True), _ptr(dx, 'dx'),
        _ptr(dact_src, 'dact_src', allow_none=True), *geom, dact, slope, ws, nb, _stream()), 'bn_conv2d_bwd_data')
    return dx


def conv2d_bwd_weight(x, dy, dw, db, geom, accumulate):
    ws, nb = _workspace(OP_CONV_BWD_W, geom, x.device)
    _check(load().bn_conv2d_bwd_weight(
        _ptr(x, 'x'), _ptr(dy, 'dy'), _ptr(dw, 'dw'), _ptr(db, 'db', allow_none=True), *geom,
        int(accumulate), ws, nb, _stream()), 'bn_conv2d_bwd_weight')


def convT2d_fwd(x, w, b, geom, act, slope, w5=None):
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    y = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device)
    ws, nb = _workspace(OP_CONVT_FWD, geom, x.device)
    _check(load().bn_convT2d_fwd(
        _ptr(x, 'x'), _ptr(w, 'w'), _ptr(w5, 'w5', allow_none=True), _ptr(b, 'b', allow_none=True), _ptr(y, 'y'),
        *geom, act, slope, ws, nb, _stream()), 'bn_convT2d_fwd')
    return y


def convT2d_bwd_data(dy, w, geom, dact_src, dact, slope, w5=None):
    N, Ci, Hi, Wi = geom[:4]
    dx = torch.empty((N, Ci, Hi, Wi), dtype=torch.float32, device=dy.device)
    ws, nb = _workspace(OP_CONVT_BWD_D, geom, dy.device)
    _check(load().bn_convT2d_bwd_data(
        _ptr(dy, 'dy'), _ptr(w, 'w'), _ptr(w5, 'w5', allow_none=True), _ptr(dx, 'dx'),
        _ptr(dact_src, 'dact_src', allow_none=True), *geom, dact, slope, ws, nb, _stream()), 'bn_convT2d_bwd_data')
    return dx


def convT2d_bwd_weight(x, dy, dw, db, geom, accumulate):
    ws, nb = _workspace(OP_CONVT_BWD_W, geom, x.device)
    _check(lib_call('bn_convT2d_bwd_weight')(
        _ptr(x, 'x'), _ptr(dy, 'dy'), _ptr(dw, 'dw'), _ptr(db, 'db', allow_none=True), *geom,
        int(accumulate), ws, nb, _stream()), 'bn_convT2d_bwd_weight')


# ------------------------------------------------------------------------------------------
# inference-only bf16 encoder stack (csrc/conv_bf16.hip).  Activations between its layers are
# torch.bfloat16 tensors of shape (N, P, Q, K): the library's private channels-last layout.
# ------------------------------------------------------------------------------------------
def conv2d_bf16_ok(geom, first=False):
    """Host-only: does the bf16 path serve this layer (as the first layer / as a body layer)?"""
    lib = load()
    return bool((lib.bn_conv2d_first_bf16_ok if first else lib.bn_conv2d_bf16_ok)(*[int(v) for v in geom]))


def conv_pack_w_bf16_bytes(w_shape):
    K, C, R, S = [int(v) for v in w_shape]
    return int(load().bn_conv_pack_w_bf16_bytes(K, C, R, S))


def conv_pack_w_bf16(w, out):
    """fp32 (K, C, R, S) weights -> bf16 operand layout in ``out`` (a uint8 device buffer of
    ``conv_pack_w_bf16_bytes`` bytes, 16-byte aligned)."""
    K, C, R, S = w.shape
    if out.numel() * out.element_size() < conv_pack_w_bf16_bytes(w.shape):
        raise HipLibraryError('conv_pack_w_bf16: output buffer too small')
    _check(load().bn_conv_pack_w_bf16(_ptr(w, 'w'), out.data_ptr(), K, C, R, S, _stream()),
           'bn_conv_pack_w_bf16')
    return out


def _bf16_out(out, shape, dtype, device, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype:
        raise HipLibraryError('%s: out must be %s of shape %s' % (what, dtype, tuple(shape)))
    return out


def conv2d_first_bf16(x, w, b, geom, act, slope, out=None):
    """Layer 1 from fp32 or uint8 NCHW frames -> bf16 (N, P, Q, K)."""
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    u8 = x.dtype == torch.uint8
    y = _bf16_out(out, (N, P, Q, K), torch.bfloat16, x.device, 'conv2d_first_bf16')
    _check(load().bn_conv2d_first_bf16(
        _ptr(x, 'x', dtype=torch.uint8 if u8 else torch.float32), int(u8), _ptr(w, 'w'),
        _ptr(b, 'b', allow_none=True), _ptr(y, 'y', dtype=torch.bfloat16), *geom, act, slope, _stream()),
        'bn_conv2d_first_bf16')
    return y


def conv2d_fwd_bf16(x, wp, b, geom, act, slope, out_f32, out=None):
    """Body layer: x bf16 (N, H, W, C), wp packed weights -> bf16 (N, P, Q, K), or fp32 (N, K, P, Q)."""
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    if tuple(x.shape) != (N, H, W, C):
        raise HipLibraryError('conv2d_fwd_bf16: expected activations (N,H,W,C)=%s, got %s'
                              % ((N, H, W, C), tuple(x.shape)))
    if out_f32:
        y = _bf16_out(out, (N, K, P, Q), torch.float32, x.device, 'conv2d_fwd_bf16')
    else:
        y = _bf16_out(out, (N, P, Q, K), torch.bfloat16, x.device, 'conv2d_fwd_bf16')
    _check(load().bn_conv2d_fwd_bf16(
        _ptr(x, 'x', dtype=torch.bfloat16), wp.data_ptr(), _ptr(b, 'b', allow_none=True),
        _ptr(y, 'y', dtype=y.dtype),
        int(bool(out_f32)), *geom, act, slope, _stream()), 'bn_conv2d_fwd_bf16')
    return y


# ------------------------------------------------------------------------------------------
# inference-only bf16 decoder stack (csrc/conv_bf16_dec.hip): the same private layout, bf16
# (N, H, W, C), between its layers; geometry tuples as convT2d_fwd.
# ------------------------------------------------------------------------------------------
def convT2d_bf16_ok(geom, last=False):
    """Host-only: does the bf16 path serve this transposed convolution (as a body layer / as the layer
    onto the frame)?"""
    lib = load()
    return bool((lib.bn_convT2d_last_bf16_ok if last else lib.bn_convT2d_bf16_ok)(*[int(v) for v in geom]))


def convT_pack_w_bf16_bytes(w_shape):
    Ci, Co, R, S = [int(v) for v in w_shape]
    return int(load().bn_convT_pack_w_bf16_bytes(Ci, Co, R, S))


def convT_pack_w_bf16(w, out):
    """fp32 nn.ConvTranspose2d weights (Ci, Co, R, S) -> bf16 operand layout in ``out`` (a uint8 device
    buffer of ``convT_pack_w_bf16_bytes`` bytes, 16-byte aligned)."""
    if w.dim() != 4:
        raise HipLibraryError('convT_pack_w_bf16: expected weights (Ci, Co, R, S), got %s' % (tuple(w.shape),))
    Ci, Co, R, S = w.shape
    if out.numel() * out.element_size() < convT_pack_w_bf16_bytes(w.shape):
        raise HipLibraryError('convT_pack_w_bf16: output buffer too small')
    _check(load().bn_convT_pack_w_bf16(_ptr(w, 'w'), out.data_ptr(), Ci, Co, R, S, _stream()),
           'bn_convT_pack_w_bf16')
    return out


def to_nhwc_bf16(x, out=None):
    """fp32 (N, C, H, W) -> bf16 (N, H, W, C), one rounding to nearest even."""
    if x.dim() != 4:
        raise HipLibraryError('to_nhwc_bf16: expected (N, C, H, W), got %s' % (tuple(x.shape),))
    N, C, H, W = x.shape
    y = _bf16_out(out, (N, H, W, C), torch.bfloat16, x.device, 'to_nhwc_bf16')
    _check(load().bn_to_nhwc_bf16(_ptr(x, 'x'), _ptr(y, 'y', dtype=torch.bfloat16), N, C, H, W, _stream()),
           'bn_to_nhwc_bf16')
    return y


def convT2d_fwd_bf16(x, wp, b, geom, act, slope, out_f32, out=None):
    """Body layer: x bf16 (N, Hi, Wi, Ci), wp packed weights -> bf16 (N, Ho, Wo, Co), or fp32 (N, Co, Ho, Wo)."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    if tuple(x.shape) != (N, Hi, Wi, Ci):
        raise HipLibraryError('convT2d_fwd_bf16: expected activations (N,Hi,Wi,Ci)=%s, got %s'
                              % ((N, Hi, Wi, Ci), tuple(x.shape)))
    if out_f32:
        y = _bf16_out(out, (N, Co, Ho, Wo), torch.float32, x.device, 'convT2d_fwd_bf16')
    else:
        y = _bf16_out(out, (N, Ho, Wo, Co), torch.bfloat16, x.device, 'convT2d_fwd_bf16')
    _check(load().bn_convT2d_fwd_bf16(
        _ptr(x, 'x', dtype=torch.bfloat16), wp.data_ptr(), _ptr(b, 'b', allow_none=True),
        _ptr(y, 'y', dtype=y.dtype),
        int(bool(out_f32)), *geom, act, slope, _stream()), 'bn_convT2d_fwd_bf16')
    return y


def convT2d_last_bf16(x, w, b, geom, act, slope, out=None):
    """The layer onto the frame: x bf16 (N, Hi, Wi, Ci), w fp32 (Ci, Co, R, S) as stored -> fp32 (N, Co, Ho, Wo)."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    if tuple(x.shape) != (N, Hi, Wi, Ci):
        raise HipLibraryError('convT2d_last_bf16: expected activations (N,Hi,Wi,Ci)=%s, got %s'
                              % ((N, Hi, Wi, Ci), tuple(x.shape)))
    if tuple(w.shape) != (Ci, Co, R, S):
        raise HipLibraryError('convT2d_last_bf16: expected weights (Ci,Co,R,S)=%s, got %s'
                              % ((Ci, Co, R, S), tuple(w.shape)))
    y = _bf16_out(out, (N, Co, Ho, Wo), torch.float32, x.device, 'convT2d_last_bf16')
    _check(load().bn_convT2d_last_bf16(
        _ptr(x, 'x', dtype=torch.bfloat16), _ptr(w, 'w'), _ptr(b, 'b', allow_none=True), _ptr(y, 'y'),
        *geom, act, slope, _stream()), 'bn_convT2d_last_bf16')
    return y


def _err_operands(what, target, mask, out, n, device):
    """(target pointer, is_u8, mask pointer, out): the target / mask / out checks the two frame-error calls share."""
    if target.dtype not in (torch.float32, torch.uint8) or not target.is_contiguous():
        raise HipLibraryError('%s: the target must be a contiguous float32 or uint8 tensor' % what)
    if mask is not None and tuple(mask.shape) != tuple(target.shape):
        raise HipLibraryError('%s: the mask must have the target\'s shape %s, got %s'
                              % (what, tuple(target.shape), tuple(mask.shape)))
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=device)
    elif tuple(out.shape) != (n,) or out.dtype != torch.float32 or not out.is_contiguous():
        raise HipLibraryError('%s: out must be a contiguous float32 tensor of shape (%d,)' % (what, n))
    return (_ptr(target, 'target', dtype=target.dtype), int(target.dtype == torch.uint8),
            _ptr(mask, 'mask', allow_none=True), out)


def frame_sq_err(xhat, target, mask=None, scale=1.0, out=None):
    """out[n] = scale * sum over the frame of (xhat[n] - target[n])^2 * mask[n] -> fp32 (N,).  xhat fp32 (N, ...);
    target fp32 or uint8 (value / 255) of xhat's shape; mask fp32 of that shape or None.  A frame's bits do not
    depend on N or on its position (csrc/frame_err.hip)."""
    if xhat.dim() < 2 or tuple(target.shape) != tuple(xhat.shape):
        raise HipLibraryError('frame_sq_err: xhat %s and target %s must share a shape (N, ...)'
                              % (tuple(xhat.shape), tuple(target.shape)))
    n = int(xhat.shape[0])
    d = xhat[0].numel()
    tp, is_u8, mp, out = _err_operands('frame_sq_err', target, mask, out, n, xhat.device)
    lib = load()
    nbytes = lib.bn_frame_sq_err_ws_bytes(n, d)
    ws = _arena(xhat.device, nbytes) if nbytes else None
    _check(lib.bn_frame_sq_err(_ptr(xhat, 'xhat'), tp, is_u8, mp, _ptr(out, 'out'), n, d, float(scale), ws, nbytes,
                               _stream()), 'bn_frame_sq_err')
    return out


def pixel_stats_accum(xhat, target, mask, acc):
    """acc (4, ...) float64 += per-pixel sums over the N frames of target (N, ...): plane 0 the squared error
    (xhat - target)^2 * mask (left alone when ``xhat`` is None), plane 1 the mask weight, planes 2 and 3 the
    mask-weighted first and second moment of the target.  xhat fp32 of target's shape or None; target fp32 or uint8
    (value / 255); mask fp32 of target's shape, of ONE frame's shape (one mask for all frames) or None.  Sums in
    float64 in a fixed order (csrc/pixel_stats.hip).  -> acc."""
    if target.dim() < 2:
        raise HipLibraryError('pixel_stats_accum: expected a target (N, ...), got %s' % (tuple(target.shape),))
    if target.dtype not in (torch.float32, torch.uint8) or not target.is_contiguous():
        raise HipLibraryError('pixel_stats_accum: the target must be a contiguous float32 or uint8 tensor')
    if xhat is not None and tuple(xhat.shape) != tuple(target.shape):
        raise HipLibraryError('pixel_stats_accum: xhat %s and target %s must share a shape (N, ...)'
                              % (tuple(xhat.shape), tuple(target.shape)))
    n, frame = int(target.shape[0]), tuple(target.shape[1:])
    d = target[0].numel() if n else 0
    mask_frames = 0
    if mask is not None:
        if tuple(mask.shape) == tuple(target.shape):
            mask_frames = n
        elif tuple(mask.shape) in (frame, (1,) + frame):
            mask_frames = 1
        else:
            raise HipLibraryError('pixel_stats_accum: the mask must have the target\'s shape %s or one frame\'s, got %s'
                                  % (tuple(target.shape), tuple(mask.shape)))
    if tuple(acc.shape) != (4,) + frame:
        raise HipLibraryError('pixel_stats_accum: acc must have the shape %s, got %s'
                              % ((4,) + frame, tuple(acc.shape)))
    lib = load()
    nbytes = lib.bn_pixel_stats_ws_bytes(n, d)
    ws = _arena(target.device, nbytes) if nbytes else None
    _check(lib.bn_pixel_stats_accum(
        _ptr(xhat, 'xhat', allow_none=True), _ptr(target, 'target', dtype=target.dtype),
        int(target.dtype == torch.uint8), _ptr(mask, 'mask', allow_none=True), mask_frames,
        _ptr(acc, 'acc', dtype=torch.float64), n, d, ws, nbytes, _stream()), 'bn_pixel_stats_accum')
    return acc


def convT2d_last_bf16_sqerr(x, w, b, target, mask, geom, act, slope, scale=1.0, out=None):
    """The layer onto the frame (``convT2d_last_bf16``) scored instead of stored: out[n] = scale * sum over the
    frame of (x_hat[n] - target[n])^2 * mask[n] -> fp32 (N,); x_hat is never written."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    if tuple(x.shape) != (N, Hi, Wi, Ci):
        raise HipLibraryError('convT2d_last_bf16_sqerr: expected activations (N,Hi,Wi,Ci)=%s, got %s'
                              % ((N, Hi, Wi, Ci), tuple(x.shape)))
    if tuple(w.shape) != (Ci, Co, R, S):
        raise HipLibraryError('convT2d_last_bf16_sqerr: expected weights (Ci,Co,R,S)=%s, got %s'
                              % ((Ci, Co, R, S), tuple(w.shape)))
    if tuple(target.shape) != (N, Co, Ho, Wo):
        raise HipLibraryError('convT2d_last_bf16_sqerr: expected a target (N,Co,Ho,Wo)=%s, got %s'
                              % ((N, Co, Ho, Wo), tuple(target.shape)))
    tp, is_u8, mp, out = _err_operands('convT2d_last_bf16_sqerr', target, mask, out, N, x.device)
    lib = load()
    nbytes = lib.bn_convT2d_last_bf16_sqerr_ws_bytes(*geom)
    ws = _arena(x.device, nbytes) if nbytes else None
    _check(lib.bn_convT2d_last_bf16_sqerr(
        _ptr(x, 'x', dtype=torch.bfloat16), _ptr(w, 'w'), _ptr(b, 'b', allow_none=True), tp, is_u8, mp,
        _ptr(out, 'out'), *geom, act, slope, float(scale), ws, nbytes, _stream()), 'bn_convT2d_last_bf16_sqerr')
    return out


def convT2d_last_bf16_u8(x, w, b, geom, act, slope, out=None):
    """The layer onto the frame (``convT2d_last_bf16``) written as stored grey levels: uint8 (N, Co, Ho, Wo), the
    bytes of ``unit_float_to_u8`` of that layer's output; the fp32 x_hat is never written."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    if tuple(x.shape) != (N, Hi, Wi, Ci):
        raise HipLibraryError('convT2d_last_bf16_u8: expected activations (N,Hi,Wi,Ci)=%s, got %s'
                              % ((N, Hi, Wi, Ci), tuple(x.shape)))
    if tuple(w.shape) != (Ci, Co, R, S):
        raise HipLibraryError('convT2d_last_bf16_u8: expected weights (Ci,Co,R,S)=%s, got %s'
                              % ((Ci, Co, R, S), tuple(w.shape)))
    y = _bf16_out(out, (N, Co, Ho, Wo), torch.uint8, x.device, 'convT2d_last_bf16_u8')
    _check(load().bn_convT2d_last_bf16_u8(
        _ptr(x, 'x', dtype=torch.bfloat16), _ptr(w, 'w'), _ptr(b, 'b', allow_none=True),
        _ptr(y, 'y', dtype=torch.uint8), *geom, act, slope, _stream()), 'bn_convT2d_last_bf16_u8')
    return y


def set_force_generic(on):
    """Route convolutions through the shape-agnostic kernels (test hook); returns previous."""
    global _generic_epoch
    _generic_epoch += 1
    return bool(load().bn_set_force_generic(1 if on else 0))


def set_bigk1_block_bytes(nbytes):
    """Frame-block size of the shifted-copies path of stride-1 7x7 / 9x9 layers (test hook); returns previous."""
    return int(load().bn_set_bigk1_block_bytes(int(nbytes)))


def lib_call(name):
    return getattr(load(), name)


def _bn_ws(n, c, device):
    nbytes = load().bn_batchnorm_ws_bytes(n, c)
    return _arena(device, nbytes, 'bn'), nbytes


def batchnorm_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, act, slope, y=None):
    """-> (y, mean, invstd); updates the running statistics in place (train mode).  ``y``: where to
    write the result (a contiguous slice of a larger batch)."""
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    mean = torch.empty((c,), dtype=torch.float32, device=x.device)
    var = torch.empty_like(mean)
    invstd = torch.empty_like(mean)
    ws, nb = _bn_ws(n, c, x.device)
    _check(load().bn_batchnorm_stats(_ptr(x, 'x'), _ptr(mean, 'mean'), _ptr(var, 'var'), n, c, hw,
                                     ws, nb, _stream()), 'bn_batchnorm_stats')
    cnt = n * hw
    unbias = cnt / (cnt - 1.0) if cnt > 1 else 1.0
    _check(load().bn_batchnorm_finalize(
        _ptr(mean, 'mean'), _ptr(var, 'var'), _ptr(invstd, 'invstd'),
        _ptr(running_mean, 'running_mean', allow_none=True),
        _ptr(running_var, 'running_var', allow_none=True), c, eps, momentum, unbias, _stream()),
        'bn_batchnorm_finalize')
    if y is None:
        y = torch.empty_like(x)
    _check(load().bn_batchnorm_act_fwd(
        _ptr(x, 'x'), _ptr(mean, 'mean'), _ptr(invstd, 'invstd'),
        _ptr(gamma, 'gamma', allow_none=True), _ptr(beta, 'beta', allow_none=True), _ptr(y, 'y'),
        n, c, hw, act, slope, _stream()), 'bn_batchnorm_act_fwd')
    return y, mean, invstd


def batchnorm_train_fwd_chunks(x, gamma, beta, running_mean, running_var, factors, eps, act, slope,
                               bounds, num_batches_tracked=None):
    """Train-mode batch norm with statistics per chunk of frames (``bounds``: [(beg, end)] in order,
    ``factors``: the running-estimate factor of every chunk's update).  One library call.
    ``num_batches_tracked``: nn.BatchNorm2d's int64 counter, advanced by len(bounds) on the device.
    -> (y, mean (n_chunks, C), invstd (n_chunks, C))."""
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or
                                            not num_batches_tracked.is_cuda):
        raise TypeError('num_batches_tracked must be an int64 device tensor')
    import ctypes
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    k = len(bounds)
    mean = torch.empty((k, c), dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    y = torch.empty_like(x)
    ws, nb = _bn_ws(max(e - b for b, e in bounds), c, x.device)
    flat = (ctypes.c_int * (2 * k))(*[v for be in bounds for v in be])
    fac = (ctypes.c_float * k)(*[float(f) for f in factors])
    _check(load().bn_batchnorm_train_fwd_chunks(
        _ptr(x, 'x'), _ptr(gamma, 'gamma', allow_none=True), _ptr(beta, 'beta', allow_none=True),
        _ptr(running_mean, 'running_mean', allow_none=True),
        _ptr(running_var, 'running_var', allow_none=True),
        num_batches_tracked.data_ptr() if num_batches_tracked is not None else None,
        _ptr(y, 'y'), _ptr(mean, 'mean'),
        _ptr(invstd, 'invstd'), ctypes.cast(flat, ctypes.c_void_p), ctypes.cast(fac, ctypes.c_void_p),
        k, c, hw, eps, act, slope, ws, nb, _stream()), 'bn_batchnorm_train_fwd_chunks')
    return y, mean, invstd


def batchnorm_bwd_chunks(x, y, dy, mean, invstd, gamma, dgamma, dbeta, accumulate, act, slope, bounds,
                         beta=None):
    """``y`` None (identity / LeakyReLU): the activation's sign is rebuilt from x through (gamma,
    ``beta``) -- the saved output is not read."""
    import ctypes
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    k = len(bounds)
    dx = torch.empty_like(x)
    ws, nb = _bn_ws(max(e - b for b, e in bounds), c, x.device)
    flat = (ctypes.c_int * (2 * k))(*[v for be in bounds for v in be])
    _check(load().bn_batchnorm_act_bwd_chunks(
        _ptr(x, 'x'), _ptr(y, 'y', allow_none=True), _ptr(dy, 'dy'), _ptr(mean, 'mean'),
        _ptr(invstd, 'invstd'), _ptr(gamma, 'gamma', allow_none=True),
        _ptr(beta, 'beta', allow_none=True), _ptr(dx, 'dx'),
        _ptr(dgamma, 'dgamma', allow_none=True), _ptr(dbeta, 'dbeta', allow_none=True),
        int(accumulate), ctypes.cast(flat, ctypes.c_void_p), k, c, hw, act, slope, ws, nb, _stream()),
        'bn_batchnorm_act_bwd_chunks')
    return dx


def batchnorm_eval_fwd(x, gamma, beta, running_mean, running_var, eps, act, slope):
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    invstd = torch.empty((c,), dtype=torch.float32, device=x.device)
    _check(load().bn_batchnorm_finalize(
        _ptr(running_mean, 'running_mean'), _ptr(running_var, 'running_var'),
        _ptr(invstd, 'invstd'), None, None, c, eps, 0.0, 1.0, _stream()), 'bn_batchnorm_finalize')
    y = torch.empty_like(x)
    _check(load().bn_batchnorm_act_fwd(
        _ptr(x, 'x'), _ptr(running_mean, 'mean'), _ptr(invstd, 'invstd'),
        _ptr(gamma, 'gamma', allow_none=True), _ptr(beta, 'beta', allow_none=True), _ptr(y, 'y'),
        n, c, hw, act, slope, _stream()), 'bn_batchnorm_act_fwd')
    return y, invstd


def batchnorm_bwd(x, y, dy, mean, invstd, gamma, dgamma, dbeta, accumulate, batch_stats, act,
                  slope, dx=None):
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    if dx is None:
        dx = torch.empty_like(x)
    ws, nb = _bn_ws(n, c, x.device)
    _check(load().bn_batchnorm_act_bwd(
        _ptr(x, 'x'), _ptr(y, 'y'), _ptr(dy, 'dy'), _ptr(mean, 'mean'), _ptr(invstd, 'invstd'),
        _ptr(gamma, 'gamma', allow_none=True), _ptr(dx, 'dx'),
        _ptr(dgamma, 'dgamma', allow_none=True), _ptr(dbeta, 'dbeta', allow_none=True),
        int(accumulate), int(batch_stats), n, c, hw, act, slope, ws, nb, _stream()),
        'bn_batchnorm_act_bwd')
    return dx


def batchnorm_sync_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, act, slope,
                             all_reduce):
    """Train-mode batch norm whose statistics are taken over the frames of ALL ranks:
    ``all_reduce(t)`` sums a small device tensor over ranks in place.  -> (y, mean, invstd,
    global count); x may hold zero frames on this rank."""
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // max(n * c, 1) if n else int(x.shape[2] * x.shape[3])
    dev = x.device
    s1 = torch.zeros((c + 1,), dtype=torch.float32, device=dev)     # channel sums + frame count
    if n:
        ws, nb = _bn_ws(n, c, dev)
        _check(load().bn_batchnorm_moment(_ptr(x, 'x'), None, _ptr(s1, 'sums'), n, c, hw, ws, nb,
                                          _stream()), 'bn_batchnorm_moment')
        s1[c] = float(n)
    all_reduce(s1)
    count = s1[c] * hw
    mean = (s1[:c] / count).contiguous()
    s2 = torch.zeros((c,), dtype=torch.float32, device=dev)
    if n:
        _check(load().bn_batchnorm_moment(_ptr(x, 'x'), _ptr(mean, 'mean'), _ptr(s2, 'sums'), n, c,
                                          hw, ws, nb, _stream()), 'bn_batchnorm_moment')
    all_reduce(s2)
    var = (s2 / count).contiguous()
    cnt = float(count.item())
    unbias = cnt / (cnt - 1.0) if cnt > 1 else 1.0
    invstd = torch.empty_like(mean)
    _check(load().bn_batchnorm_finalize(
        _ptr(mean, 'mean'), _ptr(var, 'var'), _ptr(invstd, 'invstd'),
        _ptr(running_mean, 'running_mean', allow_none=True),
        _ptr(running_var, 'running_var', allow_none=True), c, eps, momentum, unbias, _stream()),
        'bn_batchnorm_finalize')
    y = torch.empty_like(x)
    if n:
        _check(load().bn_batchnorm_act_fwd(
            _ptr(x, 'x'), _ptr(mean, 'mean'), _ptr(invstd, 'invstd'),
            _ptr(gamma, 'gamma', allow_none=True), _ptr(beta, 'beta', allow_none=True),
            _ptr(y, 'y'), n, c, hw, act, slope, _stream()), 'bn_batchnorm_act_fwd')
    return y, mean, invstd, cnt


def batchnorm_sync_bwd(x, y, dy, mean, invstd, gamma, count, act, slope, all_reduce):
    """-> (dx, this rank's sum_dz, sum_dzx): dx uses the sums of ALL ranks, the parameter
    gradients (dbeta = sum_dz, dgamma = sum_dzx) stay local -- they are summed with every other
    gradient by the all-reduce before the optimizer step."""
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // max(n * c, 1) if n else 1
    local = torch.zeros((2, c), dtype=torch.float32, device=x.device)
    if n:
        ws, nb = _bn_ws(n, c, x.device)
        _check(load().bn_batchnorm_bwd_reduce(
            _ptr(x, 'x'), _ptr(y, 'y'), _ptr(dy, 'dy'), _ptr(mean, 'mean'),
            _ptr(invstd, 'invstd'), _ptr(local[0], 'sum_dz'), _ptr(local[1], 'sum_dzx'), n, c, hw,
            act, slope, ws, nb, _stream()), 'bn_batchnorm_bwd_reduce')
    total = all_reduce(local.clone())
    dx = torch.empty_like(x)
    if n:
        _check(load().bn_batchnorm_bwd_apply(
            _ptr(x, 'x'), _ptr(y, 'y'), _ptr(dy, 'dy'), _ptr(mean, 'mean'),
            _ptr(invstd, 'invstd'), _ptr(gamma, 'gamma', allow_none=True),
            _ptr(total[0], 'sum_dz'), _ptr(total[1], 'sum_dzx'), _ptr(dx, 'dx'), n, c, hw,
            1.0 / float(count), act, slope, _stream()), 'bn_batchnorm_bwd_apply')
    return dx, local[0], local[1]


def act_fwd(x, act, slope):
    y = torch.empty_like(x)
    _check(load().bn_act_fwd(_ptr(x, 'x'), _ptr(y, 'y'), x.numel(), act, slope, _stream()),
           'bn_act_fwd')
    return y


def act_bwd(dy, y, act, slope, out=None):
    if out is None:
        out = torch.empty_like(dy)
    _check(load().bn_act_bwd(
        _ptr(dy, 'dy'), _ptr(y, 'y'), _ptr(out, 'dpre'), dy.numel(), act, slope, _stream()),
        'bn_act_bwd')
    return out


def _linear_ws(M, K, N, device):
    """(pointer, nbytes) of this stream's scratch arena, grown for the split reductions."""
    nbytes = load().bn_linear_ws_bytes(M, K, N)
    if nbytes == 0:
        return None, 0
    return _arena(device, nbytes, 'linear'), nbytes


def linear_fwd(x, w, b):
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ws, nb = _linear_ws(M, K, N, x.device)
    _check(load().bn_linear_fwd(
        _ptr(x, 'x'), _ptr(w, 'w'), _ptr(b, 'b', allow_none=True), _ptr(y, 'y'), M, K, N,
        ws, nb, _stream()), 'bn_linear_fwd')
    return y


def linear_bwd(x, w, dy, need_dx, dact_src, dact, slope, dw, db, accumulate):
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty((M, K), dtype=torch.float32, device=dy.device) if need_dx else None
    ws, nb = _linear_ws(M, K, N, dy.device) if need_dx else (None, 0)
    _check(load().bn_linear_bwd(
        _ptr(x, 'x', allow_none=True), _ptr(w, 'w'), _ptr(dy, 'dy'),
        _ptr(dx, 'dx', allow_none=True), _ptr(dact_src, 'dact_src', allow_none=True), dact, slope,
        _ptr(dw, 'dw', allow_none=True), _ptr(db, 'db', allow_none=True), int(accumulate),
        M, K, N, ws, nb, _stream()), 'bn_linear_bwd')
    return dx


def sqerr_frame_sums(pred, target, mask):
    N = pred.shape[0]
    D = pred.numel() // N
    out = torch.empty((N,), dtype=torch.float32, device=pred.device)
    _check(load().bn_sqerr_frame_sums(
        _ptr(pred, 'pred'), _ptr(target, 'target'), _ptr(mask, 'mask', allow_none=True),
        _ptr(out, 'frame_sums'), N, D, _stream()), 'bn_sqerr_frame_sums')
    return out


def sqerr_bwd(pred, target, mask, scale, gscale, out=None):
    dpred = torch.empty_like(pred) if out is None else out
    _check(load().bn_sqerr_bwd(
        _ptr(pred, 'pred'), _ptr(target, 'target'), _ptr(mask, 'mask', allow_none=True),
        _ptr(dpred, 'dpred'), pred.numel(), float(scale), _ptr(gscale, 'gscale', allow_none=True),
        _stream()), 'bn_sqerr_bwd')
    return dpred


def convT2d_fwd_sqerr(x, w, b, target, mask, geom, act, slope, want_xhat):
    """Last decoder layer + squared error in one pass -> (xhat | None, dpre, part (N, P)):
    ``part[n].sum()`` is frame n's masked squared error, ``dpre`` its gradient with respect to the
    layer's pre-activation (see include/behavenet_hip.h)."""
    N, Ci, Hi, Wi, Co, R, S, st, ct, cl, Ho, Wo = geom
    lib = load()
    P = lib.bn_convT2d_fwd_sqerr_parts(*geom)
    if P <= 0:
        raise HipLibraryError('bn_convT2d_fwd_sqerr_parts: bad geometry %s' % (geom,))
    xhat = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device) if want_xhat \
        else None
    dpre = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device)
    part = torch.empty((N, P), dtype=torch.float32, device=x.device)
    nbytes = lib.bn_convT2d_fwd_sqerr_ws_bytes(*geom, int(want_xhat))
    ws = None
    if nbytes:
        ws = _arena(x.device, nbytes, 'fwd_sqerr')
    _check(lib.bn_convT2d_fwd_sqerr(
        _ptr(x, 'x'), _ptr(w, 'w'), _ptr(b, 'b', allow_none=True), _ptr(target, 'target'),
        _ptr(mask, 'mask', allow_none=True), _ptr(xhat, 'xhat', allow_none=True),
        _ptr(dpre, 'dpre'), _ptr(part, 'part'), *geom, act, slope, ws, nbytes, _stream()),
        'bn_convT2d_fwd_sqerr')
    return xhat, dpre, part


def scale_frames(t, frame_scale, group_scale=None, group_of_frame=None):
    """In place: t[n] *= frame_scale[n] * group_scale[group_of_frame[n]]."""
    N = t.shape[0]
    _check(load().bn_scale_frames(
        _ptr(t, 't'), _ptr(frame_scale, 'frame_scale'),
        _ptr(group_scale, 'group_scale', allow_none=True),
        _ptr(group_of_frame, 'group_of_frame', dtype=torch.int32, allow_none=True),
        N, t.numel() // N, _stream()), 'bn_scale_frames')
    return t


def reduce_sum(t, scale=1.0, out=None):
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=t.device)
    _check(load().bn_reduce_sum(_ptr(t, 'in'), _ptr(out, 'out'), t.numel(), float(scale),
                                _stream()), 'bn_reduce_sum')
    return out


def reparam_fwd(mu, logvar, eps):
    z = torch.empty_like(mu)
    _check(load().bn_reparam_fwd(
        _ptr(mu, 'mu'), _ptr(logvar, 'logvar'), _ptr(eps, 'eps'), _ptr(z, 'z'), mu.numel(),
        _stream()), 'bn_reparam_fwd')
    return z


def kl_rows(mu, logvar):
    N, D = mu.shape
    out = torch.empty((N,), dtype=torch.float32, device=mu.device)
    _check(load().bn_kl_rows(_ptr(mu, 'mu'), _ptr(logvar, 'logvar'), _ptr(out, 'kl_rows'), N, D,
                             _stream()), 'bn_kl_rows')
    return out


# widest latent block the decomposed-KL kernels serve (the grid search's max_latents)
DECOMPOSED_KL_MAX_D = 64


def _check_dkl_width(D):
    if D > DECOMPOSED_KL_MAX_D:
        raise ValueError('decomposed KL: %d latent dimensions, the kernels serve at most %d'
                         % (D, DECOMPOSED_KL_MAX_D))


def decomposed_kl_fwd(z, mu, logvar, out3=None):
    """-> (out3, log_qz, lse): the three KL terms and what the backward pass needs."""
    N, D = z.shape
    _check_dkl_width(D)
    if out3 is None:
        out3 = torch.empty((3,), dtype=torch.float32, device=z.device)
    log_qz = torch.empty((N,), dtype=torch.float32, device=z.device)
    lse = torch.empty((N, D), dtype=torch.float32, device=z.device)
    terms = torch.empty((3 * N,), dtype=torch.float32, device=z.device)
    _check(load().bn_decomposed_kl_fwd(
        _ptr(z, 'z'), _ptr(mu, 'mu'), _ptr(logvar, 'logvar'), _ptr(out3, 'out3'),
        _ptr(log_qz, 'log_qz'), _ptr(lse, 'lse'), _ptr(terms, 'terms'), N, D, _stream()),
        'bn_decomposed_kl_fwd')
    return out3, log_qz, lse


def decomposed_kl_bwd(z, mu, logvar, log_qz, lse, g3, out=None):
    N, D = z.shape
    _check_dkl_width(D)
    dz, dmu, dlogvar = out if out is not None else (
        torch.empty_like(z), torch.empty_like(z), torch.empty_like(z))
    _check(load().bn_decomposed_kl_bwd(
        _ptr(z, 'z'), _ptr(mu, 'mu'), _ptr(logvar, 'logvar'), _ptr(log_qz, 'log_qz'),
        _ptr(lse, 'lse'), _ptr(g3, 'g3'), _ptr(dz, 'dz'), _ptr(dmu, 'dmu'),
        _ptr(dlogvar, 'dlogvar'), N, D, _stream()), 'bn_decomposed_kl_bwd')
    return dz, dmu, dlogvar


def psvae_head_fwd(y, w, logvar, eps, Dw, Db, labels, lmask):
    """-> (z, z_u, lv_u, yhat, row_sq, row_kl); see include/behavenet_hip.h."""
    N, L = y.shape
    U = logvar.shape[1] - L
    dev = y.device
    z = torch.empty((N, L + U), dtype=torch.float32, device=dev)
    z_u = torch.empty((N, U), dtype=torch.float32, device=dev)
    lv_u = torch.empty((N, U), dtype=torch.float32, device=dev)
    yhat = torch.empty((N, L), dtype=torch.float32, device=dev)
    rows = torch.empty((2, N), dtype=torch.float32, device=dev)
    _check(load().bn_psvae_head_fwd(
        _ptr(y, 'y'), _ptr(w, 'w', allow_none=True), _ptr(logvar, 'logvar'), _ptr(eps, 'eps'),
        _ptr(Dw, 'Dw'), _ptr(Db, 'Db', allow_none=True), _ptr(labels, 'labels'),
        _ptr(lmask, 'lmask', allow_none=True), _ptr(z, 'z'), _ptr(z_u, 'z_u'), _ptr(lv_u, 'lv_u'),
        _ptr(yhat, 'yhat'), _ptr(rows[0], 'row_sq'), _ptr(rows[1], 'row_kl'), N, L, U, _stream()),
        'bn_psvae_head_fwd')
    return z, z_u, lv_u, yhat, rows[0], rows[1]


def psvae_head_combine(row_sq, row_kl, dkl3, bounds_dev, n_chunks, alpha, kl, beta, L):
    """-> (T (n_chunks,), cols5 (n_chunks, 5))."""
    T = torch.empty((n_chunks,), dtype=torch.float32, device=row_sq.device)
    cols5 = torch.empty((n_chunks, 5), dtype=torch.float32, device=row_sq.device)
    _check(load().bn_psvae_head_combine(
        _ptr(row_sq, 'row_sq'), _ptr(row_kl, 'row_kl'), _ptr(dkl3, 'dkl3'),
        _ptr(bounds_dev, 'bounds', dtype=torch.int32), int(n_chunks), float(alpha), float(kl),
        float(beta), int(L), _ptr(T, 'T'), _ptr(cols5, 'cols5'), _stream()), 'bn_psvae_head_combine')
    return T, cols5


def psvae_head_bwd(dz, gT, bounds_dev, n_chunks, y, logvar, eps, yhat, labels, lmask, Dw, gz_u,
                   gmu_u, glv_u, alpha, dDw, dDb, accumulate):
    """-> (dy, dw, dlogvar); dDw / dDb are written (or added to) in place."""
    N, L = y.shape
    U = logvar.shape[1] - L
    dy = torch.empty_like(y)
    dw = torch.empty((N, U), dtype=torch.float32, device=y.device)
    dlogvar = torch.empty_like(logvar)
    _check(load().bn_psvae_head_bwd(
        _ptr(dz, 'dz'), _ptr(gT, 'gT'), _ptr(bounds_dev, 'bounds', dtype=torch.int32),
        int(n_chunks), _ptr(y, 'y'), _ptr(logvar, 'logvar'), _ptr(eps, 'eps'), _ptr(yhat, 'yhat'),
        _ptr(labels, 'labels'), _ptr(lmask, 'lmask', allow_none=True), _ptr(Dw, 'Dw'),
        _ptr(gz_u, 'gz_u'), _ptr(gmu_u, 'gmu_u'), _ptr(glv_u, 'glv_u'), float(alpha),
        _ptr(dy, 'dy'), _ptr(dw, 'dw'), _ptr(dlogvar, 'dlogvar'),
        _ptr(dDw, 'dDw', allow_none=True), _ptr(dDb, 'dDb', allow_none=True),
        int(bool(accumulate)), N, L, U, _stream()), 'bn_psvae_head_bwd')
    return dy, dw, dlogvar


def reparam_bwd(dz, z, mu):
    dlogvar = torch.empty_like(mu)
    _check(load().bn_reparam_bwd(
        _ptr(dz, 'dz'), _ptr(z, 'z'), _ptr(mu, 'mu'), _ptr(dlogvar, 'dlogvar'), mu.numel(),
        _stream()), 'bn_reparam_bwd')
    return dlogvar


def kl_bwd(mu, logvar, scale, gscale, out=None):
    dmu, dlogvar = out if out is not None else (torch.empty_like(mu), torch.empty_like(mu))
    _check(load().bn_kl_bwd(
        _ptr(mu, 'mu'), _ptr(logvar, 'logvar'), _ptr(dmu, 'dmu'), _ptr(dlogvar, 'dlogvar'),
        mu.numel(), float(scale), _ptr(gscale, 'gscale', allow_none=True), _stream()),
        'bn_kl_bwd')
    return dmu, dlogvar


def adam_amsgrad_step(p, g, m, v, vmax, lr, beta1, beta2, eps, weight_decay, step):
    _check(load().bn_adam_amsgrad_step(
        _ptr(p, 'p'), _ptr(g, 'g'), _ptr(m, 'm'), _ptr(v, 'v'), _ptr(vmax, 'vmax'), p.numel(),
        lr, beta1, beta2, eps, weight_decay, int(step), _stream()), 'bn_adam_amsgrad_step')


def u8_to_unit_float(u8):
    out = torch.empty(u8.shape, dtype=torch.float32, device=u8.device)
    _check(load().bn_u8_to_unit_float(
        _ptr(u8, 'in', dtype=torch.uint8), _ptr(out, 'out'), u8.numel(), _stream()),
        'bn_u8_to_unit_float')
    return out


def unit_float_to_u8(x, out=None):
    """fp32 unit-float values -> stored uint8 grey levels of the same shape: NaN -> 0, else
    clamp(rint(x * 255), 0, 255), numpy's ``rint(float32(x) * float32(255))`` bit for bit (csrc/recon_u8.hip)."""
    out = _bf16_out(out, tuple(x.shape), torch.uint8, x.device, 'unit_float_to_u8')
    _check(load().bn_unit_float_to_u8(
        _ptr(x, 'in'), _ptr(out, 'out', dtype=torch.uint8), x.numel(), _stream()), 'bn_unit_float_to_u8')
    return out


def cond_encoder_input(x, coords, n_maps=None):
    """Frames (N, C, H, W), uint8 or fp32, and label coordinates (N, >= 2 L) -> the fp32 (N, C + L, H, W) input of a
    conditional encoder: the frames (uint8: value / 255, ``u8_to_unit_float``'s division) followed by one one-hot map
    per label, x from column l and y from column L + l through ``MakeOneHot2D``'s rule (NaN counts as 0, clip, round
    half to even) -- ``torch.cat((frames, MakeOneHot2D(H, W)(coords)), 1)`` bit for bit, built in one pass on the
    current stream from coordinates the DEVICE reads (csrc/cond_input.hip; capturable).  ``n_maps`` defaults to
    ``coords.shape[1] // 2``; further columns are ignored.  Shapes, dtypes and devices are checked before any call
    (``ValueError``)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError('cond_encoder_input: expected frames (N, C, H, W), got %s'
                         % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
    if x.dtype not in (torch.uint8, torch.float32):
        raise ValueError('cond_encoder_input: frames must be uint8 or float32, got %s' % x.dtype)
    if not torch.is_tensor(coords) or coords.dim() != 2:
        raise ValueError('cond_encoder_input: expected coordinates (N, 2 * n_maps), got %s'
                         % (tuple(coords.shape) if torch.is_tensor(coords) else type(coords).__name__,))
    if coords.shape[0] != x.shape[0]:
        raise ValueError('cond_encoder_input: %d frames but %d rows of coordinates' % (x.shape[0], coords.shape[0]))
    n_maps = coords.shape[1] // 2 if n_maps is None else int(n_maps)
    if n_maps < 0 or 2 * n_maps > coords.shape[1]:
        raise ValueError('cond_encoder_input: %d maps need %d columns of coordinates, got %d'
                         % (n_maps, 2 * n_maps, coords.shape[1]))
    if coords.device != x.device:
        raise ValueError('cond_encoder_input: frames on %s, coordinates on %s' % (x.device, coords.device))
    x = x.contiguous()
    coords = coords.to(torch.float32).contiguous()
    N, C, H, W = x.shape
    out = torch.empty((N, C + n_maps, H, W), dtype=torch.float32, device=x.device)
    _check(load().bn_cond_encoder_input(
        _ptr(x, 'frames', dtype=x.dtype), int(x.dtype == torch.uint8), _ptr(coords, 'coords'), int(coords.shape[1]),
        N, C, H, W, n_maps, _ptr(out, 'out'), _stream()), 'bn_cond_encoder_input')
    return out


def mosaic_channels(ch, n_channels):
    """``(ch0, n_ch)``, the channels a mosaic's panel shows side by side, of ``ch``: an int (that channel alone),
    None (all ``n_channels``) or a pair ``(ch0, n_ch)``; ``ValueError`` for anything else and for channels outside
    [0, n_channels)."""
    C = int(n_channels)
    if isinstance(ch, (int, np.integer)):
        ch0, n_ch = int(ch), 1
        if not 0 <= ch0 < C:
            raise ValueError('frame_mosaic_u8: channel %d of frames with %d channels' % (ch0, C))
        return ch0, n_ch
    if ch is None:
        return 0, C
    if isinstance(ch, (tuple, list)) and len(ch) == 2 and all(isinstance(v, (int, np.integer)) for v in ch):
        ch0, n_ch = int(ch[0]), int(ch[1])
        if n_ch < 1 or ch0 < 0 or ch0 + n_ch > C:
            raise ValueError('frame_mosaic_u8: channels [%d, %d) of frames with %d channels' % (ch0, ch0 + n_ch, C))
        return ch0, n_ch
    raise ValueError('frame_mosaic_u8: ch must be an int, None (all channels) or a pair (ch0, n_ch), got %r' % (ch,))


def check_mosaic_args(shape, ch=0, crop=None):
    """The crop window ``(y_min, x_min, Hc, Wc)`` of a mosaic of frames of ``shape`` (P, C, H, W) -- ``crop`` or the
    whole frame -- after the checks that need no device: ``ValueError`` for a channel outside [0, C) (``ch`` as
    ``mosaic_channels`` reads it), a negative origin (a numpy slice would wrap there) or an empty window."""
    if len(shape) != 4:
        raise ValueError('frame_mosaic_u8: expected frames (P, C, H, W), got %s' % (tuple(shape),))
    P, C, H, W = (int(v) for v in shape)
    mosaic_channels(ch, C)
    y_min, x_min, Hc, Wc = (0, 0, H, W) if crop is None else (int(v) for v in crop)
    if y_min < 0 or x_min < 0:
        raise ValueError('frame_mosaic_u8: the crop window starts at (%d, %d); a negative origin is not served '
                         '(the reference\'s numpy slice wraps there)' % (y_min, x_min))
    if Hc <= 0 or Wc <= 0:
        raise ValueError('frame_mosaic_u8: the crop window is %d x %d pixels' % (Hc, Wc))
    return y_min, x_min, Hc, Wc


def check_mosaic_src(src, n_frames):
    """``src`` as a contiguous int32 numpy array (T, R, Cc) of frame indices below ``n_frames``, -1 (any negative
    value) for a blank panel; ``ValueError`` otherwise.  Checked on the host, before the upload."""
    src = np.ascontiguousarray(np.asarray(src, dtype=np.int64))
    if src.ndim == 2:
        src = src[None]
    if src.ndim != 3:
        raise ValueError('frame_mosaic_u8: expected src (T, R, Cc) or (R, Cc), got %s' % (src.shape,))
    if src.size and int(src.max()) >= n_frames:
        raise ValueError('frame_mosaic_u8: src names frame %d of %d' % (int(src.max()), n_frames))
    return np.maximum(src, -1).astype(np.int32)


def frame_mosaic_u8(frames, src, ch=0, crop=None):
    """Frames (P, C, H, W), fp32 unit floats or uint8 grey levels, -> the uint8 DEVICE mosaic (T, R * Hc, Cc * Wc)
    whose panel (t, r, c) shows channel ``ch`` of frame ``src[t, r, c]`` inside the window ``crop = (y_min, x_min, Hc,
    Wc)`` (default: the whole frame), zero where the window passes the bottom or right edge and where ``src`` is
    negative.  fp32 frames are quantised by ``unit_float_to_u8``'s rule.  ``ch=None`` shows all C channels of the
    frame side by side in its panel, as the reference's ``concat`` does, and a pair ``ch=(ch0, n_ch)`` the channels
    ``ch0 .. ch0 + n_ch - 1``: the mosaic is then (T, R * Hc, Cc * n_ch * Wc) and sub-panel q of panel (t, r, c) shows
    channel ``ch0 + q`` (``bn_frame_mosaic_ch_u8``; an int ``ch`` is ``bn_frame_mosaic_u8``).  ``src``: a host array
    (T, R, Cc) or (R, Cc), checked against P here and uploaded, or an int32 device tensor (T, R, Cc) the caller has
    checked (``check_mosaic_src``).  One pass on the current stream (csrc/frame_mosaic.hip)."""
    if not torch.is_tensor(frames) or frames.dim() != 4:
        raise ValueError('frame_mosaic_u8: expected frames (P, C, H, W), got %s'
                         % (tuple(frames.shape) if torch.is_tensor(frames) else type(frames).__name__,))
    if frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError('frame_mosaic_u8: frames must be uint8 or float32, got %s' % frames.dtype)
    y_min, x_min, Hc, Wc = check_mosaic_args(frames.shape, ch, crop)
    if not torch.is_tensor(src):
        src = torch.from_numpy(check_mosaic_src(src, frames.shape[0])).to(frames.device)
    if src.dim() != 3 or src.dtype != torch.int32:
        raise ValueError('frame_mosaic_u8: a device src must be int32 (T, R, Cc), got %s %s'
                         % (src.dtype, tuple(src.shape)))
    frames, src = frames.contiguous(), src.contiguous()
    P, C, H, W = frames.shape
    T, R, Cc = src.shape
    ch0, n_ch = mosaic_channels(ch, C)
    out = torch.empty((T, R * Hc, Cc * n_ch * Wc), dtype=torch.uint8, device=frames.device)
    if isinstance(ch, (int, np.integer)):
        _check(load().bn_frame_mosaic_u8(
            _ptr(frames, 'frames', dtype=frames.dtype), int(frames.dtype == torch.uint8), P, C, H, W, ch0, y_min,
            x_min, Hc, Wc, _ptr(src, 'src', dtype=torch.int32), T, R, Cc, _ptr(out, 'out', dtype=torch.uint8),
            _stream()), 'bn_frame_mosaic_u8')
    else:
        _check(load().bn_frame_mosaic_ch_u8(
            _ptr(frames, 'frames', dtype=frames.dtype), int(frames.dtype == torch.uint8), P, C, H, W, ch0, n_ch, y_min,
            x_min, Hc, Wc, _ptr(src, 'src', dtype=torch.int32), T, R, Cc, _ptr(out, 'out', dtype=torch.uint8),
            _stream()), 'bn_frame_mosaic_ch_u8')
    return out


def stamp_boxes_u8(movie, mark, panel_hw, box=(5, 5, 10, 10), value=255):
    """Marker boxes into the uint8 DEVICE ``movie`` (T, R * Hp, Cc * Wp), IN PLACE: for every panel (t, r, c) of
    ``panel_hw = (Hp, Wp)`` pixels with ``mark[t, r, c] != 0`` the pixels ``box = (y0, x0, h, w)`` of the panel, rows
    ``y0 .. y0 + h - 1`` and columns ``x0 .. x0 + w - 1`` clipped to the panel, are set to ``value``
    (``bn_stamp_boxes_u8``, csrc/frame_mosaic.hip); nothing else is written.  ``mark``: (T, R, Cc), a host array
    (uploaded) or a uint8 device tensor.  ``ValueError`` for a movie that is not uint8, 3-d and contiguous on the
    GPU and for a ``mark`` whose shape does not divide the movie into panels of ``panel_hw``.  -> ``movie``."""
    who = 'stamp_boxes_u8'
    if not torch.is_tensor(movie) or movie.dim() != 3 or movie.dtype != torch.uint8 or not movie.is_contiguous():
        raise ValueError('%s: expected a contiguous uint8 movie (T, R * Hp, Cc * Wp), got %s'
                         % (who, (movie.dtype, tuple(movie.shape), tuple(movie.stride())) if torch.is_tensor(movie)
                            else type(movie).__name__))
    if not movie.is_cuda:
        raise ValueError('%s: expected the movie on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, movie.device))
    if not torch.is_tensor(mark):
        mark = torch.from_numpy(np.ascontiguousarray(np.asarray(mark) != 0).astype(np.uint8)).to(movie.device)
    if mark.dtype != torch.uint8 or mark.device != movie.device:
        raise ValueError('%s: a device mark must be uint8 on %s, got %s on %s'
                         % (who, movie.device, mark.dtype, mark.device))
    Hp, Wp = (int(v) for v in panel_hw)
    y0, x0, h, w = (int(v) for v in box)
    value = int(value)
    if Hp < 1 or Wp < 1 or h < 0 or w < 0 or not 0 <= value <= 255:
        raise ValueError('%s: panels of %d x %d, a box of %d x %d, value %d' % (who, Hp, Wp, h, w, value))
    T = int(movie.shape[0])
    if mark.dim() != 3 or (int(mark.shape[0]), int(mark.shape[1]) * Hp, int(mark.shape[2]) * Wp) != tuple(movie.shape):
        raise ValueError('%s: mark %s does not divide the movie %s into panels of %d x %d'
                         % (who, tuple(mark.shape), tuple(movie.shape), Hp, Wp))
    mark = mark.contiguous()
    R, Cc = int(mark.shape[1]), int(mark.shape[2])
    if T * R * Cc:
        _check(load().bn_stamp_boxes_u8(movie.data_ptr(), T, R, Cc, Hp, Wp, mark.data_ptr(), y0, x0, h, w, value,
                                        _stream()), 'bn_stamp_boxes_u8')
    return movie


# csrc/column_select.hip's partition, restated for the tests that have to name a row count by it (held against
# bn_column_select_ws_bytes in tests/test_ranges_cpu.py): CS_HISTS, CS_MIN_ELEMS, CS_TARGET_GROUPS
COLUMN_SELECT_HISTS, COLUMN_SELECT_MIN_ELEMS, COLUMN_SELECT_TARGET_GROUPS = 60, 1 << 16, 512
COLUMN_SELECT_MAX_D, COLUMN_SELECT_MAX_R = 1024, 8


def column_select_plan(n, d, r):
    """``(cols, col_groups, slabs, rows)`` of ``bn_column_select`` on an (n, d) table with r rank slots a column:
    the columns a workgroup takes, the column groups, the row blocks and the rows of a block (cs_plan; r = 0 is
    the count pass, every column in one group)."""
    cols = min(COLUMN_SELECT_HISTS // r, d) if r else d
    col_groups = -(-d // cols)
    for_chip = max(COLUMN_SELECT_TARGET_GROUPS // col_groups, 1)
    min_rows = max(COLUMN_SELECT_MIN_ELEMS // d, 1)
    want = min(for_chip, -(-n // min_rows))
    rows = -(-n // want)
    return cols, col_groups, -(-n // rows), rows


def _column_table(who, x):
    """(n, d, ld) of a table the column kernels take: fp32 on the GPU, two dimensions, unit stride along the rows'
    elements and a row stride ld >= d (a column slice of a contiguous table is served as it is)."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('%s: expected a table (n, d), got %s'
                         % (who, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    if x.dtype != torch.float32:
        raise ValueError('%s: the table must be float32, got %s' % (who, x.dtype))
    if not x.is_cuda:
        raise ValueError('%s: expected the table on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, x.device))
    n, d = (int(v) for v in x.shape)
    if n < 1 or not 1 <= d <= COLUMN_SELECT_MAX_D:
        raise ValueError('%s: a table of %d rows and %d columns (1 to %d columns are served)'
                         % (who, n, d, COLUMN_SELECT_MAX_D))
    ld = d if n == 1 else int(x.stride(0))
    if (d > 1 and x.stride(1) != 1) or ld < d:
        raise ValueError('%s: the table\'s rows must be contiguous, got strides %s' % (who, tuple(x.stride())))
    return n, d, ld


def column_count(x):
    """The number of non-NaN values in every column of the fp32 DEVICE table ``x`` (n, d) as an int64 device tensor
    (d,), on the current stream (``bn_column_count``, csrc/column_select.hip)."""
    n, d, ld = _column_table('column_count', x)
    lib = load()
    nbytes = lib.bn_column_select_ws_bytes(n, d, 1)
    out = torch.empty((d,), dtype=torch.int64, device=x.device)
    _check(lib.bn_column_count(x.data_ptr(), n, d, ld, out.data_ptr(), _arena(x.device, nbytes, 'column_select'), nbytes,
                               _stream()), 'bn_column_count')
    return out


def column_select(x, ranks):
    """Exact order statistics of the columns of the fp32 DEVICE table ``x`` (n, d): ``out[k, j]`` is the value of
    column j with ``ranks[k, j]`` non-NaN values before it in ascending order, NaN where the rank is negative or not
    below the column's number of non-NaN values.  ``ranks``: int64 (r, d), 1 <= r <= 8, a host array (uploaded) or a
    device tensor.  -> fp32 device tensor (r, d).  Four passes over the table on the current stream
    (``bn_column_select``, csrc/column_select.hip); the same bits on every call."""
    n, d, ld = _column_table('column_select', x)
    if not torch.is_tensor(ranks):
        ranks = torch.from_numpy(np.ascontiguousarray(np.asarray(ranks), dtype=np.int64)).to(x.device)
    if ranks.dim() != 2 or ranks.dtype != torch.int64 or ranks.shape[1] != d:
        raise ValueError('column_select: expected ranks int64 (r, %d), got %s %s' % (d, ranks.dtype, tuple(ranks.shape)))
    r = int(ranks.shape[0])
    if not 1 <= r <= COLUMN_SELECT_MAX_R:
        raise ValueError('column_select: %d ranks a column (1 to %d are served)' % (r, COLUMN_SELECT_MAX_R))
    if ranks.device != x.device:
        raise ValueError('column_select: the table is on %s, the ranks on %s' % (x.device, ranks.device))
    ranks = ranks.contiguous()
    lib = load()
    nbytes = lib.bn_column_select_ws_bytes(n, d, r)
    out = torch.empty((r, d), dtype=torch.float32, device=x.device)
    _check(lib.bn_column_select(x.data_ptr(), n, d, ld, ranks.data_ptr(), r, out.data_ptr(),
                                _arena(x.device, nbytes, 'column_select'), nbytes, _stream()), 'bn_column_select')
    return out


# csrc/segment_sums.hip's partition, restated for the tests that have to name a row count by it (held against
# bn_segment_label_sums_ws_bytes in tests/test_label_r2_cpu.py): SL_MIN_ELEMS, SL_TARGET_GROUPS, SL_MAX_L
_SEGMENT_SUMS_MIN_ELEMS, _SEGMENT_SUMS_TARGET_GROUPS, _SEGMENT_SUMS_MAX_L = 1 << 14, 1024, 64


def _segment_sums_plan(n, L):
    """``(blocks, rows)`` of ``bn_segment_label_sums`` on tables of n rows and L columns: the row blocks and the rows
    of a block, the last block taking what is left (sl_plan)."""
    if n < 1:
        return 0, 1
    want = min(-(-n // (_SEGMENT_SUMS_MIN_ELEMS // L)), _SEGMENT_SUMS_TARGET_GROUPS)
    rows = -(-n // want)
    return -(-n // rows), rows


def _label_table(name, x, like=None):
    """(n, L, ld) of a table ``bn_segment_label_sums`` takes (``_column_table``'s conditions, at most 64 columns, and
    the shape of ``like``)."""
    n, L, ld = _column_table('segment_label_sums (%s)' % name, x)
    if L > _SEGMENT_SUMS_MAX_L:
        raise ValueError('segment_label_sums: %d columns (1 to %d are served)' % (L, _SEGMENT_SUMS_MAX_L))
    if like is not None and x.shape != like.shape:
        raise ValueError('segment_label_sums: pred is %s, %s is %s' % (tuple(like.shape), name, tuple(x.shape)))
    return n, L, ld


def segment_label_sums(pred, truth, mask, offsets):
    """Per row segment and column, the count, ``sum y``, ``sum y^2`` and ``sum (y - p)^2`` over the valid entries of
    the fp32 DEVICE tables ``pred`` (p) and ``truth`` (y), both (n, L) with L <= 64: a float64 device tensor
    ``(S, L, 4)``, on the current stream (``bn_segment_label_sums``, csrc/segment_sums.hip).  ``mask`` is None (every
    entry is valid) or a table (n, L): an entry is valid where the mask is exactly 1.  ``offsets``: int64 (S + 1), a
    host array (uploaded) or a device tensor; segment s is the rows ``[offsets[s], offsets[s + 1])``.  The tables may
    be the first L columns of wider ones.  Terms and sums are float64; the same bits on every call."""
    n, L, ld_pred = _label_table('pred', pred)
    ld_truth = _label_table('truth', truth, pred)[2]
    ld_mask = 0 if mask is None else _label_table('mask', mask, pred)[2]
    if not torch.is_tensor(offsets):
        offsets = torch.from_numpy(np.ascontiguousarray(np.asarray(offsets), dtype=np.int64)).to(pred.device)
    if offsets.dim() != 1 or offsets.dtype != torch.int64 or offsets.numel() < 1:
        raise ValueError('segment_label_sums: expected offsets int64 (S + 1,), got %s %s'
                         % (offsets.dtype, tuple(offsets.shape)))
    for name, t in (('truth', truth), ('mask', mask), ('offsets', offsets)):
        if t is not None and t.device != pred.device:
            raise ValueError('segment_label_sums: pred is on %s, %s on %s' % (pred.device, name, t.device))
    offsets = offsets.contiguous()
    S = int(offsets.numel()) - 1
    lib = load()
    nbytes = lib.bn_segment_label_sums_ws_bytes(n, S, L)
    out = torch.empty((S, L, 4), dtype=torch.float64, device=pred.device)
    if S:
        _check(lib.bn_segment_label_sums(pred.data_ptr(), ld_pred, truth.data_ptr(), ld_truth,
                                         None if mask is None else mask.data_ptr(), ld_mask, offsets.data_ptr(), S, L,
                                         n, out.data_ptr(), _arena(pred.device, nbytes, 'segment_sums'), nbytes,
                                         _stream()), 'bn_segment_label_sums')
    return out


# csrc/segment_gram.hip's partition, restated for the tests that have to name a row count by it (held against
# bn_segment_gram_ws_bytes in tests/test_latent_corr_cpu.py): SG_MIN_ELEMS, SG_TARGET_GROUPS, SG_SLAB_BYTES, SG_MAX_D
_SEGMENT_GRAM_MIN_ELEMS, _SEGMENT_GRAM_TARGET_GROUPS = 1 << 14, 1024
_SEGMENT_GRAM_SLAB_BYTES, _SEGMENT_GRAM_MAX_D = 32 << 20, 64


def _segment_gram_plan(n, D):
    """``(blocks, rows)`` of ``bn_segment_gram`` on a table of n rows and D columns: the row blocks and the rows of a
    block, the last block taking what is left (sg_plan); two partial matrices a block fit into 32 MiB."""
    if n < 1:
        return 0, 1
    cap = min(_SEGMENT_GRAM_SLAB_BYTES // (2 * (D + 1) * (D + 1) * 8), _SEGMENT_GRAM_TARGET_GROUPS)
    want = min(-(-n // (_SEGMENT_GRAM_MIN_ELEMS // D)), cap)
    rows = -(-n // want)
    return -(-n // rows), rows


def segment_gram(table, offsets, shift=None):
    """Per row segment the augmented second-moment matrix of the fp32 DEVICE ``table`` (n, D), D <= 64: a float64
    device tensor ``(S, D + 1, D + 1)``, the sum over the segment's rows of ``a^T a`` with ``a = (1, z - shift)`` in
    float64 -- ``[0, 0]`` the row count, ``[0, 1:]`` the column sums, ``[1:, 1:]`` the second moments -- on the current
    stream (``bn_segment_gram``, csrc/segment_gram.hip).  ``offsets``: int64 (S + 1), a host array (uploaded) or a
    device tensor; segment s is the rows ``[offsets[s], offsets[s + 1])``.  ``shift``: None (zeros) or D fp32 values
    on the device.  The table may be a column slice of a wider one (row stride >= D, unit column stride).  The same
    bits on every call."""
    n, D, ld = _column_table('segment_gram', table)
    if D > _SEGMENT_GRAM_MAX_D:
        raise ValueError('segment_gram: %d columns (1 to %d are served)' % (D, _SEGMENT_GRAM_MAX_D))
    if not torch.is_tensor(offsets):
        offsets = torch.from_numpy(np.ascontiguousarray(np.asarray(offsets), dtype=np.int64)).to(table.device)
    if offsets.dim() != 1 or offsets.dtype != torch.int64 or offsets.numel() < 1:
        raise ValueError('segment_gram: expected offsets int64 (S + 1,), got %s %s'
                         % (offsets.dtype, tuple(offsets.shape)))
    if shift is not None and (not torch.is_tensor(shift) or shift.dtype != torch.float32 or shift.shape != (D,)):
        raise ValueError('segment_gram: expected shift float32 (%d,), got %s'
                         % (D, (shift.dtype, tuple(shift.shape)) if torch.is_tensor(shift) else type(shift).__name__))
    for name, t in (('shift', shift), ('offsets', offsets)):
        if t is not None and t.device != table.device:
            raise ValueError('segment_gram: the table is on %s, %s on %s (the HIP path has no CPU fallback)'
                             % (table.device, name, t.device))
    offsets = offsets.contiguous()
    shift = None if shift is None else shift.contiguous()
    S = int(offsets.numel()) - 1
    lib = load()
    nbytes = lib.bn_segment_gram_ws_bytes(n, S, D)
    out = torch.empty((S, D + 1, D + 1), dtype=torch.float64, device=table.device)
    if S:
        _check(lib.bn_segment_gram(table.data_ptr(), ld, None if shift is None else shift.data_ptr(),
                                   offsets.data_ptr(), S, D, n, out.data_ptr(),
                                   _arena(table.device, nbytes, 'segment_gram'), nbytes, _stream()), 'bn_segment_gram')
    return out


# csrc/softmax_cv.hip's limits and partition, restated for the callers that check before a launch and for the tests
# that have to name a row count by the plan (held against the workspace queries in tests/test_classifier_cpu.py):
# SC_MAX_D, SC_MAX_S, SC_MAX_M, SC_GC, SC_MIN_ROWS, SC_TARGET_BLOCKS, SC_SLAB_BYTES, SC_ROWS
SOFTMAX_CV_MAX_D, SOFTMAX_CV_MAX_S, SOFTMAX_CV_MAX_M = 64, 8, 64
_SOFTMAX_CV_GROUP_COLUMNS, _SOFTMAX_CV_MIN_ROWS, _SOFTMAX_CV_TARGET_BLOCKS = 128, 128, 1024
_SOFTMAX_CV_SLAB_BYTES, SOFTMAX_CV_CHUNK_ROWS = 32 << 20, 32


def _softmax_cv_plan(n, D, S, M, score=False):
    """``(blocks, rows, models_per_group)`` of ``bn_softmax_cv_lossgrad`` (or ``_score``): the row blocks, the rows
    of a block (the last block takes what is left) and the models a workgroup serves (sc_plan)."""
    mg = min(_SOFTMAX_CV_GROUP_COLUMNS // S, M)
    if n < 1:
        return 0, 1, mg
    pm = 2 if score else S * (D + 1) + 2
    cap = min(_SOFTMAX_CV_SLAB_BYTES // (M * pm * 8), _SOFTMAX_CV_TARGET_BLOCKS)
    want = min(-(-n // _SOFTMAX_CV_MIN_ROWS), cap)
    rows = -(-n // want)
    return -(-n // rows), rows, mg


def _softmax_cv_operands(who, z, y, fold, W, leave):
    if not torch.is_tensor(z) or z.dim() != 2:
        raise TypeError('%s: expected a device table (n, D), got %s'
                        % (who, tuple(z.shape) if torch.is_tensor(z) else type(z).__name__))
    if z.dtype != torch.float32:
        raise TypeError('%s: the table must be float32, got %s' % (who, z.dtype))
    if not z.is_cuda:
        raise ValueError('%s: expected the table on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, z.device))
    n, D = (int(v) for v in z.shape)
    if not 1 <= D <= SOFTMAX_CV_MAX_D:
        raise ValueError('%s: %d columns (1 to %d are served)' % (who, D, SOFTMAX_CV_MAX_D))
    ld = D if n <= 1 else int(z.stride(0))
    if (D > 1 and n > 0 and z.stride(1) != 1) or ld < D:
        raise ValueError('%s: the table\'s rows must be contiguous, got strides %s' % (who, tuple(z.stride())))
    if not torch.is_tensor(W) or W.dim() != 3:
        raise TypeError('%s: expected weights (M, S, D + 1), got %s'
                        % (who, tuple(W.shape) if torch.is_tensor(W) else type(W).__name__))
    if W.dtype != torch.float64:
        raise TypeError('%s: the weights must be float64, got %s' % (who, W.dtype))
    M, S = int(W.shape[0]), int(W.shape[1])
    if W.shape[2] != D + 1:
        raise ValueError('%s: weights %s for %d columns and an intercept' % (who, tuple(W.shape), D))
    if not 2 <= S <= SOFTMAX_CV_MAX_S or not 1 <= M <= SOFTMAX_CV_MAX_M:
        raise ValueError('%s: %d classes and %d models (2 to %d classes and 1 to %d models are served)'
                         % (who, S, M, SOFTMAX_CV_MAX_S, SOFTMAX_CV_MAX_M))
    for name, t, length in (('y', y, n), ('fold', fold, n), ('leave', leave, M)):
        if t is None and name == 'fold':
            continue
        if not torch.is_tensor(t):
            raise TypeError('%s: expected %s as a device tensor, got %s' % (who, name, type(t).__name__))
        if t.dtype != torch.int32:
            raise TypeError('%s: %s must be int32, got %s' % (who, name, t.dtype))
        if t.shape != (length,):
            raise ValueError('%s: expected %s (%d,), got %s' % (who, name, length, tuple(t.shape)))
    for name, t in (('y', y), ('fold', fold), ('W', W), ('leave', leave)):
        if t is not None and t.device != z.device:
            raise ValueError('%s: the table is on %s, %s on %s (the HIP path has no CPU fallback)'
                             % (who, z.device, name, t.device))
    return (n, D, S, M, ld, y.contiguous(), None if fold is None else fold.contiguous(), W.contiguous(),
            leave.contiguous())


def softmax_cv_lossgrad(z, y, fold, W, leave, packed=False):
    """Loss, gradient and row count of M multinomial logistic models at once over the fp32 DEVICE table ``z`` (n, D),
    D <= 64 (``bn_softmax_cv_lossgrad``, csrc/softmax_cv.hip): ``y`` int32 (n) the class of a row, ``fold`` int32 (n)
    its fold or None, ``W`` float64 (M, S, D + 1) with the intercept in column D, ``leave`` int32 (M) the fold a model
    leaves out (-1: none), all on the device -> float64 device tensors ``(loss (M,), grad (M, S, D + 1), count (M,))``
    = the sums of ``logsumexp(l) - l_y`` and ``(softmax(l) - onehot(y)) (x) (z, 1)`` over the rows a model includes,
    on the current stream.  The table may be a column slice of a wider one.  The same bits on every call.
    ``packed=True`` returns the ONE buffer the three are views of instead, ``M (S (D + 1) + 2)`` doubles: the losses,
    the counts, then the gradients -- what a caller sends to the host in one transfer."""
    n, D, S, M, ld, y, fold, W, leave = _softmax_cv_operands('softmax_cv_lossgrad', z, y, fold, W, leave)
    lib = load()
    nbytes = lib.bn_softmax_cv_lossgrad_ws_bytes(n, D, S, M)
    out = torch.empty(M * (S * (D + 1) + 2), dtype=torch.float64, device=z.device)
    loss, count, grad = out[:M], out[M:2 * M], out[2 * M:].view(M, S, D + 1)
    if n == 0:          # (an empty table has no address to hand over: the sums over no rows)
        out.zero_()
        return out if packed else (loss, grad, count)
    _check(lib.bn_softmax_cv_lossgrad(z.data_ptr(), ld, y.data_ptr(), None if fold is None else fold.data_ptr(),
                                      W.data_ptr(), leave.data_ptr(), n, D, S, M, loss.data_ptr(), grad.data_ptr(),
                                      count.data_ptr(), _arena(z.device, nbytes, 'softmax_cv'), nbytes, _stream()),
           'bn_softmax_cv_lossgrad')
    return out if packed else (loss, grad, count)


def softmax_cv_score(z, y, fold, W, leave):
    """``(hits, rows)`` per model, a float64 device tensor (M, 2) of exact integers: over the rows of model m's held-out
    fold -- ``fold == leave[m]``, every row for ``leave[m] == -1`` -- with ``y`` in [0, S) the rows whose float64
    argmax logit is ``y`` (ties to the lowest class) and the rows (``bn_softmax_cv_score``).  Operands as
    ``softmax_cv_lossgrad``'s."""
    n, D, S, M, ld, y, fold, W, leave = _softmax_cv_operands('softmax_cv_score', z, y, fold, W, leave)
    lib = load()
    nbytes = lib.bn_softmax_cv_score_ws_bytes(n, D, S, M)
    out = torch.empty((M, 2), dtype=torch.float64, device=z.device)
    if n == 0:
        return out.zero_()
    _check(lib.bn_softmax_cv_score(z.data_ptr(), ld, y.data_ptr(), None if fold is None else fold.data_ptr(),
                                   W.data_ptr(), leave.data_ptr(), n, D, S, M, out.data_ptr(),
                                   _arena(z.device, nbytes, 'softmax_cv'), nbytes, _stream()), 'bn_softmax_cv_score')
    return out


# csrc/arhmm.hip's limits and the partition of bn_arhmm_moments, restated for the callers that check before a launch
# and for the tests that have to name a row count by the plan (held against the workspace query in
# tests/test_arhmm_cpu.py): AR_MAX_K, AR_MAX_L, AR_MAX_LD, AR_MO_MIN_ROWS, AR_MO_TARGET_BLOCKS, AR_MO_SLAB_BYTES
ARHMM_MAX_K, ARHMM_MAX_LAGS, ARHMM_MAX_LAGGED_COLUMNS = 32, 8, 64
_ARHMM_MIN_ROWS, _ARHMM_TARGET_BLOCKS, _ARHMM_SLAB_BYTES = 512, 1024, 60 << 20


def _arhmm_moments_plan(n, D, L, K):
    """``(blocks, rows)`` of ``bn_arhmm_moments``: the row blocks and the rows of a block, the last block taking what
    is left (ar_plan); K partial matrices (P, P) a block fit into 60 MiB."""
    if n < 1:
        return 0, 1
    P = 1 + (L + 1) * D
    cap = min(_ARHMM_SLAB_BYTES // (K * P * P * 8), _ARHMM_TARGET_BLOCKS)
    want = min(-(-n // _ARHMM_MIN_ROWS), cap)
    rows = -(-n // want)
    return -(-n // rows), rows


def _arhmm_moments_group(D, L):
    """The states a workgroup of ``bn_arhmm_moments`` takes with one staging of its rows (ar_mo_group): 4 up to 32
    columns of ``a_t``, 2 up to 64, 1 beyond."""
    P = 1 + (L + 1) * D
    return 4 if P <= 32 else (2 if P <= 64 else 1)


def check_arhmm_dims(who, D, L, K):
    """ValueError unless (D, L, K) are dimensions the ARHMM kernels serve."""
    if not 1 <= K <= ARHMM_MAX_K:
        raise ValueError('%s: %d states (1 to %d are served)' % (who, K, ARHMM_MAX_K))
    if not 0 <= L <= ARHMM_MAX_LAGS:
        raise ValueError('%s: %d lags (0 to %d are served)' % (who, L, ARHMM_MAX_LAGS))
    if D < 1 or (L + 1) * D > ARHMM_MAX_LAGGED_COLUMNS:
        raise ValueError('%s: %d columns at %d lags, (lags + 1) * columns = %d (1 to %d are served)'
                         % (who, D, L, (L + 1) * D, ARHMM_MAX_LAGGED_COLUMNS))


def _f64_operand(who, name, x, shape, device, allow_none=False):
    """``x`` as a contiguous float64 tensor of ``shape`` on ``device``: a host array is uploaded, a tensor must be
    float64 and on the device already."""
    if x is None:
        if allow_none:
            return None
        raise ValueError('%s: %s is None' % (who, name))
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float64)).to(device)
    if x.dtype != torch.float64 or tuple(x.shape) != tuple(shape):
        raise ValueError('%s: expected %s float64 %s, got %s %s' % (who, name, tuple(shape), x.dtype, tuple(x.shape)))
    if x.device != device:
        raise ValueError('%s: the table is on %s, %s on %s (the HIP path has no CPU fallback)'
                         % (who, device, name, x.device))
    return x.contiguous()


def _trial_offsets(who, offsets, device):
    if not torch.is_tensor(offsets):
        offsets = torch.from_numpy(np.ascontiguousarray(np.asarray(offsets), dtype=np.int64)).to(device)
    if offsets.dim() != 1 or offsets.dtype != torch.int64 or offsets.numel() < 1:
        raise ValueError('%s: expected offsets int64 (S + 1,), got %s %s' % (who, offsets.dtype, tuple(offsets.shape)))
    if offsets.device != device:
        raise ValueError('%s: the table is on %s, offsets on %s (the HIP path has no CPU fallback)'
                         % (who, device, offsets.device))
    return offsets.contiguous()


def _ll_table(who, ll):
    """(n, K) of a table of log-likelihoods: float64, contiguous, on the GPU, 1 <= K <= 32."""
    if not torch.is_tensor(ll) or ll.dim() != 2 or ll.dtype != torch.float64:
        raise ValueError('%s: expected ll float64 (n, K), got %s'
                         % (who, (ll.dtype, tuple(ll.shape)) if torch.is_tensor(ll) else type(ll).__name__))
    n, K = (int(v) for v in ll.shape)
    if not 1 <= K <= ARHMM_MAX_K:
        raise ValueError('%s: %d states (1 to %d are served)' % (who, K, ARHMM_MAX_K))
    if not ll.is_cuda:
        raise ValueError('%s: expected ll on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, ll.device))
    if not ll.is_contiguous():
        raise ValueError('%s: ll must be contiguous, got strides %s' % (who, tuple(ll.stride())))
    return n, K


def arhmm_loglik(table, offsets, G, cst, lags, shift=None, out=None):
    """Emission log-likelihoods of an ARHMM on the fp32 DEVICE ``table`` (n, D): a float64 device tensor (n, K)
    (``bn_arhmm_loglik``, csrc/arhmm.hip).  ``offsets``: int64 (S + 1), the trials; ``G`` float64 (K, D, P) and ``cst``
    (K), the folded parameters (``models.arhmm.ARHMM.fold``), P = 1 + (lags + 1) D; ``shift``: None or D float64 values.
    Host arrays are uploaded.  Row t of a trial with t < lags gets the standard normal density of the row for every
    state.  Rows outside the trials are left as they are (zeros in a fresh ``out``)."""
    n, D, ld = _column_table('arhmm_loglik', table)
    L = int(lags)
    if not torch.is_tensor(G) and np.ndim(G) != 3 or torch.is_tensor(G) and G.dim() != 3:
        raise ValueError('arhmm_loglik: expected G float64 (K, D, P)')
    K = int(G.shape[0])
    check_arhmm_dims('arhmm_loglik', D, L, K)
    P = 1 + (L + 1) * D
    dev = table.device
    G = _f64_operand('arhmm_loglik', 'G', G, (K, D, P), dev)
    cst = _f64_operand('arhmm_loglik', 'cst', cst, (K,), dev)
    shift = _f64_operand('arhmm_loglik', 'shift', shift, (D,), dev, allow_none=True)
    offsets = _trial_offsets('arhmm_loglik', offsets, dev)
    S = int(offsets.numel()) - 1
    if out is None:
        out = torch.zeros((n, K), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n, K) or out.device != dev or not out.is_contiguous():
        raise ValueError('arhmm_loglik: expected out float64 (%d, %d) on %s' % (n, K, dev))
    lib = load()
    nbytes = lib.bn_arhmm_loglik_ws_bytes(n, S, D, L, K)
    if S:
        _check(lib.bn_arhmm_loglik(table.data_ptr(), ld, None if shift is None else shift.data_ptr(),
                                   offsets.data_ptr(), S, D, L, K, n, G.data_ptr(), cst.data_ptr(), out.data_ptr(),
                                   _arena(dev, nbytes, 'arhmm'), nbytes, _stream()), 'bn_arhmm_loglik')
    return out


def hmm_forward_backward(ll, offsets, log_Ps, log_pi0, want_posteriors=True, gamma=None, xi=None):
    """Forward-backward per trial over the float64 DEVICE table ``ll`` (n, K) of log-likelihoods
    (``bn_hmm_forward_backward``): ``(gamma, xi, loglik)`` -- the state marginals (n, K), per trial the summed pairwise
    posteriors (S, K, K) and the log-likelihood (S,), float64 device tensors.  ``want_posteriors=False`` runs the
    forward sweep alone and returns ``(None, None, loglik)``; a ``gamma`` / ``xi`` given then is not touched.
    ``log_Ps`` (K, K) and ``log_pi0`` (K): float64, host arrays are uploaded."""
    n, K = _ll_table('hmm_forward_backward', ll)
    dev = ll.device
    log_Ps = _f64_operand('hmm_forward_backward', 'log_Ps', log_Ps, (K, K), dev)
    log_pi0 = _f64_operand('hmm_forward_backward', 'log_pi0', log_pi0, (K,), dev)
    offsets = _trial_offsets('hmm_forward_backward', offsets, dev)
    S = int(offsets.numel()) - 1
    loglik = torch.empty((S,), dtype=torch.float64, device=dev)
    want = 1 if want_posteriors else 0
    if want:
        if gamma is None:
            gamma = torch.zeros((n, K), dtype=torch.float64, device=dev)
        if xi is None:
            xi = torch.empty((S, K, K), dtype=torch.float64, device=dev)
        for name, t, shape in (('gamma', gamma, (n, K)), ('xi', xi, (S, K, K))):
            if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError('hmm_forward_backward: expected %s float64 %s on %s' % (name, shape, dev))
    lib = load()
    nbytes = lib.bn_hmm_forward_backward_ws_bytes(n, S, K)
    if S:
        _check(lib.bn_hmm_forward_backward(ll.data_ptr(), offsets.data_ptr(), S, K, n, log_Ps.data_ptr(),
                                           log_pi0.data_ptr(), want, gamma.data_ptr() if want else None,
                                           xi.data_ptr() if want else None, loglik.data_ptr(),
                                           _arena(dev, nbytes, 'arhmm'), nbytes, _stream()),
               'bn_hmm_forward_backward')
    return (gamma, xi, loglik) if want else (None, None, loglik)


def arhmm_moments(table, offsets, gamma, lags, shift=None):
    """Weighted lagged moments of the fp32 DEVICE ``table`` (n, D): ``(out, gamma0)``, float64 device tensors
    (K, P, P) and (K,) (``bn_arhmm_moments``).  ``out[k]`` is the sum over the AR rows of ``gamma[t, k] a_t^T a_t`` with
    ``a_t = (1, x_t - shift, ..., x_{t-lags} - shift)``, ``gamma0[k]`` the sum of ``gamma[t, k]`` over the first
    ``lags`` rows of every trial.  ``gamma``: float64 DEVICE (n, K)."""
    n, D, ld = _column_table('arhmm_moments', table)
    L = int(lags)
    if not torch.is_tensor(gamma) or gamma.dim() != 2:
        raise ValueError('arhmm_moments: expected gamma float64 (n, K) on the device')
    K = int(gamma.shape[1])
    check_arhmm_dims('arhmm_moments', D, L, K)
    dev = table.device
    gamma = _f64_operand('arhmm_moments', 'gamma', gamma, (n, K), dev)
    shift = _f64_operand('arhmm_moments', 'shift', shift, (D,), dev, allow_none=True)
    offsets = _trial_offsets('arhmm_moments', offsets, dev)
    S = int(offsets.numel()) - 1
    P = 1 + (L + 1) * D
    out = torch.empty((K, P, P), dtype=torch.float64, device=dev)
    gamma0 = torch.empty((K,), dtype=torch.float64, device=dev)
    if not S:
        return out.zero_(), gamma0.zero_()
    lib = load()
    nbytes = lib.bn_arhmm_moments_ws_bytes(n, S, D, L, K)
    _check(lib.bn_arhmm_moments(table.data_ptr(), ld, None if shift is None else shift.data_ptr(), offsets.data_ptr(),
                                S, D, L, K, n, gamma.data_ptr(), out.data_ptr(), gamma0.data_ptr(),
                                _arena(dev, nbytes, 'arhmm'), nbytes, _stream()), 'bn_arhmm_moments')
    return out, gamma0


def hmm_viterbi(ll, offsets, log_Ps, log_pi0):
    """The most likely state path of every trial over the float64 DEVICE table ``ll`` (n, K): an int32 device tensor
    (n,) (``bn_hmm_viterbi``); a tie goes to the lowest state.  Rows outside the trials read 0."""
    n, K = _ll_table('hmm_viterbi', ll)
    dev = ll.device
    log_Ps = _f64_operand('hmm_viterbi', 'log_Ps', log_Ps, (K, K), dev)
    log_pi0 = _f64_operand('hmm_viterbi', 'log_pi0', log_pi0, (K,), dev)
    offsets = _trial_offsets('hmm_viterbi', offsets, dev)
    S = int(offsets.numel()) - 1
    states = torch.zeros((n,), dtype=torch.int32, device=dev)
    lib = load()
    nbytes = lib.bn_hmm_viterbi_ws_bytes(n, S, K)
    if S:
        _check(lib.bn_hmm_viterbi(ll.data_ptr(), offsets.data_ptr(), S, K, n, log_Ps.data_ptr(), log_pi0.data_ptr(),
                                  states.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes, _stream()),
               'bn_hmm_viterbi')
    return states


def hmm_predictive(ll, offsets, log_Ps, log_pi0, out=None):
    """The causal state weights ``w_t = p(z_t | x_0 .. x_{t-1})`` of every trial over the float64 DEVICE table ``ll``
    (n, K): a float64 device tensor (n, K) (``bn_hmm_predictive``, csrc/arhmm.hip) -- ``hmm_forward_backward``'s
    forward sweep with one store a step.  Row t of ``ll`` does not reach ``w_t``; ``w_0 = exp(log_pi0)``.  Rows
    outside the trials are left as they are (zeros in a fresh ``out``)."""
    n, K = _ll_table('hmm_predictive', ll)
    dev = ll.device
    log_Ps = _f64_operand('hmm_predictive', 'log_Ps', log_Ps, (K, K), dev)
    log_pi0 = _f64_operand('hmm_predictive', 'log_pi0', log_pi0, (K,), dev)
    offsets = _trial_offsets('hmm_predictive', offsets, dev)
    S = int(offsets.numel()) - 1
    if out is None:
        out = torch.zeros((n, K), dtype=torch.float64, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (n, K) or out.device != dev \
            or not out.is_contiguous():
        raise ValueError('hmm_predictive: expected out float64 (%d, %d) on %s' % (n, K, dev))
    lib = load()
    nbytes = lib.bn_hmm_predictive_ws_bytes(n, S, K)
    if S:
        _check(lib.bn_hmm_predictive(ll.data_ptr(), offsets.data_ptr(), S, K, n, log_Ps.data_ptr(),
                                     log_pi0.data_ptr(), out.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes,
                                     _stream()), 'bn_hmm_predictive')
    return out


def arhmm_predict(table, offsets, W, weights, lags, out=None):
    """One-step-ahead predictions of an ARHMM on the fp32 DEVICE ``table`` (n, D): a float64 device tensor (n, D)
    (``bn_arhmm_predict``, csrc/arhmm.hip).  Row t >= lags of a trial gets
    ``sum_k weights[t, k] (b_k + sum_l A_k[l] x_{t-1-l})`` with ``W[k] = [b_k | A_k]`` float64 (K, D, 1 + lags D)
    (``models.arhmm.ARHMM.generative()[0]``; host arrays are uploaded) and ``weights`` float64 DEVICE (n, K); a row
    t < lags gets the row's own values.  Rows outside the trials are left as they are (zeros in a fresh ``out``)."""
    n, D, ld = _column_table('arhmm_predict', table)
    L = int(lags)
    if not torch.is_tensor(W) and np.ndim(W) != 3 or torch.is_tensor(W) and W.dim() != 3:
        raise ValueError('arhmm_predict: expected W float64 (K, D, 1 + lags D)')
    K = int(W.shape[0])
    check_arhmm_dims('arhmm_predict', D, L, K)
    dev = table.device
    W = _f64_operand('arhmm_predict', 'W', W, (K, D, 1 + L * D), dev)
    if not torch.is_tensor(weights) or weights.dim() != 2:
        raise ValueError('arhmm_predict: expected weights float64 (n, K) on the device')
    weights = _f64_operand('arhmm_predict', 'weights', weights, (n, K), dev)
    offsets = _trial_offsets('arhmm_predict', offsets, dev)
    S = int(offsets.numel()) - 1
    if out is None:
        out = torch.zeros((n, D), dtype=torch.float64, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (n, D) or out.device != dev \
            or not out.is_contiguous():
        raise ValueError('arhmm_predict: expected out float64 (%d, %d) on %s' % (n, D, dev))
    lib = load()
    nbytes = lib.bn_arhmm_predict_ws_bytes(n, S, D, L, K)
    if S:
        _check(lib.bn_arhmm_predict(table.data_ptr(), ld, offsets.data_ptr(), S, D, L, K, n, W.data_ptr(),
                                    weights.data_ptr(), out.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes,
                                    _stream()), 'bn_arhmm_predict')
    return out


ARHMM_MAX_HORIZONS = 32                                 # AR_FC_MAX_H


def check_arhmm_horizons(who, H):
    """ValueError unless ``H`` is a number of horizons the forecasts serve."""
    if isinstance(H, bool) or not isinstance(H, (int, np.integer)) or not 1 <= H <= ARHMM_MAX_HORIZONS:
        raise ValueError('%s: %r horizons (an int from 1 to %d is served)' % (who, H, ARHMM_MAX_HORIZONS))


def arhmm_forecast_sums(table, offsets, N, weights, lags, out=None):
    """The sums of the exact multi-step forecasts of an ARHMM on the fp32 DEVICE ``table`` (n, D): a float64 device
    tensor (H, S, D, 5) (``bn_arhmm_forecast_sums``, csrc/arhmm.hip).  Origin row t of a trial, ``t - beg >= max(lags,
    1)``, forecasts ``x_{t+h-1}`` as ``sum_k weights[t, k] N[h - 1, k] phi_t`` for every h with ``t + h - 1 < end``;
    over those pairs, per horizon, trial and dimension: the count, ``sum y``, ``sum y^2``, ``sum (y - xhat)^2`` and
    ``sum (y - x_{t-1})^2``.  ``N`` float64 (H, K, D, 1 + lags D) (``models.arhmm.ARHMM.forecast_maps``; host arrays
    are uploaded), ``weights`` float64 DEVICE (n, K).  The forecasts themselves never reach memory."""
    n, D, ld = _column_table('arhmm_forecast_sums', table)
    L = int(lags)
    if not torch.is_tensor(N) and np.ndim(N) != 4 or torch.is_tensor(N) and N.dim() != 4:
        raise ValueError('arhmm_forecast_sums: expected N float64 (H, K, D, 1 + lags D)')
    H, K = int(N.shape[0]), int(N.shape[1])
    check_arhmm_dims('arhmm_forecast_sums', D, L, K)
    check_arhmm_horizons('arhmm_forecast_sums', H)
    dev = table.device
    N = _f64_operand('arhmm_forecast_sums', 'N', N, (H, K, D, 1 + L * D), dev)
    if not torch.is_tensor(weights) or weights.dim() != 2:
        raise ValueError('arhmm_forecast_sums: expected weights float64 (n, K) on the device')
    weights = _f64_operand('arhmm_forecast_sums', 'weights', weights, (n, K), dev)
    offsets = _trial_offsets('arhmm_forecast_sums', offsets, dev)
    S = int(offsets.numel()) - 1
    if out is None:
        out = torch.zeros((H, S, D, 5), dtype=torch.float64, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (H, S, D, 5) \
            or out.device != dev or not out.is_contiguous():
        raise ValueError('arhmm_forecast_sums: expected out float64 (%d, %d, %d, 5) on %s' % (H, S, D, dev))
    lib = load()
    nbytes = lib.bn_arhmm_forecast_sums_ws_bytes(n, S, D, L, K, H)
    if S:
        _check(lib.bn_arhmm_forecast_sums(table.data_ptr(), ld, offsets.data_ptr(), S, D, L, K, H, n, N.data_ptr(),
                                          weights.data_ptr(), out.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes,
                                          _stream()), 'bn_arhmm_forecast_sums')
    return out


# A grid of models on one table (bn_arhmm_grid_*, bn_hmm_grid_forward_backward): AR_GRID_MAX_KT, AR_GRID_MAX_M.  The
# row blocks of bn_arhmm_grid_moments are _arhmm_moments_plan's with K = KT (held against the workspace query in
# tests/test_arhmm_grid_cpu.py)
ARHMM_GRID_MAX_STATES, ARHMM_GRID_MAX_MODELS = 512, 512
_HMM_GRID_CLASSES = (4, 8, 16, 32)


def check_arhmm_grid_states(who, Ks):
    """ValueError unless ``Ks`` are the state counts of a grid the kernels serve: 1 to 512 models of 1 to 32 states,
    512 states together.  -> ``(koff, xoff)``, int32 (M + 1): the prefix sums of ``K_m`` and of ``K_m^2``."""
    Ks = [int(k) for k in Ks]
    if not 1 <= len(Ks) <= ARHMM_GRID_MAX_MODELS:
        raise ValueError('%s: %d models (1 to %d are served)' % (who, len(Ks), ARHMM_GRID_MAX_MODELS))
    for k in Ks:
        if not 1 <= k <= ARHMM_MAX_K:
            raise ValueError('%s: %d states (1 to %d are served)' % (who, k, ARHMM_MAX_K))
    if sum(Ks) > ARHMM_GRID_MAX_STATES:
        raise ValueError('%s: %d states in all models together (1 to %d are served)'
                         % (who, sum(Ks), ARHMM_GRID_MAX_STATES))
    return (np.concatenate(([0], np.cumsum(Ks))).astype(np.int32),
            np.concatenate(([0], np.cumsum([k * k for k in Ks]))).astype(np.int32))


def check_arhmm_grid_dims(who, D, L, KT):
    """ValueError unless (D, L) are served and ``KT`` states together are at most 512."""
    check_arhmm_dims(who, D, L, 1)
    if not 1 <= KT <= ARHMM_GRID_MAX_STATES:
        raise ValueError('%s: %d states in all models together (1 to %d are served)'
                         % (who, KT, ARHMM_GRID_MAX_STATES))


def hmm_grid_plan(Ks):
    """Where ``bn_hmm_grid_forward_backward`` puts the models of state counts ``Ks``: ``(cls, wave, slot)``, int32
    arrays (M,).  ``cls[m]`` is the smallest of 4, 8, 16, 32 that holds ``K_m``; the models of a class keep their
    order and fill waves of ``64 / cls`` slots one after the other, ``wave[m]`` counted within the class.  Pure host
    code: the launcher and the tests go by it."""
    cls = np.asarray([next((c for c in _HMM_GRID_CLASSES if int(k) <= c), 0) for k in Ks], dtype=np.int32)
    if len(cls) and (cls.min() < 1 or min(int(k) for k in Ks) < 1):
        raise ValueError('hmm_grid_plan: state counts %s (1 to %d are served)' % (list(Ks), ARHMM_MAX_K))
    wave, slot = np.zeros_like(cls), np.zeros_like(cls)
    for c in _HMM_GRID_CLASSES:
        pos = np.arange(int(np.sum(cls == c)), dtype=np.int32)
        wave[cls == c], slot[cls == c] = pos // (64 // c), pos % (64 // c)
    return cls, wave, slot


def _hmm_grid_order(Ks):
    """``(order, counts)`` for the launch from the plan: the models class by class, and the models a class."""
    cls, wave, slot = hmm_grid_plan(Ks)
    order, counts = [], []
    for c in _HMM_GRID_CLASSES:
        members = np.flatnonzero(cls == c)
        order.extend(members[np.argsort(wave[members] * (64 // c) + slot[members], kind='stable')].tolist())
        counts.append(len(members))
    return np.asarray(order, dtype=np.int32), counts


def arhmm_grid_loglik(table, offsets, G, cst, lags, shift=None, out=None):
    """``arhmm_loglik`` for the states of a grid of models side by side: ``G`` (KT, D, P) and ``cst`` (KT) with
    KT up to 512 -> float64 (n, KT) (``bn_arhmm_grid_loglik``)."""
    who = 'arhmm_grid_loglik'
    n, D, ld = _column_table(who, table)
    L = int(lags)
    if not torch.is_tensor(G) and np.ndim(G) != 3 or torch.is_tensor(G) and G.dim() != 3:
        raise ValueError('%s: expected G float64 (KT, D, P)' % who)
    KT = int(G.shape[0])
    check_arhmm_grid_dims(who, D, L, KT)
    P = 1 + (L + 1) * D
    dev = table.device
    G = _f64_operand(who, 'G', G, (KT, D, P), dev)
    cst = _f64_operand(who, 'cst', cst, (KT,), dev)
    shift = _f64_operand(who, 'shift', shift, (D,), dev, allow_none=True)
    offsets = _trial_offsets(who, offsets, dev)
    S = int(offsets.numel()) - 1
    if out is None:
        out = torch.zeros((n, KT), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n, KT) or out.device != dev or not out.is_contiguous():
        raise ValueError('%s: expected out float64 (%d, %d) on %s' % (who, n, KT, dev))
    lib = load()
    nbytes = lib.bn_arhmm_grid_loglik_ws_bytes(n, S, D, L, KT)
    if S:
        _check(lib.bn_arhmm_grid_loglik(table.data_ptr(), ld, None if shift is None else shift.data_ptr(),
                                        offsets.data_ptr(), S, D, L, KT, n, G.data_ptr(), cst.data_ptr(),
                                        out.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes, _stream()),
               'bn_arhmm_grid_loglik')
    return out


def arhmm_grid_moments(table, offsets, gamma, lags, shift=None):
    """``arhmm_moments`` for the states of a grid of models side by side: ``gamma`` float64 DEVICE (n, KT) with KT
    up to 512 -> ``(out, gamma0)``, (KT, P, P) and (KT,) (``bn_arhmm_grid_moments``)."""
    who = 'arhmm_grid_moments'
    n, D, ld = _column_table(who, table)
    L = int(lags)
    if not torch.is_tensor(gamma) or gamma.dim() != 2:
        raise ValueError('%s: expected gamma float64 (n, KT) on the device' % who)
    KT = int(gamma.shape[1])
    check_arhmm_grid_dims(who, D, L, KT)
    dev = table.device
    gamma = _f64_operand(who, 'gamma', gamma, (n, KT), dev)
    shift = _f64_operand(who, 'shift', shift, (D,), dev, allow_none=True)
    offsets = _trial_offsets(who, offsets, dev)
    S = int(offsets.numel()) - 1
    P = 1 + (L + 1) * D
    out = torch.empty((KT, P, P), dtype=torch.float64, device=dev)
    gamma0 = torch.empty((KT,), dtype=torch.float64, device=dev)
    if not S:
        return out.zero_(), gamma0.zero_()
    lib = load()
    nbytes = lib.bn_arhmm_grid_moments_ws_bytes(n, S, D, L, KT)
    _check(lib.bn_arhmm_grid_moments(table.data_ptr(), ld, None if shift is None else shift.data_ptr(),
                                     offsets.data_ptr(), S, D, L, KT, n, gamma.data_ptr(), out.data_ptr(),
                                     gamma0.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes, _stream()),
           'bn_arhmm_grid_moments')
    return out, gamma0


def hmm_grid_forward_backward(ll, offsets, Ks, log_Ps, log_pi0, want_posteriors=True, gamma=None, xi=None):
    """Forward-backward of every (trial, model) of a grid over the float64 DEVICE table ``ll`` (n, KT), the models'
    states side by side (``bn_hmm_grid_forward_backward``): ``(gamma, xi, loglik)``, float64 device tensors (n, KT),
    (S, XT) and (M, S).  ``Ks``: the M state counts, KT = sum K_m, XT = sum K_m^2; ``log_Ps``: (XT,), the models'
    (K_m, K_m) matrices row-major one after the other; ``log_pi0``: (KT,).  Model m has the columns
    ``sum(Ks[:m]) ..`` of ``gamma`` and ``sum(K^2 for K in Ks[:m]) ..`` of ``xi``.  ``want_posteriors=False``: the
    forward sweep alone, ``(None, None, loglik)``."""
    who = 'hmm_grid_forward_backward'
    koff, xoff = check_arhmm_grid_states(who, Ks)
    M, KT, XT = len(koff) - 1, int(koff[-1]), int(xoff[-1])
    if not torch.is_tensor(ll) or ll.dim() != 2 or ll.dtype != torch.float64 or int(ll.shape[1]) != KT:
        raise ValueError('%s: expected ll float64 (n, %d), got %s'
                         % (who, KT, (ll.dtype, tuple(ll.shape)) if torch.is_tensor(ll) else type(ll).__name__))
    if not ll.is_cuda:
        raise ValueError('%s: expected ll on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, ll.device))
    if not ll.is_contiguous():
        raise ValueError('%s: ll must be contiguous, got strides %s' % (who, tuple(ll.stride())))
    n, dev = int(ll.shape[0]), ll.device
    log_Ps = _f64_operand(who, 'log_Ps', log_Ps, (XT,), dev)
    log_pi0 = _f64_operand(who, 'log_pi0', log_pi0, (KT,), dev)
    offsets = _trial_offsets(who, offsets, dev)
    S = int(offsets.numel()) - 1
    loglik = torch.empty((M, S), dtype=torch.float64, device=dev)
    want = 1 if want_posteriors else 0
    if want:
        if gamma is None:
            gamma = torch.zeros((n, KT), dtype=torch.float64, device=dev)
        if xi is None:
            xi = torch.empty((S, XT), dtype=torch.float64, device=dev)
        for name, t, shape in (('gamma', gamma, (n, KT)), ('xi', xi, (S, XT))):
            if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError('%s: expected %s float64 %s on %s' % (who, name, shape, dev))
    order, counts = _hmm_grid_order(Ks)
    tables = torch.from_numpy(np.concatenate([koff, xoff, order])).to(dev)          # one upload
    lib = load()
    nbytes = lib.bn_hmm_grid_forward_backward_ws_bytes(n, S, M, KT, XT)
    if S:
        _check(lib.bn_hmm_grid_forward_backward(ll.data_ptr(), offsets.data_ptr(), S, M, KT, XT, n,
                                                tables.data_ptr(), tables[M + 1:].data_ptr(),
                                                tables[2 * M + 2:].data_ptr(), counts[0], counts[1], counts[2],
                                                counts[3], log_Ps.data_ptr(), log_pi0.data_ptr(), want,
                                                gamma.data_ptr() if want else None, xi.data_ptr() if want else None,
                                                loglik.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes, _stream()),
               'bn_hmm_grid_forward_backward')
    return (gamma, xi, loglik) if want else (None, None, loglik)


def hmm_grid_viterbi_ws_bytes(n, S, Ks):
    """``bn_hmm_grid_viterbi_ws_bytes`` restated: the int32 offsets padded to 16 bytes and one uint8 back-pointer a
    (row, state column), padded to 16 bytes (held against the query in tests/test_arhmm_grid_states_cpu.py)."""
    pad16 = lambda b: (int(b) + 15) & ~15
    return pad16((int(S) + 1) * 4) + pad16(int(n) * int(sum(int(k) for k in Ks)))


def hmm_grid_viterbi(ll, offsets, Ks, log_Ps, log_pi0, out=None):
    """The most likely state path of every (trial, model) of a grid over the float64 DEVICE table ``ll`` (n, KT), the
    models' states side by side (``bn_hmm_grid_viterbi``): an int32 device tensor (M, n), row m the path of model m
    with the integers ``hmm_viterbi`` gives on that model's own columns; a tie goes to the lowest state.  ``Ks``,
    ``log_Ps`` (XT,) and ``log_pi0`` (KT,) as ``hmm_grid_forward_backward`` takes them.  Rows outside the trials are
    not written: they read 0 in a fresh output and are left as they are in ``out`` (int32 (M, n) on the device)."""
    who = 'hmm_grid_viterbi'
    koff, xoff = check_arhmm_grid_states(who, Ks)
    M, KT, XT = len(koff) - 1, int(koff[-1]), int(xoff[-1])
    if not torch.is_tensor(ll) or ll.dim() != 2 or ll.dtype != torch.float64 or int(ll.shape[1]) != KT:
        raise ValueError('%s: expected ll float64 (n, %d), got %s'
                         % (who, KT, (ll.dtype, tuple(ll.shape)) if torch.is_tensor(ll) else type(ll).__name__))
    if not ll.is_cuda:
        raise ValueError('%s: expected ll on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, ll.device))
    if not ll.is_contiguous():
        raise ValueError('%s: ll must be contiguous, got strides %s' % (who, tuple(ll.stride())))
    n, dev = int(ll.shape[0]), ll.device
    log_Ps = _f64_operand(who, 'log_Ps', log_Ps, (XT,), dev)
    log_pi0 = _f64_operand(who, 'log_pi0', log_pi0, (KT,), dev)
    offsets = _trial_offsets(who, offsets, dev)
    S = int(offsets.numel()) - 1
    if out is None:
        out = torch.zeros((M, n), dtype=torch.int32, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (M, n) or out.device != dev \
            or not out.is_contiguous():
        raise ValueError('%s: expected out int32 (%d, %d) on %s' % (who, M, n, dev))
    order, counts = _hmm_grid_order(Ks)
    tables = torch.from_numpy(np.concatenate([koff, xoff, order])).to(dev)          # one upload
    lib = load()
    nbytes = lib.bn_hmm_grid_viterbi_ws_bytes(n, S, M, KT, XT)
    if S:
        _check(lib.bn_hmm_grid_viterbi(ll.data_ptr(), offsets.data_ptr(), S, M, KT, XT, n, tables.data_ptr(),
                                       tables[M + 1:].data_ptr(), tables[2 * M + 2:].data_ptr(), counts[0], counts[1],
                                       counts[2], counts[3], log_Ps.data_ptr(), log_pi0.data_ptr(), out.data_ptr(),
                                       _arena(dev, nbytes, 'arhmm'), nbytes, _stream()), 'bn_hmm_grid_viterbi')
    return out


# csrc/state_runs.hip's partition, restated for the tests that have to name tile boundaries and the row count at which
# the scan over the tiles' counts takes a second step: SR_TILE rows a workgroup (held against bn_state_runs_ws_bytes
# in tests/test_state_runs_cpu.py), SR_SCAN counts a step of the scan
STATE_RUNS_TILE, STATE_RUNS_SCAN = 1024, 1024


def state_runs(states, offsets, K):
    """The runs of the int32 DEVICE state table ``states`` (n,) -- ``hmm_viterbi``'s output -- inside the trials
    ``offsets`` (int64 (S + 1), a host array is uploaded): ``(runs, frames, trans)``, device tensors
    (``bn_state_runs``, csrc/state_runs.hip).  ``runs`` int32 (R, 4): one row ``(trial, beg, end, state)`` per maximal
    stretch of equal states inside one trial, ``beg`` and ``end`` relative to the trial and ``end`` exclusive, in the
    order of the table.  ``frames`` int64 (K): the rows in trials per state.  ``trans`` int64 (K, K): the pairs
    ``(states[i - 1], states[i])`` inside one trial, self-pairs included.  Rows outside the trials are not read.  A
    state outside [0, K) on a row in a trial is a ValueError that names how many there are.  One synchronisation
    (two int64 come back: R and that count).  ``S == 0`` gives empty runs and zeros."""
    who = 'state_runs'
    if not torch.is_tensor(states) or states.dim() != 1 or states.dtype != torch.int32:
        raise ValueError('%s: expected states int32 (n,), got %s'
                         % (who, (states.dtype, tuple(states.shape)) if torch.is_tensor(states)
                            else type(states).__name__))
    if not states.is_cuda:
        raise ValueError('%s: expected states on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, states.device))
    if not states.is_contiguous():
        raise ValueError('%s: states must be contiguous, got strides %s' % (who, tuple(states.stride())))
    K = int(K)
    if not 1 <= K <= ARHMM_MAX_K:
        raise ValueError('%s: %d states (1 to %d are served)' % (who, K, ARHMM_MAX_K))
    dev = states.device
    n = int(states.shape[0])
    offsets = _trial_offsets(who, offsets, dev)
    S = int(offsets.numel()) - 1
    # frames (K), trans (K, K), n_runs and bad in one tensor: one transfer tells R and bad
    stats = torch.zeros((K + K * K + 2,), dtype=torch.int64, device=dev)
    frames, trans = stats[:K], stats[K:K + K * K].view(K, K)
    if not S or not n:
        return torch.empty((0, 4), dtype=torch.int32, device=dev), frames, trans
    runs = torch.empty((n, 4), dtype=torch.int32, device=dev)
    lib = load()
    nbytes = lib.bn_state_runs_ws_bytes(n, S, K)
    at = stats.data_ptr()
    _check(lib.bn_state_runs(states.data_ptr(), offsets.data_ptr(), S, K, n, runs.data_ptr(), n, at, at + 8 * K,
                             at + 8 * (K + K * K), at + 8 * (K + K * K + 1), _arena(dev, nbytes, 'state_runs'), nbytes,
                             _stream()), 'bn_state_runs')
    R, bad = (int(v) for v in stats[K + K * K:].cpu())
    if bad:
        raise ValueError('%s: %d rows in trials hold a state outside [0, %d)' % (who, bad, K))
    return (runs if R == n else runs[:R].clone()), frames, trans


# state_runs_grid: bytes of run buffers (16 a (model, row)) that are alive at once at most
STATE_RUNS_GRID_BYTES = 1 << 30


def state_runs_grid(states, offsets, Ks):
    """``state_runs`` for every row of the int32 DEVICE table ``states`` (M, n) -- ``hmm_grid_viterbi``'s output --
    with the state counts ``Ks``: a list of M triples ``(runs, frames, trans)`` as ``state_runs`` defines them, HOST
    arrays int32 (R_m, 4), int64 (K_m) and int64 (K_m, K_m).  The ``bn_state_runs`` launches of the models follow
    each other on the stream with no synchronisation between them; the ``K + K^2 + 2`` int64 statistics of all models
    come back in ONE transfer and the runs, trimmed on the device to the counts that transfer told, in one more.  The
    models are taken in chunks whose run buffers (16 bytes a (model, row)) stay within 1 GiB -- one chunk, so two
    transfers, up to ``2^26 / n`` models; every further chunk costs two more.  A model with a state outside
    [0, K_m) on a row in a trial is ``state_runs``' ValueError with the model named."""
    who = 'state_runs_grid'
    if not torch.is_tensor(states) or states.dim() != 2 or states.dtype != torch.int32:
        raise ValueError('%s: expected states int32 (M, n), got %s'
                         % (who, (states.dtype, tuple(states.shape)) if torch.is_tensor(states)
                            else type(states).__name__))
    if not states.is_cuda:
        raise ValueError('%s: expected states on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, states.device))
    if not states.is_contiguous():
        raise ValueError('%s: states must be contiguous, got strides %s' % (who, tuple(states.stride())))
    Ks = [int(k) for k in Ks]
    M, n = (int(v) for v in states.shape)
    if len(Ks) != M or not M:
        raise ValueError('%s: %d state counts for %d models' % (who, len(Ks), M))
    for k in Ks:
        if not 1 <= k <= ARHMM_MAX_K:
            raise ValueError('%s: %d states (1 to %d are served)' % (who, k, ARHMM_MAX_K))
    dev = states.device
    offsets = _trial_offsets(who, offsets, dev)
    S = int(offsets.numel()) - 1
    if not S or not n:
        return [(np.zeros((0, 4), dtype=np.int32), np.zeros((k,), dtype=np.int64), np.zeros((k, k), dtype=np.int64))
                for k in Ks]
    lib = load()
    per = max(1, STATE_RUNS_GRID_BYTES // (16 * n))
    out = []
    for m0 in range(0, M, per):
        ks = Ks[m0:m0 + per]
        so = np.concatenate(([0], np.cumsum([k + k * k + 2 for k in ks])))
        stats = torch.zeros((int(so[-1]),), dtype=torch.int64, device=dev)
        runs = torch.empty((len(ks), n, 4), dtype=torch.int32, device=dev)
        for i, k in enumerate(ks):
            nbytes = lib.bn_state_runs_ws_bytes(n, S, k)
            at = stats.data_ptr() + 8 * int(so[i])
            _check(lib.bn_state_runs(states[m0 + i].data_ptr(), offsets.data_ptr(), S, k, n, runs[i].data_ptr(), n,
                                     at, at + 8 * k, at + 8 * (k + k * k), at + 8 * (k + k * k + 1),
                                     _arena(dev, nbytes, 'state_runs'), nbytes, _stream()), 'bn_state_runs')
        host = stats.cpu().numpy()                                                  # the chunk's first transfer
        Rs = []
        for i, k in enumerate(ks):
            R, bad = (int(v) for v in host[so[i] + k + k * k:so[i + 1]])
            if bad:
                raise ValueError('%s: model %d: %d rows in trials hold a state outside [0, %d)'
                                 % (who, m0 + i, bad, k))
            Rs.append(R)
        trimmed = torch.cat([runs[i, :R] for i, R in enumerate(Rs)]).cpu().numpy()   # ... and its second
        ro = np.concatenate(([0], np.cumsum(Rs)))
        for i, k in enumerate(ks):
            st = host[so[i]:so[i + 1]]
            out.append((trimmed[ro[i]:ro[i + 1]].copy(), st[:k].copy(), st[k:k + k * k].reshape(k, k).copy()))
        del runs
    return out


def arhmm_sample(W, C, cdf0, cdf, offsets, eps, u=None, states=None, init=None, x=None, states_out=None):
    """Latents and states drawn from an ARHMM's generative process with the noise the caller brings
    (``bn_arhmm_sample``): ``(x, states)``, float64 (n, D) and int32 (n) DEVICE tensors.  ``W`` (K, D, 1 + L D),
    ``C`` (K, D, D), ``cdf0`` (K) and ``cdf`` (K, K): ``models.arhmm.ARHMM.generative``, float64, host arrays are
    uploaded.  ``eps``: float64 DEVICE (n, D) standard normals.  Exactly one of ``u``, float64 DEVICE (n,) uniforms in
    [0, 1) -- the states are sampled -- and ``states``, int32 DEVICE (n,) -- the states are given, and one device
    reduction checks their range over the trials' rows first: a state outside [0, K) is a ValueError and nothing is
    launched.  ``init``: None or an fp32 DEVICE table (n, D) (a row stride is served) whose rows are a trial's first L
    rows; without it those are ``eps``.  Rows outside the trials are left as they are (zeros in fresh outputs; ``x``
    and ``states_out`` may be given).  No random number is drawn here: the same operands give the same bits."""
    who = 'arhmm_sample'
    if not torch.is_tensor(eps) or eps.dim() != 2 or eps.dtype != torch.float64:
        raise ValueError('%s: expected eps float64 (n, D) on the device, got %s'
                         % (who, (eps.dtype, tuple(eps.shape)) if torch.is_tensor(eps) else type(eps).__name__))
    if not eps.is_cuda:
        raise ValueError('%s: expected eps on the GPU, got device %s (the HIP path has no CPU fallback)'
                         % (who, eps.device))
    n, D = (int(v) for v in eps.shape)
    if not torch.is_tensor(W) and np.ndim(W) != 3 or torch.is_tensor(W) and W.dim() != 3:
        raise ValueError('%s: expected W float64 (K, D, 1 + L D)' % who)
    K, cols = int(W.shape[0]), int(W.shape[2])
    if int(W.shape[1]) != D or (cols - 1) % D:
        raise ValueError('%s: W %s does not go with eps (n, %d)' % (who, tuple(W.shape), D))
    L = (cols - 1) // D
    check_arhmm_dims(who, D, L, K)
    if (u is None) == (states is None):
        raise ValueError('%s: exactly one of u (the states are sampled) and states (they are given)' % who)
    dev = eps.device
    W = _f64_operand(who, 'W', W, (K, D, cols), dev)
    C = _f64_operand(who, 'C', C, (K, D, D), dev)
    cdf0 = _f64_operand(who, 'cdf0', cdf0, (K,), dev)
    cdf = _f64_operand(who, 'cdf', cdf, (K, K), dev)
    eps = _f64_operand(who, 'eps', eps, (n, D), dev)
    u = _f64_operand(who, 'u', u, (n,), dev, allow_none=True)
    offsets = _trial_offsets(who, offsets, dev)
    S = int(offsets.numel()) - 1
    if states is not None:
        if not torch.is_tensor(states) or states.dtype != torch.int32 or tuple(states.shape) != (n,) \
                or states.device != dev:
            raise ValueError('%s: expected states int32 (%d,) on %s' % (who, n, dev))
        states = states.contiguous()
    ld_init = D
    if init is not None:
        ni, di, ld_init = _column_table(who, init)
        if (ni, di) != (n, D) or init.device != dev:
            raise ValueError('%s: expected init float32 (%d, %d) on %s, got %s on %s'
                             % (who, n, D, dev, tuple(init.shape), init.device))
    if x is None:
        x = torch.zeros((n, D), dtype=torch.float64, device=dev)
    elif x.dtype != torch.float64 or tuple(x.shape) != (n, D) or x.device != dev or not x.is_contiguous():
        raise ValueError('%s: expected x float64 (%d, %d) on %s' % (who, n, D, dev))
    if states_out is None:
        states_out = torch.zeros((n,), dtype=torch.int32, device=dev)
    elif states_out.dtype != torch.int32 or tuple(states_out.shape) != (n,) or states_out.device != dev \
            or not states_out.is_contiguous():
        raise ValueError('%s: expected states_out int32 (%d,) on %s' % (who, n, dev))
    if not S or not n:
        return x, states_out
    if states is not None:
        # the rows the launch would read: [e[0], e[S]) of the offsets made safe (clamped, non-decreasing)
        e = torch.cummax(offsets.clamp(0, n), dim=0)[0]
        lo, hi = int(e[0]), int(e[-1])
        if hi > lo:
            mn, mx = torch.aminmax(states[lo:hi])
            mn, mx = int(mn), int(mx)
            if mn < 0 or mx >= K:
                raise ValueError('%s: states from %d to %d, the model has the states 0 to %d' % (who, mn, mx, K - 1))
    lib = load()
    nbytes = lib.bn_arhmm_sample_ws_bytes(n, S, D, L, K)
    _check(lib.bn_arhmm_sample(W.data_ptr(), C.data_ptr(), cdf0.data_ptr(), cdf.data_ptr(), offsets.data_ptr(), S, D,
                               L, K, n, eps.data_ptr(), None if u is None else u.data_ptr(),
                               None if states is None else states.data_ptr(),
                               None if init is None else init.data_ptr(), ld_init, x.data_ptr(),
                               states_out.data_ptr(), _arena(dev, nbytes, 'arhmm'), nbytes, _stream()),
           'bn_arhmm_sample')
    return x, states_out


def recon_panels_u8(orig, recon, mask=None, show_orig=True, out=None, row=0, n_rows=1):
    """Frames ``orig`` and their reconstruction ``recon``, both (N, C, H, W) and each fp32 unit floats or uint8 grey
    levels (value / 255), -> row ``row`` of the uint8 DEVICE movie (N, n_rows * H, 3 * C * W): per frame and image row
    three panels with the channels side by side, the original (times ``mask``; black without ``show_orig``), the
    reconstruction and the residual ``0.5 + (orig * mask - recon)``, each step in fp32 and quantised by
    ``unit_float_to_u8``'s rule.  ``mask``: None, fp32 (N, C, H, W) or one fp32 (C, H, W) for all frames; it masks the
    original alone.  ``out``: the movie to fill (its other rows are left alone), made here when None.  Dtypes,
    shapes, devices and contiguity are checked before any call (``ValueError``).  One pass on the current stream
    (csrc/recon_panels.hip)."""
    who = 'recon_panels_u8'
    for name, t in (('orig', orig), ('recon', recon)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError('%s: expected %s (N, C, H, W), got %s'
                             % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError('%s: %s must be uint8 or float32, got %s' % (who, name, t.dtype))
    if tuple(recon.shape) != tuple(orig.shape):
        raise ValueError('%s: orig %s and recon %s must share a shape' % (who, tuple(orig.shape), tuple(recon.shape)))
    N, C, H, W = (int(v) for v in orig.shape)
    if min(C, H, W) < 1:
        raise ValueError('%s: frames of %d x %d x %d pixels' % (who, C, H, W))
    per_frame = False
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype != torch.float32:
            raise ValueError('%s: the mask must be a float32 tensor, got %s'
                             % (who, mask.dtype if torch.is_tensor(mask) else type(mask).__name__))
        if tuple(mask.shape) not in ((C, H, W), (N, C, H, W)):
            raise ValueError('%s: expected a mask %s or %s, got %s'
                             % (who, (C, H, W), (N, C, H, W), tuple(mask.shape)))
        per_frame = mask.dim() == 4
    row, n_rows = int(row), int(n_rows)
    if n_rows < 1 or not 0 <= row < n_rows:
        raise ValueError('%s: row %d of a movie of %d rows' % (who, row, n_rows))
    shape = (N, n_rows * H, 3 * C * W)
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != shape):
        raise ValueError('%s: expected out uint8 %s, got %s'
                         % (who, shape, '%s %s' % (out.dtype, tuple(out.shape)) if torch.is_tensor(out)
                            else type(out).__name__))
    named = [('orig', orig), ('recon', recon), ('mask', mask), ('out', out)]
    for name, t in named:
        if t is not None and not t.is_contiguous():
            raise ValueError('%s: %s must be contiguous' % (who, name))
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise ValueError('%s: expected %s on the GPU, got device %s (the HIP path has no CPU fallback)'
                             % (who, name, t.device))
    for name, t in named[1:]:
        if t is not None and t.device != orig.device:
            raise ValueError('%s: orig is on %s, %s on %s' % (who, orig.device, name, t.device))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=orig.device)
    strip = 3 * C * H * W
    _check(load().bn_recon_panels_u8(
        orig.data_ptr(), int(orig.dtype == torch.uint8), recon.data_ptr(), int(recon.dtype == torch.uint8),
        None if mask is None else mask.data_ptr(), int(per_frame), N, C, H, W, int(bool(show_orig)),
        out.data_ptr() + row * strip, n_rows * strip, _stream()), 'bn_recon_panels_u8')
    return out


def prof_select(family, C=0, K=0, nth=None):
    """Time the calls of one family (and channel pair); ``nth``: only the nth matching call."""
    if nth is None:
        _check(load().bn_prof_select(family, C, K), 'bn_prof_select')
    else:
        _check(load().bn_prof_select_nth(family, C, K, int(nth)), 'bn_prof_select_nth')


def prof_read():
    ms, n = ctypes.c_double(0.0), ctypes.c_long(0)
    _check(load().bn_prof_read(ctypes.byref(ms), ctypes.byref(n)), 'bn_prof_read')
    name = load().bn_prof_kernel_name()
    return ms.value, n.value, (name.decode() if name else '')


def prof_set_bracket(on):
    return load().bn_prof_set_bracket(1 if on else 0)


def prof_read_main():
    """(ms, launches) of the main kernels of the profiled calls (dispatch-attached events)."""
    ms, n = ctypes.c_double(0.0), ctypes.c_long(0)
    _check(load().bn_prof_read_main(ctypes.byref(ms), ctypes.byref(n)), 'bn_prof_read_main')
    return ms.value, n.value


# ------------------------------------------------------------------------------------------
# max pooling with indices / unpooling ('max_pooling' architectures)
# ------------------------------------------------------------------------------------------
def maxpool2d_fwd(x, k, stride, pad, out_hw):
    """x (N,C,H,W) -> (y (N,C,Ho,Wo), idx int32 (N,C,Ho,Wo)); pad = (top, left)."""
    N, C, H, W = x.shape
    Ho, Wo = out_hw
    y = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    idx = torch.empty((N, C, Ho, Wo), dtype=torch.int32, device=x.device)
    _check(load().bn_maxpool2d_fwd(_ptr(x, 'x'), _ptr(y, 'y'), _ptr(idx, 'idx', torch.int32),
                                   N * C, H, W, Ho, Wo, k, stride, pad[0], pad[1], _stream()),
           'bn_maxpool2d_fwd')
    return y, idx


def maxpool2d_act_fwd(x, act, slope):
    """2x2 / stride-2 pooling + activation in one pass -> (y, idx) or None where the kernel does not apply."""
    N, C, H, W = x.shape
    if H % 2 or W % 4:
        return None
    y = torch.empty((N, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    idx = torch.empty((N, C, H // 2, W // 2), dtype=torch.int32, device=x.device)
    rc = load().bn_maxpool2d_act_fwd(_ptr(x, 'x'), _ptr(y, 'y'), _ptr(idx, 'idx', torch.int32), N * C, H, W,
                                     int(act), float(slope), _stream())
    return (y, idx) if rc == 0 else None


def conv2d_pool_act_ok(geom):
    """Whether bn_conv2d_pool2_act_fwd serves this layer (host-side query)."""
    return bool(load().bn_conv2d_pool2_act_ok(*geom))


def conv2d_pool_bwd_weight_ws_bytes(geom):
    """Scratch of bn_conv2d_pool2_bwd_weight; 0 where the pooled-side weight gradient is not served."""
    return int(load().bn_conv2d_pool2_bwd_weight_ws_bytes(*geom))


def conv2d_pool_bwd_weight(x, dy, y, idx, dw, db, geom, act, slope, accumulate):
    """dw (+)=, db (+)= of a layer run by conv2d_pool_act_fwd from the pooled gradient `dy`, its saved output `y` and the
    winners `idx` (bn_conv2d_pool2_bwd_weight)."""
    nbytes = conv2d_pool_bwd_weight_ws_bytes(geom)
    if nbytes == 0:
        raise HipLibraryError('conv2d_pool_bwd_weight: geometry not served')
    ws = _arena(x.device, nbytes)
    _check(load().bn_conv2d_pool2_bwd_weight(
        _ptr(x, 'x'), _ptr(dy, 'dy'), _ptr(y, 'y'), _ptr(idx, 'idx', torch.int32), _ptr(dw, 'dw'),
        _ptr(db, 'db', allow_none=True), *geom, int(act), float(slope), int(accumulate), ws, nbytes, _stream()),
        'bn_conv2d_pool2_bwd_weight')


def conv2d_pool_act_fwd(x, w, b, geom, act, slope):
    """Conv2d + 2x2 / stride-2 max pooling + activation in one kernel -> (y, idx) or None where it is not served."""
    N, C, H, W, K, R, S, st, pt, pl, P, Q = geom
    if P % 2 or Q % 4 or x.dtype != torch.float32:
        return None
    y = torch.empty((N, K, P // 2, Q // 2), dtype=torch.float32, device=x.device)
    idx = torch.empty((N, K, P // 2, Q // 2), dtype=torch.int32, device=x.device)
    rc = load().bn_conv2d_pool2_act_fwd(_ptr(x, 'x'), _ptr(w, 'w'), _ptr(b, 'b', allow_none=True), _ptr(y, 'y'),
                                        _ptr(idx, 'idx', torch.int32), *geom, int(act), float(slope), _stream())
    if rc == -2:                      # BN_E_SHAPE: not served
        return None
    _check(rc, 'bn_conv2d_pool2_act_fwd')
    return y, idx


def maxpool2d_act_bwd(dy, y, idx, in_hw, act, slope):
    N, C, Ho, Wo = dy.shape
    H, W = in_hw
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    _check(load().bn_maxpool2d_act_bwd(_ptr(dy, 'dy'), _ptr(y, 'y'), _ptr(idx, 'idx', torch.int32), _ptr(dx, 'dx'),
                                       N * C, H, W, int(act), float(slope), _stream()), 'bn_maxpool2d_act_bwd')
    return dx


def maxpool2d_bwd(dy, idx, in_hw, k, stride, pad):
    N, C, Ho, Wo = dy.shape
    H, W = in_hw
    dx = torch.empty((N, C, H, W), dtype=torch.float32, device=dy.device)
    _check(load().bn_maxpool2d_bwd(_ptr(dy, 'dy'), _ptr(idx, 'idx', torch.int32), _ptr(dx, 'dx'),
                                   N * C, H, W, Ho, Wo, k, stride, pad[0], pad[1], _stream()),
           'bn_maxpool2d_bwd')
    return dx


def maxunpool2d_fwd(x, idx, out_hw, own_window=False):
    """``own_window``: idx are the indices of the 2x2 / stride-2 pooling this layer undoes (each inside its own
    window): the one-pass kernel where the maps qualify."""
    N, C, Hi, Wi = x.shape
    Ho, Wo = out_hw
    y = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    if own_window and (Ho, Wo) == (2 * Hi, 2 * Wi) and Wi % 2 == 0:
        rc = load().bn_maxunpool2d_fwd_k2(_ptr(x, 'x'), _ptr(idx, 'idx', torch.int32), _ptr(y, 'y'), N * C, Hi, Wi,
                                          _stream())
        if rc == 0:
            return y
    _check(load().bn_maxunpool2d_fwd(_ptr(x, 'x'), _ptr(idx, 'idx', torch.int32), _ptr(y, 'y'),
                                     N * C, Hi * Wi, Ho * Wo, _stream()), 'bn_maxunpool2d_fwd')
    return y


def maxunpool2d_bwd(dy, idx):
    N, C, Ho, Wo = dy.shape
    dx = torch.empty(idx.shape, dtype=torch.float32, device=dy.device)
    _check(load().bn_maxunpool2d_bwd(_ptr(dy, 'dy'), _ptr(idx, 'idx', torch.int32), _ptr(dx, 'dx'),
                                     N * C, idx.shape[2] * idx.shape[3], Ho * Wo, _stream()),
           'bn_maxunpool2d_bwd')
    return dx
