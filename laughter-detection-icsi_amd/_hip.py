"""ctypes binding of liblad_hip.so (C ABI declared in include/lad_hip.h).

The product path has no CPU fallback: if the library is missing or a call fails this module raises.
PyTorch is used only for device memory and streams (tensor.data_ptr(), current stream handle).
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LAD_HIP_LIB") or os.path.join(_HERE, "liblad_hip.so")   # (LAD_HIP_LIB: A/B builds, tools/ only)

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_i64 = ctypes.c_int64
c_float = ctypes.c_float
c_double = ctypes.c_double
c_i32 = ctypes.c_int32
c_float_p = ctypes.POINTER(ctypes.c_float)


class LadHipError(RuntimeError):
    pass


class FbankCfg(ctypes.Structure):
    _fields_ = [("n_fft", ctypes.c_int32), ("frame_len", ctypes.c_int32), ("hop", ctypes.c_int32),
                ("n_mels", ctypes.c_int32), ("n_mfcc", ctypes.c_int32), ("pad_mode", ctypes.c_int32),
                ("log_mode", ctypes.c_int32), ("remove_dc", ctypes.c_int32), ("preemph", ctypes.c_float),
                ("log_floor", ctypes.c_float)]


class AugmentParams(ctypes.Structure):
    """lad_augment_params of include/lad_hip.h (the convention is written out there)."""
    _fields_ = [("seed", ctypes.c_uint64), ("epoch", ctypes.c_uint32), ("p", ctypes.c_float), ("mix_p", ctypes.c_float),
                ("snr_lo", ctypes.c_float), ("snr_hi", ctypes.c_float), ("gain_lo", ctypes.c_float), ("gain_hi", ctypes.c_float),
                ("W", ctypes.c_int32), ("n_time", ctypes.c_int32), ("Wt", ctypes.c_int32), ("n_freq", ctypes.c_int32),
                ("Wf", ctypes.c_int32)]


# name -> (restype, argtypes); every symbol declared in include/lad_hip.h must be listed here
# (tests/test_cabi.py cross-checks this table against the header and the built library).
SIGNATURES = {
    "lad_version": (c_int, []),
    "lad_last_error": (ctypes.c_char_p, []),
    "lad_fbank_plan_create": (c_int, [ctypes.POINTER(FbankCfg), c_void_p, c_void_p, c_void_p,
                                      ctypes.POINTER(c_void_p)]),
    "lad_fbank_plan_destroy": (c_int, [c_void_p]),
    "lad_fbank_plan_set_kernel": (c_int, [c_void_p, c_int]),
    "lad_fbank_plan_has_fast_kernel": (c_int, [c_void_p]),
    "lad_fbank_num_frames": (c_i64, [c_void_p, c_i64]),
    "lad_fbank_forward": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p]),
    "lad_fbank_forward_long": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "lad_gather_segments": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_float, c_void_p, c_void_p]),
    "lad_gather_segments_aug": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_float, ctypes.POINTER(AugmentParams), c_void_p, c_i32, c_i64,
                                        c_void_p, c_void_p]),
    "lad_assemble_windows": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_act_rows": (c_i64, [c_i64, c_i32, c_i32]),
    "lad_conv_packed_weight_floats": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    "lad_conv_pack_weights": (c_int, [c_void_p, c_i32, c_i32, c_i32, c_i32, c_void_p, c_void_p]),
    "lad_conv_pack_weights_multi": (c_int, [c_void_p, c_i32, c_void_p]),
    "lad_conv_num_tiles": (c_i64, [c_i64, c_i32, c_i32]),
    "lad_conv_fwd": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_b3_packed_weight_bytes": (c_i64, []),
    "lad_conv_b3_pack_weights": (c_int, [c_void_p, c_i32, c_void_p, c_void_p]),
    "lad_conv_b3_fwd_f32": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_conv_b3c_packed_weight_bytes": (c_i64, [c_i32]),
    "lad_conv_b3c_pack_weights": (c_int, [c_void_p, c_i32, c_void_p, c_i32, c_void_p]),
    "lad_conv_b3c_fwd_f32": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_b3c_fwd_f32_bnrelu": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_b3c_dgrad_bnstat": (c_int, [c_void_p] * 7 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_h2_packed_weight_bytes": (c_i64, [c_i32]),
    "lad_conv_h2_pack_weights_multi": (c_int, [c_void_p, c_i32, c_i32, c_void_p]),
    "lad_conv_wgrad_h2": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_h2": (c_int, [c_void_p] * 11 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_wgrad_h2_bnbwd": (c_int, [c_void_p] * 11 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_wgrad_b3c_workspace_floats": (c_i64, [c_i32]),
    "lad_conv_wgrad_b3c": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_b3_fwd_f32_gated": (c_int, [c_void_p] * 7 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_conv_b3_fwd_f32_bnrelu": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_conv_wgrad_b3_bnrelu": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_wgrad_defer_begin": (c_int, []),
    "lad_wgrad_defer_flush": (c_int, [c_void_p]),
    "lad_conv_b3_dgrad_bnstat": (c_int, [c_void_p] * 9 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_conv_wgrad_b3": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_fwd": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_bn_fold": (c_int, [c_void_p] * 5 + [c_i32, c_void_p, c_void_p, c_void_p]),
    "lad_conv_fwd_eval": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_fwd_eval": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_upsample2": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_dgrad": (c_int, [c_void_p] * 3 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_wgrad_workspace_floats": (c_i64, [c_i32, c_i32, c_i32]),
    "lad_conv_s2_fwd_fused": (c_int, [c_void_p] * 8 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_dgrad_partials": (c_i64, [c_i64, c_i32, c_i32]),
    "lad_conv_s2b3_packed_weight_bytes": (c_i64, []),
    "lad_conv_s2b3_pack_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "lad_conv_s2b3_fwd": (c_int, [c_void_p] * 7 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_conv_s2b3_dgrad_packed_weight_bytes": (c_i64, []),
    "lad_conv_s2b3_dgrad_pack_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "lad_conv_s2b3_pack_weights_pair": (c_int, [c_void_p] * 5),
    "lad_conv_s2b3_dgrad_partials": (c_i64, [c_i64, c_i32, c_i32]),
    "lad_conv_s2b3_dgrad": (c_int, [c_void_p] * 8 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_dgrad_fused_bnstat": (c_int, [c_void_p] * 9 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_dgrad_fused": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_wgrad_fused_workspace_floats": (c_i64, [c_i32, c_i32]),
    "lad_conv_s2_wgrad_fused": (c_int, [c_void_p] * 7 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_s2_wgrad": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_wgrad_workspace_floats": (c_i64, [c_i32, c_i32, c_i32]),
    "lad_conv_wgrad": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_stem_fwd": (c_int, [c_void_p] * 4 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_stem_fwd_eval": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i64, c_i64, c_void_p]),
    "lad_stem_wgrad_workspace_floats": (c_i64, []),
    "lad_stem_wgrad": (c_int, [c_void_p] * 4 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_stem_wgrad_bn": (c_int, [c_void_p] * 8 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_stem_bn_bwd_groups": (c_i64, [c_i64, c_i32, c_i32]),
    "lad_stem_bn_bwd_sums": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_bn_finalize": (c_int, [c_void_p, c_i64, c_i32, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                c_void_p, c_void_p]),
    "lad_stem_moments_workspace_doubles": (c_i64, []),
    "lad_stem_moments_doubles": (c_i64, []),
    "lad_stem_bn_stats": (c_int, [c_void_p] * 6 + [c_float] + [c_void_p] * 3 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_stem_bwd_onepass_workspace_floats": (c_i64, []),
    "lad_stem_bwd_onepass": (c_int, [c_void_p] * 10 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_bn_finalize_pair": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_i64] + [c_void_p] * 10 + [c_float, c_void_p]),
    "lad_bn_act": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_bn_bwd_workspace_floats": (c_i64, [c_i32]),
    "lad_bn_act_bits": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_bn_bwd_bits": (c_int, [c_void_p] * 11 + [c_i64, c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_bn_bwd": (c_int, [c_void_p] * 17 + [c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_conv_fwd_bnstat": (c_int, [c_void_p] * 8 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_pool_fwd": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_pool_bwd": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_head_workspace_floats": (c_i64, [c_i64, c_i32]),
    "lad_head_fwd_train": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_void_p, c_void_p, c_void_p, c_float,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lad_head_fwd_train_rng": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_void_p, c_void_p, c_float, ctypes.c_uint64, c_void_p, c_void_p, c_i32,
                                       c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lad_head_fwd_eval": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_void_p, c_void_p]),
    "lad_bce_metrics": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "lad_head_bwd": (c_int, [c_void_p] * 7 + [c_i64, c_i32] + [c_void_p] * 6),
    "lad_f16_packed_weight_halfs": (c_i64, [c_i32, c_i32, c_i32]),
    "lad_f16_pack_weights": (c_int, [c_void_p, c_i32, c_i32, c_i32, c_void_p, c_void_p]),
    "lad_f16_stem_fwd": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i64, c_i64, c_void_p]),
    "lad_f16_conv_fwd": (c_int, [c_void_p] * 6 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_f16_block_fwd": (c_int, [c_void_p] * 8 + [c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_f16_conv_s2_fwd_sc": (c_int, [c_void_p] * 9 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_f16_conv_s2_fwd_mapped_sc": (c_int, [c_void_p] * 9 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_i32, c_i64, c_i64, c_i32,
                                              c_i32, c_i32, c_i32, c_void_p]),
    "lad_f16_conv_s2_fwd": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_f16_conv_s2_fwd_windows": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_f16_conv_s2_fwd_mapped": (c_int, [c_void_p] * 5 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_i32, c_i64, c_i64, c_i32,
                                                          c_i32, c_i32, c_i32, c_i32, c_void_p]),
    "lad_f16_block_fwd_stem_rows": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64] + [c_void_p] * 10 + [c_i64, c_i32, c_i32, c_void_p]),
    "lad_f16_conv_s2_strips_fwd": (c_int, [c_void_p] * 9 + [c_i64, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_i32, c_void_p]),
    "lad_f16_tail_fwd": (c_int, [c_void_p, c_i64, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_i32, c_i64, c_i64, c_void_p, c_void_p, c_i32,
                                 c_void_p, c_void_p]),
    "lad_f16_pool_fwd": (c_int, [c_void_p, c_void_p, c_i64, c_i32, c_i32, c_i32, c_void_p]),
    "lad_grad_sumsq_partials": (c_i32, []),
    "lad_grad_sumsq": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p]),
    "lad_grad_accumulate": (c_int, [c_void_p, c_void_p, c_i64, c_double, c_void_p]),
    "lad_adam_step": (c_int, [c_void_p] * 4 + [c_i64, c_void_p] + [c_double] * 6 + [c_i64, c_void_p, c_i32, c_void_p, c_void_p]),
    # threshold sweep of the probability track (csrc/runs.hip)
    "lad_runs_tile_frames": (c_i32, []),
    "lad_runs_max_thresholds": (c_i32, []),
    "lad_runs_workspace_bytes": (c_i64, [c_i64, c_i64, c_i32]),
    "lad_runs_count": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_double), c_i32, c_void_p, c_void_p]),
    "lad_runs_fill": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_double), c_i32, c_void_p,
                              ctypes.POINTER(c_i32), c_void_p, c_i64, c_void_p]),
    # scores of the sweep against transcript intervals (csrc/score.hip)
    "lad_score_max_min_lengths": (c_i32, []),
    "lad_score_workspace_bytes": (c_i64, [c_i64, c_i64, c_i32, c_i32]),
    "lad_score_runs": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_i32), c_i64, c_i64, c_i32, c_void_p, c_void_p,
                               ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i64, c_void_p, ctypes.POINTER(c_double),
                               ctypes.POINTER(c_double), c_i32, c_void_p, c_void_p, c_void_p]),
    # event-level scores of the sweep (csrc/events.hip)
    "lad_score_events_workspace_bytes": (c_i64, [c_i64, c_i64, c_i32, c_i32, c_i64]),
    "lad_score_events": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_i32), c_i64, c_i64, c_i32, c_void_p, c_void_p,
                                 ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i64, c_void_p, ctypes.POINTER(c_double),
                                 ctypes.POINTER(c_double), c_i32, c_i32, c_i32, c_void_p, c_void_p, c_void_p]),
    # threshold sweep with hysteresis and gap filling (csrc/binarize.hip)
    "lad_binarize_max_settings": (c_i32, []),
    "lad_binarize_workspace_bytes": (c_i64, [c_i64, c_i64, c_i32]),
    "lad_binarize_count": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_double), ctypes.POINTER(c_double), c_i32,
                                   c_void_p, c_void_p]),
    "lad_binarize_fill": (c_int, [c_void_p, c_i32, c_i64, c_i64] + [ctypes.POINTER(c_double)] * 3
                          + [c_i32, c_void_p, ctypes.POINTER(c_double), c_void_p, ctypes.POINTER(c_i32), c_void_p, c_void_p, c_i64,
                             c_void_p]),
    # two-state Viterbi decoding of the probability track (csrc/viterbi.hip)
    "lad_viterbi_max_settings": (c_i32, []),
    "lad_viterbi_table_entries": (c_i32, []),
    "lad_viterbi_workspace_bytes": (c_i64, [c_i64, c_i64, c_i32]),
    "lad_viterbi_count": (c_int, [c_void_p, c_i32, c_i64, c_i64, c_void_p] + [ctypes.POINTER(c_i32)] * 3
                          + [c_i32, c_void_p, c_void_p, c_void_p]),
    "lad_viterbi_fill": (c_int, [c_void_p, ctypes.POINTER(c_i32), c_i64, c_i64, c_i32, c_void_p, c_i64, c_void_p]),
    # dense threshold sweep: the scores of every level from the track's component tree (csrc/surface.hip)
    "lad_surface_max_levels": (c_i32, []),
    "lad_surface_tile_frames": (c_i32, []),
    "lad_surface_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_i32, c_i32]),
    "lad_score_surface": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_double), c_i32, c_void_p, c_void_p,
                                  ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i64, c_void_p, ctypes.POINTER(c_double),
                                  ctypes.POINTER(c_double), c_i32, c_void_p, c_void_p, c_void_p]),
    # event-level scores on the dense sweep: both score arrays of every level from one tree (csrc/surface_events.hip)
    "lad_surface_events_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64, c_i32, c_i32]),
    "lad_score_surface_events": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_double), c_i32, c_void_p, c_void_p,
                                         ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i64, c_void_p, ctypes.POINTER(c_double),
                                         ctypes.POINTER(c_double), c_i32, c_i32, c_i32, c_void_p, c_void_p, c_void_p, c_void_p]),
    # sampling-rate conversion (csrc/resample.hip)
    "lad_resample_out_len": (c_i64, [c_i64, c_i32, c_i32]),
    "lad_resample_tile_outputs": (c_i32, []),
    "lad_resample_max_up": (c_i32, []),
    "lad_resample_max_down": (c_i32, []),
    "lad_resample_max_taps": (c_i32, []),
    "lad_resample_max_lds_bytes": (c_i64, []),
    "lad_resample_lds_bytes": (c_i64, [c_i32, c_i32, c_i32]),
    "lad_resample": (c_int, [c_void_p, c_i32, c_i64, c_void_p, c_i32, c_i32, c_i32, c_i64, c_i64, c_void_p, c_void_p]),
    # zero-phase low-pass of the probability track (csrc/lowpass.hip)
    "lad_lowpass_tile_frames": (c_i32, []),
    "lad_lowpass_workspace_bytes": (c_i64, [c_i64, c_i64]),
    "lad_lowpass": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_i64)] + [ctypes.POINTER(c_double)] * 3
                    + [c_void_p, c_void_p, c_void_p]),
    # median / rank filter of the probability track (csrc/rankfilt.hip)
    "lad_rank_filter_tile_frames": (c_i32, []),
    "lad_rank_filter_max_window": (c_i32, []),
    "lad_rank_filter_workspace_bytes": (c_i64, [c_i64, c_i64, c_i32]),
    "lad_rank_filter": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_i64), c_i32, c_i32, c_void_p, c_void_p, c_void_p]),
    # confidence of an instance: sum and earliest peak of the track over every span (csrc/spanstats.hip)
    "lad_span_stats_tile_frames": (c_i32, []),
    "lad_span_stats_workspace_bytes": (c_i64, [c_i64, c_i64]),
    "lad_span_stats_prepare": (c_int, [c_void_p, c_i32, c_i64, c_i64, c_void_p, c_void_p]),
    "lad_span_stats": (c_int, [c_void_p, c_i32, c_i64, c_i64, c_void_p, c_void_p, ctypes.POINTER(c_i32), c_i32, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    # redrawing the segment table, transcript coverage of windows (csrc/sample.hip)
    "lad_sample_segments": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_i32,
                                    ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), ctypes.POINTER(c_i64),
                                    c_i32, ctypes.c_uint64, ctypes.c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lad_window_coverage": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i32, c_void_p, c_void_p, ctypes.POINTER(c_i32),
                                    ctypes.POINTER(c_i32), c_i64, c_i32, c_i32, c_void_p, c_void_p]),
    # bootstrap intervals of the sweep's figures: resample weights, weighted sums, exact quantiles (csrc/bootstrap.hip)
    "lad_bootstrap_max_units": (c_i64, []),
    "lad_bootstrap_max_replicates": (c_i64, []),
    "lad_bootstrap_weights": (c_int, [c_i32, c_i32, ctypes.c_uint64, c_void_p, c_void_p]),
    "lad_bootstrap_sums": (c_int, [c_void_p, c_void_p, c_i32, c_i64, c_i32, c_void_p, c_void_p]),
    "lad_bootstrap_quantiles": (c_int, [c_void_p, c_i64, c_i32, c_void_p, ctypes.POINTER(c_i32), c_i64, ctypes.POINTER(c_i32),
                                        ctypes.POINTER(c_i32), c_i32, c_void_p, c_void_p, c_void_p]),
    "lad_bootstrap_pair_quantiles": (c_int, [c_void_p, c_i64, c_i32, c_void_p, ctypes.POINTER(c_i32), c_i64, ctypes.POINTER(c_i32),
                                             ctypes.POINTER(c_i32), c_i32, c_void_p, c_void_p, c_void_p, c_void_p]),
    # calibration of the track: label histogram against the transcript, a 65537-entry map applied to a track (csrc/calibration.hip)
    "lad_label_histogram_slots": (c_i32, []),
    "lad_label_histogram_tile_frames": (c_i32, []),
    "lad_label_histogram_workspace_bytes": (c_i64, [c_i64, c_i64, c_i64]),
    "lad_label_histogram": (c_int, [c_void_p, c_i32, c_i64, c_i64, ctypes.POINTER(c_i64), c_void_p, c_void_p, ctypes.POINTER(c_i32),
                                    ctypes.POINTER(c_i32), c_i64, c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_i32), c_i32,
                                    c_void_p, c_void_p, c_void_p]),
    "lad_track_remap": (c_int, [c_void_p, c_i32, c_i64, c_i64, c_void_p, c_void_p, c_void_p]),
}

_lib = None


def lib():
    """Load liblad_hip.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LadHipError(
                f"{LIB_PATH} not found: build it with `python laughter-detection-icsi_amd/build.py` "
                "(there is no CPU fallback for the HIP hot path)")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


LAD_ERR_INVALID = -1   # include/lad_hip.h: bad argument / unsupported shape (nothing was launched)
LAD_NOT_COVERED = 1    # ... a try-and-fall-back entry point does not cover the geometry (nothing launched, no error string)


def check(rc, what=""):
    if rc != 0:
        msg = lib().lad_last_error().decode("utf-8", "replace")
        raise LadHipError(f"{what or 'liblad_hip'} failed ({rc}): {msg}")


def require_cuda(t, name="tensor", dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise LadHipError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise LadHipError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise LadHipError(f"{name} must have dtype {dtype}, got {t.dtype}")
    return t


def device_track(probs, what="sweep"):
    """What every device form asks of its probability tensor: (T,) or (C, T), in GPU memory, contiguous, float32 or float64.
    Returns (the (C, T) tensor, its lad_runs_dtype, whether it was a (T,) one)."""
    single = getattr(probs, "ndim", None) == 1
    if single and hasattr(probs, "unsqueeze"):
        probs = probs.unsqueeze(0)
    if getattr(probs, "ndim", None) != 2:
        raise LadHipError(f"probs must be a (T,) or (C, T) GPU tensor (the device {what} has no CPU fallback)")
    require_cuda(probs, "probs")
    if probs.dtype not in (torch.float32, torch.float64):
        raise LadHipError(f"probs must be float32 or float64, got {probs.dtype}")
    return probs, 0 if probs.dtype == torch.float32 else 1, single


def channel_lengths(lengths, C):
    """lengths= of a filter: None, or the frame counts of the C channels as a contiguous int64 array."""
    if lengths is None:
        return None
    lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    if lengths.shape != (C,):
        raise ValueError(f"{lengths.size} lengths for {C} channels")
    return lengths


def out_track(out, probs, single, dtype):
    """out= of a filter as the (C, T) tensor it writes into: a new one of `dtype`, or the caller's, which must be a contiguous GPU
    tensor of that dtype with the shape ((T,) if `single`) and device of the track.  probs: the (C, T) tensor of device_track."""
    if out is None:
        return torch.empty(probs.shape, dtype=dtype, device=probs.device)
    require_cuda(out, "out", dtype)
    if out.shape != (probs.shape[1:] if single else probs.shape) or out.device != probs.device:
        raise ValueError("out must have the shape and device of probs")
    return out.unsqueeze(0) if single else out


def workspace(query_name, *sizes, device):
    """The workspace of an entry point: a uint8 GPU tensor of as many bytes as its size query asks for these sizes (LadHipError
    with the library's message for sizes the query refuses)."""
    n_bytes = getattr(lib(), query_name)(*sizes)
    check(0 if n_bytes >= 0 else LAD_ERR_INVALID, query_name)
    return torch.empty(n_bytes, dtype=torch.uint8, device=device)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def stream_handle(device=None):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


# host-array slots: the numpy dtype a POINTER(...) parameter reads
_HOST_DTYPES = {ctypes.POINTER(c_double): np.dtype(np.float64), ctypes.POINTER(c_float): np.dtype(np.float32),
                ctypes.POINTER(c_i32): np.dtype(np.int32), ctypes.POINTER(c_i64): np.dtype(np.int64)}
_PLAIN = frozenset((int, float, type(None)))     # what most arguments are: passed on without a second look


def _marshal(name, args, a, index):
    """The slow half of launch(): a host array as the pointer its slot takes, or LadHipError for the array or tensor `a` that may
    not go where it stands (a tensor that launch() did not take: not in GPU memory, or not on the launch device `index`)."""
    i = next(k for k, x in enumerate(args) if x is a)
    argtype = SIGNATURES[name][1][i]
    where = f"{name}: argument {i + 1}"      # (counted from 1, as ctypes counts)
    if isinstance(a, torch.Tensor):
        raise LadHipError(f"{where} must be a GPU tensor on device {index}, got one on {a.device} (a host pointer in a kernel argument "
                          "is a GPU fault, not an exception)")
    want = _HOST_DTYPES.get(argtype)
    if want is None:
        raise LadHipError(f"{where} is a host array, but the parameter is {'a device pointer' if argtype is c_void_p else 'no host array'}")
    if a.dtype != want or not a.flags.c_contiguous:
        raise LadHipError(f"{where} must be a C-contiguous {want.name} array, got {a.dtype}{'' if a.flags.c_contiguous else ', not contiguous'}")
    return a.ctypes.data_as(argtype)


def launch(name, *args, stream=None, device=None, tag="", may_decline=False):
    """Call entry point `name` (one whose last parameter is the stream) with args and then the stream: `stream`, or the current
    stream of `device`, or of the first tensor argument's device.  A tensor goes in as its data_ptr() and must lie in GPU memory,
    on the launch device; a numpy array goes in as a pointer to its buffer and must stand in a POINTER(double | float | int32 |
    int64) slot of SIGNATURES, C-contiguous and of exactly that dtype; None is NULL; everything else (ctypes arrays and pointers,
    c_void_p values, structures, numbers) passes through.  A wrong argument count, tensor or array, or a value ctypes will not put
    into its slot (a tensor's address in a host-array slot), raises LadHipError before the library is reached; a non-zero return
    code raises what check() raises, for "<name> <tag>".  may_decline: LAD_NOT_COVERED is an answer, not an error: False then,
    True when the kernel was launched.  (One comprehension, no per-call objects: a train step comes through here 150 times.)"""
    if len(args) + 1 != len(SIGNATURES[name][1]):
        raise LadHipError(f"{name} takes {len(SIGNATURES[name][1]) - 1} arguments and the stream, got {len(args)}")
    if device is None:
        index = next((a.get_device() for a in args if isinstance(a, torch.Tensor)), None)    # (None: no tensor among the arguments)
        if index == -1:
            index = -2     # host memory: no tensor's get_device() is -2, so every tensor is refused
    elif device.type != "cuda":
        index = -2
    else:
        index = device.index if device.index is not None else torch.cuda.current_device()
    out = [a if a.__class__ in _PLAIN else
           (a.data_ptr() if a.get_device() == index else _marshal(name, args, a, index)) if isinstance(a, torch.Tensor) else
           _marshal(name, args, a, index) if isinstance(a, np.ndarray) else a for a in args]
    if stream is None:
        stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if index is None else index)
    try:
        rc = getattr(lib(), name)(*out, stream)
    except ctypes.ArgumentError as e:
        raise LadHipError(f"{name}: {e}") from None
    if rc != 0:
        if may_decline and rc == LAD_NOT_COVERED:
            return False
        check(rc, name + " " + tag if tag else name)
    return True
