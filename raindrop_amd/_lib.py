"""ctypes binding of libraindrop_hip.so (the C-ABI declared in include/raindrop_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol cannot be
resolved, importing/using the ops raises.  Build it with `python -m raindrop_amd.build`
(or `__graft_entry__.build()`).
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int32, c_size_t, c_void_p

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RD_LIB_PATH") or os.path.join(_PKG, "libraindrop_hip.so")   # RD_LIB_PATH: A/B builds (tools/ab_build.sh)


class RdShape(ctypes.Structure):
    """Mirror of `struct rd_shape` (include/raindrop_hip.h)."""
    _fields_ = [(n, c_int32) for n in ("B", "T", "F", "d_ob", "d_pe", "nhead", "nhid", "d_static",
                                       "n_classes", "max_len")]


class RaindropHipError(RuntimeError):
    pass


class RdEncoderPtrs(ctypes.Structure):
    """Mirror of rd_encoder_weights / rd_encoder_grads (12 device pointers)."""
    FIELDS = ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "lin1_w", "lin1_b", "lin2_w",
              "lin2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")
    _fields_ = [(n, c_void_p) for n in FIELDS]


_P = c_void_p
_ENC = POINTER(RdEncoderPtrs)
_SHP = POINTER(RdShape)

# name -> (restype, argtypes); every symbol the header declares appears here, and
# tests/test_cabi_symbols.py checks the two lists against each other.
SIGNATURES = {
    "rd_version": (c_int32, []),
    "rd_arch": (c_char_p, []),
    "rd_last_error": (c_char_p, []),
    "rd_set_precision": (c_int32, [c_int32]),
    "rd_get_precision": (c_int32, []),
    "rd_set_seed_cell": (c_int32, [_P]),
    "rd_set_side_stream": (c_int32, [_P]),
    "rd_side_join": (c_int32, [_P]),
    "rd_set_defer_trailing": (c_int32, [c_int32]),
    "rd_flush_trailing": (c_int32, [_P]),
    "rd_drop_trailing": (c_int32, []),
    "rd_seed_cell_advance": (c_int32, [_P, ctypes.c_uint64, _P]),
    "rd_token_plan_bytes": (c_size_t, [_SHP]),
    "rd_token_plan": (c_int32, [_SHP, _P, _P, _P, ctypes.c_uint64, _P]),
    "rd_set_token_plan": (c_int32, [_P]),
    "rd_graph_build": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P]),
    "rd_pe_mask": (c_int32, [_SHP, _P, _P, _P, _P, _P, _P]),
    "rd_edge_softmax": (c_int32, [c_int32, _P, _P, _P, _P]),
    "rd_edge_softmax_list": (c_int32, [c_int32, c_int32, _P, ctypes.c_int64, c_int32, _P, _P, _P, _P]),
    "rd_edge_attention_fwd": (c_int32, [c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, ctypes.c_int64, c_float, ctypes.c_uint64,
                                        _P, _P, _P, _P]),
    "rd_edge_attention_bwd": (c_int32, [c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, ctypes.c_int64, c_float, ctypes.c_uint64,
                                        _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rd_edge_softmax_list_dropout": (c_int32, [c_int32, c_int32, _P, ctypes.c_int64, c_int32, _P, c_float, ctypes.c_uint64, _P, _P, _P]),
    "rd_aggregate_fwd": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P]),
    "rd_aggregate_bwd": (c_int32, [c_int32, c_int32, _P, _P, _P, _P]),
    "rd_edge_softmax_list_batched": (c_int32, [c_int32, c_int32, c_int32, _P, ctypes.c_int64, ctypes.c_int64, c_int32, _P,
                                               ctypes.c_int64, _P, _P, _P]),
    "rd_edge_softmax_list_batched_dropout": (c_int32, [c_int32, c_int32, c_int32, _P, ctypes.c_int64, ctypes.c_int64, c_int32, _P,
                                                       ctypes.c_int64, c_float, ctypes.c_uint64, _P, _P, _P]),
    "rd_edge_gamma_dense": (c_int32, [c_int32, c_int32, _P, ctypes.c_int64, _P, _P, _P]),
    "rd_aggregate_batched_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P]),
    "rd_aggregate_batched_bwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "rd_scale_dropout": (c_int32, [ctypes.c_int64, _P, c_float, c_float, ctypes.c_uint64, ctypes.c_uint32, _P, _P]),
    "rd_obs_embed_fwd": (c_int32, [_SHP, _P, _P, c_float, ctypes.c_uint64, _P, _P]),
    "rd_obs_embed_bwd_workspace_bytes": (c_size_t, [_SHP]),
    "rd_obs_embed_bwd": (c_int32, [_SHP, _P, _P, _P, c_float, _P, _P, c_size_t, _P]),
    "rd_rows_to_tokens_fwd": (c_int32, [_SHP, _P, _P, _P, c_int32, _P]),
    "rd_rows_to_tokens_bwd": (c_int32, [_SHP, _P, c_int32, _P, _P, _P]),
    "rd_msgpass_workspace_bytes": (c_size_t, [_SHP]),
    "rd_msgpass_saved_bytes": (c_size_t, [_SHP]),
    "rd_msgpass_fwd": (c_int32, [_SHP] + [_P] * 7 + [c_float, ctypes.c_uint64, _P, c_int32, _P, c_size_t, _P]),
    "rd_sensor_stage_fwd": (c_int32, [_SHP] + [_P] * 10 + [c_float, ctypes.c_uint64, _P, _P, _P, c_size_t, _P]),
    "rd_sensor_stage_fwd_prepared": (c_int32, [_SHP] + [_P] * 10 + [c_float, ctypes.c_uint64, _P, _P, _P, c_size_t, _P]),
    "rd_msgpass_coef_table": (c_int32, [c_int32, c_int32, c_int32, _P, ctypes.c_int64, _P, _P, c_float, c_float, ctypes.c_uint64, _P, _P]),
    "rd_msgpass_fwd_coef": (c_int32, [_SHP] + [_P] * 8 + [c_float, ctypes.c_uint64, _P, c_int32, _P, c_size_t, _P]),
    "rd_sensor_stage_fwd_coef": (c_int32, [_SHP] + [_P] * 11 + [c_float, ctypes.c_uint64, _P, _P, _P, c_size_t, _P]),
    "rd_sensor_stage_fwd_prepared_coef": (c_int32, [_SHP] + [_P] * 11 + [c_float, ctypes.c_uint64, _P, _P, _P, c_size_t, _P]),
    "rd_msgpass_bwd_coef": (c_int32, [_SHP] + [_P] * 6 + [c_float, _P, c_size_t, _P, _P, c_int32] + [_P] * 5
                            + [_P, c_size_t, _P]),
    "rd_step_prepare": (c_int32, [_SHP, c_int32, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "rd_step_begin": (c_int32, [_SHP, _P, _P, _P, ctypes.c_uint64, c_int32, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "rd_step_prepare_covers": (c_int32, [_SHP, _P, _P]),
    "rd_msgpass_bwd": (c_int32, [_SHP] + [_P] * 5 + [c_float, _P, c_size_t, _P, _P, c_int32] + [_P] * 5
                       + [_P, c_size_t, _P]),
    "rd_encoder_layer_saved_bytes": (c_size_t, [_SHP]),
    "rd_encoder_layer_workspace_bytes": (c_size_t, [_SHP]),
    "rd_encoder_layer_prepare": (c_int32, [_SHP, _ENC, _P, c_size_t, _P]),
    "rd_encoder_layer_fwd": (c_int32, [_SHP, c_int32, _P, _P, _ENC, c_float, ctypes.c_uint64, _P, _P, c_size_t,
                                        _P, c_size_t, _P]),
    "rd_encoder_layer_bwd": (c_int32, [_SHP, c_int32, _P, _P, _ENC, c_float, ctypes.c_uint64, _P, c_size_t, _P, _P,
                                        _ENC, _P, c_size_t, _P]),
    "rd_attention_fwd": (c_int32, [_SHP, c_int32, _P, _P, c_float, ctypes.c_uint64, _P, _P, _P]),
    "rd_attention_bwd": (c_int32, [_SHP, c_int32, _P, _P, c_float, ctypes.c_uint64, _P, _P, _P, _P, _P, _P]),
    "rd_masked_mean_fwd": (c_int32, [_SHP, c_int32, _P, _P, _P, _P, c_int32, _P]),
    "rd_masked_mean_bwd": (c_int32, [_SHP, c_int32, _P, c_int32, _P, _P, _P, _P]),
    "rd_adam_step": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float,
                                ctypes.c_int64, _P]),
    "rd_adam_step_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P]),
    "rd_adam_state_advance": (c_int32, [_P, c_float, c_float, _P]),
    "rd_set_adam_state": (c_int32, [_P, c_float, c_float]),
    # global-norm gradient clipping / non-finite guard (include/raindrop_hip.h; raindrop_amd.optim.FlatAdam(max_grad_norm=...))
    "rd_grad_sumsq_grid": (c_int32, []),
    "rd_grad_sumsq_bytes": (c_size_t, []),
    "rd_grad_sumsq": (c_int32, [ctypes.c_int64, _P, _P, c_size_t, _P]),
    "rd_adam_step_clip": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, ctypes.c_int64,
                                    _P, c_size_t, _P, _P]),
    "rd_adam_step_clip_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P, c_size_t, _P, _P]),
    # weight averaging inside the update's launch (raindrop_amd.optim.FlatAdam(ema_decay=...)): the twins take `ema`, `ema_cell` in front of the stream
    "rd_adam_step_ema": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float,
                                   ctypes.c_int64, _P, _P, _P]),
    "rd_adam_step_ema_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P, _P, _P]),
    "rd_adam_step_clip_ema": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, ctypes.c_int64,
                                        _P, c_size_t, _P, _P, _P, _P]),
    "rd_adam_step_clip_ema_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P, c_size_t, _P, _P, _P, _P]),
    "rd_swap_f32": (c_int32, [ctypes.c_int64, _P, _P, _P]),
    # gradient accumulation over a window of micro-batches (raindrop_amd.step.TrainStep(accumulate=k)): g, acc [, scale_cell], stream
    "rd_grad_accumulate": (c_int32, [ctypes.c_int64, _P, _P, _P]),
    "rd_grad_accumulate_close": (c_int32, [ctypes.c_int64, _P, _P, _P, _P]),
    # parameter groups / decoupled weight decay (raindrop_amd.optim.FlatAdam(groups=..., decoupled=...)): the twins take `chunk_group`, `group_cell` in front of the stream
    "rd_adam_step_grp": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float,
                                   ctypes.c_int64, _P, _P, _P]),
    "rd_adam_step_grp_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P, _P, _P]),
    "rd_adam_step_clip_grp": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, ctypes.c_int64,
                                        _P, c_size_t, _P, _P, _P, _P]),
    "rd_adam_step_clip_grp_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P, c_size_t, _P, _P, _P, _P]),
    "rd_adam_step_ema_grp": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float,
                                       ctypes.c_int64, _P, _P, _P, _P, _P]),
    "rd_adam_step_ema_grp_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "rd_adam_step_clip_ema_grp": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, ctypes.c_int64,
                                            _P, c_size_t, _P, _P, _P, _P, _P, _P]),
    "rd_adam_step_clip_ema_grp_dev": (c_int32, [ctypes.c_int64, _P, _P, _P, _P, c_float, c_float, c_float, _P, _P, c_size_t, _P, _P, _P,
                                                _P, _P, _P]),
    "rd_linear_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, c_int32, _P, _P, _P, c_int32, c_int32, _P]),
    "rd_linear_fwd_fp32": (c_int32, [c_int32, c_int32, c_int32, _P, c_int32, _P, _P, _P, c_int32, c_int32, _P]),
    "rd_linear_bwd_input": (c_int32, [c_int32, c_int32, c_int32, _P, c_int32, _P, _P, c_int32, _P]),
    "rd_linear_bwd_input_gated": (c_int32, [c_int32, c_int32, c_int32, _P, c_int32, _P, _P, c_int32, _P, c_int32, _P]),
    "rd_softmax_xent": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P]),
    "rd_softmax_xent_crit": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P]),
    "rd_softmax_xent_focal": (c_int32, [c_int32, c_int32, _P, _P, _P, _P, _P, _P]),      # crit = [gamma, w_0 ..]
    "rd_set_rowgemm_rows32": (c_int32, [c_int32]),
    "rd_set_rowgemm_waves16": (c_int32, [c_int32]),
    "rd_head_train_supported": (c_int32, [c_int32, c_int32, c_int32]),
    "rd_head_train_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "rd_head_train": (c_int32, [_SHP, c_int32, c_int32, c_int32, c_int32] + [_P] * 20 + [_P, c_size_t, _P]),
    "rd_head_train_crit": (c_int32, [_SHP, c_int32, c_int32, c_int32, c_int32] + [_P] * 21 + [_P, c_size_t, _P]),
    "rd_head_train_focal": (c_int32, [_SHP, c_int32, c_int32, c_int32, c_int32] + [_P] * 21 + [_P, c_size_t, _P]),
    "rd_head_forward": (c_int32, [_SHP, c_int32, c_int32, c_int32, c_int32] + [_P] * 11 + [_P, c_size_t, _P]),
    "rd_head_backward": (c_int32, [_SHP, c_int32, c_int32, c_int32, c_int32] + [_P] * 18 + [_P, c_size_t, _P]),
    "rd_batch_gather": (c_int32, [c_int32, c_int32, c_int32, c_int32, ctypes.c_int64] + [_P] * 12),
    # the batch of a captured step from a device-resident epoch plan (raindrop_amd.feed.EpochFeed)
    "rd_feed_gather": (c_int32, [c_int32, c_int32, c_int32, c_int32, ctypes.c_int64, ctypes.c_int64] + [_P] * 13),
    "rd_feed_record": (c_int32, [c_int32, c_int32, ctypes.c_int64] + [_P] * 7),
    # the two gathers with input augmentation (raindrop_amd.feed.Augment): the plain twins' arguments, then aug_cell [, draw], stream
    "rd_batch_gather_aug": (c_int32, [c_int32, c_int32, c_int32, c_int32, ctypes.c_int64] + [_P] * 12 + [ctypes.c_uint64, _P]),
    "rd_feed_gather_aug": (c_int32, [c_int32, c_int32, c_int32, c_int32, ctypes.c_int64, ctypes.c_int64] + [_P] * 14),
    "rd_graph_beta_kept": (c_int32, [c_int32]),
    "rd_graph_beta_workspace_bytes": (c_size_t, [c_int32] * 5),
    "rd_graph_beta_fwd": (c_int32, [c_int32] * 6 + [_P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64]
                          + [_P] * 5 + [_P, c_size_t, _P]),
    "rd_graph_beta_bwd": (c_int32, [c_int32] * 6 + [_P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64]
                          + [_P] * 7 + [_P, c_size_t, _P]),
    "rd_graph_beta_bwd_alpha": (c_int32, [c_int32] * 6 + [_P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64]
                                + [_P] * 8 + [_P, c_size_t, _P]),
    "rd_graph_beta_fwd_dropout": (c_int32, [c_int32] * 6 + [_P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64,
                                                           c_float, ctypes.c_uint64] + [_P] * 5 + [_P, c_size_t, _P]),
    "rd_graph_beta_bwd_dropout": (c_int32, [c_int32] * 6 + [_P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_int64,
                                                           c_float, ctypes.c_uint64] + [_P] * 8 + [_P, c_size_t, _P]),
    "rd_graph_beta_keep": (c_int32, [c_int32, c_int32, c_int32, c_float, ctypes.c_uint64, _P, _P]),
    # inference forward: no save-for-backward buffers (include/raindrop_hip.h "inference forward")
    "rd_infer_covers": (c_int32, [_SHP, _P, _P]),
    "rd_msgpass_infer_bytes": (c_size_t, [_SHP]),
    "rd_encoder_layer_infer_bytes": (c_size_t, [_SHP]),
    "rd_beta_stage_infer_bytes": (c_size_t, [_SHP, c_int32]),
    "rd_sensor_stage_fwd_infer": (c_int32, [_SHP] + [_P] * 10 + [_P, _P, _P, c_size_t, c_int32, _P]),
    "rd_encoder_layer_fwd_infer": (c_int32, [_SHP, c_int32, _P, _P, _ENC, _P, _P, c_size_t, _P, c_size_t, _P]),
    "rd_beta_stage_fwd_infer": (c_int32, [_SHP] + [_P] * 12 + [_P, ctypes.c_int64, _P, c_int32] + [_P] * 5
                                + [_P, c_size_t, _P, c_size_t, _P]),
    "rd_structure_distance": (c_int32, [c_int32, c_int32, _P, _P, _P, _P]),
    "rd_structure_distance_bwd_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "rd_structure_distance_bwd": (c_int32, [c_int32, c_int32, _P, _P, _P, c_size_t, _P, _P]),
    "rd_beta_stage_workspace_bytes": (c_size_t, [_SHP, c_int32]),
    "rd_beta_stage_saved_bytes": (c_size_t, [_SHP, c_int32]),
    "rd_beta_stage_fwd": (c_int32, [_SHP] + [_P] * 12 + [_P, ctypes.c_int64, _P, c_int32, c_float, ctypes.c_uint64] + [_P] * 5
                          + [_P, c_size_t, _P, c_size_t, _P]),
    "rd_beta_stage_bwd": (c_int32, [_SHP] + [_P] * 6 + [_P, ctypes.c_int64, _P, c_int32, c_float, _P, _P, _P, c_size_t, _P, c_int32, _P]
                          + [_P] * 8 + [_P, c_size_t, _P]),
    "rd_beta_stage_fwd_dropout": (c_int32, [_SHP] + [_P] * 12 + [_P, ctypes.c_int64, _P, c_int32, c_float, c_float, ctypes.c_uint64]
                                  + [_P] * 5 + [_P, c_size_t, _P, c_size_t, _P]),
    "rd_beta_stage_bwd_dropout": (c_int32, [_SHP] + [_P] * 6 + [_P, ctypes.c_int64, _P, c_int32, c_float, c_float, ctypes.c_uint64, _P, _P, _P,
                                                           c_size_t, _P, c_int32, _P] + [_P] * 8 + [_P, c_size_t, _P]),
    "rd_beta_l2_tokens_fwd": (c_int32, [_SHP, c_int32, _P, _P, _P, _P, c_int32, _P, _P]),
    "rd_beta_l2_tokens_bwd": (c_int32, [_SHP, c_int32, _P, _P, _P, _P, c_int32, _P, _P, _P]),
    "rd_prep_stats_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int32]),
    "rd_prep_stats": (c_int32, [ctypes.c_int64, c_int32, _P, _P, _P, _P, c_size_t, _P]),
    "rd_prep_mask_normalize": (c_int32, [ctypes.c_int64, c_int32, c_int32, _P, _P, _P, _P, c_int32, _P]),
    "rd_prep_static": (c_int32, [ctypes.c_int64, c_int32, _P, _P, _P, _P, _P]),
    "rd_prep_time": (c_int32, [ctypes.c_int64, c_int32, _P, _P, c_int32, _P]),
    "rd_prep_remove_features": (c_int32, [ctypes.c_int64, c_int32, c_int32, _P, _P, c_int32, c_int32, c_int32, _P]),
    "rd_linear_bwd_weight_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "rd_linear_bwd_weight": (c_int32, [c_int32, c_int32, c_int32, _P, c_int32, _P, c_int32, _P, _P,
                                        _P, c_size_t, _P]),
    "rd_rank_metrics_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int32]),
    "rd_rank_metrics": (c_int32, [ctypes.c_int64, c_int32, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "rd_confusion": (c_int32, [ctypes.c_int64, c_int32, _P, ctypes.c_int64, _P, _P, _P]),
    # bootstrap of the ranking statistics (raindrop_amd.metrics.rank_bootstrap): N, C, scores, ld, y, R, seed, five outputs, workspace
    "rd_rank_bootstrap_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int32, c_int32]),
    "rd_rank_bootstrap": (c_int32, [ctypes.c_int64, c_int32, _P, ctypes.c_int64, _P, c_int32, ctypes.c_uint64] + [_P] * 5
                          + [_P, c_size_t, _P]),
    "rd_rank_bootstrap_summary": (c_int32, [c_int32, c_int32, _P, _P, _P, ctypes.c_double, _P, _P]),
    "rd_rank_bootstrap_counts": (c_int32, [ctypes.c_int64, c_int32, ctypes.c_uint64, c_int32, c_int32, _P, _P]),
    # calibration (raindrop_amd.metrics.calibration / fit_temperature): N, C, logits, ld, y, temperature, column, M, counts, table,
    # summary, workspace | N, C, logits, ld, y, result
    "rd_calibration_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int32, c_int32]),
    "rd_calibration": (c_int32, [ctypes.c_int64, c_int32, _P, ctypes.c_int64, _P, _P, c_int32, c_int32, _P, _P, _P, _P, c_size_t, _P]),
    "rd_fit_temperature": (c_int32, [ctypes.c_int64, c_int32, _P, ctypes.c_int64, _P, _P, _P]),
}
# hooks of include/raindrop_hip_debug.h that tests call through this binding (not part of the ABI)
DEBUG_SIGNATURES = {
    "rd_debug_encoder_route": (c_int32, [_SHP, c_int32, _P]),       # bits: ROUTE_BITS below
    # shape, pass (ATTN_PASSES), with_plan, aligned, words[11] (words[0]: ATTN_FAMILIES / ATTN_ROUTE_BITS below), names joined by ',', cap
    "rd_debug_attention_route": (c_int32, [_SHP, c_int32, c_int32, c_int32, _P, _P, c_size_t]),
    "rd_debug_sensor_route": (c_int32, [_SHP, c_int32, c_int32, c_int32, _P]),      # ldz, with_pe, with_coef; bits: SENSOR_ROUTE_BITS below
    "rd_debug_graph_beta_route": (c_int32, [c_int32] * 6 + [_P]),   # B, N, T, E, with_alpha, with_drop; bits: BETA_ROUTE_BITS below
    # M, N, K, sa_m, sa_k, sb_n, sb_k, nsplit, k_per_split, tile_hint, flags (GEMM_ROUTE_FLAGS), words[5], name, cap
    "rd_debug_gemm_route": (c_int32, [c_int32] * 3 + [ctypes.c_int64] * 4 + [c_int32] * 3 + [ctypes.c_uint32, _P, _P, c_size_t]),
    "rd_debug_splitk_plan": (c_int32, [ctypes.c_int64, c_int32, c_int32, _P]),      # red, rows, cols, *k_per_split -> nsplit
    # mode, B, D, d_static, Fe, C, with_crit (2: the focal form), words[11] (bits of words[0]: HEAD_ROUTE_BITS below), name, cap
    "rd_debug_head_route": (c_int32, [c_int32] * 7 + [_P, _P, c_size_t]),
    "rd_debug_calibration_route": (c_int32, [ctypes.c_int64, c_int32, _P]),         # N, C; bit 0 of *bits: staged in LDS, bits 8-31 its bytes
    "rd_debug_set_calibration_stage": (None, [c_int32]),                            # 0: never stage; 1 (default): by the budget
}
# bit i of rd_debug_encoder_route's mask (csrc/rd_temporal.hip EncRoute, in declaration order)
ROUTE_BITS = ("rg", "dx_rowblock", "tw", "panel", "tw2", "big", "lnf1", "lnf2", "lnb", "chain_fwd", "chain_bwd", "attn_tiles",
              "afuse_fwd", "afuse_bwd", "lean", "infer", "plan_ok")
# rd_debug_attention_route (csrc/rd_attention.hip AttnRoute): its pass argument; bits 0-1 of words[0]; the flags from bit 2 on
ATTN_PASSES = ("fwd", "bwd")
ATTN_FAMILIES = ("fp32", "one_b16", "mt_b16", "big")
ATTN_ROUTE_BITS = ("vec", "one_product", "wide")
# bit i of rd_debug_sensor_route's mask (csrc/rd_k1_route.h K1Route's flags, in declaration order); bits 8-9: the row-tile count rt
SENSOR_ROUTE_BITS = ("fused", "specialised", "infer", "coef", "tiles", "wgrad_stream")
# bit i of rd_debug_graph_beta_route's mask (csrc/rd_graph_beta.hip BetaFwdRoute / BetaBwdRoute); bits 8-23: the backward's chunk Tc
BETA_ROUTE_BITS = ("fwd_lds", "bwd_lds", "stage_v", "v1")
# bit i of rd_debug_gemm_route's flags; and what its words[0] packs (csrc/rd_gemm.hip GemmRoute)
GEMM_ROUTE_FLAGS = ("second", "rowsum", "batched", "scatter", "btiles", "a_aligned", "plan")
GEMM_FAMILIES = (None, "fp32", "bf16x3", "panel")
GEMM_MAPS = ("xcd", "rowmajor", "slice_xcd", "zgrid")
GEMM_TILES = ("64x64", "128x64", "128x128", "64x128", "64x160")
GEMM_PANEL_FORMS = ("small", "wide", "pc")
# bit i of rd_debug_head_route's words[0] (csrc/rd_head.hip HeadRoute); bits 8-9: the trailing launch's weight-gradient jobs
HEAD_ROUTE_BITS = ("narrow", "crit", "emb_lds", "focal")

_lib = None


def load():
    """Load the library once; raise RaindropHipError (never fall back) if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RaindropHipError(
            "libraindrop_hip.so not found at %s -- build it with `python -m raindrop_amd.build`; "
            "there is no CPU / eager fallback for the Raindrop hot path" % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64; it must be the ONE HIP runtime in the process
    # (streams and device pointers are shared with torch), so torch is imported before the dlopen.
    import torch  # noqa: F401
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise RaindropHipError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RaindropHipError("%s does not export %s (stale build?)" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    if lib.rd_version() != 1:
        raise RaindropHipError("ABI version mismatch: library %d, binding 1" % lib.rd_version())
    _lib = lib
    return lib


def call(name, *args):
    """Invoke an int-returning entry point and raise on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.rd_last_error().decode(errors="replace")
        kind = {-1: "RD_EINVAL", -2: "RD_EUNSUPPORTED"}.get(rc, "hipError %d" % rc)
        raise RaindropHipError("%s failed (%s): %s" % (name, kind, msg))


def shape(B, T, F, d_ob, d_pe=16, nhead=2, nhid=0, d_static=0, n_classes=2, max_len=None):
    return RdShape(B, T, F, d_ob, d_pe, nhead, nhid, d_static, n_classes, T if max_len is None else max_len)
