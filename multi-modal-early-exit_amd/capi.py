"""ctypes binding of libmmee_hip.so (include/mmee.h).  No torch types cross this boundary: pointers and sizes only.

The library is the product: if it cannot be loaded (not built, or no ROCm runtime) every entry point raises
``MMEEUnavailable`` — there is no CPU / PyTorch fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

ABI_VERSION = 4
MAX_ENCODER_EXITS = 64
EXIT_KIND = {"vision_avg": 0, "text_avg": 1, "text_visual_concat": 2}
FLAG_DENSE_ROWS = 1
FLAG_NO_EXIT = 2
FLAG_WHOLE_LAYERS = 4
FLAG_PROBE_ALWAYS = 8
FLAG_XPROBE = 16
FLAG_ONE_TERM = 32
FLAG_LOW_LATENCY = 64
FLAG_STREAM_RESULTS = 128
CRIT_MAX_CONFIDENCE, CRIT_ENTROPY, CRIT_PATIENCE, CRIT_MARGIN, CRIT_GATE = 0, 1, 2, 3, 4
RULE_PLAIN, RULE_STREAK, RULE_EITHER = 0, 1, 2
QUOTA_OFF, QUOTA_EXACT, QUOTA_AT_LEAST = 0, 1, 2
QUOTA_MODES = {"exact": QUOTA_EXACT, "at_least": QUOTA_AT_LEAST}
SEARCH_GRID, SEARCH_SAMPLED, SEARCH_MIXTURES = 0, 1, 2
SEARCH_REFERENCE, SEARCH_POLICY = 0, 1
RISK_BINOMIAL, RISK_HB = 0, 1
RISK_FIXED_SEQUENCE, RISK_BONFERRONI = 0, 1
# the columns of ee_exit_metrics' output rows (MMEE_METRIC_*)
(METRIC_ACCURACY, METRIC_BRIER, METRIC_NLL, METRIC_F1_MICRO, METRIC_F1_MACRO, METRIC_ECE, METRIC_AURC, METRIC_AVG_CONF,
 METRIC_COUNT) = range(9)
DT_F32, DT_F16, DT_BF16 = 0, 1, 2
CLOCK_STAMP_WORDS = 4096       # MMEE_CLOCK_STAMP_WORDS
ATTN_KERNEL_F32, ATTN_KERNEL_PAIR, ATTN_KERNEL_IDX, ATTN_KERNEL_IDX_NOBIAS = 0, 1, 2, 3
HEAD_FIT_SLAB = 32             # MMEE_HEAD_FIT_SLAB
MLP_HEAD_FIT_ROWS = 64         # MMEE_MLP_HEAD_FIT_ROWS
LTE_FIT_ROWS = 16              # MMEE_LTE_FIT_ROWS
LTE_LOSS_MSE, LTE_LOSS_BCE = 0, 1

_LIB_NAME = "libmmee_hip.so"
_LIB_PATH = os.environ.get("MMEE_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


class MMEEUnavailable(RuntimeError):
    pass


class MMEEError(RuntimeError):
    pass


class EEConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("hidden_size", C.c_int32), ("num_hidden_layers", C.c_int32), ("num_attention_heads", C.c_int32),
        ("intermediate_size", C.c_int32),
        ("vocab_size", C.c_int32), ("max_position_embeddings", C.c_int32), ("type_vocab_size", C.c_int32),
        ("pad_token_id", C.c_int32),
        ("max_2d_position_embeddings", C.c_int32), ("coordinate_size", C.c_int32), ("shape_size", C.c_int32),
        ("rel_pos_bins", C.c_int32), ("max_rel_pos", C.c_int32), ("rel_2d_pos_bins", C.c_int32),
        ("max_rel_2d_pos", C.c_int32),
        ("input_size", C.c_int32), ("patch_size", C.c_int32), ("num_channels", C.c_int32), ("num_labels", C.c_int32),
        ("layer_norm_eps", C.c_float),
        ("n_embedding_exits", C.c_int32), ("embedding_exits", C.c_int32 * 3),
        ("n_encoder_exits", C.c_int32), ("encoder_exit_layers", C.c_int32 * MAX_ENCODER_EXITS),
        ("exit_head_num_layers", C.c_int32), ("strategy", C.c_int32), ("criterion", C.c_int32),
        ("max_docs", C.c_int32), ("max_text_len", C.c_int32), ("precision", C.c_int32),
        ("arch", C.c_int32), ("use_abs_pos", C.c_int32), ("layer_scale", C.c_int32), ("use_mean_pooling", C.c_int32),
        ("use_lte", C.c_int32),
    ]


# every symbol include/mmee.h declares: (restype, argtypes)
_vp, _i32, _u32 = C.c_void_p, C.c_int32, C.c_uint32


class DebugEmbedArgs(C.Structure):
    """ee_debug_embed_args of include/mmee.h: device pointers (or None) and sizes."""
    _fields_ = ([(n, _vp) for n in ("input_ids", "attention_mask", "bbox", "position_ids", "token_type_ids")]
                + [(n, _i32) for n in ("B", "T", "G", "pad_id", "vocab", "max_2d", "max_pos", "type_vocab", "dense_rows", "H", "cs", "ss")]
                + [(n, _vp) for n in ("word", "type", "pos", "xtab", "ytab", "htab", "wtab", "inputs_embeds",
                                      "text_ln_g", "text_ln_b", "vis_ln_g", "vis_ln_b", "ln2_g", "ln2_b")]
                + [(n, C.c_float) for n in ("text_eps", "vis_eps", "eps2", "split_scale")]
                + [(n, _vp) for n in ("cls_token", "pos_embed", "vis_raw", "X", "Xs", "text_part", "vis_part", "cat_part",
                                      "pooled_text", "pooled_vis", "pooled_cat")])


class DebugXProbeArgs(C.Structure):
    """ee_debug_xprobe_args of include/mmee.h: device pointers (or None) and sizes."""
    _fields_ = ([("n_orig", _i32)] + [(n, _vp) for n in ("orig_doc_off", "pos", "x0", "y1", "masked")]
                + [(n, _i32) for n in ("n_docs", "max_docs")] + [(n, _vp) for n in ("doc_off", "doc_orig", "x_phys", "xs")]
                + [(n, _i32) for n in ("x_rows", "ctx_rows")] + [(n, _vp) for n in ("qc", "wk", "bk", "bv", "wv", "w1", "wx", "wy")]
                + [(n, _i32) for n in ("H", "heads", "bins1", "bins2", "max_rel_pos", "max_rel_2d_pos", "max_pos", "max_coord", "index_form", "cus")]
                + [(n, _vp) for n in ("ctx", "u_out", "s0_out", "cvec_out", "order_out")])


class DebugHeadOutArgs(C.Structure):
    """ee_debug_head_out_args of include/mmee.h: device pointers (or None) and sizes."""
    _fields_ = [("in_", _vp), ("in_rows", _i32), ("ld", _i32), ("gather", _vp), ("W", _vp), ("b", _vp), ("H", _i32), ("Ko", _i32), ("n_docs", _vp),
                ("max_docs", _i32), ("out", _vp), ("lte_in", _vp), ("lte_rows", _i32), ("lte_ld", _i32), ("lte_gather", _vp),
                ("lte_split_inv", C.c_float), ("lte_w", _vp), ("lte_b", _vp), ("lte_out", _vp)]


class DebugExitDecideArgs(C.Structure):
    """ee_debug_exit_decide_args of include/mmee.h: device pointers (or None), this exit's scalars and sizes."""
    _fields_ = ([(n, _i32) for n in ("mode", "rule", "criterion")] + [(n, _vp) for n in ("pol_logits", "head_logits")]
                + [(n, _i32) for n in ("K", "Kh")] + [("lte_score", _vp), ("thr", C.c_double), ("temp", C.c_double)]
                + [(n, _i32) for n in ("patience", "by_pointer", "exit_index", "is_final", "no_exit", "B")]
                + [(n, _vp) for n in ("counts", "doc_orig", "doc_off", "x_phys", "prev", "run", "n_counts", "n_doc_orig", "n_doc_off", "n_x_src",
                                      "n_meta_src", "out_logits", "out_exit", "out_conf", "out_all_logits", "out_all_crit", "out_head_logits",
                                      "out_head_crit", "meta_old", "meta_new", "row_src")])


class DebugExitQuotaArgs(C.Structure):
    """ee_debug_exit_quota_args of include/mmee.h: the decide call's arguments, this exit's quota and mode, the two device arrays the ranking fills."""
    _fields_ = [("decide", DebugExitDecideArgs), ("quota", _i32), ("quota_mode", _i32), ("crit", _vp), ("rank", _vp)]


class DebugExitAuditArgs(C.Structure):
    """ee_debug_exit_audit_args of include/mmee.h: the decide call's arguments, the audit's cut, seed and slot base, the device array of delivered marks."""
    _fields_ = [("decide", DebugExitDecideArgs), ("cut", C.c_uint64), ("seed", _u32), ("slot_base", _i32), ("delivered", _vp)]


def audit_cut(fraction: float) -> int:
    """cut = floor(fraction 2^32 + 0.5) of include/mmee.h's audited exits; the fraction must lie in [0, 1]."""
    f = float(fraction)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"audit fraction {fraction!r} outside [0, 1]")
    return int(math.floor(f * 4294967296.0 + 0.5))


class DebugAuditTallyArgs(C.Structure):
    """ee_debug_audit_tally_args of include/mmee.h: the final stage, the audit's marks and selection, the call's results; device pointers."""
    _fields_ = ([("pol_logits", _vp)] + [(n, _i32) for n in ("pol_rows", "K", "B", "E1")] + [("temp", C.c_double)]
                + [(n, _vp) for n in ("counts", "doc_orig", "delivered", "out_logits", "out_exit")]
                + [("cut", C.c_uint64), ("seed", _u32), ("slot_base", _i32), ("tally", _vp)])


class DebugControllerStepArgs(C.Structure):
    """ee_debug_controller_step_args of include/mmee.h: the path, the controller's parameters, state / tally / thresholds / log on the device."""
    _fields_ = ([("path", _vp), ("V", _i32), ("E1", _i32)] + [(n, C.c_double) for n in ("sign", "alpha", "gamma")]
                + [(n, _vp) for n in ("state", "tally", "thr", "log")] + [("log_cap", _i32)])


CTL_STATE_WORDS = 5            # p (float64 bits), calls, steps, sampled_sum, disagree_sum
CTL_MAX_E1 = 64


def controller_log_words(E1: int) -> int:
    """64-bit words of a controller log row (include/mmee.h): call, p before, p after, sampled, disagree, delivered[E], agree[E], thresholds[E1]."""
    return 5 + 2 * (E1 - 1) + E1


class DebugDeadlineCheckArgs(C.Structure):
    """ee_debug_deadline_check_args of include/mmee.h: the check launch of a deadline call with an injected clock; state / thr / row on the device."""
    _fields_ = ([("E1", _i32), ("exit_index", _i32), ("khz", _u32), ("sign", C.c_double)]
                + [(n, C.c_uint64) for n in ("call", "budget_ns", "eta_ns", "host_word", "now", "t0")] + [(n, _vp) for n in ("state", "thr", "row")])


DEADLINE_NONE = 2 ** 64 - 1    # MMEE_DEADLINE_NONE: stamp, never cut by the clock
DEADLINE_OFF = 2 ** 64 - 2     # MMEE_DEADLINE_OFF: remove the deadline
DL_STATE_WORDS = 3             # t0 (ticks), cut_exit, cut_by


def deadline_log_words(E1: int) -> int:
    """64-bit words of a deadline log row (include/mmee.h): call, budget_ns, cut_exit, cut_by, elapsed_ns[E1]."""
    return 4 + E1


class DebugExitEnsembleArgs(C.Structure):
    """ee_debug_exit_ensemble_args of include/mmee.h: device pointers (or None), this exit's temperature and sizes."""
    _fields_ = ([("pol_logits", _vp)] + [(n, _i32) for n in ("pol_rows", "K", "E1", "exit_index", "B")] + [("temp", C.c_double), ("by_pointer", _i32)]
                + [(n, _vp) for n in ("counts", "doc_orig", "w", "b", "state", "out")] + [("out_rows", _i32)])


class DebugRowsOutArgs(C.Structure):
    """ee_debug_rows_out_args of include/mmee.h: device pointers (or None) and sizes."""
    _fields_ = ([("which", _i32), ("X", _vp), ("x_rows", _i32), ("H", _i32), ("split_inv", C.c_float)]
                + [(n, _vp) for n in ("x_phys", "doc_orig", "n_docs")] + [(n, _i32) for n in ("max_docs", "B", "T", "Pv")]
                + [(n, _vp) for n in ("text_dst", "ntext", "doc_off", "out")] + [("out_rows", _i32)])


class DebugPatchProjectArgs(C.Structure):
    """ee_debug_patch_project_args of include/mmee.h: device pointers (or None) and sizes."""
    _fields_ = ([(n, _vp) for n in ("pixel_values", "weight", "bias")] + [(n, _i32) for n in ("B", "C", "R", "P", "H", "form")]
                + [(n, _vp) for n in ("out", "a_split_out")] + [("err_flag_out", C.POINTER(_i32))])


class DebugGemmRoutesArgs(C.Structure):
    """ee_debug_gemm_routes_args of include/mmee.h: device pointers (or None), sizes and scales."""
    _fields_ = ([(n, _vp) for n in ("A", "W", "bias", "resid", "Cout")] + [(n, _i32) for n in ("M", "N", "K", "epi", "out_split")]
                + [(n, C.c_float) for n in ("a_scale", "w_scale", "out_scale", "resid_scale")]
                + [("row_src", _vp), ("rows_A", _i32), ("resid_row_src", _vp), ("rows_resid", _i32)]
                + [(n, _i32) for n in ("route", "role_tag", "probe", "terms", "k_splits")] + [("split_stride", C.c_size_t), ("scale_cols", _i32),
                                                                                             ("scale", C.c_float), ("col_scale", _vp)]
                + [(n, _i32) for n in ("max_m", "m_on_device", "iters")] + [("err_flag_out", C.POINTER(_i32))])


class DebugGemmF32Args(C.Structure):
    """ee_debug_gemm_f32_args of include/mmee.h: device pointers (or None), sizes and the epilogue operands."""
    _fields_ = ([(n, _vp) for n in ("A", "W", "bias", "resid", "Cout")] + [(n, _i32) for n in ("M", "N", "K", "epi", "staging", "use_queue")]
                + [("row_src", _vp), ("rows_A", _i32), ("resid_row_src", _vp), ("rows_resid", _i32), ("scale_cols", _i32), ("scale", C.c_float),
                   ("col_scale", _vp)] + [(n, _i32) for n in ("max_m", "m_on_device", "wgs_per_cu")])


class CascadeDesc(C.Structure):
    """ee_cascade_desc of include/mmee.h: one array of ee_cascade_gather (device pointers, bytes per row)."""
    _fields_ = [("src", _vp), ("dst", _vp), ("row_bytes", C.c_int64)]


CASCADE_MAX_ARRAYS = 8         # descriptors one ee_cascade_gather launch takes

SYMBOLS = {
    "ee_cascade_select": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp, _vp]),
    "ee_cascade_gather": (C.c_int, [C.POINTER(CascadeDesc), _i32, _vp, _vp, _i32, _vp]),
    "ee_cascade_merge": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ee_create": (C.c_int, [C.POINTER(EEConfig), C.POINTER(_vp)]),
    "ee_destroy": (C.c_int, [_vp]),
    "ee_last_error": (C.c_char_p, [_vp]),
    "ee_load_tensor": (C.c_int, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i32, _i32, _i32]),
    "ee_finalize": (C.c_int, [_vp]),
    "ee_num_expected_tensors": (_i32, [_vp]),
    "ee_expected_tensor_name": (C.c_char_p, [_vp, _i32]),
    "ee_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(C.c_double),
                             C.POINTER(C.c_double), _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_embedding_inputs": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ee_forward_vision": (C.c_int, [_vp, _vp, _i32, C.POINTER(C.c_double), C.POINTER(C.c_double), _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_graph_capture": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i32)]),
    "ee_graph_launch": (C.c_int, [_vp, _i32, C.POINTER(C.c_double), C.POINTER(C.c_double), _vp]),
    "ee_graph_destroy": (C.c_int, [_vp, _i32]),
    "ee_stream_next": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(C.POINTER(_i32)), C.POINTER(_i32)]),
    "ee_last_stage_counts": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), _i32, C.POINTER(_i32), _vp]),
    "ee_last_flops": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), _vp]),
    "ee_last_layer_plan": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32, C.POINTER(C.c_double), _vp]),
    "ee_low_latency_k_splits": (_i32, [_i32, _i32, _i32, _i32]),
    "ee_last_k_splits": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "ee_set_probe_mask": (C.c_int, [_vp, _i32, C.c_uint64]),
    "ee_set_criterion": (C.c_int, [_vp, _i32]),
    "ee_set_patience": (C.c_int, [_vp, _i32]),
    "ee_set_patience_vector": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "ee_set_exit_rule": (C.c_int, [_vp, _i32]),
    "ee_set_ensemble": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ee_has_ensemble": (C.c_int, [_vp]),
    "ee_set_quotas": (C.c_int, [_vp, C.POINTER(_i32), _i32, _i32]),
    "ee_has_quotas": (C.c_int, [_vp]),
    "ee_quota_scan": (C.c_int, [_vp, C.c_double, _i32, _i32, C.POINTER(_i32), _i32, C.POINTER(C.c_double), _i32, _vp, _vp, _vp, _vp]),
    "ee_debug_exit_quota": (C.c_int, [C.POINTER(DebugExitQuotaArgs), _vp]),
    "ee_set_audit": (C.c_int, [_vp, C.c_uint64, _u32, _i32]),
    "ee_has_audit": (C.c_int, [_vp]),
    "ee_audit_selected": (C.c_int, [C.c_uint64, _u32, _i32]),
    "ee_debug_exit_audit": (C.c_int, [C.POINTER(DebugExitAuditArgs), _vp]),
    "ee_set_controller": (C.c_int, [_vp, C.POINTER(C.c_double), _i32, C.c_double, C.c_double, C.c_double, _u32, _i32]),
    "ee_has_controller": (C.c_int, [_vp]),
    "ee_controller_state": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_double), _vp]),
    "ee_controller_log": (C.c_int, [_vp, _vp, _i32, C.POINTER(_i32), _vp]),
    "ee_rolling_control": (C.c_int, [_vp, C.c_double, _vp, _i32, _i32, _vp, _i32, C.c_uint64, _u32, C.c_double, C.c_double, C.c_double, _i32, _vp,
                                     _vp, _vp, _vp]),
    "ee_debug_audit_tally": (C.c_int, [C.POINTER(DebugAuditTallyArgs), _vp]),
    "ee_debug_controller_step": (C.c_int, [C.POINTER(DebugControllerStepArgs), _vp]),
    "ee_set_deadline": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "ee_set_deadline_log": (C.c_int, [_vp, _i32]),
    "ee_has_deadline": (C.c_int, [_vp]),
    "ee_request_cut": (C.c_int, [_vp]),
    "ee_deadline_log": (C.c_int, [_vp, _vp, _i32, C.POINTER(_i32), _vp]),
    "ee_debug_deadline_check": (C.c_int, [C.POINTER(DebugDeadlineCheckArgs), _vp]),
    "ee_suggest_probe_mask": (C.c_int, [_vp, _u32, C.POINTER(C.c_uint64), _vp]),
    "ee_clock_stamp": (C.c_int, [_vp, _vp]),
    "ee_set_inputs_embeds": (C.c_int, [_vp, _vp]),
    "ee_set_hidden_states_out": (C.c_int, [_vp, _vp]),
    "ee_set_head_mask": (C.c_int, [_vp, _vp]),
    "ee_set_attentions_out": (C.c_int, [_vp, _vp]),
    "ee_policy_scan": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp]),
    "ee_criterion_scan": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp]),
    "ee_patience_scan": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ee_lte_scan": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.POINTER(C.c_double), _vp, _vp, _vp, _vp]),
    "ee_gate_scan": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp]),
    "ee_rule_scan": (C.c_int, [_vp, C.c_double, _vp, _i32, _i32, _i32, C.POINTER(C.c_double), C.POINTER(_i32), _i32, _vp, _vp, _vp, _vp, _vp]),
    "ee_rule_sweep": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, C.POINTER(_i32), _i32, _i32, _vp, _vp, _vp, _vp]),
    "ee_patience_sweep": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "ee_pack_results": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "ee_unpack_results": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ee_threshold_sweep": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "ee_threshold_search": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, C.c_int64, C.c_uint64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_threshold_search_cost": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_int64, C.c_uint64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp]),
    "ee_threshold_refine": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_threshold_refine_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32]),
    "ee_risk_control": (C.c_int, [_vp, C.c_double, _vp, _vp, _vp, _i32, _i32, _vp, _i32, C.c_double, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp, _vp]),
    "ee_binomial_bounds": (C.c_int, [C.POINTER(_i32), C.POINTER(_i32), _i32, C.c_double, _vp, _vp, _vp]),
    "ee_msp_table": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ee_csf_table": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ee_gate_table": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ee_ensemble_logits": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ee_ensemble_fit": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp]),
    "ee_ensemble_fit_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32]),
    "ee_exit_metrics": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ee_debug_gemm": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ee_debug_gemm_split": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, C.c_float, C.c_float, C.c_float, _vp,
                                      _i32, _i32, C.POINTER(C.c_float), _vp]),
    "ee_debug_gemm_split_resid": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_float, C.c_float, C.c_float, _vp, _i32, _vp, _i32,
                                            _i32, _i32, C.POINTER(C.c_float), _vp]),
    "ee_debug_gemm_routes": (C.c_int, [C.POINTER(DebugGemmRoutesArgs), C.POINTER(C.c_float), _vp]),
    "ee_debug_gemm_f32": (C.c_int, [C.POINTER(DebugGemmF32Args), _vp]),
    "ee_debug_attn_stamps": (C.c_int, [_vp]),
    "ee_debug_attention": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                     _i32, _i32, _i32, _vp, C.POINTER(_i32), _vp]),
    "ee_debug_prep": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                C.POINTER(_i32), _vp]),
    "ee_debug_embed": (C.c_int, [C.POINTER(DebugEmbedArgs), C.POINTER(_i32), _vp]),
    "ee_debug_ln_rows": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, C.c_float, _vp, C.c_float, _i32, C.c_size_t, _vp, _vp, _vp, C.c_float,
                                   C.POINTER(_i32), _vp]),
    "ee_debug_vision_pool": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_float, _i32, _i32, _i32, _vp, _vp, _vp]),
    "ee_debug_xprobe": (C.c_int, [C.POINTER(DebugXProbeArgs), C.POINTER(_i32), _vp]),
    "ee_debug_head_out": (C.c_int, [C.POINTER(DebugHeadOutArgs), _vp]),
    "ee_debug_exit_decide": (C.c_int, [C.POINTER(DebugExitDecideArgs), _vp]),
    "ee_debug_exit_ensemble": (C.c_int, [C.POINTER(DebugExitEnsembleArgs), _vp]),
    "ee_debug_rows_out": (C.c_int, [C.POINTER(DebugRowsOutArgs), _vp]),
    "ee_debug_patch_project": (C.c_int, [C.POINTER(DebugPatchProjectArgs), _vp]),
    "ee_debug_split_rows": (C.c_int, [_vp, _i32, _i32, C.c_float, _vp, C.POINTER(_i32), _vp]),
    "ee_debug_split_weight": (C.c_int, [_vp, _i32, _i32, _vp, C.POINTER(C.c_float), _vp]),
    "ee_temperature_fit": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_head_fit": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp]),
    "ee_head_fit_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "ee_debug_head_lossgrad": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp]),
    "ee_head_fit_gate": (C.c_int, [_vp, _vp, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp]),
    "ee_debug_head_gate_lossgrad": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp]),
    "ee_mlp_head_fit": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_mlp_head_fit_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "ee_debug_mlp_head_lossgrad": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp]),
    "ee_head_fit_distill": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, C.c_double, _i32, _i32, _vp,
                                      C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_debug_head_distill_lossgrad": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]),
    "ee_mlp_head_fit_distill": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, C.c_double, _i32, _i32,
                                          _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_debug_mlp_head_distill_lossgrad": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                                     _vp]),
    "ee_head_fit_weighted": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, C.c_double, _i32, _i32, _vp,
                                       C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_head_fit_weighted_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "ee_debug_head_weighted_lossgrad": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                                  _vp]),
    "ee_mlp_head_fit_weighted": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, C.c_double, _i32,
                                           _i32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_mlp_head_fit_weighted_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32]),
    "ee_debug_mlp_head_weighted_lossgrad": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp,
                                                      _vp, _vp]),
    "ee_mlp_head_fit_gate": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp]),
    "ee_mlp_head_fit_gate_weighted": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _i32, _vp, C.c_size_t, _vp, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ee_debug_mlp_head_gate_lossgrad": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp]),
    "ee_debug_mlp_head_gate_weighted_lossgrad": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp]),
    "ee_lte_fit": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp,
                             _vp, _vp, _vp]),
    "ee_lte_fit_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32]),
    "ee_debug_lte_lossgrad": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp]),
    "ee_lte_targets": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ee_lte_scores": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ee_preprocess_images": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp]),
    "ee_preprocess_workspace_bytes": (C.c_size_t, [_i32, _i32, _i32]),
    "ee_collate_pad": (C.c_int, [_vp, _vp, _vp, _i32, _i32, C.c_int64, _vp, _vp, _vp, _vp]),
    "ee_bucket_lut": (C.c_int, [_i32, _i32, _i32, _vp]),
    "ee_profile": (C.c_int, [_vp, _i32]),
    "ee_profile_read": (C.c_int, [_vp, _i32, C.c_char_p, _i32, C.POINTER(C.c_double), C.POINTER(_i32)]),
}

_lib: Optional[C.CDLL] = None


def lib_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises MMEEUnavailable with the reason when it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise MMEEUnavailable(
            f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C {os.path.dirname(_LIB_PATH)}/csrc`).  There is no CPU fallback.")
    try:
        lib = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # e.g. ROCm runtime missing
        raise MMEEUnavailable(f"cannot load {_LIB_PATH}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise MMEEUnavailable(f"{_LIB_PATH} does not export {name} (stale build?)") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error(handle=None) -> str:
    msg = load().ee_last_error(handle)
    return msg.decode() if msg else ""


def check(rc: int, handle=None, what: str = ""):
    if rc != 0:
        raise MMEEError(f"{what}: {last_error(handle)}" if what else last_error(handle))
