"""ctypes binding of libbyolo.so (include/byolo.h).  No fallback: if the HIP library is missing
the import fails loudly -- there is no CPU / eager path in the product."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BYOLO_LIB: load another build of the same library (the timing-ablation builds of csrc/build.py --ablate)
LIB_PATH = os.environ.get("BYOLO_LIB") or os.path.join(_HERE, "libbyolo.so")

OK, ERR_ARG, ERR_STATE, ERR_HIP, ERR_NOMEM, ERR_RANGE = 0, -1, -2, -3, -4, -5
DET_STANDARD, DET_ALEATORIC, DET_EPISTEMIC = 0, 1, 2
NMS_AGNOSTIC, NMS_TWO_CLASS, NMS_PER_CLASS = 0, 1, 2
NMS_MAX_CLASSES = 128          # BYOLO_NMS_MAX_CLASSES
T_LADDER_MAX, T_LADDER_MAX_CLASSES = 16, 48      # BYOLO_T_LADDER_MAX, BYOLO_T_LADDER_MAX_CLASSES
NORM_BN, NORM_DROPOUT = 1, 2
AUG_SATURATION, AUG_BRIGHTNESS, AUG_HUE = 1, 2, 3
AUG_COLORED_SALT_N_PEPPER, AUG_SALT_N_PEPPER, AUG_GAUSSIAN = 1, 2, 3


class ByoloError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libbyolo error %d: %s" % (code, msg))
        self.code = code


class Cfg(ctypes.Structure):
    _fields_ = [("img_h", ctypes.c_int32), ("img_w", ctypes.c_int32), ("img_c", ctypes.c_int32),
                ("cls_cnt", ctypes.c_int32), ("drop_prob", ctypes.c_float), ("max_out", ctypes.c_int32),
                ("iou_thresh", ctypes.c_float), ("nms_mode", ctypes.c_int32), ("keep_all_outputs", ctypes.c_int32)]


class PlanOpts(ctypes.Structure):
    """include/byolo.h byolo_plan_opts (field for field; tests/test_abi.py compares the two)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "struct_bytes", "graphs", "serialize_convs", "serialize_heads", "dedup", "lowmain", "kx3", "p1", "b2b", "kx3_wide", "wino_split", "wino_split_min_c",
        "wino_split_bn", "wino_split_rounds", "winograd", "wino_fused", "stream1x1", "gemm_stream", "ksplit", "streamk",
        "plain_epilogue", "wshift_per_layer", "nms_general", "wino_split_persist", "wino_split_feed")] + [(n, ctypes.c_float) for n in (
        "wino_split_min_gflop", "wino_split_chunk_mb", "wino_min_gflop", "wino_chunk_mb", "wino_min_ratio")]


class AugPlan(ctypes.Structure):
    """include/byolo.h byolo_aug_plan (field for field; tests/test_train_feed_cpu.py compares the two)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("y0", "x0", "ch", "cw", "row0", "rescale", "flip", "blur_k", "color_op", "noise_op")] + \
               [("color_param", ctypes.c_float), ("noise_param", ctypes.c_float), ("noise_key", ctypes.c_uint64)]


EVAL_MAX_GT, EVAL_MAX_UNC, EVAL_RECORD_HEAD = 1024, 16, 7          # BYOLO_EVAL_*


class EvalCfg(ctypes.Structure):
    """include/byolo.h byolo_eval_cfg (field for field; tests/test_eval_cpu.py compares the two)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_bytes", "row_len", "obj_idx", "cls_start_idx", "cls_cnt", "n_unc")] + \
               [("unc_cols", ctypes.c_int32 * EVAL_MAX_UNC), ("iou_thresh", ctypes.c_float), ("min_score", ctypes.c_float)]


EVAL_LOC_WORDS, EVAL_LOC_MAX_LAYERS, EVAL_LOC_MAX_PRIORS = 6, 8, 16      # BYOLO_EVAL_LOC_*


class EvalLocCfg(ctypes.Structure):
    """include/byolo.h byolo_eval_loc_cfg (field for field; tests/test_eval_loc_cpu.py compares the two)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_bytes", "layer_col", "prior_col", "n_layers")] + \
               [(n, ctypes.c_int32 * EVAL_LOC_MAX_LAYERS) for n in ("lh", "lw", "n_priors")] + \
               [(n, (ctypes.c_float * EVAL_LOC_MAX_PRIORS) * EVAL_LOC_MAX_LAYERS) for n in ("prior_w", "prior_h")]


EVAL_LADDER_MAX = 16                                                     # BYOLO_EVAL_LADDER_MAX


class EvalLadderCfg(ctypes.Structure):
    """include/byolo.h byolo_eval_ladder_cfg (field for field; tests/test_eval_ladder_cpu.py compares the two)."""
    _fields_ = [("struct_bytes", ctypes.c_int32), ("n_thr", ctypes.c_int32), ("thresholds", ctypes.c_float * EVAL_LADDER_MAX)]


EVAL_SUBSETS_MAX = 16                                                    # BYOLO_EVAL_SUBSETS_MAX


class EvalSubsetsCfg(ctypes.Structure):
    """include/byolo.h byolo_eval_subsets_cfg (field for field; tests/test_eval_subsets_cpu.py compares the two)."""
    _fields_ = [("struct_bytes", ctypes.c_int32), ("n_subsets", ctypes.c_int32), ("lo", ctypes.c_float * EVAL_SUBSETS_MAX),
                ("hi", ctypes.c_float * EVAL_SUBSETS_MAX), ("img_h", ctypes.c_float), ("ignore_thresh", ctypes.c_float),
                ("height_slack", ctypes.c_float), ("ignore_other_classes", ctypes.c_int32)]


PDQ_MAX_DET, PDQ_MAX_FRAME, PDQ_RECORD_BYTES = 1024, 4096, 56             # BYOLO_PDQ_*


class EvalPdqCfg(ctypes.Structure):
    """include/byolo.h byolo_eval_pdq_cfg (field for field; tests/test_pdq_cpu.py compares the two)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_bytes", "var", "ale_col", "epi_col", "img_h", "img_w")] + \
               [("min_score", ctypes.c_float), ("reserved", ctypes.c_int32)] + [(n, ctypes.c_double) for n in ("p_min", "eps", "var_floor")]


class EvalSummary(ctypes.Structure):
    """include/byolo.h byolo_eval_summary."""
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_bytes", "overflow", "record_words", "reserved")] + \
               [(n, ctypes.c_int64) for n in ("n_records", "n_seen", "n_images")]


VOTE_NONE, VOTE_ALE, VOTE_EPI, VOTE_TOTAL = 0, 1, 2, 3            # BYOLO_VOTE_*


class VoteCfg(ctypes.Structure):
    """include/byolo.h byolo_vote_cfg (field for field; tests/test_box_vote_cpu.py compares the two)."""
    _fields_ = [("struct_bytes", ctypes.c_int32), ("var", ctypes.c_int32)] + \
               [(n, ctypes.c_float) for n in ("sigma_t", "iou_min", "min_score", "var_floor")] + \
               [("ale_col", ctypes.c_int32), ("epi_col", ctypes.c_int32)]


SOFT_NMS_LINEAR, SOFT_NMS_GAUSSIAN = 0, 1                          # BYOLO_SOFT_NMS_*
SOFT_NMS_RESIDENT = 8192       # BYOLO_SOFT_NMS_RESIDENT: candidates of one (image, class) the soft-NMS holds in registers


class SoftNmsCfg(ctypes.Structure):
    """include/byolo.h byolo_soft_nms_cfg (field for field; tests/test_soft_nms_cpu.py compares the two)."""
    _fields_ = [("struct_bytes", ctypes.c_int32), ("method", ctypes.c_int32)] + \
               [(n, ctypes.c_float) for n in ("sigma", "iou_soft", "iou_hard", "min_score")]


VAR_RECAL_ALE, VAR_RECAL_EPI, VAR_RECAL_TOTAL = 1, 2, 3              # BYOLO_VAR_RECAL_* (target)
VAR_RECAL_SCALE, VAR_RECAL_POWER = 0, 1                             # (method)
VAR_RECAL_FITTED, VAR_RECAL_SCALE_FALLBACK, VAR_RECAL_IDENTITY, VAR_RECAL_EMPTY = 0, 1, 2, 3      # (status of a fitted segment)
VAR_RECAL_TABLE_BYTES, VAR_RECAL_FIT_WORDS = 8192, 10


class VarRecalCfg(ctypes.Structure):
    """include/byolo.h byolo_var_recal_cfg (field for field; tests/test_var_recal_cpu.py compares the two)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_bytes", "kind", "target", "n_layers")] + \
               [("n_priors", ctypes.c_int32 * EVAL_LOC_MAX_LAYERS)] + \
               [(n, ((ctypes.c_double * 4) * EVAL_LOC_MAX_PRIORS) * EVAL_LOC_MAX_LAYERS) for n in ("a", "b")]


SCORE_RECAL_MAX_K, SCORE_RECAL_MAX_GROUPS, SCORE_RECAL_TABLE_BYTES, SCORE_RECAL_FIT_WORDS = 8, 80, 5120, 36      # BYOLO_SCORE_RECAL_*
SCORE_RECAL_BY_ALL, SCORE_RECAL_BY_CLASS = 0, 1
SCORE_RECAL_F_BIAS, SCORE_RECAL_F_LOGIT, SCORE_RECAL_F_LOG_HEIGHT, SCORE_RECAL_F_COL_ID, SCORE_RECAL_F_COL_LOG = 0, 1, 2, 3, 4
SCORE_RECAL_FIT, SCORE_RECAL_IDENTITY, SCORE_RECAL_EMPTY = 0, 1, 2                                              # (status of a fitted segment)


class ScoreRecalCfg(ctypes.Structure):
    """include/byolo.h byolo_score_recal_cfg (field for field; tests/test_score_recal_cpu.py compares the two)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_bytes", "kind", "cls_cnt", "by", "K")] + \
               [(n, ctypes.c_int32 * SCORE_RECAL_MAX_K) for n in ("feat_kind", "feat_col")] + [("reserved", ctypes.c_int32)] + \
               [("w", (ctypes.c_double * SCORE_RECAL_MAX_K) * SCORE_RECAL_MAX_GROUPS)]


TTA_MAX_VIEWS = 8                                                        # BYOLO_TTA_MAX_VIEWS


class TtaSupportCfg(ctypes.Structure):
    """include/byolo.h byolo_tta_support_cfg (field for field; tests/test_tta_cpu.py compares the two)."""
    _fields_ = [("struct_bytes", ctypes.c_int32), ("n_views", ctypes.c_int32), ("iou_min", ctypes.c_float), ("min_score", ctypes.c_float),
                ("view_off", ctypes.c_int32 * (TTA_MAX_VIEWS + 1))]


_i32, _i64, _f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
_vp, _cp, _sz, _u64 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64
_P = ctypes.POINTER

# name -> (restype, argtypes); this table IS the Python view of include/byolo.h and is checked against
# the header by tests/test_abi.py
PROTOTYPES = {
    "byolo_create": (_i32, [_P(Cfg), _i32, _P(_vp)]),
    "byolo_destroy": (_i32, [_vp]),
    "byolo_last_error": (_cp, [_vp]),
    "byolo_version": (_cp, []),
    "byolo_add_conv": (_i32, [_vp, _cp, _i32, _i32, _i32, _i32]),
    "byolo_add_residual": (_i32, [_vp, _i32]),
    "byolo_add_route": (_i32, [_vp, _P(_i32), _i32]),
    "byolo_add_upsample": (_i32, [_vp]),
    "byolo_add_stack": (_i32, [_vp, _i32]),
    "byolo_add_detection": (_i32, [_vp, _cp, _i32, _P(_f32)]),
    "byolo_mark_backbone_end": (_i32, [_vp]),
    "byolo_num_params": (_i32, [_vp]),
    "byolo_param_info": (_i32, [_vp, _i32, _P(_cp), _P(_i32), _P(_i64)]),
    "byolo_set_param": (_i32, [_vp, _cp, _vp, _i64]),
    "byolo_get_param": (_i32, [_vp, _cp, _vp, _i64]),
    "byolo_finalize": (_i32, [_vp]),
    "byolo_num_layers": (_i32, [_vp]),
    "byolo_num_boxes": (_i32, [_vp, _P(_i64), _P(_i32)]),
    "byolo_workspace_bytes": (_i32, [_vp, _i32, _i32, _P(_sz)]),
    "byolo_forward": (_i32, [_vp, _vp, _i32, _i32, _u64, _i32, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "byolo_num_dropout": (_i32, [_vp]),
    "byolo_mask_layout": (_i32, [_vp, _i32, _i32, _i32, _P(_i64), _P(_i64)]),
    "byolo_set_async": (_i32, [_vp, _i32]),
    "byolo_status": (_i32, [_vp, _vp, _P(ctypes.c_uint32), _P(_i32)]),
    "byolo_clear_status": (_i32, [_vp, _vp]),
    "byolo_precision_note": (_cp, [_vp]),
    "byolo_set_first_image": (_i32, [_vp, _i64]),
    "byolo_max_images": (_i32, [_vp, _i32, _P(_i32)]),
    "byolo_layer_output": (_i32, [_vp, _i32, _P(_vp), _P(_i64)]),
    "byolo_copy_layer_output": (_i32, [_vp, _i32, _vp, _i64, _vp]),
    "byolo_set_precision": (_i32, [_vp, _i32]),
    "byolo_get_precision": (_i32, [_vp]),
    "byolo_decode": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _P(_f32), _i32, _vp, _i64, _i64, _vp]),
    "byolo_epistemic_stats": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "byolo_decode_ladder": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _P(_f32), _i32, _P(_i32), _i32, _vp, _i64, _i64, _vp]),
    "byolo_forward_ladder": (_i32, [_vp, _i32, _i32, _P(_i32), _i32, _vp, _vp]),
    "byolo_nms_workspace_bytes": (_sz, [_i32, _i64]),
    "byolo_nms_workspace_bytes_ex": (_sz, [_i32, _i64, _i32, _i32]),
    "byolo_nms_class_counts": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "byolo_sort_nms": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _sz, _vp, _vp, _vp, _vp]),
    "byolo_calibrate_bn": (_i32, [_vp, _vp, _i32, _vp, _sz, _vp]),
    "byolo_set_profiling": (_i32, [_vp, _i32]),
    "byolo_resume_profiling": (_i32, [_vp, _i32]),
    "byolo_stage_ms": (_i32, [_vp, _P(_f32)]),
    "byolo_set_profile_depth": (_i32, [_vp, _i32]),
    "byolo_select_profile": (_i32, [_vp, _i32]),
    "byolo_num_steps": (_i32, [_vp]),
    "byolo_step_profile": (_i32, [_vp, _i32, _P(_i32), _P(_i32), _P(_i64), _P(_f32), _P(ctypes.c_double)]),
    "byolo_step_split": (_i32, [_vp, _i32, _P(_i32), _P(_i32)]),
    "byolo_flops": (_i32, [_vp, _i32, _i32, _P(ctypes.c_double)]),
    "byolo_crc32c": (ctypes.c_uint32, [_vp, _sz]),
    "byolo_abi_version": (_i32, []),
    "byolo_get_plan_opts": (_i32, [_vp, _P(PlanOpts)]),
    "byolo_set_plan_opts": (_i32, [_vp, _P(PlanOpts)]),
    "byolo_graph_stats": (_i32, [_vp, _P(_i32), _P(_i64), _P(_i64), _P(_i64)]),
    "byolo_plan_num": (_i32, [_vp, _i32, _i32, _i32, _P(_i32), _P(_i32), _P(_i64)]),
    "byolo_plan_step": (_i32, [_vp, _i32, _P(_i32), _P(_i32), _P(_i32), _P(_i32)]),
    "byolo_plan_tensor": (_i32, [_vp, _i32, _P(_i64), _P(_i64), _P(_i32)]),
    "byolo_set_tshard": (_i32, [_vp, _i32, _i32]),
    "byolo_finish_tshard": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "byolo_normalize_u8": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "byolo_copy_status": (_i32, [_vp, _vp, _vp]),
    "byolo_augment_batch": (_i32, [_vp, _vp, _i32, _i32, _i32, _i64, _P(AugPlan), _i32, _i32, _vp, _vp]),
    "byolo_png_decode_batch": (_i32, [_P(_vp), _P(_sz), _i32, _i32, _i32, _i32, _vp, _i32, _P(_i32), _P(_i32)]),
    "byolo_feed_records": (_i32, [_P(_i32), _P(_i64), _P(_i64), _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _P(_i32), _P(_i32)]),
    "byolo_encode_gt": (_i32, [_vp, _i32, _P(_i32), _P(ctypes.c_double), _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "byolo_encode_gt_workspace_bytes": (_sz, [_i32, _i32]),
    "byolo_loss_workspace_bytes": (_sz, []),
    "byolo_loss": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _sz, _vp]),
    "byolo_format_ecp_json": (_i64, [_i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P(_cp), _i32, _vp, _sz]),
    "byolo_trainer_create": (_i32, [_vp, _i32, _P(_vp)]),
    "byolo_trainer_destroy": (_i32, [_vp]),
    "byolo_trainer_set_fallback": (_i32, [_vp, _vp]),
    "byolo_trainer_workspace_bytes": (_i32, [_vp, _i32, _P(_sz)]),
    "byolo_trainer_step": (_i32, [_vp, _vp, _i32, _u64, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _vp, _vp, _sz, _vp]),
    "byolo_trainer_num_vars": (_i32, [_vp]),
    "byolo_trainer_var_info": (_i32, [_vp, _i32, _P(_cp), _P(_i32), _P(_i64)]),
    "byolo_trainer_get": (_i32, [_vp, _cp, _i32, _vp, _i64]),
    "byolo_trainer_set": (_i32, [_vp, _cp, _i32, _vp, _i64]),
    "byolo_trainer_get_step": (_i32, [_vp, _P(_i64)]),
    "byolo_trainer_set_step": (_i32, [_vp, _i64]),
    "byolo_trainer_export": (_i32, [_vp, _vp]),
    "byolo_trainer_taps": (_i32, [_vp, _P(_i32), _i32]),
    "byolo_trainer_layer_output": (_i32, [_vp, _i32, _vp, _i64, _P(_i64), _vp]),
    "byolo_eval_state_bytes": (_sz, [_i32]),
    "byolo_eval_create": (_i32, [_P(EvalCfg), _vp, _i64, _vp, _P(_vp)]),
    "byolo_eval_destroy": (_i32, [_vp]),
    "byolo_eval_last_error": (_cp, [_vp]),
    "byolo_eval_reset": (_i32, [_vp, _vp]),
    "byolo_eval_add": (_i32, [_vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i32, _vp]),
    "byolo_eval_finish": (_i32, [_vp, _P(EvalSummary), _P(_i64), _i32, _vp]),
    "byolo_eval_records": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "byolo_eval_loc_bytes": (_sz, [_i64]),
    "byolo_eval_set_loc": (_i32, [_vp, _P(EvalLocCfg), _vp]),
    "byolo_eval_loc_records": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "byolo_eval_ladder_bytes": (_sz, [_i64, _i32]),
    "byolo_eval_set_ladder": (_i32, [_vp, _P(EvalLadderCfg), _vp]),
    "byolo_eval_ladder_records": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "byolo_eval_subsets_bytes": (_sz, [_i64, _i32]),
    "byolo_eval_subsets_state_bytes": (_sz, [_i32, _i32]),
    "byolo_eval_set_subsets": (_i32, [_vp, _P(EvalSubsetsCfg), _vp, _vp]),
    "byolo_eval_subsets_records": (_i32, [_vp, _vp, _i64, _i64, _vp]),
    "byolo_eval_subsets_counts": (_i32, [_vp, _P(_i64), _i32, _vp]),
    "byolo_eval_pdq_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "byolo_eval_pdq_state_bytes": (_sz, []),
    "byolo_eval_set_pdq": (_i32, [_vp, _P(EvalPdqCfg), _P(EvalLocCfg), _vp, _i64, _vp, _i64, _vp, _vp, _sz]),
    "byolo_eval_set_pdq_workspace": (_i32, [_vp, _vp, _sz]),
    "byolo_eval_pdq_images": (_i32, [_vp, _vp, _i64, _i64, _P(_i64), _vp]),
    "byolo_eval_pdq_pairs": (_i32, [_vp, _vp, _i64, _i64, _P(_i64), _vp]),
    "byolo_eval_pdq_matrix": (_i32, [_vp, _i32, _P(_i32), _vp, _vp, _vp, _vp]),
    "byolo_pdq_assign": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "byolo_box_vote_workspace_bytes": (_sz, [_i32, _i64]),
    "byolo_box_vote": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _P(VoteCfg), _P(EvalLocCfg), _vp, _vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "byolo_set_box_vote": (_i32, [_vp, _P(VoteCfg)]),
    "byolo_box_vote_counts": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "byolo_soft_nms_workspace_bytes": (_sz, [_i32, _i64, _i32, _i32]),
    "byolo_soft_nms": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _P(SoftNmsCfg), _vp, _sz, _vp, _vp, _vp, _vp]),
    "byolo_set_soft_nms": (_i32, [_vp, _P(SoftNmsCfg)]),
    "byolo_var_recal_table": (_i32, [_P(VarRecalCfg), _vp]),
    "byolo_var_recal_apply": (_i32, [_P(VarRecalCfg), _vp, _i64, _i32, _vp, _vp, _vp]),
    "byolo_set_var_recal": (_i32, [_vp, _P(VarRecalCfg)]),
    "byolo_var_recal_fit_workspace_bytes": (_sz, [_i64]),
    "byolo_var_recal_fit": (_i32, [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _sz, _vp]),
    "byolo_score_recal_table": (_i32, [_P(ScoreRecalCfg), _vp]),
    "byolo_score_recal_apply": (_i32, [_P(ScoreRecalCfg), _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "byolo_set_score_recal": (_i32, [_vp, _P(ScoreRecalCfg)]),
    "byolo_score_recal_scores": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "byolo_score_recal_features": (_i32, [_P(ScoreRecalCfg), _vp, _i64, _i32, _i32, _i32, _i32, _P(ctypes.c_int32), _vp, _vp]),
    "byolo_score_recal_fit_workspace_bytes": (_sz, [_i64, _i32]),
    "byolo_score_recal_fit": (_i32, [_vp, _vp, _vp, _i32, _i64, _i32, ctypes.c_double, _i64, _vp, _vp, _sz, _vp]),
    "byolo_tta_view_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "byolo_tta_merge": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i64, _vp]),
    "byolo_tta_support_workspace_bytes": (_sz, [_i32, _i64]),
    "byolo_tta_support": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _P(TtaSupportCfg), _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


def _load():
    # PyTorch-ROCm bundles its own libamdhip64.so.7; device pointers and HIP streams are handed from
    # torch to libbyolo, so both MUST live in the same HIP runtime instance: import torch first, the
    # dynamic linker then resolves libbyolo's NEEDED libamdhip64.so.7 to the already-loaded one.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libbyolo.so not found at %s -- build it with `python bayesian-yolov3_amd/csrc/build.py` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    have = lib.byolo_abi_version()
    if have != ABI_VERSION:
        raise ImportError("%s speaks ABI %d, this binding was written for %d (include/byolo.h: BYOLO_ABI_VERSION) -- rebuild it with "
                          "`python bayesian-yolov3_amd/csrc/build.py --force`" % (LIB_PATH, have, ABI_VERSION))
    return lib


ABI_VERSION = 7
PNG_OK, PNG_UNSUPPORTED, PNG_SHAPE, PNG_CORRUPT, FEED_IO, FEED_CRC, FEED_PROTO = 0, 1, 2, 3, 4, 5, 6
lib = _load()


def check(handle, rc):
    if rc < 0:
        msg = lib.byolo_last_error(handle)
        raise ByoloError(rc, msg.decode("utf-8", "replace") if msg else "?")
    return rc
