"""ctypes binding of libreftr_hip.so (include/reftr_hip.h) + tensor-level op wrappers.

PyTorch is used here only as the owner of device memory and of the HIP stream the kernels are enqueued
on (torch.cuda.current_stream()).  There is NO fallback: if the library is missing or a kernel reports
an error, a RuntimeError is raised.
"""
import contextlib
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libreftr_hip_lab.so" if os.environ.get("REFTR_LAB", "0") == "1" else "libreftr_hip.so")   # _build.py
ABI_VERSION = 39          # (stays 39 with rt_hsv_jitter: additive entries -- rt_predict_*, rt_eval_raw_facts / rt_eval_orig -- never bumped it)

# The Python copy of the header's #defines and enumerators (tests/test_abi.py prints each from C and compares) ...
CONSTANTS = {
    "RT_ACT_NONE": 0, "RT_ACT_RELU": 1, "RT_ACT_GELU": 2, "RT_ACT_TANH": 3,
    "RT_ACCUM_FIRST": 0, "RT_ACCUM_ADD": 1, "RT_ACCUM_FINISH": 2, "RT_GRAD_ACCUM_SLOTS": 2048,
    # gradient-norm accumulator slots (rt_sqnorm_finish)
    "RT_SQ_SLOTS": 256, "RT_SQ_STRIDE": 32,
    "RT_MASK_LOSS_PARTIALS": 1024, "RT_STATS_MAX": 40,
    "RT_BATCH_STAGE_MAX_B": 64,          # what fits the kernel's argument block
    # rt_raw_stage: the largest in / out per axis its LDS budget admits, and its output tile
    "RT_RAW_STAGE_MAX_SCALE": 4, "RT_RAW_STAGE_TILE_H": 32, "RT_RAW_STAGE_TILE_W": 64,
    # rt_eval_metrics: accumulator slots (8 bytes each: int64 but for the two double sums) and the mask kernel's pixels per workgroup
    "RT_EVAL_DET_N": 0, "RT_EVAL_DET_HIT": 1, "RT_EVAL_SEG_N": 6, "RT_EVAL_SEG_HIT": 7, "RT_EVAL_SEG_I": 12, "RT_EVAL_SEG_U": 13,
    "RT_EVAL_DET_SUM": 14, "RT_EVAL_SEG_SUM": 15, "RT_EVAL_SLOTS": 16, "RT_EVAL_CHUNK": 16384,
    # rt_eval_orig: its own accumulator slots (int64 but for the double sum)
    "RT_EVAL_ORIG_N": 0, "RT_EVAL_ORIG_HIT": 1, "RT_EVAL_ORIG_I": 6, "RT_EVAL_ORIG_U": 7, "RT_EVAL_ORIG_SUM": 8, "RT_EVAL_ORIG_SLOTS": 9,
    "RT_PREDICT_FACTS_WORDS": 8,         # int32 words per image of rt_predict_facts' table
    "RT_DEC_MAX_LAYERS": 8, "RT_DEC_HANDOFF_BYTES": 256 + 16 * 256 * 36 + 16 * 2048 * 4,
}
# ... and its public names: every key without the "RT_" (hip.ACT_RELU, hip.SQ_SLOTS, hip.EVAL_SLOTS, hip.DEC_MAX_LAYERS, ...)
globals().update({name[3:]: value for name, value in CONSTANTS.items()})

STRUCTS = {}          # C typedef name -> its ctypes class (tests/test_abi.py checks every field's offset and size against the header)


class _Abi(Structure):
    """Base of every bound struct; `c` = its typedef in the header."""

    def __init_subclass__(cls, c):
        cls.C_NAME = c
        STRUCTS[c] = cls


class ConvGemmDesc(_Abi, c="rt_conv_gemm_desc"):
    _fields_ = [("src", c_void_p), ("wgt", c_void_p), ("out_bf16", c_void_p), ("out_f32", c_void_p),
                ("bias", c_void_p), ("res_f32", c_void_p), ("res_bf16", c_void_p), ("gate", c_void_p),
                ("preact", c_void_p),
                ("B", c_int32), ("SH", c_int32), ("SW", c_int32), ("SC", c_int32),
                ("DH", c_int32), ("DW", c_int32), ("N", c_int32),
                ("KH", c_int32), ("KW", c_int32), ("stride", c_int32), ("pad", c_int32),
                ("transposed", c_int32), ("act", c_int32),
                ("gate_scale", c_float), ("drop_p", c_float), ("drop_seed", c_uint32), ("tile_hint", c_int32),
                ("out_preact", c_void_p), ("dtanh", c_void_p), ("res_first", c_int32), ("seed_dev", c_void_p),
                ("drop_shift", c_int32), ("acc2_f32", c_void_p), ("dil", c_int32)]


class ConvWgradDesc(_Abi, c="rt_conv_wgrad_desc"):
    _fields_ = [("dy", c_void_p), ("x", c_void_p), ("dw", c_void_p), ("scale", c_void_p),
                ("B", c_int32), ("SH", c_int32), ("SW", c_int32), ("SC", c_int32),
                ("DH", c_int32), ("DW", c_int32), ("N", c_int32),
                ("KH", c_int32), ("KW", c_int32), ("stride", c_int32), ("pad", c_int32),
                ("msplit", c_int32), ("dbias", c_void_p), ("variant", c_int32),
                ("workspace", c_void_p), ("workspace_bytes", c_int64), ("overwrite", c_int32), ("dil", c_int32),
                ("sqacc", c_void_p), ("g16", c_void_p)]


class LayerNormDesc(_Abi, c="rt_layernorm_desc"):
    _fields_ = [("x", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("y_f32", c_void_p), ("y_bf16", c_void_p),
                ("pos", c_void_p), ("ypos_bf16", c_void_p), ("mean", c_void_p), ("rstd", c_void_p),
                ("M", c_int32), ("D", c_int32), ("eps", c_float), ("act", c_int32),
                ("drop_p", c_float), ("drop_seed", c_uint32),
                ("grp_rows", c_int32), ("grp_stride", c_int32), ("grp_off", c_int32), ("seed_dev", c_void_p)]


class LayerNormBwdDesc(_Abi, c="rt_layernorm_bwd_desc"):
    _fields_ = [("dy", c_void_p), ("dy2", c_void_p), ("x", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
                ("mean", c_void_p), ("rstd", c_void_p), ("dx_f32", c_void_p), ("dx_bf16", c_void_p),
                ("dgamma", c_void_p), ("dbeta", c_void_p),
                ("M", c_int32), ("D", c_int32), ("act", c_int32),
                ("drop_p", c_float), ("drop_seed", c_uint32), ("drop2_p", c_float), ("drop2_seed", c_uint32),
                ("grp_rows", c_int32), ("grp_stride", c_int32), ("grp_off", c_int32), ("seed_dev", c_void_p),
                ("partials", c_void_p), ("n_blocks_out", POINTER(c_int32))]


class LnPgJob(_Abi, c="rt_ln_pg_job"):
    _fields_ = [("partials", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p), ("n_blocks", c_int32), ("D", c_int32)]


class GroupNormDesc(_Abi, c="rt_groupnorm_desc"):
    _fields_ = [("x", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("stats", c_void_p),
                ("y_f32", c_void_p), ("y_bf16", c_void_p), ("pos", c_void_p), ("ypos_bf16", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("G", c_int32), ("eps", c_float),
                ("out_rows_per_img", c_int32), ("out_row_off", c_int32), ("partials", c_void_p), ("chunks", c_int32)]


class GroupNormBwdDesc(_Abi, c="rt_groupnorm_bwd_desc"):
    _fields_ = [("dy", c_void_p), ("dy2", c_void_p), ("x", c_void_p), ("gamma", c_void_p), ("stats", c_void_p),
                ("bstats", c_void_p), ("dx_f32", c_void_p), ("dx_bf16", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("G", c_int32), ("eps", c_float),
                ("out_rows_per_img", c_int32), ("out_row_off", c_int32)]


class AttnDesc(_Abi, c="rt_attn_desc"):
    _fields_ = [("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("out", c_void_p), ("lse", c_void_p), ("kpm", c_void_p),
                ("B", c_int32), ("H", c_int32), ("Sq", c_int32), ("Sk", c_int32), ("dh", c_int32),
                ("ldq", c_int32), ("ldk", c_int32), ("ldv", c_int32), ("ldo", c_int32),
                ("scale", c_float), ("drop_p", c_float), ("drop_seed", c_uint32), ("seed_dev", c_void_p)]


class AttnBwdDesc(_Abi, c="rt_attn_bwd_desc"):
    _fields_ = [("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("out", c_void_p), ("dout", c_void_p),
                ("lse", c_void_p), ("delta", c_void_p), ("kpm", c_void_p), ("dq", c_void_p), ("dk", c_void_p), ("dv", c_void_p),
                ("B", c_int32), ("H", c_int32), ("Sq", c_int32), ("Sk", c_int32), ("dh", c_int32),
                ("ldq", c_int32), ("ldk", c_int32), ("ldv", c_int32), ("ldo", c_int32),
                ("lddq", c_int32), ("lddk", c_int32), ("lddv", c_int32),
                ("scale", c_float), ("drop_p", c_float), ("drop_seed", c_uint32), ("seed_dev", c_void_p)]


class MaskPosencDesc(_Abi, c="rt_mask_posenc_desc"):
    _fields_ = [("mask", c_void_p), ("kpm_out", c_void_p), ("pos_out", c_void_p), ("add_vec", c_void_p),
                ("B", c_int32), ("H", c_int32), ("W", c_int32), ("h", c_int32), ("w", c_int32), ("C", c_int32),
                ("kpm_stride", c_int32), ("kpm_off", c_int32), ("pos_rows_per_img", c_int32), ("pos_row_off", c_int32)]


class BottleneckDesc(_Abi, c="rt_bottleneck_desc"):
    _fields_ = [("x", c_void_p), ("w1", c_void_p), ("w2", c_void_p), ("w3", c_void_p), ("wd", c_void_p),
                ("b1", c_void_p), ("b2", c_void_p), ("b3", c_void_p), ("bd", c_void_p), ("out", c_void_p),
                ("B", c_int32), ("H", c_int32), ("W", c_int32), ("cin", c_int32), ("planes", c_int32), ("form", c_int32)]


class RowsAddDesc(_Abi, c="rt_rows_add_desc"):
    _fields_ = [("a_f32", c_void_p), ("a_bf16", c_void_p), ("b_f32", c_void_p), ("out_f32", c_void_p), ("out_bf16", c_void_p),
                ("rows", c_int32), ("D", c_int32), ("alpha", c_float), ("accumulate", c_int32),
                ("a_grp_rows", c_int32), ("a_grp_stride", c_int32), ("a_grp_off", c_int32),
                ("b_grp_rows", c_int32), ("b_grp_stride", c_int32), ("b_grp_off", c_int32),
                ("o_grp_rows", c_int32), ("o_grp_stride", c_int32), ("o_grp_off", c_int32)]


class BoxLossDesc(_Abi, c="rt_box_loss_desc"):
    _fields_ = [("logits", c_void_p), ("valid", c_void_p), ("targets", c_void_p), ("tgt_off", c_void_p),
                ("num_boxes", c_void_p), ("losses", c_void_p), ("total", c_void_p), ("dlogits", c_void_p),
                ("NL", c_int32), ("B", c_int32), ("P", c_int32), ("K", c_int32), ("w_bbox", c_float), ("w_giou", c_float),
                ("weights", c_void_p)]


class MaskPostDesc(_Abi, c="rt_mask_post_desc"):
    _fields_ = [("pred", c_void_p), ("sizes", c_void_p), ("orig", c_void_p), ("origin_off", c_void_p),
                ("masks", c_void_p), ("masks_origin", c_void_p),
                ("B", c_int32), ("Q", c_int32), ("h", c_int32), ("w", c_int32), ("max_h", c_int32), ("max_w", c_int32),
                ("max_origin", c_int64), ("threshold", c_float)]


class BoxPostDesc(_Abi, c="rt_box_post_desc"):
    _fields_ = [("boxes", c_void_p), ("valid", c_void_p), ("sizes", c_void_p), ("out", c_void_p), ("counts", c_void_p),
                ("B", c_int32), ("P", c_int32), ("K", c_int32)]


class CemDesc(_Abi, c="rt_cem_desc"):
    _fields_ = [("hs", c_void_p), ("w3", c_void_p), ("b3", c_void_p), ("res", c_void_p), ("w2", c_void_p), ("b2", c_void_p),
                ("u", c_void_p), ("energy", c_void_p), ("stats", c_void_p), ("loss", c_void_p), ("g", c_void_p),
                ("dres", c_void_p), ("dhs", c_void_p), ("dw3", c_void_p), ("db3", c_void_p), ("dw2", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("ld", c_int32), ("lddr", c_int32), ("E", c_int32), ("reserved", c_int32)]


class AdamWDesc(_Abi, c="rt_adamw_desc"):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("n", c_int64),
                ("gnorm_sq", c_void_p), ("gnorm_out", c_void_p),
                ("grad_scale", c_float), ("max_norm", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float),
                ("step", c_int32), ("n_ranges", c_int32),
                ("range_begin", c_int64 * 8), ("range_end", c_int64 * 8), ("range_lr", c_float * 8), ("range_wd", c_float * 8),
                ("step_dev", c_void_p), ("active", c_void_p), ("lr_dev", c_void_p), ("span_begin", c_int64), ("span_end", c_int64),
                ("g16", c_void_p)]


class FinishDesc(_Abi, c="rt_finish_desc"):
    _fields_ = [("step", c_void_p), ("active", c_void_p), ("cond", c_void_p), ("loss", c_void_p),
                ("sq", c_void_p), ("norm_scale", c_float), ("grad_norm", c_void_p),
                ("src", c_void_p * STATS_MAX), ("n_src", c_int), ("cond_in_stats", c_int), ("stats", c_void_p)]


class SmallWgradJob(_Abi, c="rt_small_wgrad_job"):
    _fields_ = [("dy", c_void_p), ("x", c_void_p), ("dw", c_void_p), ("dbias", c_void_p),
                ("M", c_int32), ("N", c_int32), ("K", c_int32), ("overwrite", c_int32), ("sqacc", c_void_p), ("g16", c_void_p)]


class GnNhwcDesc(_Abi, c="rt_gn_nhwc_desc"):
    _fields_ = [("x", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("stats", c_void_p), ("y_bf16", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("G", c_int32), ("ldx", c_int32), ("ldy", c_int32),
                ("act", c_int32), ("eps", c_float), ("partials", c_void_p), ("partial_blocks", c_int32)]


class GnNhwcBwdDesc(_Abi, c="rt_gn_nhwc_bwd_desc"):
    _fields_ = [("dy", c_void_p), ("x", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("stats", c_void_p),
                ("bstats", c_void_p), ("dx_bf16", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("C", c_int32), ("G", c_int32), ("ldx", c_int32), ("lddy", c_int32),
                ("lddx", c_int32), ("act", c_int32), ("eps", c_float)]


class UpsampleAddDesc(_Abi, c="rt_upsample_add_desc"):
    _fields_ = [("fpn", c_void_p), ("a_bf16", c_void_p), ("out_bf16", c_void_p),
                ("B", c_int32), ("H", c_int32), ("W", c_int32), ("h", c_int32), ("w", c_int32), ("C", c_int32),
                ("ldf", c_int32), ("lda", c_int32), ("ldo", c_int32)]


class UpsampleAddBwdDesc(_Abi, c="rt_upsample_add_bwd_desc"):
    _fields_ = [("dy", c_void_p), ("da", c_void_p), ("dy_bf16", c_void_p),
                ("B", c_int32), ("H", c_int32), ("W", c_int32), ("h", c_int32), ("w", c_int32), ("C", c_int32),
                ("lddy", c_int32), ("ldda", c_int32), ("lddyb", c_int32)]


class AttnMapDesc(_Abi, c="rt_attn_map_desc"):
    _fields_ = [("q", c_void_p), ("k", c_void_p), ("mask", c_void_p), ("P", c_void_p), ("concat_bf16", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("E", c_int32), ("nh", c_int32), ("ldk", c_int32),
                ("k_rows_per_img", c_int32), ("k_row_off", c_int32), ("ld_concat", c_int32), ("concat_col", c_int32),
                ("norm", c_float)]


class AttnMapBwdDesc(_Abi, c="rt_attn_map_bwd_desc"):
    _fields_ = [("q", c_void_p), ("k", c_void_p), ("P", c_void_p), ("dconcat", c_void_p), ("dq", c_void_p), ("dk", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("E", c_int32), ("nh", c_int32), ("ldk", c_int32),
                ("k_rows_per_img", c_int32), ("k_row_off", c_int32), ("ld_dconcat", c_int32), ("concat_col", c_int32),
                ("norm", c_float)]


class SegConcatDesc(_Abi, c="rt_seg_concat_desc"):
    _fields_ = [("src", c_void_p), ("mem", c_void_p), ("out_bf16", c_void_p),
                ("B", c_int32), ("HW", c_int32), ("E", c_int32), ("nh", c_int32), ("ldo", c_int32),
                ("mem_rows_per_img", c_int32), ("mem_row_off", c_int32), ("src_rows_per_img", c_int32), ("src_row_off", c_int32)]


class MaskLossDesc(_Abi, c="rt_mask_loss_desc"):
    _fields_ = [("pred", c_void_p), ("target", c_void_p), ("sums", c_void_p), ("losses", c_void_p),
                ("dpred", c_void_p), ("g_focal", c_void_p), ("g_dice", c_void_p),
                ("B", c_int32), ("h", c_int32), ("w", c_int32), ("Ht", c_int32), ("Wt", c_int32), ("ldp", c_int32),
                ("lddp", c_int32), ("inv_norm", c_float), ("gbuf", c_void_p)]


class EvalMetricsArgs(_Abi, c="rt_eval_metrics_args"):
    _fields_ = [("pred_boxes", c_void_p), ("valid", c_void_p), ("table", c_void_p), ("masks", c_void_p), ("sizes", c_void_p),
                ("partials", c_void_p), ("iou_det", c_void_p), ("iou_seg", c_void_p), ("iu", c_void_p), ("acc", c_void_p),
                ("B", c_int32), ("P", c_int32), ("K", c_int32), ("Q", c_int32), ("max_h", c_int32), ("max_w", c_int32),
                ("reset", c_int32)]


class EvalCanvasArgs(_Abi, c="rt_eval_canvas_args"):
    _fields_ = [("pred_boxes", c_void_p), ("valid", c_void_p), ("tgt_boxes", c_void_p), ("tgt_off", c_void_p), ("facts", c_void_p),
                ("image_ids", c_void_p), ("pred_masks", c_void_p), ("tgt_masks", c_void_p), ("partials", c_void_p),
                ("iou_det", c_void_p), ("iou_seg", c_void_p), ("iu", c_void_p), ("acc", c_void_p), ("ring_boxes", c_void_p),
                ("ring_counts", c_void_p), ("ring_ids", c_void_p), ("cursor", c_void_p), ("veto", c_void_p),
                ("B", c_int32), ("P", c_int32), ("K", c_int32), ("Q", c_int32), ("h", c_int32), ("w", c_int32), ("Hc", c_int32),
                ("Wc", c_int32), ("tgt_rows", c_int32), ("slots", c_int32), ("threshold", c_float)]


class EvalRawFactsArgs(_Abi, c="rt_eval_raw_facts_args"):
    _N = CONSTANTS["RT_BATCH_STAGE_MAX_B"]
    _fields_ = [("facts", c_void_p), ("image_ids", c_void_p), ("mask_table", c_void_p), ("max_pixels", c_int64),
                ("B", c_int32), ("Hc", c_int32), ("Wc", c_int32), ("has_ids", c_int32),
                ("img_h", c_int32 * _N), ("img_w", c_int32 * _N), ("orig_h", c_int32 * _N), ("orig_w", c_int32 * _N),
                ("image_id", c_int64 * _N), ("tm_ptr", c_void_p * _N)]


class EvalOrigArgs(_Abi, c="rt_eval_orig_args"):
    _fields_ = [("pred_masks", c_void_p), ("facts", c_void_p), ("mask_table", c_void_p), ("partials", c_void_p), ("iou_seg", c_void_p),
                ("iu", c_void_p), ("acc", c_void_p), ("veto", c_void_p), ("max_pixels", c_int64),
                ("B", c_int32), ("Q", c_int32), ("h", c_int32), ("w", c_int32), ("Hc", c_int32), ("Wc", c_int32), ("threshold", c_float)]


class PredictFactsArgs(_Abi, c="rt_predict_facts_args"):
    _N = CONSTANTS["RT_BATCH_STAGE_MAX_B"]
    _fields_ = [("facts", c_void_p), ("capacity", c_int64), ("B", c_int32), ("Q", c_int32), ("Hc", c_int32), ("Wc", c_int32),
                ("img_h", c_int32 * _N), ("img_w", c_int32 * _N), ("orig_h", c_int32 * _N), ("orig_w", c_int32 * _N)]


class PredictCanvasArgs(_Abi, c="rt_predict_canvas_args"):
    _fields_ = [("pred_boxes", c_void_p), ("valid", c_void_p), ("facts", c_void_p), ("pred_masks", c_void_p), ("out_boxes", c_void_p),
                ("out_counts", c_void_p), ("out_masks", c_void_p), ("capacity", c_int64),
                ("B", c_int32), ("P", c_int32), ("K", c_int32), ("Q", c_int32), ("h", c_int32), ("w", c_int32), ("Hc", c_int32),
                ("Wc", c_int32), ("threshold", c_float)]


class RawStageArgs(_Abi, c="rt_raw_stage_args"):
    _N = CONSTANTS["RT_BATCH_STAGE_MAX_B"]
    _fields_ = [("img", c_void_p), ("mask", c_void_p), ("tgt_masks", c_void_p), ("boxes", c_void_p), ("tgt_off", c_void_p),
                ("num_boxes", c_void_p), ("B", c_int32), ("Hc", c_int32), ("Wc", c_int32), ("boxes_per_image", c_int32),
                ("mean", c_float * 3), ("std", c_float * 3),
                ("src", c_void_p * _N), ("box_ptr", c_void_p * _N), ("tm_ptr", c_void_p * _N),
                ("h", c_int32 * _N), ("w", c_int32 * _N), ("oh", c_int32 * _N), ("ow", c_int32 * _N), ("box_n", c_int32 * _N),
                ("rw", c_float * _N), ("rh", c_float * _N)]


class HsvJitterArgs(_Abi, c="rt_hsv_jitter_args"):
    _N = CONSTANTS["RT_BATCH_STAGE_MAX_B"]
    _fields_ = [("B", c_int32), ("src", c_void_p * _N), ("dst", c_void_p * _N), ("h", c_int32 * _N), ("w", c_int32 * _N),
                ("s_gain", c_float * _N), ("v_gain", c_float * _N)]


class DecoderLayerFwd(_Abi, c="rt_decoder_layer_fwd"):
    _PTRS = ("Wv", "Wo", "Wq", "Wo2", "W1", "W2", "bv", "bo", "bq", "bo2", "b1", "b2", "g1", "be1", "g2", "be2", "g3", "be3",
             "k2", "v2", "o", "t1q16", "q2", "o2", "t2_16", "hdn", "t3_16", "u", "u2", "u3",
             "mean1", "rstd1", "mean2", "rstd2", "mean3", "rstd3", "lse2", "t3_f32")
    _SEEDS = ("seed_ad", "seed_d1", "seed_ad2", "seed_d2", "seed_dh", "seed_d3")
    _fields_ = [(n, c_void_p) for n in _PTRS] + [(n, c_uint32) for n in _SEEDS]


class DecoderLayerBwd(_Abi, c="rt_decoder_layer_bwd"):
    _PTRS = ("WT2", "WT1", "WTo2", "WTq", "WTo", "WTv", "g1", "g2", "g3", "u", "u2", "u3",
             "mean1", "rstd1", "mean2", "rstd2", "mean3", "rstd3", "hdn", "q2", "k2", "v2", "o2", "lse2", "dnorm",
             "du3b", "dhdn", "du2b", "dq2", "dub", "dv", "dk2", "dv2", "dk2p", "dv2p", "part1", "part2", "part3")
    _SEEDS = ("seed_ad", "seed_d1", "seed_ad2", "seed_d2", "seed_d3", "reserved")
    _fields_ = [(n, c_void_p) for n in _PTRS] + [(n, c_uint32) for n in _SEEDS]


class DecoderBwdDesc(_Abi, c="rt_decoder_bwd_desc"):
    _fields_ = [("layer", DecoderLayerBwd * DEC_MAX_LAYERS),
                ("dta", c_void_p), ("dqpos", c_void_p), ("kpm", c_void_p), ("handoff", c_void_p), ("seed_dev", c_void_p),
                ("n_layers", c_int32), ("M", c_int32), ("H", c_int32), ("S", c_int32), ("F", c_int32), ("ldkv", c_int32),
                ("drop_p", c_float), ("scale", c_float), ("gate_scale", c_float), ("ldkvp", c_int32)]


class DecoderFwdDesc(_Abi, c="rt_decoder_fwd_desc"):
    _fields_ = [("layer", DecoderLayerFwd * DEC_MAX_LAYERS),
                ("t32", c_void_p), ("t16", c_void_p), ("qpos", c_void_p), ("kpm", c_void_p), ("handoff", c_void_p),
                ("seed_dev", c_void_p),
                ("n_layers", c_int32), ("M", c_int32), ("H", c_int32), ("S", c_int32), ("F", c_int32), ("ldkv", c_int32),
                ("drop_p", c_float), ("eps", c_float), ("scale", c_float)]


class QencFwdDesc(_Abi, c="rt_qenc_fwd_desc"):
    _PTRS = ("mem16", "mem32", "ctx", "W1", "W2", "W3", "Wc", "Wf0", "Wf4", "b1", "b2", "b3", "bc", "bf0", "bf4",
             "gc", "betc", "g1", "bet1", "g5", "bet5", "qembed", "seed_dev",
             "cls16", "lang16", "kq", "qs", "vs", "qw", "c16", "co", "cmean", "crstd", "cat16",
             "t1", "m1", "r1", "a16", "t2", "m2", "r2", "tgt32", "tgt16", "qpos", "tgtq16")
    _fields_ = [(n, c_void_p) for n in _PTRS] + [("B", c_int32), ("S", c_int32), ("L", c_int32), ("P", c_int32), ("nq", c_int32),
                                                 ("E", c_int32), ("eps", c_float), ("drop_p", c_float), ("drop_seed", c_uint32),
                                                 ("reserved", c_int32)]


class HeadLossDesc(_Abi, c="rt_head_loss_desc"):
    _PTRS = ("t3", "gn", "betn", "W0", "W1", "W2", "W0T", "W1T", "b0", "b1", "b2", "w2_f32",
             "valid", "targets", "tgt_off", "num_boxes", "weights",
             "hs16", "y1", "y2", "hmean", "hrstd", "logits", "losses", "dlogits", "dl16", "dy2", "dy1", "dhs", "dnorm", "db2_part", "part_n", "total", "ticket")
    _fields_ = [(n, c_void_p) for n in _PTRS] + [("NL", c_int32), ("B", c_int32), ("P", c_int32), ("K", c_int32), ("E", c_int32),
                                                 ("eps", c_float), ("invert_valid", c_int32), ("reserved", c_int32)]


class QencBwdDesc(_Abi, c="rt_qenc_bwd_desc"):
    _PTRS = ("ga", "gb", "dqpos", "t2", "m2", "r2", "g5", "bet5", "t1", "m1", "r1", "g1", "bet1", "co", "cmean", "crstd", "gc", "betc",
             "kq", "qs", "vs", "qw", "Wf4T", "Wf0T", "WcT", "W1T", "W2T", "W3T", "seed_dev",
             "dt2b", "dt1b", "dcob", "dk16", "dqs16", "dvs16", "da", "dcat", "dc", "dmem", "dqembed", "part5", "part1", "partc")
    _fields_ = [(n, c_void_p) for n in _PTRS] + [("B", c_int32), ("S", c_int32), ("L", c_int32), ("P", c_int32), ("E", c_int32),
                                                 ("drop_p", c_float), ("drop_seed", c_uint32), ("reserved", c_int32)]


# name -> (restype, argtypes); every symbol include/reftr_hip.h declares must be listed here (tests/test_abi.py checks the names, the
# number of parameters and the kind of each one against the header).
_SIGNATURES = {
    "rt_abi_version": (c_int, []),
    "rt_device_arch": (c_int, [c_int, c_char_p, c_int]),
    "rt_conv_gemm": (c_int, [POINTER(ConvGemmDesc), c_void_p]),
    "rt_conv_gemm_grouped": (c_int, [c_void_p, c_int, c_void_p]),
    "rt_conv_wgrad": (c_int, [POINTER(ConvWgradDesc), c_void_p]),
    "rt_gconv": (c_int, [POINTER(ConvGemmDesc), c_int, c_void_p]),
    "rt_gconv_wgrad": (c_int, [POINTER(ConvWgradDesc), c_int, c_void_p]),
    "rt_layernorm_fwd": (c_int, [POINTER(LayerNormDesc), c_void_p]),
    "rt_layernorm_bwd": (c_int, [POINTER(LayerNormBwdDesc), c_void_p]),
    "rt_groupnorm_fwd": (c_int, [POINTER(GroupNormDesc), c_void_p]),
    "rt_groupnorm_bwd": (c_int, [POINTER(GroupNormBwdDesc), c_void_p]),
    "rt_attn_fwd": (c_int, [POINTER(AttnDesc), c_void_p]),
    "rt_attn_bwd": (c_int, [POINTER(AttnBwdDesc), c_void_p]),
    "rt_img_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_stem_conv": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_maxpool3x3s2": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_stem_pool": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_bottleneck_fwd": (c_int, [POINTER(BottleneckDesc), c_void_p]),
    "rt_weight_prep": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "rt_weight_prep_batched": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "rt_stem_weight_prep": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_bn_fold": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p]),
    "rt_mask_posenc": (c_int, [POINTER(MaskPosencDesc), c_void_p]),
    "rt_colsum": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "rt_rows_add": (c_int, [POINTER(RowsAddDesc), c_void_p]),
    "rt_bert_embed_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rt_bert_embed_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "rt_roberta_pos_ids": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "rt_context_mask": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_qenc_attn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_qenc_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_box_loss": (c_int, [POINTER(BoxLossDesc), c_void_p]),
    "rt_cem_fwd": (c_int, [POINTER(CemDesc), c_void_p]),
    "rt_cem_bwd": (c_int, [POINTER(CemDesc), c_void_p]),
    "rt_mask_postprocess": (c_int, [POINTER(MaskPostDesc), c_void_p]),
    "rt_box_postprocess": (c_int, [POINTER(BoxPostDesc), c_void_p]),
    "rt_eval_metrics": (c_int, [POINTER(EvalMetricsArgs), c_void_p]),
    "rt_eval_facts": (c_int, [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int32), c_int, c_void_p,
                              c_void_p, c_void_p]),
    "rt_eval_canvas": (c_int, [POINTER(EvalCanvasArgs), c_void_p]),
    "rt_eval_raw_facts": (c_int, [POINTER(EvalRawFactsArgs), c_void_p]),
    "rt_eval_orig": (c_int, [POINTER(EvalOrigArgs), c_void_p]),
    "rt_predict_facts": (c_int, [POINTER(PredictFactsArgs), c_void_p]),
    "rt_predict_canvas": (c_int, [POINTER(PredictCanvasArgs), c_void_p]),
    "rt_small_dgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "rt_pos_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_sqnorm": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "rt_sqnorm_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "rt_sqnorm_finish": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_round_chunks": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "rt_adamw_flat": (c_int, [POINTER(AdamWDesc), c_void_p]),
    "rt_sgd_flat": (c_int, [POINTER(AdamWDesc), c_void_p]),
    "rt_grad_accum": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_zero_chunks": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "rt_counter_add": (c_int, [c_void_p, c_int32, c_void_p]),
    "rt_ln_param_grad_grouped": (c_int, [POINTER(LnPgJob), c_int, c_void_p]),
    "rt_conv_wgrad_grouped": (c_int, [POINTER(ConvWgradDesc), c_int, c_void_p, c_int64, c_void_p]),
    "rt_small_wgrad_grouped": (c_int, [POINTER(SmallWgradJob), c_int, c_void_p]),
    "rt_resample_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "rt_img_collate_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), c_void_p]),
    "rt_batch_stage": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, POINTER(c_void_p),
                               POINTER(c_int32), c_int, c_void_p, c_void_p, c_void_p, POINTER(c_void_p), POINTER(c_int32),
                               c_void_p, c_void_p]),
    "rt_raw_stage": (c_int, [POINTER(RawStageArgs), c_void_p]),
    "rt_resample_taps": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "rt_hsv_jitter": (c_int, [POINTER(HsvJitterArgs), c_void_p]),
    "rt_gn_nhwc_fwd": (c_int, [POINTER(GnNhwcDesc), c_void_p]),
    "rt_gn_nhwc_bwd": (c_int, [POINTER(GnNhwcBwdDesc), c_void_p]),
    "rt_upsample_add": (c_int, [POINTER(UpsampleAddDesc), c_void_p]),
    "rt_upsample_add_bwd": (c_int, [POINTER(UpsampleAddBwdDesc), c_void_p]),
    "rt_attn_map_fwd": (c_int, [POINTER(AttnMapDesc), c_void_p]),
    "rt_attn_map_bwd": (c_int, [POINTER(AttnMapBwdDesc), c_void_p]),
    "rt_seg_concat": (c_int, [POINTER(SegConcatDesc), c_void_p]),
    "rt_mask_loss": (c_int, [POINTER(MaskLossDesc), c_void_p]),
    "rt_comm_unique_id": (c_int, [c_void_p]),
    "rt_comm_init": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "rt_comm_allreduce": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64), c_int, c_int, c_void_p]),
    "rt_comm_destroy": (c_int, [c_void_p]),
    "rt_decoder_fwd": (c_int, [POINTER(DecoderFwdDesc), c_void_p]),
    "rt_decoder_bwd": (c_int, [POINTER(DecoderBwdDesc), c_void_p]),
    "rt_decoder_trace": (c_int, [c_void_p]),
    "rt_decoder_supported": (c_int, [c_int]),
    "rt_decoder_set_spin": (c_int, [c_int]),
    "rt_counter_add_if_zero": (c_int, [c_void_p, c_int32, c_void_p, c_int, c_void_p]),
    "rt_stamp": (c_int, [c_void_p, c_int, c_void_p]),
    "rt_finish_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_finish_stats": (c_int, [c_void_p, c_void_p]),
    "rt_adamw_mat": (c_int, [POINTER(AdamWDesc), c_void_p, c_int, c_int, c_void_p]),
    "rt_adamw_chunks": (c_int, [POINTER(AdamWDesc), c_void_p, c_int, c_void_p]),
    "rt_qenc_fwd": (c_int, [POINTER(QencFwdDesc), c_void_p]),
    "rt_head_loss": (c_int, [POINTER(HeadLossDesc), c_void_p]),
    "rt_qenc_bwd": (c_int, [POINTER(QencBwdDesc), c_void_p]),
    "rt_qregion_trace": (c_int, [c_void_p]),
}

_lib = None
LAB_LIB_PATH = os.path.join(_HERE, "libreftr_hip_lab.so")
# rt_conv_gemm tile hints the PRODUCT library instantiates (what its heuristics can choose; csrc/rt_gemm.hip); every other measured
# variant lives in the lab library only
PRODUCT_TILE_HINTS = frozenset({0, 21, 31, 33, 51, 233, 252, 262, 281, 285})


def _load(path):
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP kernel library is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc; no CPU fallback exists).")
    L = ctypes.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    v = L.rt_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"{os.path.basename(path)} ABI {v} != binding ABI {ABI_VERSION}; rebuild")
    return L


def lib():
    """Load libreftr_hip.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


_lab_lib = None


@contextlib.contextmanager
def lab_library():
    """Route this module's calls to the LAB build (libreftr_hip_lab.so, the same sources with -DRT_LAB) inside the block: tests and
    sweeps of the rt_conv_gemm variants the product library does not instantiate.  Never used by the product path."""
    global _lib, _lab_lib
    if _lab_lib is None:
        _lab_lib = _load(LAB_LIB_PATH)
    prev = lib()
    _lib = _lab_lib
    try:
        yield
    finally:
        _lib = prev


def exported_symbols():
    return sorted(_SIGNATURES)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# what a field or an argument takes as it is: most of them, and every launch looks at each of its own
_PLAIN = frozenset({int, float, bool, type(None), POINTER(c_int32)})


def _val(v):
    """What a field or an argument holds: a tensor gives its address, a Python sequence its converted elements."""
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return tuple(_val(e) for e in v) if isinstance(v, (list, tuple)) else v


def _fill(d, fields, Tensor=torch.Tensor, plain=_PLAIN):
    for k, v in fields.items():          # (per field and per launch: locals, and no call for a plain value)
        if v.__class__ is Tensor:
            fields[k] = v.data_ptr()
        elif v.__class__ not in plain:
            fields[k] = _val(v)
    d.__init__(**fields)          # one ctypes call sets them all; a name the struct does not have it keeps as a plain attribute
    if d.__dict__:
        raise TypeError(f"{type(d).__name__} ({d.C_NAME}): no field {sorted(d.__dict__)}")
    return d


def _set(d, **fields):
    """Fills fields of the bound struct `d` BY NAME: a tensor gives its address, None gives NULL, a sequence given to an array field
    fills its leading elements; fields not named keep what they hold.  A name the struct does not have is an error."""
    return _fill(d, fields)


def _desc(cls, **fields):
    """A new `cls` filled by `_set`: fields not named are zero / NULL."""
    return _fill(cls(), fields)


def _call(name, *args, stream=True, Tensor=torch.Tensor, plain=_PLAIN, byref=ctypes.byref):
    """The library's entry point `name`: bound structs go by reference, tensors by address, and the current stream goes last (entry
    points without one: stream=False).  A non-zero return code is an error."""
    args = [a if a.__class__ in plain else a.data_ptr() if a.__class__ is Tensor
            else byref(a) if isinstance(a, Structure) else _val(a) for a in args]
    if stream:
        args.append(_stream())
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc} ({'RT_ERR' if rc < 0 else 'hipError'})")


_TIMER = None
_SEED_DEV = None


def set_seed_dev(t):
    """Device uint32/int32 word mixed into every dropout seed (lets a captured hipGraph draw fresh masks per replay)."""
    global _SEED_DEV
    _SEED_DEV = t


def _seedp(drop_p):
    return _p(_SEED_DEV) if (drop_p > 0 and _SEED_DEV is not None) else None


def set_launch_timer(records):
    """bench.py instrumentation: when `records` is a list, every rt_conv_gemm / rt_conv_wgrad launch is
    bracketed by HIP events on the launch stream and appended as {kind, flops, start, end}."""
    global _TIMER
    _TIMER = records


def _algo_bytes(tag):
    """Compulsory HBM bytes of one GEMM-family launch: each operand read once (bf16), the result written once
    (bf16 activations / fp32 weight gradients)."""
    kind, B, SH, SW, SC, DH, DW, N, KH, KW = tag[:10]
    M = B * DH * DW
    if kind == "W":
        return 2.0 * (M * N + B * SH * SW * SC) + 4.0 * N * KH * KW * SC
    return 2.0 * (B * SH * SW * SC + N * KH * KW * SC + M * N)


def _timed(kind, flops, fn, tag=None, nbytes=None, epi_bytes=0.0):
    if _TIMER is None:
        return fn()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    _TIMER.append({"kind": kind, "flops": float(flops), "start": e0, "end": e1, "tag": tag,
                   "bytes": nbytes if nbytes is not None else (_algo_bytes(tag) if tag is not None else 0.0),
                   "epi_bytes": float(epi_bytes)})
    return r


def as_u8(t):
    """A mask as the uint8 bytes the kernels read: bool tensors are re-typed in place (same bytes, no launch -- `.to(torch.uint8)` is a
    converting copy: 12 us for the [8, 640, 640] padding mask at the head of every step), everything else is converted."""
    t = t.contiguous()
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t if t.dtype == torch.uint8 else t.to(torch.uint8)


def _req(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name}: HIP kernels need a device tensor (got {t.device}); no CPU path exists")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous")


_GEOM = ("B", "SH", "SW", "SC", "DH", "DW", "N", "KH", "KW", "stride", "pad")


def _gemm_desc(src, wgt, geom, **fields):
    """A product's descriptor: the geometry tuple and every other field by name (`_set`)."""
    fields.update(src=src, wgt=wgt)
    return _fill(ConvGemmDesc(**dict(zip(_GEOM, geom, strict=True))), fields)


def _wgrad_desc(dy, x, dw, geom, **fields):
    """... of a weight gradient into `dw`, with the norm accumulator and the bf16 twin `dw` is registered for."""
    fields.update(dy=dy, x=x, dw=dw, sqacc=_sqacc(dw), g16=_g16(dw))
    return _fill(ConvWgradDesc(**dict(zip(_GEOM, geom, strict=True))), fields)


def _out_buffer(o, dtype, name, M, N, dev):
    """An [M, N] output of a product: an existing tensor to write into, True (allocate) or False / None (none)."""
    o = o if torch.is_tensor(o) else (torch.empty((M, N), dtype=dtype, device=dev) if o else None)
    _req(o, dtype, name)
    assert o is None or o.numel() == M * N
    return o


# --------------------------------------------------------------------------------------------
# op wrappers
# --------------------------------------------------------------------------------------------
def conv_gemm(src, wgt, *, geom, bias=None, res_f32=None, res_bf16=None, gate=None, gate_scale=1.0,
              preact=None, dtanh=None, res_first=False, act=ACT_NONE, drop_p=0.0, drop_seed=0, transposed=False,
              out_bf16=True, out_f32=False, out_preact=False, tile_hint=0, group=None, drop_shift=0, acc2_f32=None, dil=1):
    """out[B,DH,DW,N] = epilogue(implicit_gemm(src[B,SH,SW,SC], wgt[N,KH,KW,SC])).

    geom = (B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad).  Returns (out_bf16 | None, out_f32 | None)
    (+ the bf16 pre-activation as a third value when out_preact is given).  out_bf16 / out_f32 / out_preact may be True (allocate
    [M, N]) or an existing tensor to write into (in-place accumulation when it is also `res_f32`).
    """
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    _req(src, torch.bfloat16, "src"); _req(wgt, torch.bfloat16, "wgt")
    _req(bias, torch.float32, "bias"); _req(res_f32, torch.float32, "res_f32")
    _req(res_bf16, torch.bfloat16, "res_bf16"); _req(gate, torch.bfloat16, "gate")
    _req(preact, torch.bfloat16, "preact")
    assert src.numel() == B * SH * SW * SC, (src.shape, geom)
    assert wgt.numel() == N * KH * KW * SC, (wgt.shape, geom)
    M = B * DH * DW
    _req(dtanh, torch.bfloat16, "dtanh")
    ob = _out_buffer(out_bf16, torch.bfloat16, "out_bf16", M, N, src.device)
    of = _out_buffer(out_f32, torch.float32, "out_f32", M, N, src.device)
    _req(acc2_f32, torch.float32, "acc2_f32")
    assert acc2_f32 is None or acc2_f32.numel() == M * N
    d = _gemm_desc(src, wgt, geom, out_bf16=ob, out_f32=of, bias=bias, res_f32=res_f32, res_bf16=res_bf16, gate=gate, preact=preact,
                   transposed=int(bool(transposed)), act=act, gate_scale=gate_scale, drop_p=drop_p, drop_seed=drop_seed & 0xFFFFFFFF,
                   tile_hint=tile_hint, dtanh=dtanh, res_first=int(bool(res_first)), seed_dev=_seedp(drop_p), drop_shift=drop_shift,
                   acc2_f32=acc2_f32, dil=int(dil))
    op = _out_buffer(out_preact, torch.bfloat16, "out_preact", M, N, src.device)
    if op is not None:
        _set(d, out_preact=op)
    if transposed:     # algorithmic FLOPs of backward-data = those of the forward conv it differentiates
        flops = 2.0 * B * SH * SW * SC * N * KH * KW
    else:
        flops = 2.0 * M * N * KH * KW * SC
    # bytes of the elementwise operations fused into the epilogue (NOT part of the operand-only "algorithmic" figure): bf16
    # residual / gate / GELU-pre-activation / tanh reads, fp32 residual read, read-modify-write of the second destination, and
    # every output beyond the first bf16 one
    epi = M * N * (2.0 * sum(t is not None for t in (res_bf16, gate, preact, dtanh)) + 4.0 * (res_f32 is not None)
                   + 8.0 * (acc2_f32 is not None) + (4.0 if of is not None else 0.0) + (2.0 if ob is not None else 0.0) - 2.0
                   + (2.0 if op is not None else 0.0))
    if group is not None:      # queued: GemmGroup.run() launches every queued product at once
        group.add(d, flops, ("T" if transposed else "F",) + tuple(geom), (src, wgt, ob, of, op, bias, res_f32, res_bf16, gate, preact, dtanh), epi)
    else:
        _timed("conv_gemm", flops, lambda: _call("rt_conv_gemm", d), tag=("T" if transposed else "F",) + tuple(geom), epi_bytes=epi)
    if op is not None:
        return ob, of, op
    return ob, of


class GemmGroup:
    """Independent GEMMs queued with `conv_gemm(..., group=g)` / `linear(..., group=g)` (outputs are allocated at queue time)
    and launched together by `run()` (rt_conv_gemm_grouped: one launch when the products allow it)."""

    def __init__(self):
        self.descs, self.keep, self.flops, self.nbytes, self.epi = [], [], 0.0, 0.0, 0.0

    def add(self, d, flops, tag, keep, epi=0.0):
        self.descs.append(d); self.keep.append(keep); self.flops += flops; self.nbytes += _algo_bytes(tag); self.epi += epi

    def run(self):
        if not self.descs:
            return
        n = len(self.descs)
        for i in range(0, n, 12):
            chunk = self.descs[i:i + 12]
            arr = (ConvGemmDesc * len(chunk))(*chunk)
            share = len(chunk) / n
            _timed("conv_gemm", self.flops * share, lambda arr=arr, m=len(chunk): _call("rt_conv_gemm_grouped", arr, m),
                   nbytes=self.nbytes * share, epi_bytes=self.epi * share)
        self.descs, self.keep, self.flops, self.nbytes, self.epi = [], [], 0.0, 0.0, 0.0


def linear(x, w, bias=None, **kw):
    """y[M,N] = epilogue(x[M,K] @ w[N,K]^T): a 1x1 'conv' over M rows."""
    M, K = x.shape
    N = w.shape[0]
    return conv_gemm(x, w, geom=(M, 1, 1, K, 1, 1, N, 1, 1, 1, 0), bias=bias, **kw)


_WGRAD_WS = {}
WGRAD_WS_BYTES = 64 << 20


def _wgrad_workspace(dev):
    """Per-(device, stream) scratch for rt_conv_wgrad's split partials: launches on concurrent streams must not
    share it, launches on one stream reuse it in order."""
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    ws = _WGRAD_WS.get(key)
    if ws is None:
        ws = _WGRAD_WS[key] = torch.empty(WGRAD_WS_BYTES // 4, dtype=torch.float32, device=dev)
    return ws


# Gradient-norm accumulators: {data_ptr of a registered weight-gradient matrix: its model's slot buffer} (ParamStore registers its
# overwritable matrices here).  Every weight-gradient launch into such a matrix hands the slots to the library (`sqacc`), which adds
# |dw after|^2 - |dw before|^2 -- the clip norm then needs no pass over the gradient buffer (rt_sqnorm_finish).
_SQACC_MAP = {}


def _owned(table, dw):
    """Entry of a {data_ptr: (weakref to the owning ParamStore, value)} map, valid only while the owner is alive (its gradient
    buffer still occupies that address: nothing else can); entries of dead owners are dropped."""
    ent = table.get(dw.data_ptr())
    if ent is None:
        return None
    if ent[0]() is None:
        del table[dw.data_ptr()]
        return None
    return ent[1]


def _sqacc(dw):
    t = _owned(_SQACC_MAP, dw)
    return t.data_ptr() if t is not None else None


# bf16 exchange twins (data parallel): {data_ptr of a registered weight-gradient matrix: data_ptr of its bf16 twin} -- the launches
# that write the matrix write the rounded copy as well (rt_conv_wgrad_desc.g16); reftr_amd.parallel fills the map
_G16_MAP = {}


def _g16(dw):
    return _owned(_G16_MAP, dw)


def round_chunks(base, twin, table, n):
    """twin[i] = bf16(base[i]) over n chunks {offset, count} of a static device table (rt_round_chunks)."""
    _req(base, torch.float32, "base"); _req(twin, torch.bfloat16, "twin"); _req(table, torch.int64, "table")
    if n > 0:
        _call("rt_round_chunks", base, twin, table, int(n))


def sqnorm_finish(flat_g, table, nchunks, slots, out, extra=None):
    """out[0] = sum of the accumulator slots + |the chunks of flat_g listed in `table`|^2 (+ extra[0])."""
    _req(flat_g, torch.float32, "flat_g"); _req(slots, torch.float32, "slots"); _req(out, torch.float32, "out")
    assert slots.numel() == SQ_SLOTS * SQ_STRIDE
    _call("rt_sqnorm_finish", flat_g, table, int(nchunks), slots, extra, out)


def conv_wgrad(dy, x, dw, *, geom, scale=None, msplit=0, dbias=None, variant=0, workspace=True, overwrite=False, dil=1):
    """dw[N,KH,KW,SC] (fp32) += (overwrite: =) scale[n] * sum_m dy[m,n] * gather(x)[m,(kh,kw,c)]."""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(dw, torch.float32, "dw")
    _req(scale, torch.float32, "scale")
    assert dy.numel() == B * DH * DW * N and x.numel() == B * SH * SW * SC and dw.numel() == N * KH * KW * SC
    _req(dbias, torch.float32, "dbias")
    ws = _wgrad_workspace(dy.device) if workspace else None
    d = _wgrad_desc(dy, x, dw, geom, scale=scale, msplit=msplit, dbias=dbias, variant=variant, workspace=ws,
                    workspace_bytes=WGRAD_WS_BYTES if ws is not None else 0, overwrite=int(bool(overwrite)), dil=int(dil))
    _timed("conv_wgrad", 2.0 * B * DH * DW * N * KH * KW * SC, lambda: _call("rt_conv_wgrad", d), tag=("W",) + tuple(geom))
    return dw


def gconv(src, wgt, *, geom, groups, bias=None, gate=None, gate_scale=1.0, act=ACT_NONE, transposed=False,
          out_bf16=True, out_f32=False, dil=1, **unsupported):
    """Grouped 3x3 convolution (rt_gconv): out[B,DH,DW,N] = epilogue(grouped_conv(src[B,SH,SW,SC], wgt[SC,3,3,SC/groups])).

    geom as in conv_gemm (transposed=True: backward-data, geom of the transposed problem, `wgt` still the FORWARD layout).
    Fields the grouped kernel does not implement (res_*, preact, dropout, tile_hint, ...) are passed on and refused by the
    library.  Returns (out_bf16 | None, out_f32 | None)."""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    _req(src, torch.bfloat16, "src"); _req(wgt, torch.bfloat16, "wgt"); _req(bias, torch.float32, "bias"); _req(gate, torch.bfloat16, "gate")
    assert src.numel() == B * SH * SW * SC, (src.shape, geom)
    cg = SC // groups if groups > 0 else 0
    assert wgt.numel() == SC * KH * KW * cg, (wgt.shape, geom, groups)
    M = B * DH * DW
    ob = _out_buffer(out_bf16, torch.bfloat16, "out_bf16", M, N, src.device)
    of = _out_buffer(out_f32, torch.float32, "out_f32", M, N, src.device)
    d = _gemm_desc(src, wgt, geom, out_bf16=ob, out_f32=of, bias=bias, gate=gate, transposed=int(bool(transposed)), act=act,
                   gate_scale=gate_scale, dil=int(dil), **unsupported)      # (forwarded so that the library refuses them: no silent drop)
    spatial = B * (SH * SW if transposed else DH * DW)
    flops = 2.0 * spatial * SC * KH * KW * cg
    _timed("gconv", flops, lambda: _call("rt_gconv", d, int(groups)), nbytes=2.0 * (B * SH * SW * SC + M * N) + 2.0 * wgt.numel())
    return ob, of


def gconv_wgrad(dy, x, dw, *, geom, groups, scale=None, msplit=0, overwrite=False, dil=1, dbias=None, variant=0):
    """Grouped 3x3 weight gradient (rt_gconv_wgrad): dw[N,3,3,Cg] (fp32) += (overwrite: =) scale[n] * sum_m dy[m,n] *
    gather(x)[m, (kh, kw, g(n) * Cg + c)].  The split partials use this stream's weight-gradient workspace."""
    B, SH, SW, SC, DH, DW, N, KH, KW, stride, pad = geom
    _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(dw, torch.float32, "dw"); _req(scale, torch.float32, "scale")
    _req(dbias, torch.float32, "dbias")
    cg = SC // groups if groups > 0 else 0
    assert dy.numel() == B * DH * DW * N and x.numel() == B * SH * SW * SC and dw.numel() == N * KH * KW * cg
    ws = _wgrad_workspace(dy.device)
    d = _wgrad_desc(dy, x, dw, geom, scale=scale, msplit=msplit, dbias=dbias, variant=variant, workspace=ws,
                    workspace_bytes=WGRAD_WS_BYTES, overwrite=int(bool(overwrite)), dil=int(dil))
    _timed("gconv_wgrad", 2.0 * B * DH * DW * N * KH * KW * cg, lambda: _call("rt_gconv_wgrad", d, int(groups)),
           nbytes=2.0 * (B * DH * DW * N + B * SH * SW * SC) + 4.0 * dw.numel())
    return dw


def linear_wgrad(dy, x, dw, **kw):
    M, N = dy.shape
    K = x.shape[1]
    return conv_wgrad(dy, x, dw, geom=(M, 1, 1, K, 1, 1, N, 1, 1, 1, 0), **kw)


# --------------------------------------------------------------------------------------------
# norms
# --------------------------------------------------------------------------------------------
def _new(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


def layernorm_fwd(x, gamma, beta, eps=1e-5, *, act=ACT_NONE, drop_p=0.0, drop_seed=0, pos=None,
                  y_f32=None, y_bf16=None, ypos_bf16=None, want_f32=True, want_bf16=True,
                  rowmap=(0, 0, 0), save_stats=True):
    """y = [drop][relu](LN(x)); returns (y_f32, y_bf16, ypos_bf16, mean, rstd).  Output buffers may be passed
    in (row-mapped writes into a larger sequence buffer) or are allocated [M, D]."""
    M, D = x.shape
    _req(x, torch.float32, "x"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta")
    _req(pos, torch.float32, "pos")
    if y_f32 is None and want_f32:
        y_f32 = _new((M, D), torch.float32, x)
    if y_bf16 is None and want_bf16:
        y_bf16 = _new((M, D), torch.bfloat16, x)
    if pos is not None and ypos_bf16 is None:
        ypos_bf16 = _new((M, D), torch.bfloat16, x)
    mean = _new((M,), torch.float32, x) if save_stats else None
    rstd = _new((M,), torch.float32, x) if save_stats else None
    grp_rows, grp_stride, grp_off = rowmap
    _call("rt_layernorm_fwd", _desc(
        LayerNormDesc, x=x, gamma=gamma, beta=beta, y_f32=y_f32, y_bf16=y_bf16, pos=pos, ypos_bf16=ypos_bf16, mean=mean, rstd=rstd,
        M=M, D=D, eps=eps, act=act, drop_p=drop_p, drop_seed=drop_seed & 0xFFFFFFFF, grp_rows=grp_rows, grp_stride=grp_stride,
        grp_off=grp_off, seed_dev=_seedp(drop_p)))
    return y_f32, y_bf16, ypos_bf16, mean, rstd


class LnGradBatch:
    """LayerNorm parameter gradients of many rt_layernorm_bwd launches, reduced together (rt_ln_param_grad_grouped)."""

    def __init__(self):
        self.jobs, self.keep = [], []

    def run(self):
        if not self.jobs:
            return
        arr = (LnPgJob * len(self.jobs))(*self.jobs)
        _call("rt_ln_param_grad_grouped", arr, len(self.jobs))
        self.jobs, self.keep = [], []


def layernorm_bwd(dy, x, gamma, beta, mean, rstd, dgamma, dbeta, *, dy2=None, act=ACT_NONE, drop_p=0.0,
                  drop_seed=0, drop2_p=0.0, drop2_seed=0, rowmap=(0, 0, 0), want_f32=True, want_bf16=True, pg_batch=None):
    """Returns (dx_f32 [M,D], dx_bf16 [M,D] = bf16(dx * dropout2-mask)); dgamma/dbeta accumulated in place, or -- with
    `pg_batch` (LnGradBatch) -- queued as per-workgroup partial sums that pg_batch.run() reduces later."""
    M, D = x.shape
    _req(dy, torch.float32, "dy"); _req(dy2, torch.float32, "dy2"); _req(x, torch.float32, "x")
    dx_f32 = _new((M, D), torch.float32, x) if want_f32 else None
    dx_bf16 = _new((M, D), torch.bfloat16, x) if want_bf16 else None
    part, nb = None, c_int32(0)
    if pg_batch is not None and (dgamma is not None or dbeta is not None):
        part = _new((min((M + 3) // 4, 1024), 2, D), torch.float32, x)
    grp_rows, grp_stride, grp_off = rowmap
    _call("rt_layernorm_bwd", _desc(
        LayerNormBwdDesc, dy=dy, dy2=dy2, x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd, dx_f32=dx_f32, dx_bf16=dx_bf16,
        dgamma=dgamma, dbeta=dbeta, M=M, D=D, act=act, drop_p=drop_p, drop_seed=drop_seed & 0xFFFFFFFF, drop2_p=drop2_p,
        drop2_seed=drop2_seed & 0xFFFFFFFF, grp_rows=grp_rows, grp_stride=grp_stride, grp_off=grp_off,
        seed_dev=_seedp(max(drop_p, drop2_p)), partials=part, n_blocks_out=ctypes.pointer(nb)))
    if part is not None:
        pg_batch.jobs.append(_desc(LnPgJob, partials=part, dgamma=dgamma, dbeta=dbeta, n_blocks=nb.value, D=D))
        pg_batch.keep.append(part)
    return dx_f32, dx_bf16


def groupnorm_fwd(x, gamma, beta, G, eps, *, y_f32=None, y_bf16=None, pos=None, ypos_bf16=None,
                  rows_per_img=None, row_off=0):
    """x fp32 [B, HW, C]; outputs are sequence buffers [B*rows_per_img, C] written at row_off + pixel."""
    B, HW, C = x.shape
    _req(x, torch.float32, "x")
    rows_per_img = HW if rows_per_img is None else rows_per_img
    stats = _new((B, G, 2), torch.float32, x)
    chunks = min(64, (HW + 7) // 8)
    partials = _new((B, chunks, G, 2), torch.float32, x)
    _call("rt_groupnorm_fwd", _desc(
        GroupNormDesc, x=x, gamma=gamma, beta=beta, stats=stats, y_f32=y_f32, y_bf16=y_bf16, pos=pos, ypos_bf16=ypos_bf16,
        B=B, HW=HW, C=C, G=G, eps=eps, out_rows_per_img=rows_per_img, out_row_off=row_off, partials=partials, chunks=chunks))
    return stats


def groupnorm_bwd(dy, x, gamma, stats, dgamma, dbeta, G, eps, *, dy2=None, rows_per_img=None, row_off=0,
                  want_f32=False, want_bf16=True):
    B, HW, C = x.shape
    rows_per_img = HW if rows_per_img is None else rows_per_img
    bstats = _new((B, G, 2), torch.float32, x)
    dx_f32 = _new((B, HW, C), torch.float32, x) if want_f32 else None
    dx_bf16 = _new((B, HW, C), torch.bfloat16, x) if want_bf16 else None
    _call("rt_groupnorm_bwd", _desc(
        GroupNormBwdDesc, dy=dy, dy2=dy2, x=x, gamma=gamma, stats=stats, bstats=bstats, dx_f32=dx_f32, dx_bf16=dx_bf16,
        dgamma=dgamma, dbeta=dbeta, B=B, HW=HW, C=C, G=G, eps=eps, out_rows_per_img=rows_per_img, out_row_off=row_off))
    return dx_f32, dx_bf16


# --------------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------------
def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, "attention operands are 2-D row views with unit inner stride"
    return t.stride(0)


def attn_fwd(q, k, v, kpm, *, B, H, Sq, Sk, dh, scale, drop_p=0.0, drop_seed=0, out=None):
    """q [B*Sq, >=H*dh], k/v [B*Sk, >=H*dh] bf16 row views (head h at columns h*dh..); kpm uint8 [B, Sk] or None.
    Returns (out bf16 [B*Sq, H*dh], lse fp32 [B, H, Sq])."""
    if out is None:
        out = _new((B * Sq, H * dh), torch.bfloat16, q)
    lse = _new((B, H, Sq), torch.float32, q)
    _call("rt_attn_fwd", _desc(
        AttnDesc, q=q, k=k, v=v, out=out, lse=lse, kpm=kpm, B=B, H=H, Sq=Sq, Sk=Sk, dh=dh, ldq=_ld(q), ldk=_ld(k), ldv=_ld(v),
        ldo=_ld(out), scale=scale, drop_p=drop_p, drop_seed=drop_seed & 0xFFFFFFFF, seed_dev=_seedp(drop_p)))
    return out, lse


def attn_bwd(q, k, v, out, dout, lse, kpm, *, B, H, Sq, Sk, dh, scale, drop_p=0.0, drop_seed=0,
             dq=None, dk=None, dv=None):
    """Returns (dq, dk, dv) bf16; output row views may be supplied (e.g. halves of one packed buffer)."""
    if dq is None:
        dq = _new((B * Sq, H * dh), torch.bfloat16, q)
    if dk is None:
        dk = _new((B * Sk, H * dh), torch.bfloat16, q)
    if dv is None:
        dv = _new((B * Sk, H * dh), torch.bfloat16, q)
    delta = _new((B, H, Sq), torch.float32, q)
    d = _desc(AttnBwdDesc, q=q, k=k, v=v, out=out, dout=dout, lse=lse, delta=delta, kpm=kpm, dq=dq, dk=dk, dv=dv,
              B=B, H=H, Sq=Sq, Sk=Sk, dh=dh, ldq=_ld(q), ldk=_ld(k), ldv=_ld(v), ldo=_ld(out), lddq=_ld(dq), lddk=_ld(dk), lddv=_ld(dv),
              scale=scale, drop_p=drop_p, drop_seed=drop_seed & 0xFFFFFFFF, seed_dev=_seedp(drop_p))
    assert _ld(dout) == _ld(out)
    _call("rt_attn_bwd", d)
    return dq, dk, dv


def decoder_handoff(dev):
    """A hand-off buffer for rt_decoder_fwd / rt_decoder_bwd (zeroed once; word 0 = launch epoch, word 1 = failure flag).  Its owner
    (one model) keeps it for all its launches: they are ordered on the model's stream."""
    return torch.zeros(DEC_HANDOFF_BYTES // 4, dtype=torch.int32, device=dev)


def decoder_fwd(layers, t32, t16, qpos, kpm, *, H, S, F, drop_p, scale, handoff, eps=1e-5):
    """The decoder stack of one-query-per-image inputs as one cooperative launch (rt_decoder_fwd).  `layers`: one dict per
    layer, keys = DecoderLayerFwd._PTRS (tensors) + DecoderLayerFwd._SEEDS (ints); every output tensor is allocated by the
    caller (they are the launched chain's saved tensors).  Returns the hand-off buffer's header [epoch, failure flag]."""
    M = t32.shape[0]
    assert 1 <= len(layers) <= DEC_MAX_LAYERS
    d = _desc(DecoderFwdDesc, t32=t32, t16=t16, qpos=qpos, kpm=kpm, handoff=handoff, seed_dev=_seedp(drop_p), n_layers=len(layers),
              M=M, H=H, S=S, F=F, ldkv=_ld(layers[0]["k2"]), drop_p=drop_p, eps=eps, scale=scale)
    for i, lay in enumerate(layers):
        _set(d.layer[i], **{n: lay[n] for n in DecoderLayerFwd._PTRS}, **{n: lay[n] & 0xFFFFFFFF for n in DecoderLayerFwd._SEEDS})
    _call("rt_decoder_fwd", d)
    return handoff[:2]


def decoder_bwd(layers, dta, dqpos, kpm, *, H, S, F, drop_p, scale, gate_scale, handoff, ldkvp=0):
    """Backward of the cooperative decoder stack (rt_decoder_bwd).  `layers`: one dict per layer (first to last), keys =
    DecoderLayerBwd._PTRS (tensors, all allocated by the caller) + the dropout seeds of the forward."""
    M = dta.shape[0]
    assert 1 <= len(layers) <= DEC_MAX_LAYERS
    d = _desc(DecoderBwdDesc, dta=dta, dqpos=dqpos, kpm=kpm, handoff=handoff, seed_dev=_seedp(drop_p), n_layers=len(layers),
              M=M, H=H, S=S, F=F, ldkv=_ld(layers[0]["k2"]), drop_p=drop_p, scale=scale, gate_scale=gate_scale, ldkvp=ldkvp)
    for i, lay in enumerate(layers):
        _set(d.layer[i], **{n: lay.get(n) for n in DecoderLayerBwd._PTRS},
             **{n: lay[n] & 0xFFFFFFFF for n in DecoderLayerBwd._SEEDS[:-1]})
    _call("rt_decoder_bwd", d)
    return handoff[:2]


def decoder_trace(readback=True):
    """REFTR_DEC_TRACE=1: (workgroup 0 stamps, last workgroup stamps) of the last rt_decoder_fwd launch, 100 MHz ticks."""
    buf = (c_uint32 * 1024)()
    _call("rt_decoder_trace", ctypes.cast(buf, c_void_p) if readback else None, stream=False)
    if not readback:
        return None
    a = list(buf)
    return a[:512], a[512:]


# --------------------------------------------------------------------------------------------
# backbone-side
# --------------------------------------------------------------------------------------------
def stem_geometry(H, W):
    """conv1 7x7/2 pad 3 output size and the padded NHWC4 input size rt_stem_conv needs."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp = max(H + 6, 2 * Ho + 5)
    Wp = max(W + 6, 32 * ((Wo + 15) // 16) + 6)
    return Ho, Wo, Hp, Wp


def img_pack(img):
    B, C, H, W = img.shape
    assert C == 3
    _req(img, torch.float32, "img")
    _, _, Hp, Wp = stem_geometry(H, W)
    out = _new((B, Hp, Wp, 4), torch.bfloat16, img)
    _call("rt_img_pack", img, out, B, H, W, Hp, Wp)
    return out


def stem_conv(xp, w, bias, Ho, Wo):
    B, Hp, Wp, _ = xp.shape
    out = _new((B, Ho, Wo, 64), torch.bfloat16, xp)
    _call("rt_stem_conv", xp, w, bias, out, B, Hp, Wp, Ho, Wo)
    return out


def maxpool3x3s2(x):
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = _new((B, Ho, Wo, C), torch.bfloat16, x)
    _call("rt_maxpool3x3s2", x, y, B, H, W, C, Ho, Wo)
    return y


def stem_pool(xp, w, bias, Ho, Wo):
    """conv1 7x7/2 + FrozenBN + ReLU + MaxPool2d(3, 2, 1) in one launch: the stem output is never written."""
    B, Hp, Wp, _ = xp.shape
    out = _new((B, (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1, 64), torch.bfloat16, xp)
    _call("rt_stem_pool", xp, w, bias, out, B, Hp, Wp, Ho, Wo)
    return out


def bottleneck_fwd(x, w1, b1, w2, b2, w3, b3, wd=None, bd=None, out=None, form=0):
    """One frozen stride-1 layer1 bottleneck (planes 64) in one launch: x bf16 [B,H,W,cin] -> bf16 [B,H,W,256]."""
    _req(x, torch.bfloat16, "x")
    B, Hh, Ww, cin = x.shape
    if out is None:
        out = _new((B, Hh, Ww, 256), torch.bfloat16, x)
    d = _desc(BottleneckDesc, x=x, w1=w1, w2=w2, w3=w3, wd=wd, b1=b1, b2=b2, b3=b3, bd=bd, out=out, B=B, H=Hh, W=Ww, cin=cin,
              planes=w1.shape[0], form=form)
    # a member of the GEMM family of bench.py's roofline: the algorithmic FLOPs of the convolutions it replaces (the conv1 halo
    # recomputation is not counted), compulsory bytes = block input + output + weights once
    M = B * Hh * Ww
    macs = cin * 64 + 576 * 64 + 64 * 256 + (cin * 256 if wd is not None else 0)
    nbytes = 2.0 * (M * (cin + 256) + macs)
    _timed("bottleneck_fwd", 2.0 * M * macs, lambda: _call("rt_bottleneck_fwd", d), tag=("BNK", B, Hh, Ww, cin, Hh, Ww, 256, 3, 3, 1, 1),
           nbytes=nbytes)
    return out


def weight_prep(src, N, T, C, *, scale=None, dst=None, dst_t=None):
    """fp32 [N][T][C] master -> bf16 dst [N][T][C] and/or dst_t [C][T][N] (both * scale[n])."""
    _req(src, torch.float32, "src")
    _call("rt_weight_prep", src, scale, dst, dst_t, N, T, C)


def stem_weight_prep(src, scale, dst):
    _call("rt_stem_weight_prep", src, scale, dst)


def bn_fold(w, b, rm, rv, eps, scale, shift):
    _call("rt_bn_fold", w, b, rm, rv, eps, scale, shift, w.numel())


def mask_posenc(mask_u8, h, w, C, add_vec, kpm_out, kpm_off, pos_out, rows_per_img, row_off):
    """mask uint8 [B,H,W]; writes kpm_out[b, kpm_off + pix] and pos_out[b*rows_per_img + row_off + pix, :]."""
    B, H, W = mask_u8.shape
    _call("rt_mask_posenc", _desc(
        MaskPosencDesc, mask=mask_u8, kpm_out=kpm_out, pos_out=pos_out, add_vec=add_vec, B=B, H=H, W=W, h=h, w=w, C=C,
        kpm_stride=kpm_out.shape[1], kpm_off=kpm_off, pos_rows_per_img=rows_per_img, pos_row_off=row_off))


# --------------------------------------------------------------------------------------------
# small fused ops
# --------------------------------------------------------------------------------------------
def colsum(dy, db):
    """db[n] += sum_m dy[m, n] (dy bf16 or fp32, 2-D contiguous)."""
    M, N = dy.shape
    _call("rt_colsum", dy, 1 if dy.dtype == torch.bfloat16 else 0, db, M, N)


def rows_add(rows, D, *, a_f32=None, a_bf16=None, b_f32=None, out_f32=None, out_bf16=None, alpha=1.0,
             accumulate=False, a_map=(0, 0, 0), b_map=(0, 0, 0), o_map=(0, 0, 0)):
    (a_rows, a_stride, a_off), (b_rows, b_stride, b_off), (o_rows, o_stride, o_off) = a_map, b_map, o_map
    _call("rt_rows_add", _desc(
        RowsAddDesc, a_f32=a_f32, a_bf16=a_bf16, b_f32=b_f32, out_f32=out_f32, out_bf16=out_bf16, rows=rows, D=D, alpha=alpha,
        accumulate=int(accumulate), a_grp_rows=a_rows, a_grp_stride=a_stride, a_grp_off=a_off, b_grp_rows=b_rows, b_grp_stride=b_stride,
        b_grp_off=b_off, o_grp_rows=o_rows, o_grp_stride=o_stride, o_grp_off=o_off))


def roberta_pos_ids(ids, pad_idx):
    B, L = ids.shape
    out = torch.empty((B, L), dtype=torch.int32, device=ids.device)
    _call("rt_roberta_pos_ids", ids, out, B, L, pad_idx)
    return out


def bert_embed_fwd(ids, word, pos, type_emb, L, pos_ids=None):
    rows = ids.numel()
    D = word.shape[1]
    out = _new((rows, D), torch.float32, word)
    _call("rt_bert_embed_fwd", ids, word, pos, type_emb, out, rows, L, D, pos_ids)
    return out


def bert_embed_bwd(ids, de, dword, dpos, dtype_emb, L, pos_ids=None):
    rows, D = de.shape
    _call("rt_bert_embed_bwd", ids, de, dword, dpos, dtype_emb, rows, L, D, pos_ids)


def context_mask(smask_u8, phrase_mask_u8=None, pos_l=None, pos_r=None):
    """Returns (ctx uint8 [B,P,L] 1 = ignore, qmask uint8 [B,P] 1 = ignore) — models/reftr_transformer.py:224-248."""
    B, L = smask_u8.shape
    if phrase_mask_u8 is None:
        P, Lp = 1, 0
    else:
        _, P, Lp = phrase_mask_u8.shape
    ctx = _new((B, P, L), torch.uint8, smask_u8)
    qmask = _new((B, P), torch.uint8, smask_u8)
    _call("rt_context_mask", smask_u8, phrase_mask_u8, pos_l, pos_r, ctx, qmask, B, L, P, Lp)
    return ctx, qmask


def qenc_attn_fwd(k, qs, vs, ctx):
    """k [B,E], qs/vs [B,L,E] fp32, ctx uint8 [B,P,L] -> (w [B,P,L], c [B,P,E])."""
    B, L, E = qs.shape
    P = ctx.shape[1]
    w = _new((B, P, L), torch.float32, qs)
    c = _new((B, P, E), torch.float32, qs)
    _call("rt_qenc_attn_fwd", k, qs, vs, ctx, w, c, B, P, L, E)
    return w, c


def qenc_attn_bwd(k, qs, vs, w, dc):
    B, L, E = qs.shape
    P = w.shape[1]
    zz = torch.zeros(B * E + 2 * B * L * E, dtype=torch.float32, device=qs.device)       # one clear for the three outputs
    dk, dqs, dvs = zz[:B * E].view(B, E), zz[B * E:B * E + B * L * E].view(B, L, E), zz[B * E + B * L * E:].view(B, L, E)
    _call("rt_qenc_attn_bwd", k, qs, vs, w, dc, dk, dqs, dvs, B, P, L, E)
    return dk, dqs, dvs


def qenc_fwd(*, B, S, L, P, nq, E, eps=1e-5, drop_p=0.0, drop_seed=0, **t):
    """QueryEncoder forward + query / query_pos split as ONE launch (rt_qenc_fwd).  `t`: the named tensors of rt_qenc_fwd_desc."""
    _call("rt_qenc_fwd", _desc(QencFwdDesc, **dict(t, seed_dev=_SEED_DEV if drop_p > 0 else None), B=B, S=S, L=L, P=P, nq=nq, E=E,
                               eps=eps, drop_p=drop_p, drop_seed=drop_seed & 0xFFFFFFFF))


def head_loss(*, NL, B, P, K, E, eps=1e-5, invert_valid=False, **t):
    """decoder.norm + bbox MLP + box losses + d total / d logits + their backward-data as ONE launch (rt_head_loss)."""
    _call("rt_head_loss", _desc(HeadLossDesc, **t, NL=NL, B=B, P=P, K=K, E=E, eps=eps, invert_valid=int(bool(invert_valid))))


def qenc_bwd(*, B, S, L, P, E, drop_p=0.0, drop_seed=0, **t):
    """Backward-data of rt_qenc_fwd as ONE launch (rt_qenc_bwd)."""
    _call("rt_qenc_bwd", _desc(QencBwdDesc, **dict(t, seed_dev=_SEED_DEV if drop_p > 0 else None), B=B, S=S, L=L, P=P, E=E,
                               drop_p=drop_p, drop_seed=drop_seed & 0xFFFFFFFF))


def qregion_trace():
    """Stage stamps [3][24] (10 ns units) of workgroup 0 of the last rt_qenc_fwd / rt_head_loss / rt_qenc_bwd launches."""
    buf = (ctypes.c_uint64 * 72)()
    _call("rt_qregion_trace", ctypes.cast(buf, c_void_p), stream=False)
    return [list(buf[i * 24:(i + 1) * 24]) for i in range(3)]


def box_loss(logits, valid_u8, targets, tgt_off, num_boxes, w_bbox=1.0, w_giou=1.0, want_grad=True, weights=None):
    """logits fp32 [NL,B,P,K,4]; returns (losses [NL,2], total [1], dlogits | None).  `weights` (device fp32
    [NL,2]) overrides the scalar weights per layer."""
    NL, B, P, K, _ = logits.shape
    buf = _new((NL * 2 + 1,), torch.float32, logits)        # [NL][2] losses | total: one clear inside rt_box_loss
    losses, total = buf[:NL * 2].view(NL, 2), buf[NL * 2:]
    dl = _new(tuple(logits.shape), torch.float32, logits) if want_grad else None
    _call("rt_box_loss", _desc(BoxLossDesc, logits=logits, valid=valid_u8, targets=targets, tgt_off=tgt_off, num_boxes=num_boxes,
                               losses=losses, total=total, dlogits=dl, NL=NL, B=B, P=P, K=K, w_bbox=w_bbox, w_giou=w_giou, weights=weights))
    return losses, total, dl


def cem_fwd(hs16, w3, b3, res16, w2, b2, B, HW):
    """CEM block forward (rt_cem_fwd): returns (loss [1], saved = (u [B,16], energy [B], stats [B,2]))."""
    _req(hs16, torch.bfloat16, "hs"); _req(res16, torch.bfloat16, "res")
    for t, n in ((w3, "w3"), (b3, "b3"), (w2, "w2"), (b2, "b2")):
        _req(t, torch.float32, n)
    E = hs16.shape[-1]
    u = _new((B, 16), torch.float32, w3); energy = _new((B,), torch.float32, w3); stats = _new((B, 2), torch.float32, w3)
    loss = _new((1,), torch.float32, w3)
    _call("rt_cem_fwd", _desc(CemDesc, hs=hs16, w3=w3, b3=b3, res=res16, w2=w2, b2=b2, u=u, energy=energy, stats=stats, loss=loss,
                              B=B, HW=HW, ld=res16.shape[-1], E=E))
    return loss, (u, energy, stats)


def cem_bwd(hs16, w3, b3, res16, w2, b2, saved, g, dres, dw3, db3, dw2, B, HW):
    """CEM block backward: dres (fp32 [B*HW, ld]) += d res; dw3 / db3 / dw2 accumulate; returns d hs fp32 [B, E]."""
    _req(g, torch.float32, "g"); _req(dres, torch.float32, "dres")
    for t, n in ((dw3, "dw3"), (db3, "db3"), (dw2, "dw2")):
        _req(t, torch.float32, n)
    u, energy, stats = saved
    E = hs16.shape[-1]
    dhs = _new((B, E), torch.float32, w3)
    _call("rt_cem_bwd", _desc(CemDesc, hs=hs16, w3=w3, b3=b3, res=res16, w2=w2, b2=b2, u=u, energy=energy, stats=stats, g=g, dres=dres,
                              dhs=dhs, dw3=dw3, db3=db3, dw2=dw2, B=B, HW=HW, ld=res16.shape[-1], lddr=dres.shape[-1], E=E))
    return dhs


def mask_postprocess(pred, sizes_i32, max_hw, threshold=0.5, orig_i32=None, origin_off=None, origin_total=0, max_origin=0):
    """pred fp32 [B, Q, h, w] mask logits; sizes_i32 / orig_i32 device int32 [B, 2]; origin_off device int64 [B + 1].
    Returns (masks uint8 [B, Q, max_h, max_w], masks_origin uint8 [origin_total] | None)."""
    B, Q, h, w = pred.shape
    _req(pred, torch.float32, "pred"); _req(sizes_i32, torch.int32, "sizes")
    _req(orig_i32, torch.int32, "orig"); _req(origin_off, torch.int64, "origin_off")
    max_h, max_w = int(max_hw[0]), int(max_hw[1])
    masks = _new((B, Q, max_h, max_w), torch.uint8, pred)
    mo = _new((int(origin_total),), torch.uint8, pred) if orig_i32 is not None else None
    _call("rt_mask_postprocess", _desc(
        MaskPostDesc, pred=pred, sizes=sizes_i32, orig=orig_i32, origin_off=origin_off, masks=masks, masks_origin=mo, B=B, Q=Q, h=h, w=w,
        max_h=max_h, max_w=max_w, max_origin=int(max_origin), threshold=float(threshold)))
    return masks, mo


def box_postprocess(boxes, valid_u8, sizes_f32=None):
    """boxes fp32 [B, P, K, 4] cxcywh, valid uint8 [B, P, K]; sizes fp32 [B, 2] = (img_h, img_w) or None.
    Returns (xyxy fp32 [B, P, 4] with every image's valid phrases compacted to the front, counts int32 [B])."""
    B, P, K, _ = boxes.shape
    _req(boxes, torch.float32, "boxes"); _req(valid_u8, torch.uint8, "valid"); _req(sizes_f32, torch.float32, "sizes")
    out = torch.zeros(B, P, 4, dtype=torch.float32, device=boxes.device)
    counts = _new((B,), torch.int32, boxes)
    _call("rt_box_postprocess", _desc(BoxPostDesc, boxes=boxes, valid=valid_u8, sizes=sizes_f32, out=out, counts=counts, B=B, P=P, K=K))
    return out, counts


def eval_metrics(pred_boxes, valid_u8, table, acc, masks=None, sizes_i32=None, reset=False):
    """rt_eval_metrics for one batch: pred_boxes fp32 [B, P, K, 4] cxcywh, valid uint8 [B, P, K], table device int64 [B, 5] =
    {target boxes pointer, n_b, target mask pointer | 0, mask height, mask width}, acc device int64 [EVAL_SLOTS] (slots
    EVAL_DET_SUM / EVAL_SEG_SUM hold doubles), updated in place -- from zero when `reset`.  masks uint8 [B, Q, max_h, max_w] (what
    mask_postprocess returned) + sizes_i32 device int32 [B, 2] add the mask part (query 0 of every image).
    Returns (iou_det fp32 [B, P], iou_seg fp32 [B] | None, iu int64 [B, 2] | None) of this batch."""
    B, P, K, _ = pred_boxes.shape
    _req(pred_boxes, torch.float32, "pred_boxes"); _req(valid_u8, torch.uint8, "valid"); _req(table, torch.int64, "table")
    _req(acc, torch.int64, "acc"); _req(masks, torch.uint8, "masks"); _req(sizes_i32, torch.int32, "sizes")
    assert tuple(valid_u8.shape) == (B, P, K) and tuple(table.shape) == (B, 5) and acc.numel() == EVAL_SLOTS
    iou_det = _new((B, P), torch.float32, pred_boxes)
    Q = max_h = max_w = 0
    partials = iou_seg = iu = None
    if masks is not None:
        assert sizes_i32 is not None and masks.dim() == 4 and masks.shape[0] == B and tuple(sizes_i32.shape) == (B, 2)
        Q, max_h, max_w = (int(v) for v in masks.shape[1:])
        partials = _new((B, max(1, -(-(max_h * max_w) // EVAL_CHUNK)), 2), torch.int32, pred_boxes)
        iou_seg = _new((B,), torch.float32, pred_boxes)
        iu = _new((B, 2), torch.int64, pred_boxes)
    _call("rt_eval_metrics", _desc(
        EvalMetricsArgs, pred_boxes=pred_boxes, valid=valid_u8, table=table, masks=masks, sizes=sizes_i32, partials=partials,
        iou_det=iou_det, iou_seg=iou_seg, iu=iu, acc=acc, B=B, P=P, K=K, Q=Q, max_h=max_h, max_w=max_w, reset=1 if reset else 0))
    return iou_det, iou_seg, iu


def eval_facts(sizes, facts, image_ids, origs=None, ids=None, mask_hw=None):
    """rt_eval_facts: the per-image facts of one evaluation batch gathered on the device in one launch.  sizes / origs: B device
    int64 tensors of two elements ({h, w}; origs None: the sizes), ids: B device int64 tensors of one element (None: -1), mask_hw: B
    (h, w) pairs of python ints (None: 0, 0) -> facts int32 [B, 6], image_ids int64 [B].  The pointers go by value in the kernel
    arguments: nothing is copied to the device and nothing synchronises."""
    B = len(sizes)
    _req(facts, torch.int32, "facts"); _req(image_ids, torch.int64, "image_ids")
    assert facts.numel() == 6 * B and image_ids.numel() == B and facts.is_contiguous()

    def ptrs(ts, n):
        if ts is None:
            return None
        assert len(ts) == B
        for t in ts:
            assert t.is_cuda and t.dtype == torch.int64 and t.numel() == n and t.is_contiguous(), (t.dtype, tuple(t.shape))
        return (c_void_p * B)(*[t.data_ptr() for t in ts])
    hw = None
    if mask_hw is not None:
        assert len(mask_hw) == B
        hw = (c_int32 * (2 * B))(*[int(v) for p in mask_hw for v in p])
    _call("rt_eval_facts", ptrs(sizes, 2), ptrs(origs, 2), ptrs(ids, 1), hw, B, facts, image_ids)


class EvalCanvasState:
    """What rt_eval_canvas keeps in device memory over an evaluation: `acc` (int64 [EVAL_SLOTS], shared with rt_eval_metrics), the
    results ring of `slots` batches of B images with P phrase rows (boxes fp32 [slots, B, P, 4], counts int32 [slots, B], ids int64
    [slots, B]) and `cursor` int32 [2] = {next slot, overflow}.  The caller zeroes acc and cursor once, before the first batch."""

    def __init__(self, slots, B, P, device, acc=None):
        self.slots, self.B, self.P = int(slots), int(B), int(P)
        self.acc = torch.zeros(EVAL_SLOTS, dtype=torch.int64, device=device) if acc is None else acc
        self.boxes = torch.zeros((self.slots, B, P, 4), dtype=torch.float32, device=device)
        self.counts = torch.zeros((self.slots, B), dtype=torch.int32, device=device)
        self.ids = torch.zeros((self.slots, B), dtype=torch.int64, device=device)
        self.cursor = torch.zeros(2, dtype=torch.int32, device=device)


def eval_canvas(pred_boxes, valid_u8, tgt_boxes, tgt_off, facts, image_ids, state, pred_masks=None, tgt_masks=None, threshold=0.5,
                out=None, veto=None):
    """rt_eval_canvas for one canvas batch: pred_boxes fp32 [B, P, K, 4], valid uint8 [B, P, K], tgt_boxes / tgt_off what batch_stage
    wrote, facts / image_ids what eval_facts wrote, state an EvalCanvasState (accumulators, ring and cursor, updated in place).
    pred_masks fp32 [B, Q, h, w] + tgt_masks uint8 [B, 1, Hc, Wc] add the mask part (query 0 of every image, frame = canvas).
    veto: device int32 word; non-zero at run time -> the batch leaves accumulators, ring and cursor untouched.
    `out` = (iou_det, iou_seg, iu, partials) to write into (a captured graph's static outputs); fresh tensors when None.
    Returns (iou_det fp32 [B, P], iou_seg fp32 [B] | None, iu int64 [B, 2] | None) of this batch."""
    B, P, K, _ = pred_boxes.shape
    _req(pred_boxes, torch.float32, "pred_boxes"); _req(valid_u8, torch.uint8, "valid"); _req(tgt_boxes, torch.float32, "tgt_boxes")
    _req(tgt_off, torch.int32, "tgt_off"); _req(facts, torch.int32, "facts"); _req(image_ids, torch.int64, "image_ids")
    _req(pred_masks, torch.float32, "pred_masks"); _req(tgt_masks, torch.uint8, "tgt_masks"); _req(veto, torch.int32, "veto")
    assert tuple(valid_u8.shape) == (B, P, K) and tgt_off.numel() == B + 1 and facts.numel() == 6 * B and image_ids.numel() == B
    assert pred_boxes.is_contiguous() and valid_u8.is_contiguous() and tgt_boxes.is_contiguous()
    assert state.B == B and state.P == P and state.acc.numel() == EVAL_SLOTS
    Q = h = w = Hc = Wc = 0
    iou_det, iou_seg, iu, partials = out if out is not None else (None, None, None, None)
    if iou_det is None:
        iou_det = _new((B, P), torch.float32, pred_boxes)
    if pred_masks is not None:
        assert tgt_masks is not None and pred_masks.dim() == 4 and pred_masks.shape[0] == B and pred_masks.is_contiguous()
        Q, h, w = (int(v) for v in pred_masks.shape[1:])
        Hc, Wc = (int(v) for v in tgt_masks.shape[-2:])
        assert tgt_masks.numel() == B * Hc * Wc and tgt_masks.is_contiguous()
        if iou_seg is None:
            partials = _new((B, max(1, -(-(Hc * Wc) // EVAL_CHUNK)), 2), torch.int32, pred_boxes)
            iou_seg = _new((B,), torch.float32, pred_boxes)
            iu = _new((B, 2), torch.int64, pred_boxes)
    _call("rt_eval_canvas", _desc(
        EvalCanvasArgs, pred_boxes=pred_boxes, valid=valid_u8, tgt_boxes=tgt_boxes, tgt_off=tgt_off, facts=facts, image_ids=image_ids,
        pred_masks=pred_masks, tgt_masks=tgt_masks if pred_masks is not None else None, partials=partials, iou_det=iou_det,
        iou_seg=iou_seg, iu=iu, acc=state.acc, ring_boxes=state.boxes, ring_counts=state.counts, ring_ids=state.ids, cursor=state.cursor,
        veto=veto, B=B, P=P, K=K, Q=Q, h=h, w=w, Hc=Hc, Wc=Wc, tgt_rows=int(tgt_boxes.shape[0]), slots=state.slots,
        threshold=float(threshold)))
    return iou_det, iou_seg, iu


def eval_orig_chunks(max_pixels):
    """The chunks per image of rt_eval_orig's grid and partials: ceil(max_pixels / EVAL_CHUNK)."""
    return max(1, -(-int(max_pixels) // EVAL_CHUNK))


class EvalOrigState:
    """What rt_eval_orig reads and writes beside the model's logits, for batches of B images of at most `max_pixels` original pixels:
    mask_table int64 [B] (rt_eval_raw_facts writes it), partials int32 [B, eval_orig_chunks(max_pixels), 2], iou_seg fp32 [B], iu int64
    [B, 2].  `acc` (int64 [EVAL_ORIG_SLOTS], slot EVAL_ORIG_SUM holds a double) is handed in or made here, zeroed once by the caller."""

    def __init__(self, B, max_pixels, device, acc=None):
        self.B, self.max_pixels = int(B), int(max_pixels)
        self.acc = torch.zeros(EVAL_ORIG_SLOTS, dtype=torch.int64, device=device) if acc is None else acc
        self.mask_table = torch.zeros(self.B, dtype=torch.int64, device=device)
        self.partials = torch.zeros((self.B, eval_orig_chunks(self.max_pixels), 2), dtype=torch.int32, device=device)
        self.iou_seg = torch.zeros(self.B, dtype=torch.float32, device=device)
        self.iu = torch.zeros((self.B, 2), dtype=torch.int64, device=device)


def eval_raw_facts(sizes, origs, canvas_hw, facts, image_ids, ids=None, mask_list=None, mask_table=None, max_pixels=0):
    """rt_eval_raw_facts: sizes / origs: B (h, w) pairs of python ints (resized, raw), canvas_hw = (Hc, Wc), ids: B python ints (None:
    -1) -> facts int32 [B, 6] (rt_eval_facts' layout, the mask extent = the resized size), image_ids int64 [B]; with mask_list (B
    one-byte raw masks on the device, image b's of orig_h * orig_w bytes) also mask_table int64 [B] = their addresses, for rt_eval_orig
    with a grid sized for `max_pixels`.  Every value goes by value in the kernel arguments: nothing is copied to the device and
    nothing synchronises.  The caller keeps the masks alive until the kernels that read the table have run."""
    B, n = len(sizes), BATCH_STAGE_MAX_B
    _req(facts, torch.int32, "facts"); _req(image_ids, torch.int64, "image_ids"); _req(mask_table, torch.int64, "mask_table")
    assert 0 < B <= n and len(origs) == B and facts.numel() == 6 * B and image_ids.numel() == B and facts.is_contiguous()
    assert ids is None or len(ids) == B
    tm = (c_void_p * n)()
    if mask_table is not None:
        assert mask_list is not None and len(mask_list) == B and mask_table.numel() == B
        for t, (oh, ow) in zip(mask_list, origs):
            assert t.is_cuda and t.element_size() == 1 and t.is_contiguous() and t.numel() == int(oh) * int(ow), (t.dtype, tuple(t.shape))
        tm = (c_void_p * n)(*[t.data_ptr() for t in mask_list])
    _call("rt_eval_raw_facts", _desc(
        EvalRawFactsArgs, facts=facts, image_ids=image_ids, mask_table=mask_table, max_pixels=int(max_pixels), B=B,
        Hc=int(canvas_hw[0]), Wc=int(canvas_hw[1]), has_ids=0 if ids is None else 1,
        img_h=(c_int32 * n)(*[int(s[0]) for s in sizes]), img_w=(c_int32 * n)(*[int(s[1]) for s in sizes]),
        orig_h=(c_int32 * n)(*[int(s[0]) for s in origs]), orig_w=(c_int32 * n)(*[int(s[1]) for s in origs]),
        image_id=(c_int64 * n)(*([int(v) for v in ids] if ids is not None else [])), tm_ptr=tm))


def eval_orig(pred_masks, facts, state, canvas_hw, threshold=0.5, veto=None):
    """rt_eval_orig for one batch: pred_masks fp32 [B, Q, h, w] (query 0 of every image is scored), facts / state.mask_table what
    eval_raw_facts wrote, state an EvalOrigState (accumulators updated in place), canvas_hw = (Hc, Wc) the frame of the mask decision.
    veto: device int32 word; non-zero at run time -> the accumulators stay as they were.  Two launches, device memory only: it can be
    captured and replayed.  Returns (iou_seg fp32 [B], iu int64 [B, 2]) of this batch, views of the state."""
    _req(pred_masks, torch.float32, "pred_masks"); _req(facts, torch.int32, "facts"); _req(veto, torch.int32, "veto")
    assert pred_masks.dim() == 4 and pred_masks.is_contiguous() and facts.is_contiguous()
    B, Q, h, w = (int(v) for v in pred_masks.shape)
    assert state.B == B and facts.numel() == 6 * B and state.acc.numel() == EVAL_ORIG_SLOTS and state.acc.dtype == torch.int64
    assert state.partials.numel() == B * eval_orig_chunks(state.max_pixels) * 2
    _call("rt_eval_orig", _desc(
        EvalOrigArgs, pred_masks=pred_masks, facts=facts, mask_table=state.mask_table, partials=state.partials, iou_seg=state.iou_seg,
        iu=state.iu, acc=state.acc, veto=veto, max_pixels=state.max_pixels, B=B, Q=Q, h=h, w=w, Hc=int(canvas_hw[0]), Wc=int(canvas_hw[1]),
        threshold=float(threshold)))
    return state.iou_seg, state.iu


def predict_layout(Q, origs):
    """The mask blocks of a prediction batch (rt_predict_facts' rule, on the host): image b's Q * orig_h * orig_w bytes start at the
    16-byte unit off16[b]; -> [off16[0] = 0, ..., off16[B]] as python ints.  16 * off16[B] is the batch's used bytes."""
    off = [0]
    for oh, ow in origs:
        off.append(off[-1] + -(-(int(Q) * int(oh) * int(ow)) // 16))
    return off


class PredictState:
    """What rt_predict_canvas writes, as ONE device block so that a batch's results leave in one copy: the header -- out_boxes fp32
    [B, P, 4], then out_counts int32 [B], rounded up to 16 bytes -- and behind it the mask buffer of `capacity` bytes (a multiple of
    16; 0 without masks).  `facts` int32 [B, PREDICT_FACTS_WORDS] is rt_predict_facts' table."""

    def __init__(self, B, P, device, mask_capacity=0):
        self.B, self.P = int(B), int(P)
        self.capacity = -(-int(mask_capacity) // 16) * 16
        nb = self.B * self.P * 16
        self.header_bytes = -(-(nb + self.B * 4) // 16) * 16
        self.block = torch.zeros(self.header_bytes + self.capacity, dtype=torch.uint8, device=device)
        self.out_boxes = self.block[:nb].view(torch.float32).view(self.B, self.P, 4)
        self.out_counts = self.block[nb:nb + self.B * 4].view(torch.int32)
        self.masks = self.block[self.header_bytes:]
        self.facts = torch.zeros((self.B, PREDICT_FACTS_WORDS), dtype=torch.int32, device=device)


def predict_facts(sizes, origs, canvas_hw, facts, Q=0, capacity=0):
    """rt_predict_facts: sizes / origs: B (h, w) pairs of python ints (resized, original), canvas_hw = (Hc, Wc), Q mask queries per
    image (0: none), capacity: the mask buffer's bytes -> facts int32 [B, PREDICT_FACTS_WORDS] (predict_layout's offsets).  Every
    value goes by value in the kernel arguments: nothing is copied to the device and nothing synchronises."""
    B, n = len(sizes), BATCH_STAGE_MAX_B
    _req(facts, torch.int32, "facts")
    assert 0 < B <= n and len(origs) == B and facts.numel() == PREDICT_FACTS_WORDS * B and facts.is_contiguous()
    _call("rt_predict_facts", _desc(
        PredictFactsArgs, facts=facts, capacity=int(capacity), B=B, Q=int(Q), Hc=int(canvas_hw[0]), Wc=int(canvas_hw[1]),
        img_h=(c_int32 * n)(*[int(s[0]) for s in sizes]), img_w=(c_int32 * n)(*[int(s[1]) for s in sizes]),
        orig_h=(c_int32 * n)(*[int(s[0]) for s in origs]), orig_w=(c_int32 * n)(*[int(s[1]) for s in origs])))


def predict_canvas(pred_boxes, valid_u8, state, pred_masks=None, canvas_hw=None, threshold=0.5):
    """rt_predict_canvas for one canvas batch: pred_boxes fp32 [B, P, K, 4], valid uint8 [B, P, K], state a PredictState whose facts
    predict_facts wrote -> state.out_boxes / out_counts and, with pred_masks fp32 [B, Q, h, w] and canvas_hw = (Hc, Wc), the packed
    masks_origin blocks in state.masks.  At most two launches, device memory only: it can be captured and replayed."""
    B, P, K, _ = pred_boxes.shape
    _req(pred_boxes, torch.float32, "pred_boxes"); _req(valid_u8, torch.uint8, "valid"); _req(pred_masks, torch.float32, "pred_masks")
    assert tuple(valid_u8.shape) == (B, P, K) and pred_boxes.is_contiguous() and valid_u8.is_contiguous()
    assert state.B == B and state.P == P
    Q = h = w = Hc = Wc = 0
    if pred_masks is not None:
        assert pred_masks.dim() == 4 and pred_masks.shape[0] == B and pred_masks.is_contiguous() and canvas_hw is not None
        Q, h, w = (int(v) for v in pred_masks.shape[1:])
        Hc, Wc = int(canvas_hw[0]), int(canvas_hw[1])
    _call("rt_predict_canvas", _desc(
        PredictCanvasArgs, pred_boxes=pred_boxes, valid=valid_u8, facts=state.facts, pred_masks=pred_masks, out_boxes=state.out_boxes,
        out_counts=state.out_counts, out_masks=state.masks if pred_masks is not None else None, capacity=state.capacity,
        B=B, P=P, K=K, Q=Q, h=h, w=w, Hc=Hc, Wc=Wc, threshold=float(threshold)))


def zero_chunks(base, table, n):
    """Clears n chunks {element offset, count} (static device int64 table) of the fp32 buffer `base` in one launch."""
    _req(base, torch.float32, "base"); _req(table, torch.int64, "table")
    _call("rt_zero_chunks", base, table, int(n))


def sqnorm(g, out):
    if g.dtype == torch.bfloat16:
        _call("rt_sqnorm_bf16", g, g.numel(), out)
    else:
        _call("rt_sqnorm", g, g.numel(), out)


def grad_accum(mode, g, acc, scale=1.0, scale_dev=None, partials=None, out_sq=None):
    """rt_grad_accum over the fp32 buffers g / acc (same element count): ACCUM_FIRST acc = g, ACCUM_ADD acc += g, ACCUM_FINISH
    g = (acc + g) * scale with out_sq[0] = sum g^2 (`partials`: GRAD_ACCUM_SLOTS floats of workspace; `scale_dev`: a device float
    read instead of `scale`)."""
    _req(g, torch.float32, "g"); _req(acc, torch.float32, "acc")
    _req(scale_dev, torch.float32, "scale_dev"); _req(partials, torch.float32, "partials"); _req(out_sq, torch.float32, "out_sq")
    assert g.is_contiguous() and acc.is_contiguous() and g.numel() == acc.numel()
    assert partials is None or partials.numel() >= GRAD_ACCUM_SLOTS
    _call("rt_grad_accum", int(mode), g, acc, g.numel(), float(scale), scale_dev, partials, out_sq)


def adamw_flat(p, g, m, v, *, step, ranges, gnorm_sq=None, gnorm_out=None, grad_scale=1.0, max_norm=0.0,
               beta1=0.9, beta2=0.999, eps=1e-8, step_dev=None, active=None, lr_dev=None, span=None, g16=None, sgd=False,
               mat=None, chunks=None):
    """ranges = [(begin, end, lr, wd), ...] element ranges of the flat buffers (multiples of 4); span = (begin, end)
    restricts the launch to that element span; active / lr_dev: device words (see rt_adamw_desc).  sgd=True: rt_sgd_flat
    (m = momentum buffer, beta1 = momentum, v unused).  mat = (device job table, njobs, total tiles) and / or chunks = (device
    chunk table, nchunks): the matrix-aware form (rt_adamw_mat + rt_adamw_chunks) that also emits the bf16 operands; the
    tables say what is updated and `span` is ignored."""
    span_begin, span_end = (0, 0) if span is None else span
    begins, ends, lrs, wds = zip(*ranges) if ranges else ((), (), (), ())
    d = _desc(AdamWDesc, p=p, g=g, m=m, v=v, n=p.numel(), gnorm_sq=gnorm_sq, gnorm_out=gnorm_out, grad_scale=grad_scale,
              max_norm=max_norm, beta1=beta1, beta2=beta2, eps=eps, step=step, n_ranges=len(ranges), range_begin=begins, range_end=ends,
              range_lr=lrs, range_wd=wds, step_dev=step_dev, active=active, lr_dev=lr_dev, span_begin=span_begin, span_end=span_end,
              g16=g16)
    if mat is not None or chunks is not None:
        assert not sgd
        if mat is not None and mat[1] > 0:
            _call("rt_adamw_mat", d, mat[0], mat[1], mat[2])
        if chunks is not None and chunks[1] > 0:
            _call("rt_adamw_chunks", d, chunks[0], chunks[1])
    elif sgd:
        _call("rt_sgd_flat", d)
    else:
        _call("rt_adamw_flat", d)


def small_dgrad(dy_f32, w_f32, gate=None):
    """dx bf16 [M,K] = gate(dy[M,N<=8] @ w[N,K])."""
    M, N = dy_f32.shape
    K = w_f32.shape[1]
    dx = _new((M, K), torch.bfloat16, dy_f32)
    _call("rt_small_dgrad", dy_f32, w_f32, gate, dx, M, N, K)
    return dx


def pos_grad(dpos, d_lang_pos, d_type, d_level, B, S, L):
    E = dpos.shape[1]
    _call("rt_pos_grad", dpos, d_lang_pos, d_type, d_level, B, S, L, E)


def counter_add(ctr, inc=1, unless=None, reset_else=False):
    """*ctr += inc on the device; `unless` (a device word): only while it is 0, else *ctr is left alone or -- reset_else --
    cleared (rt_counter_add_if_zero)."""
    if unless is not None:
        _call("rt_counter_add_if_zero", ctr, inc, unless, int(bool(reset_else)))
    else:
        _call("rt_counter_add", ctr, inc)


def finish_step(step_dev, active, veto=None, loss=None):
    """*step_dev += 1, *active += 1 unless the veto word is set or the loss is not finite; else *active = 0 (rt_finish_step)."""
    _req(loss, torch.float32, "loss")
    _call("rt_finish_step", step_dev, active, veto, loss)


def finish_stats(step_dev, active, veto, loss, sq, norm_scale, grad_norm, srcs=(), cond_in_stats=False, stats=None):
    """rt_finish_stats: the iteration's counters (as finish_step), grad_norm = sqrt(sq) * norm_scale and the stats vector
    [*srcs | float(veto word) | grad_norm] in one launch.  `srcs`: fp32 device scalars (tensors of one element)."""
    assert len(srcs) <= STATS_MAX
    for t in list(srcs) + [loss, sq, grad_norm, stats]:
        _req(t, torch.float32, "finish_stats operand")
    if stats is not None:
        assert stats.numel() == len(srcs) + int(bool(cond_in_stats)) + 1
    _call("rt_finish_stats", _desc(FinishDesc, step=step_dev, active=active, cond=veto, loss=loss, sq=sq, norm_scale=float(norm_scale),
                                   grad_norm=grad_norm, src=list(srcs), n_src=len(srcs), cond_in_stats=int(bool(cond_in_stats)), stats=stats))


def stamp(buf, idx):
    """buf[idx] (int64 device tensor) = the device's 100 MHz wall clock when the current stream gets here (rt_stamp)."""
    assert buf.dtype == torch.int64 and 0 <= idx < buf.numel()
    _call("rt_stamp", buf, idx)


# Measurement aid (tools/concurrent_timeline.py): wall-clock stamps at named points of a step, on whatever stream reaches them.
# rocprofv3 serialises the concurrent streams of a replayed graph, so the step's real timeline is taken from inside the graph: with
# stamping enabled BEFORE the step is captured, every `mark` is a one-thread kernel node writing the device's 100 MHz clock.
_MARKS = None


def enable_marks(device, capacity=256):
    """Turns `mark` on: returns {'buf': int64 device tensor, 'names': {name: (slot, stream)}}.  Call before capturing the step."""
    global _MARKS
    _MARKS = {"buf": torch.zeros(capacity, dtype=torch.int64, device=device), "names": {}}
    return _MARKS


def disable_marks():
    global _MARKS
    _MARKS = None


def mark(name):
    """No-op unless enable_marks() was called (one global read)."""
    m = _MARKS
    if m is None:
        return
    ent = m["names"].get(name)
    if ent is None:
        ent = m["names"][name] = (len(m["names"]), torch.cuda.current_stream().cuda_stream)
    stamp(m["buf"], ent[0])


def decoder_supported(F=2048):
    """True when the cooperative decoder launches may be used on the current device (co-residency check, rt_decoder_supported)."""
    return lib().rt_decoder_supported(int(F)) == 0


def decoder_set_spin(spin):
    _call("rt_decoder_set_spin", int(spin), stream=False)


class WgradBatch:
    """Linear weight gradients queued during backward (they are off the backward-data dependency chain) and launched as
    one group (rt_conv_wgrad_grouped).  `workspace_mb`: scratch for the split partials of the whole group."""

    _WS = {}

    def __init__(self, workspace_mb=512):
        self.descs, self.keep, self.ws_bytes = [], [], workspace_mb << 20
        self.flops = self.nbytes = 0.0

    def _account(self, geom):
        self.flops += 2.0 * geom[0] * geom[4] * geom[5] * geom[6] * geom[7] * geom[8] * geom[3]
        self.nbytes += _algo_bytes(("W",) + tuple(geom))

    def add(self, dy, x, dw, dbias=None, overwrite=False):
        _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(dw, torch.float32, "dw"); _req(dbias, torch.float32, "dbias")
        M, N = dy.shape
        K = x.shape[1]
        assert x.shape[0] == M and dw.numel() == N * K
        geom = (M, 1, 1, K, 1, 1, N, 1, 1, 1, 0)
        self.descs.append(_wgrad_desc(dy, x, dw, geom, dbias=dbias, overwrite=int(bool(overwrite))))
        self.keep.append((dy, x))
        self._account(geom)

    def add_conv(self, dy, x, dw, geom, scale=None, overwrite=False, dil=1, dbias=None):
        """A convolution weight gradient (any geometry: the non-groupable ones are forwarded to rt_conv_wgrad at run())."""
        _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(dw, torch.float32, "dw"); _req(scale, torch.float32, "scale")
        _req(dbias, torch.float32, "dbias")
        self.descs.append(_wgrad_desc(dy, x, dw, geom, scale=scale, dbias=dbias, overwrite=int(bool(overwrite)), dil=int(dil)))
        self.keep.append((dy, x, scale))
        self._account(geom)

    def run(self):
        if not self.descs:
            return
        dev = self.keep[0][0].device
        key = (dev.index, torch.cuda.current_stream().cuda_stream, self.ws_bytes)
        ws = WgradBatch._WS.get(key)
        if ws is None:
            ws = WgradBatch._WS[key] = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=dev)
        single = _wgrad_workspace(dev)          # for the descriptors that are forwarded to rt_conv_wgrad (this stream's)
        for d in self.descs:
            _set(d, workspace=single, workspace_bytes=WGRAD_WS_BYTES)
        arr = (ConvWgradDesc * len(self.descs))(*self.descs)
        n = len(self.descs)
        _timed("conv_wgrad_grouped", self.flops,
               lambda: _call("rt_conv_wgrad_grouped", arr, n, ws, self.ws_bytes), nbytes=self.nbytes)
        self.descs, self.keep = [], []
        self.flops = self.nbytes = 0.0


class SmallWgradBatch:
    """Weight gradients of Linears over <= 16 token rows, queued during backward and launched together
    (rt_small_wgrad_grouped): they are off the backward-data dependency chain, so ~50 launch latencies become one."""

    def __init__(self):
        self.jobs, self.keep = [], []
        self.flops = self.nbytes = 0.0

    def add(self, dy, x, dw, dbias=None, overwrite=False):
        _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(dw, torch.float32, "dw"); _req(dbias, torch.float32, "dbias")
        M, N = dy.shape
        K = x.shape[1]
        assert M <= 16 and x.shape[0] == M and dw.numel() == N * K and K % 4 == 0
        self.jobs.append(_desc(SmallWgradJob, dy=dy, x=x, dw=dw, dbias=dbias, M=M, N=N, K=K, overwrite=int(bool(overwrite)),
                               sqacc=_sqacc(dw), g16=_g16(dw)))
        self.keep.append((dy, x))
        self.flops += 2.0 * M * N * K; self.nbytes += 2.0 * M * (N + K) + 4.0 * N * K

    def run(self):
        if not self.jobs:
            return
        arr = (SmallWgradJob * len(self.jobs))(*self.jobs)
        n = len(self.jobs)
        _timed("small_wgrad_grouped", self.flops, lambda: _call("rt_small_wgrad_grouped", arr, n), nbytes=self.nbytes)
        self.jobs, self.keep = [], []
        self.flops = self.nbytes = 0.0


class WeightPrepBatch:
    """All per-step operand refreshes as ONE launch: jobs are (src fp32 [N,T,C], scale|None, dst|None, dst_t|None)."""

    def __init__(self, device):
        self.jobs, self.device, self.table, self.tiles = [], device, None, 0
        self._keep = []

    def add(self, src, N, T, C, scale=None, dst=None, dst_t=None):
        assert src.is_contiguous() and src.numel() == N * T * C
        self.jobs.append([_p(src), _p(scale) or 0, _p(dst) or 0, _p(dst_t) or 0, N, T, C, self.tiles])
        self.tiles += ((N + 63) // 64) * ((C + 63) // 64) * T
        self._keep.append((src, scale, dst, dst_t))
        self.table = None

    def run(self):
        if not self.jobs:
            return
        if self.table is None:
            self.table = torch.tensor(self.jobs, dtype=torch.int64).to(self.device)
        _call("rt_weight_prep_batched", self.table, len(self.jobs), self.tiles)


# --------------------------------------------------------------------------------------------
# RES head (RefTRSeg) kernels
# --------------------------------------------------------------------------------------------
def gn_nhwc_blocks(HW, C):
    """Workgroups per image of rt_gn_nhwc_fwd's statistics pass (gn_nhwc_ppb in csrc/rt_seg.hip: about 4096 elements per workgroup):
    the rows of the `partials` workspace the caller has to bring."""
    ppb = max(1, (4096 + C - 1) // C)
    return (HW + ppb - 1) // ppb


def gn_nhwc_fwd(x, gamma, beta, B, HW, C, G=8, ldy=None, act=ACT_RELU, eps=1e-5):
    """y = [relu](GroupNorm(G, C)(x)) as a bf16 [B*HW, ldy] operand (padding zero); returns (y_bf16, stats)."""
    _req(x, torch.float32, "x"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta")
    ldx = x.shape[-1]
    ldy = ldy or ldx
    assert x.numel() == B * HW * ldx and gamma.numel() >= C
    y = torch.empty((B * HW, ldy), dtype=torch.bfloat16, device=x.device)
    stats = torch.empty((B, G, 2), dtype=torch.float32, device=x.device)
    nblk = gn_nhwc_blocks(HW, C)
    partials = torch.empty((B, nblk, G, 2), dtype=torch.float32, device=x.device)
    _call("rt_gn_nhwc_fwd", _desc(GnNhwcDesc, x=x, gamma=gamma, beta=beta, stats=stats, y_bf16=y, B=B, HW=HW, C=C, G=G, ldx=ldx, ldy=ldy,
                                  act=act, eps=eps, partials=partials, partial_blocks=nblk))
    return y, stats


def gn_nhwc_bwd(dy, x, gamma, beta, stats, dgamma, dbeta, B, HW, C, G=8, lddx=None, act=ACT_RELU, eps=1e-5):
    """dx (bf16 [B*HW, lddx], the producing convolution's output gradient); dgamma / dbeta accumulated."""
    _req(dy, torch.float32, "dy"); _req(x, torch.float32, "x")
    ldx, lddy = x.shape[-1], dy.shape[-1]
    lddx = lddx or ldx
    dx = torch.empty((B * HW, lddx), dtype=torch.bfloat16, device=x.device)
    bst = torch.empty((B, G, 2), dtype=torch.float32, device=x.device)
    _call("rt_gn_nhwc_bwd", _desc(GnNhwcBwdDesc, dy=dy, x=x, gamma=gamma, beta=beta, stats=stats, bstats=bst, dx_bf16=dx, dgamma=dgamma,
                                  dbeta=dbeta, B=B, HW=HW, C=C, G=G, ldx=ldx, lddy=lddy, lddx=lddx, act=act, eps=eps))
    return dx


def upsample_add(fpn, a, B, H, W, h, w, C, ldo=None):
    """bf16(fpn + nearest_upsample(a)): fpn fp32 [B*H*W, ldf], a bf16 [B*h*w, lda] -> bf16 [B*H*W, ldo]."""
    _req(fpn, torch.float32, "fpn"); _req(a, torch.bfloat16, "a")
    ldf, lda = fpn.shape[-1], a.shape[-1]
    ldo = ldo or ldf
    out = torch.empty((B * H * W, ldo), dtype=torch.bfloat16, device=fpn.device)
    _call("rt_upsample_add", _desc(UpsampleAddDesc, fpn=fpn, a_bf16=a, out_bf16=out, B=B, H=H, W=W, h=h, w=w, C=C, ldf=ldf, lda=lda, ldo=ldo))
    return out


def upsample_add_bwd(dy, B, H, W, h, w, C, ldda=None, lddyb=None):
    """dy fp32 [B*H*W, lddy] -> (da fp32 [B*h*w, ldda] (padding zero), bf16 copy of dy [B*H*W, lddyb])."""
    _req(dy, torch.float32, "dy")
    lddy = dy.shape[-1]
    ldda = ldda or C; lddyb = lddyb or lddy
    da = torch.zeros((B * h * w, ldda), dtype=torch.float32, device=dy.device) if ldda > C else \
        torch.empty((B * h * w, ldda), dtype=torch.float32, device=dy.device)
    dyb = torch.empty((B * H * W, lddyb), dtype=torch.bfloat16, device=dy.device)
    _call("rt_upsample_add_bwd", _desc(UpsampleAddBwdDesc, dy=dy, da=da, dy_bf16=dyb, B=B, H=H, W=W, h=h, w=w, C=C, lddy=lddy, ldda=ldda,
                                       lddyb=lddyb))
    return da, dyb


def attn_map_fwd(q, k, mask_u8, B, HW, E, nh, k_rows_per_img, k_row_off, concat=None, concat_col=0):
    _req(q, torch.float32, "q"); _req(k, torch.float32, "k"); _req(mask_u8, torch.uint8, "mask")
    P = torch.empty((B, nh, HW), dtype=torch.float32, device=q.device)
    _call("rt_attn_map_fwd", _desc(
        AttnMapDesc, q=q, k=k, mask=mask_u8, P=P, concat_bf16=concat, B=B, HW=HW, E=E, nh=nh, ldk=k.shape[-1], k_rows_per_img=k_rows_per_img,
        k_row_off=k_row_off, ld_concat=concat.shape[-1] if concat is not None else 0, concat_col=concat_col, norm=float(E / nh) ** -0.5))
    return P


def attn_map_bwd(q, k, P, dconcat, B, HW, E, nh, k_rows_per_img, k_row_off, concat_col):
    """Returns (dq fp32 [B,E], dk fp32 shaped like k: rows outside the image block are zero)."""
    _req(dconcat, torch.float32, "dconcat")
    dq = torch.empty((B, E), dtype=torch.float32, device=q.device)
    dk = torch.zeros_like(k)
    _call("rt_attn_map_bwd", _desc(
        AttnMapBwdDesc, q=q, k=k, P=P, dconcat=dconcat, dq=dq, dk=dk, B=B, HW=HW, E=E, nh=nh, ldk=k.shape[-1], k_rows_per_img=k_rows_per_img,
        k_row_off=k_row_off, ld_dconcat=dconcat.shape[-1], concat_col=concat_col, norm=float(E / nh) ** -0.5))
    return dq, dk


def seg_concat(src, mem, out, B, HW, E, nh, rows_per_img, row_off, src_dense=False):
    """src / mem rows of image b, pixel p: (b * rows_per_img + row_off + p); src_dense: src is a dense [B*HW, E]."""
    _req(src, torch.float32, "src"); _req(mem, torch.float32, "mem"); _req(out, torch.bfloat16, "out")
    _call("rt_seg_concat", _desc(
        SegConcatDesc, src=src, mem=mem, out_bf16=out, B=B, HW=HW, E=E, nh=nh, ldo=out.shape[-1], mem_rows_per_img=rows_per_img,
        mem_row_off=row_off, src_rows_per_img=HW if src_dense else rows_per_img, src_row_off=0 if src_dense else row_off))
    return out


def mask_loss(pred, target_u8, B, h, w, Ht, Wt, ldp, norm, sums=None, dpred=None, g_focal=None, g_dice=None):
    """Forward (dpred None): returns (losses[2] = {focal, dice}, sums [B,4]).  Backward: accumulates into dpred."""
    _req(pred, torch.float32, "pred"); _req(target_u8, torch.uint8, "target")
    assert target_u8.numel() == B * Ht * Wt
    common = dict(pred=pred, target=target_u8, B=B, h=h, w=w, Ht=Ht, Wt=Wt, ldp=ldp, inv_norm=1.0 / norm)
    if dpred is None:
        sums = torch.empty((B, 4), dtype=torch.float32, device=pred.device)
        losses = torch.empty(2, dtype=torch.float32, device=pred.device)
        partials = torch.empty((B, MASK_LOSS_PARTIALS), dtype=torch.float32, device=pred.device)      # fixed-order sums: no atomics
        _call("rt_mask_loss", _desc(MaskLossDesc, sums=sums, losses=losses, gbuf=partials, **common))
        return losses, sums
    _req(dpred, torch.float32, "dpred"); _req(g_focal, torch.float32, "g_focal"); _req(g_dice, torch.float32, "g_dice")
    gbuf = torch.empty(B * Ht * Wt, dtype=torch.float32, device=pred.device)
    _call("rt_mask_loss", _desc(MaskLossDesc, sums=sums, dpred=dpred, g_focal=g_focal, g_dice=g_dice, lddp=dpred.shape[-1], gbuf=gbuf,
                                **common))
    return dpred


# --------------------------------------------------------------------------------------------
# input pipeline kernels
# --------------------------------------------------------------------------------------------
def resample_u8(src, bounds, coeffs, out_len, axis):
    """One Pillow-compatible resampling pass of a uint8 [n0, n1, C] image along `axis` (0 vertical / 1 horizontal)."""
    _req(src, torch.uint8, "src"); _req(bounds, torch.int32, "bounds"); _req(coeffs, torch.int32, "coeffs")
    n0, n1, C = src.shape
    shape = (out_len, n1, C) if axis == 0 else (n0, out_len, C)
    dst = torch.empty(shape, dtype=torch.uint8, device=src.device)
    _call("rt_resample_u8", src, dst, bounds, coeffs, n0, n1, C, out_len, coeffs.shape[1], axis)
    return dst


def img_collate_norm(images, H, W, mean, std):
    """images: list of uint8 [h, w, 3] device tensors -> (fp32 [B,3,H,W] normalised + zero padded, uint8 mask [B,H,W])."""
    B = len(images)
    for im in images:
        _req(im, torch.uint8, "image")
        assert im.dim() == 3 and im.shape[2] == 3 and im.shape[0] <= H and im.shape[1] <= W
    dev = images[0].device
    tab = torch.tensor([[im.data_ptr(), im.shape[0], im.shape[1]] for im in images], dtype=torch.int64).to(dev, non_blocking=True)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    m = (c_float * 3)(*[float(v) for v in mean]); s_ = (c_float * 3)(*[float(v) for v in std])
    _call("rt_img_collate_norm", tab, out, mask, B, H, W, m, s_)
    return out, mask


def _stage_dst(B, img, mask, boxes_per_image, boxes, tgt_off, num_boxes, mask_list, tgt_masks):
    """The destination checks of a stage call (rt_batch_stage, rt_raw_stage): the canvas buffers of a batch of B -> (Hc, Wc)."""
    _req(img, torch.float32, "img"); _req(boxes, torch.float32, "boxes"); _req(tgt_off, torch.int32, "tgt_off"); _req(num_boxes, torch.float32, "num_boxes")
    Hc, Wc = img.shape[-2:]
    assert img.is_contiguous() and mask.is_contiguous() and mask.element_size() == 1
    assert tuple(img.shape) == (B, 3, Hc, Wc) and tuple(mask.shape) == (B, Hc, Wc)
    assert boxes.numel() == B * boxes_per_image * 4 and tgt_off.numel() == B + 1 and num_boxes.numel() == 1
    if mask_list is not None:
        assert len(mask_list) == B and tgt_masks is not None and tgt_masks.numel() == B * Hc * Wc and tgt_masks.element_size() == 1
        assert all(t.is_cuda and t.element_size() == 1 and t.is_contiguous() and t.numel() == t.shape[-2] * t.shape[-1] for t in mask_list)
    return Hc, Wc


def _stage_boxes(box_list, B, n):
    """The box arguments of a stage call: ctypes arrays (pointers, counts) of length n >= B; an image without boxes passes NULL."""
    assert len(box_list) == B
    for t in box_list:
        assert t.numel() == 0 or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape[-1] == 4)
    return (c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in box_list]), (c_int32 * n)(*[t.shape[0] for t in box_list])


def batch_stage(src_img, src_mask, img, mask, box_list, boxes_per_image, boxes, tgt_off, num_boxes, mask_list=None, tgt_masks=None):
    """rt_batch_stage: one batch of any size into fixed canvas buffers, one launch, every destination byte rewritten.
    src_img fp32 [B,3,hs,ws] / src_mask bool|u8 [B,hs,ws] -> img fp32 [B,3,Hc,Wc] (zero padded) / mask [B,Hc,Wc] (1 = padding);
    box_list: B fp32 [n_b, 4] device tensors -> boxes [B*boxes_per_image, 4] packed, tgt_off int32 [B+1], num_boxes fp32 [1];
    mask_list (optional): B one-byte [1, h_b, w_b] device tensors -> tgt_masks u8 [B,1,Hc,Wc].  The pointers and sizes go by value in
    the kernel arguments: nothing is copied to the device and nothing synchronises."""
    _req(src_img, torch.float32, "src_img")
    B, _, hs, ws = src_img.shape
    Hc, Wc = _stage_dst(B, img, mask, boxes_per_image, boxes, tgt_off, num_boxes, mask_list, tgt_masks)
    assert src_img.is_contiguous() and src_mask.is_contiguous() and src_mask.element_size() == 1 and tuple(src_mask.shape) == (B, hs, ws)
    bp, bn = _stage_boxes(box_list, B, B)
    tp = (c_void_p * B)(*[t.data_ptr() for t in mask_list]) if mask_list is not None else None
    thw = (c_int32 * (2 * B))(*[v for t in mask_list for v in t.shape[-2:]]) if mask_list is not None else None
    _call("rt_batch_stage", src_img, src_mask, B, hs, ws, img, mask, Hc, Wc, bp, bn, int(boxes_per_image), boxes, tgt_off, num_boxes, tp, thw,
          tgt_masks if mask_list is not None else None)


def raw_stage(images, out_sizes, img, mask, box_list, boxes_per_image, boxes, tgt_off, num_boxes, mean, std, mask_list=None,
              tgt_masks=None):
    """rt_raw_stage: one batch of raw images into fixed canvas buffers, one launch, every destination byte rewritten.
    images: B uint8 [h_b, w_b, 3] device tensors, out_sizes: their resized (oh_b, ow_b) (resample.size_with_aspect_ratio) ->
    img fp32 [B,3,Hc,Wc] (Pillow's bilinear resize, ToTensor, Normalize, zero padded) / mask [B,Hc,Wc] (1 = padding);
    box_list: B fp32 [n_b, 4] xyxy pixels of the raw frame -> boxes [B*boxes_per_image, 4] cxcywh normalised and packed, tgt_off
    int32 [B+1], num_boxes fp32 [1]; mask_list (optional): B one-byte [1, h_b, w_b] raw masks -> tgt_masks u8 [B,1,Hc,Wc] (nearest).
    Every pointer and size goes by value in the kernel arguments: nothing is copied to the device and nothing synchronises."""
    B = len(images)
    assert 0 < B <= BATCH_STAGE_MAX_B and len(out_sizes) == B
    Hc, Wc = _stage_dst(B, img, mask, boxes_per_image, boxes, tgt_off, num_boxes, mask_list, tgt_masks)
    assert all(t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 3 for t in images)
    assert mask_list is None or all(tuple(t.shape[-2:]) == tuple(im.shape[:2]) for t, im in zip(mask_list, images))
    hs, ws = [t.shape[0] for t in images], [t.shape[1] for t in images]
    ohs, ows = [int(s[0]) for s in out_sizes], [int(s[1]) for s in out_sizes]
    n = BATCH_STAGE_MAX_B          # (ready-made ctypes arrays: _desc copies them as they are, a list it would convert element by element)
    bp, bn = _stage_boxes(box_list, B, n)
    _call("rt_raw_stage", _desc(
        RawStageArgs, img=img, mask=mask, tgt_masks=tgt_masks if mask_list is not None else None, boxes=boxes, tgt_off=tgt_off,
        num_boxes=num_boxes, B=B, Hc=Hc, Wc=Wc, boxes_per_image=int(boxes_per_image), mean=(c_float * 3)(*mean), std=(c_float * 3)(*std),
        src=(c_void_p * n)(*[t.data_ptr() for t in images]), box_ptr=bp, box_n=bn,
        tm_ptr=(c_void_p * n)(*[t.data_ptr() for t in mask_list]) if mask_list is not None else (c_void_p * n)(),
        h=(c_int32 * n)(*hs), w=(c_int32 * n)(*ws), oh=(c_int32 * n)(*ohs), ow=(c_int32 * n)(*ows),
        rw=(c_float * n)(*[float(o) / float(i) for o, i in zip(ows, ws)]), rh=(c_float * n)(*[float(o) / float(i) for o, i in zip(ohs, hs)])))


def hsv_jitter(images, gains, out_list):
    """rt_hsv_jitter: the colour jitter of reftr_amd.data.jitter.apply on B raw images, one launch.  images: B uint8 [h_b, w_b, 3]
    device tensors, gains: B (s_gain, v_gain) host floats, out_list: B uint8 device tensors of h_b * w_b * 3 bytes each (out_list[b]
    may be images[b] itself; any alignment -- 16-byte aligned pairs take the 16-byte accesses).  Every pointer, size and gain goes by
    value in the kernel arguments: nothing is copied to the device and nothing synchronises."""
    B, n = len(images), BATCH_STAGE_MAX_B
    assert 0 < B <= n and len(gains) == B and len(out_list) == B
    assert all(t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 3 for t in images)
    assert all(o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and o.numel() == t.numel() for o, t in zip(out_list, images))
    _call("rt_hsv_jitter", _desc(
        HsvJitterArgs, B=B, src=(c_void_p * n)(*[t.data_ptr() for t in images]), dst=(c_void_p * n)(*[o.data_ptr() for o in out_list]),
        h=(c_int32 * n)(*[t.shape[0] for t in images]), w=(c_int32 * n)(*[t.shape[1] for t in images]),
        s_gain=(c_float * n)(*[float(g[0]) for g in gains]), v_gain=(c_float * n)(*[float(g[1]) for g in gains])))


def resample_taps(in_size, out_size, ksize, device="cuda"):
    """rt_resample_taps: the filter taps rt_raw_stage computes for one axis -> (bounds int32 [out, 2], coeffs int32 [out, ksize])."""
    bounds = torch.empty((out_size, 2), dtype=torch.int32, device=device)
    coeffs = torch.empty((out_size, ksize), dtype=torch.int32, device=device)
    _call("rt_resample_taps", int(in_size), int(out_size), bounds, coeffs, int(ksize))
    return bounds, coeffs


# --------------------------------------------------------------------------------------------
# gradient exchange behind the C ABI (rt_comm_*: RCCL bound at run time)
# --------------------------------------------------------------------------------------------
class Comm:
    """One RCCL communicator of this process (one process per GPU) through rt_comm_*.  `uid` travels from rank 0 to the other
    ranks by whatever channel the caller has (reftr_amd.parallel uses the torch.distributed rendezvous that main_vg.py set up)."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _call("rt_comm_unique_id", buf, stream=False)
        return bytes(buf.raw)

    def __init__(self, uid, rank, world):
        assert len(uid) == 128
        h = c_void_p()
        _call("rt_comm_init", ctypes.create_string_buffer(uid, 128), int(rank), int(world), ctypes.byref(h), stream=False)
        self.handle, self.rank, self.world = h, rank, world

    def allreduce(self, tensors, stream=None):
        """In-place SUM all-reduce of contiguous device tensors of one dtype (fp32 or bf16), one RCCL group, asynchronous on
        `stream` (default: the current stream)."""
        tensors = [t for t in tensors if t.numel()]
        if not tensors:
            return
        dt = tensors[0].dtype
        assert dt in (torch.float32, torch.bfloat16) and all(t.dtype == dt and t.is_cuda and t.is_contiguous() for t in tensors)
        n = len(tensors)
        ptrs = (c_void_p * n)(*[t.data_ptr() for t in tensors])
        cnts = (c_int64 * n)(*[t.numel() for t in tensors])
        s = stream.cuda_stream if stream is not None else _stream()
        _call("rt_comm_allreduce", self.handle, ptrs, cnts, n, 0 if dt == torch.float32 else 1, s, stream=False)

    def destroy(self):
        if self.handle:
            _call("rt_comm_destroy", self.handle, stream=False)
            self.handle = None


class SideStream:
    """A second HIP stream for work that is off the critical path (the BERT branch, queued weight gradients).
    `run` forks it from the current stream (event edge) -- or, with defer=True, only queues the closure until
    `flush` forks ONCE and launches the whole queue (per-launch fork edges cost more than they give inside a
    hipGraph); `join` makes the current stream wait for it.  Tensors the side work reads are kept referenced until
    the join so the caching allocator cannot hand their memory out early.  Under hipGraph capture the fork / join
    events become graph edges and the branches replay concurrently."""

    def __init__(self, enabled=True, defer=False):
        self.enabled = enabled and torch.cuda.is_available()
        self.stream = torch.cuda.Stream() if self.enabled else None
        self.defer = defer
        self.jobs = []
        self.keep = []
        self.dirty = False

    def run(self, fn, *keep):
        if not self.enabled:
            return fn()
        self.keep.extend(keep)
        if self.defer:
            self.jobs.append(fn)
            return None
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            r = fn()
        self.dirty = True
        return r

    def flush(self):
        if not self.enabled or not self.jobs:
            return
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            for fn in self.jobs:
                fn()
        self.jobs = []
        self.dirty = True

    def join(self):
        self.flush()
        if self.enabled and self.dirty:
            torch.cuda.current_stream().wait_stream(self.stream)
        self.keep.clear()
        self.dirty = False
