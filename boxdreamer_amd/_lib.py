"""ctypes binding of libboxdreamer_hip.so (the C ABI in include/boxdreamer_hip.h).

There is NO fallback: if the library is missing or a call fails, this raises.  PyTorch is used
only for device memory and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import NamedTuple

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BOXDREAMER_HIP_LIB") or os.path.join(HERE, "libboxdreamer_hip.so")   # env: deploy / A-B a build

DTYPE_BF16, DTYPE_F16, DTYPE_F32 = 0, 1, 2
PREC_BF16, PREC_F16, PREC_BF16X3, PREC_F16_OUT_BF16X3, PREC_FP8, PREC_BF16_OUT_FP8 = 0, 1, 2, 3, 4, 5
PREC_BF16X3_ATTN_X3 = 6                                # whole-path only: split-bf16 attention everywhere (7, 11, 12: removed in ABI 7)
PREC_F16C8 = 8                                         # f16 + e4m3 corrections (include/boxdreamer_hip.h)
PREC_F16_OUT_F16C8, PREC_BF16X3_OUT_F16C8 = 9, 10      # bd_attention[_q] only: f16 / split-bf16 attention, F16C8 operand out
PREC_F16C8_QK16 = 13                                   # whole-path only: F16C8 Linears, BETR's QKV split: q, k one f16 pass, v F16C8
PREC_F16X3, PREC_F16X3_ATTN_X3 = 14, 15                # split-f16 Linears (the promoted class); _ATTN_X3: split-bf16 attention everywhere
PREC_F16_OUT_F16X3, PREC_BF16X3_OUT_F16X3 = 16, 17     # bd_attention[_q] only: split-f16 planes out
F16C8_D = 11                                           # lo planes are scaled 2^D above their q plane
PREC_NAMES = {"bf16": PREC_BF16, "fp16": PREC_F16, "f16": PREC_F16, "bf16x3": PREC_BF16X3, "fp8": PREC_FP8,
              "bf16x3_attn_x3": PREC_BF16X3_ATTN_X3, "f16c8": PREC_F16C8, "f16c8_qk16": PREC_F16C8_QK16,
              "f16x3": PREC_F16X3, "f16x3_attn_x3": PREC_F16X3_ATTN_X3}
# "fp8_mixed" (configs[4], usable form): the e4m3 class with the precision-critical Linears kept in bf16 through the per-Linear
# promotion bits -- a POLICY over BD_PREC_FP8, not another library mode (fp8_mixed_policy below; the modules apply it at construction)
PREC_NAMES["fp8_mixed"] = PREC_FP8


def promoted_class(base: int) -> int:
    """Operand class a promoted Linear runs in (include/boxdreamer_hip.h: BD_PROMOTE_*)."""
    return PREC_F16X3 if base == PREC_F16C8 else (PREC_BF16 if base == PREC_FP8 else base)


def fp8_mixed_policy(depth: int, normed: bool):
    """(per-block masks, misc mask) of the mixed e4m3 mode.  e4m3 (3 mantissa bits) where the consumer is forgiving -- the MLPs and
    DINOv2's QKV (2/3 of the Linear FLOPs); bf16 where a rounding lands on the residual stream or the heatmap un-damped: every proj,
    BETR's QKV (its v columns decide the block's output; q, k are RMS-normalised from the rounded values), the adapter and the head
    (per-Linear sensitivities: profiles/r3_strict_modes.md section 1, profiles/r4_fp8_mixed.md)."""
    if normed:      # BETR
        return [PROMOTE_QKV | PROMOTE_PROJ] * depth, PROMOTE_ADAPTER_FC1 | PROMOTE_ADAPTER_FC2 | PROMOTE_BBOX_PROJ
    return [PROMOTE_PROJ] * depth, 0
ACT_NONE, ACT_GELU = 0, 1
# per-Linear promotion: F16C8 family -> split-f16, e4m3 -> bf16 (include/boxdreamer_hip.h: BD_PROMOTE_*)
PROMOTE_QKV, PROMOTE_PROJ, PROMOTE_FC1, PROMOTE_FC2, PROMOTE_ATTN = 1, 2, 4, 8, 16
PROMOTE_ADAPTER_FC1, PROMOTE_ADAPTER_FC2, PROMOTE_BBOX_EMB, PROMOTE_BBOX_PROJ = 1, 2, 4, 8
PROMOTE_PATCH_EMBED = 1
# The precision a module runs when its config names none: the fastest mode that MEETS the path's parity bar (heatmap logits
# within 1e-3 of the fp32 CPU forward, identical top-20 sets).  "bf16" -- the reference's own `precision`, 4e-2 off its fp32
# forward -- is the explicit throughput opt-in (`hip_precision: bf16` in the decoder / encoder config, or $BOXDREAMER_HIP_PREC).
DEFAULT_PREC = "f16c8_qk16"

_ERR = {-1: "BD_ERR_SHAPE", -2: "BD_ERR_DTYPE", -3: "BD_ERR_ALIGN", -4: "BD_ERR_WORKSPACE", -5: "BD_ERR_NULL"}


class HipLibraryError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("a_plane", C.c_int64),
                ("W", C.c_void_p), ("ldw", C.c_int64), ("w_plane", C.c_int64),
                ("bias", C.c_void_p), ("wscale", C.c_void_p),
                ("resid", C.c_void_p), ("ldr", C.c_int64),
                ("addtab", C.c_void_p), ("tab_rows", C.c_int),
                ("out", C.c_void_p), ("ldo", C.c_int64), ("out_plane", C.c_int64),
                ("out_f32", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("act", C.c_int),
                ("rpg_in", C.c_int), ("rpg_out", C.c_int), ("row_off", C.c_int), ("w_qexp", C.c_int),
                ("rms_wq", C.c_void_p), ("rms_wk", C.c_void_p), ("rms_eps", C.c_float), ("rms_parts", C.c_int),
                ("ln_stats_out", C.c_void_p), ("ln_op_out", C.c_void_p), ("ln_op_plane", C.c_int64), ("ln_op_ld", C.c_int64),
                ("ln_stats_in", C.c_void_p), ("ln_colsum", C.c_void_p), ("ln_eps", C.c_float), ("ln_resid_in_op", C.c_int),
                ("sk_ws", C.c_void_p), ("sk_split", C.c_int)]


GEMM_FAMILY_PC, GEMM_FAMILY_GLDS, GEMM_FAMILY_PC_F16C8 = 1, 2, 3      # BD_GEMM_FAMILY_*
GEMM_KEY_LEN, GEMM_PLAN_MAX_LAUNCHES = 13, 3


class GemmLaunch(C.Structure):
    _fields_ = [("family", C.c_int), ("row", C.c_int), ("key", C.c_int * GEMM_KEY_LEN), ("grid", C.c_int), ("block", C.c_int),
                ("row0", C.c_int), ("rows", C.c_int), ("split_k", C.c_int)]


class GemmPlan(C.Structure):
    _fields_ = [("n_launches", C.c_int), ("launch", GemmLaunch * GEMM_PLAN_MAX_LAUNCHES)]


ATTN_ENTRY_PLAIN, ATTN_ENTRY_Q, ATTN_ENTRY_PREFIX, ATTN_ENTRY_VARLEN = 0, 1, 2, 3      # BD_ATTN_ENTRY_*
ATTN_FAMILY_TILED, ATTN_FAMILY_PP = 1, 2               # BD_ATTN_FAMILY_*
ATTN_KEY_LEN = 6


class AttnCall(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("entry", "batch", "seq", "heads", "head_dim", "has_q_view", "q_len", "n_prefix", "prefix_queries",
                                       "n_views", "max_views", "tokens_per_view", "prec", "latency_forms")]


class AttnLaunch(C.Structure):
    _fields_ = [("family", C.c_int), ("row", C.c_int), ("key", C.c_int * ATTN_KEY_LEN), ("grid", C.c_int), ("block", C.c_int),
                ("q_len", C.c_int), ("q_off", C.c_int), ("out_rows", C.c_int)]


class AttnPlan(C.Structure):
    _fields_ = [("n_launches", C.c_int), ("launch", AttnLaunch * 1)]


class Linear(C.Structure):
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("wscale", C.c_void_p), ("w_qexp", C.c_int)]


class BlockWeights(C.Structure):
    _fields_ = [("ln1_w", C.c_void_p), ("ln1_b", C.c_void_p), ("ln2_w", C.c_void_p), ("ln2_b", C.c_void_p),
                ("qkv", Linear), ("proj", Linear), ("fc1", Linear), ("fc2", Linear),
                ("q_norm_w", C.c_void_p), ("k_norm_w", C.c_void_p), ("qkv16", Linear), ("promote", C.c_int),
                ("qkv_f", Linear), ("fc1_f", Linear), ("qkv16_f", Linear),
                ("qkv_s", C.c_void_p), ("fc1_s", C.c_void_p), ("qkv16_s", C.c_void_p), ("ln_resid3", C.c_int)]


class DinoWeights(C.Structure):
    _fields_ = [("depth", C.c_int), ("dim", C.c_int), ("heads", C.c_int), ("n_prefix", C.c_int),
                ("grid", C.c_int), ("patch", C.c_int), ("kpad", C.c_int),
                ("ln_eps", C.c_float),
                ("patch_embed", Linear),
                ("pos_patch", C.c_void_p), ("prefix_tokens", C.c_void_p),
                ("norm_w", C.c_void_p), ("norm_b", C.c_void_p),
                ("blocks", C.POINTER(BlockWeights)), ("promote_misc", C.c_int), ("feats_prec", C.c_int), ("latency_mode", C.c_int)]


class BetrWeights(C.Structure):
    _fields_ = [("depth", C.c_int), ("dim", C.c_int), ("heads", C.c_int), ("grid", C.c_int),
                ("patch", C.c_int), ("box_dim", C.c_int), ("kpad", C.c_int),
                ("ln_eps", C.c_float), ("adapter_ln_eps", C.c_float), ("rms_eps", C.c_float),
                ("adapter_fc1", Linear), ("adapter_fc2", Linear), ("bbox_emb", Linear), ("bbox_proj", Linear),
                ("pos_table", C.c_void_p), ("query_token", C.c_void_p),
                ("blocks", C.POINTER(BlockWeights)), ("promote_misc", C.c_int), ("latency_mode", C.c_int)]


class TraceRecord(C.Structure):
    _fields_ = [("kind", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("ms", C.c_float)]


EXPORTS = [
    "bd_abi_version", "bd_target_arch", "bd_gemm", "bd_layernorm", "bd_qk_rmsnorm", "bd_attention",
    "bd_im2col_images", "bd_patchify_heatmaps", "bd_write_prefix_tokens", "bd_query_substitute",
    "bd_gather_query_tokens", "bd_unpatchify_sigmoid", "bd_decode_topk",
    "bd_encoder_workspace_bytes", "bd_encoder_forward", "bd_decoder_workspace_bytes", "bd_decoder_forward",
    "bd_trace_begin", "bd_trace_end", "bd_render_corner_heatmaps", "bd_attention_q", "bd_gather_query_rows_f32",
    "bd_dino_match_scores", "bd_topk_mask", "bd_solve_pnp", "bd_gemm_fuses_qk_rmsnorm", "bd_gemm_takes_ln_fold", "bd_gemm_splitk_flag_bytes",
    "bd_gemm_splitk_workspace_bytes", "bd_solve_pnp_host", "bd_attention_prefix",
    "bd_lanes_prepare", "bd_encoder_workspace_bytes_lanes", "bd_encoder_forward_lanes", "bd_decoder_workspace_bytes_lanes",
    "bd_decoder_forward_lanes", "bd_pose_metrics_workspace_bytes", "bd_pose_metrics", "bd_crop_resize_frames",
    "bd_attention_varlen", "bd_query_substitute_varlen", "bd_gather_query_rows_f32_varlen", "bd_gather_query_tokens_varlen",
    "bd_decoder_workspace_bytes_ragged", "bd_decoder_forward_ragged", "bd_gather_view_rows",
    "bd_match_view_sums", "bd_match_select_rows",
    "bd_assemble_entry_tokens", "bd_decoder_entry_tokens_workspace_bytes", "bd_decoder_entry_tokens",
    "bd_decoder_entry_workspace_bytes", "bd_decoder_forward_entry", "bd_decoder_entry_workspace_bytes_ragged",
    "bd_decoder_forward_entry_ragged", "bd_solve_pnp_wave",
    "bd_solve_pnp_ransac_workspace_bytes", "bd_solve_pnp_ransac_wave", "bd_solve_pnp_ransac_host",
    "bd_round_sources", "bd_pose_select_rows",
    "bd_stream_windows", "bd_stream_windows_host", "bd_stream_results", "bd_stream_results_host", "bd_stream_select_rows",
    "bd_stream_track_windows", "bd_stream_track_windows_host",
    "bd_gemm_plan", "bd_gemm_instance", "bd_attention_plan", "bd_attention_instance",
    "bd_crop_resize_frames_fmt", "bd_frames_to_rgb_host",
]
PIXEL_RGB, PIXEL_BGR, PIXEL_RGBA, PIXEL_BGRA, PIXEL_NV12 = 0, 1, 2, 3, 4      # BD_PIXEL_*: bd_crop_resize_frames_fmt's format
STREAM_ROW_FLOATS = 66                                 # BD_STREAM_ROW_FLOATS: one sample's row of bd_stream_results
STREAM_SELECT_DINO, STREAM_SELECT_TRACK = 0, 1         # BD_STREAM_SELECT_*: bd_stream_select_rows' rule
STREAM_BOX_DETECTOR, STREAM_BOX_TRACKED, STREAM_BOX_HELD = 0, 1, 2     # BD_STREAM_BOX_*: bd_stream_track_windows' box_src

_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raise loudly if it has not been built."""
    global _lib
    # every wrapper calls load() before it hands the first tensor to ptr(): forget a device noted by a call that raised
    # between ptr() and stream() (it would make the next call on another device fail with a false "mixes tensors" error)
    _call.dev = None
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} is missing: the gfx950 HIP kernels are not built. Run "
            "`python -m boxdreamer_amd.build` (or __graft_entry__.build()). There is no CPU/PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise HipLibraryError(f"{LIB_PATH} does not export {name}")
    i, i64, vp, f, sz = C.c_int, C.c_int64, C.c_void_p, C.c_float, C.c_size_t
    lib.bd_abi_version.restype = i
    lib.bd_target_arch.restype = C.c_char_p
    lib.bd_gemm.argtypes = [C.POINTER(GemmArgs), i, vp]
    lib.bd_gemm_fuses_qk_rmsnorm.argtypes = [C.POINTER(GemmArgs), i]
    lib.bd_gemm_takes_ln_fold.argtypes = [C.POINTER(GemmArgs), i]
    lib.bd_gemm_plan.argtypes = [C.POINTER(GemmArgs), i, i, i, C.POINTER(GemmPlan)]
    lib.bd_gemm_instance.argtypes = [i, i, C.POINTER(C.c_int)]
    lib.bd_attention_plan.argtypes = [C.POINTER(AttnCall), vp, vp, vp, C.POINTER(AttnPlan)]
    lib.bd_attention_instance.argtypes = [i, i, C.POINTER(C.c_int)]
    lib.bd_gemm_splitk_flag_bytes.argtypes = [i, i]
    lib.bd_gemm_splitk_flag_bytes.restype = sz
    lib.bd_gemm_splitk_workspace_bytes.argtypes = [i, i]
    lib.bd_gemm_splitk_workspace_bytes.restype = sz
    lib.bd_layernorm.argtypes = [vp, i64, vp, vp, f, vp, i64, vp, i64, i, i, i, i, i, i, vp]
    lib.bd_qk_rmsnorm.argtypes = [vp, i64, vp, vp, f, i, i, i, i, vp]
    lib.bd_attention.argtypes = [vp, i64, vp, i64, i, i, i, i, f, i, vp]
    lib.bd_im2col_images.argtypes = [vp, i, vp, i64, i, i, i, i, i, vp]
    lib.bd_patchify_heatmaps.argtypes = [vp, i, vp, i64, i, i, i, i, i, i, vp]
    lib.bd_write_prefix_tokens.argtypes = [vp, vp, i, i, i, i, vp]
    lib.bd_query_substitute.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp]
    lib.bd_gather_query_tokens.argtypes = [vp, vp, vp, i64, i, i, i, i, i, vp]
    lib.bd_unpatchify_sigmoid.argtypes = [vp, vp, vp, i, i, i, i, vp]
    lib.bd_decode_topk.argtypes = [vp, i, i, i, i, vp, vp, vp, vp]
    lib.bd_encoder_workspace_bytes.argtypes = [C.POINTER(DinoWeights), i, i]
    lib.bd_encoder_workspace_bytes.restype = sz
    lib.bd_encoder_forward.argtypes = [C.POINTER(DinoWeights), vp, i, i, i, vp, vp, i64, vp, sz, i, vp]
    lib.bd_decoder_workspace_bytes.argtypes = [C.POINTER(BetrWeights), i, i, i]
    lib.bd_decoder_workspace_bytes.restype = sz
    lib.bd_decoder_forward.argtypes = [C.POINTER(BetrWeights), vp, i, vp, i64, vp, i, i, i, vp, vp, vp, sz, i, vp]
    lib.bd_encoder_workspace_bytes_lanes.argtypes = [C.POINTER(DinoWeights), i, i, i]
    lib.bd_encoder_workspace_bytes_lanes.restype = sz
    lib.bd_encoder_forward_lanes.argtypes = [C.POINTER(DinoWeights), vp, i, i, i, vp, vp, i64, vp, sz, i, i, vp]
    lib.bd_decoder_workspace_bytes_lanes.argtypes = [C.POINTER(BetrWeights), i, i, i, i]
    lib.bd_decoder_workspace_bytes_lanes.restype = sz
    lib.bd_decoder_forward_lanes.argtypes = [C.POINTER(BetrWeights), vp, i, vp, i64, vp, i, i, i, vp, vp, vp, sz, i, i, vp]
    lib.bd_lanes_prepare.argtypes = []
    lib.bd_attention_q.argtypes = [vp, i64, vp, i64, i, i, i, i, f, vp, i, i, vp]
    lib.bd_attention_prefix.argtypes = [vp, i64, vp, i64, i, i, i, i, f, i, i, i, vp]
    lib.bd_gather_query_rows_f32.argtypes = [vp, vp, vp, i, i, i, i, vp]
    lib.bd_render_corner_heatmaps.argtypes = [vp, i, i, i, i, vp, i, vp]
    lib.bd_dino_match_scores.argtypes = [vp, vp, i, vp, i, i, i, i, i, i, f, vp, vp, vp, vp]
    lib.bd_topk_mask.argtypes = [vp, i, i, i, vp, vp]
    lib.bd_solve_pnp.argtypes = [vp, vp, vp, i, i, i, vp, vp]
    lib.bd_solve_pnp_host.argtypes = [vp, vp, vp, i, i, i, vp, i]
    lib.bd_solve_pnp_wave.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp]
    lib.bd_solve_pnp_ransac_workspace_bytes.argtypes = [i, i]
    lib.bd_solve_pnp_ransac_workspace_bytes.restype = sz
    lib.bd_solve_pnp_ransac_wave.argtypes = [vp, vp, vp, vp, i, i, i, f, f, i, i, vp, vp, vp, vp, vp, sz, vp]
    lib.bd_solve_pnp_ransac_host.argtypes = [vp, vp, vp, vp, i, i, i, f, f, i, i, vp, vp, vp, vp, i]
    lib.bd_pose_metrics_workspace_bytes.argtypes = [i, i]
    lib.bd_pose_metrics_workspace_bytes.restype = sz
    lib.bd_pose_metrics.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, sz, vp, vp]
    lib.bd_crop_resize_frames.argtypes = [vp, i, i, i, i64, i64, vp, vp, vp, i, i, vp, i, vp]
    lib.bd_crop_resize_frames_fmt.argtypes = [vp, i, i, i, i64, i64, vp, vp, vp, i, i, vp, i, i, i64, i, i, i, i, i, i, vp]
    lib.bd_frames_to_rgb_host.argtypes = [vp, i, i, i, i64, i64, i, i64, i, i, i, i, i, i, vp]
    lib.bd_attention_varlen.argtypes = [vp, i64, vp, i64, vp, i, i, i, i, i, i, f, vp, i, vp]
    lib.bd_query_substitute_varlen.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp]
    lib.bd_gather_query_rows_f32_varlen.argtypes = [vp, vp, vp, vp, i, i, i, vp]
    lib.bd_gather_query_tokens_varlen.argtypes = [vp, vp, vp, vp, i64, i, i, i, i, vp]
    lib.bd_decoder_workspace_bytes_ragged.argtypes = [C.POINTER(BetrWeights), i, i, i]
    lib.bd_decoder_workspace_bytes_ragged.restype = sz
    lib.bd_decoder_forward_ragged.argtypes = [C.POINTER(BetrWeights), vp, i, vp, i64, vp, vp, i, i, i, i, vp, vp, vp, sz, i, vp]
    lib.bd_gather_view_rows.argtypes = [vp, i64, i, vp, i64, i, vp, vp, i64, i, i, i, i, vp, vp, vp, vp]
    lib.bd_match_view_sums.argtypes = [vp, vp, i, i, i, i, i, i, f, vp, vp, vp]
    lib.bd_match_select_rows.argtypes = [vp, vp, i, vp, vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp]
    lib.bd_round_sources.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, vp, vp]
    lib.bd_pose_select_rows.argtypes = [vp, i, vp, vp, vp, i, i, i, i, vp, vp, vp, vp]
    lib.bd_assemble_entry_tokens.argtypes = [vp, i, vp, i, vp, vp, vp, vp, i, i, i, vp]
    lib.bd_decoder_entry_tokens_workspace_bytes.argtypes = [C.POINTER(BetrWeights), i, i]
    lib.bd_decoder_entry_tokens_workspace_bytes.restype = sz
    lib.bd_decoder_entry_tokens.argtypes = [C.POINTER(BetrWeights), vp, i, vp, i64, i, i, vp, vp, sz, i, vp]
    lib.bd_decoder_entry_workspace_bytes.argtypes = [C.POINTER(BetrWeights), i, i, i, i]
    lib.bd_decoder_entry_workspace_bytes.restype = sz
    lib.bd_decoder_forward_entry.argtypes = [C.POINTER(BetrWeights), vp, i, vp, vp, i64, vp, i, i, i, vp, vp, vp, sz, i, i, vp]
    lib.bd_decoder_entry_workspace_bytes_ragged.argtypes = [C.POINTER(BetrWeights), i, i, i]
    lib.bd_decoder_entry_workspace_bytes_ragged.restype = sz
    lib.bd_decoder_forward_entry_ragged.argtypes = [C.POINTER(BetrWeights), vp, i, vp, vp, i64, vp, vp, i, i, i, i, vp, vp, vp, sz, i, vp]
    lib.bd_stream_windows.argtypes = [vp, vp, C.c_double, i, vp, vp, i, vp]
    lib.bd_stream_windows_host.argtypes = [vp, vp, C.c_double, i, vp, vp, i]
    lib.bd_stream_results.argtypes = [vp, vp, vp, vp, vp, vp, i, vp, i, vp]
    lib.bd_stream_results_host.argtypes = [vp, vp, vp, vp, vp, vp, i, vp, i]
    lib.bd_stream_select_rows.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, f, vp, vp, vp, vp, vp, vp]
    d = C.c_double
    lib.bd_stream_track_windows.argtypes = [vp, vp, vp, vp, vp, vp, vp, d, i, i, i, f, d, d, vp, vp, vp, vp, vp, i, vp]
    lib.bd_stream_track_windows_host.argtypes = [vp, vp, vp, vp, vp, vp, vp, d, i, i, i, f, d, d, vp, vp, vp, vp, vp, i]
    lib.bd_trace_begin.argtypes = [i]
    lib.bd_trace_end.argtypes = [C.POINTER(TraceRecord), i]
    if lib.bd_abi_version() != 9:
        raise HipLibraryError("libboxdreamer_hip.so ABI version mismatch")
    _lib = lib
    return lib


# Device discipline, kept central so that no call site can forget it: `ptr()` notes the device of every tensor whose address
# is handed to the library, `stream()` returns torch's current stream ON THAT DEVICE and makes the device current for the
# launch (a module moved with .to("cuda:1") while cuda:0 is current would otherwise launch on a device-0 stream with
# device-1 pointers), and `check()` restores the previous current device.  Mixed devices in one call raise.
_call = threading.local()


def check(rc: int, what: str) -> None:
    prev = getattr(_call, "restore", None)
    _call.dev = None
    if prev is not None:
        _call.restore = None
        torch.cuda.set_device(prev)
    if rc == 0:
        return
    if rc < 0:
        raise HipLibraryError(f"{what} rejected its arguments: {_ERR.get(rc, rc)}")
    raise HipLibraryError(f"{what} failed with hipError_t {rc}")


def prec_id(prec) -> int:
    if isinstance(prec, int):
        return prec
    try:
        return PREC_NAMES[prec]
    except KeyError:
        raise ValueError(f"unknown precision {prec!r}; choose from {sorted(PREC_NAMES)}") from None


class Traits(NamedTuple):
    """What a precision id says about an operand tensor (include/boxdreamer_hip.h; boxdreamer_amd/operand.py turns it into bytes)."""
    cls: int                    # operand class: the value the unit operators and the weight packer take
    planes: int
    dtype: torch.dtype          # storage element type of every plane
    plane_bytes: tuple          # bytes per element of each plane
    k_multiple: int             # K padding granularity of GEMM operands: one 128-byte tile row per slab


_CLASSES = {PREC_BF16: (1, torch.bfloat16, (2,), 64), PREC_F16: (1, torch.float16, (2,), 64),
            PREC_FP8: (1, torch.float8_e4m3fn, (1,), 128),                                           # OCP e4m3 (gfx950), not MI300's fnuz
            PREC_BF16X3: (2, torch.bfloat16, (2, 2), 64), PREC_F16X3: (2, torch.float16, (2, 2), 64),   # (hi, lo) planes
            PREC_F16C8: (2, torch.float16, (2, 1), 64)}        # plane 1: one raw e4m3 byte per element at the head of 16-bit storage
_WHOLE_PATH = {PREC_BF16X3_ATTN_X3: PREC_BF16X3, PREC_F16X3_ATTN_X3: PREC_F16X3, PREC_F16C8_QK16: PREC_F16C8}
# one row per operand class and per whole-path id that runs in one; the attention-only codes (3, 5, 9, 10, 16, 17) name no operand
TRAITS = {pid: Traits(cls, *_CLASSES[cls]) for pid, cls in {**{c: c for c in _CLASSES}, **_WHOLE_PATH}.items()}


def traits(prec) -> Traits:
    try:
        return TRAITS[prec_id(prec)]
    except KeyError:
        raise ValueError(f"precision id {prec!r} names no operand class (an attention-only code, or unknown)") from None


def operand_prec(prec) -> int:
    """Operand class of a (possibly whole-path) precision id: the value the unit operators and the weight packer take."""
    return traits(prec).cls


def op_dtype(prec) -> torch.dtype:
    return traits(prec).dtype


def k_multiple(prec) -> int:
    return traits(prec).k_multiple


def planes(prec) -> int:
    return traits(prec).planes


AUTO_LANES_MIN_VIEWS = 24      # one batch runs as two sub-batch lanes from this many (sample, view) images on (profiles/r4_subbatch_lanes.md)
# ... earlier in the classes whose small launches were re-measured in round 5 (profiles/r5_small_experiments.md: lanes at batch 2 / 3):
# bf16 / f16 from batch 2 at T = 6 (-7.5 % / -4 % per step), the F16C8 class from batch 3 (-6 %; at batch 2 two lanes cost 9 %)
AUTO_LANES_MIN_VIEWS_BY_CLASS = {PREC_BF16: 12, PREC_F16: 12, PREC_F16C8: 18}


def resolve_lanes(setting, views: int, samples: int, prec=None) -> int:
    """Sub-batch lanes of one whole-path call (include/boxdreamer_hip.h, ABI v6+): `setting` is "auto" or 1..4; `views` = images of
    the call (B x T), `samples` = the units the batch can be cut at.  Bit-identical results for every value.  "auto": two lanes from
    AUTO_LANES_MIN_VIEWS images on (per class: AUTO_LANES_MIN_VIEWS_BY_CLASS), except in the e4m3 class, whose half-batch GEMMs lose more than the filled tail rounds win
    (measured: -2.7 % at batch 64, -4 % at batch 32; 16-bit classes +2 ... +9 %)."""
    if setting in (None, "auto"):
        cls = operand_prec(prec) if prec is not None else None
        n = 2 if views >= AUTO_LANES_MIN_VIEWS_BY_CLASS.get(cls, AUTO_LANES_MIN_VIEWS) and cls != PREC_FP8 else 1
    else:
        n = int(setting)
        if not 1 <= n <= 4:
            raise ValueError(f"hip_lanes must be 'auto' or 1..4, got {setting!r}")
    return max(1, min(n, samples))


def dtype_id(t: torch.Tensor) -> int:
    try:
        return {torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_F16, torch.float32: DTYPE_F32}[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported input dtype {t.dtype} (bf16 / fp16 / fp32)") from None


def ptr(t) -> C.c_void_p:
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise HipLibraryError("the HIP path needs device tensors (got a CPU tensor); there is no CPU fallback")
    dev = getattr(_call, "dev", None)
    if dev is None:
        _call.dev = t.device
    elif dev != t.device:
        _call.dev = None
        raise HipLibraryError(f"one call mixes tensors on {dev} and {t.device}")
    return C.c_void_p(t.data_ptr())


def stream() -> C.c_void_p:
    """torch's current HIP stream on the device of the tensors passed through ptr() for this call; that device is made
    current until check() runs."""
    dev = getattr(_call, "dev", None)
    _call.dev = None
    if dev is None:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cur = torch.cuda.current_device()
    if dev.index is not None and dev.index != cur:
        _call.restore = cur
        torch.cuda.set_device(dev)
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def same_device(*tensors) -> torch.device:
    """All given (non-None) tensors must live on one HIP device; returns it."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HipLibraryError("the HIP path needs device tensors (got a CPU tensor); there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise HipLibraryError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise HipLibraryError("no HIP device visible: BoxDreamer's MI355X path cannot run (no CPU fallback)")


# ---- Ragged batches (bd_attention_varlen / bd_decoder_forward_ragged): host-side bookkeeping.  The per-sample view counts are HOST
# integers; everything the kernels need on the device is derived from them without reading anything back.
def view_counts_list(view_counts, B=None):
    """`view_counts` (a list / tuple of ints or a CPU integer tensor) -> list of Python ints.  A device tensor raises TypeError: reading
    it would cost a device synchronisation per forward."""
    if isinstance(view_counts, torch.Tensor):
        if view_counts.is_cuda:
            raise TypeError("view_counts must be host integers (a list or a CPU int tensor): reading a device tensor would synchronise "
                            "the device on every forward")
        if view_counts.dtype.is_floating_point or view_counts.dtype == torch.bool or view_counts.dim() != 1:
            raise TypeError(f"view_counts must be a 1-D integer tensor, got {view_counts.dtype} {tuple(view_counts.shape)}")
        counts = [int(c) for c in view_counts.tolist()]
    else:
        counts = list(view_counts)
        if any(isinstance(c, bool) or int(c) != c for c in counts):
            raise TypeError("view_counts must be integers")
        counts = [int(c) for c in counts]
    if B is not None and len(counts) != B:
        raise ValueError(f"view_counts has {len(counts)} entries for a batch of {B} samples")
    return counts


def check_view_counts(counts, t_max: int, query_idx=None) -> None:
    """A sample needs a reference and a query: 2 <= count <= T_max; its query view must be one of its own views."""
    for b, c in enumerate(counts):
        if not 2 <= c <= t_max:
            raise ValueError(f"view_counts[{b}] = {c} is outside [2, {t_max}] (a sample needs a reference and a query, and fits the batch's view slots)")
    if query_idx is not None:
        for b, (q, c) in enumerate(zip(query_idx, counts)):
            if not 0 <= int(q) < c:
                raise ValueError(f"query_idx[{b}] = {int(q)} is not among the sample's {c} views (view_counts)")


def view_starts(counts):
    """[0, c0, c0 + c1, ...]: sample b owns the views [start[b], start[b + 1]) of the packed batch.  Every sample needs a view: the
    kernels that take a sample's query view from these offsets (csrc/layout.hip: query_view_of) have nothing to clamp an empty
    sample to, and would address the next sample's rows -- or rows past the buffer."""
    out = [0]
    for b, c in enumerate(counts):
        if int(c) <= 0:
            raise ValueError(f"view_counts[{b}] = {int(c)}: a sample of a ragged batch needs at least one view")
    for c in counts:
        out.append(out[-1] + int(c))
    return out


def packing_index(counts, t_max: int):
    """Flat indices into the (B * T_max) padded view slots of the valid views, sample by sample: packed = padded.flatten(0, 1)[index]."""
    return [b * t_max + t for b, c in enumerate(counts) for t in range(c)]


# ---- Reference bank (cache.RefFeatureBank, bd_gather_view_rows): the batch dict's `ref_rows` table, host side.  Like the view counts it is
# a HOST value; the kernel's `src` table and the list of slots to encode are derived from it without reading anything back.
def ref_rows_table(ref_rows, B: int, t_max: int):
    """`ref_rows` (a (B, T_max) CPU integer tensor or a nested list of ints; >= 0: bank row, -1: encode this slot) -> list of B lists of
    T_max Python ints.  A tensor that is not on the CPU raises TypeError (reading it would synchronise the device on every forward);
    another shape raises ValueError."""
    if isinstance(ref_rows, torch.Tensor):
        if ref_rows.device.type != "cpu":
            raise TypeError("ref_rows must be host integers (a nested list or a CPU int tensor): reading a device tensor would synchronise "
                            "the device on every forward")
        if ref_rows.dtype.is_floating_point or ref_rows.dtype == torch.bool:
            raise TypeError(f"ref_rows must be an integer tensor, got {ref_rows.dtype}")
        if tuple(ref_rows.shape) != (B, t_max):
            raise ValueError(f"ref_rows must be (B, T_max) = {(B, t_max)}, got {tuple(ref_rows.shape)}")
        return [[int(r) for r in row] for row in ref_rows.tolist()]
    rows = [list(r) for r in ref_rows]
    if len(rows) != B or any(len(r) != t_max for r in rows):
        raise ValueError(f"ref_rows must be (B, T_max) = {(B, t_max)}, got {len(rows)} rows of lengths {sorted({len(r) for r in rows})}")
    if any(isinstance(r, bool) or int(r) != r for row in rows for r in row):
        raise TypeError("ref_rows must be integers")
    return [[int(r) for r in row] for row in rows]


def check_ref_rows(rows, counts, bank_len: int) -> None:
    """Every VALID slot (t < counts[b]) holds a row of the bank or -1; padded slots are ignored whatever they hold."""
    for b, (row, c) in enumerate(zip(rows, counts)):
        for t in range(c):
            if not -1 <= row[t] < bank_len:
                raise ValueError(f"ref_rows[{b}][{t}] = {row[t]} is neither -1 (encode this slot) nor a row of the bank (it holds {bank_len})")


def gather_sources(rows, counts, t_max: int):
    """(src, encode) for one bd_gather_view_rows launch over the valid views, sample by sample (packing_index's order): src[v] is the
    bank row of packed view v, or -(k + 1) when the view is the k-th one to encode; encode[k] is that view's flat index into the
    (B * T_max) padded slots -- images.flatten(0, 1)[encode] is what the encoder runs on."""
    src, encode = [], []
    for b, c in enumerate(counts):
        for t in range(c):
            r = rows[b][t]
            if r >= 0:
                src.append(r)
            else:
                encode.append(b * t_max + t)
                src.append(-len(encode))
    return src, encode


# ---- Dense-reference mode over the bank (bd_match_select_rows): the same `ref_rows` table names a sample's whole database of banked
# references and its one query slot.  Host values again: the kernel's (rows, n_refs) tables are derived without reading anything back.
def dense_bank_tables(rows, counts, topk: int, query_idx=None):
    """(rows [B][N_max], n_refs [B], N_max, query [B]) of one bd_match_select_rows launch from a validated `ref_rows` table
    (check_ref_rows): sample b's reference slots are its valid slots except its query slot, in slot order, padded with -1 up to
    N_max = max(counts) - 1.  The banked dense mode encodes the query only: exactly one valid slot per sample is -1, that slot is the
    query (and equals the host `query_idx[b]` when one is given); a sample needs at least `topk` references and at most 1024.
    ValueError otherwise."""
    out, n_refs, query = [], [], []
    n_max = max(counts) - 1
    for b, (row, c) in enumerate(zip(rows, counts)):
        fresh = [t for t in range(c) if row[t] < 0]
        if len(fresh) != 1:
            raise ValueError(f"ref_rows[{b}] has {len(fresh)} entries -1 among its {c} views (slots {fresh}): the banked dense-reference mode "
                             "encodes the query only, exactly one slot is -1 and every other is a row of the bank")
        q = fresh[0]
        if query_idx is not None and int(query_idx[b]) != q:
            raise ValueError(f"ref_rows[{b}][{q}] = -1 but query_idx[{b}] = {int(query_idx[b])}: the slot to encode must be the query view")
        if c - 1 < topk:
            raise ValueError(f"sample {b} has {c - 1} references, fewer than dense_cfg.filter_topk = {topk}")
        if c - 1 > 1024:
            raise ValueError(f"sample {b} has {c - 1} references, more than the 1024 one bd_match_select_rows launch ranks")
        refs = [row[t] for t in range(c) if t != q]
        n_refs.append(len(refs))
        query.append(q)
        out.append(refs + [-1] * (n_max - len(refs)))
    return out, n_refs, n_max, query


def entry_bank_queries(rows, counts, query_idx=None):
    """The query slot per sample of a batch over a bank that keeps decoder-entry tokens (cache.RefFeatureBank with decoder=), from a
    validated `ref_rows` table (check_ref_rows).  Such a bank holds finished token rows, so the one view a forward encodes is the
    query: exactly one valid slot per sample is -1, and it equals the host `query_idx[b]` when one is given (dense_bank_tables'
    rule, which does the rest of the validation).  ValueError otherwise."""
    for b, (row, c) in enumerate(zip(rows, counts)):
        fresh = [t for t in range(c) if row[t] < 0]
        if not fresh:
            raise ValueError(f"ref_rows[{b}] names no slot to encode (-1) among its {c} views: the query view is encoded in every forward")
        stray = [t for t in fresh if query_idx is None or t != int(query_idx[b])]
        if len(fresh) > 1 and stray:
            raise ValueError(f"ref_rows[{b}][{stray[-1 if query_idx is None else 0]}] = -1 at a reference slot: an entry bank takes no freshly "
                             f"encoded references (slots {fresh} of sample {b} are -1; a bank built with decoder= holds the references' "
                             "finished token rows and a forward encodes the query only -- add() the reference with its heat maps first)")
    return dense_bank_tables(rows, counts, 1, query_idx)[3]


def attention_work_list(counts, heads: int, tokens_per_view: int, q_block: int, query_only: bool = False):
    """The (sample, head, q-block) work items of one bd_attention_varlen launch in grid order -- what the kernels derive from view_start
    (consecutive q-blocks of one (sample, head) are consecutive items, so the XCD remap keeps them on one L2).  Host mirror of the device
    decomposition, for tests and for sizing: len(...) is the launch's grid."""
    bpv = tokens_per_view // q_block
    return [(b, h, q) for b, c in enumerate(counts) for h in range(heads) for q in range(bpv if query_only else c * bpv)]
