"""ctypes binding of ``libsopro_hip.so`` (C ABI declared in ``include/sopro_hip.h``).

The library is the product: there is no torch / CPU fallback behind these wrappers.  If the
shared object is missing, or a wrapper is handed a tensor that is not a contiguous CUDA(HIP)
tensor, the call raises.  Every wrapper enqueues on torch's *current* stream so that torch's
caching allocator and the kernels agree on ordering (wrap a region in
``torch.cuda.stream(s)`` to move it, e.g. for hipGraph capture).
"""
from __future__ import annotations

import ctypes as C
import gc
import os
import struct
import threading
from typing import List, Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsopro_hip.so")
ABI_VERSION = 43
# Host-side A/B switches whose decision is on record (profiles/rNN_experiments.md) are read from the environment only in DEVELOPER
# mode (SOPRO_DEV=1) - round 6 housekeeping, the Python twin of the library's `make DEV=1`: a product process ignores them.
DEV_MODE = os.environ.get("SOPRO_DEV", "0") == "1"


def dev_env(name: str, default: str) -> str:
    return os.environ.get(name, default) if DEV_MODE else default


DEFAULT_GROUP_M = 8  # tile-walk group of the split-bf16 contractions (sopro_gemm_set_group_m); measured in tools/pipeline_sweep.sh
PRO_NONE, PRO_ELU, PRO_ADDVEC = 0, 1, 2
EPI_ROPE = 6  # rotate-half RoPE of the leading columns in the contraction's epilogue (sopro_gemm_split_ext.rope_*)
EPI_NONE, EPI_GELU, EPI_GLU, EPI_RES, EPI_TANH, EPI_GLU_DW = 0, 1, 2, 3, 4, 5
NORM_RMS, NORM_LN = 0, 1

_p = C.c_void_p
_i32, _i64, _f32 = C.c_int32, C.c_int64, C.c_float


class GemmArgs(C.Structure):
    _fields_ = [("A", _p), ("lda", _i64), ("a_seg_stride", _i64), ("W", _p), ("ldw", _i64), ("bias", _p),
                ("C", _p), ("ldc", _i64), ("c_seg_stride", _i64), ("R", _p), ("ldr", _i64), ("r_seg_stride", _i64),
                ("scale", _p), ("pro_vec", _p), ("dbg", _p), ("M", _i32), ("N", _i32), ("K", _i32), ("rows_per_seg", _i32),
                ("prologue", _i32), ("epilogue", _i32)]


class SplitExt(C.Structure):
    _fields_ = [("a_format", _i32), ("c_mode", _i32), ("C2", _p), ("ldc2", _i64), ("c2_seg_stride", _i64),
                ("rms_norm", _i32), ("rms_eps", _f32), ("ksplit", _i32), ("n_tickets", _i32), ("ws", _p), ("ws_bytes", _i64),
                ("tickets", _p), ("group_m", _i32), ("acc_scale", _f32), ("range_events", _p), ("rope_cos", _p), ("rope_sin", _p),
                ("rope_cols", _i32), ("rope_dh", _i32), ("rope_pos0", _i32), ("rope_rows_per_seg", _i32), ("ln_stats", _p), ("ln_stats_out", _p)]


class SkinnyArgs(C.Structure):
    _fields_ = [("X", _p), ("ldx", _i64), ("W", _p), ("ldw", _i64), ("bias", _p), ("Y", _p), ("ldy", _i64),
                ("R", _p), ("ldr", _i64), ("scale", _p), ("ring", _p), ("dw_w", _p), ("dw_b", _p), ("step", _p),
                ("Xp", _p), ("xp_stride", _i64), ("y_part_stride", _i64), ("dbg", _p), ("eps", _f32),
                ("B", _i32), ("N", _i32), ("K", _i32), ("epilogue", _i32),
                ("ring_len", _i32), ("ring_bcap", _i32), ("dil", _i32), ("ksize", _i32),
                ("np", _i32), ("ksplit", _i32), ("rms_norm", _i32), ("w_layout", _i32),
                ("aux_W", _p), ("aux_bias", _p), ("aux_R", _p), ("aux_Y", _p), ("aux_ldy", _i64), ("aux_ldr", _i64), ("aux_y_part_stride", _i64),
                ("aux_tiles", _i32), ("aux_flags", _i32), ("ring_format", _i32), ("mt", _i32), ("nt", _i32)]


class AttnArgs(C.Structure):
    _fields_ = [("Q", _p), ("ldq", _i64), ("q_bstride", _i64), ("K", _p), ("ldk", _i64), ("k_bstride", _i64),
                ("V", _p), ("ldv", _i64), ("v_bstride", _i64), ("O", _p), ("ldo", _i64), ("o_bstride", _i64),
                ("klens", _p), ("B", _i32), ("H", _i32), ("dh", _i32), ("Tq", _i32), ("Tk", _i32),
                ("causal", _i32), ("q_pos0", _i32), ("k_pos0", _i32), ("window", _i32), ("scale", _f32), ("kv_index", _p)]


class XattnArgs(C.Structure):
    _fields_ = [("X", _p), ("ldx", _i64), ("Xp", _p), ("xp_stride", _i64), ("norm_w", _p), ("Kp", _p), ("Vp", _p), ("klens", _p),
                ("Y", _p), ("y_part_stride", _i64), ("eps", _f32), ("gate", _f32), ("scale", _f32),
                ("np", _i32), ("B", _i32), ("H", _i32), ("D", _i32), ("S_cap", _i32),
                ("Qp", _p), ("qp_stride", _i64), ("nqp", _i32), ("k_unfolded", _i32), ("kv_format", _i32)]


class ArState(C.Structure):
    _fields_ = [("x_cur", _p), ("cond", _p), ("emb", _p), ("hist", _p), ("step", _p), ("row_step", _p),
                ("first_eos", _p), ("stop_t", _p), ("n_stopped", _p), ("recent", _p), ("params", _p), ("seed", C.c_uint64),
                ("B", _i32), ("D", _i32), ("Tar", _i32), ("max_steps", _i32), ("V", _i32), ("bos_row", _i32),
                ("start", _p), ("row_max", _p), ("row_params", _p), ("nonce", _p), ("row_id", _p), ("key", _p), ("dbg", _p)]


AR_MAX_LAYERS = 16


class ArBlock(C.Structure):
    """sopro_ar_block"""
    _fields_ = [("glu_w", _p), ("glu_b", _p), ("dw_w", _p), ("dw_b", _p), ("ff1_w", _p), ("ff1_b", _p), ("ff2_w", _p), ("ff2_b", _p),
                ("ring", _p), ("kp", _p), ("vp", _p), ("dil", _i32), ("xattn", _i32), ("gate", _f32), ("pad_", _i32),
                ("qa_w", _p), ("qu_w", _p), ("q_b", _p)]


class ArFrame(C.Structure):
    """sopro_ar_frame: the buffers of one autoregressive frame (the launch sequence itself is sopro_ar_issue_frame)."""
    _fields_ = [("blk", ArBlock * AR_MAX_LAYERS), ("head_w", _p), ("head_b", _p), ("x0", _p), ("xa", _p), ("xb", _p), ("part", _p),
                ("u", _p), ("xp", _p), ("qa", _p), ("qpart", _p), ("logits", _p), ("klens", _p),
                ("n_layers", _i32), ("B", _i32), ("D", _i32), ("S_cap", _i32), ("V1", _i32), ("H", _i32), ("ksize", _i32), ("w_layout", _i32),
                ("tile_glu", _i32), ("tile_ff1", _i32), ("tile_ff2", _i32), ("tile_head", _i32), ("eps", _f32), ("k_unfold", _i32), ("store_format", _i32),
                ("st", ArState)]


class EngineCfg(C.Structure):
    """sopro_engine_cfg (stage-level entry points)."""
    _fields_ = [("d_model", _i32), ("codebook_size", _i32), ("num_codebooks", _i32), ("nar_head_dim", _i32), ("bos_row", _i32),
                ("n_layers_ar", _i32), ("ar_kernel", _i32), ("ar_dilations", _i32 * 16), ("ar_xattn", _i32 * 16), ("ar_gate", _f32 * 16),
                ("n_layers_nar", _i32), ("nar_kernel", _i32), ("nar_dilations", _i32 * 16),
                ("n_stages", _i32), ("stage_first_cb", _i32 * 8), ("stage_n_cb", _i32 * 8), ("nar_mix", (_f32 * 2) * 8),
                ("nar_prev_cb_weights", _f32 * 64),
                ("mimi_hidden", _i32), ("mimi_codebook_dim", _i32), ("mimi_heads", _i32), ("mimi_head_dim", _i32), ("mimi_layers", _i32),
                ("mimi_window", _i32), ("mimi_inter", _i32), ("mimi_n_ratios", _i32), ("mimi_ratios", _i32 * 8), ("mimi_num_filters", _i32),
                ("mimi_kernel", _i32), ("mimi_res_kernel", _i32), ("mimi_last_kernel", _i32), ("mimi_compress", _i32),
                ("mimi_n_semantic", _i32), ("mimi_rope_positions", _i32), ("mimi_norm_eps", _f32), ("mimi_final_bias", _f32), ("precision", _i32),
                ("n_layers_text", _i32), ("ref_enc_layers", _i32), ("ref_xattn_layers", _i32), ("ref_xattn_heads", _i32), ("sv_student_dim", _i32),
                ("enc_kernel", _i32)]


class NarIO(C.Structure):
    """sopro_nar_io: the refinement's operands where the stages in front of it left them (round 5)."""
    _fields_ = [("cond", _p), ("cond_bstride", _i64), ("cb0", _p), ("cb0_bstride", _i64), ("lens", _p), ("tokens", _p), ("range_out", _p),
                ("safe", _i32)]


class MimiStreamState(C.Structure):
    """sopro_mimi_stream_state"""
    _fields_ = [("kv", _p), ("cap_rows", _i32), ("kv_len", _i32), ("pos", _i32), ("evict", _i32), ("half", _i32)]


class MimiStreamBatch(C.Structure):
    """sopro_mimi_stream_batch"""
    _fields_ = [("kv", _p), ("rows_cap", _i32), ("rows", _i32), ("cap_rows", _i32), ("kv_len", _i32), ("pos", _i32), ("evict", _i32),
                ("half", _i32)]


# every symbol declared in include/sopro_hip.h: name -> (restype, argtypes)
SYMBOLS = {
    "sopro_last_error": (C.c_char_p, []),
    "sopro_abi_version": (C.c_int, []),
    "sopro_build_flags": (C.c_int, []),
    "sopro_graph_launch_n": (C.c_int, [_p, _p, _i32]),
    "sopro_host_alloc": (C.c_int, [_i64, C.POINTER(_p)]),
    "sopro_host_free": (C.c_int, [_p]),
    "sopro_copy_to_host_async": (C.c_int, [_p, _p, _i64, _p]),
    "sopro_set_lds_floor": (C.c_int, [C.c_int]),
    "sopro_set_host_wait": (C.c_int, [C.c_int]),
    "sopro_device_info": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "sopro_capture_begin": (C.c_int, [_p]),
    "sopro_capture_end": (C.c_int, [_p, C.POINTER(_p)]),
    "sopro_graph_launch": (C.c_int, [_p, _p]),
    "sopro_graph_destroy": (C.c_int, [_p]),
    "sopro_stream_create_cu_range": (C.c_int, [C.c_int, C.c_int, C.POINTER(_p)]),
    "sopro_stream_create_cu_mask": (C.c_int, [_p, _i32, _p]),
    "sopro_stream_destroy": (C.c_int, [_p]),
    "sopro_gemm_f32": (C.c_int, [C.POINTER(GemmArgs), _p]),
    "sopro_gemm_bf16x3": (C.c_int, [_p, _p, _p, _p]),
    "sopro_gemm_bf16x6": (C.c_int, [_p, _p, _p, _p]),
    "sopro_gemm_bf16x1": (C.c_int, [_p, _p, _p, _p]),
    "sopro_pack_w_bf16": (C.c_int, [_p, _i64, _i32, _i32, _i32, _p, _p]),
    "sopro_fill2d_u32": (C.c_int, [_p, _i64, _i32, _i32, C.c_uint32, _p]),
    "sopro_copy2d_u32": (C.c_int, [_p, _i64, _p, _i64, _i32, _i32, _p]),
    "sopro_pack_w_f16x2": (C.c_int, [_p, _i64, _i32, _i32, _f32, _p, _p]),
    "sopro_f16x3_a_scale": (C.c_float, []),
    "sopro_gemm_f16x3": (C.c_int, [_p, _p, _p, _p]),
    "sopro_packed_w_bytes": (C.c_int64, [_i32, _i32, _i32]),
    "sopro_packed_w_rows_bytes": (C.c_int64, [_i32, _i32]),
    "sopro_pack_w_rows_bf16": (C.c_int, [_p, _i64, _i32, _i32, _p, _p]),
    "sopro_gemm_8p_takes": (C.c_int, [_p, _p]),
    "sopro_gemm_auto_ksplit": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "sopro_gemm_bf16x3_8p": (C.c_int, [_p, _p, _p, _p]),
    "sopro_gemm_bf16_set_tile_override": (C.c_int, [C.c_int]),
    "sopro_gemm_set_group_m": (C.c_int, [C.c_int]),
    "sopro_seanet_tail_set_tiles": (C.c_int, [C.c_int]),
    "sopro_seanet_res_set_tiles": (C.c_int, [C.c_int]),
    "sopro_seanet_res128_bf16": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p]),
    "sopro_seanet_up128_bf16": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _p]),
    "sopro_seanet_tail_bf16": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _f32, _p, _i64, _i32, _i32, _p]),
    "sopro_seanet_up_set_tiles": (C.c_int, [C.c_int]),
    "sopro_seanet_uptail_set_tiles": (C.c_int, [C.c_int]),
    "sopro_seanet_uptail_f32": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _f32, _p, _i64, _i32, _i32, _i32, _p]),
    "sopro_seanet_uptail_bf16": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _p, _p, _f32, _p, _i64, _i32, _i32, _p]),
    "sopro_seanet_up128_f32": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "sopro_seanet_res128_f32": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p]),
    "sopro_gemm_set_tile_override": (C.c_int, [C.c_int]),
    "sopro_pack_skinny_w": (C.c_int, [_p, _i64, _i32, _i32, _i32, _p, _p]),
    "sopro_pack_skinny_w_bf16": (C.c_int, [_p, _i64, _i32, _i32, _i32, _p, _p]),
    "sopro_skinny_packed_floats": (_i64, [_i32, _i32, _i32]),
    "sopro_skinny_f32": (C.c_int, [C.POINTER(SkinnyArgs), _p]),
    "sopro_row_stats_f32": (C.c_int, [_p, _i64, _i64, _i32, _i32, _i32, _p, _p]),
    "sopro_norm_f32": (C.c_int, [_p, _i64, _i64, _p, _i64, _p, _p, _p, _p, _i32, _i32, _i32, _f32, _i32, _p]),
    "sopro_rms_match_f32": (C.c_int, [_p, _p, _p, _i32, _i32, _p]),
    "sopro_tanh_affine_f32": (C.c_int, [_p, _p, _f32, _f32, _i64, _p]),
    "sopro_add_pos_f32": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "sopro_masked_mean_f32": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _p]),
    "sopro_stats_pool_f32": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "sopro_l2norm_f32": (C.c_int, [_p, _p, _i32, _i32, _f32, _p]),
    "sopro_dwconv_f32": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "sopro_codebook_sum_f32": (C.c_int, [_p, _i32, _p, _p, _p, _i32, _p, _i64, _p, _f32, _f32, _p, _i64, _i64, _i32, _i32, _i32, _p]),
    "sopro_text_embed_f32": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i32, _i32, _i32, _p]),
    "sopro_argmax_rows_f32": (C.c_int, [_p, _i64, _p, _i64, _i32, _i32, _i32, _p]),
    "sopro_argmax_partials_i32": (C.c_int, [_p, _i64, _p, _i64, _i32, _i32, _i32, _i32, _p]),
    "sopro_fir1_f32": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "sopro_rvq_assign_f32": (C.c_int, [_p, _i64, _i32, _p, _p, _i64, _i32, _p, _i64, _i32, _p]),
    "sopro_attention_f32": (C.c_int, [C.POINTER(AttnArgs), _p]),
    "sopro_attention_split_bf16": (C.c_int, [C.POINTER(AttnArgs), C.c_int32, _p]),
    "sopro_attn_decode_f32": (C.c_int, [C.POINTER(AttnArgs), _p]),
    "sopro_xattn_step_f32": (C.c_int, [C.POINTER(XattnArgs), _p]),
    "sopro_rope_f32": (C.c_int, [_p, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _p]),
    "sopro_upsample2_f32": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "sopro_final_conv_f32": (C.c_int, [_p, _i64, _p, _f32, _p, _i64, _i32, _i32, _p]),
    "sopro_seanet_tail_f32": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _f32, _p, _i64, _i32, _i32, _p]),
    "sopro_seanet_res128_p_f32": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "sopro_seanet_tail_p_f32": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _f32, _p, _i64, _i32, _i32, _i32, _p]),
    "sopro_engine_create": (C.c_int, [C.POINTER(EngineCfg), C.POINTER(_p)]),
    "sopro_engine_set_tensor": (C.c_int, [_p, C.c_char_p, _p, C.POINTER(_i64), _i32]),
    "sopro_engine_finalize": (C.c_int, [_p, _p]),
    "sopro_engine_destroy": (C.c_int, [_p]),
    "sopro_ar_workspace_bytes": (_i64, [_p, _i32, _i32, _i32]),
    "sopro_ar_begin": (C.c_int, [_p, _p, _i32, _p, _p, _p, _i32, _i32, C.POINTER(_f32), C.c_uint64, C.c_uint32, _p]),
    "sopro_ar_run_graph": (C.c_int, [_p, _i32, _p]),
    "sopro_ar_tokens": (C.c_int, [_p, _p, _p, _p, _p]),
    "sopro_nar_workspace_bytes": (_i64, [_p, _i32, _i32]),
    "sopro_nar_refine": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i32, _i32, _p, _p]),
    "sopro_nar_refine_io": (C.c_int, [_p, _p, C.POINTER(NarIO), _i32, _i32, _p]),
    "sopro_nar_seed_i32": (C.c_int, [_p, _i32, _p, _i64, _i32, _i32, _i32, _p]),
    "sopro_mimi_workspace_bytes": (_i64, [_p, _i32, _i32]),
    "sopro_mimi_decode": (C.c_int, [_p, _p, _p, _i32, _i32, _p, _p]),
    "sopro_mimi_chunk_rows": (_i32, [_i32, _i32]),
    "sopro_mimi_decode_parts": (C.c_int, [_p, _p, _p, _i32, _i32, _p, _i32, _p]),
    "sopro_mimi_stream_kv_bytes": (_i64, [_p, _i32]),
    "sopro_mimi_stream_init": (C.c_int, [_p, C.POINTER(MimiStreamState), _p, _i32]),
    "sopro_mimi_stream_trim": (C.c_int, [C.POINTER(MimiStreamState), _i32]),
    "sopro_mimi_decode_stream": (C.c_int, [_p, _p, C.POINTER(MimiStreamState), _p, _i32, _p, _p]),
    "sopro_mimi_stream_batch_kv_bytes": (_i64, [_p, _i32, _i32]),
    "sopro_mimi_stream_batch_init": (C.c_int, [_p, C.POINTER(MimiStreamBatch), _p, _i32, _i32]),
    "sopro_mimi_stream_batch_trim": (C.c_int, [C.POINTER(MimiStreamBatch), _i32]),
    "sopro_mimi_stream_batch_keep": (C.c_int, [_p, C.POINTER(MimiStreamBatch), C.POINTER(_i32), _i32, _p]),
    "sopro_mimi_decode_stream_batch": (C.c_int, [_p, _p, C.POINTER(MimiStreamBatch), _p, _i32, _p, _p]),
    "sopro_ar_init": (C.c_int, [C.POINTER(ArState), _p]),
    "sopro_ar_sample": (C.c_int, [C.POINTER(ArState), _p, _i64, _p]),
    "sopro_ar_admit": (C.c_int, [C.POINTER(ArState), _i32, _p]),
    "sopro_ar_issue_frame": (C.c_int, [C.POINTER(ArFrame), _p]),
    "sopro_ar_fold_text": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _f32, _p]),
    "sopro_ar_fold_text_uk": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _f32, _p]),
    "sopro_engine_upload_tensor": (C.c_int, [_p, C.c_char_p, _p, C.POINTER(_i64), _i32, _p]),
    "sopro_checkpoint_open": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(_p)]),
    "sopro_checkpoint_close": (C.c_int, [_p]),
    "sopro_checkpoint_count": (_i32, [_p]),
    "sopro_checkpoint_tensor": (C.c_int, [_p, _i32, C.POINTER(C.c_char_p), C.POINTER(_p), C.POINTER(_i64), C.POINTER(_i32)]),
    "sopro_checkpoint_engine_cfg": (C.c_int, [_p, _i32, C.POINTER(EngineCfg)]),
    "sopro_engine_from_checkpoint": (C.c_int, [_p, _i32, _p, C.POINTER(_p)]),
    "sopro_engine_set_ar_tiles": (C.c_int, [_p, _i32, _i32, _i32, _i32]),
    "sopro_cond_workspace_bytes": (_i64, [_p, _i32, _i32, _i32]),
    "sopro_cond_prepare": (C.c_int, [_p, _p, _p, _p, _i32, _p, _p, _p, _p, _i64, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p]),
    "sopro_film_coeffs": (C.c_int, [_p, _p, _f32, _i32, _p, _p, _p, _p]),
    "sopro_ref_workspace_bytes": (_i64, [_p, _i32]),
    "sopro_ref_prepare": (C.c_int, [_p, _p, _p, _i32, _p, _p, _p, _p]),
    "sopro_mimi_encode_workspace_bytes": (_i64, [_p, _i32, _i32]),
    "sopro_mimi_encode": (C.c_int, [_p, _p, _p, _i32, _i32, _p, _p]),
    "sopro_cvt_f32_bf16": (C.c_int, [_p, _p, _i64, _p]),
    "sopro_cvt_bf16_f32": (C.c_int, [_p, _p, _i64, _p]),
    "sopro_prof_enable": (C.c_int, [C.c_int]),
    "sopro_prof_collect": (C.c_int, [_p, _i32, _p]),
    "sopro_join_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "sopro_join_edges_f32": (C.c_int, [_p, _i64, _p, _i32, _i64, _i32, _f32, _i32, _i32, _p, _p, _p]),
    "sopro_join_layout_i64": (C.c_int, [_p, _p, _i32, _p, _p]),
    "sopro_join_mix_f32": (C.c_int, [_p, _i64, _p, _p, _p, _i32, _i32, _p, _i64, _p]),
    "sopro_tsm_out_len": (_i64, [_i64, _i64]),
    "sopro_tsm_blocks": (_i64, [_i64]),
    "sopro_tsm_chunk_out_cap": (_i64, [_i64]),
    "sopro_tsm_state_bytes": (_i64, [_i32]),
    "sopro_tsm_rows_f32": (C.c_int, [_p, _i64, _p, _i64, _p, _i32, _p, _i32, _p, _p, _i64, _i64, _p, _p, _i32, _p]),
    "sopro_pitch_out_len": (_i64, [_i64, _i64]),
    "sopro_pitch_chunk_out_cap": (_i64, [_i64]),
    "sopro_pitch_state_bytes": (_i64, [_i32]),
    "sopro_pitch_rows_f32": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _p, _i32, _i32, _p, _i32, _p, _i64, _i64, _p, _p]),
    "sopro_wm_state_bytes": (_i64, [_i32]),
    "sopro_wm_chunk_out_cap": (_i64, [_i64]),
    "sopro_wm_fold_ws_bytes": (_i64, [_i32, _i64]),
    "sopro_wm_embed_rows_f32": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i32, _p, _i32, _p, _i32, _p, _p, _i64, _i64, _p, _p]),
    "sopro_wm_fold_rows_f32": (C.c_int, [_p, _i64, _p, _i64, _i32, _p, _p, _p, _p]),
    "sopro_wm_corr_rows_f32": (C.c_int, [_p, _p, _i32, _p, _i32, _p, _p]),
    "sopro_wm_peak_rows_f32": (C.c_int, [_p, _i32, _p, _p]),
    "sopro_sil_state_bytes": (_i64, [_i32]),
    "sopro_sil_chunk_out_cap": (_i64, [_i64]),
    "sopro_sil_ws_bytes": (_i64, [_i32, _i64]),
    "sopro_sil_rows_f32": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _p, _i32, _p, _i32, _p, _p, _p, _i64, _i64, _p, _p, _i32, _p, _p]),
    "sopro_align_ws_bytes": (_i64, [_i32, _i32, _i32]),
    "sopro_align_scores_f32": (C.c_int, [_p, _i64, _i64, _p, _i64, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _f32, C.c_uint32, _f32, _i32, _p, _i64,
                                         _i64, _p]),
    "sopro_align_dp_f32": (C.c_int, [_p, _i64, _i64, _p, _p, _i32, _i32, _i32, _p, _i64, _p, _i64, _p, _p, _p, _p]),
    "sopro_align_online_f32": (C.c_int, [_p, _i64, _i64, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _i64, _p]),
    "sopro_denoise_workspace_bytes": (_i64, [_i32, _i64]),
    "sopro_denoise_rows_f32": (C.c_int, [_p, _i64, _p, _p, _i32, _p, _i64, _p, _p, _i64, _p]),
    "sopro_formant_workspace_bytes": (_i64, [_i32, _i64]),
    "sopro_formant_state_bytes": (_i64, [_i32]),
    "sopro_formant_chunk_out_cap": (_i64, [_i64]),
    "sopro_formant_rows_f32": (C.c_int, [_p, _i64, _p, _p, _i32, _p, _p, _i32, _i32, _p, _i64, _i64, _p, _p, _i64, _p]),
    "sopro_crop_workspace_bytes": (_i64, [_i32, _i64]),
    "sopro_crop_rows_f32": (C.c_int, [_p, _i64, _p, _p, _i32, _i32, _p, _i64, _p, _p, _p, _p, _i64, _p]),
    "sopro_f0_workspace_bytes": (_i64, [_i32, _i64]),
    "sopro_f0_rows_f32": (C.c_int, [_p, _i64, _p, _p, _i32, _p, _p, _i64, _p, _p, _p, _p, _p, _i64, _p]),
    "sopro_f0_paths": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _p, _p, _i64, _p, _p, _i64, _p]),
    "sopro_spk_tile_frames": (_i32, []),
    "sopro_spk_workspace_bytes": (_i64, [_p, _i32, _i32]),
    "sopro_spk_embed_rows": (C.c_int, [_p, _p, _p, _i64, _p, _i32, _i32, _p, _i64, _p, _p, _p]),
    "sopro_spk_cosine": (C.c_int, [_p, _i64, _i32, _p, _i64, _i32, _i32, _i32, _p, _p]),
}

_lib: Optional[C.CDLL] = None


class SoproHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the shared object (once) and type every entry point.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SOPRO_HIP_LIB") or LIB_PATH  # developer override (ablation builds of tools/micro); same ABI checks
    if not os.path.exists(path):
        raise SoproHipError(
            f"{path} not found: the HIP kernel library is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C sopro_amd/csrc`). There is no CPU / torch fallback for the Sopro hot path.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    v = lib.sopro_abi_version()
    if v != ABI_VERSION:
        raise SoproHipError(f"{LIB_PATH} has ABI version {v}, the Python host expects {ABI_VERSION}: rebuild it")
    lib.sopro_gemm_set_group_m(int(dev_env("SOPRO_GEMM_GROUP_M", str(DEFAULT_GROUP_M))))
    if dev_env("SOPRO_GEMM_TILE", ""):  # developer A/B: tile shape of every split contraction (1: 128x128, 2: 256x128, 4: 128x64, 5: 64x64)
        lib.sopro_gemm_bf16_set_tile_override(int(dev_env("SOPRO_GEMM_TILE", "0")))
    _lib = lib
    return lib


class ProfRow(C.Structure):  # sopro_prof_row
    _fields_ = [("family", C.c_char * 40), ("launches", C.c_int64), ("gpu_bound", C.c_int64), ("flops", C.c_double),
                ("flops_bound", C.c_double), ("ms_all", C.c_double), ("ms_bound", C.c_double)]


class Profiler:
    """HIP-event timing of the heavy launches, recorded on the stream each launch is enqueued on
    (bench.py's roofline leg).  Families: the GEMM kernels, the attention kernel, AR graph replays.
    A sample whose stream was IDLE when its first event was recorded is host-bound (the span then contains the host's
    time between the record and the launch, not only the kernel): such samples are kept apart, and the family's time is
    extrapolated from the GPU-bound ones."""

    def __init__(self):
        self.rec = []  # (family, flops, ev0, ev1, gpu_bound)

    def begin(self):
        s = torch.cuda.current_stream()
        e = torch.cuda.Event(enable_timing=True)
        e.record(s)
        return (e, not s.query())  # work still queued in front of the launch: the span is GPU time

    def end(self, family: str, flops: float, e0) -> None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(torch.cuda.current_stream())
        self.rec.append((family, flops, e0[0], e1, e0[1]))

    def summary(self) -> dict:
        torch.cuda.synchronize()
        out: dict = {}
        new = lambda: {"ms": 0.0, "launches": 0, "flops": 0.0, "ms_all": 0.0, "gpu_bound": 0, "ms_bound": 0.0, "flops_bound": 0.0}  # noqa: E731
        # the launches of the stage sequences (NAR refinement, Mimi decoding, text folding) are timed inside the library
        rows = (ProfRow * 32)()
        n = C.c_int32(0)
        _check(load().sopro_prof_collect(rows, 32, C.byref(n)), "sopro_prof_collect")
        for r in rows[: n.value]:
            d = out.setdefault(r.family.decode(), new())
            d["launches"] += r.launches
            d["flops"] += r.flops
            d["ms_all"] += r.ms_all
            d["gpu_bound"] += r.gpu_bound
            d["ms_bound"] += r.ms_bound
            d["flops_bound"] += r.flops_bound
        for fam, fl, e0, e1, bound in self.rec:
            d = out.setdefault(fam, new())
            t = e0.elapsed_time(e1)
            d["ms_all"] += t
            d["launches"] += 1
            d["flops"] += fl
            if bound:
                d["gpu_bound"] += 1
                d["ms_bound"] += t
                d["flops_bound"] += fl
        for d in out.values():
            # time of the family: GPU-bound samples scaled to all launches (by flops where the family has them)
            if d["gpu_bound"] * 10 >= d["launches"] and d["ms_bound"] > 0:
                scale = (d["flops"] / d["flops_bound"]) if d["flops_bound"] > 0 else d["launches"] / d["gpu_bound"]
                d["ms"] = d["ms_bound"] * scale
            else:
                d["ms"] = d["ms_all"]
        return out


_prof: Optional[Profiler] = None
phase_log = None  # bench.py: list receiving (frames, rows, ev0, ev1) per AR phase while set


def set_profiler(p: Optional[Profiler]) -> None:
    global _prof
    _prof = p
    load().sopro_prof_enable(1 if p is not None else 0)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise SoproHipError(f"{what} failed ({rc}): {load().sopro_last_error().decode()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream  # ~1 us; the engines enqueue a few hundred launches per call


def ptr(t: Optional[torch.Tensor], dtype: torch.dtype = torch.float32) -> Optional[int]:
    """Device address of a tensor after checking that it is what the ABI expects."""
    if t is None:
        return None
    if not t.is_cuda:
        raise SoproHipError("tensor is not on a HIP device: the Sopro hot path has no CPU fallback")
    if t.dtype != dtype:
        raise SoproHipError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


# ------------------------------------------------------------------------------------------
# op wrappers (thin: argument marshalling only)
# ------------------------------------------------------------------------------------------
def gemm(A: torch.Tensor, W, Cout: torch.Tensor, *, M: int, N: int, K: int, lda: Optional[int] = None,
         ldc: Optional[int] = None, bias: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE,
         prologue: int = PRO_NONE, R: Optional[torch.Tensor] = None, ldr: Optional[int] = None,
         scale: Optional[torch.Tensor] = None, pro_vec: Optional[torch.Tensor] = None, rows_per_seg: Optional[int] = None,
         a_seg_stride: int = 0, c_seg_stride: int = 0, r_seg_stride: int = 0, a_off: int = 0, c_off: int = 0,
         r_off: int = 0, ldw: Optional[int] = None, dbg: Optional[torch.Tensor] = None, a_split: bool = False, c_mode: int = 0,
         C2: Optional[torch.Tensor] = None, ldc2: Optional[int] = None, c2_seg_stride: int = 0,
         c2_off: int = 0, rms_eps: float = 0.0, range_events: Optional[torch.Tensor] = None, rope: Optional[tuple] = None,
         ln_stats: Optional[torch.Tensor] = None, ln_eps: float = 0.0, ln_stats_out: Optional[torch.Tensor] = None,
         long_k: Optional[bool] = None, ksplit: Optional[int] = None, group_m: Optional[int] = None) -> None:
    """C = epi(pro(A) @ W^T + bias); offsets are in elements from the tensors' first element.  With a ``PackedW`` weight the
    contraction runs on the split-bf16 path, where ``a_split`` says A is in split form and ``c_mode`` 1 / 2 writes
    ELU(C) in split form (to C, or to C2 next to the fp32 C): see sopro_gemm_split_ext in include/sopro_hip.h.
    ``ksplit`` (packed weights): an explicit K-slice count instead of ``_auto_ksplit``'s, on the same per-stream scratch
    (``_splitk_buffers``); ``group_m``: sopro_gemm_split_ext.group_m (None = the library's default tile walk)."""
    n_out = N // 2 if epilogue == EPI_GLU else N
    g = GemmArgs()
    a16 = A.dtype == torch.bfloat16  # bf16 rows (a_format 2 of sopro_gemm_bf16x1): offsets / strides count bf16 elements
    c16 = c_mode in (6, 7, 8)        # bf16 rows out: Cout / C2 / R are bf16 tensors
    cdt = torch.bfloat16 if c16 else torch.float32
    g.A = ptr(A, A.dtype if a16 else torch.float32) + (2 if a16 else 4) * a_off
    g.lda = K if lda is None else lda
    g.a_seg_stride = a_seg_stride
    packed = isinstance(W, PackedW)
    if packed and (W.N != N or W.K != K):
        raise SoproHipError(f"packed weight is [{W.N}, {W.K}], the call wants [{N}, {K}]")
    g.W = None if packed else ptr(W)
    g.ldw = K if ldw is None else ldw
    g.bias = ptr(bias)
    g.C = (ptr(Cout, cdt) + (2 if c16 else 4) * c_off) if Cout is not None else None  # None only with c_mode 5 (arg-max partials to C2)
    g.ldc = n_out if ldc is None else ldc
    g.c_seg_stride = c_seg_stride
    g.R = (ptr(R, cdt) + (2 if c16 else 4) * r_off) if R is not None else None
    g.ldr = (n_out if ldr is None else ldr)
    g.r_seg_stride = r_seg_stride
    g.scale = ptr(scale)
    g.pro_vec = ptr(pro_vec)
    g.dbg = ptr(dbg, torch.int64)
    g.M, g.N, g.K = M, N, K
    g.rows_per_seg = M if rows_per_seg is None else rows_per_seg
    g.prologue, g.epilogue = prologue, epilogue
    e0 = _prof.begin() if _prof is not None else None
    x = None
    if packed:
        x = SplitExt()
        if rope is not None:  # (cos table, sin table, columns, head dim, first position, rows per utterance): EPI_ROPE
            x.rope_cos, x.rope_sin = ptr(rope[0]), ptr(rope[1])
            x.rope_cols, x.rope_dh, x.rope_pos0, x.rope_rows_per_seg = int(rope[2]), int(rope[3]), int(rope[4]), int(rope[5])
        if ln_stats is not None:  # fused LayerNorm of the A rows from the producer's statistics (W / bias carry the norm's weight / bias)
            x.ln_stats, x.rms_eps = ptr(ln_stats), float(ln_eps)
        x.ln_stats_out = ptr(ln_stats_out)  # EPI_RES: statistics of the updated stream (sopro_gemm_split_ext.ln_stats_out)
        if rms_eps > 0.0:  # fused RMSNorm of the A rows (W must carry the norm's weight vector)
            if W.pieces == 2 and not W.f16:
                raise SoproHipError("fused RMSNorm is a six-pass (pieces = 3), f16 three-pass or one-pass (pieces = 1) feature")
            x.rms_norm, x.rms_eps = 1, float(rms_eps)
        if group_m is not None:
            x.group_m = int(group_m)
        if ksplit is not None:
            ks = int(ksplit)
            # an early refusal only: what even the smallest tile (64 x 64) would need.  The library's own check, against the
            # tile it really launches, is what keeps a launch inside the workspace and the tickets.
            t64 = -(-M // 64) * -(-N // 64)
            if ks > 1 and (ks * t64 * 64 * 64 * 4 > _SPLITK_WS_BYTES or t64 > _SPLITK_TICKETS):
                raise SoproHipError(f"ksplit={ks}: {M} x {N} does not fit the split-K workspace / tickets of a stream")
        else:
            ks = _auto_ksplit(M, N, K, W.pieces, epilogue, W.f16) if (dbg is None and _splitk_enabled and rms_eps <= 0.0) else 1
        if ks > 1 or ksplit is not None:
            ws, tk = _splitk_buffers()
            x.ksplit, x.n_tickets, x.ws, x.ws_bytes, x.tickets = ks, int(tk.numel()), ptr(ws), int(ws.numel()) * 4, ptr(tk, torch.int32)
    if (a16 or c16) and not (packed and W.pieces == 1 and not W.f16):
        raise SoproHipError("bf16 rows (a_format 2, c_mode 6 / 7 / 8) belong to the one-pass (pieces = 1) path")
    if packed and W.f16:  # two fp16 pieces, three passes: the forms of the six-pass path
        if a_split or c_mode not in (0, 5):
            raise SoproHipError("split-form operands belong to the bf16 three-pass (pieces = 2) path")
        if c_mode == 5:
            x.c_mode, x.C2, x.ldc2 = 5, ptr(C2) + 4 * c2_off, (-(-N // 64) if ldc2 is None else ldc2)
        x.acc_scale = W.acc_scale
        x.range_events = ptr(range_events, torch.int32)  # optional device word (sopro_gemm_split_ext.range_events)
        _check(load().sopro_gemm_f16x3(C.byref(g), ptr(W.data, torch.int32), C.byref(x), _stream()), "sopro_gemm_f16x3")
    elif packed and W.pieces == 1:
        if a_split or c_mode in (1, 2):
            raise SoproHipError("split-form operands belong to the three-pass (pieces = 2) path")
        x.c_mode = c_mode
        x.a_format = 2 if a16 else 0
        x.C2 = (ptr(C2, cdt) + (2 if c16 else 4) * c2_off) if C2 is not None else None
        x.ldc2, x.c2_seg_stride = (n_out if ldc2 is None else ldc2), c2_seg_stride
        _check(load().sopro_gemm_bf16x1(C.byref(g), ptr(W.data, torch.int32), C.byref(x), _stream()), "sopro_gemm_bf16x1")
    elif packed and W.pieces == 3:
        if a_split or c_mode not in (0, 5):
            raise SoproHipError("split-form operands belong to the three-pass (pieces = 2) path")
        if c_mode == 5:
            x.c_mode, x.C2, x.ldc2 = 5, ptr(C2) + 4 * c2_off, (-(-N // 64) if ldc2 is None else ldc2)
        _check(load().sopro_gemm_bf16x6(C.byref(g), ptr(W.data, torch.int32), C.byref(x), _stream()), "sopro_gemm_bf16x6")
    elif packed:
        if a16 or c16:
            raise SoproHipError("bf16 rows (a_format 2, c_mode 6 / 7 / 8) belong to the one-pass (pieces = 1) path")
        x.a_format, x.c_mode = int(bool(a_split)), c_mode
        x.C2 = (ptr(C2) + 4 * c2_off) if C2 is not None else None
        x.ldc2, x.c2_seg_stride = (n_out if ldc2 is None else ldc2), c2_seg_stride
        use_8p = long_k if long_k is not None else (W.rows is not None and bool(load().sopro_gemm_8p_takes(C.byref(g), C.byref(x))))
        if use_8p:  # the long-K form: 256 x 256 tiles, both operands split in memory (csrc/gemm_8p.hip); same results bit for bit
            if W.rows is None:
                raise SoproHipError("the long-K form needs the weight's split-form rows (pack_w_bf16x3(W, rows=True))")
            x.ksplit = 0
            _check(load().sopro_gemm_bf16x3_8p(C.byref(g), W.rows.data_ptr(), C.byref(x), _stream()), "sopro_gemm_bf16x3_8p")
        else:
            _check(load().sopro_gemm_bf16x3(C.byref(g), ptr(W.data, torch.int32), C.byref(x), _stream()), "sopro_gemm_bf16x3")
    elif a_split or c_mode:
        raise SoproHipError("split-plane operands need a PackedW weight (the fp32 kernel reads and writes fp32 rows)")
    elif ksplit is not None or group_m is not None:
        raise SoproHipError("ksplit / group_m belong to the packed-weight paths (sopro_gemm_split_ext)")
    else:
        _check(load().sopro_gemm_f32(C.byref(g), _stream()), "sopro_gemm_f32")
    if e0 is not None:
        fam = "gemm_f32_kernel" if not packed else ("gemm_f16x3_kernel" if W.f16 else {1: "gemm_bf16x1_kernel", 2: "gemm_bf16x3_kernel", 3: "gemm_bf16x6_kernel"}[W.pieces])
        _prof.end(fam, 2.0 * M * N * K, e0)


_splitk_enabled = True  # (SOPRO_NO_SPLITK=1 is read by the library's rule; tests toggle this)
_splitk_pool: dict = {}  # stream handle -> (workspace, tickets): split-K scratch belongs to one stream at a time
_SPLITK_WS_BYTES = 32 << 20
_SPLITK_TICKETS = 1024


def _auto_ksplit(M: int, N: int, K: int, pieces: int, epilogue: int, f16: bool = False) -> int:
    """K slices for a problem with too few output tiles to occupy the chip (streaming chunks, batch 1): the library's rule
    (sopro_gemm_auto_ksplit, which the stage sequences ask too) for this host's per-stream scratch."""
    return load().sopro_gemm_auto_ksplit(M, N, K, pieces, int(f16), epilogue, _SPLITK_WS_BYTES, _SPLITK_TICKETS)


def _splitk_buffers():
    key = _stream()
    bufs = _splitk_pool.get(key)
    if bufs is None:
        dev = torch.cuda.current_device()
        bufs = (torch.empty(_SPLITK_WS_BYTES // 4, dtype=torch.float32, device=f"cuda:{dev}"),
                torch.zeros(_SPLITK_TICKETS, dtype=torch.int32, device=f"cuda:{dev}"))
        _splitk_pool[key] = bufs
    return bufs


class PackedW:
    """A weight matrix [N, K] as 1, 2 or 3 bf16 pieces in MFMA fragment order (sopro_pack_w_bf16)."""

    __slots__ = ("data", "N", "K", "pieces", "f16", "acc_scale", "rows")

    def __init__(self, data: torch.Tensor, N: int, K: int, pieces: int, f16: bool = False, acc_scale: float = 1.0):
        self.data, self.N, self.K, self.pieces, self.f16, self.acc_scale = data, N, K, pieces, f16, acc_scale
        self.rows = None  # pieces == 2: the same matrix as split-form ROWS for the long-K form (pack_w_rows_bf16 / sopro_gemm_bf16x3_8p)


def pack_w_bf16(W: torch.Tensor, pieces: int) -> PackedW:
    """[N, K] fp32 device matrix -> the operand of ``gemm`` on the split-bf16 matrix-core paths
    (pieces = 2: three passes, 16 mantissa bits; pieces = 3: six passes, 24 mantissa bits)."""
    if W.dim() != 2 or not W.is_contiguous():
        raise SoproHipError("pack_w_bf16 wants a contiguous [N, K] matrix")
    N, K = int(W.shape[0]), int(W.shape[1])
    lib = load()
    data = torch.empty(int(lib.sopro_packed_w_bytes(N, K, pieces)) // 4, dtype=torch.int32, device=W.device)
    _check(lib.sopro_pack_w_bf16(ptr(W), K, N, K, pieces, ptr(data, torch.int32), _stream()), "sopro_pack_w_bf16")
    return PackedW(data, N, K, pieces)


def pack_w_bf16x3(W: torch.Tensor, rows: bool = False) -> PackedW:
    """``rows``: also keep the matrix as split-form rows [N][K / 32][32 hi | 32 lo] (sopro_pack_w_rows_bf16) - the weight operand of the
    long-K form (csrc/gemm_8p.hip), which ``gemm`` picks when the library says the call is one it takes (or ``long_k=True``)."""
    pw = pack_w_bf16(W, 2)
    if rows:
        N, K = pw.N, pw.K
        lib = load()
        nb = int(lib.sopro_packed_w_rows_bytes(N, K))
        if nb <= 0:
            raise SoproHipError("split-form weight rows need K % 32 == 0")
        buf = torch.empty(nb // 4 + 32, dtype=torch.int32, device=W.device)
        off = (-buf.data_ptr() % 128) // 4  # 128-byte aligned rows
        pw.rows = buf[off: off + nb // 4]
        _check(lib.sopro_pack_w_rows_bf16(ptr(W), K, N, K, pw.rows.data_ptr(), _stream()), "sopro_pack_w_rows_bf16")
    return pw


def pack_w_f16x3(W: torch.Tensor) -> PackedW:
    """Two fp16 pieces (22 mantissa bits), three MFMA passes: the token paths' accuracy class at half the passes of bf16x6.
    The matrix is scaled by a power of two into fp16's range (max |w| lands in [2^13, 2^14)); gemm undoes it exactly."""
    if W.dim() != 2 or not W.is_contiguous():
        raise SoproHipError("pack_w_f16x3 wants a contiguous [N, K] matrix")
    import math

    N, K = int(W.shape[0]), int(W.shape[1])
    lib = load()
    amax = float(W.abs().max())
    wscale = 2.0 ** (13 - math.frexp(amax)[1] + 1) if amax > 0.0 else 1.0  # amax * wscale in [2^13, 2^14)
    data = torch.empty(int(lib.sopro_packed_w_bytes(N, K, 2)) // 4, dtype=torch.int32, device=W.device)
    _check(lib.sopro_pack_w_f16x2(ptr(W), K, N, K, wscale, ptr(data, torch.int32), _stream()), "sopro_pack_w_f16x2")
    return PackedW(data, N, K, 2, f16=True, acc_scale=1.0 / (float(lib.sopro_f16x3_a_scale()) * wscale))


def pack_w_bf16x6(W: torch.Tensor) -> PackedW:
    return pack_w_bf16(W, 3)


def pack_w_bf16x1(W: torch.Tensor) -> PackedW:
    """bf16 mode: the weight rounded to bf16 once (one MFMA pass per product)."""
    return pack_w_bf16(W, 1)


class SkinnyW:
    """AR-step weights in the fragment order of ``sopro_pack_skinny_w`` (every load instruction reads 1 KiB of consecutive memory)."""

    __slots__ = ("data", "N", "K", "glu", "bf16")

    def __init__(self, data: torch.Tensor, N: int, K: int, glu: bool, bf16: bool = False):
        self.data, self.N, self.K, self.glu, self.bf16 = data, N, K, glu, bf16


def pack_skinny_w(W: torch.Tensor, glu: bool = False, bf16: bool = False) -> SkinnyW:
    """``bf16``: the engine's bf16 mode - weights rounded to bf16 (half the bytes), one bf16 MFMA per 32-wide K chunk."""
    N, K = int(W.shape[0]), int(W.shape[1])
    n = int(load().sopro_skinny_packed_floats(N, K, int(glu)))
    if n <= 0:
        raise SoproHipError(f"pack_skinny_w: unsupported shape {N}x{K} (K % 32 == 0; glu: N even)")
    Wc = W.contiguous()
    with torch.cuda.device(W.device):
        if bf16:
            out = torch.empty(n // 2, dtype=torch.int32, device=W.device)
            _check(load().sopro_pack_skinny_w_bf16(ptr(Wc), K, N, K, int(glu), ptr(out, torch.int32), _stream()), "sopro_pack_skinny_w_bf16")
        else:
            out = torch.empty(n, dtype=torch.float32, device=W.device)
            _check(load().sopro_pack_skinny_w(ptr(Wc), K, N, K, int(glu), ptr(out), _stream()), "sopro_pack_skinny_w")
    return SkinnyW(out, N, K, bool(glu), bool(bf16))


def skinny(X: torch.Tensor, W, Y: torch.Tensor, *, B: int, N: int, K: int, ldx: Optional[int] = None,
           ldy: Optional[int] = None, rms_norm: bool = False, eps: float = 1e-6, bias: Optional[torch.Tensor] = None,
           epilogue: int = EPI_NONE, R: Optional[torch.Tensor] = None, ldr: Optional[int] = None,
           scale: Optional[torch.Tensor] = None, ring: Optional[torch.Tensor] = None, dw_w: Optional[torch.Tensor] = None,
           dw_b: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None, ring_len: int = 0, ring_bcap: int = 0,
           dil: int = 1, ksize: int = 1, Xp: Optional[torch.Tensor] = None, np_: int = 0, xp_stride: int = 0,
           ksplit: bool = False, y_part_stride: int = 0, dbg: Optional[torch.Tensor] = None, mt: int = 1, nt: int = 1,
           aux_W=None, aux_Y: Optional[torch.Tensor] = None, aux_bias: Optional[torch.Tensor] = None, aux_R: Optional[torch.Tensor] = None,
           aux_flags: int = 0, aux_y_part_stride: int = 0) -> None:
    """AR-step contraction.  With rms_norm the RMSNorm weight must already be folded into W (W * w_norm[None, :]).
    ``mt`` x ``nt``: 16-row groups x column tiles per workgroup (1 or 2 each; results are bit-identical)."""
    a = SkinnyArgs()
    a.X, a.ldx = ptr(X), (K if ldx is None else ldx)
    if isinstance(W, SkinnyW):
        if (W.N, W.K, W.glu) != (N, K, epilogue == EPI_GLU_DW):
            raise SoproHipError(f"packed weight is {W.N}x{W.K} glu={W.glu}, the call says {N}x{K} glu={epilogue == EPI_GLU_DW}")
        a.W, a.ldw, a.w_layout = (ptr(W.data, torch.int32), K, 2) if W.bf16 else (ptr(W.data), K, 1)
    else:
        a.W, a.ldw = ptr(W), K
    a.bias = ptr(bias)
    n_out = N // 2 if epilogue == EPI_GLU_DW else N
    a.Y, a.ldy = ptr(Y), (n_out if ldy is None else ldy)
    a.R, a.ldr, a.scale = ptr(R), (n_out if ldr is None else ldr), ptr(scale)
    ring_bf16 = ring is not None and ring.dtype == torch.bfloat16
    a.ring, a.dw_w, a.dw_b, a.step = ptr(ring, torch.bfloat16 if ring_bf16 else torch.float32), ptr(dw_w), ptr(dw_b), ptr(step, torch.int32)
    a.ring_format = 1 if ring_bf16 else 0
    a.Xp, a.xp_stride, a.y_part_stride, a.dbg = ptr(Xp), xp_stride, y_part_stride, ptr(dbg, torch.int64)
    a.eps = eps
    a.B, a.N, a.K, a.epilogue = B, N, K, epilogue
    a.ring_len, a.ring_bcap, a.dil, a.ksize = ring_len, ring_bcap, dil, ksize
    a.np, a.ksplit, a.rms_norm = np_, int(ksplit), int(rms_norm)
    a.mt, a.nt = int(mt), int(nt)
    if aux_W is not None:  # aux column tiles (sopro_skinny_args.aux_*): a second operand set on the same input rows
        if not isinstance(aux_W, SkinnyW) or aux_W.K != K or aux_W.glu or aux_W.bf16 != (a.w_layout == 2):
            raise SoproHipError("aux_W must be a packed (non-GLU) weight of the same K and element type as W")
        a.aux_W = ptr(aux_W.data, torch.int32) if aux_W.bf16 else ptr(aux_W.data)
        a.aux_tiles, a.aux_flags = (aux_W.N + 15) // 16, int(aux_flags)
        a.aux_Y, a.aux_ldy, a.aux_bias, a.aux_R, a.aux_ldr = ptr(aux_Y), aux_W.N, ptr(aux_bias), ptr(aux_R), aux_W.N
        a.aux_y_part_stride = aux_y_part_stride
    _check(load().sopro_skinny_f32(C.byref(a), _stream()), "sopro_skinny_f32")


def norm(x: torch.Tensor, out: torch.Tensor, w: torch.Tensor, *, rows: int, C_: int, eps: float, kind: int = NORM_RMS,
         b: Optional[torch.Tensor] = None, mul: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None,
         rows_per_seg: Optional[int] = None, ldx: Optional[int] = None, ldo: Optional[int] = None, x_off: int = 0,
         o_off: int = 0, x_seg_stride: int = 0) -> None:
    _check(load().sopro_norm_f32(ptr(x) + 4 * x_off, C_ if ldx is None else ldx, x_seg_stride, ptr(out) + 4 * o_off,
                                 C_ if ldo is None else ldo, ptr(w), ptr(b), ptr(mul), ptr(add), rows,
                                 rows if rows_per_seg is None else rows_per_seg, C_, eps, kind, _stream()), "sopro_norm_f32")


def row_stats(x: torch.Tensor, rows: int, C_: int, stats: torch.Tensor, ldx: Optional[int] = None, x_seg_stride: int = 0,
              rows_per_seg: Optional[int] = None, x_off: int = 0) -> None:
    """stats [rows, C / 64, 2] = (mean, squared deviations) per 64-column group: what a contraction with ``ln_stats`` stages by."""
    _check(load().sopro_row_stats_f32(ptr(x) + 4 * x_off, C_ if ldx is None else ldx, x_seg_stride, rows, rows if rows_per_seg is None else rows_per_seg,
                                      C_, ptr(stats), _stream()), "sopro_row_stats_f32")


def rms_match(a: torch.Tensor, x: torch.Tensor, out: torch.Tensor, rows: int, C_: int) -> None:
    _check(load().sopro_rms_match_f32(ptr(a), ptr(x), ptr(out), rows, C_, _stream()), "sopro_rms_match_f32")


def tanh_affine(x: torch.Tensor, out: torch.Tensor, c0: float, c1: float, n: int) -> None:
    _check(load().sopro_tanh_affine_f32(ptr(x), ptr(out), c0, c1, n, _stream()), "sopro_tanh_affine_f32")


def add_pos(rowvec: torch.Tensor, table: torch.Tensor, out: torch.Tensor, B: int, T: int, C_: int, pos0: int = 0) -> None:
    _check(load().sopro_add_pos_f32(ptr(rowvec), ptr(table), ptr(out), B, T, C_, pos0, _stream()), "sopro_add_pos_f32")


def masked_mean(x: torch.Tensor, lens: Optional[torch.Tensor], out: torch.Tensor, B: int, T: int, C_: int) -> None:
    _check(load().sopro_masked_mean_f32(ptr(x), ptr(lens, torch.int32), ptr(out), B, T, C_, _stream()), "sopro_masked_mean_f32")


def stats_pool(h: torch.Tensor, logit: torch.Tensor, lens: Optional[torch.Tensor], out: torch.Tensor, B: int, T: int, C_: int) -> None:
    _check(load().sopro_stats_pool_f32(ptr(h), ptr(logit), ptr(lens, torch.int32), ptr(out), B, T, C_, _stream()), "sopro_stats_pool_f32")


def l2norm(x: torch.Tensor, out: torch.Tensor, rows: int, C_: int, eps: float = 1e-6) -> None:
    _check(load().sopro_l2norm_f32(ptr(x), ptr(out), rows, C_, eps, _stream()), "sopro_l2norm_f32")


def dwconv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, B: int, T: int, C_: int,
           ksize: int, dil: int, left: int, mode: int = 0, res: Optional[torch.Tensor] = None,
           lens: Optional[torch.Tensor] = None) -> None:
    _check(load().sopro_dwconv_f32(ptr(x), ptr(w), ptr(bias), ptr(res), ptr(out), ptr(lens, torch.int32), B, T, C_, ksize,
                                   dil, left, mode, _stream()), "sopro_dwconv_f32")


def codebook_sum(tok: torch.Tensor, ldt: int, col: torch.Tensor, off: torch.Tensor, wq: torch.Tensor, table: torch.Tensor,
                 out: torch.Tensor, *, rows: int, D: int, base: Optional[torch.Tensor] = None, alpha: float = 0.0,
                 beta: float = 1.0, ldo: Optional[int] = None, rows_per_seg: Optional[int] = None, o_seg_stride: int = 0,
                 o_off: int = 0, tok_off: int = 0) -> None:
    _check(load().sopro_codebook_sum_f32(ptr(tok, torch.int32) + 4 * tok_off, ldt, ptr(col, torch.int32), ptr(off, torch.int32),
                                         ptr(wq), int(col.numel()), ptr(table), int(table.shape[0]), ptr(base), alpha, beta,
                                         ptr(out) + 4 * o_off, D if ldo is None else ldo, o_seg_stride, rows,
                                         rows if rows_per_seg is None else rows_per_seg, D, _stream()), "sopro_codebook_sum_f32")


def text_embed(ids: torch.Tensor, lens: Optional[torch.Tensor], table: torch.Tensor, pe: torch.Tensor, out: torch.Tensor,
               B: int, T: int, C_: int) -> None:
    _check(load().sopro_text_embed_f32(ptr(ids, torch.int32), ptr(lens, torch.int32), ptr(table), int(table.shape[0]), ptr(pe),
                                       ptr(out), B, T, C_, _stream()), "sopro_text_embed_f32")


def argmax_rows(x: torch.Tensor, out: torch.Tensor, *, rows: int, N: int, ldx: Optional[int] = None, ldo: int = 1,
                o_off: int = 0, inner: int = 1) -> None:
    """out[(r // inner) * ldo + r % inner] = argmax(x[r, :N]): ``inner`` consecutive rows share one output row."""
    _check(load().sopro_argmax_rows_f32(ptr(x), N if ldx is None else ldx, ptr(out, torch.int32) + 4 * o_off, ldo, inner, rows, N,
                                        _stream()), "sopro_argmax_rows_f32")


def argmax_partials(part: torch.Tensor, out: torch.Tensor, *, rows: int, heads: int, per_head: int, V: int, ldp: int, ldo: int = 1,
                    o_off: int = 0) -> None:
    """Finish the arg-max that ``gemm(..., c_mode=5, C2=part)`` started: out[r * ldo + h] = token of head h of row r."""
    _check(load().sopro_argmax_partials_i32(ptr(part), ldp, ptr(out, torch.int32) + 4 * o_off, ldo, heads, per_head, V, rows, _stream()),
           "sopro_argmax_partials_i32")


def fir1(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, B: int, n_in: int, n_out: int, C_: int, K: int, stride: int,
         left: int, bias: Optional[torch.Tensor] = None, ldo: Optional[int] = None, x_seg_stride: Optional[int] = None,
         o_seg_stride: Optional[int] = None, o_off: int = 0) -> None:
    ldo = C_ if ldo is None else ldo
    _check(load().sopro_fir1_f32(ptr(x), n_in if x_seg_stride is None else x_seg_stride, n_in, ptr(w), ptr(bias) if bias is not None else None,
                                 ptr(out) + 4 * o_off, ldo, n_out * ldo if o_seg_stride is None else o_seg_stride, B, n_out, C_, K,
                                 stride, left, _stream()), "sopro_fir1_f32")


def rvq_assign(scores: torch.Tensor, table: torch.Tensor, res: torch.Tensor, codes: torch.Tensor, *, rows: int, V: int, D: int,
               ldc: int, t_off: int = 0, c_off: int = 0) -> None:
    _check(load().sopro_rvq_assign_f32(ptr(scores), V, V, ptr(table) + 4 * t_off, ptr(res), D, D, ptr(codes, torch.int32) + 4 * c_off,
                                       ldc, rows, _stream()), "sopro_rvq_assign_f32")


def attention(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, O: torch.Tensor, *, B: int, H: int, dh: int, Tq: int,
              Tk: int, ldq: int, ldk: int, ldv: int, ldo: int, q_bstride: int, k_bstride: int, v_bstride: int,
              o_bstride: int, klens: Optional[torch.Tensor] = None, causal: bool = False, q_pos0: int = 0, k_pos0: int = 0,
              window: int = 0, scale: Optional[float] = None, q_off: int = 0, k_off: int = 0, v_off: int = 0,
              o_off: int = 0, decode: bool = False, kv_index: Optional[torch.Tensor] = None, split_passes: int = 0) -> None:
    a = AttnArgs()
    a.kv_index = ptr(kv_index, torch.int32)
    a.Q, a.ldq, a.q_bstride = ptr(Q) + 4 * q_off, ldq, q_bstride
    a.K, a.ldk, a.k_bstride = ptr(K) + 4 * k_off, ldk, k_bstride
    a.V, a.ldv, a.v_bstride = ptr(V) + 4 * v_off, ldv, v_bstride
    a.O, a.ldo, a.o_bstride = ptr(O) + 4 * o_off, ldo, o_bstride
    a.klens = ptr(klens, torch.int32)
    a.B, a.H, a.dh, a.Tq, a.Tk = B, H, dh, Tq, Tk
    a.causal, a.q_pos0, a.k_pos0, a.window = int(causal), q_pos0, k_pos0, window
    a.scale = float(scale if scale is not None else dh ** -0.5)
    if decode:
        _check(load().sopro_attn_decode_f32(C.byref(a), _stream()), "sopro_attn_decode_f32")
        return
    e0 = _prof.begin() if _prof is not None else None
    if split_passes:  # the codec decoder's waveform-path form (two bf16 pieces / three passes, or one)
        _check(load().sopro_attention_split_bf16(C.byref(a), int(split_passes), _stream()), "sopro_attention_split_bf16")
    else:
        _check(load().sopro_attention_f32(C.byref(a), _stream()), "sopro_attention_f32")
    if e0 is not None:
        pairs = float(Tq) * Tk if not causal else float(sum(max(0, min(Tk - 1, q_pos0 + q - k_pos0) - max(0, q_pos0 + q - window + 1 - k_pos0) + 1) for q in range(Tq)))
        _prof.end("attention_kernel", 4.0 * dh * pairs * B * H, e0)


def xattn_step(X: torch.Tensor, Y: torch.Tensor, norm_w: Optional[torch.Tensor], Kp: torch.Tensor, Vp: torch.Tensor, klens: Optional[torch.Tensor], *,
               B: int, H: int, D: int, S_cap: int, gate: float, scale: float, eps: float, Xp: Optional[torch.Tensor] = None, np_: int = 0,
               xp_stride: int = 0, y_part_stride: int = 0, Qp: Optional[torch.Tensor] = None, nqp: int = 0, qp_stride: int = 0) -> None:
    """``Qp`` given: unfolded keys - Kp is K [B, S_cap, D] and Qp the nqp partial sums of the raw query (sopro_xattn_args.k_unfolded)."""
    a = XattnArgs()
    if Qp is not None:
        a.Qp, a.nqp, a.qp_stride, a.k_unfolded = ptr(Qp), int(nqp), int(qp_stride), 1
    a.X, a.ldx, a.Xp, a.xp_stride, a.np = ptr(X), D, ptr(Xp), xp_stride, np_
    kv16 = Kp.dtype == torch.bfloat16
    a.norm_w, a.Kp, a.Vp, a.klens = ptr(norm_w), ptr(Kp, Kp.dtype), ptr(Vp, Kp.dtype), ptr(klens, torch.int32)
    a.kv_format = 1 if kv16 else 0
    a.Y, a.y_part_stride = ptr(Y), y_part_stride
    a.eps, a.gate, a.scale = eps, gate, scale
    a.B, a.H, a.D, a.S_cap = B, H, D, S_cap
    _check(load().sopro_xattn_step_f32(C.byref(a), _stream()), "sopro_xattn_step_f32")


def rope(x: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, *, rows: int, rows_per_seg: int, pos0: int, H: int,
         dh: int, ldx: int, x_off: int = 0) -> None:
    _check(load().sopro_rope_f32(ptr(x) + 4 * x_off, ldx, ptr(cos_t), ptr(sin_t), rows, rows_per_seg, pos0, H, dh, _stream()),
           "sopro_rope_f32")


def upsample2(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, *, B: int, T: int, C_: int, y_seg_stride: int,
              y_off: int = 0) -> None:
    _check(load().sopro_upsample2_f32(ptr(x), ptr(w), ptr(y) + 4 * y_off, y_seg_stride, B, T, C_, _stream()), "sopro_upsample2_f32")


def final_conv(h: torch.Tensor, w: torch.Tensor, bias: float, wav: torch.Tensor, *, B: int, T: int, h_seg_stride: int,
               wav_seg_stride: int) -> None:
    _check(load().sopro_final_conv_f32(ptr(h), h_seg_stride, ptr(w), bias, ptr(wav), wav_seg_stride, B, T, _stream()),
           "sopro_final_conv_f32")


def seanet_tail(h: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, wf: torch.Tensor,
                bf: float, wav: torch.Tensor, *, B: int, T: int, h_seg_stride: int, wav_seg_stride: int, passes: int = 3) -> None:
    """Fused 24 kHz tail of the SEANet decoder (sopro_seanet_tail_p_f32); passes 1 = one MFMA pass on long inputs (bf16 mode)."""
    _check(load().sopro_seanet_tail_p_f32(ptr(h), h_seg_stride, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(wf), bf, ptr(wav),
                                          wav_seg_stride, B, T, passes, _stream()), "sopro_seanet_tail_p_f32")


def seanet_res128(h: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, out: torch.Tensor, *, B: int,
                  T: int, h_seg_stride: int, out_seg_stride: int, passes: int = 3) -> None:
    """Fused 128-channel residual block of the SEANet decoder + the next layer's ELU (sopro_seanet_res128_p_f32)."""
    _check(load().sopro_seanet_res128_p_f32(ptr(h), h_seg_stride, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(out), out_seg_stride, B, T,
                                            passes, _stream()), "sopro_seanet_res128_p_f32")


def seanet_up128(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, *, B: int, T: int, x_seg_stride: int,
                 out_seg_stride: int, x_off: int = 0, out_off: int = 0, passes: int = 3) -> None:
    """Weight-stationary last transposed convolution of the SEANet decoder (sopro_seanet_up128_f32); offsets in floats."""
    _check(load().sopro_seanet_up128_f32(ptr(x) + 4 * x_off, x_seg_stride, ptr(w), ptr(bias), ptr(out) + 4 * out_off, out_seg_stride, B, T,
                                         passes, _stream()), "sopro_seanet_up128_f32")


def seanet_res128_bf16(h: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, out: torch.Tensor, *, B: int,
                       T: int, h_seg_stride: int, out_seg_stride: int) -> None:
    """sopro_seanet_res128_bf16: the fused 128-channel residual block on bf16 rows (strides in bf16 elements)."""
    _check(load().sopro_seanet_res128_bf16(ptr(h, torch.bfloat16), h_seg_stride, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(out, torch.bfloat16),
                                           out_seg_stride, B, T, _stream()), "sopro_seanet_res128_bf16")


def seanet_up128_bf16(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, *, B: int, T: int, x_seg_stride: int,
                      out_seg_stride: int, x_off: int = 0, out_off: int = 0) -> None:
    """sopro_seanet_up128_bf16: the last transposed convolution on bf16 rows (offsets / strides in bf16 elements)."""
    _check(load().sopro_seanet_up128_bf16(ptr(x, torch.bfloat16) + 2 * x_off, x_seg_stride, ptr(w), ptr(bias), ptr(out, torch.bfloat16) + 2 * out_off,
                                          out_seg_stride, B, T, _stream()), "sopro_seanet_up128_bf16")


def seanet_tail_bf16(h: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, wf: torch.Tensor,
                     bf: float, wav: torch.Tensor, *, B: int, T: int, h_seg_stride: int, wav_seg_stride: int) -> None:
    """sopro_seanet_tail_bf16: the fused 24 kHz tail on bf16 rows (h_seg_stride in bf16 elements)."""
    _check(load().sopro_seanet_tail_bf16(ptr(h, torch.bfloat16), h_seg_stride, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(wf), bf, ptr(wav),
                                         wav_seg_stride, B, T, _stream()), "sopro_seanet_tail_bf16")


def seanet_uptail(x: torch.Tensor, wu: torch.Tensor, bu: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                  wf: torch.Tensor, bf: float, wav: torch.Tensor, *, B: int, T: int, x_seg_stride: int, wav_seg_stride: int, x_off: int = 0,
                  passes: int = 3) -> None:
    """The last SEANet level in one kernel (sopro_seanet_uptail_f32 / _bf16 by the dtype of ``x``): the last transposed convolution,
    the last residual block and the last layer; offsets / strides in elements of ``x``."""
    if x.dtype == torch.bfloat16:
        _check(load().sopro_seanet_uptail_bf16(ptr(x, torch.bfloat16) + 2 * x_off, x_seg_stride, ptr(wu), ptr(bu), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                               ptr(wf), bf, ptr(wav), wav_seg_stride, B, T, _stream()), "sopro_seanet_uptail_bf16")
    else:
        _check(load().sopro_seanet_uptail_f32(ptr(x) + 4 * x_off, x_seg_stride, ptr(wu), ptr(bu), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(wf), bf,
                                              ptr(wav), wav_seg_stride, B, T, passes, _stream()), "sopro_seanet_uptail_f32")


def fill_u32(t: torch.Tensor, value: int = 0) -> None:
    """Every 32-bit word of a contiguous device tensor <- value, as a kernel of the library (sopro_fill2d_u32) on the current stream."""
    n = t.numel() * t.element_size() // 4
    if not t.is_contiguous() or t.numel() * t.element_size() % 4 or n <= 0:
        raise SoproHipError("fill_u32: a contiguous tensor of whole 32-bit words")
    rows = 1
    while n // rows > (1 << 30):
        rows *= 2
    if n % rows:
        raise SoproHipError("fill_u32: tensor too large for one launch")
    _check(load().sopro_fill2d_u32(t.data_ptr(), n // rows, rows, n // rows, int(value) & 0xFFFFFFFF, _stream()), "sopro_fill2d_u32")


def copy_u32(dst: torch.Tensor, src: torch.Tensor) -> None:
    """dst <- src (contiguous device tensors of the same byte size, whole 32-bit words) as a kernel of the library."""
    n = dst.numel() * dst.element_size() // 4
    if not (dst.is_contiguous() and src.is_contiguous()) or n * 4 != src.numel() * src.element_size() or n <= 0 or n > (1 << 30):
        raise SoproHipError("copy_u32: contiguous tensors of the same size (< 4 GiB)")
    _check(load().sopro_copy2d_u32(dst.data_ptr(), n, src.data_ptr(), n, 1, n, _stream()), "sopro_copy2d_u32")


def fill2d(p: torch.Tensor, value: int, *, rows: int, width: int, pitch: int, p_off: int = 0) -> None:
    """rows x width 32-bit words, ``pitch`` words apart, <- value (sopro_fill2d_u32); ``p_off``: word offset into ``p``."""
    _check(load().sopro_fill2d_u32(ptr(p, p.dtype) + 4 * p_off, pitch, rows, width, int(value) & 0xFFFFFFFF, _stream()), "sopro_fill2d_u32")


def copy2d(dst: torch.Tensor, src: torch.Tensor, *, rows: int, width: int, dpitch: int, spitch: int, d_off: int = 0, s_off: int = 0) -> None:
    """rows x width 32-bit words between two pitched layouts (sopro_copy2d_u32); offsets in words."""
    _check(load().sopro_copy2d_u32(ptr(dst, dst.dtype) + 4 * d_off, dpitch, ptr(src, src.dtype) + 4 * s_off, spitch, rows, width, _stream()),
           "sopro_copy2d_u32")


def nar_seed(tokens: torch.Tensor, cb0: torch.Tensor, *, Q: int, B: int, T: int, vmax: int, cb0_bstride: Optional[int] = None,
             cb0_off: int = 0) -> None:
    """Column 0 of the token matrix [B T, Q] <- codebook 0 of the AR history, clamped to [0, vmax] (sopro_nar_seed_i32)."""
    _check(load().sopro_nar_seed_i32(ptr(tokens, torch.int32), Q, ptr(cb0, torch.int32) + 4 * cb0_off, T if cb0_bstride is None else cb0_bstride,
                                     B, T, vmax, _stream()), "sopro_nar_seed_i32")


def set_lds_floor(nbytes: int) -> None:
    """Minimum dynamic-LDS request of the split-bf16 GEMM launches (> 80 KiB: one workgroup per CU); see sopro_set_lds_floor."""
    _check(load().sopro_set_lds_floor(int(nbytes)), "sopro_set_lds_floor")


def ar_init(st: ArState) -> None:
    _check(load().sopro_ar_init(C.byref(st), _stream()), "sopro_ar_init")


def ar_admit(st: ArState, row: int) -> None:
    _check(load().sopro_ar_admit(C.byref(st), int(row), _stream()), "sopro_ar_admit")


def ar_sample(st: ArState, logits: torch.Tensor, ld: int) -> None:
    _check(load().sopro_ar_sample(C.byref(st), ptr(logits), ld, _stream()), "sopro_ar_sample")


def ar_issue_frame(frame: ArFrame) -> None:
    """One autoregressive frame (23 launches) on the current stream: the sequence lives in csrc/ar_frame.hip."""
    _check(load().sopro_ar_issue_frame(C.byref(frame), _stream()), "sopro_ar_issue_frame")


def ar_fold_text(txt: torch.Tensor, nkv_weight: torch.Tensor, kv_w: torch.Tensor, q_wT: torch.Tensor, o_w: torch.Tensor, nkv: torch.Tensor,
                 kvd: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, *, B: int, S: int, S_cap: int, D: int, H: int, eps: float,
                 out_off: int = 0) -> None:
    """Folded text operands of one AR cross-attention layer (sopro_ar_fold_text); ``out_off``: float offset into kp / vp."""
    _check(load().sopro_ar_fold_text(ptr(txt), ptr(nkv_weight), ptr(kv_w), ptr(q_wT), ptr(o_w), ptr(nkv), ptr(kvd), ptr(kp) + 4 * out_off,
                                     ptr(vp) + 4 * out_off, B, S, S_cap, D, H, eps, _stream()), "sopro_ar_fold_text")


def ar_fold_text_uk(txt: torch.Tensor, nkv_weight: torch.Tensor, kv_w: torch.Tensor, o_w: torch.Tensor, nkv: torch.Tensor, kvd: torch.Tensor,
                    kq: torch.Tensor, vp: torch.Tensor, *, B: int, S: int, S_cap: int, D: int, H: int, eps: float, k_off: int = 0, v_off: int = 0) -> None:
    """Text operands of one AR cross-attention layer with UNFOLDED keys (sopro_ar_fold_text_uk); offsets in floats into kq / vp."""
    _check(load().sopro_ar_fold_text_uk(ptr(txt), ptr(nkv_weight), ptr(kv_w), ptr(o_w), ptr(nkv), ptr(kvd), ptr(kq) + 4 * k_off, ptr(vp) + 4 * v_off,
                                        B, S, S_cap, D, H, eps, _stream()), "sopro_ar_fold_text_uk")


def cvt_f32_bf16(src: torch.Tensor, dst: torch.Tensor, n: Optional[int] = None, dst_off: int = 0) -> None:
    """fp32 -> bf16 image (sopro_cvt_f32_bf16); ``dst_off``: element offset into ``dst``."""
    n = int(src.numel() if n is None else n)
    _check(load().sopro_cvt_f32_bf16(ptr(src), ptr(dst, torch.bfloat16) + 2 * dst_off, n, _stream()), "sopro_cvt_f32_bf16")


def cvt_bf16_f32(src: torch.Tensor, dst: torch.Tensor, n: Optional[int] = None) -> None:
    n = int(src.numel() if n is None else n)
    _check(load().sopro_cvt_bf16_f32(ptr(src, torch.bfloat16), ptr(dst), n, _stream()), "sopro_cvt_bf16_f32")


_fade_tabs: dict = {}  # (fade_len, device) -> the join's gain table on the device


def fade_table(fade_len: int, device) -> Optional[torch.Tensor]:
    """tab[m] = fl32(0.5 - 0.5 cos(pi (m + 0.5) / fade_len)), evaluated in float64 on the host and rounded once (the raised-cosine
    gains ``sopro_join_mix_f32`` applies to the first / last ``fade_len`` kept samples of a segment); None for ``fade_len == 0``."""
    import numpy as np

    fade_len = int(fade_len)
    if fade_len <= 0:
        return None
    key = (fade_len, str(device))
    t = _fade_tabs.get(key)
    if t is None:
        tab = (0.5 - 0.5 * np.cos(np.pi * (np.arange(fade_len, dtype=np.float64) + 0.5) / fade_len)).astype(np.float32)
        t = _fade_tabs[key] = torch.from_numpy(tab).to(device)
    return t


def _lens_list(lens) -> List[int]:
    """Per-row integers (lengths, gaps) as a host list, from a host sequence or a tensor."""
    return [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]


def join_segments(wav: torch.Tensor, lens, gaps, *, hop: int = 240, rel: float = 0.01, keep: int = 3, fade_len: int = 120,
                  trim: bool = True, out: Optional[torch.Tensor] = None):
    """The long-form join (sopro_join_edges_f32 / _layout_i64 / _mix_f32, contract in include/sopro_hip.h): ``wav`` fp32
    [n_seg, >= max(lens)] on the device (rows ``wav.stride(0)`` apart: a decoder batch as it is), ``lens`` valid samples per row,
    ``gaps`` samples of silence after each row (host sequences) -> (out[:total] on the device, edges int32 [n_seg, 2] and offs int64
    [n_seg + 1] on the host).  ``out`` is allocated at the upper bound sum(lens) + sum(gaps) unless given; the three steps are
    launched back to back on the current stream and the one host copy of (offs | edges) at the end is the only synchronisation."""
    lens_h = _lens_list(lens)
    gaps_h = _lens_list(gaps)
    n = len(lens_h)
    ptr(wav)  # a contiguous-row fp32 tensor on the device, or it raises here
    if wav.dim() != 2 or int(wav.shape[0]) != n or len(gaps_h) != n:
        raise SoproHipError(f"join_segments wants wav [n_seg, samples] with one length and one gap per row, got {tuple(wav.shape)}, {n}, {len(gaps_h)}")
    if n and (min(lens_h) < 0 or min(gaps_h) < 0 or max(lens_h) > int(wav.shape[1])):
        raise SoproHipError("join_segments: lens must lie in [0, wav.shape[1]] and gaps must not be negative")
    if int(wav.shape[1]) > 1 and wav.stride(1) != 1:
        raise SoproHipError("join_segments: the samples of a row must be contiguous")
    dev = wav.device
    bound = sum(lens_h) + sum(gaps_h)
    if out is None:
        out = torch.empty(bound, dtype=torch.float32, device=dev)
    elif out.dim() != 1 or not out.is_contiguous():
        raise SoproHipError("join_segments: out must be a contiguous vector")
    if n == 0:
        return out[:0], torch.zeros(0, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    lib = load()
    max_len = max(lens_h)
    tab = fade_table(fade_len, dev)
    with torch.cuda.device(dev):
        args = torch.tensor([lens_h, gaps_h], dtype=torch.int32).to(dev)  # [2, n]: one upload
        meta = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)    # offs [n + 1] | edges [n][2] as int32 pairs: one download
        offs_d, edges_d = meta[: n + 1], meta[n + 1:].view(torch.int32)
        ws = torch.empty(max(1, int(lib.sopro_join_workspace_bytes(n, max_len, int(hop))) // 4), dtype=torch.float32, device=dev) if trim else None
        s = _stream()
        _check(lib.sopro_join_edges_f32(ptr(wav), int(wav.stride(0)), args[0].data_ptr(), n, max_len, int(hop), float(rel), int(keep), int(bool(trim)),
                                        ptr(ws), edges_d.data_ptr(), s), "sopro_join_edges_f32")
        _check(lib.sopro_join_layout_i64(edges_d.data_ptr(), args[1].data_ptr(), n, offs_d.data_ptr(), s), "sopro_join_layout_i64")
        _check(lib.sopro_join_mix_f32(ptr(wav), int(wav.stride(0)), edges_d.data_ptr(), offs_d.data_ptr(), ptr(tab), int(fade_len), n, ptr(out),
                                      int(out.numel()), s), "sopro_join_mix_f32")
        host = meta.cpu()
    offs, edges = host[: n + 1].clone(), host[n + 1:].view(torch.int32).reshape(n, 2).clone()
    total = int(offs[n])
    if total > int(out.numel()):
        raise SoproHipError(f"join_segments: the joined waveform has {total} samples, out holds {int(out.numel())}")
    return out[:total], edges, offs


# ---- speaking rate (sopro_tsm_*; definition in include/sopro_hip.h, numpy restatement in tests/tsm_ref.py) ----
TSM_W, TSM_HS, TSM_R = 960, 480, 240
SPEED_MIN, SPEED_MAX = 0.5, 2.0
tsm_calls = 0  # launches of sopro_tsm_rows_f32 by this process: the speed == 1.0 paths never add to it


def tsm_step(speed) -> int:
    """round(speed * HS * 65536): all the device sees of a speaking rate.  ``ValueError`` outside [0.5, 2.0]."""
    try:
        v = float(speed)
    except (TypeError, ValueError):
        raise ValueError(f"speed must be a number in [{SPEED_MIN}, {SPEED_MAX}], got {speed!r}") from None
    if not (SPEED_MIN <= v <= SPEED_MAX):  # (NaN fails both comparisons)
        raise ValueError(f"speed must lie in [{SPEED_MIN}, {SPEED_MAX}], got {speed!r}")
    return int(round(v * TSM_HS * 65536))


def tsm_steps(speed, rows: int) -> List[int]:
    """One step per row from a float or one float per row."""
    return [tsm_step(v) for v in _per_row(speed, rows, "speed")]


def tsm_out_len(in_len: int, step: int) -> int:
    """Samples a row of ``in_len`` samples has after the stretch: (in_len * HS * 65536) // step (sopro_tsm_out_len)."""
    in_len, step = int(in_len), int(step)
    if in_len < 0 or not (TSM_HS << 15) <= step <= (TSM_HS << 17):
        raise ValueError("in_len >= 0 and step in [HS << 15, HS << 17]")
    return (in_len * TSM_HS * 65536) // step


def tsm_blocks(out_len: int) -> int:
    return max(0, -(-int(out_len) // TSM_HS))


def _tsm_launch(wav, in_cap: int, lens_h, steps_h, state, flush: bool, out, want_deltas: bool):
    """One sopro_tsm_rows_f32 on the current stream -> (out_lens on the device, deltas on the device or None, blocks_cap)."""
    global tsm_calls
    rows = len(lens_h)
    dev = out.device
    lib = load()
    with torch.cuda.device(dev):
        args = torch.tensor([steps_h, lens_h], dtype=torch.int64).to(dev)  # one upload
        in_lens = args[1].to(torch.int32)
        out_lens = torch.empty(rows, dtype=torch.int32, device=dev)
        blocks_cap = int(out.shape[1]) // TSM_HS + 1
        deltas = torch.zeros(rows, blocks_cap, dtype=torch.int32, device=dev) if want_deltas else None
        tsm_calls += 1
        _check(lib.sopro_tsm_rows_f32(ptr(wav) if in_cap > 0 else None, int(wav.stride(0)) if in_cap > 0 else 0, in_lens.data_ptr(), int(in_cap),
                                      args[0].data_ptr(), rows, state.data_ptr() if state is not None else None, int(bool(flush)),
                                      ptr(fade_table(TSM_HS, dev)), ptr(out), int(out.stride(0)), int(out.shape[1]), out_lens.data_ptr(),
                                      deltas.data_ptr() if deltas is not None else None, blocks_cap, _stream()), "sopro_tsm_rows_f32")
    return out_lens, deltas, blocks_cap


def _check_rows(wav: torch.Tensor, lens_h: List[int], what: str) -> None:
    ptr(wav)
    if wav.dim() != 2 or int(wav.shape[0]) != len(lens_h):
        raise SoproHipError(f"{what} wants wav [rows, samples] with one length per row, got {tuple(wav.shape)} and {len(lens_h)} lengths")
    if lens_h and (min(lens_h) < 0 or max(lens_h) > int(wav.shape[1])):
        raise SoproHipError(f"{what}: lens must lie in [0, wav.shape[1]]")
    if int(wav.shape[1]) > 1 and wav.stride(1) != 1:
        raise SoproHipError(f"{what}: the samples of a row must be contiguous")


def _out_buffer(out: Optional[torch.Tensor], rows: int, cap: int, what: str) -> None:
    """A caller's ``out=`` holds fp32 [rows, >= cap] with contiguous rows (None: the operator allocates its own)."""
    if out is None:
        return
    ptr(out)
    if out.dim() != 2 or int(out.shape[0]) != rows or int(out.shape[1]) < cap or (int(out.shape[1]) > 1 and out.stride(1) != 1):
        raise SoproHipError(f"{what}: out must be fp32 [rows, >= {cap}] with contiguous rows, got {tuple(out.shape)}")


class _RowsState:
    """What the chunked forms share: ``rows`` streams whose state lives on the device (``sopro_<op>_state_bytes``), the chunk a
    ``feed`` takes with the buffer its output goes to (``sopro_<op>_chunk_out_cap``), and ``flush``."""
    _op = ""  # tsm, pitch, wm, sil

    def __init__(self, rows: int, device):
        self.rows = int(rows)
        if self.rows < 1:
            raise ValueError("rows >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise SoproHipError(f"{type(self).__name__} lives on a HIP device: the Sopro hot path has no CPU fallback")
        self.state = torch.zeros(int(getattr(load(), f"sopro_{self._op}_state_bytes")(self.rows)) // 8, dtype=torch.int64, device=self.device)

    def _chunk(self, wav: Optional[torch.Tensor], lens):
        """``wav`` [rows, n] or None, ``lens`` valid samples per row (default n) -> (n, lens on the host, the call's output buffer)."""
        if wav is None:
            n, lens_h = 0, [0] * self.rows
        else:
            n = int(wav.shape[-1])
            lens_h = [n] * self.rows if lens is None else _lens_list(lens)
            _check_rows(wav, lens_h, f"{type(self).__name__}.feed")
        cap = int(getattr(load(), f"sopro_{self._op}_chunk_out_cap")(n))
        return n, lens_h, torch.empty(self.rows, cap, dtype=torch.float32, device=self.device)

    def flush(self):
        """What the rows still hold back, their input taken as ended; the state is fresh afterwards."""
        return self.feed(None, flush=True)


def _tsm_steps_given(steps, rows: int) -> List[int]:
    """Steps handed over as they are (``prosody_steps``: a rate divided by a pitch ratio), one per row and in the operator's range."""
    vals = [int(s) for s in steps]
    if len(vals) != int(rows) or any(not (TSM_HS << 15) <= s <= (TSM_HS << 17) for s in vals):
        raise ValueError(f"steps: one per row ({rows}) in [HS << 15, HS << 17], got {vals}")
    return vals


def time_stretch(wav: torch.Tensor, lens, speed, *, out: Optional[torch.Tensor] = None, deltas: bool = False, steps=None):
    """Speaking rate on the rows of a padded batch (sopro_tsm_rows_f32, one-shot form): ``wav`` fp32 [rows, >= max(lens)] on the
    device (rows ``wav.stride(0)`` apart, any pitch), ``lens`` valid samples per row, ``speed`` a float or one per row in [0.5, 2.0]
    (> 1: faster, shorter) -> (out [rows, max(out_lens)], out_lens) with row b valid for out_lens[b] = tsm_out_len(lens[b], step_b)
    samples.  One launch on the current stream and no synchronisation: the output lengths are host arithmetic.  ``out``: a
    [rows, >= max(out_lens)] fp32 buffer to write into (nothing past a row's out_len is touched).  ``deltas=True`` (tests,
    debugging) also returns the chosen offsets d_k per row as lists, and checks the lengths the device reports (one host copy).
    ``steps``: one step per row instead of ``speed`` (which is then not looked at)."""
    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "time_stretch")
    steps_h = tsm_steps(speed, rows) if steps is None else _tsm_steps_given(steps, rows)
    out_lens_h = [tsm_out_len(n, s) for n, s in zip(lens_h, steps_h)]
    cap = max(out_lens_h, default=0)
    _out_buffer(out, rows, cap, "time_stretch")
    if out is None:
        out = torch.empty(rows, max(1, cap), dtype=torch.float32, device=wav.device)
    if rows == 0:
        return (out[:, :0], [], []) if deltas else (out[:, :0], [])
    got_d, deltas_d, blocks_cap = _tsm_launch(wav, int(wav.shape[1]), lens_h, steps_h, None, True, out, deltas)
    res = out[:, :cap]
    if not deltas:
        return res, out_lens_h
    got = got_d.tolist()
    if got != out_lens_h:
        raise SoproHipError(f"time_stretch: the device reports lengths {got}, the host expected {out_lens_h}")
    d = deltas_d.cpu().tolist()
    return res, out_lens_h, [d[b][: tsm_blocks(out_lens_h[b])] for b in range(rows)]


class TimeStretchState(_RowsState):
    """Chunked form of ``time_stretch`` for ``rows`` streams: ``feed`` appends a chunk per row and returns the blocks that became
    ready, ``flush`` the rest.  Any chunking followed by ``flush`` gives the one-shot result bit for bit.  The state (block index,
    last position, samples received, a retained tail of < 1920 samples per row) lives on the device; every call is one launch and
    one small host copy (the lengths it produced)."""

    _op = "tsm"

    def __init__(self, rows: int, speed, device, *, steps=None):
        super().__init__(rows, device)
        self.steps = tsm_steps(speed, self.rows) if steps is None else _tsm_steps_given(steps, self.rows)

    def feed(self, wav: Optional[torch.Tensor], lens=None, *, flush: bool = False, deltas: bool = False):
        """``wav`` [rows, n] (row b valid for lens[b] samples; default n) -> (out [rows, max(out_lens)], out_lens[, deltas])."""
        n, lens_h, out = self._chunk(wav, lens)
        got_d, deltas_d, _ = _tsm_launch(wav, n, lens_h, self.steps, self.state, flush, out, deltas)
        got = got_d.tolist()
        if min(got) < 0:
            raise SoproHipError("TimeStretchState: a row's blocks did not fit the output buffer")
        res = out[:, : max(got)]
        if not deltas:
            return res, got
        d = deltas_d.cpu().tolist()
        return res, got, [d[b][: tsm_blocks(got[b])] for b in range(self.rows)]

    def flush(self, *, deltas: bool = False):
        """The remaining blocks (zero extension, the last one cut at the row's total output length); the state is fresh afterwards."""
        return self.feed(None, flush=True, deltas=deltas)


# ---- pitch (sopro_pitch_*; definition in include/sopro_hip.h, numpy restatement in tests/pitch_ref.py) ----
PITCH_NT, PITCH_P, PITCH_TILE = 64, 256, 2048
PITCH_MIN, PITCH_MAX = -12.0, 12.0
PITCH_ONE = 1 << 32  # the increment of pitch 0: the resampler is a copy there
pitch_calls = 0  # calls of sopro_pitch_rows_f32 by this process (one launch each; a chunked call adds its small state update): the
#                  pitch == 0 paths never add to it
_pitch_banks: dict = {}  # (max(inc, 2^32), device) -> [257, 64] on the device; a tuple of such keys -> the stacked banks of a batch


def pitch_inc(semitones) -> int:
    """round(2^(semitones / 12) * 2^32): all the device sees of a pitch.  ``ValueError`` outside [-12, 12]."""
    try:
        v = float(semitones)
    except (TypeError, ValueError):
        raise ValueError(f"pitch must be a number of semitones in [{PITCH_MIN}, {PITCH_MAX}], got {semitones!r}") from None
    if not (PITCH_MIN <= v <= PITCH_MAX):  # (NaN fails both comparisons)
        raise ValueError(f"pitch must lie in [{PITCH_MIN}, {PITCH_MAX}] semitones, got {semitones!r}")
    return min(1 << 33, max(1 << 31, int(round(2.0 ** (v / 12.0) * 4294967296.0))))


def _per_row(value, rows: int, what: str) -> list:
    if isinstance(value, (list, tuple)) or (hasattr(value, "__len__") and not isinstance(value, str)):
        vals = list(value)
        if len(vals) != int(rows):
            raise ValueError(f"{what}: one value or one per row ({rows}), got {len(vals)}")
        return vals
    return [value] * int(rows)


def pitch_incs(pitch, rows: int) -> List[int]:
    """One increment per row from a number of semitones or one per row."""
    return [pitch_inc(v) for v in _per_row(pitch, rows, "pitch")]


def pitch_out_len(in_len: int, inc: int) -> int:
    """Samples a row of ``in_len`` samples has after the resampler: (in_len << 32) // inc (sopro_pitch_out_len)."""
    in_len, inc = int(in_len), int(inc)
    if in_len < 0 or in_len > (1 << 30) or not (1 << 31) <= inc <= (1 << 33):
        raise ValueError("in_len in [0, 2^30] and inc in [2^31, 2^33]")
    return (in_len << 32) // inc


def prosody_step(speed, pitch) -> Tuple[int, int]:
    """(stretch step, resampler increment) for one speaking rate and one pitch: a shift by rho = inc / 2^32 is a stretch by rho and
    a resample that reads rho times as fast, so the stretch runs at speed / rho: step' = round(speed * 480 * 65536 * 2^32 / inc)
    (``tsm_step(speed)`` at pitch 0).  ``ValueError`` for a ``speed`` or a ``pitch`` out of range, and for a pair whose step' is
    outside the stretch's own range."""
    tsm_step(speed)
    inc = pitch_inc(pitch)
    step = int(round(float(speed) * TSM_HS * 65536 * 4294967296.0 / inc))
    if not (TSM_HS << 15) <= step <= (TSM_HS << 17):
        raise ValueError(f"speed={speed!r} with pitch={pitch!r}: speed / 2^(pitch / 12) must lie in [{SPEED_MIN}, {SPEED_MAX}] "
                         "(the pitch shift stretches by 2^(pitch / 12) before it resamples)")
    return step, inc


def prosody_steps(speed, pitch, rows: int) -> List[Tuple[int, int]]:
    """``prosody_step`` per row, from one value or one per row of each."""
    return [prosody_step(sp, pt) for sp, pt in zip(_per_row(speed, rows, "speed"), _per_row(pitch, rows, "pitch"))]


def is_plain(pairs) -> bool:
    """Neither stage has anything to do for any row."""
    return all(step == TSM_HS << 16 and inc == PITCH_ONE for step, inc in pairs)


def pitch_bank_host(inc: int):
    """The filter bank of an increment, float32 [257, 64] (numpy): Kaiser-windowed sinc rows (beta = 7, cut-off
    0.5 min(1, 2^32 / inc) - 0.034 cycles per input sample), evaluated in float64, each row normalised to sum 1, rounded once."""
    import numpy as np

    fc = 0.5 * min(1.0, PITCH_ONE / max(int(inc), PITCH_ONE)) - 0.034
    p = np.arange(PITCH_P + 1, dtype=np.float64)[:, None]
    j = np.arange(PITCH_NT, dtype=np.float64)[None, :]
    t = j - (PITCH_NT // 2 - 1) - p / PITCH_P
    u = 1.0 - (t / (PITCH_NT // 2)) ** 2
    w = np.where(u > 0.0, np.i0(7.0 * np.sqrt(np.maximum(u, 0.0))) / np.i0(7.0), 0.0)
    g = 2.0 * fc * np.sinc(2.0 * fc * t) * w
    return (g / g.sum(axis=1, keepdims=True)).astype(np.float32)


def pitch_bank(inc: int, device) -> torch.Tensor:
    """``pitch_bank_host`` on the device, cached per (max(inc, 2^32), device): every inc <= 2^32 has the same bank."""
    key = (max(int(inc), PITCH_ONE), str(device))
    t = _pitch_banks.get(key)
    if t is None:
        t = _pitch_banks[key] = torch.from_numpy(pitch_bank_host(key[0])).to(device)
    return t


def _pitch_banks_for(incs_h: List[int], device) -> Tuple[torch.Tensor, List[int]]:
    """The banks a batch needs, [n_banks, 257, 64], and every row's index into them (rows at 2^32 never read theirs)."""
    keys: List[int] = []
    idx = []
    for inc in incs_h:
        k = max(int(inc), PITCH_ONE)
        if k not in keys:
            keys.append(k)
        idx.append(keys.index(k))
    if len(keys) == 1:
        return pitch_bank(keys[0], device).unsqueeze(0), idx
    key = (tuple(keys), str(device))
    t = _pitch_banks.get(key)
    if t is None:
        if len(_pitch_banks) > 64:  # (a service with a new mix of pitches per batch: the stacks are cheap to make again)
            for k in [k for k in _pitch_banks if isinstance(k[0], tuple)]:
                del _pitch_banks[k]
        t = _pitch_banks[key] = torch.stack([pitch_bank(k, device) for k in keys])
    return t, idx


def _pitch_launch(wav, in_cap: int, lens_h, incs_h, state, flush: bool, out):
    """One sopro_pitch_rows_f32 on the current stream -> out_lens on the device."""
    global pitch_calls
    rows = len(lens_h)
    dev = out.device
    lib = load()
    with torch.cuda.device(dev):
        banks, idx = _pitch_banks_for(incs_h, dev)
        args = torch.tensor([incs_h, lens_h, idx], dtype=torch.int64).to(dev)  # one upload
        small = args[1:].to(torch.int32)
        out_lens = torch.empty(rows, dtype=torch.int32, device=dev)
        pitch_calls += 1
        _check(lib.sopro_pitch_rows_f32(ptr(wav) if in_cap > 0 else None, int(wav.stride(0)) if in_cap > 0 else 0, small[0].data_ptr(), int(in_cap),
                                        args[0].data_ptr(), small[1].data_ptr(), ptr(banks), int(banks.shape[0]), rows,
                                        state.data_ptr() if state is not None else None, int(bool(flush)), ptr(out), int(out.stride(0)),
                                        int(out.shape[1]), out_lens.data_ptr(), _stream()), "sopro_pitch_rows_f32")
    return out_lens


def pitch_shift(wav: torch.Tensor, lens, pitch, *, out: Optional[torch.Tensor] = None, incs=None):
    """The resampler of the pitch control on the rows of a padded batch (sopro_pitch_rows_f32, one-shot form): ``wav`` fp32
    [rows, >= max(lens)] on the device (rows ``wav.stride(0)`` apart, any alignment), ``lens`` valid samples per row, ``pitch``
    semitones in [-12, 12], one value or one per row -> (out [rows, max(out_lens)], out_lens) with row b valid for out_lens[b] =
    pitch_out_len(lens[b], inc_b) samples: every frequency of the row multiplied by 2^(pitch / 12), and the duration divided by it
    (the public ``pitch=`` stretches by the same ratio first: ``prosody_steps``).  One launch on the current stream and no
    synchronisation: the output lengths are host arithmetic.  ``out``: a [rows, >= max(out_lens)] fp32 buffer to write into
    (nothing past a row's out_len is touched).  ``incs``: one increment per row instead of ``pitch``."""
    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "pitch_shift")
    incs_h = pitch_incs(pitch, rows) if incs is None else [int(v) for v in incs]
    if len(incs_h) != rows:
        raise ValueError(f"incs: one per row ({rows}), got {len(incs_h)}")
    out_lens_h = [pitch_out_len(n, s) for n, s in zip(lens_h, incs_h)]
    cap = max(out_lens_h, default=0)
    _out_buffer(out, rows, cap, "pitch_shift")
    if out is None:
        out = torch.empty(rows, max(1, cap), dtype=torch.float32, device=wav.device)
    if rows == 0:
        return out[:, :0], []
    _pitch_launch(wav, int(wav.shape[1]), lens_h, incs_h, None, True, out)
    return out[:, :cap], out_lens_h


def apply_prosody(wav: torch.Tensor, lens, pairs) -> Tuple[torch.Tensor, List[int]]:
    """Speaking rate and pitch on a padded batch: ``time_stretch`` at every row's step', then ``pitch_shift`` at its inc
    (``pairs`` from ``prosody_steps``), on the current stream.  A stage at its identity for every row is not launched; a row at
    its identity in a launched stage comes back bit for bit."""
    lens = _lens_list(lens)
    steps, incs = [p[0] for p in pairs], [p[1] for p in pairs]
    if any(s != TSM_HS << 16 for s in steps):
        wav, lens = time_stretch(wav, lens, None, steps=steps)
    if any(i != PITCH_ONE for i in incs):
        wav, lens = pitch_shift(wav, lens, None, incs=incs)
    return wav, lens


class PitchShiftState(_RowsState):
    """Chunked form of ``pitch_shift`` for ``rows`` streams: ``feed`` appends a chunk per row and returns the outputs whose taps
    are all in, ``flush`` the rest.  Any chunking followed by ``flush`` gives the one-shot result bit for bit.  The state (next
    output, samples received, a retained tail of < 64 samples per row) lives on the device; every call is one launch plus the
    state's small update and one small host copy (the lengths it produced)."""

    _op = "pitch"

    def __init__(self, rows: int, pitch, device, *, incs=None):
        super().__init__(rows, device)
        self.incs = pitch_incs(pitch, self.rows) if incs is None else [int(v) for v in incs]
        if len(self.incs) != self.rows:
            raise ValueError(f"incs: one per row ({self.rows}), got {len(self.incs)}")

    def feed(self, wav: Optional[torch.Tensor], lens=None, *, flush: bool = False):
        """``wav`` [rows, n] (row b valid for lens[b] samples; default n) -> (out [rows, max(out_lens)], out_lens)."""
        n, lens_h, out = self._chunk(wav, lens)
        got = _pitch_launch(wav, n, lens_h, self.incs, self.state, flush, out).tolist()
        if min(got) < 0:
            raise SoproHipError("PitchShiftState: a row's outputs did not fit the output buffer")
        return out[:, : max(got)], got


# ---- formant control (sopro_formant_*; definition in include/sopro_hip.h, numpy restatement in tests/formant_ref.py) ----
FM_N, FM_H, FM_Q, FM_STATE = 512, 128, 32, 896
FORMANT_ONE = 1.0  # 1 / sigma of a row whose envelope stays where the pitch put it: nothing to do
formant_calls = 0  # calls of sopro_formant_rows_f32 by this process: the formant=None paths never add to it


def formant_inv(formant, pitch=0.0) -> float:
    """1 / sigma as the fp32 value the device sees (a Python float that holds it exactly), sigma = 2^((formant - pitch) / 12): the
    factor the envelope is warped by so that it sits ``formant`` semitones from the decoded voice's after a shift by ``pitch``.
    ``formant=None``: the envelope goes where ``pitch`` takes it, 1.0.  Computed in float64, rounded once.  ``ValueError`` for a
    ``pitch`` out of range, a ``formant`` that is no finite number, and a sigma outside [0.5, 2]."""
    pitch_inc(pitch)
    if formant is None:
        return FORMANT_ONE
    try:
        d = float(formant) - float(pitch)
    except (TypeError, ValueError):
        raise ValueError(f"formant must be None or a number of semitones, got {formant!r}") from None
    if not (-12.0 <= d <= 12.0):  # (NaN fails both comparisons)
        raise ValueError(f"formant={formant!r} with pitch={pitch!r}: sigma = 2^((formant - pitch) / 12) must lie in [0.5, 2.0]")
    return struct.unpack("f", struct.pack("f", min(2.0, max(0.5, 2.0 ** (-d / 12.0)))))[0]


def _formant_invs_given(invs, rows: int) -> List[float]:
    vals = [float(v) for v in _per_row(invs, rows, "invs")]
    if any(not (0.5 <= v <= 2.0) or struct.unpack("f", struct.pack("f", v))[0] != v for v in vals):
        raise ValueError(f"invs: fp32 values in [0.5, 2.0] (formant_inv), got {vals}")
    return vals


def _formant_launch(wav, lens_h, invs_h, state, held, phase: int, flush: bool, out) -> List[int]:
    """One sopro_formant_rows_f32 on the current stream -> the rows' output lengths (host arithmetic of the library: no copy)."""
    global formant_calls
    rows = len(lens_h)
    dev = out.device
    lib = load()
    n_in = max(lens_h, default=0)
    with torch.cuda.device(dev):
        cap = int(out.shape[1])
        ws_bytes = int(lib.sopro_formant_workspace_bytes(rows, cap))
        if ws_bytes < 0:
            raise SoproHipError(f"formant: {rows} rows of up to {cap} samples are outside the operator's range")
        ws = torch.empty(max(1, ws_bytes // 8), dtype=torch.int64, device=dev)
        got = (C.c_int32 * rows)()
        formant_calls += 1
        _check(lib.sopro_formant_rows_f32(ptr(wav) if n_in > 0 else None, int(wav.stride(0)) if n_in > 0 else 0, (C.c_int32 * rows)(*lens_h),
                                          (C.c_float * rows)(*invs_h), rows, state.data_ptr() if state is not None else None,
                                          (C.c_int32 * rows)(*held) if held is not None else None, int(phase), int(bool(flush)), ptr(out),
                                          int(out.stride(0)), cap, got, ws.data_ptr(), ws_bytes, _stream()), "sopro_formant_rows_f32")
    return list(got)


def formant_shift(wav: torch.Tensor, lens, invs, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The envelope warp of the formant control on the rows of a padded batch (sopro_formant_rows_f32, one-shot form): ``wav`` fp32
    [rows, >= max(lens)] on the device (rows ``wav.stride(0)`` apart, any alignment), ``lens`` valid samples per row, ``invs`` one
    1 / sigma or one per row (``formant_inv``) -> out [rows, max(lens)], row b valid for lens[b] samples: the row with its spectral
    envelope's frequencies multiplied by sigma, its pitch, length and timing as they were; a row at 1.0 comes back bit for bit.  Two
    launches per 64 rows on the current stream and no synchronisation.  ``out``: a [rows, >= max(lens)] fp32 buffer to write into
    (nothing past a row's length is touched); it must not overlap ``wav``.  All rows at 1.0: nothing is launched and
    ``wav[:, :max(lens)]`` is returned as it is."""
    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "formant_shift")
    invs_h = _formant_invs_given(invs, rows)
    cap = max(lens_h, default=0)
    _out_buffer(out, rows, cap, "formant_shift")
    if rows == 0 or cap == 0 or all(v == FORMANT_ONE for v in invs_h):
        if out is None:
            return wav[:, :cap]
        out[:, :cap].copy_(wav[:, :cap])  # (a caller that asked for its own buffer gets the rows there)
        return out[:, :cap]
    if out is None:
        out = torch.empty(rows, cap, dtype=torch.float32, device=wav.device)
    _formant_launch(wav, lens_h, invs_h, None, None, 0, True, out)
    return out[:, :cap]


class FormantState(_RowsState):
    """Chunked form of ``formant_shift`` for ``rows`` streams: ``feed`` appends a chunk per row and returns the 128-sample hops whose
    four frames are all in (a hop comes out once the 512 samples of its last frame are there, so fewer than 512 samples are held
    back), ``flush`` the rest, zero-extended.  Any chunking followed by ``flush`` gives the one-shot result bit for bit: the frame
    grid is fixed from sample 0.  The state (the last 384 emitted samples and the held ones, two halves written in turn) lives on the
    device; the counts are host arithmetic, so a call is two or three launches and copies nothing back."""

    _op = "formant"

    def __init__(self, rows: int, invs, device):
        super().__init__(rows, device)
        self.invs = _formant_invs_given(invs, self.rows)
        self.held = [0] * self.rows
        self.phase = 0

    def feed(self, wav: Optional[torch.Tensor], lens=None, *, flush: bool = False):
        """``wav`` [rows, n] (row b valid for lens[b] samples; default n) -> (out [rows, max(out_lens)], out_lens)."""
        n, lens_h, out = self._chunk(wav, lens)
        if n == 0 and not (flush and any(self.held)):  # (nothing new and nothing to bring out: the state stays as it is)
            return out[:, :0], [0] * self.rows
        got = _formant_launch(wav, lens_h, self.invs, self.state, self.held, self.phase, flush, out)
        self.held = [0 if flush else h + a - g for h, a, g in zip(self.held, lens_h, got)]
        self.phase ^= 1
        return out[:, : max(got)], got


# ---- watermark (sopro_wm_*; definition in include/sopro_hip.h, numpy restatement in tests/wm_ref.py; host tables in watermark.py) ----
WM_HS, WM_P, WM_TILE, WM_TAIL = 480, 8192, 3840, 1536
_wm_calls = {"embed": 0, "detect": 0}  # calls of sopro_wm_embed_rows_f32 / of the detector's launch sequence by this process


def wm_calls() -> int:
    """Calls of the watermark kernels by this process (embedder and detector together): the ``watermark=None`` paths never add to it."""
    return _wm_calls["embed"] + _wm_calls["detect"]


def _wm_launch(wav, in_cap: int, lens_h, marks, state, flush: bool, out):
    """One sopro_wm_embed_rows_f32 on the current stream -> out_lens on the device."""
    import numpy as np

    from . import watermark as wm

    rows = len(lens_h)
    dev = out.device
    lib = load()
    with torch.cuda.device(dev):
        cars, idx = wm.carrier_tables(marks, dev)
        alpha_bits = np.array([m.alpha if m is not None else 0.0 for m in marks], dtype=np.float32).view(np.int32).tolist()
        args = torch.tensor([lens_h, idx, alpha_bits], dtype=torch.int32).to(dev)  # one upload
        out_lens = torch.empty(rows, dtype=torch.int32, device=dev)
        _wm_calls["embed"] += 1
        _check(lib.sopro_wm_embed_rows_f32(ptr(wav) if in_cap > 0 else None, int(wav.stride(0)) if in_cap > 0 else 0, args[0].data_ptr(), int(in_cap),
                                           args[1].data_ptr(), cars.data_ptr(), int(cars.shape[0]), args[2].data_ptr(), rows,
                                           state.data_ptr() if state is not None else None, int(bool(flush)), ptr(fade_table(WM_HS, dev)),
                                           ptr(out), int(out.stride(0)), int(out.shape[1]), out_lens.data_ptr(), _stream()),
               "sopro_wm_embed_rows_f32")
    return out_lens


def wm_embed(wav: torch.Tensor, lens, marks, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The watermark on the rows of a padded batch (sopro_wm_embed_rows_f32, one-shot form): ``wav`` fp32 [rows, >= max(lens)] on
    the device (rows ``wav.stride(0)`` apart, any alignment), ``lens`` valid samples per row, ``marks`` one ``Watermark`` or None,
    or one per row -> out [rows, max(lens)], row b valid for lens[b] samples: the row plus its mark's carrier at ``strength_db``
    below the row's local peak; a row whose mark is None comes back bit for bit.  One launch on the current stream and no
    synchronisation.  ``out``: a [rows, >= max(lens)] fp32 buffer to write into (nothing past a row's length is touched); it must
    not overlap ``wav`` (a tile reads its neighbours' samples).  All marks None: nothing is launched and ``wav[:, :max(lens)]`` is
    returned as it is."""
    from . import watermark as wm

    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "wm_embed")
    marks = wm.per_row(marks, rows, "marks")
    cap = max(lens_h, default=0)
    _out_buffer(out, rows, cap, "wm_embed")
    if rows == 0 or all(m is None for m in marks):
        if out is None:
            return wav[:, :cap]
        out[:, :cap].copy_(wav[:, :cap])  # (a caller that asked for its own buffer gets the rows there)
        return out[:, :cap]
    if out is None:
        out = torch.empty(rows, max(1, cap), dtype=torch.float32, device=wav.device)
    _wm_launch(wav, int(wav.shape[1]), lens_h, marks, None, True, out)
    return out[:, :cap]


class WatermarkState(_RowsState):
    """Chunked form of ``wm_embed`` for ``rows`` streams: ``feed`` appends a chunk per row and returns the 480-sample blocks whose
    envelope is final (a chunk comes out up to 1440 samples short, and the rest follows), ``flush`` the rest.  Any chunking followed
    by ``flush`` gives the one-shot result bit for bit.  The state (samples emitted, samples received, a retained tail of < 1440
    samples per row) lives on the device; every call is one launch plus the state's small update and one small host copy (the
    lengths it produced)."""

    _op = "wm"

    def __init__(self, rows: int, marks, device):
        from . import watermark as wm

        super().__init__(rows, device)
        self.marks = wm.per_row(marks, self.rows, "marks")

    def feed(self, wav: Optional[torch.Tensor], lens=None, *, flush: bool = False):
        """``wav`` [rows, n] (row b valid for lens[b] samples; default n) -> (out [rows, max(out_lens)], out_lens)."""
        n, lens_h, out = self._chunk(wav, lens)
        got = _wm_launch(wav, n, lens_h, self.marks, self.state, flush, out).tolist()
        if min(got) < 0:
            raise SoproHipError("WatermarkState: a row's samples did not fit the output buffer")
        return out[:, : max(got)], got


def wm_detect_rows(wav: torch.Tensor, lens, keys, *, details: bool = False):
    """The watermark detector on the rows of a padded batch (sopro_wm_fold_rows_f32, _corr_rows_f32, _peak_rows_f32): ``wav`` fp32
    [rows, >= max(lens)] on the device, ``lens`` valid samples per row, ``keys`` one 64-bit key per row -> one
    ``watermark.WatermarkResult`` per row.  Four launches on the current stream and one small host copy (two offsets and two peak
    statistics per row).  ``details=True`` (tests) also returns the folded rows f [rows, 8192] and the correlations R [rows, 2, 8192]."""
    from . import watermark as wm

    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "wm_detect_rows")
    keys = list(keys)
    if len(keys) != rows:
        raise ValueError(f"keys: one per row ({rows}), got {len(keys)}")
    if rows == 0:
        return ([], None, None) if details else []
    dev = wav.device
    lib = load()
    in_cap = int(wav.shape[1])
    with torch.cuda.device(dev):
        dtab, idx = wm.template_tables(keys, dev)
        args = torch.tensor([lens_h, idx], dtype=torch.int32).to(dev)  # one upload
        ws = torch.empty(max(1, int(lib.sopro_wm_fold_ws_bytes(rows, in_cap)) // 4), dtype=torch.float32, device=dev)
        f = torch.empty(rows, WM_P, dtype=torch.float32, device=dev)
        R = torch.empty(rows, 2, WM_P, dtype=torch.float32, device=dev)
        pk = torch.empty(rows, 4, dtype=torch.int32, device=dev)
        s = _stream()
        _wm_calls["detect"] += 1
        _check(lib.sopro_wm_fold_rows_f32(ptr(wav), int(wav.stride(0)), args[0].data_ptr(), in_cap, rows, ptr(fade_table(WM_HS, dev)), ws.data_ptr(),
                                          f.data_ptr(), s), "sopro_wm_fold_rows_f32")
        _check(lib.sopro_wm_corr_rows_f32(f.data_ptr(), dtab.data_ptr(), int(dtab.shape[0]), args[1].data_ptr(), rows, R.data_ptr(), s),
               "sopro_wm_corr_rows_f32")
        _check(lib.sopro_wm_peak_rows_f32(R.data_ptr(), rows, pk.data_ptr(), s), "sopro_wm_peak_rows_f32")
        host = pk.cpu()
    o = host[:, :2].tolist()
    z = host[:, 2:].contiguous().view(torch.float32).tolist()
    res = [wm.result_of(o[b][0], o[b][1], z[b][0], z[b][1]) for b in range(rows)]
    return (res, f, R) if details else res


# ---- silence control (sopro_sil_*; definition in include/sopro_hip.h, numpy restatement in tests/sil_ref.py; parameters in silence.py) ----
SIL_HOP, SIL_TAIL, SIL_TILE, SIL_PLAN_WORDS = 240, 4608, 2048, 64
sil_calls = 0  # calls of sopro_sil_rows_f32 by this process: the silence=None paths never add to it


def _sil_cuts_cap(lens_h, sils) -> int:
    """Cuts a row can have: one per cap_h + 2 hops (a run longer than the cap and the active hop that ends it), the leading and the
    trailing one."""
    return max((-(-n // SIL_HOP)) // (s.cap_hops + 2) + 2 if s is not None else 0 for n, s in zip(lens_h, sils))


def _sil_launch(wav, in_cap: int, lens_h, tot_h, sils, state, flush: bool, out):
    """One sopro_sil_rows_f32 on the current stream and one host copy of what it found -> (out_lens, cuts per row as (source
    position, samples removed) tuples).  ``tot_h``: the samples a row can hold cuts for (a chunked row: everything received)."""
    global sil_calls
    import numpy as np

    rows = len(lens_h)
    dev = out.device
    lib = load()
    with torch.cuda.device(dev):
        thr_bits = np.array([s.thr if s is not None else 1.0 for s in sils], dtype=np.float32).view(np.int32).tolist()
        args = torch.tensor([lens_h, [s.cap_hops if s is not None else 0 for s in sils], [s.onset_hops if s is not None else 1 for s in sils],
                             thr_bits], dtype=torch.int32).to(dev)  # one upload
        cuts_cap = max(1, _sil_cuts_cap(tot_h, sils))
        vcap = int(in_cap) if state is None else int(lib.sopro_sil_chunk_out_cap(int(in_cap)))
        ws = torch.empty(max(1, int(lib.sopro_sil_ws_bytes(rows, vcap)) // 8), dtype=torch.int64, device=dev)
        res = torch.empty(rows * (2 + 2 * cuts_cap), dtype=torch.int32, device=dev)  # out_lens | n_cuts | cuts: one download
        out_lens, n_cuts, cuts = res[:rows], res[rows: 2 * rows], res[2 * rows:]
        sil_calls += 1
        _check(lib.sopro_sil_rows_f32(ptr(wav) if in_cap > 0 else None, int(wav.stride(0)) if in_cap > 0 else 0, args[0].data_ptr(), int(in_cap),
                                      args[3].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), rows,
                                      state.data_ptr() if state is not None else None, int(bool(flush)), ptr(fade_table(SIL_HOP, dev)),
                                      ws.data_ptr(), ptr(out), int(out.stride(0)), int(out.shape[1]), out_lens.data_ptr(), cuts.data_ptr(),
                                      cuts_cap, n_cuts.data_ptr(), _stream()), "sopro_sil_rows_f32")
        host = res.cpu()
    got = host[:rows].tolist()
    nc = host[rows: 2 * rows].tolist()
    table = host[2 * rows:].reshape(rows, cuts_cap, 2).tolist()
    return got, [[(int(p), int(n)) for p, n in table[r][: nc[r]]] for r in range(rows)]


def silence_squeeze(wav: torch.Tensor, lens, sils, *, out: Optional[torch.Tensor] = None):
    """Silence control on the rows of a padded batch (sopro_sil_rows_f32, one-shot form): ``wav`` fp32 [rows, >= max(lens)] on the
    device (rows ``wav.stride(0)`` apart, any alignment), ``lens`` valid samples per row, ``sils`` one ``Silence`` or None, or one
    per row -> (out [rows, max(out_lens)], out_lens, cuts): row b valid for out_lens[b] samples, cuts[b] its (source position,
    samples removed) pairs in order (``align.map_cuts``).  A row whose ``Silence`` is None comes back bit for bit, without cuts.
    Three launches on the current stream and one small host copy (the lengths and the cuts).  ``out``: a [rows, >= max(lens)] fp32
    buffer to write into; it must not overlap ``wav``.  All None: nothing is launched and ``wav[:, :max(lens)]`` is returned as it is."""
    from . import silence as S

    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "silence_squeeze")
    sils = S.per_row(sils, rows, "sils")
    cap = max(lens_h, default=0)
    _out_buffer(out, rows, cap, "silence_squeeze")
    if rows == 0 or all(s is None for s in sils):
        if out is None:
            return wav[:, :cap], lens_h, [[] for _ in range(rows)]
        out[:, :cap].copy_(wav[:, :cap])  # (a caller that asked for its own buffer gets the rows there)
        return out[:, :cap], lens_h, [[] for _ in range(rows)]
    if out is None:
        out = torch.empty(rows, max(1, cap), dtype=torch.float32, device=wav.device)
    got, cuts = _sil_launch(wav, int(wav.shape[1]), lens_h, lens_h, sils, None, True, out)
    if min(got) < 0:
        raise SoproHipError("silence_squeeze: a row's samples or cuts did not fit")
    return out[:, : max(got)], got, cuts


class SilenceState(_RowsState):
    """Chunked form of ``silence_squeeze`` for ``rows`` streams: ``feed`` appends a chunk per row and returns what is decided (sound
    at once, the first hops of a pause at once, the rest of a pause when sound resumes), ``flush`` the rest.  Any chunking followed by
    ``flush`` gives the one-shot result bit for bit.  The state (speech seen, run length, samples received and emitted, a retained
    tail of at most 18 hops and 239 samples per row) lives on the device; every call is four launches and one small host copy.
    ``cuts[b]`` collects row b's cuts, in the row's total source coordinates, until the flush that ends the row."""

    _op = "sil"

    def __init__(self, rows: int, sils, device):
        from . import silence as S

        super().__init__(rows, device)
        self.sils = S.per_row(sils, self.rows, "sils")
        self.recv = [0] * self.rows
        self.cuts: List[list] = [[] for _ in range(self.rows)]
        self._ended = False

    def feed(self, wav: Optional[torch.Tensor], lens=None, *, flush: bool = False):
        """``wav`` [rows, n] (row b valid for lens[b] samples; default n) -> (out [rows, max(out_lens)], out_lens)."""
        if self._ended:  # (the first call after a flush starts new rows)
            self.recv, self.cuts, self._ended = [0] * self.rows, [[] for _ in range(self.rows)], False
        n, lens_h, out = self._chunk(wav, lens)
        self.recv = [a + b for a, b in zip(self.recv, lens_h)]
        got, cuts = _sil_launch(wav, n, lens_h, self.recv, self.sils, self.state, flush, out)
        if min(got) < 0:
            raise SoproHipError("SilenceState: a row's samples or cuts did not fit")
        for b in range(self.rows):
            self.cuts[b] += cuts[b]
        self._ended = bool(flush)
        return out[:, : max(got)], got


# ---- reference denoising (sopro_denoise_*; definition in include/sopro_hip.h, numpy restatement in tests/denoise_ref.py; parameters in denoise.py) ----
DN_N, DN_H, DN_BINS, DN_SPAN = 512, 128, 257, 94
denoise_calls = 0  # calls of sopro_denoise_rows_f32 by this process: the denoise=None paths never add to it


def denoise(wav: torch.Tensor, lens, params, *, out: Optional[torch.Tensor] = None, report: bool = False):
    """The stationary-noise suppressor on the rows of a padded batch (sopro_denoise_rows_f32): ``wav`` fp32 [rows, >= max(lens)] on
    the device (rows ``wav.stride(0)`` apart, any alignment), ``lens`` valid samples per row, ``params`` one ``Denoise`` or None, or
    one per row -> out [rows, max(lens)], row b valid for lens[b] samples; a row whose ``Denoise`` is None comes back bit for bit.
    Five launches per 64 rows on the current stream and no synchronisation (the lengths and parameters are host values that travel
    as kernel arguments).  ``report=True`` -> (out, [DenoiseReport or None per row]), which costs one small host copy.  ``out``: a
    [rows, >= max(lens)] fp32 buffer to write into (nothing past a row's length is touched).  All None: nothing is launched and
    ``wav[:, :max(lens)]`` is returned as it is."""
    from . import denoise as D

    global denoise_calls
    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "denoise")
    dns = D.per_row(params, rows, "params")
    cap = max(lens_h, default=0)
    _out_buffer(out, rows, cap, "denoise")
    if rows == 0 or all(d is None for d in dns):
        none = [None] * rows
        if out is None:
            return (wav[:, :cap], none) if report else wav[:, :cap]
        out[:, :cap].copy_(wav[:, :cap])  # (a caller that asked for its own buffer gets the rows there)
        return (out[:, :cap], none) if report else out[:, :cap]
    dev = wav.device
    if out is None:
        out = torch.empty(rows, max(1, cap), dtype=torch.float32, device=dev)
    lib = load()
    with torch.cuda.device(dev):
        ws_bytes = int(lib.sopro_denoise_workspace_bytes(rows, cap))
        if ws_bytes < 0:
            raise SoproHipError(f"denoise: {rows} rows of up to {cap} samples are outside the operator's range")
        ws = torch.empty(max(1, ws_bytes // 8), dtype=torch.int64, device=dev)
        rep = torch.empty(rows, 2, dtype=torch.float32, device=dev) if report else None
        lens_c = (C.c_int32 * rows)(*lens_h)
        par_c = (C.c_float * (2 * rows))(*[v for d in dns for v in ((d.atten_db, d.bias) if d is not None else (0.0, 0.0))])
        denoise_calls += 1
        _check(lib.sopro_denoise_rows_f32(ptr(wav) if cap > 0 else None, int(wav.stride(0)), lens_c, par_c, rows, ptr(out) if cap > 0 else None,
                                          int(out.stride(0)), ptr(rep), ws.data_ptr(), ws_bytes, _stream()), "sopro_denoise_rows_f32")
        if not report:
            return out[:, :cap]
        vals = rep.cpu().tolist()
    return out[:, :cap], [D.DenoiseReport(float(v[0]), float(v[1])) if d is not None else None for v, d in zip(vals, dns)]


# ---- reference crop selection (sopro_crop_*; definition in include/sopro_hip.h, numpy restatement in tests/crop_ref.py; parameters in crop.py) ----
CROP_H, CROP_SMOOTH, CROP_REPORT_WORDS = 240, 5, 8
crop_calls = 0  # calls of sopro_crop_rows_f32 by this process: the crop=None paths never add to it


def speech_crop(wav: torch.Tensor, lens, params, win: int, *, out: Optional[torch.Tensor] = None, report: bool = False, blocks: bool = False):
    """The window of ``win`` samples with the most speech and the least clipping of every row of a padded batch
    (sopro_crop_rows_f32): ``wav`` fp32 [rows, >= max(lens)] on the device (rows ``wav.stride(0)`` apart, any alignment), ``lens``
    valid samples per row, ``params`` one ``SpeechCrop`` or None, or one per row, ``win`` a positive multiple of 240 ->
    (out[:, :min(max(lens), win)], out_lens): row b holds ``wav[b, start : start + out_lens[b]]`` bit for bit, out_lens[b] =
    min(lens[b], win).  A row no longer than ``win`` comes back whole; a row whose ``SpeechCrop`` is None is not searched and comes
    back as its first out_lens[b] samples.  Three launches per 64 rows on the current stream and no synchronisation (the lengths and
    parameters are host values that travel as kernel arguments; the gather reads the chosen starts from device memory).
    ``report=True`` appends [CropReport or None per row], which costs one small host copy; ``blocks=True`` appends the per-block
    features [(e float32 [F], flags int32 [F]: bit 0 active, bit 1 clipped) or None per row], for tests.  ``out``: a [rows, >=
    min(max(lens), win)] fp32 buffer to write into, not overlapping ``wav`` (nothing past a row's out_lens is touched).  All None:
    nothing is launched and ``wav[:, :min(max(lens), win)]`` is returned as it is."""
    from . import crop as CR

    global crop_calls
    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "speech_crop")
    crs = CR.per_row(params, rows, "params")
    win = int(win)
    if win <= 0 or win % CROP_H:
        raise SoproHipError(f"speech_crop: win must be a positive multiple of {CROP_H}, got {win}")
    cap = max(lens_h, default=0)
    width = min(cap, win)
    out_lens = [min(n, win) for n in lens_h]
    _out_buffer(out, rows, width, "speech_crop")
    extra = ([[None] * rows] if report else []) + ([[None] * rows] if blocks else [])
    if rows == 0 or all(c is None for c in crs):
        if out is None:
            return (wav[:, :width], out_lens, *extra)
        out[:, :width].copy_(wav[:, :width])  # (a caller that asked for its own buffer gets the rows there)
        return (out[:, :width], out_lens, *extra)
    dev = wav.device
    if out is None:
        out = torch.empty(rows, max(1, width), dtype=torch.float32, device=dev)
    lib = load()
    with torch.cuda.device(dev):
        ws_bytes = int(lib.sopro_crop_workspace_bytes(rows, cap))
        if ws_bytes < 0:
            raise SoproHipError(f"speech_crop: {rows} rows of up to {cap} samples are outside the operator's range")
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.int32, device=dev)
        starts = torch.empty(rows, dtype=torch.int32, device=dev)
        rep = torch.empty(rows, CROP_REPORT_WORDS, dtype=torch.int32, device=dev) if report else None
        fc = cap // CROP_H
        blk = torch.zeros(rows, 2, max(1, fc), dtype=torch.int32, device=dev) if blocks else None
        lens_c = (C.c_int32 * rows)(*lens_h)
        par_c = (C.c_float * (4 * rows))(*[v for c in crs for v in ((c.range_db, c.margin_db, c.clip_level, float(c.clip_weight))
                                                                       if c is not None else (0.0, 0.0, 0.0, 0.0))])
        crop_calls += 1
        _check(lib.sopro_crop_rows_f32(ptr(wav) if cap > 0 else None, int(wav.stride(0)), lens_c, par_c, rows, win, ptr(out) if cap > 0 else None,
                                       int(out.stride(0)), ptr(starts, torch.int32), ptr(rep, torch.int32), ptr(blk, torch.int32), ws.data_ptr(),
                                       ws_bytes, _stream()), "sopro_crop_rows_f32")
        res = [out[:, :width], out_lens]
        if report:
            words = rep.cpu()
            level = words[:, CROP_REPORT_WORDS - 1].contiguous().view(torch.float32).tolist()
            res.append([CR.CropReport(*[int(v) for v in w[: CROP_REPORT_WORDS - 1]], float(lv)) if c is not None else None
                        for w, lv, c in zip(words.tolist(), level, crs)])
        if blocks:
            host, feats = blk.cpu(), []
            for b, (n, c) in enumerate(zip(lens_h, crs)):
                F = (n - (((n - win) // 2) % CROP_H if n > win else 0)) // CROP_H
                feats.append((host[b, 0, :F].contiguous().view(torch.float32).numpy().copy(), host[b, 1, :F].numpy().copy()) if c is not None else None)
            res.append(feats)
    return tuple(res)


# ---- pitch tracking (sopro_f0_*; definition in include/sopro_hip.h, numpy restatement in tests/f0_ref.py; parameters in f0.py) ----
F0_H, F0_W, F0_TMIN, F0_TMAX, F0_SPAN, F0_K, F0_PARAMS = 240, 720, 48, 400, 1120, 4, 6
f0_calls = 0  # calls of sopro_f0_rows_f32 / sopro_f0_paths by this process: nothing else in the engine adds to it


def _f0_params(params, rows: int):
    from . import f0 as F0

    ps = F0.per_row(params, rows, "params")
    return (C.c_float * (F0_PARAMS * rows))(*[v for p in ps for v in p.as_floats()])


def f0_track(wav: torch.Tensor, lens, params=None, *, debug: bool = False, f0: Optional[torch.Tensor] = None,
             strength: Optional[torch.Tensor] = None):
    """The fundamental frequency of every 10 ms frame of every row of a padded batch (sopro_f0_rows_f32): ``wav`` fp32 [rows, >=
    max(lens)] on the device at 24 kHz (rows ``wav.stride(0)`` apart, any alignment), ``lens`` valid samples per row, ``params`` one
    ``PitchParams`` or None (the defaults), or one per row -> (f0 fp32 [rows, fcap] in Hz with 0.0 = unvoiced, strength fp32 [rows,
    fcap], nvoiced int32 [rows], frames) with frames[b] = 0 for lens[b] < 1120, else (lens[b] - 1120) // 240 + 1 (a host list) and
    fcap = max(frames); all three tensors stay on the device, entries past a row's frames are not written (fresh buffers are zero,
    given ``f0=`` / ``strength=`` buffers keep what they held).  Three launches per 64 rows on the current stream and no
    synchronisation.  ``debug=True`` appends (v fp32 [rows, fcap, 401], e fp32 [rows, fcap], cands int32 [rows, fcap, 4]): the
    normalised difference, the window energies and the kept lags (0 = none), for tests."""
    from . import f0 as F0

    global f0_calls
    lens_h = _lens_list(lens)
    rows = len(lens_h)
    _check_rows(wav, lens_h, "f0_track")
    if rows == 0:
        raise SoproHipError("f0_track: at least one row")
    par_c = _f0_params(params, rows)
    cap = max(lens_h)
    frames = [F0.frames_of(n) for n in lens_h]
    fcap = max(frames)
    dev = wav.device
    _out_buffer(f0, rows, fcap, "f0_track")
    _out_buffer(strength, rows, fcap, "f0_track")
    lib = load()
    with torch.cuda.device(dev):
        ws_bytes = int(lib.sopro_f0_workspace_bytes(rows, cap))
        if ws_bytes < 0:
            raise SoproHipError(f"f0_track: {rows} rows of up to {cap} samples are outside the operator's range")
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.int32, device=dev)
        if f0 is None:
            f0 = torch.zeros(rows, max(1, fcap), dtype=torch.float32, device=dev)
        if strength is None:
            strength = torch.zeros(rows, max(1, fcap), dtype=torch.float32, device=dev)
        if rows > 1 and f0.stride(0) != strength.stride(0):
            raise SoproHipError("f0_track: f0 and strength must have the same row stride")
        nvoiced = torch.empty(rows, dtype=torch.int32, device=dev)
        dv = torch.zeros(rows, max(1, fcap), F0_TMAX + 1, dtype=torch.float32, device=dev) if debug else None
        de = torch.zeros(rows, max(1, fcap), dtype=torch.float32, device=dev) if debug else None
        dc = torch.zeros(rows, max(1, fcap), F0_K, dtype=torch.int32, device=dev) if debug else None
        lens_c = (C.c_int32 * rows)(*lens_h)
        f0_calls += 1
        _check(lib.sopro_f0_rows_f32(ptr(wav), int(wav.stride(0)), lens_c, par_c, rows, ptr(f0), ptr(strength), int(f0.stride(0)),
                                     ptr(nvoiced, torch.int32), ptr(dv), ptr(de), ptr(dc, torch.int32), ws.data_ptr(), ws_bytes, _stream()),
               "sopro_f0_rows_f32")
    res = (f0[:, :fcap], strength[:, :fcap], nvoiced, frames)
    return res + (dv[:, :fcap], de[:, :fcap], dc[:, :fcap]) if debug else res


def f0_paths(v: torch.Tensor, e: torch.Tensor, frames, params=None):
    """Candidates, path and output of the pitch tracker from a given normalised difference (sopro_f0_paths): ``v`` fp32 [rows, fcap,
    401] (finite, >= 0) and ``e`` fp32 [rows, fcap], contiguous and on the device, ``frames`` valid frames per row -> (f0 fp32 [rows,
    fcap], strength fp32 [rows, fcap], cands int32 [rows, fcap, 4]); entries past a row's frames are zero.  What ``f0_track`` does
    after its front end, for tests of that half.  Three launches per 64 rows on the current stream."""
    global f0_calls
    ptr(v)
    ptr(e)
    if v.dim() != 3 or int(v.shape[2]) != F0_TMAX + 1 or not v.is_contiguous() or tuple(e.shape) != tuple(v.shape[:2]) or not e.is_contiguous():
        raise SoproHipError(f"f0_paths: v must be a contiguous fp32 [rows, fcap, {F0_TMAX + 1}] and e a contiguous fp32 [rows, fcap]")
    rows, fcap = int(v.shape[0]), int(v.shape[1])
    fr_h = _lens_list(frames)
    if len(fr_h) != rows or (fr_h and (min(fr_h) < 0 or max(fr_h) > fcap)):
        raise SoproHipError(f"f0_paths: one frame count in [0, {fcap}] per row ({rows})")
    if rows == 0:
        raise SoproHipError("f0_paths: at least one row")
    par_c = _f0_params(params, rows)
    dev = v.device
    lib = load()
    with torch.cuda.device(dev):
        ws_bytes = int(lib.sopro_f0_workspace_bytes(rows, F0_SPAN + (fcap - 1) * F0_H if fcap > 0 else 0))
        if ws_bytes < 0:
            raise SoproHipError(f"f0_paths: {rows} rows of up to {fcap} frames are outside the operator's range")
        ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.int32, device=dev)
        f0 = torch.zeros(rows, max(1, fcap), dtype=torch.float32, device=dev)
        strength = torch.zeros(rows, max(1, fcap), dtype=torch.float32, device=dev)
        dc = torch.zeros(rows, max(1, fcap), F0_K, dtype=torch.int32, device=dev)
        fr_c = (C.c_int32 * rows)(*fr_h)
        f0_calls += 1
        _check(lib.sopro_f0_paths(ptr(v), ptr(e), fr_c, par_c, rows, fcap, ptr(f0), ptr(strength), int(f0.stride(0)), ptr(dc, torch.int32),
                                  ws.data_ptr(), ws_bytes, _stream()), "sopro_f0_paths")
    return f0[:, :fcap], strength[:, :fcap], dc[:, :fcap]


# ---- word timestamps (sopro_align_*; definition in include/sopro_hip.h, restatement in tests/align_ref.py) ----
ALIGN_S_MAX, ALIGN_DH = 2048, 96
ALIGN_STATE_WORDS, ALIGN_WINDOW_MAX = 5, 63  # SOPRO_ALIGN_STATE_WORDS / SOPRO_ALIGN_WINDOW_MAX
align_calls = 0  # launches of sopro_align_scores_f32 / sopro_align_dp_f32 / sopro_align_online_f32 by this process: a call that asks for no timing never adds to it


def _align_lens(tlens, slens, B: int, dev):
    """(tlens, slens) as int32 device vectors (host sequences are uploaded together)."""
    if isinstance(tlens, torch.Tensor) and isinstance(slens, torch.Tensor):
        return tlens.to(dev, torch.int32).contiguous(), slens.to(dev, torch.int32).contiguous()
    th = [int(v) for v in (tlens.tolist() if isinstance(tlens, torch.Tensor) else tlens)]
    sh = [int(v) for v in (slens.tolist() if isinstance(slens, torch.Tensor) else slens)]
    if len(th) != B or len(sh) != B:
        raise SoproHipError(f"one frame count and one text length per row ({B}), got {len(th)} and {len(sh)}")
    both = torch.tensor([th, sh], dtype=torch.int32).to(dev)
    return both[0], both[1]


def align_scores(Q: torch.Tensor, K: torch.Tensor, tlens, slens, acc: torch.Tensor, *, head_mask: int, weight: float, mode: int,
                 scale: Optional[float] = None, H: Optional[int] = None, ldq: Optional[int] = None, ldk: Optional[int] = None,
                 q_bstride: Optional[int] = None, k_bstride: Optional[int] = None, q_off: int = 0, k_off: int = 0) -> None:
    """One attention layer's share of the alignment scores (sopro_align_scores_f32): ``Q`` [B, T_cap, H * 96], ``K`` [B, S_cap, H * 96]
    (or wider rows through ``ldq`` / ``ldk`` and element offsets), ``acc`` fp32 [B, T_cap, >= S_cap] with contiguous rows.  ``mode`` 0
    writes the weighted sum of the heads in ``head_mask`` into ``acc``, 1 adds to it, 2 adds and finishes with log(max(acc, 1e-9))."""
    global align_calls
    ptr(acc)
    if acc.dim() != 3 or acc.stride(2) != 1:
        raise SoproHipError("align_scores: acc must be fp32 [B, T_cap, S_cap] with contiguous rows")
    B, T_cap, S_cap = (int(v) for v in acc.shape)
    H = int(H if H is not None else int(Q.shape[-1]) // ALIGN_DH)
    ldq = int(Q.stride(-2) if ldq is None else ldq)
    ldk = int(K.stride(-2) if ldk is None else ldk)
    q_bstride = int((Q.stride(0) if Q.dim() == 3 else T_cap * ldq) if q_bstride is None else q_bstride)
    k_bstride = int((K.stride(0) if K.dim() == 3 else S_cap * ldk) if k_bstride is None else k_bstride)
    tl, sl = _align_lens(tlens, slens, B, acc.device)
    align_calls += 1
    _check(load().sopro_align_scores_f32(ptr(Q) + 4 * q_off, ldq, q_bstride, ptr(K) + 4 * k_off, ldk, k_bstride, ptr(tl, torch.int32),
                                         ptr(sl, torch.int32), B, T_cap, S_cap, H, ALIGN_DH, float(scale if scale is not None else ALIGN_DH ** -0.5),
                                         int(head_mask), float(weight), int(mode), ptr(acc), int(acc.stride(1)), int(acc.stride(0)), _stream()),
           "sopro_align_scores_f32")


def align_paths(score: torch.Tensor, tlens, slens, *, path: Optional[torch.Tensor] = None, bounds: Optional[torch.Tensor] = None,
                total: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """The best monotonic path through each row's score matrix (sopro_align_dp_f32): ``score`` fp32 [B, T_cap, S_cap] on the device
    (rows ``score.stride(1)`` apart, any pitch), ``tlens`` / ``slens`` frames and text positions per row -> (path int32 [B, T_cap],
    bounds int32 [B, S_cap, 2] = (first frame, last frame + 1) per text position, total fp32 [B], status int32 [B]) on the device; entries
    past a row's lengths are not written (given buffers keep what they held, fresh ones are zero).  One launch on the current stream."""
    global align_calls
    ptr(score)
    if score.dim() != 3 or (int(score.shape[2]) > 1 and score.stride(2) != 1):
        raise SoproHipError("align_paths: score must be fp32 [B, T_cap, S_cap] with contiguous rows")
    B, T_cap, S_cap = (int(v) for v in score.shape)
    if S_cap > ALIGN_S_MAX:
        raise SoproHipError(f"align_paths: at most {ALIGN_S_MAX} text positions, got {S_cap}")
    dev = score.device
    lib = load()
    with torch.cuda.device(dev):
        tl, sl = _align_lens(tlens, slens, B, dev)
        path = torch.zeros(B, T_cap, dtype=torch.int32, device=dev) if path is None else path
        bounds = torch.zeros(B, S_cap, 2, dtype=torch.int32, device=dev) if bounds is None else bounds
        total = torch.zeros(B, dtype=torch.float32, device=dev) if total is None else total
        status = torch.zeros(B, dtype=torch.int32, device=dev) if status is None else status
        if tuple(path.shape) != (B, T_cap) or path.stride(1) != 1 or tuple(bounds.shape) != (B, S_cap, 2) or not bounds.is_contiguous():
            raise SoproHipError("align_paths: path must be int32 [B, T_cap] and bounds a contiguous int32 [B, S_cap, 2]")
        need = int(lib.sopro_align_ws_bytes(B, T_cap, S_cap))
        if ws is None:
            ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
        elif ws.numel() * ws.element_size() < need:
            raise SoproHipError(f"align_paths: the workspace holds {ws.numel() * ws.element_size()} bytes, {need} are needed")
        align_calls += 1
        _check(lib.sopro_align_dp_f32(ptr(score), int(score.stride(1)), int(score.stride(0)), ptr(tl, torch.int32), ptr(sl, torch.int32), B, T_cap,
                                      S_cap, ws.data_ptr(), int(ws.numel() * ws.element_size()), ptr(path, torch.int32), int(path.stride(0)),
                                      ptr(bounds, torch.int32), ptr(total), ptr(status, torch.int32), _stream()), "sopro_align_dp_f32")
    return path, bounds, total, status


def align_online_state(B: int, device) -> torch.Tensor:
    """A fresh online-aligner state: int32 [B, 5] = (c, p, status, e, base bits) = (-1, -1, 0, 0, 0.0f) per row."""
    st = torch.zeros(int(B), ALIGN_STATE_WORDS, dtype=torch.int32)
    st[:, :2] = -1
    return st.to(device)


def align_online(score, t1s, slens, finals, lag: int, state, path) -> None:
    """One step of the online path operator for every row (sopro_align_online_f32): ``score`` fp32 [B, T_cap, S_cap] on the device
    (rows ``score.stride(1)`` apart) holding frames [0, t1s[b]) of row b, ``slens`` text positions per row, ``finals`` nonzero for rows
    whose last frame is in, ``lag`` frames held back from the commit; ``state`` int32 [B, 5] (``align_online_state``) and ``path``
    int32 [B, >= T_cap] are updated in place: frames c + 1 .. u are committed (include/sopro_hip.h).  ``t1s`` / ``slens`` / ``finals``:
    int32 device vectors, or host sequences (uploaded together).  A row may step over at most 63 uncommitted frames (the committed
    frontier lives on the device, so a longer window shows as status 3 on a row that is otherwise left as it was; a caller stepping
    by k frames at lag L never exceeds k + L).  One launch on the current stream."""
    global align_calls
    lag = int(lag)
    if lag < 0:
        raise SoproHipError(f"align_online: lag must be >= 0, got {lag}")
    for name, v in (("score", score), ("state", state), ("path", path)):
        if not isinstance(v, torch.Tensor):
            raise SoproHipError(f"align_online: {name} must be a tensor on the device")
    ptr(score)
    ptr(state, torch.int32)
    ptr(path, torch.int32)
    if score.dim() != 3 or (int(score.shape[2]) > 1 and score.stride(2) != 1):
        raise SoproHipError("align_online: score must be fp32 [B, T_cap, S_cap] with contiguous rows")
    B, T_cap, S_cap = (int(v) for v in score.shape)
    if S_cap > ALIGN_S_MAX:
        raise SoproHipError(f"align_online: at most {ALIGN_S_MAX} text positions, got {S_cap}")
    if tuple(state.shape) != (B, ALIGN_STATE_WORDS) or not state.is_contiguous():
        raise SoproHipError(f"align_online: state must be a contiguous int32 [{B}, {ALIGN_STATE_WORDS}]")
    if path.dim() != 2 or int(path.shape[0]) != B or int(path.shape[1]) < T_cap or path.stride(1) != 1:
        raise SoproHipError(f"align_online: path must be int32 [{B}, >= {T_cap}] with contiguous rows")
    dev = score.device
    with torch.cuda.device(dev):
        if all(isinstance(v, torch.Tensor) for v in (t1s, slens, finals)):
            tl, sl, fl = (v.to(dev, torch.int32).contiguous() for v in (t1s, slens, finals))
        else:
            host = [[int(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)] for v in (t1s, slens, finals)]
            if any(len(h) != B for h in host):
                raise SoproHipError(f"align_online: one frame count, one text length and one final flag per row ({B})")
            all3 = torch.tensor(host, dtype=torch.int32).to(dev)
            tl, sl, fl = all3[0], all3[1], all3[2]
        if tl.numel() != B or sl.numel() != B or fl.numel() != B:
            raise SoproHipError(f"align_online: one frame count, one text length and one final flag per row ({B})")
        align_calls += 1
        _check(load().sopro_align_online_f32(ptr(score), int(score.stride(1)), int(score.stride(0)), ptr(tl, torch.int32), ptr(sl, torch.int32),
                                             ptr(fl, torch.int32), B, T_cap, S_cap, lag, ptr(state, torch.int32), ptr(path, torch.int32),
                                             int(path.stride(0)), _stream()), "sopro_align_online_f32")


def set_host_wait(blocking: bool, device=None) -> None:
    """How host threads wait for ``device`` (sopro_set_host_wait -> hipSetDeviceFlags): spin (the runtime's default: one busy core
    per waiting thread) or block on the completion interrupt.  Call it ONCE, AT PROCESS START, before any stream of the device
    exists (before the engine is built): the runtime creates a queue's completion signals for the wait mode in force when the
    queue is made, and a blocking wait on a signal made for spinning never wakes up - measured: hipHostFree hung in a
    process that switched modes after its streams existed (profiles/r04_experiments.md).  A process that runs lanes of a
    pipeline / a serving loop wants True (r04: 0.083 -> 0.040 CPU-s per 24 ms step at unchanged throughput)."""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        _check(load().sopro_set_host_wait(1 if blocking else 0), "sopro_set_host_wait")


def ar_tile_code(spec: str) -> int:
    """'2x1' -> (mt << 4) | nt of sopro_ar_frame.tile_*"""
    mt, nt = (int(v) for v in spec.lower().split("x"))
    if mt not in (1, 2) or nt not in (1, 2):
        raise ValueError(f"AR tile shape must be 1x1, 1x2, 2x1 or 2x2, got {spec!r}")
    return (mt << 4) | nt



def cond_prepare(engine, ws: torch.Tensor, ids: torch.Tensor, lens: torch.Tensor, ragged: bool, film_mul: torch.Tensor, film_add: torch.Tensor,
                 ref_k, ref_v, kv_bstride: int, kv_index: Optional[torch.Tensor], ref_klens: Optional[torch.Tensor], B: int, S: int, Tar: int,
                 Tr: int, txt_seq: torch.Tensor, txt_pool: torch.Tensor, cond_ar: torch.Tensor) -> None:
    """sopro_cond_prepare: the conditioning launch sequence of B utterances (csrc/stages.hip)."""
    ka = (C.c_void_p * len(ref_k))(*[ptr(t) for t in ref_k])
    va = (C.c_void_p * len(ref_v))(*[ptr(t) for t in ref_v])
    _check(load().sopro_cond_prepare(engine, ptr(ws), ptr(ids, torch.int32), ptr(lens, torch.int32), int(bool(ragged)), ptr(film_mul), ptr(film_add),
                                     ka, va, int(kv_bstride), ptr(kv_index, torch.int32), ptr(ref_klens, torch.int32), B, S, Tar, Tr,
                                     ptr(txt_seq), ptr(txt_pool), ptr(cond_ar), _stream()), "sopro_cond_prepare")


def film_coeffs(engine, sv: torch.Tensor, style: float, n: int, scratch: torch.Tensor, mul: torch.Tensor, add: torch.Tensor) -> None:
    _check(load().sopro_film_coeffs(engine, ptr(sv), float(style), n, ptr(scratch), ptr(mul), ptr(add), _stream()), "sopro_film_coeffs")


def ref_prepare(engine, ws: torch.Tensor, tokens: torch.Tensor, T: int, sv: torch.Tensor, ref_seq: torch.Tensor, kvs) -> None:
    """sopro_ref_prepare: Token2SV, reference encoder and the K | V rows of the reference cross-attention blocks of one voice."""
    if ref_seq is None:  # speaker vector only (SoproTTS.encode_speaker)
        _check(load().sopro_ref_prepare(engine, ptr(ws), ptr(tokens, torch.int32), T, ptr(sv), None, None, _stream()), "sopro_ref_prepare")
        return
    ka = (C.c_void_p * len(kvs))(*[ptr(t) for t in kvs])
    _check(load().sopro_ref_prepare(engine, ptr(ws), ptr(tokens, torch.int32), T, ptr(sv), ptr(ref_seq), ka, _stream()), "sopro_ref_prepare")


# ---- voice similarity (sopro_spk_*; definition in include/sopro_hip.h, numpy restatement in tests/spk_ref.py) ----
spk_calls = 0  # calls of sopro_spk_embed_rows / sopro_spk_cosine by this process: nothing else in the engine adds to it


def __getattr__(name: str):
    if name == "SPK_TILE_FRAMES":  # frames of one row per workgroup of the ragged Token2SV: the library's own constant
        return int(load().sopro_spk_tile_frames())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def spk_embed_rows(engine, tokens: torch.Tensor, lens, *, debug: bool = False, out: Optional[torch.Tensor] = None,
                   ws: Optional[torch.Tensor] = None):
    """The unit speaker vector of every row of a padded token batch (sopro_spk_embed_rows).  ``engine``: the model's
    ``stages.EngineHandle`` (``model.eng``), or its raw handle together with ``out=``.  ``tokens`` int32 [rows, t_cap, Q] on the
    device (frames contiguous, rows ``tokens.stride(0)`` apart, any alignment), ``lens`` valid frames per row - a host sequence
    (uploaded here) or an int32 device tensor (used where it is: nothing on the host waits) -> sv fp32 [rows, sv_student_dim] on the
    device.  Every row is Token2SV of its own ``tokens[b, :lens[b]]`` as an unpadded utterance; frames past ``lens[b]`` are never
    read and a row of length 0 gives a zero vector.  ``out``: fp32 [rows, >= sv_student_dim] with contiguous rows to write into
    (other entries keep what they held).  ``ws``: int32 scratch of at least ``sopro_spk_workspace_bytes`` (allocated otherwise).
    Two launches on the current stream and no synchronisation.  ``debug=True`` -> (sv, h fp32 [rows, t_cap, SD], logit fp32 [rows,
    t_cap]): the encoder output and the pooling logit, written for t < lens[b] only (zero elsewhere), for tests."""
    global spk_calls
    h = getattr(engine, "h", engine)
    ptr(tokens, torch.int32)
    if tokens.dim() != 3 or tokens.stride(2) != 1 or (int(tokens.shape[1]) > 1 and tokens.stride(1) != int(tokens.shape[2])):
        raise SoproHipError(f"spk_embed_rows wants tokens int32 [rows, t_cap, Q] with contiguous frames, got {tuple(tokens.shape)} strides {tokens.stride()}")
    rows, t_cap = int(tokens.shape[0]), int(tokens.shape[1])
    dev = tokens.device
    if isinstance(lens, torch.Tensor) and lens.is_cuda:
        if lens.dtype != torch.int32 or lens.dim() != 1 or int(lens.numel()) != rows or not lens.is_contiguous():
            raise SoproHipError("spk_embed_rows: device lens must be a contiguous int32 vector with one entry per row")
        lens_d = lens
    else:
        lens_h = _lens_list(lens)
        if len(lens_h) != rows or (lens_h and (min(lens_h) < 0 or max(lens_h) > t_cap)):
            raise SoproHipError(f"spk_embed_rows: one length in [0, {t_cap}] per row ({rows}), got {lens_h}")
        lens_d = None
    if rows == 0 or t_cap == 0:
        raise SoproHipError("spk_embed_rows: at least one row and one frame of capacity")
    lib = load()
    with torch.cuda.device(dev):
        if lens_d is None:
            lens_d = torch.tensor(lens_h, dtype=torch.int32).to(dev, non_blocking=True)
        ws_bytes = int(lib.sopro_spk_workspace_bytes(h, rows, t_cap))
        if ws_bytes <= 0:
            raise SoproHipError("spk_embed_rows: the engine holds no Token2SV tensors")
        if ws is None:
            ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        elif ws.dtype != torch.int32 or not ws.is_cuda or ws.numel() * 4 < ws_bytes:
            raise SoproHipError(f"spk_embed_rows: ws must be int32 on the device with at least {ws_bytes} bytes")
        # the width of the speaker vector and of the encoder: the engine's own (a wrong guess here would be refused by the library)
        svd = int(engine.sv_dim) if getattr(engine, "sv_dim", None) else None
        if out is None:
            if svd is None:
                raise SoproHipError("spk_embed_rows: pass out= (the engine handle does not say how wide a speaker vector is)")
            out = torch.zeros(rows, svd, dtype=torch.float32, device=dev)
        else:
            ptr(out)
            if out.dim() != 2 or int(out.shape[0]) != rows or (int(out.shape[1]) > 1 and out.stride(1) != 1) or (svd is not None and int(out.shape[1]) < svd):
                raise SoproHipError(f"spk_embed_rows: out must be fp32 [rows, >= sv_student_dim] with contiguous rows, got {tuple(out.shape)}")
        dh = dl = None
        if debug:
            if not getattr(engine, "spk_width", None):
                raise SoproHipError("spk_embed_rows(debug=True) wants the EngineHandle (it knows the encoder's width)")
            sd = int(engine.spk_width)
            dh = torch.zeros(rows, t_cap, sd, dtype=torch.float32, device=dev)
            dl = torch.zeros(rows, t_cap, dtype=torch.float32, device=dev)
        spk_calls += 1
        _check(lib.sopro_spk_embed_rows(h, ws.data_ptr(), tokens.data_ptr(), int(tokens.stride(0)), lens_d.data_ptr(), rows, t_cap, ptr(out),
                                        int(out.stride(0)), ptr(dh), ptr(dl), _stream()), "sopro_spk_embed_rows")
    sv = out if svd is None else out[:, :svd]
    return (sv, dh, dl) if debug else sv


def spk_cosine(a: torch.Tensor, b: torch.Tensor, *, bank: bool = False) -> torch.Tensor:
    """Cosine of speaker vectors (sopro_spk_cosine): ``a`` fp32 [na, dim], ``b`` fp32 [nb, dim] on the device with contiguous rows ->
    fp32 [na] with a[i] . b[i] / max(|a[i]| |b[i]|, 1e-12) (``na == nb``), or with ``bank=True`` fp32 [na, nb] of every a[i] against
    every b[n].  The norms are recomputed, so the vectors need not be unit; a zero vector gives 0.0.  One launch on the current
    stream and no synchronisation."""
    global spk_calls
    ptr(a)
    ptr(b)
    for t, nm in ((a, "a"), (b, "b")):
        if t.dim() != 2 or int(t.shape[0]) < 1 or int(t.shape[1]) < 1 or (int(t.shape[1]) > 1 and t.stride(1) != 1):
            raise SoproHipError(f"spk_cosine: {nm} must be fp32 [n >= 1, dim >= 1] with contiguous rows, got {tuple(t.shape)}")
    na, nb, dim = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    if int(b.shape[1]) != dim or a.device != b.device:
        raise SoproHipError(f"spk_cosine: a and b must have the same width and device, got {tuple(a.shape)} and {tuple(b.shape)}")
    if not bank and na != nb:
        raise SoproHipError(f"spk_cosine: pairwise mode wants as many rows in a as in b, got {na} and {nb} (bank=True compares every pair)")
    with torch.cuda.device(a.device):
        out = torch.empty((na, nb) if bank else (na,), dtype=torch.float32, device=a.device)
        spk_calls += 1
        _check(load().sopro_spk_cosine(ptr(a), int(a.stride(0)) if na > 1 else dim, na, ptr(b), int(b.stride(0)) if nb > 1 else dim, nb, dim,
                                       1 if bank else 0, ptr(out), _stream()), "sopro_spk_cosine")
    return out

class Graph:
    """A recorded launch sequence (hipGraphExec) replayable on any stream."""

    def __init__(self, handle: int, family: str = "ar_step_graph"):
        self.handle = handle
        self.family = family

    def launch(self) -> None:
        e0 = _prof.begin() if _prof is not None else None
        _check(load().sopro_graph_launch(self.handle, _stream()), "sopro_graph_launch")
        if e0 is not None:
            _prof.end(self.family, 0.0, e0)

    def launch_n(self, n: int) -> None:
        """n replays back to back (one call: the interpreter lock is dropped once for all of them)."""
        if _prof is not None:
            for _ in range(int(n)):
                self.launch()
            return
        _check(load().sopro_graph_launch_n(self.handle, _stream(), int(n)), "sopro_graph_launch_n")

    def __del__(self):
        # Never destroy here: the collector may run this INSIDE another recording (any allocation can trigger it), and
        # hipGraphExecDestroy during a stream capture invalidates that capture ("operation failed due to a previous error
        # during capture", seen once in a few suite runs).  The handle is parked and destroyed at the next safe point.
        if self.handle and _dead_graphs is not None:  # (None: module globals already torn down at interpreter exit)
            _dead_graphs.append(self.handle)
            self.handle = 0


_dead_graphs: list = []


def reap_graphs() -> None:
    """Destroy the graphs whose owners are gone; called where no recording can be open (capture_begin takes the lock first)."""
    while _dead_graphs:
        h = _dead_graphs.pop()
        try:
            if _lib is not None:
                _lib.sopro_graph_destroy(h)
        except Exception:
            pass


def profiling() -> bool:
    """True while bench.py's per-launch event timing is attached (recorded graphs would hide the launches from it)."""
    return _prof is not None


class GraphCache:
    """Recorded launch sequences keyed by problem shape, for host code whose launches depend only on that shape.
    A shape is run eagerly the first time (scratch buffers get allocated), recorded the second time, replayed after."""

    def __init__(self, family: str, cap: int = 8):
        self.family, self.cap = family, cap
        self.graphs: dict = {}
        self.seen: dict = {}

    def run(self, key, issue) -> None:
        """``issue()`` enqueues the launches on the current stream; it must not allocate, synchronise or touch the host."""
        if profiling():  # per-launch event timing wants to see the launches one by one
            issue()
            return
        g = self.graphs.get(key)
        if g is not None:
            g.launch()
            return
        n = self.seen.get(key, 0)
        if n == 0 and len(self.seen) >= 8 * max(8, self.cap):  # keys may hold caller pointers (temporary tensors): keep the census bounded
            self.seen.pop(next(iter(self.seen)))
        self.seen[key] = n + 1
        if n == 0:
            issue()
            return
        capture_begin()
        try:
            issue()
        finally:
            g = capture_end()
        g.family = self.family
        if len(self.graphs) >= self.cap:
            self.graphs.pop(next(iter(self.graphs)))
        self.graphs[key] = g
        g.launch()

    def clear(self) -> None:
        self.graphs.clear()
        self.seen.clear()
        reap_parked_graphs()  # the handles were only parked by Graph.__del__: destroy them now if no recording is open


# A recording is thread-local (hipStreamCaptureModeThreadLocal), but the runtime still refused a pinned-host allocation made
# by ANOTHER thread while one was open ("operation not permitted when stream is capturing", once in a few hundred pipelined
# runs, when one lane recorded its launch sequence while another made its first poll buffer).  Recordings and pinned
# allocations are rare and short: they take turns.
_capture_lock = threading.RLock()


def reap_parked_graphs() -> bool:
    """Destroy the parked graph handles NOW if no recording is open in any thread (a warmed-up server may never record again,
    and the handles keep their workspaces' launch descriptors alive: ADVICE r3).  Non-blocking: returns False, leaving them for
    the next capture_begin, when another thread holds the recording lock."""
    if not _dead_graphs:
        return True
    if not _capture_lock.acquire(blocking=False):
        return False
    try:
        if getattr(_capture_depth, "n", 0) == 0:  # (the lock is re-entrant: not inside THIS thread's own recording either)
            reap_graphs()
            return True
        return False
    finally:
        _capture_lock.release()


_capture_depth = threading.local()


_gc_paused = [0, False]  # (open recordings, was the collector enabled) - guarded by _capture_lock


def _gc_pause() -> None:
    """No cyclic garbage collection while a launch sequence is being recorded: a collection runs finalizers of WHATEVER became garbage
    in the process - an engine of an earlier module (sopro_engine_destroy: hipFree), page-locked blocks, torch storages - on the thread
    that happens to allocate next, and a free on the recording thread invalidates the recording ("operation failed due to a previous
    error during capture", seen once in ~20 suite runs, at the first launch of an AR frame recording)."""
    if _gc_paused[0] == 0:
        _gc_paused[1] = gc.isenabled()
        gc.disable()
    _gc_paused[0] += 1


def _gc_resume() -> None:
    _gc_paused[0] = max(0, _gc_paused[0] - 1)
    if _gc_paused[0] == 0 and _gc_paused[1]:
        gc.enable()


def capture_begin() -> None:
    _capture_lock.acquire()
    try:
        if getattr(_capture_depth, "n", 0) == 0:
            reap_graphs()
        _gc_pause()
        try:
            _check(load().sopro_capture_begin(_stream()), "sopro_capture_begin")
        except BaseException:
            _gc_resume()
            raise
        _capture_depth.n = getattr(_capture_depth, "n", 0) + 1
    except BaseException:
        _capture_lock.release()
        raise


def capture_end() -> Graph:
    out = _p()
    try:
        _check(load().sopro_capture_end(_stream(), C.byref(out)), "sopro_capture_end")
    finally:
        _capture_depth.n = max(0, getattr(_capture_depth, "n", 0) - 1)
        _gc_resume()
        _capture_lock.release()
    return Graph(out.value)


class HostMirror:
    """``n`` int32 of page-locked host memory that a host loop polls: ``copy_from(t)`` queues the device -> host copy behind
    the launches issued so far on the current stream (record an event after it and wait for that event before reading
    ``values()``).  Outside torch's pinned-memory cache on purpose (see sopro_host_alloc)."""

    def __init__(self, n: int):
        self.n = int(n)
        out = _p()
        with _capture_lock:  # no page-locked allocation while another thread records a launch sequence
            _check(load().sopro_host_alloc(4 * self.n, C.byref(out)), "sopro_host_alloc")
        self.ptr = out.value
        self._view = (C.c_int32 * self.n).from_address(self.ptr)
        self._keep = None

    def copy_from(self, t: torch.Tensor) -> None:
        """Queue device -> host behind the current stream's launches.  A KERNEL of the library writes the page-locked words
        (sopro_copy2d_u32): the timed path holds no runtime copy - no `__amd_rocclr_copyBuffer`, no DMA packet - at all (round 5)."""
        if t.dtype not in (torch.int32, torch.float32) or not t.is_contiguous() or t.numel() != self.n or not t.is_cuda:
            raise SoproHipError(f"HostMirror.copy_from: expected a contiguous device int32 / float32 tensor of {self.n} elements")
        self._keep = t  # the source of a queued copy stays alive
        _check(load().sopro_copy2d_u32(self.ptr, self.n, t.data_ptr(), self.n, 1, self.n, _stream()), "sopro_copy2d_u32")

    def copy_to(self, t: torch.Tensor) -> None:
        """Queue host -> device: the kernel reads the page-locked words when it RUNS, so the host must leave them alone until the
        stream has passed this point (the users write a block, queue the launches that read it and synchronise before the next write)."""
        m = t.numel()  # (a block may be larger than what this call sends: the first m words go)
        if t.dtype not in (torch.int32, torch.float32) or not t.is_contiguous() or not (0 < m <= self.n) or not t.is_cuda or not self.ptr:
            raise SoproHipError(f"HostMirror.copy_to: expected a contiguous device int32 / float32 tensor of at most {self.n} elements")
        _check(load().sopro_copy2d_u32(t.data_ptr(), m, self.ptr, m, 1, m, _stream()), "sopro_copy2d_u32")

    def values(self) -> list:
        return list(self._view)

    def array(self):
        """The words as a writable numpy int32 view (``.view(np.float32)`` for float parameters)."""
        import numpy as np

        return np.ctypeslib.as_array(self._view)

    def free(self) -> None:
        """Give the page-locked words back NOW.  The caller has made sure no queued kernel and no recorded launch sequence still
        holds the address.  Under the recording lock, like the allocation: the runtime refuses page-locked (de)allocations made
        while another thread records."""
        p, self.ptr = getattr(self, "ptr", None), None
        if p and _lib is not None:
            self._view = None
            with _capture_lock:
                _lib.sopro_host_free(p)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def cu_range_stream(first_cu: int, n_cus: int, device: Optional[torch.device] = None) -> "torch.cuda.Stream":
    """A torch-visible stream whose kernels are confined to CUs [first_cu, first_cu + n_cus).
    The owner must hand it back with ``destroy_stream`` (torch does not own external streams)."""
    out = _p()
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):  # the C side creates it on the current device
        _check(load().sopro_stream_create_cu_range(first_cu, n_cus, C.byref(out)), "sopro_stream_create_cu_range")
    return torch.cuda.ExternalStream(out.value, device=device)


def cu_mask_stream(cus, device: Optional[torch.device] = None) -> "torch.cuda.Stream":
    """A torch-visible stream confined to the CUs whose mask bits are in ``cus`` (see sopro_stream_create_cu_mask for what
    the bits mean on gfx950).  Hand it back with ``destroy_stream``."""
    cus = sorted(set(int(c) for c in cus))
    words = (max(cus) >> 5) + 1
    arr = (C.c_uint32 * words)()
    for c in cus:
        arr[c >> 5] |= 1 << (c & 31)
    out = _p()
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        _check(load().sopro_stream_create_cu_mask(arr, words, C.byref(out)), "sopro_stream_create_cu_mask")
    return torch.cuda.ExternalStream(out.value, device=device)


def destroy_stream(s: "torch.cuda.Stream") -> None:
    _splitk_pool.pop(s.cuda_stream, None)
    _check(load().sopro_stream_destroy(s.cuda_stream), "sopro_stream_destroy")


def device_info(device: int = 0) -> dict:
    arr = (C.c_int * 4)()
    _check(load().sopro_device_info(device, arr), "sopro_device_info")
    return {"cus": arr[0], "lds_per_block": arr[1], "clock_khz": arr[2], "gfx": arr[3]}
