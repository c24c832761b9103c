"""ctypes view of the C ABI declared in include/svdq_amd.h (struct layouts must match it)."""

import ctypes as C
import os

# torch must initialise ITS bundled HIP runtime first: libsvdq_amd.so then binds to the already
# loaded libamdhip64 (same soname) instead of pulling a second runtime from /opt/rocm, which on a
# GPU box ends in "no ROCm-capable device is detected" for our launches.
import torch  # noqa: F401

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libsvdq_amd.so")

SVDQ_BF16, SVDQ_FP16 = 0, 1
FUSE_NONE, FUSE_SILU, FUSE_GELU_QUANT, FUSE_RMSNORM_ROPE = 0, 1, 2, 3
ABI_VERSION = 24
LORA_ACT_F32, LORA_ACT_Q32, LORA_ACT_Q32_RUNS = 0, 1, 2


class QuantizeArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("smooth", C.c_void_p), ("lora_down", C.c_void_p),
        ("act", C.c_void_p), ("ascales", C.c_void_p), ("lora_act", C.c_void_p),
        ("M", C.c_int32), ("M_pad", C.c_int32), ("K", C.c_int32), ("R", C.c_int32),
        ("ldx", C.c_int32), ("dtype", C.c_int32), ("fuse_glu", C.c_int32), ("fp4", C.c_int32),
        ("ln_stats", C.c_void_p), ("mod_scale", C.c_void_p), ("mod_shift", C.c_void_p),
        ("x2", C.c_void_p), ("smooth2", C.c_void_p), ("lora_down2", C.c_void_p), ("mod_scale2", C.c_void_p),
        ("mod_shift2", C.c_void_p), ("ln_stats2", C.c_void_p), ("M2", C.c_int32), ("ldx2", C.c_int32),
        ("split_rows", C.c_int32), ("lora_act_zeroed", C.c_int32), ("lora_act_format", C.c_int32), ("reserved", C.c_int32),
    ]


class ResidualArgs(C.Structure):
    _fields_ = [
        ("res", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p), ("gate", C.c_void_p), ("out", C.c_void_p),
        ("stats", C.c_void_p), ("M", C.c_int32), ("C", C.c_int32), ("ld", C.c_int32), ("dtype", C.c_int32),
        ("eps", C.c_float), ("clamp_fp16", C.c_int32), ("zero_ptr", C.c_void_p), ("zero_bytes", C.c_int64),
        ("res2", C.c_void_p), ("a2", C.c_void_p), ("b2", C.c_void_p), ("gate2", C.c_void_p), ("out2", C.c_void_p),
        ("stats2", C.c_void_p), ("M2", C.c_int32), ("reserved2", C.c_int32),
    ]


class ResidualDiffResult(C.Structure):
    _fields_ = [
        ("sum_diff", C.c_float), ("sum_prev", C.c_float), ("mean_diff", C.c_float), ("mean_prev", C.c_float),
        ("ratio", C.c_float), ("rows", C.c_int32), ("reserved", C.c_int32 * 2),
    ]


class ResidualDiffArgs(C.Structure):
    _fields_ = [
        ("cur", C.c_void_p), ("base", C.c_void_p), ("prev", C.c_void_p), ("out_res", C.c_void_p),
        ("cur2", C.c_void_p), ("base2", C.c_void_p), ("prev2", C.c_void_p), ("out_res2", C.c_void_p),
        ("partials", C.c_void_p), ("result", C.c_void_p),
        ("M", C.c_int32), ("M2", C.c_int32), ("C", C.c_int32), ("ld", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


class ModulatedDiffArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("stats", C.c_void_p), ("mod_scale", C.c_void_p), ("mod_shift", C.c_void_p),
        ("prev", C.c_void_p), ("out_mod", C.c_void_p), ("partials", C.c_void_p), ("result", C.c_void_p),
        ("M", C.c_int32), ("C", C.c_int32), ("ld", C.c_int32), ("dtype", C.c_int32),
    ]


class IpAttentionArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
        ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32),
        ("T", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("head_dim", C.c_int32),
        ("dtype", C.c_int32), ("q_prescaled", C.c_int32), ("scale", C.c_float), ("out_scale", C.c_float),
    ]


class LinearAttentionArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("kv", C.c_void_p), ("out", C.c_void_p), ("vk", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("q_bs", C.c_int64), ("kv_bs", C.c_int64), ("out_bs", C.c_int64),
        ("ldq", C.c_int32), ("ldkv", C.c_int32), ("ldo", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("head_dim", C.c_int32),
        ("dtype", C.c_int32), ("eps", C.c_float), ("reserved", C.c_int32),
    ]


class Dwconv3x3Args(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("weight", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("x_bs", C.c_int64), ("out_bs", C.c_int64),
        ("ldx", C.c_int32), ("ldo", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("dtype", C.c_int32), ("reserved", C.c_int32),
    ]


class GemmArgs(C.Structure):
    _fields_ = [
        ("act", C.c_void_p), ("wgt", C.c_void_p), ("ascales", C.c_void_p), ("wscales", C.c_void_p),
        ("bias", C.c_void_p), ("lora_act_in", C.c_void_p), ("lora_up", C.c_void_p),
        ("lora_scales", C.POINTER(C.c_float)), ("out", C.c_void_p),
        ("qout", C.c_void_p), ("oscales", C.c_void_p), ("next_smooth", C.c_void_p),
        ("next_lora_down", C.c_void_p), ("lora_act_out", C.c_void_p),
        ("norm_q", C.c_void_p), ("norm_k", C.c_void_p), ("rotary_emb", C.c_void_p),
        ("M", C.c_int32), ("M_pad", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("R", C.c_int32), ("R2", C.c_int32), ("ldo", C.c_int32), ("dtype", C.c_int32),
        ("act_unsigned", C.c_int32), ("fuse", C.c_int32), ("variant", C.c_int32), ("reserved", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("out_vt", C.c_void_p), ("ldvt", C.c_int32), ("geometry", C.c_int32),
        ("wgt2", C.c_void_p), ("wscales2", C.c_void_p), ("bias2", C.c_void_p), ("lora_up2", C.c_void_p),
        ("next_smooth2", C.c_void_p), ("next_lora_down2", C.c_void_p), ("norm_q2", C.c_void_p), ("norm_k2", C.c_void_p),
        ("split_rows", C.c_int32), ("lora_act_format", C.c_int32), ("status", C.c_void_p),
        ("q_scale", C.c_float), ("reserved2", C.c_int32),
        ("next_lora_down_packed", C.c_void_p), ("next_lora_down_packed2", C.c_void_p), ("lora_up_packed", C.c_void_p),
    ]


class AttentionArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("vt", C.c_void_p), ("out", C.c_void_p),
        ("q_hs", C.c_int64), ("k_hs", C.c_int64), ("vt_hs", C.c_int64), ("o_hs", C.c_int64),
        ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldvt", C.c_int32), ("ldo", C.c_int32),
        ("L", C.c_int32), ("H", C.c_int32), ("head_dim", C.c_int32), ("dtype", C.c_int32),
        ("scale", C.c_float), ("reserved", C.c_int32), ("zero_ptr", C.c_void_p), ("zero_bytes", C.c_int64),
        ("qact", C.c_void_p), ("qscales", C.c_void_p), ("qlora_act", C.c_void_p), ("qsmooth", C.c_void_p),
        ("qlora_down", C.c_void_p), ("qsmooth2", C.c_void_p), ("qlora_down2", C.c_void_p), ("qR", C.c_int32),
        ("qsplit_rows", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("qlora_act_format", C.c_int32), ("q_prescaled", C.c_int32), ("status", C.c_void_p),
        ("kv_len0", C.c_int32), ("kv_start1", C.c_int32), ("kv_end1", C.c_int32), ("geometry", C.c_int32),
        ("qlora_down_packed", C.c_void_p), ("qlora_down_packed2", C.c_void_p),
    ]


class GemvAwqArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("qweight", C.c_void_p), ("scales", C.c_void_p), ("zeros", C.c_void_p),
        ("bias", C.c_void_p), ("out", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("ldx", C.c_int32),
        ("group_size", C.c_int32), ("dtype", C.c_int32), ("out_chunks", C.c_int32), ("reserved", C.c_int32),
    ]


class GemvLoraArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("down", C.c_void_p), ("up", C.c_void_p), ("out", C.c_void_p), ("t", C.c_void_p),
        ("strength", C.c_float), ("r", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("dtype", C.c_int32), ("out_chunks", C.c_int32), ("reserved", C.c_int32 * 2),
    ]


class GemmAwqArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("qweight", C.c_void_p), ("scales", C.c_void_p), ("scaled_zeros", C.c_void_p),
        ("bias", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("ldx", C.c_int32),
        ("group_size", C.c_int32), ("dtype", C.c_int32),
    ]


class CrossAttentionArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
        ("key_offsets", C.c_void_p), ("key_counts", C.c_void_p),
        ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("head_dim", C.c_int32),
        ("Nrows", C.c_int32), ("max_keys", C.c_int32),
        ("dtype", C.c_int32), ("scale", C.c_float),
    ]


class AttentionD64Args(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
        ("q_bs", C.c_int64), ("k_bs", C.c_int64), ("v_bs", C.c_int64), ("out_bs", C.c_int64),
        ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("N", C.c_int32),
        ("head_dim", C.c_int32), ("dtype", C.c_int32), ("scale", C.c_float), ("reserved", C.c_int32),
    ]


class SanaGlueArgs(C.Structure):
    _fields_ = [
        ("res", C.c_void_p), ("a", C.c_void_p), ("timestep", C.c_void_p), ("gate_table", C.c_void_p), ("mod_table", C.c_void_p),
        ("out", C.c_void_p), ("out_mod", C.c_void_p), ("stats", C.c_void_p),
        ("timestep_bs", C.c_int64),
        ("ld_res", C.c_int32), ("ld_a", C.c_int32), ("ld_out", C.c_int32), ("ld_mod", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("C_pad", C.c_int32),
        ("gate_row", C.c_int32), ("scale_row", C.c_int32), ("shift_row", C.c_int32),
        ("dtype", C.c_int32), ("eps", C.c_float), ("reserved", C.c_int32),
    ]


class SandwichNormArgs(C.Structure):
    _fields_ = [
        ("res", C.c_void_p), ("a", C.c_void_p), ("w_post", C.c_void_p), ("gate", C.c_void_p), ("w_pre", C.c_void_p), ("scale", C.c_void_p),
        ("out", C.c_void_p), ("out_mod", C.c_void_p), ("stats", C.c_void_p),
        ("gate_bs", C.c_int64), ("scale_bs", C.c_int64),
        ("ld_res", C.c_int32), ("ld_a", C.c_int32), ("ld_out", C.c_int32), ("ld_mod", C.c_int32),
        ("M", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("dtype", C.c_int32),
        ("eps", C.c_float), ("reserved", C.c_int32),
    ]


class QkNormRopeArgs(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("norm_q", C.c_void_p), ("norm_k", C.c_void_p), ("freqs", C.c_void_p), ("vt", C.c_void_p), ("rstd", C.c_void_p),
        ("ld", C.c_int32), ("ldvt", C.c_int32),
        ("T", C.c_int32), ("L_pad", C.c_int32), ("H", C.c_int32), ("head_dim", C.c_int32),
        ("dtype", C.c_int32), ("eps", C.c_float),
    ]


QWEN_ROTARY_MAX_GRIDS, QWEN_ROTARY_POSITIONS = 8, 4096


class QwenRotaryArgs(C.Structure):
    _fields_ = [
        ("pos_cs", C.c_void_p), ("neg_cs", C.c_void_p),
        ("img", C.c_void_p), ("txt", C.c_void_p), ("all", C.c_void_p), ("img_cs", C.c_void_p), ("txt_cs", C.c_void_p),
        ("grids", C.c_int32 * (3 * QWEN_ROTARY_MAX_GRIDS)),
        ("count", C.c_int32), ("txt_len", C.c_int32), ("txt_start", C.c_int32), ("scale_rope", C.c_int32),
        ("c_frame", C.c_int32), ("c_height", C.c_int32),
    ]


class PulidCaArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("stats", C.c_void_p), ("a_fold", C.c_void_p), ("colsum", C.c_void_p), ("cbias", C.c_void_p),
        ("b_fold", C.c_void_p), ("probs", C.c_void_p), ("out", C.c_void_p), ("acc", C.c_void_p), ("o_acc", C.c_void_p),
        ("ldx", C.c_int32), ("ldo", C.c_int32),
        ("T", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("N", C.c_int32),
        ("dtype", C.c_int32), ("out_scale", C.c_float),
    ]


EXPORTS = {
    "svdq_quantize_w4a4_act_fuse_lora": (C.c_int, [C.POINTER(QuantizeArgs), C.c_void_p]),
    "svdq_quantize_plan": (C.c_int, [C.POINTER(QuantizeArgs), C.POINTER(C.c_int32)]),
    "svdq_gemm_w4a4": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p]),
    "svdq_attention": (C.c_int, [C.POINTER(AttentionArgs), C.c_void_p]),
    "svdq_gemv_awq": (C.c_int, [C.POINTER(GemvAwqArgs), C.c_void_p]),
    "svdq_gemv_awq_batched": (C.c_int, [C.POINTER(GemvAwqArgs), C.c_int32, C.c_void_p]),
    "svdq_gemv_awq_lora_batched": (C.c_int, [C.POINTER(GemvLoraArgs), C.c_int32, C.c_void_p]),
    "svdq_gemm_awq": (C.c_int, [C.POINTER(GemmAwqArgs), C.c_void_p]),
    "svdq_gemm_awq_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "svdq_residual_gate_stats": (C.c_int, [C.POINTER(ResidualArgs), C.c_void_p]),
    "svdq_residual_diff": (C.c_int, [C.POINTER(ResidualDiffArgs), C.c_void_p]),
    "svdq_modulated_diff": (C.c_int, [C.POINTER(ModulatedDiffArgs), C.c_void_p]),
    "svdq_ip_attention": (C.c_int, [C.POINTER(IpAttentionArgs), C.c_void_p]),
    "svdq_linear_attention": (C.c_int, [C.POINTER(LinearAttentionArgs), C.c_void_p]),
    "svdq_linear_attention_workspace_bytes": (C.c_int64, [C.POINTER(LinearAttentionArgs)]),
    "svdq_dwconv3x3": (C.c_int, [C.POINTER(Dwconv3x3Args), C.c_void_p]),
    "svdq_cross_attention": (C.c_int, [C.POINTER(CrossAttentionArgs), C.c_void_p]),
    "svdq_sana_glue": (C.c_int, [C.POINTER(SanaGlueArgs), C.c_void_p]),
    "svdq_attention_d64": (C.c_int, [C.POINTER(AttentionD64Args), C.c_void_p]),
    "svdq_sandwich_norm": (C.c_int, [C.POINTER(SandwichNormArgs), C.c_void_p]),
    "svdq_qk_norm_rope": (C.c_int, [C.POINTER(QkNormRopeArgs), C.c_void_p]),
    "svdq_pulid_ca": (C.c_int, [C.POINTER(PulidCaArgs), C.c_void_p]),
    "svdq_qwen_rotary": (C.c_int, [C.POINTER(QwenRotaryArgs), C.c_void_p]),
    "svdq_gemm_workspace_bytes": (C.c_int64, []),
    "svdq_gemm_workspace_bytes_for": (C.c_int64, [C.POINTER(GemmArgs)]),
    "svdq_gemm_workspace_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "svdq_gemm_last_plan": (C.c_int, [C.POINTER(C.c_int32)]),
    "svdq_gemm_plan": (C.c_int, [C.POINTER(GemmArgs), C.c_int32, C.POINTER(C.c_int32)]),
    "svdq_attention_workspace_bytes": (C.c_int64, []),
    "svdq_attention_workspace_bytes_for": (C.c_int64, [C.POINTER(AttentionArgs)]),
    "svdq_attention_workspace_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "svdq_attention_schedule": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "svdq_attention_plan": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "svdq_attention_last_plan": (C.c_int, [C.POINTER(C.c_int32)]),
    "svdq_gemm_schedule": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "svdq_gemm_schedule_ex": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "svdq_repack_qweight": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_repack_wscales": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_repack_vec": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "svdq_repack_lowrank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_unrepack_qweight": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_unrepack_wscales": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_unrepack_vec": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "svdq_unrepack_lowrank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_unpack_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_unpack_scales": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_pack_lora_down_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "svdq_pack_lora_down": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_pack_lora_up_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "svdq_pack_lora_up": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "svdq_prof_enable": (C.c_int, [C.c_int32]),
    "svdq_prof_reset": (C.c_int, []),
    "svdq_prof_select": (C.c_int, [C.c_uint32]),
    "svdq_prof_read": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "svdq_last_error": (C.c_char_p, []),
    "svdq_abi_version": (C.c_int, []),
}

_lib = None


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load libsvdq_amd.so.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} is missing: build it with `python -m nunchaku_amd.build` "
            "(or __graft_entry__.build()).  nunchaku_amd has no CPU/PyTorch fallback for its kernels."
        )
    lib = C.CDLL(_LIB_PATH)
    for name, (res, argt) in EXPORTS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, argt
    if lib.svdq_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libsvdq_amd.so ABI {lib.svdq_abi_version()} != binding ABI {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().svdq_last_error().decode("utf-8", "replace")
        if rc == 1:
            raise ValueError(f"{what}: {msg}")
        if rc == 2:
            raise NotImplementedError(f"{what}: {msg}")
        raise RuntimeError(f"{what}: {msg}")
