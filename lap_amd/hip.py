"""ctypes binding of liblap_hip.so — the C ABI declared in include/lap_hip.h.

This module is the only place where Python touches the kernels.  It takes torch tensors
(device memory + the current HIP stream are PyTorch's job: plumbing), checks dtype /
contiguity, and passes raw device pointers.  There is NO fallback: if the shared library
is missing or a launch is rejected, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import pathlib

import torch

import os as _os

# LAP_HIP_LIB_VARIANT=<v>: load lap_amd/liblap_hip_<v>.so (a probe build with the ablation bits of LAP_GEMM_EXPERIMENTAL compiled in,
# `python -m lap_amd.build --variant=<v>`) instead of the production library.  Timing probes only; a missing file fails like the default.
_LIB_PATH = pathlib.Path(__file__).resolve().parent / (
    f"liblap_hip_{_os.environ['LAP_HIP_LIB_VARIANT']}.so" if _os.environ.get("LAP_HIP_LIB_VARIANT") else "liblap_hip.so")

GEMM_OUT_F32 = 1
GEMM_ACCUM = 2
GEMM_GELU = 4
GEMM_BIAS_F32 = 8
GEMM_PARTIALS = 16
GEMM_GELU_BF16 = 32
GEMM_GELU_EXP2 = 128
GEMM_GEGLU = 64


class LapHipError(RuntimeError):
    pass


def _load() -> C.CDLL:
    if not _LIB_PATH.exists():
        raise ImportError(
            f"{_LIB_PATH} not found: build it with `python -m lap_amd.build` (hipcc --offload-arch=gfx950). "
            "lap_amd has no CPU / eager fallback."
        )
    return C.CDLL(str(_LIB_PATH))


_lib = _load()

_vp, _i, _f, _ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong


class AttnFwdArgs(C.Structure):
    _fields_ = [
        ("q", _vp * 2), ("o", _vp * 2), ("k", _vp * 2), ("v", _vp * 2),
        ("q_len", _i * 2), ("k_len", _i * 2),
        ("q_rs", _i * 2), ("kv_rs", _i * 2), ("o_rs", _i * 2),
        ("qinfo", _vp), ("kinfo", _vp), ("lse", _vp),
        ("scratch", _vp), ("scratch_floats", _ll),
        ("scale", _f), ("nsplit", _i),
        ("B", _i), ("NH", _i), ("NKV", _i), ("HD", _i),
    ]


CHAIN_MAX_DEPTH = 32    # LAP_CHAIN_MAX_DEPTH (include/lap_hip.h)


class ServeChainArgs(C.Structure):
    _fields_ = [
        ("depth", _i), ("B", _i), ("S", _i), ("D", _i), ("H", _i), ("NH", _i), ("HD", _i), ("prefix_len", _i),
        ("x_in", _vp), ("x_out", _vp),
        ("mod", _vp), ("mod_slot_stride", _i),
        ("wqkv", _vp * CHAIN_MAX_DEPTH), ("wo", _vp * CHAIN_MAX_DEPTH), ("wgu", _vp * CHAIN_MAX_DEPTH), ("wd", _vp * CHAIN_MAX_DEPTH),
        ("cache_k", _vp * CHAIN_MAX_DEPTH), ("cache_v", _vp * CHAIN_MAX_DEPTH),
        ("kv_rs", _i),
        ("rope_table", _vp), ("qinfo", _vp), ("kinfo", _vp),
        ("q_scale", _f), ("eps", _f),
        ("q", _vp), ("k", _vp), ("v", _vp), ("o", _vp), ("xa", _vp), ("act", _vp),
        ("attn_scratch", _vp), ("attn_scratch_floats", _ll),
        ("counters", _vp), ("debug_clock", _vp),
        ("packed", _i), ("xs", _vp),
        ("tp_slabs", _vp), ("tp_xs", _vp), ("tp_xn", _vp), ("tp_k", _vp), ("tp_v", _vp),
    ]


class AttnBwdArgs(C.Structure):
    _fields_ = [
        ("q", _vp * 2), ("o", _vp * 2), ("d_o", _vp * 2), ("k", _vp * 2), ("v", _vp * 2),
        ("dq", _vp * 2), ("dk", _vp * 2), ("dv", _vp * 2),
        ("q_len", _i * 2), ("k_len", _i * 2),
        ("q_rs", _i * 2), ("kv_rs", _i * 2), ("o_rs", _i * 2),
        ("qinfo", _vp), ("kinfo", _vp), ("lse", _vp), ("delta", _vp),
        ("scratch", _vp), ("scratch_floats", _ll),
        ("scale", _f), ("hsplit", _i),
        ("B", _i), ("NH", _i), ("NKV", _i), ("HD", _i), ("stop_q1_to_k0", _i),
    ]


class GemmLeg(C.Structure):
    """lap_gemm_leg (include/lap_hip.h): one launch of a planned GEMM."""
    _fields_ = [(n, _ll) for n in ("off_a", "off_b", "off_c", "off_bias", "off_res")] + [
        (n, _i) for n in ("engine", "M", "N", "ksplit", "tile_base", "tile_count", "sub256", "part_compact", "f32_tile", "part", "reduce")]


GEMM_MAX_LEGS = 6                    # LAP_GEMM_MAX_LEGS
LEG_ASM, LEG_ASM_BIAS, LEG_ASM_RES, LEG_ASM_WGRAD_SUMSQ = 32, 33, 34, 35
ROUTE_WGRAD_SUMSQ = 65536
ROUTE_SWITCHES = {"LAP_GEMM_NO_ASM": 1, "LAP_GEMM_NO_ASM_NN": 2, "LAP_GEMM_NO_ASM_RES": 4, "LAP_GEMM_NO_MSPLIT": 8, "LAP_GEMM_NO_MSPLIT_LONGK": 16,
                  "LAP_GEMM_NO_NSPLIT": 32, "LAP_GEMM_NO_SERVING_TILES": 64, "LAP_GEMM_NO_PINGPONG": 128, "LAP_GEMM_NO_KTAIL": 256}

# name -> argtypes; every entry point of include/lap_hip.h must be listed here (tests check it).
SIGNATURES: dict[str, list] = {
    "lap_abi_version": [],
    "lap_gemm_bf16": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp],
    "lap_gemm_bf16_ex": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _i, _vp, _ll, _vp],
    "lap_gemm_set_debug": [_i],
    "lap_gemm_asm": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gemm_asm_ok": [_i, _i, _i, _i, _i, _i, _i, _i, _i],
    "lap_gemm_asm_launch_counts": [C.POINTER(C.c_longlong), _i],
    "lap_gemm_plan": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _i, _vp, _ll, C.c_uint, _vp, _i, C.POINTER(_i)],
    "lap_gemm_asm_bias": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gemm_asm_bias_ok": [_i, _i, _i, _i, _i, _i],
    "lap_gemm_asm_res": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gemm_asm_res_ok": [_i, _i, _i, _i, _i, _i, _i],
    "lap_gemm_asm_geglu_bwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gemm_asm_geglu_bwd_ok": [_i, _i, _i, _i, _i, _i],
    "lap_gemm_asm_geglu_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gemm_asm_geglu_fwd_ok": [_i, _i, _i, _i, _i, _i, _i],
    "lap_gemm_asm_wgrad": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "lap_gemm_wgrad_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _ll, _vp],
    "lap_gemm_asm_wgrad_b16": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "lap_gemm_wgrad_bf16": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _ll, _vp],
    "lap_gemm_asm_bias_gelu": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gemm_asm_gelu_bwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gemm_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp],
    "lap_amax_bf16": [_vp, _ll, _i, _ll, _vp, _vp],
    "lap_quantize_fp8": [_vp, _ll, _i, _ll, _vp, _vp, _ll, _vp, _vp],
    "lap_quantize_fp8_weight": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "lap_gemm_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp],
    "lap_rmsnorm_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp],
    "lap_rmsnorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "lap_rmsnorm_bwd_rows": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "lap_layernorm_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp],
    "lap_layernorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_layernorm_bwd_sum": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_rope_split_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp],
    "lap_rope_split_bwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp],
    "lap_rope_split_fwd_rows": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp],
    "lap_rope_split_bwd_rows": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp],
    "lap_geglu_fwd": [_vp, _vp, _i, _i, _vp],
    "lap_geglu_bwd": [_vp, _vp, _vp, _i, _i, _vp],
    "lap_geglu_fwd_ld": [_vp, _vp, _i, _i, _i, _i, _vp],
    "lap_geglu_bwd_ld": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "lap_gelu_fwd": [_vp, _vp, _ll, _vp],
    "lap_gelu_bwd": [_vp, _vp, _vp, _ll, _vp],
    "lap_embed_gather": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _i, _vp],
    "lap_embed_scatter_add": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp],
    "lap_gated_residual_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_gated_residual_bwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "lap_colsum_bf16": [_vp, _vp, _i, _i, _i, _vp],
    "lap_colsum_f32": [_vp, _vp, _i, _i, _i, _vp],
    "lap_cast_f32_to_bf16": [_vp, _vp, _ll, _vp],
    "lap_split_f32_hilo": [_vp, _i, _i, _i, _vp, _vp, _i, _vp],
    "lap_cast_bf16_to_f32": [_vp, _vp, _ll, _vp],
    "lap_add_bf16": [_vp, _vp, _vp, _ll, _vp],
    "lap_copy2d_bf16": [_vp, _vp, _i, _i, _i, _i, _vp],
    "lap_copy_rows_bf16": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "lap_gather_rows_bf16": [_vp, _vp, _vp, _i, _i, _vp],
    "lap_im2col_patch": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    "lap_augment_images": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_add_posemb_cast": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_add_posemb_cast_bwd": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_attention_fwd": [C.POINTER(AttnFwdArgs), _vp],
    "lap_attention_serve_splits": [_i, _i, _i, _i, _i],
    "lap_attention_serve": [C.POINTER(AttnFwdArgs), _vp],
    "lap_attention_serve_shared": [C.POINTER(AttnFwdArgs), _i, _vp],
    "lap_attention_bwd": [C.POINTER(AttnBwdArgs), _vp],
    "lap_attention_set_variant": [_i],
    "lap_rope_table": [_vp, _vp, _i, _i, _i, _i, _i, _vp],
    "lap_fused_reduce_rope_split": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp],
    "lap_fused_reduce_geglu": [_vp, _i, _vp, _i, _i, _vp],
    "lap_fused_reduce_residual_norm": [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _f, _vp],
    "lap_fused_reduce_norm": [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _vp],
    "lap_serve_infos": [C.POINTER(_vp), _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "lap_serve_qkv_rope": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp],
    "lap_serve_gate_up": [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _f, _vp],
    "lap_serve_proj_residual": [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp],
    "lap_serve_set_variant": [_i],
    "lap_serve_embed_actions": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_serve_chain_ok": [_i, _i, _i, _i, _i, _i, _i, _i],
    "lap_serve_chain_tp_ok": [_i, _i, _i, _i, _i, _i, _i, _i],
    "lap_serve_chain_counter_words": [],
    "lap_serve_chain_status": [_vp, C.POINTER(_i)],
    "lap_serve_chain": [C.POINTER(ServeChainArgs), _vp],
    "lap_serve_pack_weight": [_vp, _vp, _i, _i, _i, _i, _vp],
    "lap_serve_final_euler_embed": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp],
    "lap_panel_gemm_ok": [_i, _i, _i, _i],
    "lap_panel_gemm_pf": [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _f, _i, _i, _i, _i, _i, _vp, _i, _vp, _ll, _vp],
    "lap_panel_gemm": [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _f, _i, _i, _i, _i, _i, _vp, _i, _vp],
    "lap_serve_final_euler": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp],
    "lap_serve_final_euler_inpaint": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _f, _f, _vp],
    "lap_serve_final_euler_embed_inpaint": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp],
    "lap_ce_chunk_update": [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_ce_chunk_update_argmax": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_token_metrics": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp],
    "lap_ce_chunk_grad": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_ce_chunk_grad_hilo": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_adamw_ema_hilo": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _f, _f, _f, _f, _f, _vp],
    "lap_sumsq_f32": [_vp, _ll, _vp, _vp],
    "lap_sumsq_bf16": [_vp, _ll, _vp, _vp],
    "lap_grad_fold": [_vp, _vp, _i, _ll, _i, _vp, _vp],
    "lap_adamw_ema_g16": [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _f, _f, _f, _f, _f, _vp],
    "lap_argmax_rows_f32": [_vp, _i, _i, _i, _vp, _vp],
    "lap_gumbel_argmax_rows_f32": [_vp, _i, _i, _i, _f, C.c_uint, C.c_uint, _i, _vp, _vp],
    "lap_adamw_ema": [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp, _f, _f, _f, _f, _f, _vp],
    "lap_fm_mix": [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "lap_posemb_sincos": [_vp, _vp, _i, _i, _f, _f, _vp],
    "lap_swish_fwd": [_vp, _vp, _ll, _vp],
    "lap_swish_bwd": [_vp, _vp, _vp, _ll, _vp],
    "lap_mse_fwd_bwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "lap_axpy_f32": [_vp, _vp, _f, _ll, _vp],
    "lap_euler_inpaint_f32": [_vp, _vp, _f, _vp, _vp, _vp, _f, _f, _i, _i, _vp],
    "lap_action_select": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_lora_down": [_vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _f, _vp],
    "lap_lora_up_add": [_vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _f, _vp],
    "lap_lora_wgrad": [_vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp, _ll, _vp],
    "lap_lora_merge": [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _f, _vp],
    "lap_decode_ok": [_i, _i, _i, _i, _i, _i, _i],
    "lap_decode_state_words": [],
    "lap_decode_lm_blocks": [],
    "lap_decode_attn_scratch_floats": [_i, _i, _i],
    "lap_decode_init": [_vp, _vp, _vp, _i, _i, _vp],
    "lap_decode_embed": [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _i, _f, _vp],
    "lap_decode_qkv": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "lap_decode_attention": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _ll, _i, _i, _i, _i, _vp],
    "lap_decode_proj_residual": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_decode_gate_up": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp],
    "lap_decode_lm_head": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_finish": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_decode_sampling_words": [],
    "lap_decode_lm_head_sample": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_quantize_fp8_rows": [_vp, _i, _vp, _vp, _ll, _i, _vp],
    "lap_decode_qkv_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "lap_decode_gate_up_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp],
    "lap_decode_proj_residual_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_decode_lm_head_fp8": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_lm_head_sample_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_lm_head_subset": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_lm_head_subset_sample": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_lm_head_subset_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_lm_head_subset_sample_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_lm_head_lp": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "lap_decode_finish_lp": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_filter_gumbel_argmax_rows_f32": [_vp, _i, _i, _i, _f, C.c_uint, C.c_uint, _i, _i, _f, _vp, _vp, _vp, _vp],
    "lap_decode_filter_words": [],
    "lap_decode_filter_finish": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "lap_decode_spec_draft": [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp],
    "lap_decode_spec_embed": [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _f, _vp],
    "lap_decode_spec_qkv": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp],
    "lap_decode_spec_attention": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _ll, _i, _i, _i, _i, _vp],
    "lap_decode_spec_accept": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_decode_score_embed": [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _i, _f, _vp],
    "lap_decode_lm_head_score": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "lap_decode_lm_head_score_fp8": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "lap_decode_score_finish": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp],
    "lap_decode_grammar_finish": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_decode_grammar_draft": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp],
    "lap_decode_grammar_spec_finish": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_decode_beam_words": [],
    "lap_decode_beam_topn": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_decode_beam_select": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_decode_beam_reorder": [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "lap_decode_beam_grammar_topn": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "lap_decode_beam_grammar_select": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
}

_fn = {}
for _name, _args in SIGNATURES.items():
    _f_ = getattr(_lib, _name)  # AttributeError here = header / library mismatch: fail loudly
    _f_.argtypes = _args
    _f_.restype = C.c_int
    _fn[_name] = _f_

ABI_VERSION = _fn["lap_abi_version"]()
LIB_PATH = str(_LIB_PATH)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _chk(rc: int, name: str) -> None:
    if rc != 0:
        raise LapHipError(f"{name} failed with code {rc}" + (" (LAP_ERR_ARG: rejected arguments)" if rc == 1001 else ""))


def call(name: str, *args) -> None:
    """Raw call: args are python ints/floats/pointers; the current torch stream is appended."""
    _chk(_fn[name](*args, _stream()), name)


def _req(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    if t.dtype != dtype or not t.is_cuda:
        raise TypeError(f"{name}: expected cuda {dtype}, got {t.device} {t.dtype}")


# ------------------------------------------------------------------------------ GEMM
_SCRATCH: dict = {}
_NSPLIT_ENV = __import__("os").environ.get("LAP_ATTN_NSPLIT")
_SERVE_ATTN = __import__("os").environ.get("LAP_SERVE_ATTN", "1") != "0"     # A/B switch: "0" = the generic key-split kernel


def _gemm_scratch(device, floats: int = 160 * 1024 * 1024):
    """Per-stream f32 scratch (640 MB) lent to the GEMM for two-phase split-K; its uses are ordered by that stream."""
    key = (device.type, device.index, torch.cuda.current_stream().cuda_stream)
    t = _SCRATCH.get(key)
    if t is None:
        t = torch.empty(floats, dtype=torch.float32, device=device)
        _SCRATCH[key] = t
    return t


def gemm(a, b, out, *, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, bias=None, residual=None, ldr=0,
         alpha=1.0, gelu=False, accum=False, tile=-1, ksplit=0):
    """out[M,N] = epi(alpha * opA . opB); see include/lap_hip.h lap_gemm_bf16 / lap_gemm_bf16_ex."""
    _req(a, torch.bfloat16, "A"); _req(b, torch.bfloat16, "B")
    flags = 0
    if out.dtype == torch.float32:
        flags |= GEMM_OUT_F32
    elif out.dtype != torch.bfloat16:
        raise TypeError("gemm out must be bf16 or f32")
    if accum:
        flags |= GEMM_ACCUM
    if gelu:
        flags |= GEMM_GELU | (GEMM_GELU_BF16 if gelu == "bf16" else 0)   # "bf16": round the pre-activation to bf16 first
    if bias is not None and bias.dtype == torch.float32:
        flags |= GEMM_BIAS_F32
    # the library decides on two-phase split-K itself when it is lent scratch (poorly filled grids, skinny-M serving); an
    # accumulating product gets it too when its output is small and its contraction long (the LM head's hi / lo data gradients:
    # 16 output tiles over K = 257,152 — unsplit that is 16 CUs walking 4,018 k-tiles; the reduce pass adds onto C)
    scratch = _gemm_scratch(a.device) if (ksplit == 0 and (not accum or (K >= 16384 and M * N <= (1 << 22)))) else None
    call("lap_gemm_bf16_ex", _p(a), _p(b), _p(out), _p(bias), _p(residual), M, N, K, lda, ldb, ldc, ldr, float(alpha),
         int(a_kc), int(b_kc), flags, tile, ksplit, _p(scratch), scratch.numel() * 4 if scratch is not None else 0)
    return out


def linear_fwd(x, wt, out=None, *, bias=None, residual=None, gelu=False, out_dtype=torch.bfloat16, tile=-1, ksplit=0):
    """y[M,out] = x[M,in] @ wt[out,in]^T (+bias)(gelu)(+residual)."""
    M, K = x.shape
    N = wt.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=x.device)
    return gemm(x, wt, out, M=M, N=N, K=K, lda=x.stride(0), ldb=wt.stride(0), ldc=out.stride(0), bias=bias,
                residual=residual, ldr=(residual.stride(0) if residual is not None else 0), gelu=gelu, tile=tile,
                ksplit=ksplit)


def linear_geglu(x, wgu, exp2=False):
    """act[M, H] = GeGLU(x @ wgu[2H, in]^T): the gate|up projection and lap_geglu_fwd in one launch (serving prefill, M <= 640).
    exp2: the GELU through v_exp / v_rcp (the training kernel lap_gemm_asm_geglu_fwd's arithmetic) instead of tanhf."""
    M, K = x.shape
    H = wgu.shape[0] // 2
    act = torch.empty((M, H), dtype=torch.bfloat16, device=x.device)
    call("lap_gemm_bf16_ex", _p(x), _p(wgu), _p(act), None, None, M, 2 * H, K, x.stride(0), wgu.stride(0), H, 0, 1.0, 1, 1,
         GEMM_GEGLU | (GEMM_GELU_EXP2 if exp2 else 0), -1, 0,
         None, 0)
    return act


def linear_dgrad(dy, wt, out=None, *, out_dtype=torch.bfloat16, accum=False, tile=-1, ksplit=0):
    """dx[M,in] = dy[M,out] @ wt[out,in]."""
    M, K = dy.shape
    N = wt.shape[1]
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=dy.device)
    return gemm(dy, wt, out, M=M, N=N, K=K, lda=dy.stride(0), ldb=wt.stride(0), ldc=out.stride(0), a_kc=True,
                b_kc=False, accum=accum, tile=tile, ksplit=ksplit)


def linear_wgrad(dy, x, out, *, accum=False, ksplit=0, tile=-1):
    """dWt[out,in] (f32) = dy[M,out]^T @ x[M,in].  ksplit > 1 needs accum=True (adds onto `out`)."""
    Mrows, Nout = dy.shape
    Kin = x.shape[1]
    return gemm(dy, x, out, M=Nout, N=Kin, K=Mrows, lda=dy.stride(0), ldb=x.stride(0), ldc=out.stride(0), a_kc=False,
                b_kc=False, accum=accum, ksplit=ksplit, tile=tile)


def gemm_plan(*, M, N, K, lda, ldb, ldc, ldr=0, alpha=1.0, a_kc=True, b_kc=True, flags=0, tile=-1, ksplit=0, a=256, b=256, c=256, bias=None,
              residual=None, scratch=None, scratch_bytes=0, switches=0):
    """What lap_gemm_bf16_ex would launch for these arguments under the LAP_ROUTE_* `switches` (include/lap_hip.h: lap_gemm_plan): a list
    of GemmLeg.  No device is touched; pointers are plain integers (None: null) that only their alignment matters of.  Rejected
    arguments raise LapHipError with the code of the real call."""
    legs, n = (GemmLeg * GEMM_MAX_LEGS)(), _i(0)
    _chk(_fn["lap_gemm_plan"](a, b, c, bias, residual, M, N, K, lda, ldb, ldc, ldr, float(alpha), int(a_kc), int(b_kc), flags, tile, ksplit,
                              scratch, scratch_bytes, switches, legs, GEMM_MAX_LEGS, C.byref(n)), "lap_gemm_plan")
    return list(legs[:n.value])


ASM_KERNELS = ("nt", "nn", "tn", "nt_bias", "tn_t", "nt_res", "nt_bias_res", "nn_geglu_bwd", "nt_geglu", "nn_gelu_bwd", "nt_bias_gelu",
               "tn_b16", "tn_t_b16")


def gemm_asm_launch_counts() -> dict:
    """Launches of each assembly GEMM kernel since the library was loaded (include/lap_hip.h: lap_gemm_asm_launch_counts)."""
    buf = (C.c_longlong * len(ASM_KERNELS))()
    _chk(_fn["lap_gemm_asm_launch_counts"](buf, len(ASM_KERNELS)), "lap_gemm_asm_launch_counts")
    return dict(zip(ASM_KERNELS, (int(v) for v in buf)))


def linear_wgrad_sumsq(dy, x, out, sumsq):
    """dWt[out, in] (f32, or bf16: ParamStore.grad_dtype) = dy^T x like linear_wgrad, and where the assembly kernel takes the product sum(dWt^2) is added to the
    one-element f32 tensor `sumsq` on the way out; returns whether that happened (else the caller still owes the norm a pass)."""
    import ctypes
    Mrows, Nout = dy.shape
    Kin = x.shape[1]
    _req(dy, torch.bfloat16, "dy"); _req(x, torch.bfloat16, "x"); _req(sumsq, torch.float32, "sumsq")
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("linear_wgrad_sumsq: out must be f32 or bf16")
    folded = ctypes.c_int(0)
    scratch = _gemm_scratch(dy.device)
    call("lap_gemm_wgrad_f32" if out.dtype == torch.float32 else "lap_gemm_wgrad_bf16", _p(dy), _p(x), _p(out), Nout, Kin, Mrows, dy.stride(0), x.stride(0), out.stride(0), _p(sumsq),
         ctypes.byref(folded), _p(scratch), scratch.numel() * 4)
    return bool(folded.value)


def split_f32_hilo(x, ld_out=None):
    """x f32 [rows, cols] -> (hi, lo) bf16 [rows, ld_out] with hi + lo ~ x (16 mantissa bits), zero padded columns."""
    _req(x, torch.float32, "x")
    rows, cols = x.shape
    ld_out = (cols + 7) // 8 * 8 if ld_out is None else ld_out
    hi = torch.empty((rows, ld_out), dtype=torch.bfloat16, device=x.device)
    lo = torch.empty_like(hi)
    call("lap_split_f32_hilo", _p(x), rows, cols, x.stride(0), _p(hi), _p(lo), ld_out)
    return hi, lo


def argmax_rows(x, out=None):
    """x f32 [rows, n] (row stride x.stride(0)) -> int32 [rows], lowest index among ties."""
    _req(x, torch.float32, "x")
    if out is None:
        out = torch.empty((x.shape[0],), dtype=torch.int32, device=x.device)
    call("lap_argmax_rows_f32", _p(x), x.shape[0], x.shape[1], x.stride(0), _p(out))
    return out


def sampling_words(seed, temperature):
    """(seed low word, seed high word, inv_t) of a device-sampled draw (lap_amd/sampling.py): `seed` is taken modulo 2^64,
    inv_t = float32(1 / temperature), 0 (greedy) for temperature <= 0; a temperature whose inverse is not finite raises."""
    from lap_amd.sampling import inverse_temperature

    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32, float(inverse_temperature(temperature))


def gumbel_argmax_rows(x, temperature, seed, step, out=None):
    """x f32 [rows, n] -> int32 [rows]: argmax of x / temperature + the Gumbel noise of (seed, step, row, column), one pass."""
    _req(x, torch.float32, "x")
    lo, hi, inv_t = sampling_words(seed, temperature)
    if out is None:
        out = torch.empty((x.shape[0],), dtype=torch.int32, device=x.device)
    call("lap_gumbel_argmax_rows_f32", _p(x), x.shape[0], x.shape[1], x.stride(0), inv_t, lo, hi, int(step), _p(out))
    return out


def filter_gumbel_argmax_rows(x, temperature, seed, step, top_k=None, top_p=None, out=None, kept=None, cut=None):
    """`gumbel_argmax_rows` over the entries that top_k / top_p keep (lap_filter_gumbel_argmax_rows_f32; `sampling.filter_keep`
    restates the kept set): x f32 [rows, n] -> int32 [rows].  None is the neutral value of either filter, and with both neutral the
    token is `gumbel_argmax_rows`'.  kept (int32 [rows]) / cut (f32 [rows]), debug: the size of the kept set, the smallest kept z."""
    from lap_amd.sampling import check_filter

    _req(x, torch.float32, "x")
    k, p = check_filter(top_k, top_p)
    lo, hi, inv_t = sampling_words(seed, temperature)
    if x.dim() != 2 or x.stride(1) != 1:
        raise TypeError("filter_gumbel_argmax_rows: x must be [rows, n] with contiguous rows")
    if out is None:
        out = torch.empty((x.shape[0],), dtype=torch.int32, device=x.device)
    if kept is not None:
        _dreq(kept, torch.int32, "kept")
    if cut is not None:
        _dreq(cut, torch.float32, "cut")
    for t, n in ((out, "out"), (kept, "kept"), (cut, "cut")):
        if t is not None and t.numel() < x.shape[0]:
            raise TypeError(f"filter_gumbel_argmax_rows: {n} holds one entry per row")
    call("lap_filter_gumbel_argmax_rows_f32", _p(x), x.shape[0], x.shape[1], x.stride(0), inv_t, lo, hi, int(step), k, p, _p(out),
         _p(kept), _p(cut))
    return out


def gemm_f32(a, b, out, *, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, bias=None, alpha=1.0, accum=False):
    for t, n in ((a, "A"), (b, "B"), (out, "C")):
        _req(t, torch.float32, n)
    call("lap_gemm_f32", _p(a), _p(b), _p(out), _p(bias), M, N, K, lda, ldb, ldc, float(alpha), int(a_kc), int(b_kc),
         int(accum))
    return out


# ------------------------------------------------------------------- normalisation
def rmsnorm_fwd(x, scale=None, mod=None, rows_per_sample=0, eps=1e-6, save_rstd=True, mod_ld=None):
    """mod: bf16 [B, >=3D] view (row stride = mod.stride(0)) holding scale|shift|gate; mod_ld=0 shares row 0
    between all samples (serving: the condition depends on the denoise time only)."""
    rows, D = x.shape
    y = torch.empty_like(x)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_rstd else None
    if mod_ld is None:
        mod_ld = mod.stride(0) if mod is not None else 0
    call("lap_rmsnorm_fwd", _p(x), _p(scale), _p(mod), _p(y), _p(rstd), rows, D, rows_per_sample, mod_ld, float(eps))
    return y, rstd


def _row_map(t, n, name):
    """`t`: int32 [n] on the device, every entry -1 or a row of a compact tensor (the caller keeps them in range: no host sync here)."""
    _req(t, torch.int32, name)
    if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous int32 [{n}] tensor, got shape {tuple(t.shape)}")


def rmsnorm_bwd(x, dy, rstd, scale=None, mod=None, rows_per_sample=0, dx=None, dscale=None, dmod=None, accum_dx=False, add_row=None,
                addend=None):
    """add_row / addend (plain form only): dx[r] = norm-backward(dy)[r] + addend[add_row[r]] where add_row[r] >= 0, one pass."""
    rows, D = x.shape
    if dx is None:
        dx = torch.empty_like(x)
    if add_row is not None:
        if mod is not None or accum_dx or addend is None or scale is None or dscale is None:
            raise ValueError("rmsnorm_bwd: add_row goes with scale / dscale and an addend, not with mod or accum_dx")
        _row_map(add_row, rows, "add_row")
        _req(addend, torch.bfloat16, "addend")
        if addend.dim() != 2 or addend.shape[1] != D or not addend.is_contiguous() or not dx.is_contiguous() or dx.shape != x.shape:
            raise ValueError(f"rmsnorm_bwd: addend {tuple(addend.shape)} / dx {tuple(dx.shape)} do not fit x {tuple(x.shape)}")
        call("lap_rmsnorm_bwd_rows", _p(x), _p(scale), _p(rstd), _p(dy), _p(dx), _p(dscale), _p(add_row), _p(addend), rows, D)
        return dx
    call("lap_rmsnorm_bwd", _p(x), _p(scale), _p(mod), _p(rstd), _p(dy), _p(dx), _p(dscale), _p(dmod), rows, D,
         rows_per_sample, mod.stride(0) if mod is not None else 0, dmod.stride(0) if dmod is not None else 0,
         int(accum_dx))
    return dx


def layernorm_fwd(x, gamma, beta, eps=1e-6):
    rows, D = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    call("lap_layernorm_fwd", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, D, float(eps))
    return y, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, dgamma, dbeta, dx=None, accum_dx=False, dxsum=None):
    """dxsum: f32 [D] that the column sums of the returned dx are ADDED to (a bias gradient for free), or None."""
    rows, D = x.shape
    if dx is None:
        dx = torch.empty_like(x)
    call("lap_layernorm_bwd_sum", _p(x), _p(gamma), _p(mean), _p(rstd), _p(dy), _p(dx), _p(dgamma), _p(dbeta), _p(dxsum), rows, D,
         int(accum_dx))
    return dx


# --------------------------------------------------------------------- elementwise
def rope_split_fwd(qkv, pos, B, T_seg, T_total, seg_off, NH, HD, q_scale, q_row=None, q_rows=0):
    """q_row (int32 [B * T_seg]: the row of q that row r gets, or -1) with q_rows = the height of q: q comes out compact, k / v whole."""
    rows = B * T_seg
    q = torch.empty((rows if q_row is None else q_rows, NH * HD), dtype=torch.bfloat16, device=qkv.device)
    k = torch.empty((rows, HD), dtype=torch.bfloat16, device=qkv.device)
    v = torch.empty((rows, HD), dtype=torch.bfloat16, device=qkv.device)
    if q_row is not None:
        _row_map(q_row, rows, "q_row")
        if q_rows <= 0:
            raise ValueError("rope_split_fwd: q_row needs q_rows, the height of the compact q")
        call("lap_rope_split_fwd_rows", _p(qkv), _p(pos), _p(q_row), _p(q), _p(k), _p(v), B, T_seg, T_total, seg_off, NH, HD, float(q_scale))
    else:
        call("lap_rope_split_fwd", _p(qkv), _p(pos), _p(q), _p(k), _p(v), B, T_seg, T_total, seg_off, NH, HD, float(q_scale))
    return q, k, v


def rope_split_bwd(dq, dk, dv, pos, B, T_seg, T_total, seg_off, NH, HD, q_scale, q_row=None):
    """q_row as in rope_split_fwd: dq is compact, dqkv has all B * T_seg rows, zeros in the q columns of the rows without a dq row."""
    dqkv = torch.empty((B * T_seg, (NH + 2) * HD), dtype=torch.bfloat16, device=dq.device)
    if q_row is not None:
        _row_map(q_row, B * T_seg, "q_row")
        call("lap_rope_split_bwd_rows", _p(dq), _p(dk), _p(dv), _p(pos), _p(q_row), _p(dqkv), B, T_seg, T_total, seg_off, NH, HD,
             float(q_scale))
    else:
        call("lap_rope_split_bwd", _p(dq), _p(dk), _p(dv), _p(pos), _p(dqkv), B, T_seg, T_total, seg_off, NH, HD,
             float(q_scale))
    return dqkv


def _padded_rows(rows, cols, device, pad):
    """[rows, cols] bf16 view of a buffer whose rows are `pad` elements longer: see lap_geglu_fwd_ld in include/lap_hip.h"""
    return torch.empty((rows, cols + pad), dtype=torch.bfloat16, device=device)[:, :cols]


def _row_pad(cols):
    """64 elements when the dense row would be a multiple of 16 KiB (the bad strides measured: 32 and 64 KiB), else none"""
    return 64 if cols * 2 >= 16384 and (cols * 2) % 16384 == 0 else 0


def geglu_fwd(gu, pad=False):
    rows, H2 = gu.shape
    act = _padded_rows(rows, H2 // 2, gu.device, _row_pad(H2 // 2) if pad else 0)
    call("lap_geglu_fwd_ld", _p(gu), _p(act), rows, H2 // 2, gu.stride(0), act.stride(0))
    return act


def linear_bias_gelu_train_ok(x, wt, bias):
    M, K = x.shape
    N = wt.shape[0]
    return (x.dtype == wt.dtype == torch.bfloat16 and bias is not None and bias.dtype == torch.float32 and x.stride(1) == 1 and wt.stride(1) == 1
            and bool(_lib.lap_gemm_asm_bias_ok(M, N, K, x.stride(0), wt.stride(0), N)))


def linear_bias_gelu_train(x, wt, bias):
    """(h, a) = (x @ wt^T + bias, gelu(h)) in one launch, both kept (training: the backward pass reads h)"""
    M, K = x.shape
    N = wt.shape[0]
    h = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    a = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    call("lap_gemm_asm_bias_gelu", _p(x), _p(wt), _p(h), _p(a), _p(bias), M, N, K, x.stride(0), wt.stride(0), N)
    return h, a


def dgrad_gelu_bwd_ok(dy, w, h):
    M, K = dy.shape
    N = w.shape[1]
    return (dy.dtype == w.dtype == h.dtype == torch.bfloat16 and tuple(h.shape) == (M, N) and h.stride(1) == 1 and dy.stride(1) == 1 and w.stride(1) == 1
            and w.shape[0] == K and bool(_lib.lap_gemm_asm_ok(1, 0, 0, M, N, K, dy.stride(0), w.stride(0), h.stride(0))))


def linear_dgrad_gelu_bwd(dy, w, h):
    """d(h) = gelu_bwd(h, dy @ w) in one launch (the second Dense's data gradient with the GELU backward as its epilogue)"""
    M, K = dy.shape
    N = w.shape[1]
    if tuple(h.shape) != (M, N) or w.shape[0] != K:
        raise LapHipError(f"linear_dgrad_gelu_bwd: dy {tuple(dy.shape)}, w {tuple(w.shape)}, h {tuple(h.shape)} do not fit")
    dh = torch.empty((M, h.stride(0)), dtype=torch.bfloat16, device=h.device)[:, :N]
    call("lap_gemm_asm_gelu_bwd", _p(dy), _p(w), _p(dh), _p(h), M, N, K, dy.stride(0), w.stride(0), h.stride(0))
    return dh


def linear_geglu_train_ok(x, wgu, pad=True):
    M, K = x.shape
    N = wgu.shape[0]
    p = _row_pad(N) if pad else 0
    pa = _row_pad(N // 2) if pad else 0
    return (x.dtype == wgu.dtype == torch.bfloat16 and x.stride(1) == 1 and wgu.stride(1) == 1 and N % 256 == 0
            and bool(_lib.lap_gemm_asm_geglu_fwd_ok(M, N, K, x.stride(0), wgu.stride(0), N + p, N // 2 + pa)))


def linear_geglu_train(x, wgu, pad=True):
    """(gu, act) = (x @ wgu^T, GeGLU(gu)) in one launch, both kept (training: the backward pass reads gu); rows padded off the
    16 KiB strides like geglu_fwd / geglu_bwd do."""
    M, K = x.shape
    N = wgu.shape[0]
    gu = _padded_rows(M, N, x.device, _row_pad(N) if pad else 0)
    act = _padded_rows(M, N // 2, x.device, _row_pad(N // 2) if pad else 0)
    call("lap_gemm_asm_geglu_fwd", _p(x), _p(wgu), _p(gu), _p(act), M, N, K, x.stride(0), wgu.stride(0), gu.stride(0), act.stride(0))
    return gu, act


def dgrad_geglu_bwd_ok(dy, w, gu):
    """whether linear_dgrad_geglu_bwd takes (dy [M, K], w [K, N], gu [M, 2N] with any row stride >= 2N)"""
    M, K = dy.shape
    N = w.shape[1]
    return (dy.dtype == w.dtype == gu.dtype == torch.bfloat16 and gu.shape == (M, 2 * N) and gu.stride(1) == 1 and dy.stride(1) == 1 and w.stride(1) == 1
            and bool(_lib.lap_gemm_asm_geglu_bwd_ok(M, N, K, dy.stride(0), w.stride(0), gu.stride(0))))


def linear_dgrad_geglu_bwd(dy, w, gu):
    """dgu = geglu_bwd(gu, dy @ w) in one launch (the down projection's data gradient with the GeGLU backward as its epilogue);
    dgu gets gu's row stride."""
    M, K = dy.shape
    N = w.shape[1]
    if tuple(gu.shape) != (M, 2 * N) or w.shape[0] != K:
        raise LapHipError(f"linear_dgrad_geglu_bwd: dy {tuple(dy.shape)}, w {tuple(w.shape)}, gate|up {tuple(gu.shape)} do not fit")
    ld = gu.stride(0)
    dgu = torch.empty((M, ld), dtype=torch.bfloat16, device=gu.device)[:, :2 * N]
    call("lap_gemm_asm_geglu_bwd", _p(dy), _p(w), _p(dgu), _p(gu), M, N, K, dy.stride(0), w.stride(0), ld)
    return dgu


def geglu_bwd(gu, dact, pad=False):
    rows, H2 = gu.shape
    dgu = _padded_rows(rows, H2, gu.device, _row_pad(H2) if pad else 0)
    call("lap_geglu_bwd_ld", _p(gu), _p(dact), _p(dgu), rows, H2 // 2, gu.stride(0), dact.stride(0), dgu.stride(0))
    return dgu


def gelu_fwd(x):
    y = torch.empty_like(x)
    call("lap_gelu_fwd", _p(x), _p(y), x.numel())
    return y


def gelu_bwd(x, dy):
    dx = torch.empty_like(x)
    call("lap_gelu_bwd", _p(x), _p(dy), _p(dx), x.numel())
    return dx


def embed_gather(table, tok, out, rows, T, D, dst_rps, dst_off, scale, row_lo=0, row_hi=None):
    """table: f32 rows [row_lo, row_hi) of the vocabulary (default: the whole table)."""
    if row_hi is None:
        row_hi = row_lo + table.shape[0]
    call("lap_embed_gather", _p(table), _p(tok), _p(out), rows, T, D, dst_rps, dst_off, float(scale), row_lo, row_hi)


def embed_scatter_add(dtable, tok, dout, rows, T, D, src_rps, src_off, scale):
    call("lap_embed_scatter_add", _p(dtable), _p(tok), _p(dout), rows, T, D, src_rps, src_off, float(scale))


def gated_residual_fwd(x, u, gate=None, rows_per_sample=0, ldg=0):
    y = torch.empty_like(x)
    call("lap_gated_residual_fwd", _p(x), _p(u), _p(gate), _p(y), x.shape[0], x.shape[1], rows_per_sample, ldg)
    return y


def gated_residual_bwd(dy, u, gate, rows_per_sample, ldg, dgate, ldg_out):
    du = torch.empty_like(dy)
    call("lap_gated_residual_bwd", _p(dy), _p(u), _p(gate), _p(du), _p(dgate), dy.shape[0], dy.shape[1],
         rows_per_sample, ldg, ldg_out)
    return du


def colsum(x, out, rows=None, cols=None, ld=None):
    """out[c] += sum_r x[r, c] (f32 atomics; caller zeroes)."""
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1] if cols is None else cols
    ld = x.stride(0) if ld is None else ld
    call("lap_colsum_bf16" if x.dtype == torch.bfloat16 else "lap_colsum_f32", _p(x), _p(out), rows, cols, ld)


def cast_f32_to_bf16(x, y=None):
    if y is None:
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    call("lap_cast_f32_to_bf16", _p(x), _p(y), x.numel())
    return y


def cast_bf16_to_f32(x, y=None):
    if y is None:
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("lap_cast_bf16_to_f32", _p(x), _p(y), x.numel())
    return y


def add_bf16(a, b, y=None):
    if y is None:
        y = torch.empty_like(a)
    call("lap_add_bf16", _p(a), _p(b), _p(y), a.numel())
    return y


def copy2d_bf16(src, dst, rows, cols, lds, ldd):
    call("lap_copy2d_bf16", _p(src), _p(dst), rows, cols, lds, ldd)


def copy_rows_bf16(src, dst, rows, T, D, src_rps, src_off, dst_rps, dst_off, accumulate=False):
    call("lap_copy_rows_bf16", _p(src), _p(dst), rows, T, D, src_rps, src_off, dst_rps, dst_off, int(accumulate))


def gather_rows_bf16(src, idx):
    """out[r] = src[idx[r]]: bf16 [n, D] from bf16 [rows, D] and int32 [n] (in range: the caller's duty), lap_copy_rows_bf16's kernel."""
    _req(src, torch.bfloat16, "src")
    n = idx.numel()
    _row_map(idx, n, "idx")
    if src.dim() != 2 or not src.is_contiguous():
        raise ValueError(f"gather_rows_bf16: src must be a contiguous [rows, D] tensor, got {tuple(src.shape)}")
    out = torch.empty((n, src.shape[1]), dtype=torch.bfloat16, device=src.device)
    call("lap_gather_rows_bf16", _p(src), _p(idx), _p(out), n, src.shape[1])
    return out


def im2col_patch(img, P):
    B, H, W, Cc = img.shape
    out = torch.empty((B * (H // P) * (W // P), P * P * Cc), dtype=torch.float32, device=img.device)
    call("lap_im2col_patch", _p(img), _p(out), B, H, W, Cc, P)
    return out


def add_posemb_cast(x, pos, T):
    rows, D = x.shape
    y = torch.empty((rows, D), dtype=torch.bfloat16, device=x.device)
    call("lap_add_posemb_cast", _p(x), _p(pos), _p(y), rows, T, D)
    return y


def add_posemb_cast_bwd(dy, dpos, T):
    rows, D = dy.shape
    dx = torch.empty((rows, D), dtype=torch.float32, device=dy.device)
    call("lap_add_posemb_cast_bwd", _p(dy), _p(dx), _p(dpos), rows, T, D)
    return dx


# ----------------------------------------------------------------------- attention
def attention_set_variant(variant: int):
    """Test / benchmark knob: -1 automatic, 0 generic kernels, 1 / 2 row groups of the HD = 256 LDS-DMA kernels."""
    _chk(_fn["lap_attention_set_variant"](int(variant)), "lap_attention_set_variant")


def attention_fwd(q, k, v, q_len, k_len, B, NH, NKV, HD, qinfo=None, kinfo=None, need_lse=True, scale=1.0,
                  q_rs=(0, 0), kv_rs=(0, 0), nsplit_hint=None, o_out=None, lse_out=None):
    """q/k/v: lists of up to two segment tensors (None for an empty segment).  q_rs / kv_rs: row strides in
    elements when q / k / v are column slices of a wider (fused qkv) buffer; outputs are packed [B*len, NH*HD].
    o_out (a list of packed bf16 [B*len, NH*HD] per segment) / lse_out (f32 [B, NH, Tq]): write into the caller's buffers."""
    a = AttnFwdArgs()
    outs = []
    for s in range(2):
        qs = q[s] if s < len(q) else None
        a.q[s] = _p(qs)
        a.q_rs[s], a.kv_rs[s], a.o_rs[s] = q_rs[s], kv_rs[s], 0
        o = None
        if qs is not None:
            o = torch.empty((B * q_len[s], NH * HD), dtype=torch.bfloat16, device=qs.device) if o_out is None else \
                (o_out[s] if s < len(o_out) else None)
            if o is None or o.shape != (B * q_len[s], NH * HD) or o.dtype != torch.bfloat16 or not o.is_contiguous():
                raise TypeError("o_out must hold packed bf16 [B*len, NH*HD] tensors")
        outs.append(o)
        a.o[s] = _p(o)
        a.k[s] = _p(k[s]) if s < len(k) and k[s] is not None else None
        a.v[s] = _p(v[s]) if s < len(v) and v[s] is not None else None
        a.q_len[s] = q_len[s] if s < len(q_len) else 0
        a.k_len[s] = k_len[s] if s < len(k_len) else 0
    for nm, inf in (("qinfo", qinfo), ("kinfo", kinfo)):
        if inf is not None and (inf.dtype != torch.int32 or not inf.is_contiguous()):
            raise TypeError(f"{nm} must be a contiguous int32 tensor, got {inf.dtype}")
    Tq = a.q_len[0] + a.q_len[1]
    dev = next(t for t in q if t is not None).device
    lse = None
    if need_lse:
        lse = lse_out if lse_out is not None else torch.empty((B, NH, Tq), dtype=torch.float32, device=dev)
        if lse.shape != (B, NH, Tq) or lse.dtype != torch.float32 or not lse.is_contiguous():
            raise TypeError("lse_out must be a contiguous f32 [B, NH, Tq] tensor")
    a.qinfo, a.kinfo, a.lse = _p(qinfo), _p(kinfo), _p(lse)
    a.scale = float(scale)
    a.B, a.NH, a.NKV, a.HD = B, NH, NKV, HD
    # batch-1 denoise step: a handful of suffix queries against [KV cache | fresh keys] -> the load-everything-up-front kernel
    if _SERVE_ATTN and HD == 256 and a.q_len[0] == 0 and 0 < a.q_len[1] <= 64 and not need_lse and nsplit_hint is None and scale > 0:
        ns = _fn["lap_attention_serve_splits"](a.k_len[0], a.k_len[1], B, NH, a.q_len[1])
        if 0 < ns <= 16:
            a.nsplit = ns
            scratch = torch.empty(ns * B * Tq * NH * (HD + 1), dtype=torch.float32, device=dev)
            a.scratch, a.scratch_floats = _p(scratch), scratch.numel()
            _chk(_fn["lap_attention_serve"](C.byref(a), _stream()), "lap_attention_serve")
            return outs, None
    # few query tiles (serving): split the key tiles over more blocks
    ntq = (a.q_len[0] + 63) // 64 + (a.q_len[1] + 63) // 64
    ntk = (a.k_len[0] + 63) // 64 + (a.k_len[1] + 63) // 64
    blocks = B * NH * ntq
    nsplit = 1
    if nsplit_hint is None and _NSPLIT_ENV and blocks < 128 and ntk > 1:
        nsplit_hint = min(int(_NSPLIT_ENV), ntk)     # tuning knob (tools/bench_serve_split.py)
    if nsplit_hint is not None:
        nsplit = nsplit_hint
    elif blocks < 128 and ntk > 1:
        nsplit = min((ntk + 1) // 2, max(1, 256 // blocks))   # >= 128 keys per split: the combine cost grows with the split count
    a.nsplit = nsplit
    if nsplit > 1:
        scratch = torch.empty(nsplit * B * Tq * NH * (HD + 1), dtype=torch.float32, device=dev)
        a.scratch, a.scratch_floats = _p(scratch), scratch.numel()
    a.B, a.NH, a.NKV, a.HD = B, NH, NKV, HD
    _chk(_fn["lap_attention_fwd"](C.byref(a), _stream()), "lap_attention_fwd")
    return outs, lse


SERVE_SHARED_FORM = int(__import__("os").environ.get("LAP_SERVE_SHARED_FORM", "0"))     # A/B switch: 0 = resident image, 1 = one unit per block


def attention_serve_shared(q, k, v, prefix_k, prefix_v, N, S, Pn, NH, NKV, HD, qinfo=None, kinfo=None, scale=1.0, o_out=None, form=None):
    """The denoise-step attention of N candidate chunks of ONE observation (csrc/attention_serve_shared.hpp): q bf16 [N*S, NH*HD] and
    the fresh k / v bf16 [N*S, NKV*HD] are per candidate, prefix_k / prefix_v bf16 [Pn, NKV*HD] exist ONCE; qinfo [N, S] / kinfo
    [N, Pn + S] are the info words of a batch of N (the caller replicates the batch-1 words).  Returns o bf16 [N*S, NH*HD], bit-equal
    to `attention_fwd` on the prefix replicated N times.  ValueError on shapes the kernel does not take (HD != 256, S > 64, N > 8, ...)."""
    if HD != 256 or not 1 <= S <= 64 or not 1 <= N <= 8 or Pn < 1 or NH < 1 or NKV < 1 or NH % NKV or not scale > 0:
        raise ValueError(f"attention_serve_shared: HD = {HD} (256), S = {S} (1..64), N = {N} (1..8), Pn = {Pn} (>= 1), NH = {NH}, NKV = {NKV}, scale = {scale}")
    for nm, t, shape in (("q", q, (N * S, NH * HD)), ("k", k, (N * S, NKV * HD)), ("v", v, (N * S, NKV * HD)),
                         ("prefix_k", prefix_k, (Pn, NKV * HD)), ("prefix_v", prefix_v, (Pn, NKV * HD))):
        if t is None or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"attention_serve_shared: {nm} must be contiguous {shape}, got {None if t is None else tuple(t.shape)}")
        _req(t, torch.bfloat16, nm)
    if (qinfo is None) != (kinfo is None):
        raise ValueError("attention_serve_shared: qinfo and kinfo go together")
    for nm, inf, n in (("qinfo", qinfo, N * S), ("kinfo", kinfo, N * (Pn + S))):
        if inf is not None and (inf.dtype != torch.int32 or not inf.is_contiguous() or inf.numel() != n or not inf.is_cuda):
            raise ValueError(f"attention_serve_shared: {nm} must be a contiguous cuda int32 tensor of {n} words")
    o = torch.empty((N * S, NH * HD), dtype=torch.bfloat16, device=q.device) if o_out is None else o_out
    if tuple(o.shape) != (N * S, NH * HD) or o.dtype != torch.bfloat16 or not o.is_contiguous():
        raise ValueError("attention_serve_shared: o_out must be a packed bf16 [N*S, NH*HD] tensor")
    ns = _fn["lap_attention_serve_splits"](Pn, S, N, NH, S)
    if not 0 < ns <= 16:
        raise ValueError(f"attention_serve_shared: {Pn} + {S} keys do not fit the serving attention's key runs")
    a = AttnFwdArgs()
    a.q[1], a.o[1] = _p(q), _p(o)
    a.k[0], a.v[0], a.k[1], a.v[1] = _p(prefix_k), _p(prefix_v), _p(k), _p(v)
    a.q_len[1], a.k_len[0], a.k_len[1] = S, Pn, S
    a.qinfo, a.kinfo = _p(qinfo), _p(kinfo)
    a.scale, a.nsplit = float(scale), ns
    scratch = torch.empty(ns * N * S * NH * (HD + 1), dtype=torch.float32, device=q.device)
    a.scratch, a.scratch_floats = _p(scratch), scratch.numel()
    a.B, a.NH, a.NKV, a.HD = N, NH, NKV, HD
    _chk(_fn["lap_attention_serve_shared"](C.byref(a), SERVE_SHARED_FORM if form is None else int(form), _stream()), "lap_attention_serve_shared")
    return o


def attention_bwd(q, k, v, o, d_o, lse, q_len, k_len, B, NH, NKV, HD, qinfo=None, kinfo=None, stop_q1_to_k0=False,
                  scale=1.0, q_rs=(0, 0), kv_rs=(0, 0), dq_out=None, dk_out=None, dv_out=None):
    """Gradients are written with the same row strides as q / k / v (pass dq_out/dk_out/dv_out views of a fused
    dqkv buffer when q_rs / kv_rs are set)."""
    a = AttnBwdArgs()
    dq, dk, dv = [], [], []
    for s in range(2):
        def g(lst):
            return lst[s] if lst is not None and s < len(lst) else None
        a.q[s], a.o[s], a.d_o[s] = _p(g(q)), _p(g(o)), _p(g(d_o))
        a.k[s], a.v[s] = _p(g(k)), _p(g(v))
        a.q_rs[s], a.kv_rs[s], a.o_rs[s] = q_rs[s], kv_rs[s], 0
        dq.append(g(dq_out) if g(dq_out) is not None else (torch.empty_like(g(q)) if g(q) is not None else None))
        dk.append(g(dk_out) if g(dk_out) is not None else (torch.empty_like(g(k)) if g(k) is not None else None))
        dv.append(g(dv_out) if g(dv_out) is not None else (torch.empty_like(g(v)) if g(v) is not None else None))
        a.dq[s], a.dk[s], a.dv[s] = _p(dq[s]), _p(dk[s]), _p(dv[s])
        a.q_len[s] = q_len[s] if s < len(q_len) else 0
        a.k_len[s] = k_len[s] if s < len(k_len) else 0
    for nm, inf in (("qinfo", qinfo), ("kinfo", kinfo)):
        if inf is not None and (inf.dtype != torch.int32 or not inf.is_contiguous()):
            raise TypeError(f"{nm} must be a contiguous int32 tensor, got {inf.dtype}")
    Tq = a.q_len[0] + a.q_len[1]
    delta = torch.empty((B, NH, Tq), dtype=torch.float32, device=lse.device)
    a.qinfo, a.kinfo, a.lse, a.delta = _p(qinfo), _p(kinfo), _p(lse), _p(delta)
    a.scale = float(scale)
    hpk = NH // NKV
    hsplit = 1
    if hpk > 1:  # MQA / GQA: more blocks for the dK/dV kernel
        hsplit = 4 if hpk % 4 == 0 else (2 if hpk % 2 == 0 else 1)
    a.hsplit = hsplit
    if hsplit > 1:
        Tk = a.k_len[0] + a.k_len[1]
        scratch = torch.empty(2 * hsplit * B * Tk * NKV * HD, dtype=torch.float32, device=lse.device)
        a.scratch, a.scratch_floats = _p(scratch), scratch.numel()
    a.B, a.NH, a.NKV, a.HD, a.stop_q1_to_k0 = B, NH, NKV, HD, int(stop_q1_to_k0)
    _chk(_fn["lap_attention_bwd"](C.byref(a), _stream()), "lap_attention_bwd")
    return dq, dk, dv


# ----------------------------------------------------------------- loss / optimizer
def ce_chunk_update(logits, target, m, l, tl, v0):
    rows, vc = logits.shape
    call("lap_ce_chunk_update", _p(logits), logits.stride(0), _p(target), _p(m), _p(l), _p(tl), rows, v0, vc)


def ce_chunk_update_argmax(logits, target, m, l, tl, amax, v0):
    """ce_chunk_update plus the running row argmax into amax (int32 [rows], lowest index among ties): call once per vocab chunk
    in ascending v0, starting from the same m / l / tl state as ce_chunk_update (m below every logit)."""
    _req2(logits, torch.float32, "logits")
    rows, vc = logits.shape
    for t, dt, nm in ((target, torch.int32, "target"), (m, torch.float32, "m"), (l, torch.float32, "l"), (tl, torch.float32, "tl"),
                      (amax, torch.int32, "amax")):
        _req(t, dt, nm)
        if not t.is_contiguous() or t.numel() != rows:
            raise ValueError(f"{nm}: expected a contiguous tensor of {rows} elements, got shape {tuple(t.shape)}")
    call("lap_ce_chunk_update_argmax", _p(logits), logits.stride(0), _p(target), _p(m), _p(l), _p(tl), _p(amax), rows, int(v0), vc)


def token_metrics(pred, target, nll, lm, *, sel=None, critical=None, number=None, direction=None):
    """Verbose token metrics of metrics.py:7-45 in one launch (include/lap_hip.h lap_token_metrics).  pred / target (int32) and
    nll (f32): [B * Ls] over the computed rows; sel: int32 [B, Ls] positions of those rows (None: all Lm = Lt - 1 rows); lm: f32
    [B, Lm] loss weights; critical / number / direction: bool [B, Lm] class masks or None.  Returns per_token_loss f32 [B, Lm]
    and counts f32 [B, 4, 2] = (correct, total) for the loss mask, critical, number and direction tokens."""
    _req(lm, torch.float32, "lm")
    if lm.dim() != 2 or not lm.is_contiguous():
        raise ValueError(f"lm: expected a contiguous [B, Lm] tensor, got shape {tuple(lm.shape)}")
    B, Lm = lm.shape
    if sel is not None:
        _req2(sel, torch.int32, "sel")
        if sel.shape[0] != B or not sel.is_contiguous() or not 0 < sel.shape[1] <= Lm:
            raise ValueError(f"sel: expected a contiguous [{B}, <= {Lm}] tensor, got shape {tuple(sel.shape)}")
        Ls = sel.shape[1]
    else:
        Ls = Lm
    for t, dt, nm in ((pred, torch.int32, "pred"), (target, torch.int32, "target"), (nll, torch.float32, "nll")):
        _req(t, dt, nm)
        if not t.is_contiguous() or t.numel() != B * Ls:
            raise ValueError(f"{nm}: expected a contiguous tensor of B * Ls = {B * Ls} elements, got shape {tuple(t.shape)}")
    for t, nm in ((critical, "critical"), (number, "number"), (direction, "direction")):
        if t is not None:
            _req(t, torch.bool, nm)
            if tuple(t.shape) != (B, Lm) or not t.is_contiguous():
                raise ValueError(f"{nm}: expected a contiguous [{B}, {Lm}] bool tensor, got shape {tuple(t.shape)}")
    ptl = torch.empty((B, Lm), dtype=torch.float32, device=lm.device)
    counts = torch.empty((B, 4, 2), dtype=torch.float32, device=lm.device)
    call("lap_token_metrics", _p(pred), _p(target), _p(nll), _p(sel), Ls, _p(lm), _p(critical), _p(number), _p(direction), B, Lm,
         _p(ptl), _p(counts))
    return ptl, counts


def ce_chunk_grad(logits, target, m, l, w, dlogits, v0, dlogits_lo=None):
    """dlogits (bf16) = w * (softmax - onehot); with `dlogits_lo` also the bf16 residual plane (hi + lo ~ the f32 value)."""
    rows, vc = logits.shape
    if dlogits_lo is None:
        call("lap_ce_chunk_grad", _p(logits), logits.stride(0), _p(target), _p(m), _p(l), _p(w), _p(dlogits),
             dlogits.stride(0), rows, v0, vc)
    else:
        if dlogits_lo.stride(0) != dlogits.stride(0):
            raise ValueError("hi / lo planes must share the row stride")
        call("lap_ce_chunk_grad_hilo", _p(logits), logits.stride(0), _p(target), _p(m), _p(l), _p(w), _p(dlogits), _p(dlogits_lo),
             dlogits.stride(0), rows, v0, vc)


def sumsq_f32(x, out):
    """out[0] += sum x^2; x: an f32 or a bf16 gradient buffer (squares accumulated in f32 either way)."""
    if x.dtype == torch.bfloat16:
        call("lap_sumsq_bf16", _p(x), x.numel(), _p(out))
        return
    call("lap_sumsq_f32", _p(x), x.numel(), _p(out))


def grad_fold(acc, g, first, sumsq=None):
    """Gradient accumulation: acc = g (`first`) or acc += g, element by element in f32; g a bf16 or an f32 gradient buffer of acc's
    size.  `sumsq` (a one-element f32 tensor, on the last micro-step): sumsq[0] += sum of the squares of the values stored."""
    _req(acc, torch.float32, "acc")
    if g.dtype not in (torch.bfloat16, torch.float32) or not g.is_cuda:
        raise TypeError(f"g: expected cuda bf16 or f32, got {g.device} {g.dtype}")
    if g.numel() != acc.numel() or not (acc.is_contiguous() and g.is_contiguous()):
        raise ValueError("grad_fold: acc and g must be contiguous and of one size")
    if sumsq is not None:
        _req(sumsq, torch.float32, "sumsq")
    call("lap_grad_fold", _p(acc), _p(g), int(g.dtype == torch.bfloat16), acc.numel(), int(bool(first)), _p(sumsq))


def adamw_ema(p, m, v, ema, g, p16, scalars, b1, b2, eps, wd, max_norm, p16lo=None):
    if g.dtype == torch.bfloat16:       # GEMM-produced weight gradients (round 5): bf16 gradient buffer
        if p16lo is not None:
            raise ValueError("the hi / lo unit (embedding table) keeps f32 gradients")
        call("lap_adamw_ema_g16", _p(p), _p(m), _p(v), _p(ema), _p(g), _p(p16), p.numel(), _p(scalars), float(b1), float(b2),
             float(eps), float(wd), float(max_norm))
        return
    if p16lo is not None:
        call("lap_adamw_ema_hilo", _p(p), _p(m), _p(v), _p(ema), _p(g), _p(p16), _p(p16lo), p.numel(), _p(scalars), float(b1), float(b2),
             float(eps), float(wd), float(max_norm))
        return
    call("lap_adamw_ema", _p(p), _p(m), _p(v), _p(ema), _p(g), _p(p16), p.numel(), _p(scalars), float(b1), float(b2),
         float(eps), float(wd), float(max_norm))


def fm_mix(noise, actions, t):
    B = noise.shape[0]
    n_per = noise.numel() // B
    x_t = torch.empty_like(noise); u_t = torch.empty_like(noise)
    call("lap_fm_mix", _p(noise), _p(actions), _p(t), _p(x_t), _p(u_t), B, n_per)
    return x_t, u_t


def posemb_sincos(t, D, min_period, max_period):
    out = torch.empty((t.shape[0], D), dtype=torch.float32, device=t.device)
    call("lap_posemb_sincos", _p(t), _p(out), t.shape[0], D, float(min_period), float(max_period))
    return out


def swish_fwd(x):
    y = torch.empty_like(x)
    call("lap_swish_fwd", _p(x), _p(y), x.numel())
    return y


def swish_bwd(x, dy):
    dx = torch.empty_like(x)
    call("lap_swish_bwd", _p(x), _p(dy), _p(dx), x.numel())
    return dx


def mse_fwd_bwd(v, u, coef=None, need_grad=True):
    B = v.shape[0]
    n_per = v.numel() // B
    per = torch.empty(B, dtype=torch.float32, device=v.device)
    dv = torch.empty_like(v) if need_grad else None
    call("lap_mse_fwd_bwd", _p(v), _p(u), _p(coef), _p(per), _p(dv), B, n_per)
    return per, dv


def axpy_f32(x, v, dt):
    call("lap_axpy_f32", _p(x), _p(v), float(dt), x.numel())


# ------------------------------------------------ split-K partials + fused consumers (batch-1 denoise step)
SELECT_MODES = {"medoid": 0, "coherence": 1}


def action_select(cand, mode, known=None, weights=None, scores=None, index=None, best=None):
    """lap_action_select (lap_amd/action_select.py is the specification): cand f32 [N, S, ad] -> (scores f32 [N], index int32 [1],
    best f32 [S, ad] = a bit copy of cand[index]); mode "medoid", or "coherence" with known f32 [S, ad] and weights f32 [S].
    One launch, nothing read back: the outputs may be the caller's persistent buffers (graph capture)."""
    if mode not in SELECT_MODES:
        raise ValueError(f"action_select: mode must be 'medoid' or 'coherence', got {mode!r}")
    if cand.dim() != 3 or not cand.is_contiguous():
        raise ValueError(f"action_select: cand must be contiguous [N, S, action_dim], got {tuple(cand.shape)}")
    _req(cand, torch.float32, "cand")
    N, S, ad = cand.shape
    if not 1 <= N <= 64 or S < 1 or ad < 1 or S * ad > 4096:
        raise ValueError(f"action_select: N = {N} (1..64), S * action_dim = {S * ad} (1..4096)")
    if mode == "coherence":
        if known is None or weights is None:
            raise ValueError("action_select: mode 'coherence' needs known and weights")
        if tuple(known.shape) != (S, ad) or tuple(weights.shape) != (S,) or not known.is_contiguous() or not weights.is_contiguous():
            raise ValueError(f"action_select: known / weights have shapes {tuple(known.shape)} / {tuple(weights.shape)}, expected {(S, ad)} / {(S,)}")
        _req(known, torch.float32, "known"); _req(weights, torch.float32, "weights")
    else:
        known = weights = None
    dev = cand.device
    scores = torch.empty(N, dtype=torch.float32, device=dev) if scores is None else scores
    index = torch.empty(1, dtype=torch.int32, device=dev) if index is None else index
    best = torch.empty((S, ad), dtype=torch.float32, device=dev) if best is None else best
    for nm, t, shape, dt in (("scores", scores, (N,), torch.float32), ("index", index, (1,), torch.int32), ("best", best, (S, ad), torch.float32)):
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"action_select: {nm} must be contiguous {shape}, got {tuple(t.shape)}")
        _req(t, dt, nm)
    call("lap_action_select", _p(cand), _p(known), _p(weights), _p(scores), _p(index), _p(best), N, S, ad, SELECT_MODES[mode])
    return scores, index, best


def linear_partials(x, wt, scratch, ksplit=None, tile=6):
    """Raw f32 partial products of y = x @ wt^T, [ksplit, M, N] in `scratch` (a 1-D f32 tensor); returns (view, ksplit)."""
    M, K = x.shape
    N = wt.shape[0]
    if ksplit is None:
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        ksplit = max(1, min(K // 256, 256 // max(tiles, 1), 16))   # (K // 128, 384-512 blocks, K // 512 measured: no better)
    need = ksplit * M * N
    if scratch.numel() < need:
        raise ValueError("scratch too small for the requested split")
    call("lap_gemm_bf16_ex", _p(x), _p(wt), None, None, None, M, N, K, x.stride(0), wt.stride(0), N, 0, 1.0, 1, 1,
         GEMM_OUT_F32 | GEMM_PARTIALS, tile, ksplit, _p(scratch), scratch.numel() * 4)
    return scratch[:need].view(ksplit, M, N), ksplit


def serve_infos(img_masks, T_img, prompt_mask, langact_mask, S, suffix_idx):
    """Token info words / positions of the sampler (lap.py:624-654) in one launch: (qinfo_p, kinfo_p, ppos, qinfo_s, kinfo_all,
    pos_all), int32; masks are torch.bool tensors on the device."""
    B, Lt = prompt_mask.shape
    for t in (*img_masks, prompt_mask, *(() if langact_mask is None else (langact_mask,))):
        if t.dtype != torch.bool or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("serve_infos: contiguous cuda bool masks")
    Pn = len(img_masks) * T_img + Lt
    dev = prompt_mask.device
    mk = lambda n: torch.empty((B, n), dtype=torch.int32, device=dev)
    outs = (mk(Pn), mk(Pn), mk(Pn), mk(S), mk(Pn + S), mk(Pn + S))
    arr = (_vp * max(len(img_masks), 1))(*[_p(t) for t in img_masks])
    call("lap_serve_infos", arr, len(img_masks), T_img, _p(prompt_mask), _p(langact_mask), B, Lt, S, suffix_idx, *[_p(t) for t in outs])
    return outs


def fused_reduce_norm(part, ksplit, rows, D, *, bias=None, residual=None, norm=0, gamma=None, beta=None, eps=1e-6):
    """xn = bf16(sum of the split-K slabs (+ f32 bias) (+ bf16 residual)); h = RMSNorm (norm=1, gamma = the f32 scale) or
    LayerNorm (norm=2) of xn, or None (norm=0).  One pass: the serving prefill's reduce + epilogue + next norm."""
    xn = torch.empty((rows, D), dtype=torch.bfloat16, device=part.device)
    h = torch.empty_like(xn) if norm else None
    call("lap_fused_reduce_norm", _p(part), ksplit, _p(bias), _p(residual), norm, _p(gamma), _p(beta), _p(xn), _p(h), rows, D, float(eps))
    return xn, h


def augment_images(img, params):
    """img f32 [B, H, W, 3] in [-1, 1], params f32 [B, 12] (include/lap_hip.h) -> augmented copy."""
    _req(img, torch.float32, "img"); _req(params, torch.float32, "params")
    B, H, W, C = img.shape
    if C != 3 or params.shape != (B, 12) or not img.is_contiguous() or not params.is_contiguous():
        raise ValueError("augment_images: img [B, H, W, 3] and params [B, 12], both contiguous")
    out = torch.empty_like(img)
    call("lap_augment_images", _p(img), _p(out), _p(params), B, H, W)
    return out


def rope_table(pos, B, T_seg, T_total, seg_off, HD):
    """sin / cos of a segment's positions, f32 [B*T_seg, HD/2, 2] (hoisted out of the denoise loop's RoPE kernels)."""
    tab = torch.empty((B * T_seg, HD // 2, 2), dtype=torch.float32, device=pos.device)
    call("lap_rope_table", _p(pos), _p(tab), B, T_seg, T_total, seg_off, HD)
    return tab


def fused_reduce_rope_split(part, ksplit, pos, B, T_seg, T_total, seg_off, NH, HD, q_scale, table=None):
    rows = B * T_seg
    dev = part.device
    q = torch.empty((rows, NH * HD), dtype=torch.bfloat16, device=dev)
    k = torch.empty((rows, HD), dtype=torch.bfloat16, device=dev)
    v = torch.empty((rows, HD), dtype=torch.bfloat16, device=dev)
    call("lap_fused_reduce_rope_split", _p(part), ksplit, _p(pos), _p(table), _p(q), _p(k), _p(v), B, T_seg, T_total, seg_off, NH, HD,
         float(q_scale))
    return q, k, v


def fused_reduce_geglu(part, ksplit, rows, H):
    act = torch.empty((rows, H), dtype=torch.bfloat16, device=part.device)
    call("lap_fused_reduce_geglu", _p(part), ksplit, _p(act), rows, H)
    return act


def fused_reduce_residual_norm(part, ksplit, x, gate, ldg, mod, mod_ld, rows_per_sample, eps=1e-6):
    rows, D = x.shape
    xn = torch.empty_like(x)
    h = torch.empty_like(x) if mod is not None else None
    call("lap_fused_reduce_residual_norm", _p(part), ksplit, _p(x), _p(gate), ldg, _p(mod), mod_ld, _p(xn), _p(h), rows, D,
         rows_per_sample, float(eps))
    return xn, h


# ------------------------------------------------ skinny-M fused projections (batch-1 denoise step, csrc/serve_skinny.hip)
def serve_supported(D, HD, mlp_dim, NH):
    """Shapes the skinny kernels are built for (the LAP-3B action expert); anything else takes the partials + consumers path."""
    return D == 1024 and HD == 256 and NH * HD in (1024, 2048, 4096) and mlp_dim in (1024, 2048, 4096)


def serve_qkv_rope(x, mod, mod_ld, rps, wqkv, table, NH, HD, q_scale, eps=1e-6):
    M, D = x.shape
    q = torch.empty((M, NH * HD), dtype=torch.bfloat16, device=x.device)
    k = torch.empty((M, HD), dtype=torch.bfloat16, device=x.device)
    v = torch.empty((M, HD), dtype=torch.bfloat16, device=x.device)
    call("lap_serve_qkv_rope", _p(x), _p(mod), mod_ld, rps, _p(wqkv), _p(table), _p(q), _p(k), _p(v), M, D, NH, HD, float(q_scale), float(eps))
    return q, k, v


def serve_gate_up(x, mod, mod_ld, rps, wgu, eps=1e-6):
    M, D = x.shape
    H = wgu.shape[0] // 2
    act = torch.empty((M, H), dtype=torch.bfloat16, device=x.device)
    call("lap_serve_gate_up", _p(x), _p(mod), mod_ld, rps, _p(wgu), _p(act), M, D, H, float(eps))
    return act


def serve_proj_residual(a, w, x, gate, gate_ld, rps):
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    call("lap_serve_proj_residual", _p(a), _p(w), _p(x), _p(gate), gate_ld, rps, _p(out), M, N, K)
    return out


def serve_chain_ok(B, S, D, H, NH, HD, NKV, prefix_len) -> bool:
    """Shapes the one-launch denoise step (lap_serve_chain) is built for."""
    return bool(_fn["lap_serve_chain_ok"](B, S, D, H, NH, HD, NKV, prefix_len))


def serve_chain_counters(device) -> torch.Tensor:
    """The chain's barrier counters: zero before the first launch, left zero by every launch (allocate ONCE, outside stream capture)."""
    return torch.zeros(_fn["lap_serve_chain_counter_words"](), dtype=torch.int32, device=device)


def serve_chain_failed(counters: torch.Tensor) -> bool:
    """True if a block of some launch gave up waiting at a grid barrier (that launch's results are invalid).  Synchronises."""
    st = C.c_int(0)
    _chk(_fn["lap_serve_chain_status"](_p(counters), C.byref(st)), "lap_serve_chain_status")
    return bool(st.value)


PACK_QKV, PACK_GATE_UP, PACK_PLAIN = 1, 2, 3     # lap_serve_pack_weight kinds (= the skinny kernels' epilogue ids)


def serve_pack_weight(w, kind: int, HD: int = 0, out=None):
    """Fragment-packed image of a K-contiguous bf16 weight [N, K] for the packed chain (include/lap_hip.h: lap_serve_pack_weight)."""
    _req(w, torch.bfloat16, "w")
    N, K = w.shape
    if not w.is_contiguous():
        raise ValueError("serve_pack_weight: w must be contiguous")
    if out is None:
        out = torch.empty_like(w)
    call("lap_serve_pack_weight", _p(w), _p(out), N, K, kind, HD)
    return out


def panel_gemm_ok(M, N, K, ksplit=1) -> bool:
    return bool(_fn["lap_panel_gemm_ok"](M, N, K, ksplit))


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def panel_linear(x, wp, N, *, bias=None, residual=None, norm=0, gamma=None, beta=None, eps=1e-6, gelu=False, out=None, nt=0, prefetch=None):
    """y[M, N] = epi(norm(x)[M, K] @ W[N, K]^T) on the row-panel kernel (csrc/serve_panel.hip); wp = serve_pack_weight(W, PACK_PLAIN).
    prefetch: the weight tensor of the NEXT launch of the chain (pulled into the Infinity Cache beside this product)."""
    M, K = x.shape
    _req(x, torch.bfloat16, "x"); _req(wp, torch.bfloat16, "wp")
    if wp.numel() != N * K or not wp.is_contiguous():
        raise ValueError(f"panel_linear: wp must be the contiguous packed image of a [{N}, {K}] weight, got {tuple(wp.shape)}")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    flags = 0
    if gelu:    # "bf16": the pre-activation rounded to bf16 first; "exp2": that, with the GELU through v_exp / v_rcp (the training kernels' form)
        flags |= GEMM_GELU | (GEMM_GELU_BF16 if gelu in ("bf16", "exp2") else 0) | (GEMM_GELU_EXP2 if gelu == "exp2" else 0)
    call("lap_panel_gemm_pf", _p(x), x.stride(0), _p(wp), _p(out), out.stride(0), _p(bias), _p(residual),
         residual.stride(0) if residual is not None else 0, norm, _p(gamma), _p(beta), float(eps), M, N, K, flags, 1, None, nt,
         _p(prefetch), _nbytes(prefetch))
    return out


def panel_partials(x, wp, N, scratch, ksplit, nt=0, prefetch=None):
    """Raw f32 partial products [ksplit, M, N] of x @ W^T on the row-panel kernel (the consumers: fused_reduce_norm,
    fused_reduce_rope_split); ksplit = 1: the whole product as one f32 slab."""
    M, K = x.shape
    _req(x, torch.bfloat16, "x"); _req(wp, torch.bfloat16, "wp")
    if wp.numel() != N * K or not wp.is_contiguous():
        raise ValueError(f"panel_partials: wp must be the contiguous packed image of a [{N}, {K}] weight, got {tuple(wp.shape)}")
    need = ksplit * M * N
    if scratch.numel() < need:
        raise ValueError("scratch too small for the requested split")
    call("lap_panel_gemm_pf", _p(x), x.stride(0), _p(wp), None, 0, None, None, 0, 0, None, None, 0.0, M, N, K, 0, ksplit, _p(scratch), nt,
         _p(prefetch), _nbytes(prefetch))
    return scratch[:need].view(ksplit, M, N), ksplit


def serve_chain_tp_ok(B, S, D, H, NH, HD, NKV, prefix_len) -> bool:
    """Shapes (and device) the tensor-parallel form of the packed chain takes (lap_serve_chain with packed = 2)."""
    return bool(_fn["lap_serve_chain_tp_ok"](B, S, D, H, NH, HD, NKV, prefix_len))


def serve_chain_scratch(device, D, H, NH, HD, tp: bool = False) -> dict:
    """The packed chain's activation buffers (64 rows each, zero: the pad rows are never written).  Allocate ONCE per sampler,
    outside stream capture; a launch may be replayed from a graph that holds these addresses.  tp: also the tensor-parallel
    form's per-XCD buffers and partial-sum slabs."""
    z = lambda cols: torch.zeros((64, cols), dtype=torch.bfloat16, device=device)
    d = dict(q=z(NH * HD), o=z(NH * HD), xa=z(D), act=z(H), xs=z(D))
    if tp:
        z8 = lambda cols: torch.zeros((8, 64, cols), dtype=torch.bfloat16, device=device)
        d.update(tp_slabs=torch.zeros((2, 8, 64, D), dtype=torch.float32, device=device), tp_xs=z8(D), tp_xn=z8(D), tp_k=z8(HD), tp_v=z8(HD))
    return d


def serve_chain(x_in, mod, slot_stride, weights, caches, rope_table, qinfo, kinfo, B, S, NH, HD, H, prefix_len, q_scale, counters,
                eps=1e-6, debug_clock=None, keep=None, packed_scratch=None, tp: bool = False):
    """All action-expert layers of one denoise step in one persistent launch (include/lap_hip.h: lap_serve_chain).
    weights: per layer (wqkv, wo, wgu, wd); caches: per layer (k, v) of the prefix.  Returns the residual stream [B*S, D].
    `packed_scratch` (serve_chain_scratch): the weights are lap_serve_pack_weight images and the activations between the stages are
    fragment-packed too (same bits, every operand load 1 KiB contiguous per wave instruction).  `tp` (with a scratch made with
    tp=True): the tensor-parallel form, lap_serve_chain packed = 2."""
    M, D = x_in.shape
    dev = x_in.device
    depth = len(weights)
    a = ServeChainArgs()
    a.depth, a.B, a.S, a.D, a.H, a.NH, a.HD, a.prefix_len = depth, B, S, D, H, NH, HD, prefix_len
    out = torch.empty_like(x_in)
    a.x_in, a.x_out, a.mod, a.mod_slot_stride = _p(x_in), _p(out), _p(mod), slot_stride
    for l, (wqkv, wo, wgu, wd) in enumerate(weights):
        a.wqkv[l], a.wo[l], a.wgu[l], a.wd[l] = _p(wqkv), _p(wo), _p(wgu), _p(wd)
        ck, cv = caches[l]
        a.cache_k[l], a.cache_v[l] = _p(ck), _p(cv)
    a.kv_rs = 0
    a.rope_table, a.qinfo, a.kinfo = _p(rope_table), _p(qinfo), _p(kinfo)
    a.q_scale, a.eps = float(q_scale), float(eps)
    bf = dict(dtype=torch.bfloat16, device=dev)
    k, v = torch.empty((M, HD), **bf), torch.empty((M, HD), **bf)
    if packed_scratch is not None:
        ps = packed_scratch
        q, o, xa, act = ps["q"], ps["o"], ps["xa"], ps["act"]
        a.packed, a.xs = 1, _p(ps["xs"])
        if tp:
            a.packed = 2
            a.tp_slabs, a.tp_xs, a.tp_xn, a.tp_k, a.tp_v = (_p(ps[n]) for n in ("tp_slabs", "tp_xs", "tp_xn", "tp_k", "tp_v"))
    else:
        q, o = torch.empty((M, NH * HD), **bf), torch.empty((M, NH * HD), **bf)
        xa, act = torch.empty((M, D), **bf), torch.empty((M, H), **bf)
        a.packed, a.xs = 0, None
    ns = _fn["lap_attention_serve_splits"](prefix_len, S, B, NH, S)
    scratch = torch.empty(ns * M * NH * (HD + 1), dtype=torch.float32, device=dev)
    a.q, a.k, a.v, a.o, a.xa, a.act = _p(q), _p(k), _p(v), _p(o), _p(xa), _p(act)
    a.attn_scratch, a.attn_scratch_floats, a.counters = _p(scratch), scratch.numel(), _p(counters)
    a.debug_clock = _p(debug_clock)
    if keep is not None:      # (tests / debugging: the last layer's intermediates)
        keep.update(q=q, k=k, v=v, o=o, xa=xa, act=act)
    _chk(_fn["lap_serve_chain"](C.byref(a), _stream()), "lap_serve_chain")
    return out


def serve_embed_actions(x_t, w_in, b_in):
    rows, ad = x_t.shape
    D = w_in.shape[0]
    tok = torch.empty((rows, D), dtype=torch.bfloat16, device=x_t.device)
    call("lap_serve_embed_actions", _p(x_t), _p(w_in), _p(b_in), _p(tok), rows, ad, D)
    return tok


def serve_final_euler(x, mod, mod_ld, rps, w_out, b_out, x_t, dt, v_out=None, eps=1e-6):
    rows, D = x.shape
    call("lap_serve_final_euler", _p(x), _p(mod), mod_ld, rps, _p(w_out), _p(b_out), _p(x_t), _p(v_out), rows, D, w_out.shape[0], float(dt), float(eps))


def serve_final_euler_embed(x, mod, mod_ld, rps, w_out, b_out, x_t, dt, v_out=None, eps=1e-6, w_in=None, b_in=None, tokens=None):
    """serve_final_euler (action_dim 7 or 8 at width 1024) and, with `tokens` (a [rows, D] bf16 tensor to fill), the next step's serve_embed_actions in one launch."""
    rows, D = x.shape
    call("lap_serve_final_euler_embed", _p(x), _p(mod), mod_ld, rps, _p(w_out), _p(b_out), _p(x_t), _p(v_out), rows, D, w_out.shape[0], float(dt), float(eps),
         _p(w_in), _p(b_in), _p(tokens))


def _inpaint_args(x_t, noise, known, mask, t_next):
    """Checked (noise, known, mask, t', 1 - t') of the inpainting tails: x_t f32 [rows, ad]; noise, known like it; mask uint8 [rows]."""
    _req(x_t, torch.float32, "x_t")
    if x_t.dim() != 2 or not x_t.is_contiguous():
        raise ValueError(f"x_t: expected a contiguous [rows, action_dim] tensor, got {tuple(x_t.shape)}")
    for name, t in (("noise", noise), ("known", known)):
        _req(t, torch.float32, name)
        if t.shape != x_t.shape or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous {tuple(x_t.shape)} tensor, got {tuple(t.shape)}")
    _req(mask, torch.uint8, "mask")
    if mask.dim() != 1 or mask.shape[0] != x_t.shape[0] or not mask.is_contiguous():
        raise ValueError(f"mask: expected a contiguous [{x_t.shape[0]}] tensor (one flag per row), got {tuple(mask.shape)}")
    tp, omtp = (float(t) for t in t_next)
    return _p(noise), _p(known), _p(mask), tp, omtp


def serve_final_euler_inpaint(x, mod, mod_ld, rps, w_out, b_out, x_t, dt, noise, known, mask, t_next, v_out=None, eps=1e-6):
    """serve_final_euler with the rows flagged in `mask` (uint8 [rows]) set to t' noise + (1 - t') known, `t_next` = (t', 1 - t')
    rounded from float64 (`flow_sample.inpaint_times`); the free rows are bit-identical to serve_final_euler.  Not in the reference."""
    rows, D = x.shape
    call("lap_serve_final_euler_inpaint", _p(x), _p(mod), mod_ld, rps, _p(w_out), _p(b_out), _p(x_t), _p(v_out), rows, D, w_out.shape[0], float(dt),
         float(eps), *_inpaint_args(x_t, noise, known, mask, t_next))


def serve_final_euler_embed_inpaint(x, mod, mod_ld, rps, w_out, b_out, x_t, dt, noise, known, mask, t_next, v_out=None, eps=1e-6,
                                    w_in=None, b_in=None, tokens=None):
    """serve_final_euler_embed with frozen rows as in serve_final_euler_inpaint; a frozen row's interpolation is what `tokens` embeds."""
    rows, D = x.shape
    call("lap_serve_final_euler_embed_inpaint", _p(x), _p(mod), mod_ld, rps, _p(w_out), _p(b_out), _p(x_t), _p(v_out), rows, D, w_out.shape[0],
         float(dt), float(eps), _p(w_in), _p(b_in), _p(tokens), *_inpaint_args(x_t, noise, known, mask, t_next))


def euler_inpaint_f32(x_t, v, dt, noise, known, mask, t_next):
    """axpy_f32 on x_t, v [rows, ad] with the frozen rows of serve_final_euler_inpaint (the same expression: the same bits)."""
    _req(v, torch.float32, "v")
    if v.shape != x_t.shape or not v.is_contiguous():
        raise ValueError(f"v: expected a contiguous {tuple(x_t.shape)} tensor, got {tuple(v.shape)}")
    args = _inpaint_args(x_t, noise, known, mask, t_next)
    call("lap_euler_inpaint_f32", _p(x_t), _p(v), float(dt), *args, x_t.shape[0], x_t.shape[1])


def serve_set_variant(feature_tiles: int):
    """Tuning knob of lap_serve_proj_residual (tools/bench_skinny.py)."""
    _chk(_fn["lap_serve_set_variant"](int(feature_tiles)), "lap_serve_set_variant")


# ------------------------------------------------------------------------- fp8 GEMM path (csrc/gemm_fp8.hip, config 5)
def quantize_fp8(x):
    """bf16 [rows, cols] (row stride x.stride(0)) -> (uint8 [rows, cols] e4m3 bytes, f32 scale [1]); per-tensor current scaling."""
    _req(x, torch.bfloat16, "x")
    rows, cols = x.shape
    amax = torch.zeros(1, dtype=torch.float32, device=x.device)
    call("lap_amax_bf16", _p(x), rows, cols, x.stride(0), _p(amax))
    out = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    call("lap_quantize_fp8", _p(x), rows, cols, x.stride(0), _p(amax), _p(out), cols, _p(scale))
    return out, scale


def quantize_fp8_weight(wt):
    """bf16 Wt [out, in] contiguous -> (W8 [out, in], W8t [in, out], scale [1])."""
    _req(wt, torch.bfloat16, "wt")
    if not wt.is_contiguous():
        raise ValueError("quantize_fp8_weight needs a contiguous weight")
    rows, cols = wt.shape
    amax = torch.zeros(1, dtype=torch.float32, device=wt.device)
    call("lap_amax_bf16", _p(wt), rows, cols, cols, _p(amax))
    w8 = torch.empty((rows, cols), dtype=torch.uint8, device=wt.device)
    w8t = torch.empty((cols, rows), dtype=torch.uint8, device=wt.device)
    scale = torch.empty(1, dtype=torch.float32, device=wt.device)
    call("lap_quantize_fp8_weight", _p(wt), rows, cols, _p(amax), _p(w8), _p(w8t), _p(scale))
    return w8, w8t, scale


def gemm_fp8(a8, sa, b8, sb, out=None, *, residual=None, out_dtype=torch.bfloat16, accum=False, alpha=1.0):
    """out[M, N] = alpha / (sa * sb) * a8[M, K] @ b8[N, K]^T (+ residual): fp8 e4m3 operands, f32 accumulate."""
    M, K = a8.shape
    N = b8.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a8.device)
    flags = (GEMM_OUT_F32 if out.dtype == torch.float32 else 0) | (GEMM_ACCUM if accum else 0)
    call("lap_gemm_fp8", _p(a8), _p(b8), _p(out), _p(residual), _p(sa), _p(sb), M, N, K, a8.stride(0), b8.stride(0), out.stride(0),
         residual.stride(0) if residual is not None else 0, float(alpha), flags)
    return out


def stream_with_hip_priority(device, level: str):
    """A HIP stream of the LOWEST ("low") or HIGHEST ("high") priority the device offers, wrapped for torch (torch itself only
    creates streams of normal or higher priority).  hipStreamNonBlocking, like torch's own pool streams.  The wrapper keeps no
    ownership: the stream lives for the rest of the process (one per pipeline object)."""
    import ctypes
    rt = ctypes.CDLL("libamdhip64.so")
    least, greatest = ctypes.c_int(0), ctypes.c_int(0)
    if rt.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) != 0:
        raise LapHipError("hipDeviceGetStreamPriorityRange failed")
    handle = ctypes.c_void_p()
    dev = torch.device(device)
    with torch.cuda.device(dev):
        rc = rt.hipStreamCreateWithPriority(ctypes.byref(handle), ctypes.c_uint(1), ctypes.c_int(least.value if level == "low" else greatest.value))
    if rc != 0 or not handle.value:
        raise LapHipError(f"hipStreamCreateWithPriority failed: {rc}")
    return torch.cuda.ExternalStream(handle.value, device=dev)


# ------------------------------------------------------------------------------ LoRA (csrc/lora.hip)
def _req2(t, dtype, name):
    _req(t, dtype, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a row-major 2-D tensor, got shape {tuple(t.shape)} strides {t.stride()}")


def lora_down(x, w, *, G=1, nsum=1, xg=0, s=1.0, out=None):
    """t[M, G*R] = bf16(x . w^T) per group (include/lap_hip.h lap_lora_down): the forward down projection t = x A^T (G = 1, w = A),
    or the data gradient dt of t (x = dy, xg = the group's column stride in dy, w = B with `nsum` stacked copies, s = the adapter
    scaling: dy is taken as bf16(s dy))."""
    _req2(x, torch.bfloat16, "x"); _req2(w, torch.bfloat16, "w")
    M = x.shape[0]
    R = w.shape[0] // (G * nsum)
    K = w.shape[1]
    if out is None:
        out = torch.empty((M, G * R), dtype=torch.bfloat16, device=x.device)
    _req2(out, torch.bfloat16, "out")
    call("lap_lora_down", _p(x), x.stride(0), xg, _p(w), w.stride(0), nsum, _p(out), out.stride(0), M, K, G, R, float(s))
    return out


def lora_up_add(y, t, b, *, G=1, nsum=1, s=1.0):
    """y[:, g*Ng:(g+1)*Ng] = bf16(y + bf16(s bf16(t_g . B_g))) in place (lap_lora_up_add): the LoRA term of a projection (b = B,
    `nsum` stacked copies summed), or the data-gradient add dx += bf16(dt . A) (b = A, G = 1)."""
    _req2(y, torch.bfloat16, "y"); _req2(t, torch.bfloat16, "t"); _req2(b, torch.bfloat16, "b")
    R = b.shape[0] // (G * nsum)
    Ng = b.shape[1]
    if y.shape[1] != G * Ng or t.shape[1] < G * R or t.shape[0] != y.shape[0]:
        raise ValueError(f"lora_up_add: y {tuple(y.shape)}, t {tuple(t.shape)}, b {tuple(b.shape)}, G {G}")
    call("lap_lora_up_add", _p(t), t.stride(0), _p(b), b.stride(0), nsum, _p(y), y.stride(0), y.shape[0], Ng, G, R, float(s))
    return y


def lora_wgrad(a, b, out, *, G=1, bg=0, ncopy=1, s=1.0, msplit=0):
    """out[(n*G + g)*R + i][c] = sum_m a[m][g*R + i] bs[m][g*bg + c] for n < ncopy (lap_lora_wgrad): dA = dt^T x (G = 1) and
    dB = t^T dy (bs = bf16(s dy)), into a bf16 or f32 gradient buffer.  msplit = 0: split M until the grid has ~1024 blocks."""
    _req2(a, torch.bfloat16, "a"); _req2(b, torch.bfloat16, "b")
    if out.dtype not in (torch.bfloat16, torch.float32) or out.dim() != 2 or out.stride(1) != 1:
        raise TypeError("lora_wgrad: out must be a row-major 2-D bf16 / f32 tensor")
    M = a.shape[0]
    GR = out.shape[0] // ncopy
    R, Ng = GR // G, out.shape[1]
    if b.shape[0] != M:
        raise ValueError("lora_wgrad: a and b need the same rows")
    if msplit <= 0:
        blocks = ((Ng + 63) // 64) * (GR // 16)
        msplit = max(1, min((1024 + blocks - 1) // blocks, M // 256))
    scratch = _gemm_scratch(a.device) if msplit > 1 else None
    call("lap_lora_wgrad", _p(a), a.stride(0), _p(b), b.stride(0), bg, _p(out), out.stride(0), ncopy, int(out.dtype == torch.float32),
         M, Ng, G, R, float(s), msplit, _p(scratch), scratch.numel() if scratch is not None else 0)
    return out


def lora_merge(w, a, b, out, *, G=1, nsum=1, s=1.0):
    """out = bf16(w + s . (B^T A) per group) (lap_lora_merge): the merged bf16 weight of a LoRA'd projection from f32 w [G*Ng][I],
    a [G*R][I], b [nsum*G*R][Ng] (the serving paths' weights)."""
    for t, nm in ((w, "w"), (a, "a"), (b, "b")):
        _req2(t, torch.float32, nm)
    _req2(out, torch.bfloat16, "out")
    R = a.shape[0] // G
    Ng = b.shape[1]
    if w.shape[0] != G * Ng or out.shape != w.shape or a.shape[1] != w.shape[1] or b.shape[0] != nsum * G * R:
        raise ValueError(f"lora_merge: w {tuple(w.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)}, G {G}, nsum {nsum}")
    call("lap_lora_merge", _p(w), w.stride(0), _p(a), a.stride(0), _p(b), b.stride(0), nsum, _p(out), out.stride(0), w.shape[1], Ng, G,
         R, float(s))
    return out


# ------------------------------------------------------------------ fused single-token decode (csrc/decode.hip)
DECODE_KWAVES_DOWN = 4      # lap_decode_proj_residual's K split for the down projection (K 16384): tools/bench_ar.py --kwaves


def decode_ok(B, D, NH, NKV, HD, H, V) -> bool:
    """True when lap_decode_* serve these widths (Gemma-2B: D 2048, 8 / 1 heads of 256, MLP 16384; 1 <= B <= 8)."""
    return bool(_fn["lap_decode_ok"](int(B), int(D), int(NH), int(NKV), int(HD), int(H), int(V)))


def decode_state(B, device):
    """Device state of one decode (include/lap_hip.h lap_decode_*): int32 [lap_decode_state_words()]."""
    return torch.zeros(_fn["lap_decode_state_words"](), dtype=torch.int32, device=device)


def decode_lm_partials(B, device):
    n = _fn["lap_decode_lm_blocks"]() * B
    return torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.int32, device=device)


def decode_attn_scratch(B, Pn, cap, device):
    n = _fn["lap_decode_attn_scratch_floats"](int(B), int(Pn), int(cap))
    if n <= 0:
        raise LapHipError("lap_decode_attn_scratch_floats: rejected arguments")
    return torch.empty(n, dtype=torch.float32, device=device)


def _dreq(t, dtype, name):
    _req(t, dtype, name)
    if not t.is_contiguous():
        raise TypeError(f"{name} must be contiguous")


def decode_init(state, plen, out):
    _dreq(state, torch.int32, "state"); _dreq(plen, torch.int32, "plen"); _dreq(out, torch.int32, "out")
    call("lap_decode_init", _p(state), _p(plen), _p(out), out.shape[0], out.shape[1])


def decode_embed(state, table, row_lo, row_hi, out, x, scale):
    _dreq(x, torch.bfloat16, "x"); _dreq(table, torch.float32, "table")
    call("lap_decode_embed", _p(state), _p(table), int(row_lo), int(row_hi), _p(out), out.shape[1], _p(x), x.shape[0], x.shape[1],
         float(scale))


def _f8req(w, wscale, name):
    """An fp8 weight of the fused decode: e4m3 codes [N, K] (torch.float8_e4m3fn or its bytes as uint8) + f32 scales [N]."""
    if w.dtype not in (torch.uint8, torch.float8_e4m3fn) or not w.is_cuda or not w.is_contiguous() or w.dim() != 2:
        raise TypeError(f"{name}: expected contiguous cuda e4m3 codes [N, K] (float8_e4m3fn / uint8), got {w.device} {w.dtype}")
    _dreq(wscale, torch.float32, name + " scales")
    if wscale.numel() != w.shape[0]:
        raise TypeError(f"{name}: {w.shape[0]} rows but {wscale.numel()} scales")


def quantize_fp8_rows(w, codes=None, scales=None):
    """w bf16 or f32 [N, K] -> (codes float8_e4m3fn [N, K], scales f32 [N] = 2^e) in the row format of lap_amd/fp8.py; `codes` /
    `scales` given: written in place (the buffers a captured decode graph holds)."""
    if w.dtype not in (torch.bfloat16, torch.float32) or not w.is_cuda or not w.is_contiguous() or w.dim() != 2:
        raise TypeError(f"quantize_fp8_rows: expected a contiguous cuda bf16 / f32 matrix, got {w.device} {w.dtype} {tuple(w.shape)}")
    N, K = w.shape
    if codes is None:
        codes = torch.empty((N, K), dtype=torch.float8_e4m3fn, device=w.device)
    if scales is None:
        scales = torch.empty((N,), dtype=torch.float32, device=w.device)
    _f8req(codes, scales, "codes")
    if tuple(codes.shape) != (N, K):
        raise TypeError(f"quantize_fp8_rows: codes {tuple(codes.shape)} for a weight {(N, K)}")
    call("lap_quantize_fp8_rows", _p(w), 1 if w.dtype == torch.float32 else 0, _p(codes), _p(scales), N, K)
    return codes, scales


def decode_qkv(state, x, gamma, wqkv, q, cache_k, cache_v, NH, HD, q_scale, eps=1e-6, wscale=None):
    """cache_k / cache_v: bf16 [B, cap, HD].  wscale given: wqkv is e4m3 codes with these row scales (lap_decode_qkv_fp8); the
    other decode_* projections and LM heads take an fp8 weight the same way."""
    for t, n in ((x, "x"), (q, "q"), (cache_k, "cache_k"), (cache_v, "cache_v")):
        _dreq(t, torch.bfloat16, n)
    _dreq(gamma, torch.float32, "gamma")
    B, D = x.shape
    if wscale is not None:
        _f8req(wqkv, wscale, "wqkv")
        call("lap_decode_qkv_fp8", _p(state), _p(x), _p(gamma), _p(wqkv), _p(wscale), _p(q), _p(cache_k), _p(cache_v), B, D, NH, HD,
             cache_k.shape[1], float(q_scale), float(eps))
        return
    _dreq(wqkv, torch.bfloat16, "wqkv")
    call("lap_decode_qkv", _p(state), _p(x), _p(gamma), _p(wqkv), _p(q), _p(cache_k), _p(cache_v), B, D, NH, HD, cache_k.shape[1],
         float(q_scale), float(eps))


def decode_attention(state, q, prefix_k, prefix_v, kinfo, Pn, cache_k, cache_v, o, scratch, NH, NKV, HD):
    for t, n in ((q, "q"), (prefix_k, "prefix_k"), (prefix_v, "prefix_v"), (cache_k, "cache_k"), (cache_v, "cache_v"), (o, "o")):
        _dreq(t, torch.bfloat16, n)
    _dreq(kinfo, torch.int32, "kinfo"); _dreq(scratch, torch.float32, "scratch")
    B = q.shape[0]
    call("lap_decode_attention", _p(state), _p(q), _p(prefix_k), _p(prefix_v), _p(kinfo), int(Pn), _p(cache_k), _p(cache_v),
         cache_k.shape[1], _p(o), _p(scratch), scratch.numel(), B, NH, NKV, HD)


def decode_proj_residual(state, a, w, x, y, kwaves=4, wscale=None):
    for t, n in ((a, "a"), (x, "x"), (y, "y")):
        _dreq(t, torch.bfloat16, n)
    B, K = a.shape
    if wscale is not None:
        _f8req(w, wscale, "w")
        call("lap_decode_proj_residual_fp8", _p(state), _p(a), _p(w), _p(wscale), _p(x), _p(y), B, w.shape[0], K, int(kwaves))
        return
    _dreq(w, torch.bfloat16, "w")
    call("lap_decode_proj_residual", _p(state), _p(a), _p(w), _p(x), _p(y), B, w.shape[0], K, int(kwaves))


def decode_gate_up(state, x, gamma, wgu, act, eps=1e-6, wscale=None):
    for t, n in ((x, "x"), (act, "act")):
        _dreq(t, torch.bfloat16, n)
    _dreq(gamma, torch.float32, "gamma")
    B, D = x.shape
    if wscale is not None:
        _f8req(wgu, wscale, "wgu")
        call("lap_decode_gate_up_fp8", _p(state), _p(x), _p(gamma), _p(wgu), _p(wscale), _p(act), B, D, act.shape[1], float(eps))
        return
    _dreq(wgu, torch.bfloat16, "wgu")
    call("lap_decode_gate_up", _p(state), _p(x), _p(gamma), _p(wgu), _p(act), B, D, act.shape[1], float(eps))


def _ids_req(ids, V):
    """The allowed set of a constrained LM head: int32 device ids [n], 1 <= n <= V (sorted, unique and inside [0, V): the caller's
    part, see ar_decode.check_allowed_tokens; checking it here would read the device on every token)."""
    _dreq(ids, torch.int32, "ids")
    if ids.dim() != 1 or not 1 <= ids.numel() <= V:
        raise ValueError(f"ids: expected 1 <= n <= V = {V} ids in one dimension, got shape {tuple(ids.shape)}")


def _decode_lm_head(fn, sampling, state, x, gamma, hi, lo, pval, pidx, logits, eps, wscale, ids, plp=None):
    """The body of `decode_lm_head` (sampling None), `decode_lm_head_sample` and `decode_lm_head_lp` (plp given); `fn` names the
    caller in error messages."""
    _dreq(x, torch.bfloat16, "x"); _dreq(gamma, torch.float32, "gamma")
    smp, lead = "", (_p(state),)
    if sampling is not None:
        _dreq(sampling, torch.int32, "sampling")
        if sampling.numel() < _fn["lap_decode_sampling_words"]():
            raise TypeError("sampling: int32 [lap_decode_sampling_words()]")
        smp, lead = "_sample", (_p(state), _p(sampling))
    if logits is not None:
        _dreq(logits, torch.float32, "logits")
    B, D = x.shape
    sub, tail = "", ()
    if ids is not None:
        _ids_req(ids, hi.shape[0])
        sub, tail = "_subset", (_p(ids), ids.numel())
    if wscale is not None:
        _f8req(hi, wscale, "hi")
        if lo is not None:
            raise TypeError(f"{fn}: the fp8 table is one plane (lo must be None)")
        planes, f8 = (_p(hi), _p(wscale)), "_fp8"
    else:
        _dreq(hi, torch.bfloat16, "hi")
        if lo is not None:
            _dreq(lo, torch.bfloat16, "lo")
        planes, f8 = (_p(hi), _p(lo)), ""
    if plp is not None:     # one entry point for every form
        _dreq(plp, torch.float32, "plp")
        if plp.numel() < 3 * B * _fn["lap_decode_lm_blocks"]():
            raise TypeError(f"{fn}: plp holds f32 [lap_decode_lm_blocks()][B][3]")
        call("lap_decode_lm_head_lp", _p(state), _p(sampling), _p(x), _p(gamma), _p(hi), _p(lo), _p(wscale), _p(ids),
             0 if ids is None else ids.numel(), B, D, hi.shape[0], float(eps), _p(logits), _p(pval), _p(pidx), _p(plp))
        return
    call(f"lap_decode_lm_head{sub}{smp}{f8}", *lead, _p(x), _p(gamma), *planes, *tail, B, D, hi.shape[0], float(eps), _p(logits),
         _p(pval), _p(pidx))


def decode_lm_head(state, x, gamma, hi, lo, pval, pidx, logits=None, eps=1e-6, wscale=None, ids=None):
    """logits (debug): f32 [B, V] written when given.  wscale given: `hi` is the one e4m3 code plane of the table, lo is None.
    ids given: the head over that allowed set only (lap_decode_lm_head_subset*): partials over the rows ids[.], logits written
    at those indices alone."""
    _decode_lm_head("decode_lm_head", None, state, x, gamma, hi, lo, pval, pidx, logits, eps, wscale, ids)


def decode_sampling(device):
    """The sampling words of a decode (lap_decode_lm_head_sample): int32 [4] = {seed low, seed high, bits of inv_t, 0}; zeros are
    a greedy decode.  A captured graph holds its address; `decode_set_sampling` rewrites it between replays."""
    return torch.zeros(_fn["lap_decode_sampling_words"](), dtype=torch.int32, device=device)


def decode_set_sampling(buf, seed, temperature):
    """Fill the sampling words with a plain host-to-device copy (no kernel).  temperature <= 0 is greedy."""
    import numpy as np

    _dreq(buf, torch.int32, "sampling")
    lo, hi, inv_t = sampling_words(seed, temperature)
    words = np.array([lo, hi, int(np.float32(inv_t).view(np.uint32)), 0], dtype=np.uint32).view(np.int32)
    buf.copy_(torch.from_numpy(words))


def decode_lm_head_sample(state, sampling, x, gamma, hi, lo, pval, pidx, logits=None, eps=1e-6, wscale=None, ids=None):
    """`decode_lm_head` with the sampler of `sampling` (see `decode_sampling`) as its epilogue; logits (debug) stay raw.  ids: the
    allowed set, as in `decode_lm_head`; the noise of a row stays that of its vocabulary index."""
    _decode_lm_head("decode_lm_head_sample", sampling, state, x, gamma, hi, lo, pval, pidx, logits, eps, wscale, ids)


def decode_finish(state, pval, pidx, out, eos_token):
    call("lap_decode_finish", _p(state), _p(pval), _p(pidx), _p(out), out.shape[0], out.shape[1], int(eos_token))


def decode_lm_logp_partials(B, device):
    """The log-sum-exp partials of `decode_lm_head_lp`: f32 [lap_decode_lm_blocks(), B, 3] = {m, s, z of the block's best}."""
    return torch.empty((_fn["lap_decode_lm_blocks"](), B, 3), dtype=torch.float32, device=device)


def decode_lm_head_lp(state, sampling, x, gamma, hi, lo, pval, pidx, plp, logits=None, eps=1e-6, wscale=None, ids=None):
    """`decode_lm_head` (sampling None) or `decode_lm_head_sample` of the same arguments, with the same pval / pidx / logits bit
    for bit, that also leaves the log-sum-exp partials of z = logit * inv_t (the raw logits when greedy) in `plp` for
    `decode_finish_lp` (lap_decode_lm_head_lp).  ids must be distinct (as `ar_decode.check_allowed_tokens` delivers them): a
    repeated id would enter the sum once per occurrence, while `sampling.token_logprobs` counts a set."""
    _decode_lm_head("decode_lm_head_lp", sampling, state, x, gamma, hi, lo, pval, pidx, logits, eps, wscale, ids, plp=plp)


def decode_finish_lp(state, pval, pidx, plp, out, logp, eos_token):
    """`decode_finish` that also writes logp[:, t], the log-probability of the chosen token under the noise-free softmax of z
    (lap_amd/sampling.py `token_logprobs`).  logp: f32 [B, cap] beside out; columns never written keep what they held."""
    _dreq(plp, torch.float32, "plp"); _dreq(logp, torch.float32, "logp")
    if tuple(logp.shape) != tuple(out.shape):
        raise TypeError(f"decode_finish_lp: logp {tuple(logp.shape)} beside out {tuple(out.shape)}")
    call("lap_decode_finish_lp", _p(state), _p(pval), _p(pidx), _p(plp), _p(out), _p(logp), out.shape[0], out.shape[1], int(eos_token))


def decode_filter(device):
    """The filter words of a filtering decode (lap_decode_filter_finish): int32 [4] = {top_k, bits of float32 top_p, 0, 0}; the
    neutral words {0, bits of 1.0, 0, 0} keep every candidate.  A captured graph holds its address; `decode_set_filter` rewrites
    it between replays."""
    buf = torch.zeros(_fn["lap_decode_filter_words"](), dtype=torch.int32, device=device)
    decode_set_filter(buf, None, None)
    return buf


def decode_set_filter(buf, top_k, top_p):
    """Fill the filter words with a plain host-to-device copy (no kernel).  None: the neutral value."""
    import numpy as np

    from lap_amd.sampling import check_filter

    _dreq(buf, torch.int32, "filter")
    k, p = check_filter(top_k, top_p)
    words = np.array([k, int(np.float32(p).view(np.uint32)), 0, 0], dtype=np.uint32).view(np.int32)
    buf.copy_(torch.from_numpy(words))


def decode_filter_finish(state, sampling, filt, logits, out, eos_token, logp=None, kept=None, cut=None):
    """`decode_finish` / `decode_finish_lp` of a filtering step: the token of every row is drawn from the f32 `logits` [B, V] that
    the LM head of the step stored, over the entries the filter words keep, with the sampler's score (lap_decode_filter_finish).
    logp (f32 [B, cap] beside out): also the token's log-probability over ALL candidates at tau = inv_t.  kept / cut: debug."""
    _dreq(state, torch.int32, "state"); _dreq(sampling, torch.int32, "sampling"); _dreq(filt, torch.int32, "filter")
    _dreq(logits, torch.float32, "logits"); _dreq(out, torch.int32, "out")
    B, cap = out.shape
    if logits.dim() != 2 or logits.shape[0] != B:
        raise TypeError(f"decode_filter_finish: logits {tuple(logits.shape)} for {B} rows")
    if sampling.numel() < _fn["lap_decode_sampling_words"]() or filt.numel() < _fn["lap_decode_filter_words"]():
        raise TypeError("decode_filter_finish: sampling / filter words: int32 [4] each")
    if logp is not None:
        _dreq(logp, torch.float32, "logp")
        if tuple(logp.shape) != tuple(out.shape):
            raise TypeError(f"decode_filter_finish: logp {tuple(logp.shape)} beside out {tuple(out.shape)}")
    if kept is not None:
        _dreq(kept, torch.int32, "kept")
    if cut is not None:
        _dreq(cut, torch.float32, "cut")
    for t, n in ((kept, "kept"), (cut, "cut")):
        if t is not None and t.numel() < B:
            raise TypeError(f"decode_filter_finish: {n} holds one entry per row")
    call("lap_decode_filter_finish", _p(state), _p(sampling), _p(filt), _p(logits), _p(out), _p(logp), B, logits.shape[1], cap,
         int(eos_token), _p(kept), _p(cut))


def decode_grammar_finish(state, sampling, gstate, offsets, ids, nxt, logits, out, eos_token, logp=None):
    """`decode_finish` / `decode_finish_lp` of a grammar-constrained step (lap_decode_grammar_finish): row b draws among the edges of
    its automaton state gstate[b] (int32 [B], advanced in place) from the f32 `logits` [B, V] that the SUBSET LM head over the
    automaton's union stored.  offsets [Q+1], ids [E], nxt [E]: the int32 device CSR of `grammar.TokenAutomaton.to_device` (checked
    there, once: checking it here would read the device on every token).  sampling: the sampling words, or None (greedy).
    logp (f32 [B, cap] beside out): also the token's log-probability over its state's set."""
    _dreq(state, torch.int32, "state"); _dreq(gstate, torch.int32, "gstate"); _dreq(logits, torch.float32, "logits")
    _dreq(out, torch.int32, "out")
    for t, n in ((offsets, "offsets"), (ids, "ids"), (nxt, "next")):
        _dreq(t, torch.int32, n)
    B, cap = out.shape
    if logits.dim() != 2 or logits.shape[0] != B or gstate.numel() != B:
        raise TypeError(f"decode_grammar_finish: logits {tuple(logits.shape)}, gstate {tuple(gstate.shape)} for {B} rows")
    if offsets.numel() < 2 or nxt.numel() != ids.numel() or ids.numel() < 1:
        raise TypeError(f"decode_grammar_finish: offsets [Q+1], ids [E], next [E]; got {offsets.numel()}, {ids.numel()}, {nxt.numel()}")
    if sampling is not None:
        _dreq(sampling, torch.int32, "sampling")
        if sampling.numel() < _fn["lap_decode_sampling_words"]():
            raise TypeError("decode_grammar_finish: sampling words: int32 [4]")
    if logp is not None:
        _dreq(logp, torch.float32, "logp")
        if tuple(logp.shape) != tuple(out.shape):
            raise TypeError(f"decode_grammar_finish: logp {tuple(logp.shape)} beside out {tuple(out.shape)}")
    call("lap_decode_grammar_finish", _p(state), _p(sampling), _p(gstate), _p(offsets), _p(ids), _p(nxt), offsets.numel() - 1,
         ids.numel(), _p(logits), _p(out), _p(logp), B, logits.shape[1], cap, int(eos_token))


def _automaton_req(fn, offsets, ids, nxt):
    for t, n in ((offsets, "offsets"), (ids, "ids"), (nxt, "next")):
        _dreq(t, torch.int32, n)
    if offsets.numel() < 2 or nxt.numel() != ids.numel() or ids.numel() < 1:
        raise TypeError(f"{fn}: offsets [Q+1], ids [E], next [E]; got {offsets.numel()}, {ids.numel()}, {nxt.numel()}")


def decode_grammar_draft(state, gstate, offsets, ids, nxt, draft, out, V, eos_token):
    """The drafts of a jump-forward step (lap_decode_grammar_draft; `speculate.grammar_drafts`), over the raw reference drafts that
    `decode_spec_draft` left in draft [S - 1]: from the state gstate[0], a state with a single edge drafts that id, any other keeps
    the reference's draft when it is one of its edges, and the first position with neither ends the run (-1 from there on).
    out: the [1, cap] token output of the one sequence (its cap bounds t, as in `decode_spec_draft`)."""
    cap = _spec_out(out)
    _dreq(state, torch.int32, "state"); _dreq(gstate, torch.int32, "gstate"); _dreq(draft, torch.int32, "draft")
    _automaton_req("decode_grammar_draft", offsets, ids, nxt)
    if gstate.numel() != 1:
        raise TypeError(f"decode_grammar_draft: gstate of one sequence, got {tuple(gstate.shape)}")
    call("lap_decode_grammar_draft", _p(state), _p(gstate), _p(offsets), _p(ids), _p(nxt), offsets.numel() - 1, ids.numel(), int(V),
         cap, int(eos_token), _p(draft), draft.numel() + 1)


def decode_grammar_spec_finish(state, sampling, gstate, offsets, ids, nxt, logits, draft, out, eos_token, logp=None):
    """The finish of a jump-forward step (lap_decode_grammar_spec_finish; `speculate.grammar_verify`): the S = draft.numel() + 1 rows
    of f32 `logits` [S, V] are drawn in sequence, row r from the state the rows before it led to, at step t + r, each with the bits
    of `decode_grammar_finish` at B = 1; then the accept rule of `decode_spec_accept`.  out / logp: [1, cap]."""
    cap = _spec_out(out)
    _dreq(state, torch.int32, "state"); _dreq(gstate, torch.int32, "gstate"); _dreq(logits, torch.float32, "logits")
    _dreq(draft, torch.int32, "draft")
    _automaton_req("decode_grammar_spec_finish", offsets, ids, nxt)
    S = draft.numel() + 1
    if logits.dim() != 2 or logits.shape[0] != S or gstate.numel() != 1:
        raise TypeError(f"decode_grammar_spec_finish: logits {tuple(logits.shape)}, gstate {tuple(gstate.shape)} for {S} rows of one sequence")
    if sampling is not None:
        _dreq(sampling, torch.int32, "sampling")
        if sampling.numel() < _fn["lap_decode_sampling_words"]():
            raise TypeError("decode_grammar_spec_finish: sampling words: int32 [4]")
    if logp is not None:
        _dreq(logp, torch.float32, "logp")
        if tuple(logp.shape) != tuple(out.shape):
            raise TypeError(f"decode_grammar_spec_finish: logp {tuple(logp.shape)} beside out {tuple(out.shape)}")
    call("lap_decode_grammar_spec_finish", _p(state), _p(sampling), _p(gstate), _p(offsets), _p(ids), _p(nxt), offsets.numel() - 1,
         ids.numel(), _p(logits), _p(draft), _p(out), _p(logp), S, logits.shape[1], cap, int(eos_token))


# ---- greedy speculative decoding of one sequence (csrc/decode_spec.hip; lap_amd/speculate.py restates the rules)
def _spec_out(out):
    """The token output of a speculating context: int32 [1, cap] (one sequence)."""
    _dreq(out, torch.int32, "out")
    if out.dim() != 2 or out.shape[0] != 1:
        raise TypeError(f"speculative decoding serves one sequence: out [1, cap], got {tuple(out.shape)}")
    return out.shape[1]


def decode_spec_ref(cap, device):
    """The reference sequence of a speculating context: int32 [1 + cap] = {its length n, ref[0 .. cap)}; a captured graph holds
    its address and `decode_set_spec_ref` rewrites it between requests."""
    return torch.zeros(1 + int(cap), dtype=torch.int32, device=device)


def decode_set_spec_ref(buf, ids):
    """ids (any integer sequence, or None: no draft) truncated to the buffer's capacity: one host-to-device copy."""
    cap = buf.numel() - 1
    ids = [] if ids is None else [int(i) for i in torch.as_tensor(ids).reshape(-1).tolist()][:cap]
    host = torch.zeros(1 + cap, dtype=torch.int32)
    host[0] = len(ids)
    if ids:
        host[1:1 + len(ids)] = torch.tensor(ids, dtype=torch.int32)
    buf.copy_(host)


def decode_spec_draft(state, refbuf, out, draft):
    """draft[0 .. S-2] (int32 [S - 1]) = the tokens that follow the best anchor of (out[t-2], out[t-1]) in the reference
    (lap_decode_spec_draft; `speculate.draft_tokens`)."""
    cap = _spec_out(out)
    _dreq(state, torch.int32, "state"); _dreq(refbuf, torch.int32, "refbuf"); _dreq(draft, torch.int32, "draft")
    if refbuf.numel() != cap + 1:
        raise TypeError(f"decode_spec_draft: the reference buffer holds {refbuf.numel() - 1} ids beside an out of {cap}")
    call("lap_decode_spec_draft", _p(state), refbuf.data_ptr() + 4, _p(refbuf), _p(out), cap, _p(draft), draft.numel() + 1)


def decode_spec_embed(state, table, row_lo, row_hi, out, draft, x, scale):
    """x [S, D]: row 0 embeds out[t-1], row r embeds draft[r-1] (lap_decode_spec_embed)."""
    cap = _spec_out(out)
    _dreq(x, torch.bfloat16, "x"); _dreq(table, torch.float32, "table"); _dreq(draft, torch.int32, "draft")
    if draft.numel() != x.shape[0] - 1:
        raise TypeError(f"decode_spec_embed: {draft.numel()} drafted tokens for {x.shape[0]} rows")
    call("lap_decode_spec_embed", _p(state), _p(table), int(row_lo), int(row_hi), _p(out), _p(draft), cap, _p(x), x.shape[0],
         x.shape[1], float(scale))


def decode_spec_qkv(state, x, gamma, wqkv, q, cache_k, cache_v, NH, HD, q_scale, eps=1e-6, wscale=None):
    """`decode_qkv` whose S rows are the positions t-1 .. t-1+S-1 of one sequence: cache_k / cache_v bf16 [cap, HD] (or [1, cap,
    HD]) of that sequence, q [S, NH * HD] (lap_decode_spec_qkv)."""
    for t, n in ((x, "x"), (q, "q"), (cache_k, "cache_k"), (cache_v, "cache_v")):
        _dreq(t, torch.bfloat16, n)
    _dreq(gamma, torch.float32, "gamma")
    S, D = x.shape
    if cache_k.numel() != cache_v.numel() or cache_k.numel() % HD or q.shape[0] != S:
        raise TypeError("decode_spec_qkv: caches [cap, HD] of one sequence and q of S rows")
    if wscale is not None:
        _f8req(wqkv, wscale, "wqkv")
    else:
        _dreq(wqkv, torch.bfloat16, "wqkv")
    call("lap_decode_spec_qkv", _p(state), _p(x), _p(gamma), _p(wqkv), _p(wscale), _p(q), _p(cache_k), _p(cache_v), S, D, NH, HD,
         cache_k.numel() // HD, float(q_scale), float(eps))


def decode_spec_attention(state, q, prefix_k, prefix_v, kinfo, Pn, cache_k, cache_v, o, scratch, NH, NKV, HD):
    """`decode_attention` whose row r is q row r against the prefix of sample 0 and min(t + r, cap) generated keys of the one
    sequence; scratch as `decode_attn_scratch(S, Pn, cap)` (lap_decode_spec_attention)."""
    for t, n in ((q, "q"), (prefix_k, "prefix_k"), (prefix_v, "prefix_v"), (cache_k, "cache_k"), (cache_v, "cache_v"), (o, "o")):
        _dreq(t, torch.bfloat16, n)
    _dreq(kinfo, torch.int32, "kinfo"); _dreq(scratch, torch.float32, "scratch")
    if prefix_k.numel() < Pn * HD or prefix_v.numel() < Pn * HD or kinfo.numel() < Pn or o.shape[0] != q.shape[0]:
        raise TypeError("decode_spec_attention: a prefix of Pn keys with its kinfo words, and o beside q")
    call("lap_decode_spec_attention", _p(state), _p(q), _p(prefix_k), _p(prefix_v), _p(kinfo), int(Pn), _p(cache_k), _p(cache_v),
         cache_k.numel() // HD, _p(o), _p(scratch), scratch.numel(), q.shape[0], NH, NKV, HD)


def decode_spec_accept(state, pval, pidx, draft, out, eos_token):
    """The finish of a verify step: the per-row argmax of the S = draft.numel() + 1 rows of partials, then the accept rule
    (lap_decode_spec_accept; `speculate.accept`)."""
    cap = _spec_out(out)
    _dreq(state, torch.int32, "state"); _dreq(pval, torch.float32, "pval"); _dreq(pidx, torch.int32, "pidx")
    _dreq(draft, torch.int32, "draft")
    S = draft.numel() + 1
    if pval.numel() < S * _fn["lap_decode_lm_blocks"]() or pidx.numel() < S * _fn["lap_decode_lm_blocks"]():
        raise TypeError("decode_spec_accept: pval / pidx hold [lap_decode_lm_blocks()][S] partials")
    call("lap_decode_spec_accept", _p(state), _p(pval), _p(pidx), _p(draft), _p(out), S, cap, int(eos_token))


# ---- teacher-forced scoring of one given sequence (csrc/decode_score.hip; lap_amd/score.py restates the quantity).  The candidate
# buffer is `decode_spec_ref`'s {length, ids[cap]}, filled by `decode_set_spec_ref`.
def _score_cand(cand):
    _dreq(cand, torch.int32, "cand")
    if cand.dim() != 1 or cand.numel() < 2:
        raise TypeError(f"cand: the candidate buffer int32 [1 + cap] of decode_spec_ref, got shape {tuple(cand.shape)}")
    return cand.numel() - 1


def decode_score_embed(state, table, row_lo, row_hi, cand, x, scale):
    """x [S, D]: row r embeds the candidate's ids[t-1+r]; a row at or past its length is zero (lap_decode_score_embed)."""
    cap = _score_cand(cand)
    _dreq(state, torch.int32, "state"); _dreq(x, torch.bfloat16, "x"); _dreq(table, torch.float32, "table")
    call("lap_decode_score_embed", _p(state), _p(table), int(row_lo), int(row_hi), _p(cand), cap, _p(x), x.shape[0], x.shape[1],
         float(scale))


def decode_lm_head_score(state, sampling, cand, x, gamma, hi, lo, pval, pidx, plp, logits=None, eps=1e-6, wscale=None, ids=None):
    """`decode_lm_head_lp` of the same arguments whose third plp word is the z of row b's target, the candidate's ids[t + b], in
    the block that owns it (-inf elsewhere), and whose pval / pidx are the greedy head's; `sampling` only carries the temperature
    (None: z = logit) (lap_decode_lm_head_score / _fp8)."""
    cap = _score_cand(cand)
    _dreq(state, torch.int32, "state"); _dreq(x, torch.bfloat16, "x"); _dreq(gamma, torch.float32, "gamma")
    _dreq(pval, torch.float32, "pval"); _dreq(pidx, torch.int32, "pidx"); _dreq(plp, torch.float32, "plp")
    if sampling is not None:
        _dreq(sampling, torch.int32, "sampling")
        if sampling.numel() < _fn["lap_decode_sampling_words"]():
            raise TypeError("sampling: int32 [lap_decode_sampling_words()]")
    if logits is not None:
        _dreq(logits, torch.float32, "logits")
    B, D = x.shape
    nblk = _fn["lap_decode_lm_blocks"]()
    if pval.numel() < B * nblk or pidx.numel() < B * nblk or plp.numel() < 3 * B * nblk:
        raise TypeError("decode_lm_head_score: pval / pidx hold [lap_decode_lm_blocks()][B] partials, plp [lap_decode_lm_blocks()][B][3]")
    if logits is not None and logits.numel() < B * hi.shape[0]:
        raise TypeError("decode_lm_head_score: logits holds f32 [B, V]")
    n = 0
    if ids is not None:
        _ids_req(ids, hi.shape[0])
        n = ids.numel()
    if wscale is not None:
        _f8req(hi, wscale, "hi")
        if lo is not None:
            raise TypeError("decode_lm_head_score: the fp8 table is one plane (lo must be None)")
        call("lap_decode_lm_head_score_fp8", _p(state), _p(sampling), _p(cand), cap, _p(x), _p(gamma), _p(hi), _p(wscale), _p(ids), n,
             B, D, hi.shape[0], float(eps), _p(logits), _p(pval), _p(pidx), _p(plp))
        return
    _dreq(hi, torch.bfloat16, "hi")
    if lo is not None:
        _dreq(lo, torch.bfloat16, "lo")
    call("lap_decode_lm_head_score", _p(state), _p(sampling), _p(cand), cap, _p(x), _p(gamma), _p(hi), _p(lo), _p(ids), n, B, D,
         hi.shape[0], float(eps), _p(logits), _p(pval), _p(pidx), _p(plp))


def decode_score_finish(state, pval, pidx, plp, cand, logp, greedy, S):
    """The finish of a score step of S rows: logp[t + r] and greedy[t + r] for r < n = min(S, length - t), t += n, done = t >=
    length, and the two counters (lap_decode_score_finish).  logp f32 / greedy int32 hold cap entries each."""
    cap = _score_cand(cand)
    _dreq(state, torch.int32, "state"); _dreq(pval, torch.float32, "pval"); _dreq(pidx, torch.int32, "pidx")
    _dreq(plp, torch.float32, "plp"); _dreq(logp, torch.float32, "logp"); _dreq(greedy, torch.int32, "greedy")
    S = int(S)
    nblk = _fn["lap_decode_lm_blocks"]()
    if not 1 <= S <= 8 or pval.numel() < S * nblk or pidx.numel() < S * nblk or plp.numel() < 3 * S * nblk:
        raise TypeError("decode_score_finish: 1 <= S <= 8 rows of partials [lap_decode_lm_blocks()][S] and plp [..][S][3]")
    if logp.numel() != cap or greedy.numel() != cap:
        raise TypeError(f"decode_score_finish: logp / greedy of {logp.numel()} / {greedy.numel()} entries beside a candidate buffer of {cap}")
    call("lap_decode_score_finish", _p(state), _p(pval), _p(pidx), _p(plp), _p(cand), _p(logp), _p(greedy), S, cap)


# ---- beam search over the rows of one fused decode batch (csrc/decode_beam.hip; lap_amd/beam.py restates the rules)
def decode_beam_init_words(N, early_stop, device):
    """The beam buffer of a fresh decode of N beams (lap_hip.h: scores {0, -inf, ...}, nothing finished, parent = own index, the
    early_stop flag, the reorder counter at zero): int32 [lap_decode_beam_words()].  A context copies it over its live buffer with
    a device op inside the prefill part, so a captured graph starts every request from it."""
    import numpy as np

    if not 1 <= int(N) <= 8:
        raise ValueError(f"decode_beam_init_words: 1 <= N <= 8, got {N}")
    words = np.zeros(_fn["lap_decode_beam_words"](), dtype=np.int32)
    scores = np.full(8, -np.inf, dtype=np.float32)
    scores[0] = 0.0
    words[0:8] = scores.view(np.int32)
    words[16:24] = np.arange(8)
    words[24] = 1 if early_stop else 0
    return torch.from_numpy(words).to(device)


def _beam_req(fn, state, beam, N):
    _dreq(state, torch.int32, "state"); _dreq(beam, torch.int32, "beam")
    if not 1 <= N <= 8:
        raise ValueError(f"{fn}: 1 <= N <= 8 beams, got {N}")
    if state.numel() < _fn["lap_decode_state_words"]() or beam.numel() < _fn["lap_decode_beam_words"]():
        raise TypeError(f"{fn}: state int32 [lap_decode_state_words()], beam int32 [lap_decode_beam_words()]")


def decode_beam_topn(state, beam, logits, cand_logp, cand_id, cap):
    """cand_logp / cand_id [N, N]: the N best (log-probability, id) of every row of the f32 `logits` [N, V] that the LM head of the
    step stored; id -1 where a row has fewer (lap_decode_beam_topn; `beam.row_topn`).  cap: the budget of the decode."""
    _dreq(logits, torch.float32, "logits"); _dreq(cand_logp, torch.float32, "cand_logp"); _dreq(cand_id, torch.int32, "cand_id")
    if logits.dim() != 2:
        raise TypeError(f"decode_beam_topn: logits [N, V], got {tuple(logits.shape)}")
    N, V = logits.shape
    _beam_req("decode_beam_topn", state, beam, N)
    if tuple(cand_logp.shape) != (N, N) or tuple(cand_id.shape) != (N, N):
        raise TypeError(f"decode_beam_topn: cand_logp / cand_id [{N}, {N}], got {tuple(cand_logp.shape)}, {tuple(cand_id.shape)}")
    call("lap_decode_beam_topn", _p(state), _p(beam), _p(logits), _p(cand_logp), _p(cand_id), N, V, int(cap))


def decode_beam_select(state, beam, cand_logp, cand_id, out, logp, V, eos_token):
    """The finish of a beam step (lap_decode_beam_select; `beam.beam_step`): the N best of the candidates become the beams in rank
    order; out / logp [N, cap] are permuted by parent up to t and get column t; the beam buffer, the EOS words, t and done move."""
    _dreq(cand_logp, torch.float32, "cand_logp"); _dreq(cand_id, torch.int32, "cand_id")
    _dreq(out, torch.int32, "out"); _dreq(logp, torch.float32, "logp")
    if out.dim() != 2 or tuple(logp.shape) != tuple(out.shape):
        raise TypeError(f"decode_beam_select: out [N, cap] with logp beside it, got {tuple(out.shape)}, {tuple(logp.shape)}")
    N, cap = out.shape
    _beam_req("decode_beam_select", state, beam, N)
    if tuple(cand_logp.shape) != (N, N) or tuple(cand_id.shape) != (N, N):
        raise TypeError(f"decode_beam_select: cand_logp / cand_id [{N}, {N}], got {tuple(cand_logp.shape)}, {tuple(cand_id.shape)}")
    call("lap_decode_beam_select", _p(state), _p(beam), _p(cand_logp), _p(cand_id), _p(out), _p(logp), N, int(V), cap, int(eos_token))


def decode_beam_reorder(state, beam, gen):
    """gen bf16 [depth, 2, N, cap, head_dim] (`decode_ctx.DecodeCtx.gen`): row b of every layer's K and V becomes row parent[b], in place, at
    the positions below t (lap_decode_beam_reorder); nothing moves when the parents are the identity."""
    _dreq(gen, torch.bfloat16, "gen")
    if gen.dim() != 5 or gen.shape[1] != 2 or gen.shape[4] % 8:
        raise TypeError(f"decode_beam_reorder: gen [depth, 2, N, cap, head_dim], head_dim a multiple of 8, got {tuple(gen.shape)}")
    depth, _, N, cap, HD = gen.shape
    _beam_req("decode_beam_reorder", state, beam, N)
    call("lap_decode_beam_reorder", _p(state), _p(beam), _p(gen), N, 2 * depth, cap, HD)


def _beam_cands(fn, N, cand_logp, cand_id, cand_next):
    _dreq(cand_logp, torch.float32, "cand_logp"); _dreq(cand_id, torch.int32, "cand_id"); _dreq(cand_next, torch.int32, "cand_next")
    if tuple(cand_logp.shape) != (N, N) or tuple(cand_id.shape) != (N, N) or tuple(cand_next.shape) != (N, N):
        raise TypeError(f"{fn}: cand_logp / cand_id / cand_next [{N}, {N}], got {tuple(cand_logp.shape)}, {tuple(cand_id.shape)}, "
                        f"{tuple(cand_next.shape)}")


def decode_beam_grammar_topn(state, beam, gstate, offsets, ids, nxt, logits, cand_logp, cand_id, cand_next, cap):
    """`decode_beam_topn` under a grammar (lap_decode_beam_grammar_topn; `beam.grammar_beam_step`): row b offers the N best edges of
    its automaton state gstate[b] (int32 [N]) from the f32 `logits` [N, V] that the SUBSET head over the automaton's union stored,
    with log-probabilities over that state's set; cand_next [N, N]: the state every candidate's edge leads to.  offsets, ids, nxt:
    the int32 device CSR of `grammar.TokenAutomaton.to_device`."""
    _dreq(logits, torch.float32, "logits"); _dreq(gstate, torch.int32, "gstate")
    if logits.dim() != 2:
        raise TypeError(f"decode_beam_grammar_topn: logits [N, V], got {tuple(logits.shape)}")
    N, V = logits.shape
    _beam_req("decode_beam_grammar_topn", state, beam, N)
    _automaton_req("decode_beam_grammar_topn", offsets, ids, nxt)
    if gstate.numel() != N:
        raise TypeError(f"decode_beam_grammar_topn: gstate [{N}], got {tuple(gstate.shape)}")
    _beam_cands("decode_beam_grammar_topn", N, cand_logp, cand_id, cand_next)
    call("lap_decode_beam_grammar_topn", _p(state), _p(beam), _p(gstate), _p(offsets), _p(ids), _p(nxt), offsets.numel() - 1, ids.numel(),
         _p(logits), _p(cand_logp), _p(cand_id), _p(cand_next), N, V, int(cap))


def decode_beam_grammar_select(state, beam, gstate, cand_logp, cand_id, cand_next, out, logp, V, eos_token):
    """`decode_beam_select` under a grammar (lap_decode_beam_grammar_select): also gstate[r] = the state of beam r after its token
    (its parent's old state when that parent had finished or beam r is padding)."""
    _dreq(out, torch.int32, "out"); _dreq(logp, torch.float32, "logp"); _dreq(gstate, torch.int32, "gstate")
    if out.dim() != 2 or tuple(logp.shape) != tuple(out.shape):
        raise TypeError(f"decode_beam_grammar_select: out [N, cap] with logp beside it, got {tuple(out.shape)}, {tuple(logp.shape)}")
    N, cap = out.shape
    _beam_req("decode_beam_grammar_select", state, beam, N)
    if gstate.numel() != N:
        raise TypeError(f"decode_beam_grammar_select: gstate [{N}], got {tuple(gstate.shape)}")
    _beam_cands("decode_beam_grammar_select", N, cand_logp, cand_id, cand_next)
    call("lap_decode_beam_grammar_select", _p(state), _p(beam), _p(gstate), _p(cand_logp), _p(cand_id), _p(cand_next), _p(out), _p(logp),
         N, int(V), cap, int(eos_token))
