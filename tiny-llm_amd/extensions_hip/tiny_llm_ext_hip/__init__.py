"""ctypes binding of ``libtinyllm_hip.so`` with the reference extension's Python surface.

Mirrors the nanobind module ``tiny_llm_ext_ref._ext``
(reference: src/extensions_ref/bindings.cpp:11-65): same function names, keyword
names and defaults, but the arrays are PyTorch-ROCm tensors and the kernels are
hand-written gfx950 HIP behind the C ABI declared in ``include/tinyllm_hip.h``.

Like the reference, the extension is GPU-only: every op raises ``RuntimeError``
for host tensors (reference ``eval_cpu`` throws, quantized_matmul.cpp:103-109),
and importing this module fails loudly when the shared library is missing.
There is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch

_LIB_NAME = "libtinyllm_hip.so"
_LIB_PATH = Path(__file__).resolve().parent / _LIB_NAME

if not _LIB_PATH.exists():
    raise ImportError(
        f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C tiny-llm_amd/csrc` (hipcc, gfx950). There is no CPU fallback."
    )

_lib = ctypes.CDLL(str(_LIB_PATH), mode=os.RTLD_LOCAL if hasattr(os, "RTLD_LOCAL") else 0)

_c_void_p = ctypes.c_void_p
_c_int = ctypes.c_int
_c_float = ctypes.c_float
_c_size_t = ctypes.c_size_t

TL_F32, TL_F16, TL_BF16 = 0, 1, 2
_DTYPES = {torch.float32: TL_F32, torch.float16: TL_F16, torch.bfloat16: TL_BF16}

# name -> (restype, argtypes); every symbol declared in include/tinyllm_hip.h and
# include/tinyllm_engine.h must appear here (tests/test_abi.py checks the headers).
_SIGNATURES = {
    "tl_last_error": (ctypes.c_char_p, []),
    "tl_abi_version": (_c_int, []),
    "tl_load_library": (_c_int, [ctypes.c_char_p]),
    "tl_quantized_matmul": (
        _c_int,
        [_c_void_p] * 5 + [_c_int] * 5 + [_c_int, _c_int, _c_int, _c_void_p, _c_size_t, _c_void_p],
    ),
    "tl_quantized_matmul_workspace_bytes": (_c_size_t, [_c_int] * 6),
    "tl_gather_quantized_matvec": (_c_int, [_c_void_p] * 6 + [_c_int] * 7 + [_c_void_p]),
    "tl_quantized_matmul_split_k": (_c_int, [_c_int] * 5),
    "tl_quantized_embedding": (_c_int, [_c_void_p, _c_int] + [_c_void_p] * 4 + [_c_int] * 6 + [_c_void_p]),
    "tl_rms_norm": (_c_int, [_c_void_p] * 3 + [_c_int, _c_int, _c_float, _c_int, _c_void_p]),
    "tl_rope": (_c_int, [_c_void_p] * 3 + [_c_int] * 5 + [_c_float, _c_int, _c_int, _c_void_p]),
    "tl_swiglu": (_c_int, [_c_void_p] * 3 + [_c_size_t, _c_int, _c_void_p]),
    "tl_decode_attention": (_c_int, [_c_void_p] * 5 + [_c_int] * 6 + [_c_float, _c_int, _c_int, _c_int, _c_void_p]),
    "tl_paged_cache_update": (_c_int, [_c_void_p] * 2 + [_c_int] * 8 + [_c_void_p]),
    "tl_paged_attention": (
        _c_int,
        [_c_void_p] * 6 + [_c_int] * 8 + [_c_float, _c_int, _c_int, _c_int, _c_void_p, _c_size_t, _c_void_p],
    ),
    "tl_paged_attention_workspace_bytes": (_c_size_t, [_c_int] * 8),
    "tl_paged_attention_waves": (_c_int, [_c_int]),
    # FP8 (E4M3) KV pages (include/tinyllm_hip.h, last operator section; no reference counterpart)
    "tl_kv_fp8_quantize_rows": (_c_int, [_c_void_p, _c_void_p, _c_void_p, ctypes.c_long, _c_int, _c_void_p]),
    "tl_kv_fp8_dequantize_rows": (_c_int, [_c_void_p, _c_void_p, _c_void_p, ctypes.c_long, _c_int, _c_void_p]),
    "tl_paged_cache_update_fp8": (_c_int, [_c_void_p] * 3 + [_c_int] * 7 + [_c_void_p]),
    "tl_paged_attention_fp8": (
        _c_int,
        [_c_void_p] * 8 + [_c_int] * 8 + [_c_float, _c_int, _c_int, _c_void_p, _c_size_t, _c_void_p],
    ),
}



# ---- decode engine ABI (include/tinyllm_engine.h) ------------------------------------------------
class TlW4(ctypes.Structure):
    _fields_ = [("weight_dev", _c_void_p), ("scales_dev", _c_void_p), ("biases_dev", _c_void_p),
                ("rows", _c_int), ("cols", _c_int)]


class TlLayerWeights(ctypes.Structure):
    _fields_ = [("wqkv", TlW4), ("wo", TlW4), ("wgu", TlW4), ("wdown", TlW4),
                ("input_norm_dev", _c_void_p), ("post_norm_dev", _c_void_p),
                ("q_norm_dev", _c_void_p), ("k_norm_dev", _c_void_p)]


class TlMoeWeights(ctypes.Structure):
    _fields_ = [("router", TlW4), ("gate_dev", _c_void_p), ("up_dev", _c_void_p), ("down_dev", _c_void_p),
                ("gate_scales_dev", _c_void_p), ("gate_biases_dev", _c_void_p), ("up_scales_dev", _c_void_p),
                ("up_biases_dev", _c_void_p), ("down_scales_dev", _c_void_p), ("down_biases_dev", _c_void_p),
                ("num_experts", _c_int), ("experts_per_token", _c_int), ("intermediate_size", _c_int),
                ("norm_topk_prob", _c_int)]


class TlEngineConfig(ctypes.Structure):
    _fields_ = [("hidden_size", _c_int), ("num_layers", _c_int), ("num_heads", _c_int), ("num_kv_heads", _c_int),
                ("head_dim", _c_int), ("intermediate_size", _c_int), ("vocab_size", _c_int),
                ("rope_theta", _c_float), ("rms_norm_eps", _c_float),
                ("page_size", _c_int), ("num_pages", _c_int), ("max_batch", _c_int), ("max_pages_per_seq", _c_int),
                ("max_prefill_rows", _c_int)]


class TlEngineStats(ctypes.Structure):
    _fields_ = [("pages_in_use", _c_int), ("pages_free", _c_int), ("peak_pages_in_use", _c_int),
                ("page_allocations", ctypes.c_long), ("reused_page_allocations", ctypes.c_long),
                ("decode_steps", ctypes.c_long), ("graph_captures", ctypes.c_long), ("graph_replays", ctypes.c_long),
                ("prefill_tokens", ctypes.c_long), ("kv_bytes", _c_size_t), ("workspace_bytes", _c_size_t),
                ("graph_cache_flushes", ctypes.c_long), ("aql_steps", ctypes.c_long)]


class TlStepProfile(ctypes.Structure):
    _fields_ = [("kernel_us", ctypes.c_double * 8), ("launches", _c_int * 8), ("gemv_bytes", ctypes.c_double * 5),
                ("span_us", ctypes.c_double), ("clock_khz", _c_int), ("n_splits", _c_int)]


class TlStepCheck(ctypes.Structure):
    _fields_ = [("launches", _c_int), ("written_once_plan", _c_int), ("n_splits", _c_int), ("double_writes", ctypes.c_long),
                ("elements_written", ctypes.c_long), ("first_launch", _c_int), ("first_kind", _c_int), ("first_region", _c_int),
                ("first_offset", ctypes.c_long)]


TL_MAX_TOP_LOGPROBS = 20
TL_MAX_LOGIT_BIAS = 1024  # entries of a slot's logit-bias list (include/tinyllm_engine.h)
TL_DRY_MAX_MATCH = 64     # the longest match DRY and the n-gram ban look at
TL_MAX_DRY_BREAKERS = 64  # entries of a slot's DRY breaker list
TL_LOOKUP_MAX_NGRAM = 16     # the longest match prompt lookup looks for
TL_LOOKUP_MAX_PROPOSALS = 7  # proposals per slot (a verification chunk holds the pending token and up to 7 more)


class TlTokenLogprob(ctypes.Structure):
    """tl_token_logprob (include/tinyllm_engine.h): the produced token's log-probability and the top-N entries (id -1 / -inf past N)."""
    _fields_ = [("logprob", ctypes.c_float), ("top_ids", ctypes.c_int32 * TL_MAX_TOP_LOGPROBS),
                ("top_logprobs", ctypes.c_float * TL_MAX_TOP_LOGPROBS)]


TL_MAX_BEAMS = 8
TL_MAX_BEAM_CANDIDATES = 32


class TlBeamCandidate(ctypes.Structure):
    """tl_beam_candidate (include/tinyllm_engine.h "Beam search"): parent -1 / token -1 / -inf / -inf past the rankable pairs."""
    _fields_ = [("parent", ctypes.c_int32), ("token", ctypes.c_int32), ("score", ctypes.c_float), ("logprob", ctypes.c_float)]


class TlLinearInfo(ctypes.Structure):
    _fields_ = [("kernel", _c_int), ("launches", _c_int), ("rows_per_pass", _c_int), ("p", _c_int * 5)]


class TlLinearEx(ctypes.Structure):
    _fields_ = [("merge_ws_dev", _c_void_p), ("n_splits", _c_int), ("ss_in_dev", _c_void_p), ("ss_in_n", _c_int),
                ("ss_out_dev", _c_void_p), ("norm_out_dev", _c_void_p), ("out_w_dev", _c_void_p), ("fragment_order", _c_int)]


class TlPrefixStats(ctypes.Structure):
    """tl_prefix_stats (include/tinyllm_engine.h): the prefix cache's counters."""
    _fields_ = [("lookups", ctypes.c_long), ("hits", ctypes.c_long), ("tokens_matched", ctypes.c_long),
                ("tail_rows_copied", ctypes.c_long), ("pages_registered", ctypes.c_long), ("pages_evicted", ctypes.c_long),
                ("entries", _c_int), ("pages_retained", _c_int), ("max_retained_pages", _c_int), ("enabled", _c_int)]


class TlKvPoolDesc(ctypes.Structure):
    """tl_kv_pool_desc: one pool [pages][heads][page_size][row_bytes] of tl_kv_copy_rows' device table."""
    _fields_ = [("base_dev", _c_void_p), ("row_bytes", _c_size_t)]


class TlSwapStats(ctypes.Structure):
    """tl_swap_stats (include/tinyllm_engine.h): the swap space's records and the park / unpark counters."""
    _fields_ = [("host_pages", _c_int), ("host_pages_in_use", _c_int), ("parks", ctypes.c_long), ("unparks", ctypes.c_long),
                ("pages_out", ctypes.c_long), ("pages_in", ctypes.c_long), ("record_bytes", _c_size_t)]


TL_MAX_LORA_RANK = 64
TL_MAX_LORA_ADAPTERS = 32
LORA_TARGETS = ("q", "k", "v", "o", "gate", "up", "down")  # TL_LORA_Q .. TL_LORA_DOWN
LORA_MODES = {"add": 0, "residual_pre": 1, "swiglu": 2}    # TL_LORA_ADD, TL_LORA_RESIDUAL_PRE, TL_LORA_SWIGLU
LORA_SEG_MODES = {"plain": 0, "blocks": 1, "interleaved": 2}


class TlLoraLayer(ctypes.Structure):
    """tl_lora_layer: per target (LORA_TARGETS) the device matrices A [rank, in] and B [out, rank], bf16; a NULL pair = not adapted."""
    _fields_ = [("a_dev", _c_void_p * len(LORA_TARGETS)), ("b_dev", _c_void_p * len(LORA_TARGETS))]


class TlLoraStats(ctypes.Structure):
    """tl_lora_stats (include/tinyllm_engine.h): resident adapters, their device bytes, adapter decode steps, adapter prefill rows."""
    _fields_ = [("resident", _c_int), ("bytes", _c_size_t), ("adapter_steps", ctypes.c_long), ("adapter_prefill_rows", ctypes.c_long)]


class TlLoraMatrices(ctypes.Structure):
    """tl_lora_matrices: one adapter of tl_lora_rows in the fused layout -- A [rank * present segments, in], B [out, rank]."""
    _fields_ = [("a_dev", _c_void_p), ("b_dev", _c_void_p), ("rank", _c_int), ("seg_mask", _c_int), ("scale", _c_float)]


TL_MAX_STOP_IDS = 16
TL_MAX_STOP_STRINGS = 16
TL_MAX_STOP_BYTES = 1024
STOP_REASONS = ("none", "id", "string", "length")  # TL_STOP_NONE .. TL_STOP_LENGTH


class TlStopState(ctypes.Structure):
    """tl_stop_state (include/tinyllm_engine.h): a slot's stop record -- reason (STOP_REASONS), index into the set's ids / strings,
    tokens examined since arming, context length, text bytes since arming and the bytes ahead of the matched string."""
    _fields_ = [("reason", ctypes.c_int32), ("index", ctypes.c_int32), ("generated", ctypes.c_int32), ("context", ctypes.c_int32),
                ("text_bytes", ctypes.c_uint32), ("cut_bytes", ctypes.c_uint32)]


class TlAttentionInfo(ctypes.Structure):
    _fields_ = [("n_splits", _c_int), ("tokens_per_split", _c_int), ("heads_per_workgroup", _c_int),
                ("launches", _c_int)]


class TlVerifyResult(ctypes.Structure):
    """tl_verify_result (include/tinyllm_engine.h): one sequence of tl_engine_verify_batch -- ``count`` ids, the accepted proposals
    followed by the correction or the bonus token (-1 behind them)."""
    _fields_ = [("count", ctypes.c_int32), ("ids", ctypes.c_int32 * 8)]


_P = ctypes.POINTER
_SIGNATURES.update({
    "tl_tiled_w4_create": (_c_int, [_P(TlW4), _c_void_p, _P(_c_void_p)]),
    "tl_tiled_w4_destroy": (None, [_c_void_p]),
    "tl_decode_linear_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "tl_decode_linear": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_float,
                                  _c_int, _c_void_p, _c_size_t, _c_void_p, _P(TlLinearInfo)]),
    "tl_decode_linear_ex": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_float,
                                     _c_int, _c_void_p, _c_size_t, _c_void_p, _P(TlLinearEx), _P(TlLinearInfo)]),
    "tl_prefill_weights_bf16": (_c_int, [_P(TlW4), _c_void_p, _c_void_p]),
    "tl_prefill_matmul_bf16": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p]),
    "tl_decode_gemv_variant_compiled": (_c_int, [_c_int, _c_int, _c_int, _c_int]),
    "tl_decode_attention_fused_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int]),
    "tl_decode_attention_fused": (_c_int, [_c_void_p] * 8 + [_c_int] * 6 + [_c_float, _c_float, _c_int, _c_void_p, _c_size_t,
                                                             _c_void_p, _P(TlAttentionInfo)]),
    "tl_engine_profile_step": (_c_int, [_c_void_p, _c_int, _P(TlStepProfile)]),
    "tl_engine_check_step": (_c_int, [_c_void_p, _c_int, _P(TlStepCheck)]),
    "tl_engine_create": (_c_int, [_P(TlEngineConfig), _P(TlLayerWeights), _P(TlW4), _c_void_p, _P(TlW4), _c_void_p,
                                  _P(_c_void_p)]),
    "tl_engine_create_kv": (_c_int, [_P(TlEngineConfig), _P(TlLayerWeights), _P(TlW4), _c_void_p, _P(TlW4), _c_void_p, _c_int,
                                     _P(_c_void_p)]),
    "tl_engine_kv_format": (_c_int, [_c_void_p]),
    "tl_decode_attention_fused_fp8": (_c_int, [_c_void_p] * 10 + [_c_int] * 6 + [_c_float, _c_float, _c_int, _c_void_p, _c_size_t,
                                                                  _c_void_p, _P(TlAttentionInfo)]),
    "tl_engine_set_moe_layer": (_c_int, [_c_void_p, _c_int, _P(TlMoeWeights)]),
    "tl_decode_gemv_plan": (_c_int, [_c_int, _c_int, _c_int, _P(_c_int)]),
    "tl_decode_batched_plan": (_c_int, [_c_int, _c_int, _c_int, _P(_c_int)]),
    "tl_decode_batched_variant_compiled": (_c_int, [_c_int, _c_int]),
    "tl_decode_streaming_plan": (_c_int, [_c_int, _c_int, _c_int, _P(_c_int)]),
    "tl_decode_streaming_variant_compiled": (_c_int, [_c_int, _c_int]),
    "tl_decode_attention_plan": (_c_int, [_c_int, _c_int, _c_int, _c_int, _P(_c_int)]),
    "tl_engine_set_option": (_c_int, [_c_void_p, ctypes.c_char_p, _c_int]),
    "tl_engine_destroy": (None, [_c_void_p]),
    "tl_engine_synchronize": (_c_int, [_c_void_p]),
    "tl_engine_begin": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_reserve": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_release": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_rewind": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_context_len": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_move": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_fork": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_read_pending": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32)]),
    "tl_engine_prefix_cache": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_prefix_attach": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _c_int, _P(_c_int)]),
    "tl_engine_prefix_extend": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _c_int]),
    "tl_engine_prefix_clear": (_c_int, [_c_void_p]),
    "tl_engine_prefix_stats": (_c_int, [_c_void_p, _P(TlPrefixStats)]),
    "tl_kv_copy_rows": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p]),
    "tl_engine_swap_space": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_park": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_unpark": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_slot_parked": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_step_pages": (_c_int, [_c_void_p, _c_int, _P(_c_int), _P(_c_int)]),
    "tl_engine_swap_stats": (_c_int, [_c_void_p, _P(TlSwapStats)]),
    "tl_kv_page_record_bytes": (_c_size_t, [_c_void_p, _c_int, _c_int, _c_int]),
    "tl_kv_gather_pages": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p, _c_size_t, _c_void_p]),
    "tl_kv_scatter_pages": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p, _c_size_t, _c_void_p]),
    "tl_engine_prefill": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _c_int, _c_int]),
    "tl_engine_prefill_packed": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int), _P(ctypes.c_int32), _P(ctypes.c_int), _P(ctypes.c_int)]),
    "tl_engine_verify": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _c_int, _P(ctypes.c_int32)]),
    "tl_engine_verify_sampled": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _c_int, _c_void_p, ctypes.c_float, _c_int, ctypes.c_float,
                                          _P(ctypes.c_int32), _P(_c_int)]),
    "tl_engine_verify_batch": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int), _P(ctypes.c_int32), _P(ctypes.c_int), _c_int, _P(TlVerifyResult)]),
    "tl_verify_attention_rows": (_c_int, [_c_void_p] * 8 + [_c_int, _P(ctypes.c_int), _P(ctypes.c_int), _P(ctypes.c_int), _c_void_p] + [_c_int] * 4 +
                                 [_c_float, _c_float, _c_void_p, _P(TlAttentionInfo)]),
    "tl_verify_accept_rows": (_c_int, [_c_void_p, _c_int, _c_int, _P(ctypes.c_int), _P(ctypes.c_int), _c_void_p, _c_void_p, _c_void_p]),
    "tl_engine_verify_batch_sampled": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int), _P(ctypes.c_int32), _P(ctypes.c_int), _c_void_p, ctypes.c_float,
                                                _c_int, ctypes.c_float, _c_int, _P(TlVerifyResult)]),
    "tl_engine_copy_verify_logits": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p]),
    "tl_verify_sample_rows": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int, _P(ctypes.c_int), _P(ctypes.c_int), _P(ctypes.c_int)] + [_c_void_p] * 5 +
                              [ctypes.c_float, _c_int, ctypes.c_float, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "tl_engine_lookup_propose_sampled": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int), _P(ctypes.c_int), _c_int, _c_int, _c_int, _P(ctypes.c_int32),
                                                  _P(ctypes.c_int)]),
    "tl_engine_set_token": (_c_int, [_c_void_p, _c_int, ctypes.c_int32]),
    "tl_engine_set_lookup": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_lookup_propose": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int), _P(ctypes.c_int), _c_int, _c_int, _c_int, _P(ctypes.c_int32),
                                          _P(ctypes.c_int)]),
    "tl_engine_lookup_state": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int), _P(ctypes.c_int), _P(ctypes.c_int)]),
    "tl_lookup_rows": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "tl_engine_set_sampling": (_c_int, [_c_void_p, _c_int, _c_float, _c_int, _c_float, ctypes.c_uint64]),
    "tl_sample_logits": (_c_int, [_c_void_p, _c_int, _c_int] + [_c_void_p] * 7),
    "tl_engine_set_logprobs": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_set_penalties": (_c_int, [_c_void_p, _c_int, _c_float, _c_float, _c_float]),
    "tl_engine_set_logit_bias": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _P(_c_float), _c_int]),
    "tl_process_logits": (_c_int, [_c_void_p, _c_int, _c_int] + [_c_void_p] * 9),
    "tl_engine_set_dry": (_c_int, [_c_void_p, _c_int, _c_float, _c_float, _c_int, _c_int, _c_int, _P(ctypes.c_int32), _c_int]),
    "tl_dry_rows": (_c_int, [_c_void_p, _c_int, _c_int] + [_c_void_p] * 11 + [_c_int, _c_void_p]),
    "tl_engine_set_truncation": (_c_int, [_c_void_p, _c_int, _c_float, _c_float]),
    "tl_engine_set_mirostat": (_c_int, [_c_void_p, _c_int, _c_float, _c_float]),
    "tl_engine_mirostat_mu": (_c_int, [_c_void_p, _c_int, _P(_c_float)]),
    "tl_engine_copy_filtered_logits": (_c_int, [_c_void_p, _c_void_p, _c_int]),
    "tl_truncate_rows": (_c_int, [_c_void_p, _c_int, _c_int] + [_c_void_p] * 7),
    "tl_spec_sample_rows": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_int] + [_c_void_p] * 12),
    "tl_mirostat_update_rows": (_c_int, [_c_void_p, _c_int, _c_int] + [_c_void_p] * 7),
    "tl_vocab_create": (_c_int, [_c_int, _c_void_p, _c_void_p, _c_void_p, _P(_c_void_p)]),
    "tl_vocab_destroy": (None, [_c_void_p]),
    "tl_grammar_create": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _P(_c_void_p)]),
    "tl_grammar_destroy": (None, [_c_void_p]),
    "tl_engine_set_grammar": (_c_int, [_c_void_p, _c_int, _c_void_p]),
    "tl_engine_grammar_state": (_c_int, [_c_void_p, _c_int, _P(_c_int), _P(_c_int)]),
    "tl_grammar_mask_rows": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "tl_grammar_create_stack": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int,
                                         _c_void_p, _P(_c_void_p)]),
    "tl_engine_grammar_config": (_c_int, [_c_void_p, _c_int, _P(_c_int), _P(_c_int), _P(ctypes.c_uint64), _P(_c_int)]),
    "tl_grammar_mask_rows_stack": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "tl_engine_read_logprobs": (_c_int, [_c_void_p, _c_int, _c_int, _P(TlTokenLogprob)]),
    "tl_engine_read_pending_logprobs": (_c_int, [_c_void_p, _c_int, _P(TlTokenLogprob)]),
    "tl_engine_score": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _c_int, ctypes.c_int32, _P(_c_float), _P(ctypes.c_int32)]),
    "tl_logprob_rows": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "tl_beam_rows": (_c_int, [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p]),
    "tl_engine_beam_select": (_c_int, [_c_void_p, _c_int, _c_int, _P(_c_float), _c_int, _P(TlBeamCandidate)]),
    "tl_engine_beam_reorder": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _P(ctypes.c_int), _P(ctypes.c_int32)]),
    "tl_engine_embed_packed": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int), _P(ctypes.c_int32), _P(ctypes.c_int), _P(ctypes.c_int), _c_int, _c_int,
                                        _c_int, _P(_c_float)]),
    "tl_engine_embed": (_c_int, [_c_void_p, _c_int, _P(ctypes.c_int32), _c_int, _c_int, _c_int, _c_int, _c_int, _P(_c_float)]),
    "tl_pool_rows": (_c_int, [_c_void_p, _c_int, _c_int, _P(ctypes.c_int), _P(ctypes.c_int), _P(ctypes.c_int), _P(ctypes.c_int), _c_int, _c_void_p,
                              _c_int, _c_int, _c_void_p, _c_void_p]),
    "tl_moe_route_rows": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p]),
    "tl_moe_experts_workspace_bytes": (_c_size_t, [_c_int, _c_int, _c_int, _c_int]),
    "tl_moe_experts_rows": (_c_int, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _P(TlMoeWeights), _c_int, _c_int, _c_void_p, _c_void_p, _c_size_t,
                                     _c_void_p]),
    "tl_engine_lora_load": (_c_int, [_c_void_p, _P(TlLoraLayer), _c_int, _c_float, _P(_c_int)]),
    "tl_engine_lora_unload": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_set_lora": (_c_int, [_c_void_p, _c_int, _c_int]),
    "tl_engine_slot_lora": (_c_int, [_c_void_p, _c_int]),
    "tl_engine_lora_stats": (_c_int, [_c_void_p, _P(TlLoraStats)]),
    "tl_lora_rows": (_c_int, [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _P(TlLoraMatrices), _c_int, _c_int, _c_int, _c_int, _P(ctypes.c_int),
                              _P(ctypes.c_int), _P(ctypes.c_int), _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_float, _c_void_p]),
    "tl_stop_create": (_c_int, [_c_void_p, _P(ctypes.c_int32), _c_int, _c_void_p, _P(ctypes.c_int32), _c_int, _c_void_p, _P(_c_void_p)]),
    "tl_stop_destroy": (None, [_c_void_p]),
    "tl_engine_set_stop": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_int]),
    "tl_engine_stop_state": (_c_int, [_c_void_p, _c_int, _P(TlStopState)]),
    "tl_stop_rows": (_c_int, [_c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "tl_engine_decode": (_c_int, [_c_void_p, _c_int, _c_int, _c_int]),
    "tl_engine_read_tokens": (_c_int, [_c_void_p, _c_int, _c_int, _P(ctypes.c_int32)]),
    "tl_engine_logits_dev": (_c_void_p, [_c_void_p]),
    "tl_engine_copy_logits": (_c_int, [_c_void_p, _c_void_p, _c_int]),
    "tl_engine_copy_processed_logits": (_c_int, [_c_void_p, _c_void_p, _c_int]),
    "tl_engine_tokens_dev": (_c_void_p, [_c_void_p]),
    "tl_engine_get_stats": (_c_int, [_c_void_p, _P(TlEngineStats)]),
    "tl_engine_replay_route": (ctypes.c_char_p, [_c_void_p]),
    "tl_engine_step_bytes": (_c_size_t, [_c_void_p, _c_int]),
})

for _name, (_res, _args) in _SIGNATURES.items():
    _fn = getattr(_lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args


def _bind_optional(name: str, restype, argtypes) -> bool:
    fn = getattr(_lib, name, None)
    if fn is None:
        return False
    fn.restype = restype
    fn.argtypes = argtypes
    return True


def lib() -> ctypes.CDLL:
    """The loaded shared library (used by the decode engine binding)."""
    return _lib


def check(status: int) -> None:
    """Raise RuntimeError(tl_last_error()) for a non-zero tl_status."""
    _check(status)


def library_path() -> str:
    return str(_LIB_PATH)


def _check(status: int) -> None:
    if status != 0:
        message = _lib.tl_last_error()
        raise RuntimeError(message.decode() if message else f"tinyllm_hip error {status}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_gpu(op: str, *tensors: torch.Tensor) -> None:
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{op}: the course extension is GPU-only")


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


_workspaces: dict[tuple[int, int], torch.Tensor] = {}


def _workspace(nbytes: int, device: torch.device) -> torch.Tensor | None:
    """Per-(device, stream) scratch buffer; grows geometrically, reused across calls."""
    if nbytes <= 0:
        return None
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def load_library(path: str) -> None:
    """reference: load_library(path) registers the metallib (utils.cpp:9-14). Here: verify a gfx950 device."""
    _check(_lib.tl_load_library(str(path).encode()))


def quantized_matmul(
    scales: torch.Tensor,
    biases: torch.Tensor,
    group_size: int,
    bits: int,
    a: torch.Tensor,
    b: torch.Tensor,
    transpose_b: bool = False,
    use_simdgroup: bool = True,
    use_split_k: bool = False,
    stream=None,
) -> torch.Tensor:
    """W4A16 ``a[M,N] @ dequant(b[K,N/8]).T`` (reference quantized_matmul.cpp:14-80 for the checks)."""
    if scales.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("quantized_matmul: scales must be float16 or bfloat16")
    if scales.dtype != biases.dtype:
        raise RuntimeError("quantized_matmul: scales and biases must be the same dtype")
    if b.dtype not in (torch.uint32, torch.int32):
        raise RuntimeError("quantized_matmul: b must be uint32")
    if a.dtype != scales.dtype:
        raise RuntimeError("quantized_matmul: a must be the same dtype as scales")
    if a.dim() != 2:
        raise RuntimeError("quantized_matmul: a must be a 2D array")
    if b.dim() != 2:
        raise RuntimeError("quantized_matmul: b must be a 2D array")
    if bits != 4:
        raise RuntimeError("quantized_matmul: bits must be 4")
    if group_size != 128:
        raise RuntimeError("quantized_matmul: group_size must be 128")
    if not transpose_b:
        raise RuntimeError("quantized_matmul: b must be transposed")
    if scales.shape != biases.shape:
        raise RuntimeError("quantized_matmul: scales and biases must have the same shape")
    if b.shape[0] != scales.shape[0]:
        raise RuntimeError("quantized_matmul: b must have the same number of rows as scales")
    M, N = a.shape
    K = b.shape[0]
    if N % group_size != 0:
        raise RuntimeError("quantized_matmul: a columns must be divisible by group_size")
    if scales.dim() != 2 or scales.shape[1] != N // group_size:
        raise RuntimeError("quantized_matmul: scales must have one column per input group")
    if b.shape[1] != N // 8:
        raise RuntimeError("quantized_matmul: a must have the same number of columns as b")
    _require_gpu("quantized_matmul", scales, biases, a, b)
    if not a.is_contiguous():
        raise RuntimeError("quantized_matmul: a must be contiguous")
    if not b.is_contiguous():
        raise RuntimeError("quantized_matmul: b must be contiguous")
    scales = scales.contiguous()
    biases = biases.contiguous()
    dt = _DTYPES[a.dtype]
    out = torch.empty((M, K), dtype=a.dtype, device=a.device)
    ws_bytes = _lib.tl_quantized_matmul_workspace_bytes(M, N, K, dt, int(use_simdgroup), int(use_split_k))
    ws = _workspace(ws_bytes, a.device)
    _check(
        _lib.tl_quantized_matmul(
            _ptr(scales), _ptr(biases), _ptr(a), _ptr(b), _ptr(out), M, N, K, group_size, bits, dt,
            int(use_simdgroup), int(use_split_k), _ptr(ws) if ws is not None else None,
            ws.numel() if ws is not None else 0, _stream(),
        )
    )
    return out


def gather_quantized_matvec(scales: torch.Tensor, biases: torch.Tensor, group_size: int, bits: int, a: torch.Tensor,
                            b: torch.Tensor, expert_ids: torch.Tensor, stream=None) -> torch.Tensor:
    """Grouped-expert W4A16 product ``out[m] = a[m] @ dequant(b[expert_ids[m]]).T`` (what the reference gets from
    ``mx.gather_qmm`` in grouped_expert_linear, src/tiny_llm_ref/moe.py:7-36).  b [E,K,N/8], scales/biases [E,K,N/128],
    a [M,N], expert_ids [M] int32 on the device."""
    if scales.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("gather_quantized_matvec: scales must be float16 or bfloat16")
    if scales.dtype != biases.dtype or a.dtype != scales.dtype:
        raise RuntimeError("gather_quantized_matvec: scales, biases and a must share one dtype")
    if b.dtype not in (torch.uint32, torch.int32):
        raise RuntimeError("gather_quantized_matvec: b must be uint32")
    if bits != 4 or group_size != 128:
        raise RuntimeError("gather_quantized_matvec: only 4-bit weights in groups of 128 are supported")
    if a.dim() != 2 or b.dim() != 3 or scales.dim() != 3 or scales.shape != biases.shape:
        raise RuntimeError("gather_quantized_matvec: expected a [M,N], b [E,K,N/8], scales/biases [E,K,N/128]")
    M, N = a.shape
    E, K = b.shape[0], b.shape[1]
    if N % group_size != 0 or b.shape[2] != N // 8 or tuple(scales.shape) != (E, K, N // group_size):
        raise RuntimeError("gather_quantized_matvec: shapes of a, b and scales do not describe one [E,K,N] weight stack")
    if expert_ids.dtype != torch.int32 or tuple(expert_ids.shape) != (M,):
        raise RuntimeError("gather_quantized_matvec: expert_ids must be int32 with one entry per row of a")
    _require_gpu("gather_quantized_matvec", scales, biases, a, b, expert_ids)
    for name, t in (("a", a), ("b", b), ("scales", scales), ("biases", biases), ("expert_ids", expert_ids)):
        if not t.is_contiguous():
            raise RuntimeError(f"gather_quantized_matvec: {name} must be contiguous")
    out = torch.empty((M, K), dtype=a.dtype, device=a.device)
    _check(_lib.tl_gather_quantized_matvec(_ptr(scales), _ptr(biases), _ptr(a), _ptr(b), _ptr(expert_ids), _ptr(out), M, N,
                                           K, E, int(group_size), int(bits), _DTYPES[a.dtype], _stream()))
    return out


def quantized_embedding(
    indices: torch.Tensor,
    scales: torch.Tensor,
    biases: torch.Tensor,
    weight: torch.Tensor,
    group_size: int,
    bits: int,
    stream=None,
) -> torch.Tensor:
    """Gather + dequantize rows of a packed table (reference quantized_matmul.cpp:82-101)."""
    if indices.dtype not in (torch.int32, torch.uint32) or weight.dtype not in (torch.uint32, torch.int32):
        raise RuntimeError("quantized_embedding: indices and weight must use 32-bit integers")
    if scales.dtype != biases.dtype or scales.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("quantized_embedding: scales and biases must have the same 16-bit dtype")
    if group_size != 128 or bits != 4 or scales.shape != biases.shape:
        raise RuntimeError("quantized_embedding: expected 4-bit weights with group size 128")
    dim = weight.shape[1] * 8
    if scales.shape[0] != weight.shape[0] or scales.shape[1] != dim // group_size:
        raise RuntimeError("quantized_embedding: incompatible parameter shapes")
    _require_gpu("quantized_embedding", indices, scales, biases, weight)
    indices = indices.contiguous()
    out = torch.empty((*indices.shape, dim), dtype=scales.dtype, device=scales.device)
    _check(
        _lib.tl_quantized_embedding(
            _ptr(indices), int(indices.dtype == torch.uint32), _ptr(scales.contiguous()), _ptr(biases.contiguous()),
            _ptr(weight.contiguous()), _ptr(out), indices.numel(), dim, weight.shape[0], group_size, bits,
            _DTYPES[scales.dtype], _stream(),
        )
    )
    return out


def _require_float(x: torch.Tensor, name: str) -> None:
    if x.dtype not in _DTYPES:
        raise RuntimeError(f"{name}: expected float32, float16, or bfloat16")


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float, stream=None) -> torch.Tensor:
    """Fused RMSNorm over the last dim (reference week2_kernels.cpp:36-42)."""
    _require_float(x, "rms_norm")
    if x.dtype != weight.dtype or weight.dim() != 1 or weight.shape[0] != x.shape[-1]:
        raise RuntimeError("rms_norm: weight must match the input dtype and final dimension")
    _require_gpu("rms_norm", x, weight)
    x = x.contiguous()
    weight = weight.contiguous()
    out = torch.empty_like(x)
    dim = x.shape[-1]
    rows = x.numel() // dim if dim else 0
    _check(_lib.tl_rms_norm(_ptr(x), _ptr(weight), _ptr(out), rows, dim, float(eps), _DTYPES[x.dtype], _stream()))
    return out


def rope(
    x: torch.Tensor, offsets: torch.Tensor, dims: int, base: float, traditional: bool = False, stream=None
) -> torch.Tensor:
    """Fused RoPE, x=[B,L,H,D], one int32 offset per batch row (reference week2_kernels.cpp:44-55)."""
    _require_float(x, "rope")
    if x.dim() != 4 or offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] != x.shape[0]:
        raise RuntimeError("rope: expected x=[B,L,H,D] and one int32 offset per batch row")
    if dims <= 0 or dims > x.shape[3] or dims % 2 != 0:
        raise RuntimeError("rope: dims must be positive, even, and no larger than the head dimension")
    _require_gpu("rope", x, offsets)
    x = x.contiguous()
    offsets = offsets.contiguous()
    out = torch.empty_like(x)
    B, L, H, D = x.shape
    _check(
        _lib.tl_rope(_ptr(x), _ptr(offsets), _ptr(out), B, L, H, D, int(dims), float(base), int(bool(traditional)),
                     _DTYPES[x.dtype], _stream())
    )
    return out


def swiglu(gate: torch.Tensor, up: torch.Tensor, stream=None) -> torch.Tensor:
    """``silu(gate) * up`` (reference week2_kernels.cpp:57-63)."""
    _require_float(gate, "swiglu")
    if gate.dtype != up.dtype or gate.shape != up.shape:
        raise RuntimeError("swiglu: gate and up must have the same shape and dtype")
    _require_gpu("swiglu", gate, up)
    gate = gate.contiguous()
    up = up.contiguous()
    out = torch.empty_like(gate)
    _check(_lib.tl_swiglu(_ptr(gate), _ptr(up), _ptr(out), gate.numel(), _DTYPES[gate.dtype], _stream()))
    return out


def decode_attention(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    mask: torch.Tensor,
    scale: float,
    is_causal: bool,
    has_mask: bool,
    num_heads: int,
    num_kv_heads: int,
    stream=None,
) -> torch.Tensor:
    """Dense-KV online-softmax GQA attention (reference week2_kernels.cpp:65-84)."""
    _require_float(query, "decode_attention")
    if query.dtype != key.dtype or query.dtype != value.dtype or mask.dtype != torch.float32:
        raise RuntimeError("decode_attention: q, k, and v dtypes must match; mask must be float32")
    if (
        query.dim() != 3 or key.dim() != 3 or value.dim() != 3 or query.shape[2] > 256
        or query.shape[2] != key.shape[2] or query.shape[2] != value.shape[2] or key.shape != value.shape
        or num_heads % num_kv_heads != 0
    ):
        raise RuntimeError("decode_attention: incompatible attention shapes")
    if has_mask and (
        mask.dim() != 3 or mask.shape[0] != query.shape[0] or mask.shape[1] != query.shape[1]
        or mask.shape[2] != key.shape[1]
    ):
        raise RuntimeError("decode_attention: mask must have shape [B*Hq,L,S]")
    _require_gpu("decode_attention", query, key, value)
    if has_mask:
        _require_gpu("decode_attention", mask)
    query, key, value, mask = query.contiguous(), key.contiguous(), value.contiguous(), mask.contiguous()
    out = torch.empty_like(query)
    q_rows, L, D = query.shape
    S = key.shape[1]
    _check(
        _lib.tl_decode_attention(
            _ptr(query), _ptr(key), _ptr(value), _ptr(mask) if has_mask else None, _ptr(out), q_rows, L, S, D,
            int(num_heads), int(num_kv_heads), float(scale), int(bool(is_causal)), int(bool(has_mask)),
            _DTYPES[query.dtype], _stream(),
        )
    )
    return out


def paged_cache_update(pages: torch.Tensor, values: torch.Tensor, page_id: int, start: int, stream=None) -> torch.Tensor:
    """In-place write of ``values[1,H,len,D]`` into ``pages[P,H,page,D]``; returns ``pages`` itself
    (the reference output aliases the input buffer, paged_attention.cpp:46-49)."""
    if pages.dtype not in (torch.float32, torch.bfloat16) or values.dtype != pages.dtype:
        raise RuntimeError("paged_cache_update: pages and values must have the same float32 or bfloat16 dtype")
    if pages.dim() != 4 or values.dim() != 4 or values.shape[0] != 1:
        raise RuntimeError("paged_cache_update: expected pages [P, H, page_size, D] and values [1, H, length, D]")
    if values.shape[1] != pages.shape[1] or values.shape[3] != pages.shape[3]:
        raise RuntimeError("paged_cache_update: values must match the page head count and head dimension")
    if page_id < 0 or page_id >= pages.shape[0] or start < 0 or start + values.shape[2] > pages.shape[2]:
        raise RuntimeError("paged_cache_update: destination slice is outside page storage")
    _require_gpu("paged_cache_update", pages, values)
    if not pages.is_contiguous() or not values.is_contiguous():
        raise RuntimeError("paged_cache_update: pages and values must be contiguous")
    P, H, page_size, D = pages.shape
    _check(
        _lib.tl_paged_cache_update(_ptr(pages), _ptr(values), P, H, page_size, D, values.shape[2], int(page_id),
                                   int(start), _DTYPES[pages.dtype], _stream())
    )
    return pages


def paged_attention(
    query: torch.Tensor,
    key_pages: torch.Tensor,
    value_pages: torch.Tensor,
    block_table: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float = 1.0,
    is_causal: bool = False,
    *,
    num_kv_heads: int,
    num_heads: int,
    stream=None,
    max_context_hint: int = 0,
) -> torch.Tensor:
    """Block-table attention over paged K/V (reference paged_attention.cpp:77-122 for the checks).

    ``max_context_hint`` (extension of the reference signature) is a host-known upper
    bound of ``context_lens`` used only to size the context split of the decode kernel.
    """
    if query.dtype not in (torch.float32, torch.bfloat16) or key_pages.dtype != query.dtype \
            or value_pages.dtype != query.dtype:
        raise RuntimeError(
            "paged_attention: q, key_pages, and value_pages must have the same float32 or bfloat16 dtype")
    if block_table.dtype != torch.int32 or context_lens.dtype != torch.int32:
        raise RuntimeError("paged_attention: block_table and context_lens must be int32")
    if query.dim() != 3:
        raise RuntimeError("paged_attention: q must be 3D [B * H_q, L, D]")
    if key_pages.dim() != 4 or value_pages.dim() != 4:
        raise RuntimeError("paged_attention: page tensors must be 4D [P, H_kv, page_size, D]")
    if block_table.dim() != 2 or context_lens.dim() != 1:
        raise RuntimeError("paged_attention: block_table must be 2D and context_lens must be 1D")
    if num_heads % num_kv_heads != 0:
        raise RuntimeError("paged_attention: num_heads must be divisible by num_kv_heads")
    if query.shape[0] % num_heads != 0:
        raise RuntimeError("paged_attention: q.shape[0] must be divisible by num_heads")
    if key_pages.shape != value_pages.shape:
        raise RuntimeError("paged_attention: key_pages and value_pages must have the same shape")
    if key_pages.shape[1] != num_kv_heads:
        raise RuntimeError("paged_attention: page tensor head count must equal num_kv_heads")
    if query.shape[2] != key_pages.shape[3]:
        raise RuntimeError("paged_attention: q and page tensors must have the same head dimension")
    if block_table.shape[0] != context_lens.shape[0]:
        raise RuntimeError("paged_attention: block_table and context_lens batch sizes must match")
    if query.shape[0] // num_heads != block_table.shape[0]:
        raise RuntimeError("paged_attention: q batch size must match block_table batch size")
    _require_gpu("paged_attention", query, key_pages, value_pages, block_table, context_lens)
    N, L, D = query.shape
    P, _, page_size, _ = key_pages.shape
    max_pages = block_table.shape[1]
    if D > 128:
        raise RuntimeError("paged_attention: head dimension must be at most 128")
    if L > 8 and query.dtype == torch.bfloat16 and D != 128:
        raise RuntimeError("paged_attention: bfloat16 prefill requires head dimension 128")
    for name, t in (("q", query), ("key_pages", key_pages), ("value_pages", value_pages),
                    ("block_table", block_table), ("context_lens", context_lens)):
        if not t.is_contiguous():
            raise RuntimeError(f"paged_attention: {name} must be contiguous")
    out = torch.empty_like(query)
    ws_bytes = _lib.tl_paged_attention_workspace_bytes(N, L, D, page_size, max_pages, num_heads, num_kv_heads,
                                                       int(max_context_hint))
    ws = _workspace(ws_bytes, query.device)
    _check(
        _lib.tl_paged_attention(
            _ptr(query), _ptr(key_pages), _ptr(value_pages), _ptr(block_table), _ptr(context_lens), _ptr(out), N, L,
            D, P, page_size, max_pages, int(num_heads), int(num_kv_heads), float(scale), int(bool(is_causal)),
            int(max_context_hint), _DTYPES[query.dtype], _ptr(ws) if ws is not None else None,
            ws.numel() if ws is not None else 0, _stream(),
        )
    )
    return out


__all__ = [
    "load_library",
    "quantized_matmul",
    "gather_quantized_matvec",
    "quantized_embedding",
    "rms_norm",
    "rope",
    "swiglu",
    "decode_attention",
    "paged_cache_update",
    "paged_attention",
]


# ---- kernel-level entry points of the decode path (include/tinyllm_engine.h, last section) -------------------------
PRO_NONE, PRO_RMSNORM, PRO_ATTN_MERGE, PRO_RMS_WEIGHTED = 0, 1, 2, 3
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU = 0, 1, 2
ATTN_PARTIAL_ROW = 128 + 4  # floats per (head, split) row of decode-attention split partials: 128 value sums, max, sum, 2 pad
# values of tl_linear_info.kernel (what RAN); the `kernel` argument of decode_linear selects: 0 engine routing, 1 GEMV,
# 2 skinny matmul (grid by shape), 3 / 4 skinny matmul on its one-shot / persistent grid, 5 register-resident batched matmul
LINEAR_KERNELS = {1: "qmv3 (fused MFMA GEMV)", 2: "qmm3 (skinny MFMA matmul + slice reduction)",
                  3: "qmv (packed-dot GEMV fallback)", 4: "prefill GEMM path", 5: "qmm6 (register-resident batched matmul)"}


class TiledW4:
    """One W4 matrix re-packed into the decode engine's tiled layout (tl_tiled_w4).  Keeps the checkpoint tensors alive."""

    def __init__(self, weight: torch.Tensor, scales: torch.Tensor, biases: torch.Tensor):
        _require_gpu("TiledW4", weight, scales, biases)
        if weight.dtype not in (torch.int32, torch.uint32) or weight.dim() != 2:
            raise RuntimeError("TiledW4: weight must be a 2-D uint32 tensor [rows, cols/8]")
        if scales.dtype != torch.bfloat16 or biases.dtype != torch.bfloat16:
            raise RuntimeError("TiledW4: the decode path is bfloat16")
        self.weight, self.scales, self.biases = weight.contiguous(), scales.contiguous(), biases.contiguous()
        self.rows, self.cols = int(weight.shape[0]), int(weight.shape[1]) * 8
        if tuple(self.scales.shape) != (self.rows, self.cols // 128) or self.scales.shape != self.biases.shape:
            raise RuntimeError("TiledW4: scales / biases must be [rows, cols/128]")
        w4 = TlW4(_ptr(self.weight), _ptr(self.scales), _ptr(self.biases), self.rows, self.cols)
        handle = _c_void_p()
        _check(_lib.tl_tiled_w4_create(ctypes.byref(w4), _stream(), ctypes.byref(handle)))
        self._h = handle

    def close(self) -> None:
        if getattr(self, "_h", None):
            torch.cuda.synchronize()
            _lib.tl_tiled_w4_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_linear(w: TiledW4, a: torch.Tensor | None, *, prologue: int = PRO_NONE, epilogue: int = EPI_STORE,
                  norm_weight: torch.Tensor | None = None, residual: torch.Tensor | None = None, eps: float = 1e-6,
                  kernel: int = 0, merge_partials: torch.Tensor | None = None, ss_in: torch.Tensor | None = None,
                  want_ss_out: bool = False, norm_out: torch.Tensor | None = None, fragment_order: bool = False,
                  fragment_rows: int | None = None):
    """One projection of a decode step over ``a`` [M <= 64, cols] bf16 (tl_decode_linear).  Returns (out, info) where info
    names the kernel that ran and its launch parameters.

    The keyword arguments after ``kernel`` reach the routes of tl_decode_linear_ex (include/tinyllm_engine.h):
    ``merge_partials`` [cols / 128, n_splits, 132] fp32 with prologue PRO_ATTN_MERGE (``a`` is None, one row);
    ``ss_in`` [M, n] fp32 partial sums of squares for prologue PRO_RMSNORM / PRO_RMS_WEIGHTED; ``want_ss_out`` /
    ``norm_out`` [rows] with the residual epilogue -- info then carries "ss_out" [M, rows / 16] and "out_w" [M, rows].
    ``fragment_order``: the weighted rows on either side (``a`` with PRO_RMS_WEIGHTED through kernel 5: [ceil16(M), cols] in fragment
    order; "out_w": [ceil16(M), rows]) lie in the batched step's fragment order (fragment_order_of / rows_from_fragment_order)."""
    extended = merge_partials is not None or ss_in is not None or want_ss_out or norm_out is not None or fragment_order \
        or prologue in (PRO_ATTN_MERGE, PRO_RMS_WEIGHTED)
    if prologue == PRO_ATTN_MERGE:
        if merge_partials is None or a is not None:
            raise RuntimeError("decode_linear: the merging prologue takes merge_partials and no activation rows")
        _require_gpu("decode_linear", merge_partials)
        if merge_partials.dtype != torch.float32 or merge_partials.dim() != 3 or not merge_partials.is_contiguous() \
                or merge_partials.shape[0] * 128 != w.cols or merge_partials.shape[2] != ATTN_PARTIAL_ROW:
            raise RuntimeError("decode_linear: merge_partials must be contiguous float32 [cols / 128, n_splits, 132]")
        M, device = 1, merge_partials.device
    else:
        _require_gpu("decode_linear", a)
        if a.dtype != torch.bfloat16 or a.dim() != 2 or a.shape[1] != w.cols or not a.is_contiguous():
            raise RuntimeError("decode_linear: a must be a contiguous bfloat16 [M, cols] tensor")
        M, device = int(a.shape[0]), a.device
        if fragment_order and prologue == PRO_RMS_WEIGHTED:  # rows padded to 16: the caller says how many are real
            if M % 16 != 0 or fragment_rows is None or not (M - 16 < fragment_rows <= M):
                raise RuntimeError("decode_linear: rows in fragment order come as [ceil16(M), cols] with fragment_rows = M")
            M = int(fragment_rows)
    out_cols = w.rows // 2 if epilogue == EPI_SWIGLU else w.rows
    out = torch.empty((M, out_cols), dtype=torch.bfloat16, device=device)
    if residual is not None and (residual.dtype != torch.bfloat16 or tuple(residual.shape) != (M, w.rows)
                                 or not residual.is_contiguous()):
        raise RuntimeError("decode_linear: residual must be a contiguous bfloat16 [M, rows] tensor")
    if norm_weight is not None and (norm_weight.dtype != torch.bfloat16 or tuple(norm_weight.shape) != (w.cols,)):
        raise RuntimeError("decode_linear: norm_weight must be bfloat16 [cols]")
    ws_bytes = _lib.tl_decode_linear_workspace_bytes(M, w.rows, w.cols)
    ws = _workspace(ws_bytes, device)
    info = TlLinearInfo()
    common = (w._h, _ptr(a) if a is not None else None, _ptr(out), M, int(prologue), int(epilogue),
              _ptr(norm_weight) if norm_weight is not None else None, _ptr(residual) if residual is not None else None,
              float(eps), int(kernel), _ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0, _stream())
    extra = {}
    if not extended:
        _check(_lib.tl_decode_linear(*common, ctypes.byref(info)))
    else:
        ex = TlLinearEx()
        if merge_partials is not None:
            ex.merge_ws_dev, ex.n_splits = _ptr(merge_partials), int(merge_partials.shape[1])
        if ss_in is not None:
            if ss_in.dtype != torch.float32 or ss_in.dim() != 2 or ss_in.shape[0] != M or not ss_in.is_contiguous():
                raise RuntimeError("decode_linear: ss_in must be contiguous float32 [M, partials]")
            _require_gpu("decode_linear", ss_in)
            ex.ss_in_dev, ex.ss_in_n = _ptr(ss_in), int(ss_in.shape[1])
        if want_ss_out:
            extra["ss_out"] = torch.full((M, w.rows // 16), float("nan"), dtype=torch.float32, device=device)
            ex.ss_out_dev = _ptr(extra["ss_out"])
        if norm_out is not None:
            if norm_out.dtype != torch.bfloat16 or tuple(norm_out.shape) != (w.rows,):
                raise RuntimeError("decode_linear: norm_out must be bfloat16 [rows]")
            extra["out_w"] = torch.zeros(((M + 15) // 16 * 16 if fragment_order else M, w.rows), dtype=torch.bfloat16, device=device)
            ex.norm_out_dev, ex.out_w_dev = _ptr(norm_out), _ptr(extra["out_w"])
        ex.fragment_order = 1 if fragment_order else 0
        _check(_lib.tl_decode_linear_ex(*common, ctypes.byref(ex), ctypes.byref(info)))
    return out, {"kernel": info.kernel, "kernel_name": LINEAR_KERNELS.get(info.kernel, "?"), "launches": info.launches,
                 "rows_per_pass": info.rows_per_pass, "p": list(info.p), **extra}


def prefill_weights_bf16(weight: torch.Tensor, scales: torch.Tensor, biases: torch.Tensor) -> torch.Tensor:
    """W4 [rows, cols/8] -> bf16 [rows, cols] = bf16(q * scale + bias): the B operand of the reference's tile GEMM (tl_prefill_weights_bf16)."""
    _require_gpu("prefill_weights_bf16", weight, scales, biases)
    rows, cols = int(weight.shape[0]), int(weight.shape[1]) * 8
    w4 = TlW4(_ptr(weight.contiguous()), _ptr(scales.contiguous()), _ptr(biases.contiguous()), rows, cols)
    out = torch.empty((rows, cols), dtype=torch.bfloat16, device=weight.device)
    _check(_lib.tl_prefill_weights_bf16(ctypes.byref(w4), _ptr(out), _stream()))
    return out


def prefill_matmul_bf16(a: torch.Tensor, w_bf16: torch.Tensor, *, epilogue: int = 0, residual: torch.Tensor | None = None) -> torch.Tensor:
    """out = epilogue(a @ w_bf16^T): the plain bf16 GEMM large prefill chunks run on (tl_prefill_matmul_bf16, csrc/gemm8.h)."""
    _require_gpu("prefill_matmul_bf16", a, w_bf16)
    if a.dtype != torch.bfloat16 or w_bf16.dtype != torch.bfloat16 or a.dim() != 2 or w_bf16.dim() != 2 or a.shape[1] != w_bf16.shape[1]:
        raise RuntimeError("prefill_matmul_bf16: a [M, cols] and w_bf16 [rows, cols] must be bfloat16 with the same cols")
    M, rows, cols = int(a.shape[0]), int(w_bf16.shape[0]), int(a.shape[1])
    out = torch.empty((M, rows // 2 if epilogue == 2 else rows), dtype=torch.bfloat16, device=a.device)
    res = residual.contiguous() if residual is not None else None
    _check(_lib.tl_prefill_matmul_bf16(_ptr(a.contiguous()), _ptr(w_bf16.contiguous()), _ptr(out), M, rows, cols, int(epilogue),
                                       _ptr(res) if res is not None else None, _stream()))
    return out


def fragment_order_of(rows: torch.Tensor) -> torch.Tensor:
    """[M, cols] -> the batched step's fragment order, [ceil16(M), cols] (zero rows appended): [16-row block][128-column group]
    [k-step t][lane = r + 16 c][8 elements] = row 16 block + r, columns 128 g + 32 c + 8 t .. + 7 (csrc/qmm6.h, qmm6_frag_offset)."""
    M, cols = rows.shape
    pad = (M + 15) // 16 * 16
    x = torch.zeros((pad, cols), dtype=rows.dtype, device=rows.device)
    x[:M] = rows
    x = x.reshape(pad // 16, 16, cols // 128, 4, 4, 8)      # [block, r, g, c, t, e]
    return x.permute(0, 2, 4, 3, 1, 5).contiguous().reshape(pad, cols)  # [block, g, t, c, r, e]


def rows_from_fragment_order(frag: torch.Tensor, M: int) -> torch.Tensor:
    """Inverse of fragment_order_of: [ceil16(M), cols] in fragment order -> [M, cols] row-major."""
    pad, cols = frag.shape
    x = frag.reshape(pad // 16, cols // 128, 4, 4, 16, 8)   # [block, g, t, c, r, e]
    return x.permute(0, 4, 1, 3, 2, 5).contiguous().reshape(pad, cols)[:M]


def decode_attention_fused(qkv: torch.Tensor, q_norm: torch.Tensor, k_norm: torch.Tensor, key_pages: torch.Tensor,
                           value_pages: torch.Tensor, block_table: torch.Tensor, context_lens: torch.Tensor, *,
                           num_heads: int, num_kv_heads: int, rope_theta: float, eps: float,
                           max_context: int) -> tuple[torch.Tensor, dict]:
    """The attention launch of one decode layer (tl_decode_attention_fused): q/k-norm + RoPE + in-place KV append +
    paged GQA attention over ``context_lens + 1`` tokens.  qkv [B, (Hq + 2 Hkv) D]; pages [P, Hkv, page, D] (modified)."""
    _require_gpu("decode_attention_fused", qkv, q_norm, k_norm, key_pages, value_pages, block_table, context_lens)
    B = int(qkv.shape[0])
    P, Hkv, page, D = (int(x) for x in key_pages.shape)
    if Hkv != num_kv_heads or tuple(value_pages.shape) != tuple(key_pages.shape):
        raise RuntimeError("decode_attention_fused: page pools must be [P, num_kv_heads, page_size, D] and alike")
    if qkv.dim() != 2 or qkv.shape[1] != (num_heads + 2 * num_kv_heads) * D:
        raise RuntimeError("decode_attention_fused: qkv must be [batch, (Hq + 2 Hkv) * D]")
    for name, t in (("qkv", qkv), ("key_pages", key_pages), ("value_pages", value_pages), ("q_norm", q_norm),
                    ("k_norm", k_norm)):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise RuntimeError(f"decode_attention_fused: {name} must be contiguous bfloat16")
    if block_table.dtype != torch.int32 or context_lens.dtype != torch.int32 or block_table.dim() != 2 \
            or block_table.shape[0] != B or tuple(context_lens.shape) != (B,):
        raise RuntimeError("decode_attention_fused: block_table [B, max_pages] and context_lens [B] must be int32")
    out = torch.empty((B, num_heads * D), dtype=torch.bfloat16, device=qkv.device)
    ws_bytes = _lib.tl_decode_attention_fused_workspace_bytes(B, num_heads, D)
    ws = _workspace(ws_bytes, qkv.device)
    info = TlAttentionInfo()
    _check(_lib.tl_decode_attention_fused(_ptr(qkv), _ptr(q_norm), _ptr(k_norm), _ptr(key_pages), _ptr(value_pages),
                                          _ptr(block_table.contiguous()), _ptr(context_lens), _ptr(out), B, num_heads,
                                          num_kv_heads, D, page, int(block_table.shape[1]), float(rope_theta), float(eps),
                                          int(max_context), _ptr(ws), ws.numel(), _stream(), ctypes.byref(info)))
    return out, {name: getattr(info, name) for name, _ in info._fields_}


def verify_attention_rows(qkv: torch.Tensor, q_norm: torch.Tensor, k_norm: torch.Tensor, key_pages: torch.Tensor, value_pages: torch.Tensor,
                          block_table: torch.Tensor, slots, starts, lens, *, num_heads: int, num_kv_heads: int, rope_theta: float,
                          eps: float, key_scales: torch.Tensor | None = None, value_scales: torch.Tensor | None = None) -> tuple[torch.Tensor, dict]:
    """The attention stage of a batched verification pass (tl_verify_attention_rows): the rows of several sequences back to back in
    qkv [R, (Hq + 2 Hkv) 128]; sequence i holds ``lens[i]`` (1 .. 8) rows from position ``starts[i]`` of block-table row ``slots[i]``.
    q/k-norm + RoPE + in-place KV append (pages [P, Hkv, page, 128] bf16, or uint8 codes with key_scales / value_scales [P, Hkv, page]
    float32) + causal paged attention -> ([R, Hq * 128] bf16 row-major, the split plan)."""
    _require_gpu("verify_attention_rows", qkv, q_norm, k_norm, key_pages, value_pages, block_table)
    fp8 = key_scales is not None or value_scales is not None
    P, Hkv, page, D = (int(x) for x in key_pages.shape)
    R = int(qkv.shape[0])
    if D != 128 or Hkv != num_kv_heads or tuple(value_pages.shape) != tuple(key_pages.shape):
        raise RuntimeError("verify_attention_rows: page pools must be [P, num_kv_heads, page_size, 128] and alike")
    if qkv.dim() != 2 or qkv.shape[1] != (num_heads + 2 * num_kv_heads) * D or R != sum(int(n) for n in lens):
        raise RuntimeError("verify_attention_rows: qkv must be [sum(lens), (Hq + 2 Hkv) * 128]")
    for name, t in (("qkv", qkv), ("q_norm", q_norm), ("k_norm", k_norm)):
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise RuntimeError(f"verify_attention_rows: {name} must be contiguous bfloat16")
    want = torch.uint8 if fp8 else torch.bfloat16
    for name, t in (("key_pages", key_pages), ("value_pages", value_pages)):
        if t.dtype != want or not t.is_contiguous():
            raise RuntimeError(f"verify_attention_rows: {name} must be contiguous {want}")
    if fp8:
        for name, t in (("key_scales", key_scales), ("value_scales", value_scales)):
            if t is None or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (P, Hkv, page) or not t.is_contiguous():
                raise RuntimeError(f"verify_attention_rows: {name} must be contiguous float32 [P, Hkv, page] on the GPU")
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or not block_table.is_contiguous():
        raise RuntimeError("verify_attention_rows: block_table [slots, max_pages] must be contiguous int32")
    n = len(lens)
    if len(slots) != n or len(starts) != n or any(not 0 <= int(s) < block_table.shape[0] for s in slots):
        raise RuntimeError("verify_attention_rows: slots, starts and lens must be alike, every slot a row of block_table")
    out = torch.empty((R, num_heads * D), dtype=torch.bfloat16, device=qkv.device)
    arr = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])
    info = TlAttentionInfo()
    _check(_lib.tl_verify_attention_rows(_ptr(qkv), _ptr(q_norm), _ptr(k_norm), _ptr(key_pages), _ptr(value_pages),
                                         _ptr(key_scales) if fp8 else None, _ptr(value_scales) if fp8 else None, _ptr(block_table), n,
                                         arr(slots), arr(starts), arr(lens), _ptr(out), num_heads, num_kv_heads, page,
                                         int(block_table.shape[1]), float(rope_theta), float(eps), _stream(), ctypes.byref(info)))
    return out, {name: getattr(info, name) for name, _ in info._fields_}


def verify_accept_rows(logits: torch.Tensor, row0, lens, tokens: torch.Tensor) -> list[list[int]]:
    """The acceptance stage of a batched verification pass over caller rows (tl_verify_accept_rows): logits [R, vocab] bf16, tokens [R]
    int32 (the tokens the rows were fed); sequence i owns the rows [row0[i], row0[i] + lens[i]).  Returns per sequence the accepted
    proposals followed by the correction or the bonus token."""
    _require_gpu("verify_accept_rows", logits, tokens)
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_contiguous():
        raise RuntimeError("verify_accept_rows: logits must be contiguous bfloat16 [rows, vocab]")
    if tokens.dtype != torch.int32 or tokens.dim() != 1 or tokens.shape[0] != logits.shape[0] or not tokens.is_contiguous():
        raise RuntimeError("verify_accept_rows: tokens must be contiguous int32 [rows]")
    n = len(lens)
    if len(row0) != n or any(int(r) < 0 or int(r) + int(k) > logits.shape[0] for r, k in zip(row0, lens)):
        raise RuntimeError("verify_accept_rows: every sequence's rows must lie inside logits")
    arr = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])
    out = torch.zeros((max(n, 1), 9), dtype=torch.int32, device=logits.device)  # tl_verify_result: count, ids[8]
    _check(_lib.tl_verify_accept_rows(_ptr(logits), int(logits.shape[1]), n, arr(row0), arr(lens), _ptr(tokens), _ptr(out), _stream()))
    host = out.cpu().tolist()
    return [rec[1:1 + rec[0]] for rec in host[:n]]


def verify_sample_rows(target: torch.Tensor, draft, row0, lens, starts, tokens: torch.Tensor, temperature, top_k, top_p, seed,
                       draft_sampling=(0.0, 0, 1.0)):
    """The acceptance stage of a batched speculative-sampling pass over caller rows (tl_verify_sample_rows): ``target`` [R, vocab] bf16,
    ``draft`` the rows the proposals were drawn from under ``draft_sampling`` = (temperature, top_k, top_p), or None for point proposals
    (one-hot at the proposed id); ``tokens`` [R] int32 the tokens the rows were fed; sequence i owns the rows [row0[i], row0[i] +
    lens[i]) and held starts[i] tokens before them; ``temperature`` / ``top_k`` / ``top_p`` / ``seed``: a scalar or one value per
    sequence.  Returns (accept int32 [R], alt int32 [R] on the device, per sequence the accepted proposals followed by one more token)."""
    _require_gpu("verify_sample_rows", target, tokens)
    if target.dtype != torch.bfloat16 or target.dim() != 2 or not target.is_contiguous():
        raise RuntimeError("verify_sample_rows: target must be contiguous bfloat16 [rows, vocab]")
    if draft is not None and (not isinstance(draft, torch.Tensor) or draft.dtype != torch.bfloat16 or draft.shape != target.shape or
                              draft.device != target.device or not draft.is_contiguous()):
        raise RuntimeError("verify_sample_rows: draft must be None or contiguous bfloat16 of the target's shape, on its device")
    if tokens.dtype != torch.int32 or tokens.dim() != 1 or tokens.shape[0] != target.shape[0] or not tokens.is_contiguous():
        raise RuntimeError("verify_sample_rows: tokens must be contiguous int32 [rows]")
    n = len(lens)
    if len(row0) != n or len(starts) != n or any(int(r) < 0 or int(r) + int(k) > target.shape[0] for r, k in zip(row0, lens)):
        raise RuntimeError("verify_sample_rows: every sequence's rows must lie inside target (one row0 / lens / starts per sequence)")
    dev = target.device

    def per_seq(v, dtype):
        t = torch.as_tensor(v, dtype=dtype).reshape(-1)
        if t.numel() == 1:
            t = t.expand(max(n, 1))
        if t.numel() != n:
            raise ValueError("a verification parameter needs one value per sequence")
        return t.contiguous().to(dev)

    seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in (seed if hasattr(seed, "__len__") else [seed] * n)]
    if len(seeds) != n:
        raise ValueError("a verification parameter needs one value per sequence")
    seed_t = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64).to(dev)  # uint64 bits
    tt, tk, tp = per_seq(temperature, torch.float32), per_seq(top_k, torch.int32), per_seq(top_p, torch.float32)
    arr = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])
    rows = int(target.shape[0])
    accept = torch.zeros(rows, dtype=torch.int32, device=dev)
    alt = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    out = torch.zeros((max(n, 1), 9), dtype=torch.int32, device=dev)  # tl_verify_result: count, ids[8]
    dt, dk, dp = draft_sampling
    _check(_lib.tl_verify_sample_rows(_ptr(target), _ptr(draft) if draft is not None else None, int(target.shape[1]), n, arr(row0), arr(lens),
                                      arr(starts), _ptr(tokens), _ptr(tt), _ptr(tk), _ptr(tp), _ptr(seed_t), float(dt), int(dk or 0),
                                      float(1.0 if dp is None else dp), _ptr(accept), _ptr(alt), _ptr(out), _stream()))
    host = out.cpu().tolist()
    return accept, alt, [rec[1:1 + rec[0]] for rec in host[:n]]


# ---- FP8 (E4M3) KV pages: the quantised twins of paged_cache_update / paged_attention -------------------------------------
# (include/tinyllm_hip.h "FP8 KV pages"; SURVEY section 8f row 4 -- the reference has no quantised cache, README.md:134-135, so these
# are NOT part of the reference's interface and stay out of __all__)
KV_BF16, KV_FP8_E4M3 = 0, 1


def kv_fp8_quantize_rows(values: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """values [..., 128] bfloat16 -> (codes [..., 128] uint8, scales [...] float32): OCP E4M3 codes and one power-of-two scale per row."""
    _require_gpu("kv_fp8_quantize_rows", values)
    if values.dtype != torch.bfloat16 or values.shape[-1] != 128 or not values.is_contiguous():
        raise RuntimeError("kv_fp8_quantize_rows: contiguous bfloat16 rows of 128 values")
    rows = values.numel() // 128
    codes = torch.empty(values.shape, dtype=torch.uint8, device=values.device)
    scales = torch.empty(values.shape[:-1], dtype=torch.float32, device=values.device)
    _check(_lib.tl_kv_fp8_quantize_rows(_ptr(values), _ptr(codes), _ptr(scales), rows, 128, _stream()))
    return codes, scales


def kv_fp8_dequantize_rows(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(codes [..., 128] uint8, scales [...] float32) -> bfloat16 [..., 128] (exact)."""
    _require_gpu("kv_fp8_dequantize_rows", codes, scales)
    if codes.dtype != torch.uint8 or scales.dtype != torch.float32 or codes.shape[-1] != 128 or tuple(codes.shape[:-1]) != tuple(scales.shape) \
            or not codes.is_contiguous() or not scales.is_contiguous():
        raise RuntimeError("kv_fp8_dequantize_rows: contiguous uint8 codes [..., 128] and float32 scales [...]")
    out = torch.empty(codes.shape, dtype=torch.bfloat16, device=codes.device)
    _check(_lib.tl_kv_fp8_dequantize_rows(_ptr(codes), _ptr(scales), _ptr(out), codes.numel() // 128, 128, _stream()))
    return out


def paged_cache_update_fp8(pages: torch.Tensor, page_scales: torch.Tensor, values: torch.Tensor, page_id: int,
                           start: int) -> tuple[torch.Tensor, torch.Tensor]:
    """In-place quantising write of bfloat16 ``values[1,H,len,128]`` into ``pages[P,H,page,128]`` uint8 + ``page_scales[P,H,page]``."""
    if pages.dtype != torch.uint8 or page_scales.dtype != torch.float32 or values.dtype != torch.bfloat16:
        raise RuntimeError("paged_cache_update_fp8: uint8 pages, float32 page_scales, bfloat16 values")
    if pages.dim() != 4 or values.dim() != 4 or values.shape[0] != 1 or tuple(page_scales.shape) != tuple(pages.shape[:3]):
        raise RuntimeError("paged_cache_update_fp8: expected pages [P, H, page_size, 128], page_scales [P, H, page_size] and values [1, H, length, 128]")
    if values.shape[1] != pages.shape[1] or values.shape[3] != pages.shape[3]:
        raise RuntimeError("paged_cache_update_fp8: values must match the page head count and head dimension")
    if page_id < 0 or page_id >= pages.shape[0] or start < 0 or start + values.shape[2] > pages.shape[2]:
        raise RuntimeError("paged_cache_update_fp8: destination slice is outside page storage")
    _require_gpu("paged_cache_update_fp8", pages, page_scales, values)
    if not pages.is_contiguous() or not values.is_contiguous() or not page_scales.is_contiguous():
        raise RuntimeError("paged_cache_update_fp8: pages, page_scales and values must be contiguous")
    P, H, page_size, D = pages.shape
    _check(_lib.tl_paged_cache_update_fp8(_ptr(pages), _ptr(page_scales), _ptr(values), P, H, page_size, D, values.shape[2],
                                          int(page_id), int(start), _stream()))
    return pages, page_scales


def paged_attention_fp8(query: torch.Tensor, key_pages: torch.Tensor, key_scales: torch.Tensor, value_pages: torch.Tensor,
                        value_scales: torch.Tensor, block_table: torch.Tensor, context_lens: torch.Tensor, scale: float = 1.0,
                        is_causal: bool = False, *, num_kv_heads: int, num_heads: int, max_context_hint: int = 0) -> torch.Tensor:
    """paged_attention over FP8 pages: bfloat16 ``query`` [B * Hq, L, 128], uint8 pages [P, Hkv, page, 128], float32 scales [P, Hkv, page]."""
    if query.dtype != torch.bfloat16 or key_pages.dtype != torch.uint8 or value_pages.dtype != torch.uint8 \
            or key_scales.dtype != torch.float32 or value_scales.dtype != torch.float32:
        raise RuntimeError("paged_attention_fp8: bfloat16 q, uint8 pages, float32 scales")
    if block_table.dtype != torch.int32 or context_lens.dtype != torch.int32:
        raise RuntimeError("paged_attention_fp8: block_table and context_lens must be int32")
    if query.dim() != 3 or key_pages.dim() != 4 or key_pages.shape != value_pages.shape or block_table.dim() != 2 or context_lens.dim() != 1:
        raise RuntimeError("paged_attention_fp8: q [B * H_q, L, D], pages [P, H_kv, page_size, D], block_table [B, max_pages], context_lens [B]")
    if tuple(key_scales.shape) != tuple(key_pages.shape[:3]) or tuple(value_scales.shape) != tuple(value_pages.shape[:3]):
        raise RuntimeError("paged_attention_fp8: scales must be [P, H_kv, page_size]")
    if num_heads % num_kv_heads != 0 or query.shape[0] % num_heads != 0 or key_pages.shape[1] != num_kv_heads:
        raise RuntimeError("paged_attention_fp8: incompatible head counts")
    if query.shape[2] != 128 or key_pages.shape[3] != 128:
        raise RuntimeError("paged_attention_fp8: FP8 pages need head dimension 128")
    if query.shape[0] // num_heads != block_table.shape[0] or block_table.shape[0] != context_lens.shape[0]:
        raise RuntimeError("paged_attention_fp8: q batch size must match block_table and context_lens")
    tensors = (query, key_pages, key_scales, value_pages, value_scales, block_table, context_lens)
    _require_gpu("paged_attention_fp8", *tensors)
    if not all(t.is_contiguous() for t in tensors):
        raise RuntimeError("paged_attention_fp8: every tensor must be contiguous")
    N, L, D = query.shape
    P, _, page_size, _ = key_pages.shape
    max_pages = block_table.shape[1]
    out = torch.empty_like(query)
    ws_bytes = _lib.tl_paged_attention_workspace_bytes(N, L, D, page_size, max_pages, num_heads, num_kv_heads, int(max_context_hint))
    ws = _workspace(ws_bytes, query.device)
    _check(_lib.tl_paged_attention_fp8(
        _ptr(query), _ptr(key_pages), _ptr(key_scales), _ptr(value_pages), _ptr(value_scales), _ptr(block_table), _ptr(context_lens),
        _ptr(out), N, L, D, P, page_size, max_pages, int(num_heads), int(num_kv_heads), float(scale), int(bool(is_causal)),
        int(max_context_hint), _ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0, _stream()))
    return out


def decode_attention_fused_fp8(qkv: torch.Tensor, q_norm: torch.Tensor, k_norm: torch.Tensor, key_pages: torch.Tensor,
                               key_scales: torch.Tensor, value_pages: torch.Tensor, value_scales: torch.Tensor,
                               block_table: torch.Tensor, context_lens: torch.Tensor, *, num_heads: int, num_kv_heads: int,
                               rope_theta: float, eps: float, max_context: int) -> tuple[torch.Tensor, dict]:
    """decode_attention_fused over FP8 pages (tl_decode_attention_fused_fp8): the appended K / V rows are quantised in place."""
    _require_gpu("decode_attention_fused_fp8", qkv, q_norm, k_norm, key_pages, key_scales, value_pages, value_scales, block_table, context_lens)
    B = int(qkv.shape[0])
    P, Hkv, page, D = (int(x) for x in key_pages.shape)
    if D != 128 or Hkv != num_kv_heads or tuple(value_pages.shape) != tuple(key_pages.shape) \
            or tuple(key_scales.shape) != (P, Hkv, page) or tuple(value_scales.shape) != (P, Hkv, page):
        raise RuntimeError("decode_attention_fused_fp8: pages [P, num_kv_heads, page_size, 128] uint8 and scales [P, num_kv_heads, page_size]")
    if qkv.dim() != 2 or qkv.shape[1] != (num_heads + 2 * num_kv_heads) * D:
        raise RuntimeError("decode_attention_fused_fp8: qkv must be [batch, (Hq + 2 Hkv) * D]")
    for name, t, dt in (("qkv", qkv, torch.bfloat16), ("q_norm", q_norm, torch.bfloat16), ("k_norm", k_norm, torch.bfloat16),
                        ("key_pages", key_pages, torch.uint8), ("value_pages", value_pages, torch.uint8),
                        ("key_scales", key_scales, torch.float32), ("value_scales", value_scales, torch.float32)):
        if t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"decode_attention_fused_fp8: {name} must be contiguous {dt}")
    if block_table.dtype != torch.int32 or context_lens.dtype != torch.int32 or block_table.dim() != 2 \
            or block_table.shape[0] != B or tuple(context_lens.shape) != (B,):
        raise RuntimeError("decode_attention_fused_fp8: block_table [B, max_pages] and context_lens [B] must be int32")
    out = torch.empty((B, num_heads * D), dtype=torch.bfloat16, device=qkv.device)
    ws = _workspace(_lib.tl_decode_attention_fused_workspace_bytes(B, num_heads, D), qkv.device)
    info = TlAttentionInfo()
    _check(_lib.tl_decode_attention_fused_fp8(_ptr(qkv), _ptr(q_norm), _ptr(k_norm), _ptr(key_pages), _ptr(key_scales), _ptr(value_pages),
                                              _ptr(value_scales), _ptr(block_table.contiguous()), _ptr(context_lens), _ptr(out), B,
                                              num_heads, num_kv_heads, D, page, int(block_table.shape[1]), float(rope_theta), float(eps),
                                              int(max_context), _ptr(ws), ws.numel(), _stream(), ctypes.byref(info)))
    return out, {name: getattr(info, name) for name, _ in info._fields_}


def paged_attention_waves(waves: int = 0) -> int:
    """Test / lab hook (tl_paged_attention_waves): 8 or 4 waves per workgroup in the bf16 FlashAttention prefill kernel; returns the previous value."""
    return int(_lib.tl_paged_attention_waves(int(waves)))


def sample_logits(logits: torch.Tensor, temperature, top_k, top_p, seed, position) -> torch.Tensor:
    """The decode engine's device sampler (tl_sample_logits) over rows of bf16 logits [rows, vocab]: per-row temperature (0 = greedy),
    top_k (0 = off), top_p (outside (0, 1) = off), seed (uint64) and position -> int32 ids [rows].  Each parameter is a scalar or one
    value per row."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("sample_logits takes a [rows, vocab] bf16 tensor on the GPU")
    logits = logits.contiguous()
    rows, dev = logits.shape[0], logits.device

    def per_row(v, dtype):
        t = torch.as_tensor(v, dtype=dtype).reshape(-1)
        if t.numel() == 1:
            t = t.expand(rows)
        if t.numel() != rows:
            raise ValueError("a sampling parameter needs one value per row")
        return t.contiguous().to(dev)

    seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in (seed if hasattr(seed, "__len__") else [seed] * rows)]
    seed_t = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64).to(dev)  # uint64 bits
    if seed_t.numel() != rows:
        raise ValueError("a sampling parameter needs one value per row")
    t_t, k_t, p_t, pos_t = per_row(temperature, torch.float32), per_row(top_k, torch.int32), per_row(top_p, torch.float32), per_row(position, torch.int32)
    ids = torch.empty(rows, dtype=torch.int32, device=dev)
    check(_lib.tl_sample_logits(logits.data_ptr(), rows, logits.shape[1], t_t.data_ptr(), k_t.data_ptr(), p_t.data_ptr(), seed_t.data_ptr(),
                                pos_t.data_ptr(), ids.data_ptr(), _stream()))
    return ids


def spec_sample_rows(target: torch.Tensor, draft: torch.Tensor, proposal, temperature, top_k, top_p, draft_temperature, draft_top_k,
                     draft_top_p, seed, position):
    """Speculative sampling (tl_spec_sample_rows) over rows of bf16 logits: ``target`` and ``draft`` [rows, vocab], row i of ``draft`` the
    row proposal i was drawn from; per-row proposal (< 0: a bonus row), the target's and the draft's temperature / top_k / top_p, seed
    (uint64) and position, each a scalar or one value per row.  Returns (accept int32 [rows], alt int32 [rows]: -1 where accepted)."""
    for t in (target, draft):
        if t.dtype != torch.bfloat16 or t.dim() != 2 or not t.is_cuda:
            raise ValueError("spec_sample_rows takes [rows, vocab] bf16 tensors on the GPU")
    if target.shape != draft.shape or target.device != draft.device:
        raise ValueError("spec_sample_rows: target and draft rows must have one shape and one device")
    target, draft = target.contiguous(), draft.contiguous()
    rows, dev = target.shape[0], target.device

    def per_row(v, dtype):
        t = torch.as_tensor(v, dtype=dtype).reshape(-1)
        if t.numel() == 1:
            t = t.expand(rows)
        if t.numel() != rows:
            raise ValueError("a speculative-sampling parameter needs one value per row")
        return t.contiguous().to(dev)

    seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in (seed if hasattr(seed, "__len__") else [seed] * rows)]
    if len(seeds) != rows:
        raise ValueError("a speculative-sampling parameter needs one value per row")
    seed_t = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seeds], dtype=torch.int64).to(dev)  # uint64 bits
    x_t, pos_t = per_row(proposal, torch.int32), per_row(position, torch.int32)
    tt, tk, tp = per_row(temperature, torch.float32), per_row(top_k, torch.int32), per_row(top_p, torch.float32)
    dt, dk, dp = per_row(draft_temperature, torch.float32), per_row(draft_top_k, torch.int32), per_row(draft_top_p, torch.float32)
    accept = torch.empty(rows, dtype=torch.int32, device=dev)
    alt = torch.empty(rows, dtype=torch.int32, device=dev)
    check(_lib.tl_spec_sample_rows(target.data_ptr(), draft.data_ptr(), rows, target.shape[1], x_t.data_ptr(), tt.data_ptr(), tk.data_ptr(),
                                   tp.data_ptr(), dt.data_ptr(), dk.data_ptr(), dp.data_ptr(), seed_t.data_ptr(), pos_t.data_ptr(),
                                   accept.data_ptr(), alt.data_ptr(), _stream()))
    return accept, alt


def logprob_rows(logits: torch.Tensor, ids=None, top_n: int = 0):
    """The decode engine's log-probability routine (tl_logprob_rows) over rows of bf16 logits [rows, vocab]: ``ids`` None (each row's
    greedy id), one id for every row or one per row (an id < 0 gives NaN); ``top_n`` 0 .. 20.  Returns (logprob float32 [rows],
    top_ids int32 [rows, top_n], top_logprobs float32 [rows, top_n])."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("logprob_rows takes a [rows, vocab] bf16 tensor on the GPU")
    if isinstance(top_n, bool) or not isinstance(top_n, int) or not 0 <= top_n <= TL_MAX_TOP_LOGPROBS:
        raise ValueError(f"top_n must be an int in [0, {TL_MAX_TOP_LOGPROBS}], got {top_n!r}")
    logits = logits.contiguous()
    rows, dev = logits.shape[0], logits.device
    ids_t = None
    if ids is not None:
        ids_t = torch.as_tensor(ids, dtype=torch.int32).reshape(-1)
        if ids_t.numel() == 1:
            ids_t = ids_t.expand(rows)
        if ids_t.numel() != rows:
            raise ValueError("ids needs one value per row")
        ids_t = ids_t.contiguous().to(dev)
    lp = torch.empty(rows, dtype=torch.float32, device=dev)
    top_ids = torch.empty((rows, top_n), dtype=torch.int32, device=dev)
    top_lp = torch.empty((rows, top_n), dtype=torch.float32, device=dev)
    check(_lib.tl_logprob_rows(logits.data_ptr(), rows, logits.shape[1], ids_t.data_ptr() if ids_t is not None else None, top_n,
                               lp.data_ptr(), top_ids.data_ptr() if top_n else None, top_lp.data_ptr() if top_n else None, _stream()))
    return lp, top_ids, top_lp


def beam_rows(logits: torch.Tensor, scores, n_cand: int) -> list[tuple[int, int, float, float]]:
    """The decode engine's beam-search selection (tl_beam_rows) over 1 .. 8 rows of bf16 logits [rows, vocab] with one cumulative
    log-probability per row: the best ``n_cand`` (1 .. 32) (parent, token, score, logprob), best first; (-1, -1, -inf, -inf) past the
    rankable pairs.  Synchronises."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("beam_rows takes a [rows, vocab] bf16 tensor on the GPU")
    if isinstance(n_cand, bool) or not isinstance(n_cand, int) or not 1 <= n_cand <= TL_MAX_BEAM_CANDIDATES:
        raise ValueError(f"n_cand must be an int in [1, {TL_MAX_BEAM_CANDIDATES}], got {n_cand!r}")
    logits = logits.contiguous()
    rows, dev = logits.shape[0], logits.device
    if not 1 <= rows <= TL_MAX_BEAMS:
        raise ValueError(f"beam_rows takes between 1 and {TL_MAX_BEAMS} rows")
    scores_t = torch.as_tensor(scores, dtype=torch.float32).reshape(-1).contiguous().to(dev)
    if scores_t.numel() != rows:
        raise ValueError("scores needs one value per row")
    out = torch.empty(n_cand * 4, dtype=torch.int32, device=dev)
    check(_lib.tl_beam_rows(logits.data_ptr(), rows, logits.shape[1], scores_t.data_ptr(), n_cand, out.data_ptr(), _stream()))
    words = out.cpu()
    ints, floats = words.view(-1, 4), words.view(torch.float32).view(-1, 4)
    return [(int(ints[i, 0]), int(ints[i, 1]), float(floats[i, 2]), float(floats[i, 3])) for i in range(n_cand)]


def moe_route_rows(logits: torch.Tensor, top_k: int, norm_topk_prob: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """The decode engine's MoE router (tl_moe_route_rows) over rows of bf16 router logits [rows, experts]: (ids [rows, top_k] int32,
    scores [rows, top_k] bf16), descending probability, equal probabilities the lower expert first.  Stream ordered."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("moe_route_rows takes a [rows, experts] bf16 tensor on the GPU")
    logits = logits.contiguous()
    rows, dev = logits.shape[0], logits.device
    k = max(int(top_k), 0)
    ids = torch.empty((rows, k), dtype=torch.int32, device=dev)
    scores = torch.empty((rows, k), dtype=torch.bfloat16, device=dev)
    check(_lib.tl_moe_route_rows(logits.data_ptr(), rows, logits.shape[1], int(top_k), int(bool(norm_topk_prob)), ids.data_ptr(), scores.data_ptr(),
                                 _stream()))
    return ids, scores


def moe_experts_rows(xn: torch.Tensor, h: torch.Tensor, ids: torch.Tensor, scores: torch.Tensor, gate, up, down) -> tuple[torch.Tensor, dict]:
    """Everything of the engine's MoE MLP behind the router (tl_moe_experts_rows) over bf16 rows ``xn`` / ``h`` [rows, hidden] with the
    caller's ``ids`` [rows, top_k] int32 and ``scores`` [rows, top_k] bf16.  ``gate`` / ``up`` / ``down``: (weight [E, out, in/8] int32 words,
    scales, biases [E, out, in/128] bf16) of the stacked experts.  Returns (out [rows, hidden] bf16, the stages as the call's workspace
    holds them: {"gate", "up", "act": [rows * top_k, I], "y": [rows * top_k, hidden]}).  Stream ordered."""
    for t in (xn, h, scores, *gate[1:], *up[1:], *down[1:]):
        if t.dtype != torch.bfloat16 or not t.is_cuda:
            raise ValueError("moe_experts_rows takes bf16 tensors on the GPU")
    if ids.dtype != torch.int32 or not ids.is_cuda or ids.dim() != 2 or ids.shape != scores.shape or xn.shape != h.shape or xn.dim() != 2:
        raise ValueError("moe_experts_rows: xn / h [rows, hidden], ids (int32) / scores [rows, top_k]")
    xn, h, ids, scores = xn.contiguous(), h.contiguous(), ids.contiguous(), scores.contiguous()
    gate, up, down = (tuple(t.contiguous() for t in w) for w in (gate, up, down))
    (rows, hidden), k, dev = xn.shape, ids.shape[1], xn.device
    n_experts, inter = gate[0].shape[0], gate[0].shape[1]
    if ids.shape[0] != rows or gate[0].shape[2] * 8 != hidden or up[0].shape != gate[0].shape or down[0].shape != (n_experts, hidden, inter // 8):
        raise ValueError("moe_experts_rows: the expert tensors do not fit the rows")
    w = TlMoeWeights(TlW4(), gate[0].data_ptr(), up[0].data_ptr(), down[0].data_ptr(), gate[1].data_ptr(), gate[2].data_ptr(), up[1].data_ptr(),
                     up[2].data_ptr(), down[1].data_ptr(), down[2].data_ptr(), n_experts, k, inter, 0)
    nbytes = _lib.tl_moe_experts_workspace_bytes(rows, k, hidden, inter)
    ws = torch.empty(max(nbytes, 16) // 2, dtype=torch.bfloat16, device=dev)
    out = torch.empty_like(xn)
    check(_lib.tl_moe_experts_rows(xn.data_ptr(), h.data_ptr(), ids.data_ptr(), scores.data_ptr(), ctypes.byref(w), rows, hidden, out.data_ptr(),
                                   ws.data_ptr(), nbytes, _stream()))
    n = rows * k * inter
    stages = {"gate": ws[:n].view(rows * k, inter), "up": ws[n:2 * n].view(rows * k, inter), "act": ws[2 * n:3 * n].view(rows * k, inter),
              "y": ws[3 * n:3 * n + rows * k * hidden].view(rows * k, hidden)}
    return out, stages


POOL_LAST, POOL_MEAN = 0, 1  # TL_POOL_LAST / TL_POOL_MEAN
POOLING_MODES = {"last": POOL_LAST, "mean": POOL_MEAN}


def pooling_args(pooling, normalize, dim, hidden: int) -> tuple[int, int, int]:
    """(pooling mode, normalize, dim) as the C ABI takes them; ``dim`` None = ``hidden``.  ValueError for anything else."""
    if not isinstance(pooling, str) or pooling not in POOLING_MODES:
        raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
    if not isinstance(normalize, (bool, int)) or normalize not in (0, 1):
        raise ValueError(f"normalize must be a bool, got {normalize!r}")
    dim = hidden if dim is None else dim
    if isinstance(dim, bool) or not isinstance(dim, int) or not 1 <= dim <= hidden:
        raise ValueError(f"dim must be an int in [1, {hidden}], got {dim!r}")
    return POOLING_MODES[pooling], int(normalize), dim


def pool_rows(rows: torch.Tensor, seqs, *, pooling: str = "last", normalize: bool = True, dim: int | None = None, finish=None, prior=None,
              sums: torch.Tensor | None = None) -> torch.Tensor:
    """The engine's pooling routine (tl_pool_rows) over final-normalised bf16 rows [total, hidden]: ``seqs`` = up to 16 (row0, len) pairs;
    ``finish`` (default: all) marks the sequences whose vector is written; mean pooling accumulates into ``sums`` [n_seqs, hidden] float32
    (allocated when None), whose row i already holds ``prior[i]`` rows (default 0: it is replaced).  Returns float32 [finishing, dim]."""
    if rows.dtype != torch.bfloat16 or rows.dim() != 2 or not rows.is_cuda:
        raise ValueError("pool_rows takes a [total, hidden] bf16 tensor on the GPU")
    rows = rows.contiguous()
    total, hidden = rows.shape
    mode, norm, dim = pooling_args(pooling, normalize, dim, hidden)
    seqs = [(int(a), int(b)) for a, b in seqs]
    n = len(seqs)
    if not 1 <= n <= 16:
        raise ValueError("pool_rows takes between 1 and 16 sequences")
    for r0, ln in seqs:
        if r0 < 0 or ln < 1 or r0 + ln > total:
            raise ValueError(f"sequence ({r0}, {ln}) is outside the {total} rows")
    finish = [1] * n if finish is None else [int(bool(f)) for f in finish]
    prior = [0] * n if prior is None else [int(p) for p in prior]
    if len(finish) != n or len(prior) != n:
        raise ValueError("finish and prior need one value per sequence")
    if mode == POOL_MEAN:
        if sums is None:
            sums = torch.zeros((n, hidden), dtype=torch.float32, device=rows.device)
        if sums.dtype != torch.float32 or tuple(sums.shape) != (n, hidden) or not sums.is_cuda or not sums.is_contiguous():
            raise ValueError("sums must be a contiguous [n_seqs, hidden] float32 tensor on the GPU")
    out = torch.empty((sum(finish), dim), dtype=torch.float32, device=rows.device)
    ints = lambda v: (ctypes.c_int * n)(*v)
    check(_lib.tl_pool_rows(rows.data_ptr(), hidden, n, ints([s[0] for s in seqs]), ints([s[1] for s in seqs]), ints(finish), ints(prior), mode,
                            sums.data_ptr() if mode == POOL_MEAN else None, norm, dim, out.data_ptr() if out.numel() else None, _stream()))
    return out


def lora_rows(x: torch.Tensor, row_adapter, adapters, *, out_cols: int, mode: str = "add", base: torch.Tensor | None = None,
              seg_mode: str = "plain", seg_ends=(0, 0), tiles=None, norm_weight: torch.Tensor | None = None, eps: float = 1e-6) -> torch.Tensor:
    """The engine's LoRA routine (tl_lora_rows, csrc/lora.h) over bf16 rows ``x`` [rows, in] for one projection group of ``out_cols``
    columns.  ``row_adapter``: per row the index of its adapter in ``adapters`` or -1; ``adapters``: (A, B, scale, seg_mask) in the
    FUSED layout -- A [rank * present segments, in], B [out_cols, rank], bf16 on the GPU; seg_mask bit s = segment s is present.
    ``seg_mode``: "plain", "blocks" (three column blocks ending at seg_ends[0], seg_ends[1], out_cols: q | k | v) or "interleaved"
    (column parity: gate | up).  ``tiles``: None (blocks of 16 rows that look every row up) or (row0, rows <= 16, adapter) triples with
    adapter -1 = none, -2 = per row.  ``mode``: "add" -> bf16(base + delta) [rows, out_cols]; "residual_pre" -> the same over a residual;
    "swiglu" -> base holds interleaved gate|up rows, returns [rows, out_cols / 2].  ``norm_weight``: x is the row ahead of an RMSNorm of
    that weight and ``eps``, applied inside."""
    if mode not in LORA_MODES or seg_mode not in LORA_SEG_MODES:
        raise ValueError(f"lora_rows: mode is one of {sorted(LORA_MODES)}, seg_mode one of {sorted(LORA_SEG_MODES)}")
    if x.dtype != torch.bfloat16 or x.dim() != 2 or not x.is_cuda:
        raise ValueError("lora_rows takes a [rows, in] bf16 tensor on the GPU")
    x = x.contiguous()
    rows, cols = x.shape
    if base is None or base.dtype != torch.bfloat16 or tuple(base.shape) != (rows, out_cols) or not base.is_cuda:
        raise ValueError("lora_rows: base must be a [rows, out_cols] bf16 tensor on the GPU")
    base = base.contiguous()
    keep = []
    mats = (TlLoraMatrices * max(len(adapters), 1))()
    for i, (a, b, scale, mask) in enumerate(adapters):
        if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or not a.is_cuda or not b.is_cuda or a.dim() != 2 or b.dim() != 2:
            raise ValueError("lora_rows: adapter matrices are 2-D bf16 tensors on the GPU")
        a, b = a.contiguous(), b.contiguous()
        rank = b.shape[1]
        if a.shape[1] != cols or b.shape[0] != out_cols or a.shape[0] != rank * bin(int(mask)).count("1"):
            raise ValueError("lora_rows: A must be [rank * present segments, in] and B [out_cols, rank]")
        keep += [a, b]
        mats[i] = TlLoraMatrices(a.data_ptr(), b.data_ptr(), int(rank), int(mask), float(scale))
    ids = torch.as_tensor(list(row_adapter), dtype=torch.int32).to(x.device) if not isinstance(row_adapter, torch.Tensor) else row_adapter.to(x.device, torch.int32).contiguous()
    if ids.numel() != rows:
        raise ValueError("lora_rows: row_adapter needs one id per row")
    if int(ids.max()) >= len(adapters) or int(ids.min()) < -1:
        raise ValueError("lora_rows: a row's adapter is -1 or an index into adapters")
    if norm_weight is not None:
        if norm_weight.dtype != torch.bfloat16 or tuple(norm_weight.shape) != (cols,) or not norm_weight.is_cuda:
            raise ValueError("lora_rows: norm_weight must be a [in] bf16 tensor on the GPU")
        norm_weight = norm_weight.contiguous()
    n_tiles = 0 if tiles is None else len(tiles)
    arr = lambda k: (ctypes.c_int * max(n_tiles, 1))(*[int(t[k]) for t in (tiles or [])])
    if LORA_MODES[mode] == 0:
        out = base.clone()
    elif LORA_MODES[mode] == 1:
        out = torch.empty_like(base)
    else:
        out = torch.empty((rows, out_cols // 2), dtype=torch.bfloat16, device=x.device)
    check(_lib.tl_lora_rows(x.data_ptr(), rows, cols, out_cols, ids.data_ptr(), mats, len(adapters), LORA_SEG_MODES[seg_mode], int(seg_ends[0]),
                            int(seg_ends[1]), arr(0), arr(1), arr(2), n_tiles, LORA_MODES[mode], base.data_ptr(), out.data_ptr(),
                            norm_weight.data_ptr() if norm_weight is not None else None, float(eps), _stream()))
    return out


def process_logits(logits: torch.Tensor, history: torch.Tensor, repetition=1.0, presence=0.0, frequency=0.0, bias=None) -> torch.Tensor:
    """The decode engine's logit processing (tl_process_logits) over rows of bf16 logits [rows, vocab]: ``history`` [rows, vocab] of
    uint16 bits in an int16 tensor (bit 15 = the token was in the prompt, bits 0-14 = how often it was produced); per-row repetition /
    presence / frequency penalties (a scalar or one value per row); ``bias`` None, or one {id: value} dict per row (None for a row
    without a list; at most TL_MAX_LOGIT_BIAS entries each).  Returns the processed rows [rows, vocab] bf16."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("process_logits takes a [rows, vocab] bf16 tensor on the GPU")
    if history.dtype != torch.int16 or history.shape != logits.shape or not history.is_cuda:
        raise ValueError("history must be an int16 tensor (uint16 bits) of the logits' shape on the GPU")
    logits, history = logits.contiguous(), history.contiguous()
    rows, vocab, dev = logits.shape[0], logits.shape[1], logits.device

    def per_row(v):
        t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(rows)
        if t.numel() != rows:
            raise ValueError("a penalty needs one value per row")
        return t.contiguous().to(dev)

    r_t, p_t, f_t = per_row(repetition), per_row(presence), per_row(frequency)
    lists = [None] * rows if bias is None else list(bias)
    if len(lists) != rows:
        raise ValueError("bias needs one dict (or None) per row")
    n_h = torch.zeros(rows, dtype=torch.int32)
    ids_h = torch.zeros((rows, TL_MAX_LOGIT_BIAS), dtype=torch.int32)
    vals_h = torch.zeros((rows, TL_MAX_LOGIT_BIAS), dtype=torch.float32)
    for i, d in enumerate(lists):
        ids, vals = logit_bias_arg(d, vocab)
        n_h[i] = len(ids)
        if ids:
            ids_h[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
            vals_h[i, :len(ids)] = torch.tensor(vals, dtype=torch.float32)
    n_t, ids_t, vals_t = n_h.to(dev), ids_h.to(dev), vals_h.to(dev)
    out = torch.empty_like(logits)
    check(_lib.tl_process_logits(logits.data_ptr(), rows, vocab, history.data_ptr(), r_t.data_ptr(), p_t.data_ptr(), f_t.data_ptr(),
                                 ids_t.data_ptr(), vals_t.data_ptr(), n_t.data_ptr(), out.data_ptr(), _stream()))
    return out


def dry_rows(logits: torch.Tensor, sequences: torch.Tensor, start, end, multiplier=0.0, base=1.75, allowed_length=2, range=0,  # noqa: A002
             no_repeat_ngram=0, breakers=None, table: torch.Tensor | None = None) -> torch.Tensor:
    """The decode engine's DRY and n-gram ban (tl_dry_rows) over rows of bf16 logits [rows, vocab]: ``sequences`` [rows, cap] int32 on the
    GPU, row r holding S[start[r] .. end[r]]; the parameters a scalar or one value per row; ``breakers`` None, or one sequence of token ids
    per row (at most TL_MAX_DRY_BREAKERS each).  ``table``: the match table [rows, vocab] of uint32 words in an int32 tensor, all zeros
    (made here when None); it is all zeros again after the call.  Returns the rewritten rows [rows, vocab] bf16."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("dry_rows takes a [rows, vocab] bf16 tensor on the GPU")
    if sequences.dtype != torch.int32 or sequences.dim() != 2 or sequences.shape[0] != logits.shape[0] or not sequences.is_cuda:
        raise ValueError("sequences must be a [rows, cap] int32 tensor on the GPU")
    rows, vocab, dev = logits.shape[0], logits.shape[1], logits.device
    sequences = sequences.contiguous()
    cap = sequences.shape[1]

    def per_row(v, dtype, what):
        t = torch.as_tensor(v, dtype=dtype).reshape(-1)
        if t.numel() == 1:
            t = t.expand(rows)
        if t.numel() != rows:
            raise ValueError(f"{what} needs one value per row")
        return t.contiguous().to(dev)

    start_t, end_t = per_row(start, torch.int32, "start"), per_row(end, torch.int32, "end")
    if int(end_t.max()) >= cap:
        raise ValueError("end must lie inside the sequence capacity")
    m_t, b_t = per_row(multiplier, torch.float32, "multiplier"), per_row(base, torch.float32, "base")
    a_t, r_t = per_row(allowed_length, torch.int32, "allowed_length"), per_row(range, torch.int32, "range")
    n_t = per_row(no_repeat_ngram, torch.int32, "no_repeat_ngram")
    lists = [()] * rows if breakers is None else [tuple(b or ()) for b in breakers]
    if len(lists) != rows:
        raise ValueError("breakers needs one sequence (or None) per row")
    nb_h = torch.zeros(rows, dtype=torch.int32)
    brk_h = torch.zeros((rows, TL_MAX_DRY_BREAKERS), dtype=torch.int32)
    for i, ids in enumerate(lists):
        if len(ids) > TL_MAX_DRY_BREAKERS:
            raise ValueError(f"at most {TL_MAX_DRY_BREAKERS} breakers per row")
        nb_h[i] = len(ids)
        if ids:
            brk_h[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    nb_t, brk_t = nb_h.to(dev), brk_h.to(dev)
    if table is None:
        table = torch.zeros((rows, vocab), dtype=torch.int32, device=dev)
    if table.dtype != torch.int32 or tuple(table.shape) != (rows, vocab) or not table.is_cuda or not table.is_contiguous():
        raise ValueError("table must be a contiguous [rows, vocab] int32 tensor on the GPU")
    out = logits.contiguous().clone()
    check(_lib.tl_dry_rows(sequences.data_ptr(), rows, cap, start_t.data_ptr(), end_t.data_ptr(), m_t.data_ptr(), b_t.data_ptr(), a_t.data_ptr(),
                           r_t.data_ptr(), n_t.data_ptr(), brk_t.data_ptr(), nb_t.data_ptr(), table.data_ptr(), out.data_ptr(), vocab, _stream()))
    return out


def lookup_params(max_ngram: int, min_ngram: int, num_proposals: int) -> tuple[int, int, int]:
    """Validated (max_ngram, min_ngram, num_proposals) of the prompt-lookup rule: max_ngram 1 .. 16, min_ngram 1 .. max_ngram,
    num_proposals 1 .. 7."""
    for name, v in (("max_ngram", max_ngram), ("min_ngram", min_ngram), ("num_proposals", num_proposals)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if not 1 <= max_ngram <= TL_LOOKUP_MAX_NGRAM:
        raise ValueError(f"max_ngram must be 1 .. {TL_LOOKUP_MAX_NGRAM}, got {max_ngram!r}")
    if not 1 <= min_ngram <= max_ngram:
        raise ValueError(f"min_ngram must be 1 .. max_ngram, got {min_ngram!r}")
    if not 1 <= num_proposals <= TL_LOOKUP_MAX_PROPOSALS:
        raise ValueError(f"num_proposals must be 1 .. {TL_LOOKUP_MAX_PROPOSALS}, got {num_proposals!r}")
    return max_ngram, min_ngram, num_proposals


def lookup_rows(sequences: torch.Tensor, start, end, max_ngram: int = 3, min_ngram: int = 1, num_proposals: int = 4, want_match: bool = False):
    """The decode engine's prompt-lookup rule (tl_lookup_rows) over rows of ids: ``sequences`` [rows, cap] int32 on the GPU, row r holding
    T[start[r] .. end[r]] (``start`` / ``end``: a scalar or one value per row; a row with end < start has no proposals).  Returns
    (proposals [rows, 8] int32 with -1 behind each row's proposals, counts [rows] int32) and, with ``want_match``, also match [rows, 2]:
    the chosen position and its match length, (-1, 0) without a choice."""
    if not isinstance(sequences, torch.Tensor) or sequences.dtype != torch.int32 or sequences.dim() != 2 or not sequences.is_cuda:
        raise ValueError("lookup_rows takes a [rows, cap] int32 tensor on the GPU")
    lookup_params(max_ngram, min_ngram, num_proposals)
    rows, cap, dev = sequences.shape[0], sequences.shape[1], sequences.device
    if rows < 1 or cap < 1:
        raise ValueError("lookup_rows needs at least one row and one id per row")
    sequences = sequences.contiguous()

    def per_row(v, what):
        t = torch.as_tensor(v, dtype=torch.int32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(rows)
        if t.numel() != rows:
            raise ValueError(f"{what} needs one value per row")
        return t.contiguous().to(dev)

    start_t, end_t = per_row(start, "start"), per_row(end, "end")
    if int(end_t.max()) >= cap:
        raise ValueError("end must lie inside the sequence capacity")
    proposals = torch.empty((rows, 8), dtype=torch.int32, device=dev)
    counts = torch.empty(rows, dtype=torch.int32, device=dev)
    match = torch.empty((rows, 2), dtype=torch.int32, device=dev) if want_match else None
    check(_lib.tl_lookup_rows(sequences.data_ptr(), rows, cap, start_t.data_ptr(), end_t.data_ptr(), max_ngram, min_ngram, num_proposals,
                              proposals.data_ptr(), counts.data_ptr(), match.data_ptr() if want_match else None, _stream()))
    return (proposals, counts, match) if want_match else (proposals, counts)


def _rows_f32(v, rows: int, dev, what: str) -> torch.Tensor:
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(rows)
    if t.numel() != rows:
        raise ValueError(f"{what} needs one value per row")
    return t.contiguous().to(dev)


def truncate_rows(logits: torch.Tensor, temperature, min_p=0.0, typical_p=1.0, mu=float("nan")):
    """The decode engine's truncation (tl_truncate_rows) over rows of bf16 logits [rows, vocab]: per-row temperature, min_p (0 = off),
    typical_p (outside (0, 1) = off) and Mirostat's mu (NaN = no Mirostat; a Mirostat row ignores the other two), each a scalar or one
    value per row.  Returns (filtered rows [rows, vocab] bf16, kept log-sums float32 [rows]: ln sum_kept exp(x / T) of a Mirostat row)."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("truncate_rows takes a [rows, vocab] bf16 tensor on the GPU")
    logits = logits.contiguous()
    rows, dev = logits.shape[0], logits.device
    t_t, m_t, y_t, mu_t = (_rows_f32(v, rows, dev, "a truncation parameter") for v in (temperature, min_p, typical_p, mu))
    out = torch.empty_like(logits)
    logsum = torch.empty(rows, dtype=torch.float32, device=dev)
    check(_lib.tl_truncate_rows(logits.data_ptr(), rows, logits.shape[1], t_t.data_ptr(), m_t.data_ptr(), y_t.data_ptr(), mu_t.data_ptr(),
                                out.data_ptr(), logsum.data_ptr(), _stream()))
    return out, logsum


def mirostat_update_rows(filtered: torch.Tensor, ids, temperature, kept_logsum: torch.Tensor, tau, eta, mu) -> torch.Tensor:
    """Mirostat's update (tl_mirostat_update_rows) for the tokens ``ids`` [rows] chosen from the filtered rows of truncate_rows and
    their kept log-sums: returns the new mu float32 [rows] (``mu`` itself is not changed)."""
    if filtered.dtype != torch.bfloat16 or filtered.dim() != 2 or not filtered.is_cuda:
        raise ValueError("mirostat_update_rows takes a [rows, vocab] bf16 tensor on the GPU")
    filtered = filtered.contiguous()
    rows, dev = filtered.shape[0], filtered.device
    ids_t = torch.as_tensor(ids, dtype=torch.int32).reshape(-1).contiguous().to(dev)
    if ids_t.numel() != rows or kept_logsum.dtype != torch.float32 or kept_logsum.numel() != rows or not kept_logsum.is_cuda:
        raise ValueError("ids and kept_logsum (float32, on the GPU) need one value per row")
    t_t, tau_t, eta_t = (_rows_f32(v, rows, dev, "a Mirostat parameter") for v in (temperature, tau, eta))
    mu_t = _rows_f32(mu, rows, dev, "mu").clone()
    check(_lib.tl_mirostat_update_rows(filtered.data_ptr(), rows, filtered.shape[1], ids_t.data_ptr(), t_t.data_ptr(), kept_logsum.contiguous().data_ptr(),
                                       tau_t.data_ptr(), eta_t.data_ptr(), mu_t.data_ptr(), _stream()))
    return mu_t


def stop_rows(stop, tokens: torch.Tensor, states: torch.Tensor, automaton: torch.Tensor, max_new: torch.Tensor, armed: torch.Tensor | None = None) -> None:
    """The stop check (tl_stop_rows) over caller rows, in place: ``stop`` a tl_stop handle (a tiny_llm_hip.stop.StopSet's ``_h``) or
    None (budgets alone); ``tokens`` int32 [rows]; ``states`` int32 [rows, 6], the rows' tl_stop_state records (reason, index,
    generated, context, text_bytes, cut_bytes); ``automaton`` int32 [rows]; ``max_new`` int32 [rows]; ``armed`` int32 [rows] or None
    (every row).  All on the GPU and contiguous."""
    rows = tokens.numel()
    for t, shape in ((tokens, (rows,)), (states, (rows, 6)), (automaton, (rows,)), (max_new, (rows,))) + (((armed, (rows,)),) if armed is not None else ()):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_cuda or not t.is_contiguous():
            raise ValueError("stop_rows takes contiguous int32 tensors on the GPU: tokens / automaton / max_new / armed [rows], states [rows, 6]")
    check(_lib.tl_stop_rows(stop, tokens.data_ptr(), rows, armed.data_ptr() if armed is not None else None, max_new.data_ptr(), automaton.data_ptr(),
                            states.data_ptr(), _stream()))


def logit_bias_arg(bias, vocab: int) -> tuple[list[int], list[float]]:
    """Validated (ids, values) of a logit-bias list for tl_engine_set_logit_bias: None or a mapping {token id: value} of at most
    TL_MAX_LOGIT_BIAS entries, ids ints in [0, vocab) (distinct: 3 and 3.0 or True are refused, not merged), values finite or -inf."""
    if bias is None:
        return [], []
    if not hasattr(bias, "items"):
        raise ValueError("logit_bias must be None or a mapping {token id: value}")
    items = list(bias.items())
    if len(items) > TL_MAX_LOGIT_BIAS:
        raise ValueError(f"logit_bias takes at most {TL_MAX_LOGIT_BIAS} entries, got {len(items)}")
    ids, vals = [], []
    for k, v in items:
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < vocab:
            raise ValueError(f"logit_bias id must be an int in [0, {vocab}), got {k!r}")
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v == float("inf"):
            raise ValueError(f"logit_bias value must be finite or -inf, got {v!r}")
        ids.append(int(k))
        vals.append(float(v))
    if len(set(ids)) != len(ids):
        raise ValueError("logit_bias ids must be distinct")
    return ids, vals
