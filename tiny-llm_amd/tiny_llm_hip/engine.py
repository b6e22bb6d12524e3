"""Fused decode engine: host mirror of include/tinyllm_engine.h.

The reference decodes by calling its operators one by one from Python (``Qwen3ModelWeek3.__call__``,
src/tiny_llm_ref/qwen3_week3.py:320-338, driven by benches/bench.py:run_one_request_week2 277-312).  That
loop is kept (``Qwen3ModelWeek2/3`` in this package run it op by op on the HIP operators); this module is
the production path behind it: the same arithmetic issued as 5 fused kernels per layer inside one replayed
hipGraph, with tokens / context lengths / block tables resident on the device.

``DecodeEngine.from_model(mlx_shaped_model)`` re-packs the checkpoint once (QKV rows concatenated, gate/up
rows interleaved) and then exposes a request-level API: ``begin`` / ``prefill`` / ``decode`` / ``release``.
"""

from __future__ import annotations

import ctypes
import os
from typing import Any, NamedTuple, Sequence

import torch

from . import scheduler
from .request import (DRY_OFF, SETTINGS_KEYS, RequestSettings, dry_args, dry_breaker_ids, logprobs_arg, penalty_args,  # noqa: F401
                      request_settings, sampling_args, truncation_args)
from ._ext import tiny_llm_ext_hip as _ext

_lib = _ext.lib()


def _w4(weight: torch.Tensor, scales: torch.Tensor, biases: torch.Tensor) -> "_ext.TlW4":
    rows, words = weight.shape
    return _ext.TlW4(weight.data_ptr(), scales.data_ptr(), biases.data_ptr(), rows, words * 8)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype != torch.int32 else t


class _Fused:
    """Keeps the re-packed tensors alive for the lifetime of the engine."""

    def __init__(self, weight, scales, biases):
        self.weight = _bits(weight).contiguous()
        self.scales = scales.to(torch.bfloat16).contiguous()
        self.biases = biases.to(torch.bfloat16).contiguous()

    @staticmethod
    def concat(layers: Sequence[Any]) -> "_Fused":
        return _Fused(torch.cat([_bits(l.weight) for l in layers], 0), torch.cat([l.scales for l in layers], 0),
                      torch.cat([l.biases for l in layers], 0))

    @staticmethod
    def interleave(a: Any, b: Any) -> "_Fused":
        def il(x, y):
            return torch.stack([x, y], dim=1).reshape(x.shape[0] * 2, *x.shape[1:])

        return _Fused(il(_bits(a.weight), _bits(b.weight)), il(a.scales, b.scales), il(a.biases, b.biases))

    def c(self) -> "_ext.TlW4":
        return _w4(self.weight, self.scales, self.biases)


class DecodeEngine:
    """Owns the fused weights, the paged KV pools and the captured decode graphs for one model on one GPU."""

    def __init__(self, mlx_model: Any, *, page_size: int = 128, num_pages: int = 512, max_batch: int = 1,
                 max_pages_per_seq: int | None = None, max_prefill_rows: int = 2048, options: dict | None = None,
                 kv_format: str = "bf16", prefix_cache: bool | int = False, swap_pages: int = 0):
        """``swap_pages``: room for that many KV pages in pinned host memory (tl_engine_swap_space): ``park`` moves a sequence's K / V
        there and frees its pages, ``unpark`` brings it back, and the serving loops preempt under page pressure instead of failing
        (tiny_llm_hip.preempt).  0 (the default): nothing is allocated and the loops are the programs they were.
        ``prefix_cache``: keep the K / V of full pages after their request is released and hand them to later requests that start
        with the same tokens (tl_engine_prefix_cache; prefix_attach / prefix_extend); an int (> 0) also caps the retained pages.  Off
        by default: the engine then is the program it was.
        ``kv_format``: "bf16" (the reference's cache) or "fp8" -- K / V pages as OCP FP8 E4M3 codes with one power-of-two scale per
        row (tl_engine_create_kv; head_dim 128; the reference has no quantised cache, README.md:134-135: an extension, off by default).
        ``options`` (tests / lab tools only): routes with an A/B twin, by the names of tl_engine_set_option (include/tinyllm_engine.h),
        e.g. {"qmm7": 0}; the environment variable TL_ENGINE_OPTIONS ("qmm7=0,aql_fences=1") adds to them for the A/B scripts under tools/."""
        args = mlx_model.args
        if not torch.cuda.is_available():
            raise RuntimeError("DecodeEngine: the course extension is GPU-only")
        self.args = args
        self._keep: list[Any] = []
        layers = (_ext.TlLayerWeights * args.num_hidden_layers)()
        moe_layers: dict[int, Any] = {}  # Qwen3-MoE layers (reference qwen3_week3.py:209-214, 258-272): attached after create
        for i, layer in enumerate(mlx_model.model.layers):
            attn, mlp = layer.self_attn, layer.mlp
            qkv = _Fused.concat([attn.q_proj, attn.k_proj, attn.v_proj])
            wo = _Fused(attn.o_proj.weight, attn.o_proj.scales, attn.o_proj.biases)
            norms = [layer.input_layernorm.weight, layer.post_attention_layernorm.weight, attn.q_norm.weight,
                     attn.k_norm.weight]
            norms = [n.to(torch.bfloat16).contiguous() for n in norms]
            if hasattr(mlp, "switch_mlp"):  # router + stacked experts: no dense MLP in this layer
                moe_layers[i] = mlp
                none = _ext.TlW4(None, None, None, 0, 0)
                self._keep += [qkv, wo, norms]
                layers[i] = _ext.TlLayerWeights(qkv.c(), wo.c(), none, none, norms[0].data_ptr(), norms[1].data_ptr(),
                                                norms[2].data_ptr(), norms[3].data_ptr())
                continue
            gu = _Fused.interleave(mlp.gate_proj, mlp.up_proj)
            down = _Fused(mlp.down_proj.weight, mlp.down_proj.scales, mlp.down_proj.biases)
            self._keep += [qkv, wo, gu, down, norms]
            layers[i] = _ext.TlLayerWeights(qkv.c(), wo.c(), gu.c(), down.c(), norms[0].data_ptr(),
                                            norms[1].data_ptr(), norms[2].data_ptr(), norms[3].data_ptr())
        emb = mlx_model.model.embed_tokens
        embed = _Fused(emb.weight, emb.scales, emb.biases)
        final_norm = mlx_model.model.norm.weight.to(torch.bfloat16).contiguous()
        self._keep += [embed, final_norm]
        head = None
        if not getattr(args, "tie_word_embeddings", True):
            hl = mlx_model.lm_head
            head = _Fused(hl.weight, hl.scales, hl.biases)
            self._keep.append(head)
        if max_pages_per_seq is None:
            max_pages_per_seq = num_pages
        cfg = _ext.TlEngineConfig(
            args.hidden_size, args.num_hidden_layers, args.num_attention_heads, args.num_key_value_heads,
            args.head_dim, args.intermediate_size, args.vocab_size, float(args.rope_theta), float(args.rms_norm_eps),
            page_size, num_pages, max_batch, max_pages_per_seq, max_prefill_rows)
        self.page_size, self.max_batch, self.vocab_size = page_size, max_batch, args.vocab_size
        self.max_prefill_rows = int(max_prefill_rows)
        self.max_pages_per_seq = int(max_pages_per_seq)
        self.num_hidden_layers = int(args.num_hidden_layers)
        self.device = emb.weight.device
        handle = ctypes.c_void_p()
        embed_c = embed.c()
        head_c = head.c() if head is not None else None
        if kv_format not in ("bf16", "fp8"):
            raise ValueError("DecodeEngine: kv_format must be 'bf16' or 'fp8'")
        self.kv_format = kv_format
        _ext.check(_lib.tl_engine_create_kv(
            ctypes.byref(cfg), layers, ctypes.byref(embed_c), final_norm.data_ptr(),
            ctypes.byref(head_c) if head_c is not None else None, None,
            _ext.KV_FP8_E4M3 if kv_format == "fp8" else _ext.KV_BF16, ctypes.byref(handle)))
        self._h = handle
        opts = dict(item.split("=", 1) for item in os.environ.get("TL_ENGINE_OPTIONS", "").replace("+", ",").split(",") if "=" in item)
        opts.update(options or {})
        for name, value in opts.items():
            _ext.check(_lib.tl_engine_set_option(self._h, str(name).strip().encode(), int(value)))
        for i, mlp in moe_layers.items():
            self._attach_moe(i, mlp, args)
        if isinstance(prefix_cache, bool):
            cap = 0
        elif isinstance(prefix_cache, int) and prefix_cache > 0:
            cap = prefix_cache
        else:
            raise ValueError(f"prefix_cache must be a bool or a positive int (the retention cap in pages), got {prefix_cache!r}")
        self.prefix_cache_enabled = bool(prefix_cache)
        if self.prefix_cache_enabled:
            _ext.check(_lib.tl_engine_prefix_cache(self._h, 1, cap))
        if isinstance(swap_pages, bool) or not isinstance(swap_pages, int) or swap_pages < 0:
            raise ValueError(f"swap_pages must be an int >= 0 (host records of one KV page each), got {swap_pages!r}")
        self.swap_enabled = swap_pages > 0
        if self.swap_enabled:
            _ext.check(_lib.tl_engine_swap_space(self._h, swap_pages))

    def _attach_moe(self, layer: int, mlp: Any, args: Any) -> None:
        """Hand the router and the stacked experts of one sparse layer to the engine (tl_engine_set_moe_layer)."""
        router = _Fused(mlp.gate.weight, mlp.gate.scales, mlp.gate.biases)
        sw = mlp.switch_mlp
        experts = {}
        for name in ("gate_proj", "up_proj", "down_proj"):
            p = getattr(sw, name)
            w = _bits(p.weight).contiguous()
            if w.dim() != 3:
                raise ValueError(f"layer {layer}: switch_mlp.{name}.weight must be [experts, rows, words]")
            experts[name] = (w, p.scales.to(torch.bfloat16).contiguous(), p.biases.to(torch.bfloat16).contiguous())
        n_experts, inter, _ = experts["gate_proj"][0].shape
        self._keep += [router, experts]
        g, u, d = experts["gate_proj"], experts["up_proj"], experts["down_proj"]
        w = _ext.TlMoeWeights(router.c(), g[0].data_ptr(), u[0].data_ptr(), d[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
                              u[1].data_ptr(), u[2].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), int(n_experts),
                              int(args.num_experts_per_tok), int(inter), int(bool(getattr(args, "norm_topk_prob", False))))
        _ext.check(_lib.tl_engine_set_moe_layer(self._h, layer, ctypes.byref(w)))

    @classmethod
    def from_model(cls, mlx_model: Any, **kwargs) -> "DecodeEngine":
        return cls(mlx_model, **kwargs)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.tl_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- slots -------------------------------------------------------------------------------------
    def _held_stops(self) -> dict:
        """slot -> the StopSet it is armed with (set_stop): the engine borrows the set, this keeps it alive."""
        return self.__dict__.setdefault("_stop_sets", {})

    def begin(self, slot: int = 0) -> None:
        _ext.check(_lib.tl_engine_begin(self._h, slot))
        self._held_stops().pop(slot, None)

    def reserve(self, slot: int, total_tokens: int) -> None:
        _ext.check(_lib.tl_engine_reserve(self._h, slot, total_tokens))

    def release(self, slot: int = 0) -> None:
        _ext.check(_lib.tl_engine_release(self._h, slot))
        self._held_stops().pop(slot, None)

    def rewind(self, slot: int, n: int) -> None:
        _ext.check(_lib.tl_engine_rewind(self._h, slot, n))

    def move(self, src: int, dst: int) -> None:
        _ext.check(_lib.tl_engine_move(self._h, src, dst))
        held = self._held_stops()
        if src in held:
            held[dst] = held.pop(src)

    def fork(self, src: int, dst: int) -> None:
        """Make free slot ``dst`` a copy-on-write twin of ``src`` (shared prefix pages, own tail page)."""
        _ext.check(_lib.tl_engine_fork(self._h, src, dst))
        held = self._held_stops()
        if src in held:
            held[dst] = held[src]

    # -- beam search (tl_engine_beam_*; include/tinyllm_engine.h "Beam search"; the policy is beam.py) --------
    def beam_select(self, row0: int, rows: int, scores: Sequence[float], n_cand: int) -> list[tuple[int, int, float, float]]:
        """The best ``n_cand`` (1 .. 32) continuations of the beams behind rows [row0, row0 + rows) of the most recent logits (after a
        decode step row i is slot i; after a prefill there is row 0), ranked on the device: ``scores`` are the beams' cumulative
        log-probabilities, the result (parent, token, score, logprob) tuples, best first, (-1, -1, -inf, -inf) past the rankable
        pairs.  The slots must be plain greedy ones.  Synchronises."""
        scores = [float(s) for s in scores]
        if len(scores) != rows:
            raise ValueError("beam_select needs one score per row")
        if isinstance(n_cand, bool) or not isinstance(n_cand, int) or not 1 <= n_cand <= _ext.TL_MAX_BEAM_CANDIDATES:
            raise ValueError(f"n_cand must be an int in [1, {_ext.TL_MAX_BEAM_CANDIDATES}], got {n_cand!r}")
        arr = (ctypes.c_float * max(rows, 1))(*scores)
        out = (_ext.TlBeamCandidate * n_cand)()
        _ext.check(_lib.tl_engine_beam_select(self._h, row0, rows, arr, n_cand, out))
        return [(c.parent, c.token, c.score, c.logprob) for c in out]

    def beam_reorder(self, slot0: int, n_src: int, parents: Sequence[int], tokens: Sequence[int]) -> None:
        """The beam group in slots [slot0, slot0 + n_src) becomes its next generation in place: slot ``slot0 + i`` continues the
        sequence of slot ``slot0 + parents[i]`` with pending token ``tokens[i]``, for i < len(parents) (the new width; slots between
        n_src and the width must be free, sources past the width are released).  Parents nobody chose are released; shared prefixes
        stay shared, a partial tail page is copied for every further child.  All or nothing.  Does not synchronise."""
        parents, tokens = [int(p) for p in parents], [int(t) for t in tokens]
        if len(parents) != len(tokens) or not parents:
            raise ValueError("beam_reorder needs one token per parent and at least one")
        arr_p = (ctypes.c_int * len(parents))(*parents)
        arr_t = (ctypes.c_int32 * len(tokens))(*tokens)
        _ext.check(_lib.tl_engine_beam_reorder(self._h, slot0, n_src, len(parents), arr_p, arr_t))

    # -- prefix cache (tl_engine_prefix_*; include/tinyllm_engine.h "Prefix cache") --------------------------
    def prefix_attach(self, slot: int, tokens: Sequence[int]) -> int:
        """Give the freshly begun ``slot`` the cached K / V of the longest known prefix of ``tokens`` (at most len(tokens) - 1 of them:
        the last token's row yields the logits) and return how many tokens it now holds: prefill ``tokens[matched:]``.  0 with the cache
        off.  Call it after the slot's settings (penalties, grammar, sampling) and before its first chunk."""
        tokens = [int(t) for t in tokens]
        if not tokens:
            raise ValueError("prefix_attach needs at least one token")
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        matched = ctypes.c_int(0)
        _ext.check(_lib.tl_engine_prefix_attach(self._h, slot, arr, len(tokens), ctypes.byref(matched)))
        return matched.value

    def prefix_extend(self, slot: int, tokens: Sequence[int]) -> None:
        """Declare the ids of the tokens the slot holds beyond the ones the engine knows (decode steps keep their ids on the device):
        a scheduler passes ``out[:-1]`` before ``release`` -- the last produced token was never fed -- so that a follow-up turn finds
        prompt and answer cached.  The engine cannot verify the ids.  Nothing happens for an empty list or with the cache off."""
        tokens = [int(t) for t in tokens]
        if not tokens:
            return
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        _ext.check(_lib.tl_engine_prefix_extend(self._h, slot, arr, len(tokens)))

    def set_prefix_cache(self, enabled: bool, max_retained_pages: int = 0) -> None:
        """Switch the cache on or off at any time (tl_engine_prefix_cache); off drops every entry first.  0 pages = no cap."""
        _ext.check(_lib.tl_engine_prefix_cache(self._h, int(bool(enabled)), int(max_retained_pages)))
        self.prefix_cache_enabled = bool(enabled)

    def prefix_clear(self) -> None:
        """Drop every cached entry; retained pages return to the free list."""
        _ext.check(_lib.tl_engine_prefix_clear(self._h))

    def prefix_stats(self) -> dict:
        s = _ext.TlPrefixStats()
        _ext.check(_lib.tl_engine_prefix_stats(self._h, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in s._fields_}

    # -- KV swap (tl_engine_swap_space / _park / _unpark; include/tinyllm_engine.h "KV swap") ----------------------
    def set_swap_space(self, host_pages: int) -> None:
        """Allocate (or, with 0, free) the host arena of ``host_pages`` page records; an error while a slot is parked."""
        _ext.check(_lib.tl_engine_swap_space(self._h, int(host_pages)))
        self.swap_enabled = int(host_pages) > 0

    def park(self, slot: int) -> None:
        """Move the live slot's K / V to host memory and let go of its pages (tl_engine_park); everything else of the slot -- pending
        token, sampling, penalties, grammar state, log-probability records, produced ids -- stays.  Does not synchronise."""
        _ext.check(_lib.tl_engine_park(self._h, slot))

    def unpark(self, slot: int) -> None:
        """Bring a parked slot's K / V back into fresh pages (tl_engine_unpark); an error, with the slot still parked, when the pool
        cannot give ceil(context / page_size) pages."""
        _ext.check(_lib.tl_engine_unpark(self._h, slot))

    def is_parked(self, slot: int) -> bool:
        return _lib.tl_engine_slot_parked(self._h, slot) == 1

    def step_pages(self, batch: int | None = None) -> tuple[int, int]:
        """(pages the next decode step over slots [0, batch) would take, free + evictable pages): host only."""
        need, obtainable = ctypes.c_int(), ctypes.c_int()
        _ext.check(_lib.tl_engine_step_pages(self._h, batch or self.max_batch, ctypes.byref(need), ctypes.byref(obtainable)))
        return need.value, obtainable.value

    def swap_stats(self) -> dict:
        s = _ext.TlSwapStats()
        _ext.check(_lib.tl_engine_swap_stats(self._h, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in s._fields_}

    # -- LoRA adapters (tl_engine_lora_*; include/tinyllm_engine.h "LoRA adapters") ---------------------------------
    def load_lora(self, adapter) -> int:
        """Make a ``lora.LoraAdapter`` (or an adapter directory: lora.load_adapter) resident and return its id (tl_engine_lora_load):
        the engine copies the matrices into the fused layouts of its base weights, so nothing of ``adapter`` needs to stay alive."""
        from .lora import TARGETS, LoraAdapter, check_adapter, load_adapter

        if not isinstance(adapter, LoraAdapter):
            adapter = load_adapter(adapter)
        check_adapter(adapter)
        layers = (_ext.TlLoraLayer * self.num_hidden_layers)()
        keep = []
        for (layer, target), (a, b) in adapter.weights.items():
            if layer >= self.num_hidden_layers:
                raise ValueError(f"the adapter has layer {layer}, the model {self.num_hidden_layers} layers")
            a_dev, b_dev = (t.to(self.device, torch.bfloat16).contiguous() for t in (a, b))
            keep += [a_dev, b_dev]
            t = TARGETS.index(target)
            layers[layer].a_dev[t], layers[layer].b_dev[t] = a_dev.data_ptr(), b_dev.data_ptr()
        torch.cuda.current_stream().synchronize()  # the uploads ran on torch's stream
        out = ctypes.c_int(-1)
        _ext.check(_lib.tl_engine_lora_load(self._h, layers, int(adapter.rank), float(adapter.scale), ctypes.byref(out)))
        return out.value

    def unload_lora(self, adapter: int) -> None:
        """Free a resident adapter (tl_engine_lora_unload); an error while a live or parked slot carries it."""
        _ext.check(_lib.tl_engine_lora_unload(self._h, int(adapter)))

    def set_lora(self, slot: int, adapter: int | None) -> None:
        """The live slot's adapter (tl_engine_set_lora): an id from load_lora, or None / -1 for the base model.  Only while the slot
        holds no tokens: a sequence's K / V are all computed under one adapter.  begin / release reset it, move carries it, fork copies it."""
        _ext.check(_lib.tl_engine_set_lora(self._h, slot, -1 if adapter is None else int(adapter)))

    def slot_lora(self, slot: int) -> int:
        return _lib.tl_engine_slot_lora(self._h, slot)

    def lora_stats(self) -> dict:
        s = _ext.TlLoraStats()
        _ext.check(_lib.tl_engine_lora_stats(self._h, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in s._fields_}

    def read_pending(self, count: int | None = None) -> list[int]:
        """Pending (= most recently generated) token id of slots [0, count); synchronises."""
        count = count or self.max_batch
        out = (ctypes.c_int32 * count)()
        _ext.check(_lib.tl_engine_read_pending(self._h, count, out))
        return list(out)

    def context_len(self, slot: int = 0) -> int:
        return _lib.tl_engine_context_len(self._h, slot)

    def set_token(self, slot: int, token: int) -> None:
        _ext.check(_lib.tl_engine_set_token(self._h, slot, int(token)))

    def set_lookup(self, slot: int, on: bool = True) -> None:
        """Arm (or disarm) a live slot for prompt lookup (tl_engine_set_lookup): from now on the engine keeps the slot's ordered ids
        resident on the device, so that ``lookup_propose`` can propose continuations without the host seeing an id.  Ids the slot held
        before the call are unknown and never matched: arm right after ``begin``.  Decode steps are unchanged.  begin / release switch
        it off, move carries the history along, fork copies it, park / unpark keep it."""
        _ext.check(_lib.tl_engine_set_lookup(self._h, slot, int(bool(on))))

    def lookup_state(self, slot: int) -> tuple[bool, int, int]:
        """(armed, the position the slot's history starts at, the position it is recorded up to) of tl_engine_lookup_state."""
        a, s, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _ext.check(_lib.tl_engine_lookup_state(self._h, slot, ctypes.byref(a), ctypes.byref(s), ctypes.byref(r)))
        return bool(a.value), s.value, r.value

    def lookup_propose(self, slots: Sequence[int], max_lens: Sequence[int] | None = None, max_ngram: int = 3, min_ngram: int = 1,
                       num_proposals: int = 4, sampled: bool = False) -> list[list[int]]:
        """Prompt-lookup proposals for several armed slots in one launch (tl_engine_lookup_propose): per slot the chunk
        ``verify_batch`` takes -- the pending token followed by the ids that followed the longest earlier occurrence of the slot's last
        1 .. ``max_ngram`` ids (at least ``min_ngram``), at most ``num_proposals`` and at most ``max_lens[i] - 1`` of them; the pending
        token alone where nothing matches.  ``sampled``: the chunks are meant for ``verify_batch_sampled`` (tl_engine_lookup_propose_sampled),
        which takes slots that sample and refuses slots that truncate.  Synchronises once."""
        slots = [int(s) for s in slots]
        if not 1 <= len(slots) <= 64:
            raise ValueError("lookup_propose takes between 1 and 64 slots")
        _ext.lookup_params(max_ngram, min_ngram, num_proposals)
        n = len(slots)
        lens_in = None
        if max_lens is not None:
            max_lens = [int(m) for m in max_lens]
            if len(max_lens) != n or any(not 1 <= m <= 8 for m in max_lens):
                raise ValueError("max_lens needs one value in 1 .. 8 per slot")
            if sum(max_lens) > 64:
                raise ValueError("the chunks together may hold at most 64 tokens")
            lens_in = (ctypes.c_int * n)(*max_lens)
        elif 8 * n > 64:
            raise ValueError("more than 8 slots need max_lens (the chunks together may hold at most 64 tokens)")
        tokens = (ctypes.c_int32 * 64)()
        lens = (ctypes.c_int * n)()
        propose = _lib.tl_engine_lookup_propose_sampled if sampled else _lib.tl_engine_lookup_propose
        _ext.check(propose(self._h, n, (ctypes.c_int * n)(*slots), lens_in, max_ngram, min_ngram, num_proposals, tokens, lens))
        out, at = [], 0
        for i in range(n):
            out.append(list(tokens[at:at + lens[i]]))
            at += lens[i]
        return out

    def set_sampling(self, slot: int, temperature: float = 0.0, top_k: int | None = None, top_p: float | None = None,
                     seed: int = 0) -> None:
        """Per-slot sampling on the device (tl_engine_set_sampling): every token the live slot produces from now on is drawn under
        (temperature, top_k, top_p, seed); temperature 0 is greedy.  begin / release reset the slot to greedy, move carries the
        parameters along, fork copies them (give a forked child its own seed)."""
        t, k, p, s = sampling_args(temperature, top_k, top_p, seed)
        _ext.check(_lib.tl_engine_set_sampling(self._h, slot, t, k, p, s))

    def set_logprobs(self, slot: int, top_n: int | None) -> None:
        """Per-token log-probabilities (tl_engine_set_logprobs): from the slot's next produced token on, record the model's
        temperature-1 log-probability of every token it produces and its ``top_n`` (0 .. 20) most likely alternatives; None switches
        recording off.  begin / release switch it off, move carries it along, fork copies it."""
        _ext.check(_lib.tl_engine_set_logprobs(self._h, slot, logprobs_arg(top_n)))

    def set_penalties(self, slot: int, repetition: float = 1.0, presence: float = 0.0, frequency: float = 0.0) -> None:
        """Per-slot penalties on the device (tl_engine_set_penalties): every logits row the live slot chooses a token from is first
        processed -- the repetition penalty over the tokens of its prompt and its output, presence and frequency over its output.  The
        history is tracked from the call that makes the slot process, so call this before the prompt's prefill; all-neutral values
        (1, 0, 0) forget it.  begin / release make the slot neutral, move carries everything along, fork copies it."""
        _ext.check(_lib.tl_engine_set_penalties(self._h, slot, *penalty_args(repetition, presence, frequency)))

    def set_dry(self, slot: int, multiplier: float = 0.0, base: float = 1.75, allowed_length: int = 2, range: int = 0,  # noqa: A002
                no_repeat_ngram: int = 0, breakers: Sequence[int] = ()) -> None:
        """DRY and the n-gram ban on the device (tl_engine_set_dry): repetition control that looks at the order of the slot's tokens.
        DRY (text-generation-webui's sampler) subtracts ``multiplier * base ** (L - allowed_length)`` from the token that would extend a
        verbatim repeat of L >= ``allowed_length`` tokens (matches are capped at 64, looked for in the last ``range`` tokens, 0 = all, and
        never run across a token of ``breakers``: dry_breaker_ids); ``no_repeat_ngram`` n (0 = off, else 2 .. 64) bans the token that
        would complete an n-gram the sequence already holds, as Hugging Face's no_repeat_ngram_size.  The ids are recorded from the call
        that arms the slot, so call this before the prompt's prefill; multiplier 0 with no_repeat_ngram 0 switches both off.  begin /
        release switch them off, move carries everything along, fork copies it."""
        args = dry_args(multiplier, base, allowed_length, range, no_repeat_ngram, breakers, self.vocab_size)
        ids = (ctypes.c_int32 * max(1, len(args[5])))(*args[5])
        _ext.check(_lib.tl_engine_set_dry(self._h, slot, args[0], args[1], args[2], args[3], args[4], ids, len(args[5])))

    def set_truncation(self, slot: int, min_p: float = 0.0, typical_p: float = 1.0) -> None:
        """Per-slot min-p and locally typical sampling on the device (tl_engine_set_truncation): every row a SAMPLING slot chooses a
        token from is first filtered -- min-p keeps p_i >= min_p * p_max (0 = off), typical-p the tokens whose surprise is closest to
        the entropy until their mass reaches typical_p (1 = off), ties with the boundary included -- and the sampler (with the slot's
        top-k / top-p) runs on the filtered row.  begin / release reset, move carries, fork copies.  Refused on a Mirostat slot."""
        m, y, _, _ = truncation_args(min_p, typical_p)
        _ext.check(_lib.tl_engine_set_truncation(self._h, slot, m, y))

    def set_mirostat(self, slot: int, tau: float, eta: float = 0.1) -> None:
        """Mirostat v2 on the device (tl_engine_set_mirostat): tokens whose surprise -log2 p exceeds the slot's state mu are dropped,
        and after every draw mu <- mu - eta (s - tau); mu starts at 2 tau with this call.  tau 0 switches it off.  Mirostat excludes
        top-k, top-p, min-p and typical-p on the slot (ValueError / RuntimeError for the call that would combine them)."""
        _, _, t, h = truncation_args(mirostat_tau=tau, mirostat_eta=eta)
        _ext.check(_lib.tl_engine_set_mirostat(self._h, slot, t, h))

    def mirostat_mu(self, slot: int) -> float:
        """The slot's Mirostat state mu (tl_engine_mirostat_mu; NaN without Mirostat); synchronises."""
        mu = ctypes.c_float()
        _ext.check(_lib.tl_engine_mirostat_mu(self._h, slot, ctypes.byref(mu)))
        return float(mu.value)

    def set_logit_bias(self, slot: int, bias) -> None:
        """The slot's logit bias (tl_engine_set_logit_bias): a mapping {token id: value} of at most 1,024 entries added to the logits
        before the choice (-inf bans a token, a large value forces it); None or {} clears the list.  A call replaces the whole list."""
        ids, vals = _ext.logit_bias_arg(bias, self.vocab_size)
        n = len(ids)
        _ext.check(_lib.tl_engine_set_logit_bias(self._h, slot, (ctypes.c_int32 * max(n, 1))(*ids), (ctypes.c_float * max(n, 1))(*vals), n))

    def make_vocab(self, offsets, data=None) -> "Vocab":
        """The vocabulary as byte strings on the device (tl_vocab_create): ``offsets`` [V + 1] and ``data`` (the concatenated bytes), as
        grammar.vocabulary_bytes / vocabulary_bytes_from_strings return them -- or a list of V byte strings alone.  Upload it once."""
        if data is None:
            from .grammar import vocabulary_bytes_from_strings
            offsets, data = vocabulary_bytes_from_strings(offsets)
        self._vocab = Vocab(offsets, data)
        return self._vocab

    def make_grammar(self, dfa, eos_ids, vocab: "Vocab | None" = None) -> "Grammar":
        """A byte-level automaton (grammar.compile_regex, or a StackDFA: grammar.compile_json) with the token ids that end the text (tl_grammar_create), over ``vocab``
        (default: the vocabulary of the last make_vocab)."""
        vocab = vocab if vocab is not None else getattr(self, "_vocab", None)
        if vocab is None:
            raise ValueError("make_grammar: call make_vocab first (or pass a Vocab)")
        return Grammar(vocab, dfa, eos_ids)

    def set_grammar(self, slot: int, grammar: "Grammar | None") -> None:
        """Constrain the live slot to the grammar's language (tl_engine_set_grammar), from its start state; None lifts the constraint.
        Set it before the prompt's prefill.  begin / release clear it, move carries grammar and state, fork copies them.  The Grammar
        (and its Vocab) must stay alive while a slot uses it."""
        if grammar is not None and not isinstance(grammar, Grammar):
            raise ValueError("set_grammar takes a Grammar (DecodeEngine.make_grammar) or None")
        _ext.check(_lib.tl_engine_set_grammar(self._h, slot, grammar._h if grammar is not None else None))

    def grammar_state(self, slot: int) -> tuple[int, bool]:
        """(automaton state of the slot's sequence including its pending token, or GRAMMAR_END; whether EOS is allowed next);
        synchronises."""
        state, acc = ctypes.c_int(), ctypes.c_int()
        _ext.check(_lib.tl_engine_grammar_state(self._h, slot, ctypes.byref(state), ctypes.byref(acc)))
        return state.value, bool(acc.value)

    def grammar_config(self, slot: int) -> tuple[int, int, int, bool]:
        """(state, depth, stack, whether EOS is allowed next) of the slot's sequence including its pending token
        (tl_engine_grammar_config): the configuration of a stack grammar (grammar.StackDFA; GRAMMAR_END is (-1, 0, 0)); a regex grammar
        reports its state with depth 0 and an empty stack.  Synchronises."""
        state, depth, acc, stack = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
        _ext.check(_lib.tl_engine_grammar_config(self._h, slot, ctypes.byref(state), ctypes.byref(depth), ctypes.byref(stack), ctypes.byref(acc)))
        return state.value, depth.value, stack.value, bool(acc.value)

    def make_stop_set(self, ids=(), strings=(), vocab: "Vocab | None" = None) -> "StopSet":
        """A stop set (tl_stop_create; tiny_llm_hip.stop.StopSet): token ``ids`` and byte ``strings`` (bytes, or str -> UTF-8) that end
        a sequence.  Strings are matched in the text the tokens spell, across token boundaries, so they need a vocabulary: ``vocab``,
        or the one of the last make_vocab.  A set of ids works without one; the record's text_bytes / cut_bytes then stay 0 (text is
        counted in the set's vocabulary).  Upload it once; it may arm any number of slots."""
        from .stop import StopSet
        if vocab is None:
            vocab = getattr(self, "_vocab", None)
        return StopSet(ids, strings, vocab, vocab_size=self.vocab_size)

    def set_stop(self, slot: int, stop: "StopSet | None" = None, max_new_tokens: int = 0) -> None:
        """Arm the live slot (tl_engine_set_stop): from now on every token it commits is checked on the device against the set's ids,
        its strings and the budget (0 = none), and the slot freezes at the token that stops it.  ``None`` with budget 0 disarms.  The
        call always restarts the slot's record and resumes a stopped slot.  begin / release disarm, move carries, fork copies."""
        from .stop import StopSet
        if stop is not None and not isinstance(stop, StopSet):
            raise ValueError("set_stop takes a StopSet (DecodeEngine.make_stop_set) or None")
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 0:
            raise ValueError("set_stop: max_new_tokens is a nonnegative int (0 = no budget)")
        _ext.check(_lib.tl_engine_set_stop(self._h, slot, stop._h if stop is not None else None, max_new_tokens))
        self._held_stops()[slot] = stop  # (the slot borrows the set: it stays alive while the slot is armed with it)

    def stop_state(self, slot: int) -> "StopState":
        """The slot's stop record (tl_engine_stop_state; tiny_llm_hip.stop.StopState); synchronises."""
        from .stop import REASONS, StopState
        st = _ext.TlStopState()
        _ext.check(_lib.tl_engine_stop_state(self._h, slot, ctypes.byref(st)))
        return StopState(REASONS[st.reason], st.index, st.generated, st.context, st.text_bytes, st.cut_bytes)

    def read_logprobs(self, slot: int, count: int) -> list["TokenLogprob"]:
        """Records of the slot's last ``count`` produced tokens (like read_tokens); synchronises."""
        out = (_ext.TlTokenLogprob * max(count, 1))()
        _ext.check(_lib.tl_engine_read_logprobs(self._h, slot, count, out))
        return [TokenLogprob.of(out[i]) for i in range(count)]

    def read_pending_logprobs(self, count: int | None = None) -> list["TokenLogprob"]:
        """Record of the pending token of slots [0, count) (the companion of read_pending); synchronises."""
        count = count or self.max_batch
        out = (_ext.TlTokenLogprob * count)()
        _ext.check(_lib.tl_engine_read_pending_logprobs(self._h, count, out))
        return [TokenLogprob.of(out[i]) for i in range(count)]

    # -- compute -----------------------------------------------------------------------------------
    def prefill(self, slot: int, tokens: Sequence[int], *, chunk: int | None = None, want_logits: bool = True) -> None:
        """Chunked prefill (reference Request.try_prefill, batch.py:48-76): all chunks append K/V, the last one
        also produces the first generated token."""
        tokens = [int(t) for t in tokens]
        if not tokens:
            raise ValueError("prefill needs at least one token")
        chunk = self.max_prefill_rows if chunk is None else chunk  # (the largest chunk the engine was built for: 4,096-token chunks prefill at 100k tokens/s, 2,048 at 84k)
        for start in range(0, len(tokens), chunk):
            part = tokens[start:start + chunk]
            arr = (ctypes.c_int32 * len(part))(*part)
            last = start + chunk >= len(tokens)
            _ext.check(_lib.tl_engine_prefill(self._h, slot, arr, len(part), int(last and want_logits)))

    def prefill_packed(self, chunks: Sequence[tuple[int, Sequence[int], bool]]) -> None:
        """One pass of the multi-token path over several slots' chunks: ``chunks`` = (slot, token ids, ends_prompt) for up to 16
        slots, together at most ``max_prefill_rows`` tokens (tl_engine_prefill_packed).  A chunk that ends its prompt produces
        the slot's first generated token, like the last chunk of ``prefill``."""
        if not 1 <= len(chunks) <= 16:
            raise ValueError("prefill_packed takes between 1 and 16 chunks")
        flat = [int(t) for _, toks, _ in chunks for t in toks]
        n = len(chunks)
        slots = (ctypes.c_int * n)(*[int(c[0]) for c in chunks])
        lens = (ctypes.c_int * n)(*[len(c[1]) for c in chunks])
        want = (ctypes.c_int * n)(*[int(bool(c[2])) for c in chunks])
        arr = (ctypes.c_int32 * len(flat))(*flat)
        _ext.check(_lib.tl_engine_prefill_packed(self._h, n, slots, arr, lens, want))

    def verify(self, slot: int, tokens: Sequence[int]) -> list[int]:
        """Speculative verification: append 1..8 tokens to the slot and return, for each of them, the greedy token that
        follows it (reference speculative_generate's target call with logits_to_keep = all rows).  Synchronises."""
        tokens = [int(t) for t in tokens]
        if not 1 <= len(tokens) <= 8:
            raise ValueError("verify takes between 1 and 8 tokens")
        arr = (ctypes.c_int32 * len(tokens))(*tokens)
        out = (ctypes.c_int32 * len(tokens))()
        _ext.check(_lib.tl_engine_verify(self._h, slot, arr, len(tokens), out))
        return list(out)

    def verify_batch(self, chunks: Sequence[tuple[int, Sequence[int]]], commit: bool = False) -> list[list[int]]:
        """Batched speculative verification (tl_engine_verify_batch): ``chunks`` = (slot, token ids) -- each slot's pending token and up
        to 7 proposals, together at most 64 tokens, no slot twice -- verified greedily in ONE pass.  Returns per chunk the accepted
        proposals followed by one more token (the correction, or the bonus token when every proposal was accepted).  ``commit``: the
        engine also rewinds each slot's rejected suffix and sets that last token as its pending input; otherwise the caller rewinds
        ``len(tokens) - len(result)`` tokens and sets it, as after ``verify``.  All or nothing.  Synchronises once."""
        chunks = [(int(s), [int(t) for t in toks]) for s, toks in chunks]
        if not chunks:
            raise ValueError("verify_batch needs at least one chunk")
        if any(not 1 <= len(toks) <= 8 for _, toks in chunks):
            raise ValueError("verify_batch takes between 1 and 8 tokens per slot")
        flat = [t for _, toks in chunks for t in toks]
        if len(flat) > 64:
            raise ValueError("verify_batch takes at most 64 tokens per call")
        n = len(chunks)
        slots = (ctypes.c_int * n)(*[s for s, _ in chunks])
        lens = (ctypes.c_int * n)(*[len(toks) for _, toks in chunks])
        arr = (ctypes.c_int32 * len(flat))(*flat)
        out = (_ext.TlVerifyResult * n)()
        _ext.check(_lib.tl_engine_verify_batch(self._h, n, slots, arr, lens, int(bool(commit)), out))
        return [list(r.ids[:r.count]) for r in out]

    def verify_batch_sampled(self, chunks: Sequence[tuple[int, Sequence[int]]], commit: bool = False, draft_rows: torch.Tensor | None = None,
                             draft_sampling=(0.0, None, None)) -> list[list[int]]:
        """Batched speculative sampling (tl_engine_verify_batch_sampled): ``verify_batch`` for slots that sample -- every proposal is
        verified under its slot's own sampling parameters (set_sampling), so the ids returned are distributed exactly as if the slot had
        sampled them alone; a greedy slot in the same call gets ``verify_batch``'s result.  ``draft_rows`` None: point proposals, a
        deterministic function of the sequence such as ``lookup_propose``'s (one-hot at the proposed id; only the target rows are read).
        ``draft_rows`` [sum of chunk lengths, vocab] bf16 on the device: row r is the logits row the draft drew token r + 1 of the
        flattened chunks from under ``draft_sampling`` = (temperature, top_k, top_p) (or a dict with those keys); the row at a chunk's
        last position is never read.  ``commit`` as in ``verify_batch``.  All or nothing.  Synchronises once."""
        chunks = [(int(s), [int(t) for t in toks]) for s, toks in chunks]
        if not chunks:
            raise ValueError("verify_batch_sampled needs at least one chunk")
        if any(not 1 <= len(toks) <= 8 for _, toks in chunks):
            raise ValueError("verify_batch_sampled takes between 1 and 8 tokens per slot")
        flat = [t for _, toks in chunks for t in toks]
        if len(flat) > 64:
            raise ValueError("verify_batch_sampled takes at most 64 tokens per call")
        if isinstance(draft_sampling, dict):
            draft_sampling = (draft_sampling.get("temperature", 0.0), draft_sampling.get("top_k"), draft_sampling.get("top_p"))
        t, k, p, _ = sampling_args(*draft_sampling)
        ptr = None
        if draft_rows is not None:
            if not isinstance(draft_rows, torch.Tensor) or draft_rows.dtype != torch.bfloat16 or draft_rows.dim() != 2 or not draft_rows.is_cuda \
                    or not draft_rows.is_contiguous() or draft_rows.shape[0] != len(flat) or draft_rows.shape[1] != self.vocab_size:
                raise ValueError(f"draft_rows must be a contiguous bf16 tensor [{len(flat)}, {self.vocab_size}] on the GPU")
            ptr = draft_rows.data_ptr()
        n = len(chunks)
        slots = (ctypes.c_int * n)(*[s for s, _ in chunks])
        lens = (ctypes.c_int * n)(*[len(toks) for _, toks in chunks])
        arr = (ctypes.c_int32 * len(flat))(*flat)
        out = (_ext.TlVerifyResult * n)()
        _ext.check(_lib.tl_engine_verify_batch_sampled(self._h, n, slots, arr, lens, ptr, t, k, p, int(bool(commit)), out))
        return [list(r.ids[:r.count]) for r in out]

    def verify_logits(self, rows: int, row0: int = 0) -> torch.Tensor:
        """A copy of rows [row0, row0 + rows) of the last batched verification's own logits block [rows, vocab] (bf16)
        (tl_engine_copy_verify_logits): the rows the acceptance stage of ``verify_batch`` / ``verify_batch_sampled`` read."""
        out = torch.empty((rows, self.vocab_size), dtype=torch.bfloat16, device=self.device)
        torch.cuda.current_stream().synchronize()
        _ext.check(_lib.tl_engine_copy_verify_logits(self._h, int(row0), int(rows), out.data_ptr()))
        self.synchronize()
        return out

    def verify_sampled(self, slot: int, tokens: Sequence[int], draft_rows: torch.Tensor | None, draft_sampling=(0.0, None, None)) -> list[int]:
        """Speculative sampling (tl_engine_verify_sampled): append 1..8 tokens to the slot -- its pending token and the draft's
        proposals -- and verify the proposals under the slot's own sampling parameters (set_sampling).  ``draft_rows`` [>= n-1, vocab]
        bf16 on the device: row i is the logits row the draft drew ``tokens[i+1]`` from under ``draft_sampling`` = (temperature, top_k,
        top_p) (or a dict with those keys); None with a single token.  Returns the accepted proposals followed by one more token -- the
        residual draw where a proposal was rejected, the slot's ordinary draw after the last row where none was -- distributed exactly
        as if the slot had sampled them alone.  The caller rewinds ``len(tokens) - len(result)`` tokens and sets the next input, as
        after ``verify``.  The rows must be complete before the call (they are read on this engine's stream).  Synchronises."""
        tokens = [int(t) for t in tokens]
        if not 1 <= len(tokens) <= 8:
            raise ValueError("verify_sampled takes between 1 and 8 tokens")
        if isinstance(draft_sampling, dict):
            draft_sampling = (draft_sampling.get("temperature", 0.0), draft_sampling.get("top_k"), draft_sampling.get("top_p"))
        t, k, p, _ = sampling_args(*draft_sampling)
        n = len(tokens)
        ptr = None
        if n > 1:
            if draft_rows is None or draft_rows.dtype != torch.bfloat16 or draft_rows.dim() != 2 or not draft_rows.is_cuda \
                    or not draft_rows.is_contiguous() or draft_rows.shape[0] < n - 1 or draft_rows.shape[1] != self.vocab_size:
                raise ValueError(f"draft_rows must be a contiguous bf16 tensor [>= {n - 1}, {self.vocab_size}] on the GPU")
            ptr = draft_rows.data_ptr()
        arr = (ctypes.c_int32 * n)(*tokens)
        out = (ctypes.c_int32 * n)()
        count = ctypes.c_int(0)
        _ext.check(_lib.tl_engine_verify_sampled(self._h, slot, arr, n, ptr, t, k, p, out, ctypes.byref(count)))
        return list(out[:count.value])

    def score(self, tokens: Sequence[int], *, slot: int = 0, chunk: int | None = None) -> list[float]:
        """Log-probabilities of ``tokens[1:]``, each given the tokens before it (tl_engine_score), on the free ``slot`` as a fresh
        sequence, in chunks of at most ``chunk`` (default: max_prefill_rows) tokens; each chunk's last row scores the next chunk's
        first token.  The slot is released afterwards.  Synchronises."""
        tokens = [int(t) for t in tokens]
        if not tokens:
            raise ValueError("score needs at least one token")
        chunk = self.max_prefill_rows if chunk is None else chunk
        if isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= self.max_prefill_rows:
            raise ValueError(f"chunk must be an int in [1, {self.max_prefill_rows}], got {chunk!r}")
        out: list[float] = []
        self.begin(slot)
        try:
            for start in range(0, len(tokens), chunk):
                part = tokens[start:start + chunk]
                nxt = tokens[start + chunk] if start + chunk < len(tokens) else -1
                arr = (ctypes.c_int32 * len(part))(*part)
                lp = (ctypes.c_float * len(part))()
                _ext.check(_lib.tl_engine_score(self._h, slot, arr, len(part), nxt, lp, None))
                out.extend(lp)
        finally:
            self.release(slot)
        return out[:-1]

    def embed(self, tokens: Sequence[int], *, slot: int = 0, pooling: str = "last", normalize: bool = True, dim: int | None = None,
              chunk: int | None = None):
        """The text's embedding (tl_engine_embed), float32 [dim] as a numpy array: the model's output rows -- final RMSNorm included --
        pooled by ``pooling`` ("last": the last token's row, what Qwen3-Embedding models use; "mean": the mean over all tokens), cut to
        the first ``dim`` components (default: hidden_size) and, with ``normalize``, divided by their Euclidean norm.  Runs on the free
        ``slot`` as a fresh sequence in chunks of at most ``chunk`` (default: max_prefill_rows) tokens and releases it.  Synchronises."""
        import numpy as np

        tokens = [int(t) for t in tokens]
        if not tokens:
            raise ValueError("embed needs at least one token")
        mode, norm, dim = _ext.pooling_args(pooling, normalize, dim, int(self.args.hidden_size))
        chunk = self.max_prefill_rows if chunk is None else chunk
        if isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= self.max_prefill_rows:
            raise ValueError(f"chunk must be an int in [1, {self.max_prefill_rows}], got {chunk!r}")
        out = np.empty(dim, dtype=np.float32)
        out_p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        self.begin(slot)
        try:
            for start in range(0, len(tokens), chunk):
                part = tokens[start:start + chunk]
                arr = (ctypes.c_int32 * len(part))(*part)
                last = start + chunk >= len(tokens)
                _ext.check(_lib.tl_engine_embed(self._h, slot, arr, len(part), int(last), mode, norm, dim, out_p))
        finally:
            self.release(slot)
        return out

    def embed_packed(self, chunks: Sequence[tuple[int, Sequence[int], bool]], *, pooling: str = "last", normalize: bool = True,
                     dim: int | None = None):
        """One pass of the multi-token path over several slots' chunks, pooled (tl_engine_embed_packed): ``chunks`` = (slot, token ids,
        ends_text) for up to 16 live slots, together at most ``max_prefill_rows`` tokens.  Returns float32 [chunks that end their
        text, dim] in the order of ``chunks``; synchronises only when some chunk ends its text.  The slots stay live: the caller
        begins and releases them."""
        import numpy as np

        if not 1 <= len(chunks) <= 16:
            raise ValueError("embed_packed takes between 1 and 16 chunks")
        mode, norm, dim = _ext.pooling_args(pooling, normalize, dim, int(self.args.hidden_size))
        flat = [int(t) for _, toks, _ in chunks for t in toks]
        n = len(chunks)
        slots = (ctypes.c_int * n)(*[int(c[0]) for c in chunks])
        lens = (ctypes.c_int * n)(*[len(c[1]) for c in chunks])
        finish = (ctypes.c_int * n)(*[int(bool(c[2])) for c in chunks])
        arr = (ctypes.c_int32 * max(len(flat), 1))(*flat)
        out = np.empty((sum(finish), dim), dtype=np.float32)
        _ext.check(_lib.tl_engine_embed_packed(self._h, n, slots, arr, lens, finish, mode, norm, dim,
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def decode(self, steps: int, batch: int | None = None, use_graph: bool = True) -> None:
        """Enqueue ``steps`` decode steps over slots [0, batch) (greedy, or each slot's sampler: set_sampling); does not synchronise
        on the hipGraph route."""
        _ext.check(_lib.tl_engine_decode(self._h, batch or self.max_batch, int(steps), int(use_graph)))

    def read_tokens(self, slot: int, count: int) -> list[int]:
        out = (ctypes.c_int32 * count)()
        _ext.check(_lib.tl_engine_read_tokens(self._h, slot, count, out))
        return list(out)

    def logits(self, rows: int = 1) -> torch.Tensor:
        """A copy of the most recent logits [rows, vocab] (bf16)."""
        out = torch.empty((rows, self.vocab_size), dtype=torch.bfloat16, device=self.device)
        torch.cuda.current_stream().synchronize()  # `out` is allocated on torch's stream
        _ext.check(_lib.tl_engine_copy_logits(self._h, out.data_ptr(), rows))
        self.synchronize()
        return out

    def logits_buffer(self, rows: int) -> torch.Tensor:
        """An uninitialised [rows, vocab] bf16 tensor on the engine's device for ``copy_logits_into``, safe to write on the engine
        stream (torch's stream, which allocated it, has finished with the memory)."""
        out = torch.empty((rows, self.vocab_size), dtype=torch.bfloat16, device=self.device)
        torch.cuda.current_stream().synchronize()
        return out

    def copy_logits_into(self, dst: torch.Tensor, rows: int = 1) -> None:
        """Enqueue a copy of the most recent logits rows into ``dst`` (contiguous bf16 on the device, at least rows * vocab elements)
        on the engine stream (tl_engine_copy_logits); does not synchronise.  ``dst`` must not be in use on another stream."""
        if dst.dtype != torch.bfloat16 or not dst.is_cuda or not dst.is_contiguous() or dst.numel() < rows * self.vocab_size:
            raise ValueError(f"copy_logits_into needs a contiguous bf16 tensor of at least {rows} x {self.vocab_size} elements on the GPU")
        _ext.check(_lib.tl_engine_copy_logits(self._h, dst.data_ptr(), rows))

    def processed_logits(self, rows: int = 1) -> torch.Tensor:
        """A copy of the processed rows [rows, vocab] (bf16) of the last decode step in which some slot processed its logits
        (tl_engine_copy_processed_logits): row i is what slot i's token was chosen from; the row of a slot that does not process is its
        raw row."""
        out = torch.empty((rows, self.vocab_size), dtype=torch.bfloat16, device=self.device)
        torch.cuda.current_stream().synchronize()
        _ext.check(_lib.tl_engine_copy_processed_logits(self._h, out.data_ptr(), rows))
        self.synchronize()
        return out

    def filtered_logits(self, rows: int = 1) -> torch.Tensor:
        """A copy of the filtered rows [rows, vocab] (bf16) of the last decode step in which some slot truncated
        (tl_engine_copy_filtered_logits): row i is what slot i's token was drawn from -- kept tokens with their bits, the others -inf;
        the row of a slot that does not truncate is its processed or raw row."""
        out = torch.empty((rows, self.vocab_size), dtype=torch.bfloat16, device=self.device)
        torch.cuda.current_stream().synchronize()
        _ext.check(_lib.tl_engine_copy_filtered_logits(self._h, out.data_ptr(), rows))
        self.synchronize()
        return out

    def synchronize(self) -> None:
        _ext.check(_lib.tl_engine_synchronize(self._h))

    def step_bytes(self, batch: int | None = None) -> int:
        return int(_lib.tl_engine_step_bytes(self._h, batch or self.max_batch))

    PROFILE_KINDS = ("gemv_qkv", "gemv_o", "gemv_gate_up", "gemv_down", "gemv_lm_head", "attention",
                     "attention_merge", "step_end")

    def profile_step(self, batch: int | None = None) -> dict:
        """One real decode step with in-kernel clock stamps (tl_engine_profile_step): per-kind kernel time."""
        p = _ext.TlStepProfile()
        _ext.check(_lib.tl_engine_profile_step(self._h, batch or self.max_batch, ctypes.byref(p)))
        out = {"span_us": p.span_us, "clock_khz": p.clock_khz, "n_splits": p.n_splits, "kinds": {}}
        for i, name in enumerate(self.PROFILE_KINDS):
            out["kinds"][name] = {"us": p.kernel_us[i], "launches": p.launches[i],
                                  "bytes": p.gemv_bytes[i] if i < 5 else 0.0}
        return out

    def check_step(self, batch: int | None = None) -> dict:
        """One real decode step with the written-once checker behind every launch (tl_engine_check_step; test aid of the AQL route)."""
        c = _ext.TlStepCheck()
        _ext.check(_lib.tl_engine_check_step(self._h, batch or self.max_batch, ctypes.byref(c)))
        return {name: getattr(c, name) for name, _ in c._fields_}

    def replay_route(self) -> str:
        """"aql" (captured steps replay as AQL packets on the engine's own HSA queue) or "hipgraph: <why>" (include/tinyllm_engine.h)."""
        return (_lib.tl_engine_replay_route(self._h) or b"").decode()

    def stats(self) -> dict:
        s = _ext.TlEngineStats()
        _ext.check(_lib.tl_engine_get_stats(self._h, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in s._fields_}

    # -- convenience: one request, like benches/bench.py:run_one_request_week2 --------------------------
    def generate(self, prompt: Sequence[int], max_new_tokens: int, *, slot: int = 0, chunk: int | None = None, logprobs: int | None = None,
                 stop: "StopSet | None" = None, decode_block: int = 32, **settings):
        """One request: prefill, then ``max_new_tokens - 1`` decode steps in one call.  ``settings``: what the request sets on its slot, as
        keywords -- the keys of tiny_llm_hip.request.SETTINGS with their defaults there (a plain greedy request), validated by
        request_settings (ValueError, also for an unknown key) and set before the prefill (RequestSettings.apply), so the prompt's
        tokens are in the history that penalties, DRY and the n-gram ban look at.  With a ``grammar`` the ids are text of its language,
        followed by EOS ids once it has ended.  On an engine with the prefix cache on, the slot first attaches the cached prefix of the
        prompt (prefix_attach), prefills the rest and declares the answer before its release (prefix_extend); a ``lora`` request bypasses it.
        With ``logprobs`` an int (0 .. 20 alternatives, set_logprobs): returns (ids, records).  ``stop``: a StopSet (make_stop_set).  The
        slot is armed with it and the budget ``max_new_tokens`` before the prefill, decodes in blocks of ``decode_block`` steps and leaves
        after the block in which it stopped; the result is the ids up to and including the stopping token -- exactly
        ``stop_state().generated`` of them -- and likewise the records; ``last_stop_state`` keeps the slot's final StopState."""
        if stop is not None and (isinstance(decode_block, bool) or not isinstance(decode_block, int) or decode_block < 1):
            raise ValueError("generate: decode_block is a positive int")
        settings = request_settings(settings, 1, vocab_size=self.vocab_size, logprobs=logprobs, stop=stop, limits=[max_new_tokens])[0]
        self.begin(slot)
        try:
            settings.apply(self, slot)
            prompt = [int(t) for t in prompt]
            matched = self.prefix_attach(slot, prompt) if self.prefix_cache_enabled and prompt else 0
            self.prefill(slot, prompt[matched:], chunk=chunk)
            count = max_new_tokens
            if stop is not None:
                left = max_new_tokens - 1
                state = self.stop_state(slot)
                while not state.stopped and left > 0:
                    steps = min(decode_block, left)
                    self.decode(steps, batch=slot + 1)
                    left -= steps
                    state = self.stop_state(slot)
                count = state.generated
                self.last_stop_state = state  # (why and where the request ended: the slot is released below)
            elif max_new_tokens > 1:
                self.decode(max_new_tokens - 1, batch=slot + 1)
            ids = self.read_tokens(slot, count)
            # only fed tokens are declared (the last one never was), so that a follow-up turn finds prompt and answer cached
            if self.prefix_cache_enabled:
                self.prefix_extend(slot, ids[:-1])
            return (ids, self.read_logprobs(slot, count)) if settings.top_n >= 0 else ids
        finally:
            self.release(slot)


class TokenLogprob(NamedTuple):
    """One produced token's record: its log-probability under the model (temperature 1, unfiltered) and the top-N alternatives as
    (id, log-probability) pairs, most likely first."""
    logprob: float
    top: list

    @staticmethod
    def of(rec: "_ext.TlTokenLogprob") -> "TokenLogprob":
        return TokenLogprob(float(rec.logprob), [(int(i), float(v)) for i, v in zip(rec.top_ids, rec.top_logprobs) if i >= 0])


GRAMMAR_END = -1  # TL_GRAMMAR_END


class Vocab:
    """tl_vocab: token id -> byte string, on the device.  ``offsets`` int32 [V + 1], ``data`` the bytes."""

    def __init__(self, offsets, data):
        import numpy as np

        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        data = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8)
        if offsets.ndim != 1 or offsets.size < 2 or data.ndim != 1 or int(offsets[-1]) != data.size:
            raise ValueError("Vocab: offsets [V + 1] must end at len(data)")
        self.size = offsets.size - 1
        handle = ctypes.c_void_p()
        _ext.check(_lib.tl_vocab_create(self.size, offsets.ctypes.data, data.ctypes.data if data.size else None, None, ctypes.byref(handle)))
        self._h = handle

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.tl_vocab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Grammar:
    """tl_grammar: a ByteDFA (table uint16 [S, 256], accepting, start) or a StackDFA (with ops and pop_table: tl_grammar_create_stack)
    over a Vocab, with its EOS ids."""

    def __init__(self, vocab: Vocab, dfa, eos_ids):
        import numpy as np

        table = np.ascontiguousarray(dfa.table, dtype=np.uint16)
        accepting = np.ascontiguousarray(dfa.accepting, dtype=np.uint8)
        if table.ndim != 2 or table.shape[1] != 256 or accepting.shape != (table.shape[0],):
            raise ValueError("Grammar: table must be [S, 256] and accepting [S]")
        eos = [int(t) for t in eos_ids]
        arr = (ctypes.c_int32 * max(len(eos), 1))(*eos)
        handle = ctypes.c_void_p()
        if hasattr(dfa, "pop_table"):
            ops = np.ascontiguousarray(dfa.ops, dtype=np.uint8)
            pops = np.ascontiguousarray(dfa.pop_table, dtype=np.uint16).reshape(-1, 5)
            if ops.shape != table.shape:
                raise ValueError("Grammar: ops must have the table's shape")
            _ext.check(_lib.tl_grammar_create_stack(vocab._h, table.shape[0], table.ctypes.data, ops.ctypes.data, pops.shape[0],
                                                    pops.ctypes.data if pops.size else None, accepting.ctypes.data, int(dfa.start), arr, len(eos),
                                                    None, ctypes.byref(handle)))
        else:
            _ext.check(_lib.tl_grammar_create(vocab._h, table.shape[0], table.ctypes.data, accepting.ctypes.data, int(dfa.start), arr, len(eos),
                                              None, ctypes.byref(handle)))
        self._h = handle
        self.vocab, self.dfa, self.eos_ids = vocab, dfa, tuple(eos)  # (the vocabulary must outlive the grammar)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.tl_grammar_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def batch_generate_ids(engine: DecodeEngine, prompts: Sequence[Sequence[int]], max_new_tokens: int | Sequence[int],
                       batch_size: int, prefill_step: int = 128, eos_token_id: int | None = None,
                       on_step=None, sampling=None, base_seed: int = 0, logprobs: int | None = None, stop=None,
                       decode_block: int = 1) -> list[tuple]:
    """Continuous batching over engine slots with the reference scheduler's shape (batch_generate,
    src/tiny_llm_ref/batch.py:136-285; benches/bench.py:run_batch_requests_serving 351-572): every loop turn
    (a) admits one pending request and prefills ONE chunk of at most ``prefill_step`` tokens in the staging slot,
    (b) adopts it into the lowest free decode slot once its prefill is complete, (c) runs one batched decode step over
    the occupied prefix of the slots (the reference steps all ``batch_size`` rows; idle rows carry context 0 and produce
    nothing, so skipping the idle tail changes no result), (d) retires finished requests and returns their pages.
    Token-id in, token-id out (no tokenizer can be downloaded here).  Needs ``engine.max_batch >= batch_size + 1``:
    the last slot is the prefill staging slot.  Returns [(prompt_idx, generated ids)] in completion order.
    ``sampling``: None (greedy), one dict or one dict per prompt (request_settings: the keys of tiny_llm_hip.request.SETTINGS; a ``grammar``'s
    EOS ids then end the request like ``eos_token_id``); applied when a request enters the staging slot (RequestSettings.apply),
    and carried by the engine through its slot moves.  ``logprobs``: None, or an int (0 .. 20 alternatives): every request records
    its tokens' log-probabilities (set_logprobs), read in the same turn as the pending ids, and the result is
    [(prompt_idx, generated ids, records)].
    An engine built with ``prefix_cache`` has every request attach the cached prefix of its prompt (prefix_attach: after its settings,
    before its first chunk, which then starts at the matched offset) and declare its fed answer tokens at retirement (prefix_extend
    before release), so a follow-up turn finds prompt and answer cached.  Results keep their order and content rules.
    ``sampling["lora"]``: the id of a resident adapter (DecodeEngine.load_lora) -- one for every request, a list with one per request,
    or per dict -- set when the request enters the staging slot and carried by the engine through its slot moves; None / -1 = the base
    model.  Requests under different adapters share decode steps; a request with an adapter bypasses the prefix cache.
    An engine built with ``swap_pages`` preempts under page pressure instead of failing with "KV page pool exhausted"
    (tiny_llm_hip.preempt): before a decode step the staging request is released and re-queued, or the running request admitted last
    is parked; parked requests resume oldest first, and nothing new is admitted while one is parked.  A request's ids do not depend on
    being preempted beyond the usual row-bucket band (a step's arithmetic follows its row count) -- except that a Mirostat request
    which is recomputed instead of unparked (the staging request that gives way) restarts its mu at 2 tau.
    ``stop``: one StopSet (DecodeEngine.make_stop_set) for every request, or a sequence with one (or None) per request.  Each request
    is then armed on the device with its set and its ``max_new_tokens`` budget when it enters the staging slot (set_stop), and retires
    on its stop state (stop_state) instead of the host's comparison: its ids end with the stopping token.  ``eos_token_id`` is not
    combined with it (put the id into the set), and a grammar's EOS ids end such a request only where the set holds them.
    ``decode_block`` > 1 (with ``stop``): while the queue is empty, nothing is staged and the engine has no swap space, a turn runs
    that many decode steps in one call -- a slot that stops inside the block freezes at its stopping token -- and reads each slot's
    ids of the block from the ring by its ``generated`` count.  Calls that pass neither argument behave exactly as before.
    The turn itself is tiny_llm_hip.scheduler.Scheduler's, shared with benches/serving.py; what is this front-end's own is _BatchFrontend."""
    if isinstance(decode_block, bool) or not isinstance(decode_block, int) or decode_block < 1:
        raise ValueError("decode_block is a positive int")
    if stop is None and decode_block != 1:
        raise ValueError("decode_block > 1 needs stop conditions on the device (stop=)")
    if stop is not None and eos_token_id is not None:
        raise ValueError("stop= and eos_token_id= are not combined: put the id into the stop set")
    if batch_size <= 0 or prefill_step <= 0:
        raise ValueError("batch_size and prefill_step must be positive")
    if engine.max_batch < batch_size + 1:
        raise ValueError("engine needs batch_size + 1 slots (one prefill staging slot)")
    settings = request_settings(sampling, len(prompts), base_seed, engine.vocab_size if sampling is not None else 0, logprobs, stop, max_new_tokens)
    fe = _BatchFrontend(engine, prompts, settings, eos_token_id, on_step, decode_block)
    sched = scheduler.Scheduler(engine, fe, range(len(prompts)), batch_size=batch_size, prefill_step=prefill_step)
    sched.run()
    return [(s["req"], s["out"]) + ((s["lp"],) if fe.top_n >= 0 else ()) for s in sched.finished]


class _BatchFrontend(scheduler.Frontend):
    """batch_generate_ids' side of the scheduler: requests are prompt indices; every produced id is read back, and a request is
    finished by the host's comparison (limit, ``eos_token_id``, its grammar's EOS ids) or, armed, by the device's stop state."""
    rows_cover_parked = True

    def __init__(self, engine, prompts, settings, eos_token_id, on_step, decode_block):
        self.engine, self.prompts, self.settings, self.eos_token_id, self.on_step = engine, prompts, settings, eos_token_id, on_step
        self.decode_block = decode_block
        self.top_n = settings[0].top_n if settings else -1
        self.armed = bool(settings) and settings[0].armed

    def admit(self, slot, state):
        s = self.settings[state["req"]]
        s.apply(self.engine, slot)
        state.update(tokens=[int(t) for t in self.prompts[state["req"]]], lp=[], limit=s.budget,
                     eos=s.grammar.eos_ids if s.grammar is not None else None)

    def prefilled(self, chunks):
        for state, _, last in chunks:
            if last:
                state["out"].append(self.engine.read_tokens(state["staging"], 1)[0])
                if self.top_n >= 0:
                    state["lp"].append(self.engine.read_logprobs(state["staging"], 1)[0])

    def _ended(self, state):  # the host's comparison; the request's own EOS ids where it has a grammar
        token = state["out"][-1]
        return len(state["out"]) >= state["limit"] or token == self.eos_token_id or (state["eos"] is not None and token in state["eos"])

    def finished_in_staging(self, slot, state):
        return self.engine.stop_state(slot).stopped if self.armed else self._ended(state)

    def stepped(self, rows, active, steps):
        if not self.armed:
            self.tokens = self.engine.read_pending(rows)
            self.records = self.engine.read_pending_logprobs(rows) if self.top_n >= 0 else None
        if self.on_step is not None:
            for _ in range(steps):
                self.on_step(len(active))

    def collect(self, slot, state):
        if self.armed:  # the device decided: the slot's new ids from its ring, as many as its record counted
            stop = self.engine.stop_state(slot)
            new = stop.generated - len(state["out"])
            state["out"].extend(self.engine.read_tokens(slot, new))
            if self.top_n >= 0:
                state["lp"].extend(self.engine.read_logprobs(slot, new))
            return stop.stopped
        state["out"].append(self.tokens[slot])
        if self.records is not None:
            state["lp"].append(self.records[slot])
        return self._ended(state)


def speculative_generate_ids(target: DecodeEngine, draft: DecodeEngine, prompt: Sequence[int], max_new_tokens: int,
                             proposal_length: int = 4, eos_token_id: int | None = None, *, slot: int = 0,
                             chunk: int = 2048, stats: dict | None = None, temperature: float = 0.0, top_k: int | None = None,
                             top_p: float | None = None, seed: int = 0) -> list[int]:
    """Speculative decoding over two engines (reference speculative_generate, src/tiny_llm_ref/generate.py:84-322;
    token ids in, token ids out).  The draft engine free-runs ``proposal_length`` fused decode steps on the device; the
    target scores the pending token plus the proposals in one ``verify`` call (at most 8 rows through the paged decode
    kernel) and both KV caches are rewound to the accepted prefix.  Returns exactly the target's greedy continuation
    (up to ``max_new_tokens`` ids, stopping before ``eos_token_id``); ``stats`` receives call and acceptance counts.

    ``temperature`` > 0: speculative sampling (Leviathan et al. 2023).  Both engines sample on the device under (temperature, top_k,
    top_p) -- the target from ``seed``, the draft from a seed derived from it; the draft runs one step per ``decode`` call, each
    followed by a stream-ordered copy of its logits row, and the target accepts or redraws in one ``verify_sampled`` call.  The ids
    are distributed exactly as if the target had sampled alone, and the same arguments give the same ids.  ``stats["resampled"]``
    counts the rounds that ended in a residual draw."""
    sampled = sampling_args(temperature, top_k, top_p, seed)
    sampling = sampled[0] > 0
    if sampling and proposal_length and draft.vocab_size != target.vocab_size:
        raise ValueError("speculative sampling needs one vocabulary: the draft's rows are compared with the target's")
    if sampling and slot != 0:
        raise ValueError("speculative sampling runs on slot 0 (the draft's logits row is copied from the front of its rows)")
    if not isinstance(proposal_length, int) or isinstance(proposal_length, bool) or proposal_length < 0:
        raise ValueError("proposal_length must be a non-negative integer")
    if proposal_length > 7:
        raise ValueError("proposal_length must be at most 7 (8 verification rows)")
    prompt = [int(t) for t in prompt]
    if not prompt:
        raise ValueError("prompt must hold at least one token")
    counts = {"target_calls": 0, "draft_steps": 0, "proposed": 0, "accepted": 0, "resampled": 0}
    out: list[int] = []
    target.begin(slot)
    draft_live = False
    draft_rows = None
    try:
        if sampling:
            target.set_sampling(slot, temperature, top_k, top_p, seed)
        target.prefill(slot, prompt, chunk=chunk)
        token = target.read_tokens(slot, 1)[0]
        counts["target_calls"] += 1
        if proposal_length > 0:
            draft.begin(slot)
            draft_live = True
            if sampling:  # the draft's own stream of draws; its rows go to the target through this buffer
                draft.set_sampling(slot, temperature, top_k, top_p, seed ^ 0x9E3779B97F4A7C15)
                draft_rows = draft.logits_buffer(7)
            draft.prefill(slot, prompt, chunk=chunk, want_logits=False)
        while len(out) < max_new_tokens and token != eos_token_id:
            room = max_new_tokens - len(out) - 1          # proposals that could still be emitted after `token`
            k = min(proposal_length, room)
            proposals: list[int] = []
            if k > 0:
                draft.set_token(slot, token)
                if sampling:  # one step per call: a multi-step call would overwrite the rows the proposals were drawn from
                    for i in range(k):
                        draft.decode(1, batch=slot + 1)
                        draft.copy_logits_into(draft_rows[i], 1)
                else:
                    draft.decode(k, batch=slot + 1)
                proposals = draft.read_tokens(slot, k)             # (synchronises the draft's stream: the copied rows are complete)
                counts["draft_steps"] += k
                if eos_token_id in proposals:              # the draft stops proposing after its own EOS
                    keep = proposals.index(eos_token_id) + 1
                    draft.rewind(slot, k - keep)
                    proposals = proposals[:keep]
            fed = [token] + proposals
            if sampling:
                emitted = target.verify_sampled(slot, fed, draft_rows, (temperature, top_k, top_p))
                counts["target_calls"] += 1
                counts["proposed"] += len(proposals)
                a = len(emitted) - 1                       # proposals accepted; emitted[a] follows fed[0..a]
                stop = next((i for i in range(1, a + 1) if fed[i] == eos_token_id), None)
                if stop is None and a == len(proposals):   # everything accepted: the last row's own draw is a bonus token
                    out.extend(fed)
                    counts["accepted"] += len(proposals)
                    if proposals:
                        draft.decode(1, batch=slot + 1)
                        counts["draft_steps"] += 1
                    token = emitted[a]
                    continue
                cut = a + 1 if stop is None else stop      # fed[:cut] is emitted, fed[cut:] leaves both caches
                out.extend(fed[:cut])
                counts["accepted"] += cut - 1
                counts["resampled"] += int(stop is None)
                target.rewind(slot, len(fed) - cut)
                if proposals:
                    draft.rewind(slot, len(proposals) - cut)
                token = emitted[a] if stop is None else eos_token_id
                continue
            predicted = target.verify(slot, fed)
            counts["target_calls"] += 1
            counts["proposed"] += len(proposals)
            own = [token] + predicted[:-1]                 # what the target alone would have fed at each row
            cut = next((i for i, (mine, given) in enumerate(zip(own, fed))
                        if mine != given or mine == eos_token_id), None)
            if cut is None:                                # everything accepted: the last prediction is a bonus token
                out.extend(own)
                counts["accepted"] += len(proposals)
                if proposals:                              # the draft has not consumed its last proposal yet
                    draft.decode(1, batch=slot + 1)
                    counts["draft_steps"] += 1
                token = predicted[-1]
                continue
            out.extend(own[:cut])
            counts["accepted"] += cut - 1
            target.rewind(slot, len(fed) - cut)
            if proposals:
                draft.rewind(slot, len(proposals) - cut)
            token = own[cut]
        if stats is not None:
            stats.update(counts)
        return out[:max_new_tokens]
    finally:
        target.release(slot)
        if draft_live:
            draft.release(slot)


def batch_speculative_generate_ids(target, draft, prompts: Sequence[Sequence[int]], max_new_tokens: int | Sequence[int], proposal_length: int = 4,
                                   eos_token_id: int | None = None, *, stats: dict | None = None) -> list[list[int]]:
    """Greedy speculative decoding for several prompts at once: ``speculative_generate_ids``' loop with every target call of a round
    folded into ONE ``verify_batch(..., commit=True)``.  Prompts run in waves of at most ``min(target.max_batch, draft.max_batch,
    64 // (proposal_length + 1))`` slots, prompt i of a wave on slot i of both engines.  Per round: the live slots' pending tokens go to
    the draft, one ``draft.decode(k, batch)`` proposes for all of them (k = the most any of them may still emit; a slot with less
    room, or whose draft proposed its own EOS, keeps fewer and its draft is rewound), one ``verify_batch`` accepts, and each slot's
    draft is rewound to the accepted prefix -- or, where everything was accepted, takes the one step that consumes its last proposal
    (one batched step for all slots, rewound again on the others).  A sequence that finishes is released and drops out of later rounds;
    the last id it may emit is its pending token, which costs no pass, so every round of a sequence yields at least one id and
    ``rounds`` stays below the ids emitted.
    Returns, per prompt, exactly the target's greedy continuation (up to ``max_new_tokens`` ids -- one number, or one per prompt as
    ``batch_generate_ids`` takes them -- stopping before ``eos_token_id``).
    ``stats`` receives the single-slot loop's counters, summed over the prompts, and ``rounds`` (verify_batch calls);
    ``target_calls`` counts one call per prefill and one per round."""
    if not isinstance(proposal_length, int) or isinstance(proposal_length, bool) or not 0 <= proposal_length <= 7:
        raise ValueError("proposal_length must be an integer in [0, 7] (8 verification rows per slot)")
    prompts = [[int(t) for t in p] for p in prompts]
    if any(not p for p in prompts):
        raise ValueError("every prompt must hold at least one token")
    limits = [max_new_tokens] * len(prompts) if isinstance(max_new_tokens, int) else list(max_new_tokens)
    if len(limits) != len(prompts) or any(not isinstance(n, int) or isinstance(n, bool) or n < 0 for n in limits):
        raise ValueError("max_new_tokens must be a non-negative integer, or one per prompt")
    wave = min(int(target.max_batch), int(draft.max_batch), 64 // (proposal_length + 1))
    if wave < 1:
        raise ValueError("the engines hold no slot")
    counts = {"target_calls": 0, "draft_steps": 0, "proposed": 0, "accepted": 0, "resampled": 0, "rounds": 0}
    outs: list[list[int]] = [[] for _ in prompts]
    for first in range(0, len(prompts), wave):
        group = prompts[first:first + wave]
        token: dict[int, int] = {}       # live slots: the pending token (predicted by the target, not yet emitted or cached)
        drafted: set[int] = set()
        held_t: set[int] = set()

        def finish(s: int) -> None:
            token.pop(s, None)
            if s in held_t:
                held_t.discard(s)
                target.release(s)
            if s in drafted:
                drafted.discard(s)
                draft.release(s)

        def settle(s: int) -> None:
            """The sequence ends where its pending token is the EOS or the last id it may emit (no pass is spent on that one)."""
            if token[s] != eos_token_id and len(outs[first + s]) == limits[first + s] - 1:
                outs[first + s].append(token[s])
            if len(outs[first + s]) >= limits[first + s] or token[s] == eos_token_id:
                finish(s)

        try:
            for s, prompt in enumerate(group):
                if limits[first + s] == 0:
                    continue
                target.begin(s)
                held_t.add(s)
                target.prefill(s, prompt)
                token[s] = target.read_tokens(s, 1)[0]
                counts["target_calls"] += 1
                if proposal_length > 0:
                    draft.begin(s)
                    drafted.add(s)
                    draft.prefill(s, prompt, want_logits=False)
            for s in list(token):
                settle(s)
            while True:
                if not token:
                    break
                live = sorted(token)
                batch = live[-1] + 1
                room = {s: limits[first + s] - len(outs[first + s]) - 1 for s in live}  # proposals that could still be emitted after the pending token
                k = min(proposal_length, max(room.values()))
                proposals: dict[int, list[int]] = {s: [] for s in live}
                if k > 0:
                    for s in live:
                        draft.set_token(s, token[s])
                    draft.decode(k, batch=batch)
                    for s in live:
                        got = draft.read_tokens(s, k)
                        counts["draft_steps"] += k
                        keep = min(k, room[s])
                        if eos_token_id in got[:keep]:  # the draft stops proposing after its own EOS
                            keep = got.index(eos_token_id) + 1
                        if keep < k:
                            draft.rewind(s, k - keep)
                        proposals[s] = got[:keep]
                fed = {s: [token[s]] + proposals[s] for s in live}
                results = target.verify_batch([(s, fed[s]) for s in live], commit=True)
                counts["target_calls"] += 1
                counts["rounds"] += 1
                # fed[:a + 1] is what the target itself would have fed: emitted, unless an accepted proposal is the EOS
                accepted = {s: len(r) - 1 for s, r in zip(live, results)}
                for s, r in zip(live, results):
                    a = accepted[s]
                    counts["proposed"] += len(proposals[s])
                    stop = next((i for i in range(1, a + 1) if fed[s][i] == eos_token_id), None)
                    if stop is not None:
                        outs[first + s].extend(fed[s][:stop])
                        counts["accepted"] += stop - 1
                        finish(s)
                        continue
                    outs[first + s].extend(fed[s][:a + 1])
                    counts["accepted"] += a
                    token[s] = r[a]
                    settle(s)
                # the drafts of the slots that go on: fed[:a + 1] stays.  A draft whose proposals were all accepted has not consumed
                # the last one yet: one step for every live slot, taken back where it was not wanted.  (The step feeds each draft its
                # device-side pending token: for a bonus slot that is its last proposal, because a slot that kept fewer than k proposals
                # and had them all accepted has reached its limit or an EOS and is gone; what the others feed is rewound at once.)
                going = [s for s in live if s in token and s in drafted]
                bonus = [s for s in going if proposals[s] and accepted[s] == len(proposals[s])]
                if bonus:
                    draft.decode(1, batch=max(going) + 1)
                    counts["draft_steps"] += len(bonus)
                for s in going:
                    if s in bonus:
                        continue
                    back = len(proposals[s]) - (accepted[s] + 1) + (1 if bonus else 0)
                    if back > 0:
                        draft.rewind(s, back)
        finally:
            for s in sorted(held_t | drafted):
                finish(s)
    if stats is not None:
        stats.update(counts)
    return [o[:n] for o, n in zip(outs, limits)]


def lookup_generate_ids(engine, prompts: Sequence[Sequence[int]], max_new_tokens: int | Sequence[int], proposal_length: int = 4, max_ngram: int = 3,
                        min_ngram: int = 1, eos_token_id: int | None = None, *, stats: dict | None = None, sampling=None,
                        base_seed: int = 0) -> list[list[int]]:
    """Speculative decoding without a draft model: ``batch_speculative_generate_ids``' loop with prompt lookup as the proposer
    (``DecodeEngine.lookup_propose``: the ids that followed the longest earlier occurrence of a sequence's last 1 .. ``max_ngram`` ids).
    Prompts run in waves of at most ``min(engine.max_batch, 64 // (proposal_length + 1))`` slots, prompt i of a wave on slot i, each
    armed before its prefill so that the prompt is part of what is matched.  Per round ONE ``lookup_propose`` over the live slots (each
    clipped to the ids it may still emit); where any slot got a proposal, one ``verify_batch(..., commit=True)`` over all live slots --
    a slot without a proposal goes in with its pending token alone -- and where none did, one captured ``decode(1, batch)`` step whose
    ids are read back.  A sequence that finishes is released and drops out of later rounds; the last id it may emit is its pending
    token, which costs no pass.
    Returns, per prompt, the engine's greedy continuation (up to ``max_new_tokens`` ids -- one number, or one per prompt -- stopping
    before ``eos_token_id``).  ``stats`` receives ``rounds`` (verify_batch calls), ``steps`` (decode steps), ``proposed`` and
    ``accepted``.
    ``sampling``: one dict for every request or one per prompt with the keys ``temperature``, ``top_k``, ``top_p`` and ``seed`` only
    (verification takes the raw rows, so any other key is a ValueError that names it); a request without a seed draws from ``base_seed``
    + its index.  Each slot then gets ``set_sampling`` before it is armed and prefilled -- its first token is the device sampler's --
    the rounds use ``lookup_propose(..., sampled=True)`` and ``verify_batch_sampled(..., commit=True)``, and the ids returned are
    distributed exactly as ``batch_generate_ids`` would sample them for the same settings (a lookup proposal is a deterministic function
    of the sequence: its draft distribution is one-hot, and the accept / residual rule is exact for it).  None: the greedy loop, with
    exactly the calls it has always made."""
    if not isinstance(proposal_length, int) or isinstance(proposal_length, bool) or not 1 <= proposal_length <= 7:
        raise ValueError("proposal_length must be an integer in [1, 7] (8 verification rows per slot)")
    _ext.lookup_params(max_ngram, min_ngram, proposal_length)
    prompts = [[int(t) for t in p] for p in prompts]
    if any(not p for p in prompts):
        raise ValueError("every prompt must hold at least one token")
    limits = [max_new_tokens] * len(prompts) if isinstance(max_new_tokens, int) else list(max_new_tokens)
    if len(limits) != len(prompts) or any(not isinstance(n, int) or isinstance(n, bool) or n < 0 for n in limits):
        raise ValueError("max_new_tokens must be a non-negative integer, or one per prompt")
    settings = None
    if sampling is not None:
        dicts = [sampling] if isinstance(sampling, dict) else list(sampling)
        other = sorted({k for d in dicts if isinstance(d, dict) for k in d} - {"temperature", "top_k", "top_p", "seed"})
        if other:
            raise ValueError(f"lookup_generate_ids verifies raw rows: sampling takes temperature, top_k, top_p and seed only, not {other}")
        settings = [r.sampling for r in request_settings(sampling, len(prompts), base_seed)]
    wave = min(int(engine.max_batch), 64 // (proposal_length + 1))
    if wave < 1:
        raise ValueError("the engine holds no slot")
    counts = {"rounds": 0, "steps": 0, "proposed": 0, "accepted": 0}
    outs: list[list[int]] = [[] for _ in prompts]
    for first in range(0, len(prompts), wave):
        group = prompts[first:first + wave]
        token: dict[int, int] = {}  # live slots: the pending token (predicted, not yet emitted or cached)
        held: set[int] = set()

        def finish(s: int) -> None:
            token.pop(s, None)
            if s in held:
                held.discard(s)
                engine.release(s)

        def settle(s: int) -> None:
            """The sequence ends where its pending token is the EOS or the last id it may emit (no pass is spent on that one)."""
            if token[s] != eos_token_id and len(outs[first + s]) == limits[first + s] - 1:
                outs[first + s].append(token[s])
            if len(outs[first + s]) >= limits[first + s] or token[s] == eos_token_id:
                finish(s)

        try:
            for s, prompt in enumerate(group):
                if limits[first + s] == 0:
                    continue
                engine.begin(s)
                held.add(s)
                if settings is not None:
                    engine.set_sampling(s, *settings[first + s])
                engine.set_lookup(s)
                engine.prefill(s, prompt)
                token[s] = engine.read_tokens(s, 1)[0]
            for s in list(token):
                settle(s)
            while token:
                live = sorted(token)
                room = {s: limits[first + s] - len(outs[first + s]) - 1 for s in live}  # proposals that could still be emitted after the pending token
                fed = dict(zip(live, engine.lookup_propose(live, [1 + min(proposal_length, room[s]) for s in live], max_ngram, min_ngram, proposal_length,
                                                           **({} if settings is None else {"sampled": True}))))
                for s in live:  # nothing is proposed behind an EOS
                    if eos_token_id in fed[s][1:]:
                        fed[s] = fed[s][:fed[s].index(eos_token_id, 1) + 1]
                if all(len(fed[s]) == 1 for s in live):
                    engine.decode(1, batch=live[-1] + 1)
                    counts["steps"] += 1
                    for s in live:
                        outs[first + s].append(token[s])
                        token[s] = engine.read_tokens(s, 1)[0]
                        settle(s)
                    continue
                verify = engine.verify_batch if settings is None else engine.verify_batch_sampled
                results = verify([(s, fed[s]) for s in live], commit=True)
                counts["rounds"] += 1
                for s, r in zip(live, results):
                    a = len(r) - 1
                    counts["proposed"] += len(fed[s]) - 1
                    stop = next((i for i in range(1, a + 1) if fed[s][i] == eos_token_id), None)
                    if stop is not None:  # fed[:a + 1] is what the engine itself would have fed: emitted, unless an accepted proposal is the EOS
                        outs[first + s].extend(fed[s][:stop])
                        counts["accepted"] += stop - 1
                        finish(s)
                        continue
                    outs[first + s].extend(fed[s][:a + 1])
                    counts["accepted"] += a
                    token[s] = r[a]
                    settle(s)
        finally:
            for s in sorted(held):
                finish(s)
    if stats is not None:
        stats.update(counts)
    return [o[:n] for o, n in zip(outs, limits)]
