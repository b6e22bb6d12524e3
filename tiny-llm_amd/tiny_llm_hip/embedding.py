"""Token embeddings, dense and W4 (reference: src/tiny_llm_ref/embedding.py)."""

import torch

from ._ext import tiny_llm_ext_hip
from .basics import linear
from .quantize import QuantizedWeights, dequantize_weights, quantized_linear


class Embedding:
    def __init__(self, vocab_size: int, embedding_dim: int, weight: torch.Tensor):
        self.vocab_size = vocab_size
        self.embedding_dim = embedding_dim
        self.weight = weight

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.weight[x.long()]

    def as_linear(self, x: torch.Tensor) -> torch.Tensor:
        return linear(x, self.weight)


class QuantizedEmbedding:
    """W4 table.  ``use_custom_kernel`` selects the fused gather+dequant kernel; without it (or without
    biases) rows are gathered and dequantised with readable torch ops (reference embedding.py:24-57)."""

    def __init__(self, vocab_size: int, embedding_dim: int, weight: QuantizedWeights, use_custom_kernel: bool = False):
        self.vocab_size = vocab_size
        self.embedding_dim = embedding_dim
        self.weight = weight
        self.use_custom_kernel = use_custom_kernel

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        w = self.weight
        if self.use_custom_kernel and w.biases is not None:
            return tiny_llm_ext_hip.quantized_embedding(
                x.to(torch.int32), w.scales, w.biases, w.weight, w.group_size, w.bits
            )
        rows = x.long()
        return dequantize_weights(
            w.weight[rows], w.scales[rows], None if w.biases is None else w.biases[rows], w.group_size, w.bits
        )

    def as_linear(self, x: torch.Tensor) -> torch.Tensor:
        return quantized_linear(x, self.weight)


# ---------------------------------------------------------------------------------------------------------------------
# Text embeddings: pooled, normalised output rows of the decode engine (DecodeEngine.embed / embed_packed)
# ---------------------------------------------------------------------------------------------------------------------
PACKED_SEQS = 16  # sequences per packed pass (tl_engine_embed_packed)


def embed_ids(engine, prompts, *, pooling: str = "last", normalize: bool = True, dim: int | None = None, lora=None):
    """Embeddings of ``prompts`` (lists of token ids) as float32 [len(prompts), dim], in input order.

    A batch scheduler over ``engine.embed_packed``: every pass is filled with up to 16 sequences (and the engine's ``max_batch``
    slots) and ``max_prefill_rows`` tokens; a prompt longer than the room left is split and its remainder leads the next pass; a
    prompt is admitted only while the pages of its whole length are obtainable (free plus evictable retained pages, less what the
    sequences already admitted will still take); one that does not fit an otherwise idle engine, or is longer than a sequence can
    be (``max_pages_per_seq * page_size``), is an error raised before anything runs or with every slot released.  With the prefix
    cache on and ``pooling="last"`` a prompt first attaches its cached prefix (``prefix_attach``) and embeds from its remaining
    tokens; never for ``"mean"``, whose vector needs every row.  Uses slots [0, min(16, max_batch)), which must be free; every slot
    it began is released, also on error.  ``lora``: the id of a resident LoRA adapter (DecodeEngine.load_lora) for every prompt, or a
    list with one id (or None / -1) per prompt; a prompt under an adapter bypasses the prefix cache."""
    import numpy as np

    loras = list(lora) if isinstance(lora, (list, tuple)) else [lora] * len(prompts)
    if len(loras) != len(prompts):
        raise ValueError("embed_ids: lora needs one adapter id per prompt (or one for all)")
    loras = [-1 if a is None else int(a) for a in loras]

    mode_args = tiny_llm_ext_hip.pooling_args(pooling, normalize, dim, int(engine.args.hidden_size))
    dim = mode_args[2]
    prompts = [[int(t) for t in p] for p in prompts]
    for i, p in enumerate(prompts):
        if not p:
            raise ValueError(f"embed_ids: prompt {i} is empty")
    out = np.zeros((len(prompts), dim), dtype=np.float32)
    rows_cap, page = int(engine.max_prefill_rows), int(engine.page_size)
    pages_of = lambda tokens: -(-tokens // page)
    seq_tokens = getattr(engine, "max_pages_per_seq", None)  # the longest sequence a slot can hold, where the engine tells
    seq_tokens = None if seq_tokens is None else int(seq_tokens) * page
    for i, p in enumerate(prompts):
        if seq_tokens is not None and len(p) > seq_tokens:
            raise RuntimeError(f"embed_ids: prompt {i} ({len(p)} tokens) can never fit: a sequence holds at most "
                               f"max_pages_per_seq * page_size = {seq_tokens} tokens")
    free = list(range(min(PACKED_SEQS, int(engine.max_batch))))[::-1]  # pop() hands out the lowest slot
    attach = bool(getattr(engine, "prefix_cache_enabled", False)) and pooling == "last"
    pending = list(range(len(prompts)))[::-1]
    held: dict[int, int] = {}  # slot -> prompt index
    carry = None  # (slot, prompt index, tokens done): the split prompt whose remainder leads the next pass
    try:
        while pending or carry is not None:
            chunks, owners, room, promised = [], [], rows_cap, 0
            _, obtainable = engine.step_pages(1)

            def take(slot, idx, pos):
                nonlocal room, carry
                n = min(room, len(prompts[idx]) - pos)
                ends = pos + n == len(prompts[idx])
                chunks.append((slot, prompts[idx][pos:pos + n], ends))
                owners.append((slot, idx))
                room -= n
                if not ends:
                    carry = (slot, idx, pos + n)

            if carry is not None:
                slot, idx, pos = carry
                carry = None
                promised += pages_of(len(prompts[idx])) - pages_of(pos)
                take(slot, idx, pos)
            while pending and free and room > 0 and len(chunks) < PACKED_SEQS:
                idx = pending[-1]
                need = pages_of(len(prompts[idx]))
                if need + promised > obtainable:
                    if not held:
                        raise RuntimeError(f"embed_ids: prompt {idx} ({len(prompts[idx])} tokens, {need} KV pages) can never fit: "
                                           f"{obtainable} pages are obtainable on the idle engine")
                    break
                pending.pop()
                slot = free.pop()
                engine.begin(slot)
                held[slot] = idx
                promised += need
                if loras[idx] >= 0:
                    engine.set_lora(slot, loras[idx])
                pos = engine.prefix_attach(slot, prompts[idx]) if attach else 0
                take(slot, idx, pos)
            vectors = engine.embed_packed(chunks, pooling=pooling, normalize=normalize, dim=dim)
            done = [(slot, idx) for (slot, idx), chunk in zip(owners, chunks) if chunk[2]]
            for row, (slot, idx) in enumerate(done):
                out[idx] = vectors[row]
                engine.release(slot)
                del held[slot]
                free.append(slot)
    finally:
        for slot in list(held):
            try:
                engine.release(slot)
            except Exception:
                pass
    return out


def format_query(task: str, text: str) -> str:
    """A query in the Qwen3-Embedding instruction format (documents are embedded as they are)."""
    return f"Instruct: {task}\nQuery:{text}"


ENDOFTEXT = "<|endoftext|>"  # the token Qwen3-Embedding models pool on: their tokenizer appends it to every text


def text_ids(tokenizer, text: str, *, task: str | None = None, eos_id: int | None = None) -> list[int]:
    """Token ids of ``text`` as a Qwen3-Embedding model expects them: ``format_query(task, text)`` when ``task`` is given (a query),
    the bare text otherwise (a document), then the end-of-text id -- ``eos_id``, or the tokenizer's id of ``<|endoftext|>``.  Feed
    the result to ``embed_ids`` with ``pooling="last"``."""
    if eos_id is None:
        eos_id = tokenizer.convert_tokens_to_ids(ENDOFTEXT)
        if eos_id is None or int(eos_id) < 0:
            raise ValueError(f"text_ids: the tokenizer has no {ENDOFTEXT} token; pass eos_id")
    full = format_query(task, text) if task is not None else text
    try:  # (a Qwen3-Embedding tokenizer appends the id itself when asked for special tokens: it is appended once, here)
        ids = tokenizer.encode(full, add_special_tokens=False)
    except TypeError:
        ids = tokenizer.encode(full)
    return [int(t) for t in ids] + [int(eos_id)]
