/*
 * tinyllm_engine.h — C ABI of the fused Qwen3 W4A16 forward ("decode engine").
 *
 * The reference runs one token through ~690 separately dispatched MLX primitives
 * (layer loop: src/tiny_llm_ref/qwen3_week2.py:357-392, qwen3_week3.py:320-338;
 * per-layer ops: qwen3_week3.py:55-121,141-147,181-187).  On an MI355X the whole
 * 382 us/token budget would be spent in launch gaps, so the same arithmetic is
 * issued here as 5 kernels per layer, captured once in a hipGraph and replayed:
 *
 *   1. RMSNorm -> fused QKV W4 GEMV                 (input_layernorm + wq|wk|wv)
 *   2. q/k-RMSNorm + RoPE + paged KV append + split-context GQA attention
 *      (+ a merge kernel only when the context is split)
 *   3. wo W4 GEMV + residual add
 *   4. RMSNorm -> gate|up W4 GEMV -> SwiGLU         (post_attention_layernorm + MLP in)
 *   5. w_down W4 GEMV + residual add
 *   final: RMSNorm -> lm_head W4 GEMV -> argmax -> next-token embedding gather.
 *
 * Every reference op boundary is kept as a bf16 rounding point inside the fused
 * kernels, so logits track the op-by-op path (tests/test_engine_gpu.py).
 *
 * State that changes every token (token ids, context lengths, step counter) lives
 * in device memory and is advanced by the last kernel of the step, so a captured
 * step replays without host involvement; the host only appends a page id to a
 * block-table row when a sequence crosses a page boundary.
 *
 * The multi-token path (chunked prefill, reference Request.try_prefill
 * src/tiny_llm_ref/batch.py:48-76) uses the MFMA W4 GEMM and the paged
 * FlashAttention kernel of tinyllm_hip.h with the same fused weight layout.
 *
 * KV storage is the reference's paged layout, one pool per layer:
 * key/value pages [P, Hkv, page_size, D] bf16 (paged_kv_cache.py:21-242), block
 * table [max_batch, max_pages_per_seq] int32 (-1 = unused), context_lens
 * [max_batch] int32 (kv_cache.py:210-224).  Pools are owned by the engine and
 * sized once at creation (288 GB of HBM: no growth path on the hot loop).
 *
 * All functions return 0 / negative tl_status; message via tl_last_error().
 * Pointers named *_dev are device pointers; everything else is host memory.
 */
#ifndef TINYLLM_ENGINE_H
#define TINYLLM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tl_engine tl_engine;

/* One W4 (group 128) linear: packed [rows, in/8] uint32, scales/biases [rows, in/128] bf16. */
typedef struct tl_w4 {
    const uint32_t *weight_dev;
    const void *scales_dev;
    const void *biases_dev;
    int rows; /* out features */
    int cols; /* in features  */
} tl_w4;

/* Per-layer weights in the engine's fused layout (built by the host mirror,
 * tiny_llm_hip/engine.py, from the mlx_lm-shaped checkpoint object):
 *   wqkv  rows = [q (Hq*D) | k (Hkv*D) | v (Hkv*D)]                      cols = hidden
 *   wo    rows = hidden                                                  cols = Hq*D
 *   wgu   rows interleaved: 2i = gate_proj row i, 2i+1 = up_proj row i   cols = hidden
 *   wdown rows = hidden                                                  cols = intermediate */
typedef struct tl_layer_weights {
    tl_w4 wqkv, wo, wgu, wdown;
    const void *input_norm_dev; /* [hidden] bf16 */
    const void *post_norm_dev;  /* [hidden] bf16 */
    const void *q_norm_dev;     /* [D] bf16 */
    const void *k_norm_dev;     /* [D] bf16 */
} tl_layer_weights;

typedef struct tl_engine_config {
    int hidden_size, num_layers, num_heads, num_kv_heads, head_dim, intermediate_size, vocab_size;
    float rope_theta, rms_norm_eps;
    int page_size;         /* tokens per KV page (reference default 128, qwen3_week3.py:222) */
    int num_pages;         /* physical pages per layer pool */
    int max_batch;         /* sequence slots */
    int max_pages_per_seq; /* block-table width */
    int max_prefill_rows;  /* largest prefill chunk (rows of the activation workspace).  From 1,792 rows the engine also keeps the layer
                              matrices as bf16 (rows x cols x 2 bytes each: 7.3 GB at Qwen3-4B) for the plain bf16 GEMM of large chunks */
} tl_engine_config;

/* Counters mirroring the pool statistics the reference serving bench prints
 * (paged_kv_cache.py:36-40, benches/bench.py:546-556). */
typedef struct tl_engine_stats {
    int pages_in_use, pages_free, peak_pages_in_use;
    long page_allocations, reused_page_allocations;
    long decode_steps, graph_captures, graph_replays, prefill_tokens;
    size_t kv_bytes, workspace_bytes;
    long graph_cache_flushes; /* times the cache of captured decode graphs (48 plans) was emptied */
    long aql_steps;           /* decode steps replayed as AQL packets on the engine's own HSA queue (TL_AQL=1; 0 on the hipGraph route) */
} tl_engine_stats;

/* A Qwen3-MoE layer (reference: src/tiny_llm_ref/qwen3_week3.py:209-214, 258-272 builds a Moe block for it; moe.py:39-89 is the
 * block: router softmax in fp32 -> top_k experts -> gathered gate / up / down W4 products -> probability-weighted sum).
 * router [E, hidden]; experts stacked on a leading axis: gate / up [E, I, hidden/8] words, down [E, hidden, I/8] words, scales /
 * biases [E, rows, cols/128] bf16.  W4, group 128.  Borrowed memory, like every weight. */
typedef struct tl_moe_weights {
    tl_w4 router;
    const uint32_t *gate_dev, *up_dev, *down_dev;
    const void *gate_scales_dev, *gate_biases_dev, *up_scales_dev, *up_biases_dev, *down_scales_dev, *down_biases_dev;
    int num_experts;        /* E <= 1024 */
    int experts_per_token;  /* top_k <= 16 */
    int intermediate_size;  /* I (moe_intermediate_size), a multiple of 128 */
    int norm_topk_prob;     /* renormalise the selected probabilities (Qwen3-MoE: true) */
} tl_moe_weights;

/* embed: the quantized embedding table [vocab, hidden]; lm_head: NULL for tied
 * embeddings (reference qwen3_week3.py:314-318).  Weight memory is borrowed and
 * must outlive the engine.  `stream` is the hipStream_t all work is issued on;
 * NULL makes the engine create and own a non-blocking stream (the legacy default
 * stream cannot be graph-captured) after a device-wide synchronise. */
int tl_engine_create(const tl_engine_config *cfg, const tl_layer_weights *layers, const tl_w4 *embed,
                     const void *final_norm_dev, const tl_w4 *lm_head, void *stream, tl_engine **out);
/* The same engine with its KV pages in another format ("quantized-KV"; NO reference interface is
 * replaced -- the reference lists quantised KV caches as not covered, README.md:134-135).  TL_KV_FP8_E4M3 (head_dim 128 only):
 * every K / V row is stored as 128 OCP FP8 E4M3 codes + one power-of-two float32 scale (include/tinyllm_hip.h, csrc/kv8.h,
 * oracle/kv_fp8.py): 132 bytes per row instead of 256.  Rows are quantised where they are written (prefill's qkv_post launch, the
 * decode attention's append) and every attention kernel reads the codes; the token being decoded is quantised before it is attended
 * to.  The model's arithmetic is otherwise unchanged: attention over the dequantised rows, which are exact bfloat16 values.
 * tl_engine_create == tl_engine_create_kv(..., TL_KV_BF16, ...). */
enum { TL_KV_BF16 = 0, TL_KV_FP8_E4M3 = 1 };
int tl_engine_create_kv(const tl_engine_config *cfg, const tl_layer_weights *layers, const tl_w4 *embed, const void *final_norm_dev,
                        const tl_w4 *lm_head, void *stream, int kv_format, tl_engine **out);
/* TL_KV_BF16 or TL_KV_FP8_E4M3 */
int tl_engine_kv_format(const tl_engine *e);
/* Make `layer` a mixture-of-experts layer (after tl_engine_create, before the first prefill / decode of the engine).  The layer's
 * dense wgu / wdown may be null in tl_engine_create's `layers` then; a layer with neither is an error at its first use.  The MoE
 * MLP runs as the reference's op sequence inside the captured step: RMSNorm, router GEMV, route kernel, gathered gate and up
 * GEMVs (one launch each, an expert per row), SiLU x up, gathered down GEMV, weighted sum + residual. */
int tl_engine_set_moe_layer(tl_engine *e, int layer, const tl_moe_weights *w);
/* Test / lab hook: switch a route that has an A/B twin, per engine, before its first prefill / decode (an error afterwards: captured
 * steps hold the routes they were captured with).  value 0 = off, anything else = on.  Options (defaults in brackets):
 *   "qmm3" [1] rows > 8 of a decode step on the K-sliced skinny matmul (0: the prefill GEMM's op sequence);  "qmm6" [1] the
 *   register-resident batched matmul (0: the K-sliced one everywhere);  "qmm7" [1] the row-streaming matmul for gate|up / qkv (0: qmm6);
 *   "gemm8" [1] prefill chunks of 1,792 rows and more through the plain bf16 GEMM over the bf16 weight copy (0: the W4 GEMM at every size);
 *   "attn_qkv_partials" [1] the decode attention adds the qkv slice planes itself;  "lmhead_tile_max" [1] per-tile maxima from the lm_head
 *   GEMV;  "gemm_fused_epilogue" [1] residual / SwiGLU inside the prefill GEMM;  "prefill_reduce_norm" [1] the split-K residual
 *   reduction of a small prefill chunk also writes the RMSNorm behind it;  "aql_fences" [0] HIP's agent-scope fences back on every
 *   packet of the AQL route.  Not part of the reference's surface: product code never calls it. */
int tl_engine_set_option(tl_engine *e, const char *name, int value);
void tl_engine_destroy(tl_engine *e);
/* Block the host until everything enqueued on the engine stream has finished. */
int tl_engine_synchronize(tl_engine *e);

/* Sequence slots ------------------------------------------------------------
 * begin: claim slot (must be free), context 0.  Fails with TL_ERR_INVALID when
 *        the slot is live.
 * reserve: make sure pages exist for `total_tokens` tokens of context (allocates
 *        from the free list, appends to the slot's block-table row); fails
 *        without side effects when the pool or the table width is exhausted
 *        (transactional like TinyKvPagedCache._append_chunk, paged_kv_cache.py:271-312).
 * release: return the slot's pages to the free list, context 0, row = -1.
 * rewind: drop the last n tokens of the slot (reference rewind(), paged_kv_cache.py:414-434). */
int tl_engine_begin(tl_engine *e, int slot);
int tl_engine_reserve(tl_engine *e, int slot, int total_tokens);
int tl_engine_release(tl_engine *e, int slot);
int tl_engine_rewind(tl_engine *e, int slot, int n);
int tl_engine_context_len(const tl_engine *e, int slot);  /* host mirror, <0 if slot free */
/* Adopt the sequence of slot `src` into the free slot `dst` (reference BatchingKvCache.add_request,
 * kv_cache.py:226-238): block-table row, context length and pending token change hands, no K/V bytes move. */
int tl_engine_move(tl_engine *e, int src, int dst);

/* Chunked prefill of ONE slot: runs `n` tokens (host int32 ids) at positions
 * [context, context+n) through the multi-token path, appends their K/V, and, when
 * want_logits != 0, computes the last row's logits + greedy token which becomes
 * the slot's pending input token for the next decode step.  n <= max_prefill_rows. */
int tl_engine_prefill(tl_engine *e, int slot, const int32_t *tokens, int n, int want_logits);

/* The same for up to 16 slots in ONE pass (continuous batching: several admitted prompts prefilled together -- reference
 * batch.py:48-76 prefills one request per turn; here the projections run once over the concatenated rows, at the row count
 * the MFMA GEMM is efficient at, while RoPE / KV append / paged attention stay per sequence).  tokens = the chunks back to
 * back (sum of lens <= max_prefill_rows), lens[i] tokens for slots[i] at positions [context_i, context_i + lens[i]);
 * want_logits[i] != 0: that chunk ends its prompt -> last-row logits + greedy token become the slot's pending token.
 * All-or-nothing: slot states, page counts and row totals are checked before anything is reserved. */
int tl_engine_prefill_packed(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens,
                             const int *want_logits);

/* Prefix sharing (reference KvPrefixGenerator fork/restore, agent/branching.py:42-208): make the
 * free slot `dst` a second sequence with the same tokens as the live slot `src`.  Full KV pages are shared (reference
 * counted, never rewritten), a partially filled tail page is copied; the pending input token is copied too.  Afterwards
 * both slots decode, rewind and release independently. */
int tl_engine_fork(tl_engine *e, int src, int dst);

/* Prefix cache: K/V reuse ACROSS requests (csrc/prefix_cache.h, csrc/kv_copy.h; the reference lists cross-request
 * prefix caching as not covered, README.md:134-135: an extension, off by default).  With the cache off the engine is the program it
 * was: tl_engine_release returns every page to the free list, and nothing below is allocated.  It touches no decode step.
 *   record   while the cache is enabled the engine keeps, per live slot, the token ids of positions [0, known) on the host.
 *            tl_engine_prefill, tl_engine_prefill_packed, tl_engine_score and tl_engine_verify extend it when they append at position
 *            == known.  Decode steps do not (their ids live on the device): tl_engine_prefix_extend lets the caller declare the tokens
 *            of [known, known + n), known + n <= context length, from tl_engine_read_tokens.  THE ENGINE CANNOT VERIFY DECLARED IDS: a
 *            caller that declares other tokens than the slot holds publishes K/V under a wrong key.  tl_engine_rewind sets known =
 *            min(known, context), tl_engine_move carries the record, tl_engine_fork copies it, begin / release empty it.
 *   index    a full page whose page_size tokens all lie inside known is registered as an ENTRY, keyed by (parent entry, the page's
 *            tokens); the root is the parent of page 0.  Registration is stream ordered, like tl_engine_fork: a later attach reads the
 *            bytes behind everything enqueued before it.  A hash speeds the lookup up; a match is decided by comparing the stored
 *            tokens, never by the hash alone.  If an equal entry already exists under another physical page, the existing entry
 *            stays, the slot's page stays private and the slot's later pages register as children of the existing entry.  An indexed
 *            page is never written again.
 *   retention  when the last slot lets go of an indexed page it becomes RETAINED, not free: pages_in_use + pages_free +
 *            pages_retained == num_pages at every return.  Wherever a need was compared with the free pages (reserve, a decode step's
 *            pages, rewind's and fork's copy, packed prefill) it is compared with free + evictable pages, all-or-nothing as before; a
 *            page is taken from the free list first, then by eviction, and only then is the answer "KV page pool exhausted".
 *   eviction  victims are entries that no slot references and that have no indexed child, least recently used first, ties by the
 *            lower page id.  An attach or a registration touches the whole chain, so ancestors are never older than descendants and
 *            eviction is leaf first; an entry never stays indexed under a parent that is gone; a page a slot references is never
 *            taken.  (A retained entry above a referenced descendant -- a slot that registered under an equal entry of another
 *            request -- waits for the descendant.)  max_retained_pages > 0 caps the retained pages: whenever a page becomes retained,
 *            victims go back to the free list until the cap holds or no victim is left; 0 = no cap.
 *   attach   tl_engine_prefix_attach(e, slot, tokens, n, &matched): the slot is live, its context is 0, it holds no pages, n >= 1.
 *            Cache disabled: TL_OK and matched = 0 (a scheduler may call it unconditionally).  Otherwise matched is the largest
 *            m <= n - 1 obtainable -- one token is always left to prefill, because its row yields the logits: walk the chain of full
 *            pages while page j's tokens equal tokens[j P, (j + 1) P) and (j + 1) P <= n - 1; these f pages are shared (reference
 *            counted).  Then the child of the last matched entry (a page-0 entry when f = 0) with the longest common prefix r >= 1
 *            against tokens[f P, min(n - 1, (f + 1) P)) -- ties by most recent use, then the lower page id -- has its first r rows copied
 *            into a fresh private page (one launch, tl_kv_copy_rows): m = f P + r.  A prompt that ends exactly on a cached page
 *            boundary therefore matches n - 1 tokens.  If no page can be had for the copy the tail is skipped; that is no error.
 *            The block-table row, the device and host context length change exactly as tl_engine_fork changes them, known = m, the
 *            pending token does not change: tl_engine_set_token + tl_engine_decode work afterwards as after a fork.  A slot that
 *            processes its logits has the matched tokens marked as prompt tokens in its history (the launch prefill uses), so a hit
 *            equals a cold run with the parameters set before the prefill.  Sampling positions, grammar state and log-probability
 *            settings depend on the context length alone.
 *   rewind   the copy-on-write condition of tl_engine_rewind is "the tail page is shared OR INDEXED": a rewind that lands inside an
 *            indexed page gives the slot a private copy before anything is appended.
 *   reproducibility  a hit reads the publisher's K/V bytes: the result is that of a cold run whose prefix was prefilled in the
 *            publisher's chunks, bit for bit; against a cold run chunked differently it agrees within the usual chunked-versus-
 *            one-shot band.
 * tl_engine_prefix_cache: enabled 0 / 1, max_retained_pages >= 0; switching off clears the index first; legal at any time (a slot that
 * is live when the cache is switched on has known = 0).  The first enabling call allocates the index and a device table of the pools;
 * an engine that never enables the cache allocates nothing.  tl_engine_prefix_extend with the cache disabled is TL_OK and does nothing.
 * tl_engine_prefix_clear drops every entry: retained pages return to the free list, pages in use stay with their slots.  Bad input is
 * TL_ERR_INVALID with nothing changed. */
typedef struct tl_prefix_stats {
    long lookups, hits, tokens_matched, tail_rows_copied, pages_registered, pages_evicted;
    int entries, pages_retained, max_retained_pages, enabled;
} tl_prefix_stats;
int tl_engine_prefix_cache(tl_engine *e, int enabled, int max_retained_pages);
int tl_engine_prefix_attach(tl_engine *e, int slot, const int32_t *tokens, int n, int *matched);
int tl_engine_prefix_extend(tl_engine *e, int slot, const int32_t *tokens, int n);
int tl_engine_prefix_clear(tl_engine *e);
int tl_engine_prefix_stats(const tl_engine *e, tl_prefix_stats *out);
/* The tail copy over caller pools, in one launch (csrc/kv_copy.h): pools_dev is a DEVICE table of n_pools descriptors; pool i is
 * [pages][heads][page_size][row_bytes_i] bytes.  Rows [0, rows) of every head of page from_page are copied to page to_page in every
 * pool (16 bytes per lane where a head's run is 16-byte aligned, 4 bytes per lane otherwise, e.g. row_bytes 4); nothing else is
 * written.  1 <= rows <= page_size, from_page != to_page; the page ids are the caller's to keep inside its pools.  Stream ordered. */
typedef struct tl_kv_pool_desc {
    void *base_dev;
    size_t row_bytes;
} tl_kv_pool_desc;
int tl_kv_copy_rows(const tl_kv_pool_desc *pools_dev, int n_pools, int heads, int page_size, int from_page, int to_page, int rows,
                    void *stream);

/* KV swap: preempt a sequence under page pressure by moving its K/V to host memory, resume it later (csrc/kv_swap.h,
 * csrc/kv_swap_model.h; the reference has no preemption: an extension, off by default).  It touches no decode step
 * and no existing kernel, and an engine that never calls tl_engine_swap_space allocates nothing.
 *   swap space  tl_engine_swap_space(e, host_pages): a pinned host arena of host_pages PAGE RECORDS and a device staging buffer (up to 32 MiB
 *            of records, at least one); 0 frees both; TL_ERR_INVALID while a slot is parked.  A record holds one page of every pool
 *            (tl_kv_page_record_bytes); tl_swap_stats.record_bytes reports it.
 *   park     tl_engine_park(e, slot): the slot is live, not parked, context >= 1, and ceil(context / page_size) host records are free --
 *            otherwise TL_ERR_INVALID with nothing changed.  On the engine stream, in groups of at most the staging buffer's pages: one
 *            gather launch (tl_kv_gather_pages over the slot's block-table row), then one device-to-host copy per run of consecutive
 *            records (one per group unless the arena is fragmented).  Then the slot lets go of its pages exactly as tl_engine_release
 *            does -- reference counts drop, pages others share stay with them, indexed pages become retained, the rest return to the free
 *            list (pages reserved beyond the context go too) -- its block-table row becomes -1 and the DEVICE context length and live
 *            word become 0.  Everything else of the slot stays where it is: pending token, sampling parameters, log-probability setting
 *            and pending record, penalties, bias list and history row, grammar and its state, token ring and produced count, the prefix
 *            record's known tokens, and the host context length (tl_engine_context_len keeps answering it).  Freed pages may be taken
 *            again at once: the gather is enqueued first and stream order protects the bytes.  The call does not synchronise; unpark
 *            and release order themselves behind it on the same stream.
 *   unpark   tl_engine_unpark(e, slot): needs ceil(context / page_size) obtainable pages (free first, then eviction), otherwise
 *            TL_ERR_INVALID, nothing changes and the slot stays parked.  Fresh private pages, host-to-device copies + one scatter launch
 *            per group, block-table row, context length and live word restored, host records returned to the arena.  With the prefix
 *            cache on, the slot's full pages inside its known tokens go through the registration a prefill uses (an equal entry under
 *            another page stays, the slot's page stays private).  pages_in_use + pages_free + pages_retained == num_pages at every return.
 *   a parked slot  is a slot without a sequence to tl_engine_decode: plan selection, page reservation, tl_engine_step_bytes and the step's
 *            kernels leave every piece of its state untouched (its device penalty / bias / grammar parameters are held neutral while it
 *            is parked and written back by unpark, because the processing launch does not read the live word; the step end rewrites the
 *            activation row and RoPE factors of every row of the range, and the next tl_engine_decode derives both again from the pending
 *            token and the context length before its first step).  tl_engine_move carries the parked records with the slot;
 *            tl_engine_release returns them to the arena.  Refused with TL_ERR_INVALID, nothing changed: prefill, prefill_packed, score,
 *            verify, fork (as source), rewind, reserve, prefix_attach, prefix_extend, and park again.  Still accepted: the set_* calls
 *            (they write per-slot arrays only) and the read calls.
 *   routes   both replay routes are supported: park and unpark are stream work, and on the AQL route tl_engine_decode waits for the
 *            stream before its first captured step and drains its queue before it returns, which orders a step behind an unpark and a
 *            park behind a step.
 * tl_engine_slot_parked: 1 / 0, < 0 if the slot is free.  tl_engine_step_pages (host only): `need` = pages the next decode step over
 * slots [0, batch) would take, `obtainable` = free + evictable pages: a scheduler preempts while need > obtainable. */
typedef struct tl_swap_stats {
    int host_pages, host_pages_in_use;
    long parks, unparks, pages_out, pages_in;
    size_t record_bytes;
} tl_swap_stats;
int tl_engine_swap_space(tl_engine *e, int host_pages);
int tl_engine_park(tl_engine *e, int slot);
int tl_engine_unpark(tl_engine *e, int slot);
int tl_engine_slot_parked(const tl_engine *e, int slot);
int tl_engine_step_pages(const tl_engine *e, int batch, int *need, int *obtainable);
int tl_engine_swap_stats(const tl_engine *e, tl_swap_stats *out);
/* The two launches over caller pools (csrc/kv_swap.h): the pages named by the DEVICE list page_ids_dev[n_pages] are copied into
 * (gather) / out of (scatter) a contiguous staging buffer of page records.  Record j lies at j * record_bytes and holds, pool after pool
 * in table order, that pool's [heads][page_size][row_bytes_i] bytes; record_offsets_dev[i] = heads * page_size * (row_bytes_0 + .. +
 * row_bytes_{i-1}) is a device table the caller fills once; record_bytes >= tl_kv_page_record_bytes(...) (0 on bad input).  Of the LAST
 * page only rows [0, tail_rows) of every head move, 1 <= tail_rows <= page_size: gather leaves the rest of that record, scatter the
 * rest of that page, as it was; scatter writes nothing outside the named pages.  A negative page id is skipped.  1 <= n_pages <= 65,535.
 * Stream ordered; bad input is TL_ERR_INVALID. */
size_t tl_kv_page_record_bytes(const tl_kv_pool_desc *pools_host, int n_pools, int heads, int page_size);
int tl_kv_gather_pages(const tl_kv_pool_desc *pools_dev, const size_t *record_offsets_dev, int n_pools, int heads, int page_size,
                       const int32_t *page_ids_dev, int n_pages, int tail_rows, void *staging_dev, size_t record_bytes, void *stream);
int tl_kv_scatter_pages(const tl_kv_pool_desc *pools_dev, const size_t *record_offsets_dev, int n_pools, int heads, int page_size,
                        const int32_t *page_ids_dev, int n_pages, int tail_rows, const void *staging_dev, size_t record_bytes, void *stream);

/* Speculative verification (reference speculative_generate, generate.py:84-322: one target call over the pending token
 * plus the draft's proposals, logits_to_keep = all rows).  Appends n (1..8) tokens to the slot exactly like a prefill chunk
 * and returns in out_ids[i] the greedy token that follows tokens[0..i].  Nothing is recorded as generated; the caller
 * rewinds the rejected suffix with tl_engine_rewind and sets the next input with tl_engine_set_token.  Synchronises. */
int tl_engine_verify(tl_engine *e, int slot, const int32_t *tokens, int n, int32_t *out_ids);

/* Speculative sampling: verification for a slot that samples (csrc/spec_sample.h; Leviathan et al. 2023, Chen et
 * al. 2023).  Appends the n (1..8) tokens exactly like tl_engine_verify, then runs tl_spec_sample_rows once on the engine stream over the n
 * rows of logits: the slot's own (temperature, top_k, top_p, seed) for the target; proposals tokens[1..n-1] and -1 (a bonus row) for the
 * last row; draft_logits_dev [n-1, V] bf16 on the device, row i the row the draft drew tokens[i+1] from under (draft_temperature,
 * draft_top_k, draft_top_p) (may be NULL when n == 1); position of row i = context length before the call + i + 1, the sampler's own
 * position rule.  With a = the first rejected row (n-1 when none is): out_ids[0..a) = tokens[1..a+1), out_ids[a] = that row's alt,
 * *out_count = a + 1 -- tokens distributed exactly as if the slot had sampled them alone, whatever the draft.  Nothing is recorded as
 * generated; the caller rewinds n - 1 - a tokens and sets the next input, as after tl_engine_verify.  Refuses what tl_engine_verify
 * refuses except sampling, and a slot that truncates (min-p / typical-p) or runs Mirostat (their kept sets are not this routine's); a
 * greedy slot is verified greedily.  The 8-row scratch is allocated by the first call.  Synchronises. */
int tl_engine_verify_sampled(tl_engine *e, int slot, const int32_t *tokens, int n, const void *draft_logits_dev, float draft_temperature,
                             int draft_top_k, float draft_top_p, int32_t *out_ids, int *out_count);

/* Batched speculative verification (csrc/verify_attn.h): up to 8 tokens for each of n_seqs >= 1 slots in ONE pass
 * over the decode route, acceptance decided on the device.  `tokens` holds the chunks back to back as tl_engine_prefill_packed takes
 * them; lens[i] is 1..8, their sum at most 64, no slot twice.  Sequence i appends its n = lens[i] tokens exactly like tl_engine_verify
 * (the first is the pending token, the others the proposals).  With g[j] the greedy id behind row j (the lower id of a tie, never a
 * NaN) and a the first j < n - 1 with g[j] != tokens[j + 1] (n - 1 when there is none): out[i].count = a + 1 and out[i].ids[0..a] =
 * g[0..a] (the accepted proposals, then the correction or the bonus token); the other ids are -1.  Nothing is recorded as generated.
 *   commit == 0   the caller rewinds n - 1 - a tokens and sets the next input itself, as after tl_engine_verify;
 *   commit != 0   the call rewinds every slot by n - 1 - a and sets ids[a] as its pending token before it returns, by the paths of
 *                 tl_engine_rewind and tl_engine_set_token (copy of a shared tail page, known tokens and page accounting as there).
 * The pass is eager on the engine stream: per layer the projections over all rows at once on the shared-buffer decode route (the GEMV up
 * to 4 rows, the batched matmuls from 5) and one attention stage for all sequences; its own logits block, so the rows of the last decode
 * step or verification stay where they were.  All or nothing: every check -- slot state, the pages the chunks (and, with commit, the
 * copy of a tail page a rewind may need) ask of the pool, token range -- is made before anything is reserved or written.  Refuses
 * (TL_ERR_INVALID) what tl_engine_verify refuses -- parked or stopped slots, slots that sample, slots that process their logits -- a
 * slot that carries a LoRA adapter, head_dim != 128, and a model with MoE layers when the rows exceed max(max_batch, max_prefill_rows).
 * FP8 KV pages and MoE layers are supported.  Out of scope: adapters, and captured or AQL replay of the pass; slots that sample are
 * verified in batch by tl_engine_verify_batch_sampled below.  The scratch (activations, logits and matmul workspace for 64 rows,
 * descriptors, results) is allocated by the first call and counted in stats.workspace_bytes.  Synchronises once. */
typedef struct tl_verify_result {
    int32_t count;
    int32_t ids[8];
} tl_verify_result;
int tl_engine_verify_batch(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, int commit,
                           tl_verify_result *out);

/* Batched speculative SAMPLING (csrc/verify_sample.h): tl_engine_verify_batch for slots that sample.  The same
 * checks, the same all-or-nothing behaviour, the same pass over the same scratch and the same `commit` handling; only the acceptance
 * launches and what is refused of a slot differ.  Greedy and sampling slots may share a call.
 *   rows       sequence i owns rows row0[i] .. row0[i] + lens[i] - 1 of the pass (the chunks back to back); its context length before
 *              the call is starts[i].  For row r = row0[i] + j: the proposal is x = tokens[r + 1] for j < lens[i] - 1 and -1, a bonus
 *              row, on the last row; the position is starts[i] + j + 1 (the sampler's own position rule, tl_engine_verify_sampled's);
 *              the target parameters are the slot's own (temperature, top_k, top_p, seed), read on the device where
 *              tl_engine_set_sampling keeps them -- no per-call record is uploaded.
 *   weights    kept set, weights wp and Wp = sum wp (fp32), one-hot rows and the uniforms u_acc (third counter word 0x53504143) and
 *              u_res (0x53505253) are exactly tl_spec_sample_rows'; a bonus row gives tl_sample_logits' own draw, bit for bit.
 *   drafted    draft_logits_dev != NULL: row r of draft_logits_dev [R, V] bf16 is the row tokens[r + 1] was drawn from; one
 *              (draft_temperature, draft_top_k, draft_top_p) holds for the whole call; the draft row at a bonus position is never read.
 *              accept and alt of a row are tl_spec_sample_rows', unchanged.
 *   point      draft_logits_dev == NULL: the proposal is a deterministic function of the sequence (prompt lookup), so its draft
 *              distribution is one-hot at x.  Accepted iff u_acc Wp < wp_x (one fp32 product).  Rejected: r_j = wp_j for j != x, r_x = 0,
 *              alt = the first id whose inclusive cumulative r exceeds u_res R, with tl_spec_sample_rows' fallbacks where rounding
 *              leaves no crossing.  x >= V is rejected without a read at x and the residual is wp whole.  By construction this is what
 *              tl_spec_sample_rows returns for a draft row whose first maximum is x under draft temperature 0 (wq = Wq = 1) -- without
 *              the draft row: the target row alone is read.
 *   result     a = the first j < lens[i] - 1 whose row rejects (lens[i] - 1 when none does): out[i].count = a + 1, ids[0 .. a) the
 *              accepted proposals tokens[row0 + 1 .. row0 + a], ids[a] row a's alt (the residual draw, or the bonus row's ordinary
 *              draw), the rest -1 -- distributed exactly as the slot's own samples, whatever was proposed.  A greedy slot (temperature
 *              0) has a one-hot target row: its result is exactly tl_engine_verify_batch's.
 * Refuses what tl_engine_verify_batch refuses except sampling -- parked or stopped slots, a slot twice, slots that process their logits,
 * adapter slots, head_dim != 128, the MoE row limit -- and a slot that truncates (min-p, typical-p, Mirostat); needs V <= 524,288 and a
 * finite draft_temperature >= 0.  Out of scope: a sampled draft-model loop on top of the drafted path, verification of processing or
 * truncating slots, adapters, captured replay of the pass.  accept / alt of 64 rows are allocated by the first call (workspace_bytes).
 * Synchronises once.
 * tl_engine_copy_verify_logits: rows [row0, row0 + rows) of the last batched verification's own logits block (either call) to dst_dev
 * [rows, V] bf16, device to device, stream ordered: the very rows its acceptance stage read.  TL_ERR_INVALID before the first pass or
 * when the range lies outside the rows of the last pass. */
int tl_engine_verify_batch_sampled(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens,
                                   const void *draft_logits_dev, float draft_temperature, int draft_top_k, float draft_top_p, int commit,
                                   tl_verify_result *out);
int tl_engine_copy_verify_logits(tl_engine *e, int row0, int rows, void *dst_dev);

/* Prompt lookup: draft-free proposals for tl_engine_verify_batch, made on the device (csrc/lookup.h).  The
 * proposer -- "ngram" speculation, prompt_lookup_num_tokens -- finds the last few ids of a sequence earlier in the sequence and proposes
 * what followed them.
 *   rule       T[s0 .. e] are a row's ids, last = T[e]; N = max_ngram in 1 .. TL_LOOKUP_MAX_NGRAM, min_ngram in 1 .. N, K = num_proposals in
 *              1 .. TL_LOOKUP_MAX_PROPOSALS.  A candidate is every i in [s0, e) with T[i] == last; raw(i) = the largest
 *              m <= min(N, i - s0 + 1) with T[i - j] == T[e - j] for all 0 <= j < m; it is eligible with raw(i) >= min_ngram;
 *              avail(i) = min(K, e - i).  The choice is the eligible candidate with the largest (raw, avail, i), compared in that order:
 *              the longest match, then the most continuation ids, then the most recent.  The proposals are T[i + 1 .. i + avail]; none
 *              where nothing is eligible.  Integer compares decide everything: the result is the same on every run.
 *   history    tl_engine_set_lookup(e, slot, 1) arms a live slot: from then on the engine keeps the slot's ordered ids resident on the
 *              device, H[j] = the id whose K/V sits at position j, for s0 <= j < context length, s0 = the context length at arming (ids
 *              before it are unknown and never matched; arm right after tl_engine_begin to have the prompt matched).  e is the context
 *              length and last the slot's pending token.  The ids of prefill, packed prefill, score, embed and verify chunks and of a
 *              prefix attach are recorded as they are uploaded; tl_engine_set_token's token too.  A DECODE STEP RECORDS NOTHING: it is
 *              the program it was, with or without an armed slot.  The ids the steps produced lie in the slot's token ring (4,096 ids);
 *              the propose launch fetches them from there first, and so do tl_engine_rewind, tl_engine_fork, tl_engine_move and a chunk
 *              about to be recorded (one small launch, only where the slot is behind).  A decode call that would leave more than 4,095
 *              unrecorded ids launches that fetch ahead of itself; a single call of more than 4,095 steps starts the slot's history over
 *              instead: s0 = the context length the call leaves.
 *   life       tl_engine_begin and tl_engine_release switch it off, tl_engine_move carries the history, tl_engine_fork copies it, park /
 *              unpark keep it, tl_engine_rewind shortens it (a rewind below s0 lowers s0), beam search refuses the slot.  Arming an
 *              armed slot changes nothing.  The history rows (max_batch x max_pages_per_seq x page_size x 4 bytes) and the results of one
 *              launch are allocated by the first arming call and counted in stats.workspace_bytes.
 * tl_engine_lookup_propose: proposals for n_seqs (1 .. 64) armed slots in one launch (one workgroup per slot), one small device-to-host
 * copy and one synchronisation.  tokens_out / lens_out are exactly the `tokens` / `lens` of tl_engine_verify_batch over the same slots:
 * each chunk is the slot's pending token followed by its proposals, at most min(K, max_lens[i] - 1) of them (max_lens NULL: 8 each),
 * the chunks back to back (tokens_out: room for the sum of max_lens, at most 64).  It refuses, with nothing done, whatever
 * tl_engine_verify_batch refuses of a slot (parked, stopped, sampling, processing, Mirostat or adapter slots), an unarmed slot, a slot
 * named twice, a sum of max_lens above 64 and parameters out of range.
 * tl_engine_lookup_state: whether the slot is armed, s0, and how far H is recorded (NULL: not wanted). */
#define TL_LOOKUP_MAX_NGRAM 16
#define TL_LOOKUP_MAX_PROPOSALS 7
int tl_engine_set_lookup(tl_engine *e, int slot, int on);
int tl_engine_lookup_propose(tl_engine *e, int n_seqs, const int *slots, const int *max_lens, int max_ngram, int min_ngram, int num_proposals,
                             int32_t *tokens_out, int *lens_out);
int tl_engine_lookup_state(const tl_engine *e, int slot, int *armed, int *start, int *recorded);
/* tl_engine_lookup_propose for the slots of tl_engine_verify_batch_sampled: the same arguments, results and proposer launch; it refuses
 * of a slot what that call refuses (so a sampling slot is taken, a truncating one is not) in place of what tl_engine_verify_batch refuses. */
int tl_engine_lookup_propose_sampled(tl_engine *e, int n_seqs, const int *slots, const int *max_lens, int max_ngram, int min_ngram,
                                     int num_proposals, int32_t *tokens_out, int *lens_out);

/* Set the pending input token of a slot explicitly (e.g. sampled on the host). */
int tl_engine_set_token(tl_engine *e, int slot, int32_t token);

/* Per-slot sampling on the device (csrc/sample.h).  The live slot draws every token it produces from here on --
 * the first token of a later prefill with want_logits, and every decode step -- under (temperature, top_k, top_p, seed):
 *   order   tokens by logit, highest first, equal logits by the lower id first (NaN logits are never ranked, counted or drawn);
 *   top-k   top_k > 0: exactly the first min(top_k, V) tokens of that order (ties at the k-th are cut by id; the host mirror
 *           tiny_llm_hip.make_sampler keeps every token tied with the k-th instead);
 *   top-p   0 < top_p < 1: a token stays while the temperature-1 probability exp(l - m) / sum_V exp(l - m) (full vocabulary, m the
 *           row maximum, NOT renormalised after top-k) of the kept tokens ranked before it sums to less than top_p; the first stays;
 *   draw    w_i = exp((l_i - m) / T) over the kept set, W = sum w_i (fp32); u = Philox4x32-10 with key (seed & 0xffffffff, seed >> 32)
 *           and counter (position, 0, 0x53414d50, 0), u = (word 0 >> 8) * 2^-24; the token is the first kept token in ascending id
 *           whose inclusive cumulative w exceeds u W (rounding leaving none: the last kept token).  position = tokens in the sequence
 *           before the sampled one (the prompt length for the first token after a prefill, +1 per decode step), so a draw depends
 *           on (logits row, parameters, seed, position) only -- not on the slot, the batch, the replay route or how steps are split.
 * temperature 0 (the default) is greedy: the same id as an engine that never calls this.  temperature must be finite and >= 0;
 * top_k 0 or >= V: no top-k; top_p outside (0, 1): no top-p.  Sampling needs V <= 524,288.  The parameters live in a host mirror
 * and a per-slot device array written on the engine stream between steps.  tl_engine_begin / tl_engine_release reset the slot to
 * greedy, tl_engine_move moves the parameters with the sequence, tl_engine_fork copies them (seed included: give the child its own
 * seed, or both draw the same tokens).  tl_engine_verify refuses a sampling slot (verification is greedy; tl_engine_verify_sampled
 * verifies one). */
int tl_engine_set_sampling(tl_engine *e, int slot, float temperature, int top_k, float top_p, uint64_t seed);

/* Per-token log-probabilities (csrc/logprob.h).  For a bf16 logits row l of V entries, m its maximum over non-NaN
 * entries:
 *   lse      m + log(sum_j exp(l_j - m)), summed in fp32 over non-NaN entries;  logprob(t) = l_t - lse.  This is the model's
 *            distribution at temperature 1, unfiltered (the reference's logits - logsumexp(logits)).  For a slot that samples, the value
 *            reported is still the model's log-probability of the token drawn -- NOT its probability under the sampler's truncated or
 *            rescaled distribution;
 *   top-N    (0 <= N <= TL_MAX_TOP_LOGPROBS) the first N tokens in exactly the sampler's order: logit descending, equal logits by the
 *            lower id, NaN never ranked (the kept set of top_k = N, listed in that order).  Entries past N, or past the number of
 *            rankable tokens, are id -1 with logprob -inf;
 *   edges    a NaN logit has logprob NaN; a row without a finite maximum (all NaN / -inf, or holding +inf) has every logprob NaN,
 *            and its top-N ids still follow the order.
 * A row's values depend on the row alone: not on the batch, the replay route, eager or captured steps or how steps are split.
 *
 * tl_engine_set_logprobs: top_n -1 switches the slot off (the default), 0 .. 20 records one tl_token_logprob per token the slot
 * produces from its next one on -- the first token of a later prefill with want_logits (tl_engine_prefill, tl_engine_prefill_packed)
 * and every decode step.  A step in which some live slot records ends with the logprob twin of the step-end launch (its own captured
 * plan); otherwise the step is unchanged.  The first call that switches a slot on allocates the records (max_batch x ring capacity x
 * 164 bytes); an engine that never asks allocates nothing.  tl_engine_begin / tl_engine_release switch the slot off, tl_engine_move
 * carries the setting and the pending record with the sequence, tl_engine_fork copies them.  tl_engine_verify records nothing.
 * tl_engine_read_logprobs: the records of the last `count` tokens of the slot (like tl_engine_read_tokens: the same ring capacity,
 * restarted by tl_engine_move); TL_ERR_INVALID when count exceeds the tokens produced since logprobs were switched on (0 while off).
 * tl_engine_read_pending_logprobs: the record of each pending token of slots [0, count) (a slot that never recorded: logprob NaN,
 * ids -1), one copy after synchronising -- the companion of tl_engine_read_pending. */
#define TL_MAX_TOP_LOGPROBS 20
typedef struct tl_token_logprob {           /* 164 bytes */
    float logprob;                           /* log p(token) of the produced token */
    int32_t top_ids[TL_MAX_TOP_LOGPROBS];    /* -1 past top_n */
    float top_logprobs[TL_MAX_TOP_LOGPROBS]; /* -inf past top_n */
} tl_token_logprob;
int tl_engine_set_logprobs(tl_engine *e, int slot, int top_n);
int tl_engine_read_logprobs(tl_engine *e, int slot, int count, tl_token_logprob *out);
int tl_engine_read_pending_logprobs(tl_engine *e, int count, tl_token_logprob *out);

/* Penalties and logit bias (csrc/logit_process.h): what changes the logits BEFORE the choice.  For a slot that
 * processes, every logits row the slot would choose a token from -- each decode step, and the last row of a prefill / packed prefill with
 * want_logits -- is first turned into a processed bf16 row, and the existing choice (greedy first maximum, or the sampler of
 * tl_engine_set_sampling) runs on the processed row exactly as it runs on a raw row otherwise.
 *   history  per slot and token id j:  prompt[j] (a flag): j was among the tokens the slot consumed through tl_engine_prefill,
 *            tl_engine_prefill_packed or tl_engine_score while it was processing;  count[j]: how many of the tokens the slot produced and
 *            then fed back were j -- it goes up by one in every decode step the slot takes while processing, for that step's input token
 *            (the pending token the previous step end, or a prefill with want_logits, produced), BEFORE the step's row is processed.  So
 *            when token n + 1 is chosen, tokens 1 .. n of the output are counted, and a pending token that is never fed (the slot is
 *            released, or prefilled further) is never counted.  count saturates at 32,767.  (The split of vLLM and the OpenAI API:
 *            repetition looks at prompt and output, presence and frequency at the output only.)
 *   element  in fp32, ONE IEEE-754 single-precision operation per line, no fused multiply-add, division correctly rounded:
 *                v = float(l[j])                                                    the bf16 logit
 *                if prompt[j] or count[j] > 0:  v = v / r  if v > 0 else  v * r     r = repetition_penalty
 *                v = v - (frequency_penalty * float(count[j]))                      two operations
 *                if count[j] > 0:               v = v - presence_penalty
 *                v = v + bias[j]                                                    0 where the slot has no entry
 *                out[j] = bf16 round to nearest even of v
 *            A row that processes goes through every line, neutral stages included (a -0.0 logit may come out as +0.0 after v + 0.0; the
 *            two tie in every routine).  A row that does not process is copied bit for bit.  A NaN logit stays NaN (the sampler never
 *            ranks it); -inf as a bias value bans the token.  Subnormal fp32 values follow the device's fp32 denormal mode.
 *   slots    repetition_penalty finite and > 0 (1 = off), presence_penalty and frequency_penalty finite (0 = off; negative values
 *            encourage repetition, as in the OpenAI API).  Logit bias: up to TL_MAX_LOGIT_BIAS pairs (id, value), ids in [0, vocab) and
 *            distinct, values finite or -inf; a call replaces the slot's whole list, n = 0 clears it.  Anything else is TL_ERR_INVALID
 *            with nothing changed.  A slot PROCESSES iff some parameter is not neutral or its list is not empty.  History is tracked from
 *            the call that makes the slot process (set the parameters before the prompt's prefill); the call that makes it neutral again
 *            forgets the history.  Vocabulary limit as for the sampler (524,288).
 *   unchanged  tl_engine_logits_dev / tl_engine_copy_logits keep returning the RAW logits.  Log-probability records stay the model's
 *            distribution at temperature 1, unfiltered: computed from the raw row, for the token chosen from the processed row (a banned
 *            token is never the produced token, but may appear in the top-N).  The Philox position, the draw and the tie rules.  A step
 *            in which no live slot processes is the program it was: same captured plan, same kernels, same launches; a step in which one
 *            does has one more launch (many workgroups per row) between the lm_head and the step end, in a captured plan of its own.
 *   life     tl_engine_begin / tl_engine_release make the slot neutral and empty its history, tl_engine_move carries parameters, bias
 *            list and history with the sequence, tl_engine_fork copies them.  tl_engine_verify, tl_engine_rewind and tl_engine_set_token
 *            refuse a processing slot with TL_ERR_INVALID (after them the history would no longer be the tokens the sequence holds); they
 *            work again once the slot is neutral or re-begun.
 * The history table (max_batch x vocab x 2 bytes), the processed rows (the same size) and the bias lists are allocated by the first call
 * that makes a slot process; an engine that never asks allocates nothing. */
#define TL_MAX_LOGIT_BIAS 1024
int tl_engine_set_penalties(tl_engine *e, int slot, float repetition_penalty, float presence_penalty, float frequency_penalty);
int tl_engine_set_logit_bias(tl_engine *e, int slot, const int32_t *ids, const float *values, int n);

/* DRY and the n-gram ban: repetition control that looks at the ORDER of the tokens (csrc/dry.h).  DRY ("don't repeat
 * yourself", the sampler of text-generation-webui, llama.cpp and koboldcpp) penalises the token that would extend a verbatim repetition,
 * growing exponentially with the length of the repeat; no_repeat_ngram (Hugging Face generate's no_repeat_ngram_size) bans the token that
 * would complete an n-gram already present.  A slot with either on PROCESSES (above): the two launches of csrc/dry.h rewrite its
 * processed row -- the row after repetition / presence / frequency, bias and grammar mask; the raw row where nothing else is on -- and
 * the greedy rule, the sampler, the truncation launch and tl_engine_copy_processed_logits see that row.
 *   sequence   at the moment a token is chosen the slot's recorded ids are S[s0 .. e]: s0 = the context length the slot had when it was
 *              armed (0 right after tl_engine_begin, the normal use); S[e] = last = the token the step has just fed (for the first token
 *              after a prefill with want_logits: the prompt's last token).  Ids before s0 are unknown and never matched.
 *              M = TL_DRY_MAX_MATCH = 64.
 *   candidate  every i in [s0, e) with S[i] == last; its continuation is S[i + 1].  raw(i) = the largest m in [1, min(M, i - s0 + 1)]
 *              with S[i - j] == S[e - j] for all 0 <= j < m.
 *   n-gram     no_repeat_ngram n = 0 (off) or 2 .. 64: every continuation with raw(i) >= n - 1 is banned.  Breakers and the range do not
 *              apply to it.  With s0 = 0 this is transformers.NoRepeatNGramLogitsProcessor(n).
 *   DRY        (multiplier, base, allowed_length, range, breakers): multiplier finite and >= 0 (0 = DRY off), base finite and >= 1,
 *              allowed_length >= 1, range >= 0 (0 = the whole recorded sequence), up to TL_MAX_DRY_BREAKERS distinct token ids.
 *                lo = range > 0 ? max(s0, e + 1 - range) : s0
 *                B  = the number of consecutive j >= 0 with e - j >= lo and S[e - j] not a breaker, capped at M (a last token that is a
 *                     breaker gives B = 0: no DRY penalty on this choice)
 *                d(i) = min(raw(i), B, i - lo + 1), for a candidate with i >= lo whose continuation is not a breaker
 *                L[t] = the largest d(i) over the candidates whose continuation is t; it counts where L[t] >= allowed_length
 *              (text-generation-webui's loop with the match capped at 64; at the default base 1.75 a 64-token match is a ban in effect)
 *   penalty    p = multiplier, then L[t] - allowed_length times p = p * base: fp32 products, rounded one by one (no powf).
 *   element    a banned token becomes bf16 -inf.  A token with a DRY entry becomes bf16 round to nearest even of float(v) - p; -inf where p
 *              is not finite; a NaN keeps its bits.  Every other token keeps its bits.  Log-probabilities go on describing the raw row.
 *   life       as for every processing slot: tl_engine_begin / tl_engine_release switch it off, tl_engine_move carries the parameters, the
 *              breakers, s0 and the sequence row, tl_engine_fork copies them, park / unpark keep them; tl_engine_rewind,
 *              tl_engine_set_token, the verify calls and beam search refuse the slot.  Changing parameters of an armed slot keeps s0 and
 *              the sequence; switching everything off and on again makes s0 the current context length.  The ids a slot consumes through
 *              tl_engine_prefill, tl_engine_prefill_packed, tl_engine_score or tl_engine_prefix_attach while it is armed are recorded.  A
 *              stopped slot's sequence and s0 stand where the text ended.
 *   plans      a step in which no live slot is armed is the program it was.  One in which a slot is has two more launches behind the
 *              processing launch, in a captured plan of its own (plan-key bit 53) that replays through hipGraphLaunch.
 * The sequence rows (max_batch x max_pages_per_seq x page_size x 4 bytes), the match table (max_batch x vocab x 4 bytes, all zeros between
 * steps) and the parameter arrays are allocated by the first call that arms a slot; an engine that never asks allocates nothing. */
#define TL_DRY_MAX_MATCH 64
#define TL_MAX_DRY_BREAKERS 64
int tl_engine_set_dry(tl_engine *e, int slot, float multiplier, float base, int allowed_length, int range, int no_repeat_ngram,
                      const int32_t *breaker_ids, int n_breakers);

/* Truncation: min-p, locally typical sampling and Mirostat v2 (csrc/truncate.h).  For a slot that SAMPLES
 * (temperature T > 0) and truncates, the bf16 row x the choice would be made from -- the raw row, or the processed row when the slot
 * processes penalties, bias or a grammar -- is first turned into a FILTERED bf16 row, and the existing choice runs on the filtered row
 * exactly as it runs on any row.  A greedy slot is never filtered: every filter below keeps the maximum.  With m the row maximum,
 * p_i = exp((x_i - m) / T) / sum_j exp((x_j - m) / T), summed over non-NaN entries in fp32 (NaN logits are never kept, as in the sampler).
 * The stages run in this order, each over the survivors of the one before:
 *   min-p      0 < min_p <= 1 (0 = off): token i stays iff p_i >= min_p * p_max, i.e. (x_i - m) / T >= ln(min_p)
 *              (transformers.MinPLogitsWarper applied to x / T);
 *   typical-p  0 < typical_p < 1 (anything else = off): over the survivors, renormalised, H = -sum p ln p and d_i = |(-ln p_i) - H|;
 *              delta* is the smallest deviation for which the mass of {d_i <= delta*} reaches typical_p; token i stays iff
 *              d_i <= delta*.  EVERY token tied with the boundary on deviation stays: the set depends on no ordering and no key is cut
 *              (transformers.TypicalLogitsWarper's kept set, closed under ties);
 *   Mirostat   v2 (Basu et al. 2021, algorithm 2): tau > 0, 0 < eta <= 1; per-slot state mu, 2 tau from every tl_engine_set_mirostat
 *              call with tau > 0.  Token i stays iff -log2 p_i <= mu; the first maximum always stays.  After the slot's token t has been
 *              drawn: s = -log2(p_t / sum_kept p) and mu <- mu - eta (s - tau), in fp32.  Mirostat excludes every other truncation of
 *              the slot (top-k, top-p, min-p, typical-p), as in llama.cpp: the call that would combine them -- tl_engine_set_sampling
 *              as much as the two calls below -- is TL_ERR_INVALID with nothing changed.
 *   filtered   tokens that stay keep their bf16 bits, every other token becomes bf16 -inf.  A row whose maximum is not finite (all NaN /
 *              -inf, or holding +inf) is copied bit for bit: its choice (token 0, the first +inf) depends on no filter.  So is the row
 *              of a slot that does not truncate or does not sample.
 *   sees it    the sampling twin and the logprob twin of the step end, with their tie rules, Philox position and draw; the slot's top-k
 *              and top-p therefore see the filtered row (top-p's mass is over the survivors).  Log-probability records stay the model's
 *              raw distribution, as for processed rows.  tl_engine_logits_dev / tl_engine_copy_logits keep returning the raw rows and
 *              tl_engine_copy_processed_logits keeps its meaning; tl_engine_copy_filtered_logits copies the filtered rows of the last
 *              step in which some live slot truncated (stream ordered; TL_ERR_INVALID before any slot has truncated).
 *   plan       a step in which no live slot truncates is the program it was.  One in which one does has one launch more ahead of the
 *              step end (one 1,024-thread workgroup per row, writing rows of its own: nothing is filtered in place) and the Mirostat
 *              update launch behind it (a no-op for rows without Mirostat), in a captured plan of its own.  The same pair runs where a
 *              prefill / packed prefill with want_logits chooses the slot's first token.  A plan with a live Mirostat slot stays on
 *              hipGraphLaunch (the update reads the token the step end stored, which only a launch boundary with cache maintenance
 *              hands over); tl_engine_replay_route says so while such a slot is live.
 *   life       tl_engine_begin / tl_engine_release reset the parameters, tl_engine_move carries them and mu with the sequence,
 *              tl_engine_fork copies them, park / unpark leave them alone.  tl_engine_rewind and tl_engine_set_token refuse a MIROSTAT
 *              slot with TL_ERR_INVALID (mu would no longer belong to the tokens held); min-p / typical-p slots are not refused.
 *              tl_engine_verify already refuses a sampling slot.
 * tl_engine_set_truncation: min_p in [0, 1], typical_p not NaN.  tl_engine_set_mirostat: tau finite and >= 0 (0 switches it off), eta
 * in (0, 1] when tau > 0.  tl_engine_mirostat_mu: the slot's mu (NaN without Mirostat) after synchronising.  Vocabulary limit as for
 * the sampler.  The filtered rows (max_batch x vocab x 2 bytes) and the parameters are allocated by the first call that makes a slot
 * truncate; an engine that never asks allocates nothing. */
int tl_engine_set_truncation(tl_engine *e, int slot, float min_p, float typical_p);
int tl_engine_set_mirostat(tl_engine *e, int slot, float tau, float eta);
int tl_engine_mirostat_mu(tl_engine *e, int slot, float *mu);
int tl_engine_copy_filtered_logits(tl_engine *e, void *dst_dev, int rows);

/* Grammars: regex-constrained decoding on the device (csrc/grammar.h).  A slot with a grammar may only produce
 * text that a byte-level DFA can still accept; the allowed set changes with every token and is decided inside the processing launch,
 * from tables uploaded once.  Nothing is uploaded per step.
 *   vocabulary  tl_vocab: for each token id j in [0, V) a byte string, given as offsets[V + 1] (int32, non-decreasing, offsets[0] = 0)
 *            plus bytes[offsets[V]].  A token with an empty byte string (special / control tokens) is never allowed under a grammar,
 *            unless it is one of the grammar's EOS ids.
 *   automaton  tl_grammar: n_states in 1 .. 32,768; table[n_states][256] uint16: the next state, 0xFFFF = no transition;
 *            accepting[n_states] uint8; start; eos_ids[n_eos], 1 <= n_eos <= 8, distinct, in [0, V).
 *            walk(s, j): feed token j's bytes from state s; the state reached, or DEAD if any step has no transition; an empty string
 *            is DEAD.
 *   state    per slot: a DFA state or TL_GRAMMAR_END.  tl_engine_set_grammar sets it to the start state.  Every token the slot produces
 *            AND THEN FEEDS BACK advances it, at the moment penalties count a token: the pending token, at the start of the decode step
 *            that consumes it, before that step's row is processed.  state' = END if the token is an EOS id or state is END, else
 *            walk(state, token) with DEAD -> END.  A pending token that is never fed advances nothing.
 *   allowed  in END: exactly the EOS ids.  Otherwise: token j with walk(s, j) != DEAD, plus the EOS ids iff accepting[s].  An EOS id is
 *            decided by the state alone, whatever its bytes: allowed in END and in an accepting state, disallowed in every other state
 *            even if its byte string could be walked (an EOS id ends the text; it never counts as text).
 *   element  one more line at the end of the processing definition above, after v = v + bias[j]:
 *                if not allowed[j]:  v = -inf
 *            so a bias cannot resurrect a disallowed token, and a NaN logit of a disallowed token becomes -inf.  A slot with a grammar
 *            PROCESSES: every rule of a processing slot applies to it.  Raw logits and log-probability records stay raw.
 *   edge     a state that is not accepting and in which no token of the vocabulary can be walked gives an all -inf row.  The choice
 *            routines then do what they do on any row without a finite maximum: token 0 (csrc/sample.h, the greedy rule and the
 *            sampler alike); token 0 cannot be walked from that state, so the next state is END.  A vocabulary that holds all 256
 *            single-byte tokens rules this out for an automaton whose every state can reach acceptance.
 *   life     tl_engine_begin / tl_engine_release clear the grammar; tl_engine_move carries grammar and state, tl_engine_fork copies
 *            them; tl_engine_verify, tl_engine_rewind and tl_engine_set_token refuse a grammar slot as they refuse any processing slot.
 *            g == NULL clears the grammar (the slot stops processing if nothing else makes it process); setting a grammar, the same one
 *            included, restarts at its start state.  Set on a slot that already holds a pending token, that token is still fed by the
 *            next step and advances the new state then (tl_engine_grammar_state includes it at once).  Grammar and vocabulary memory is borrowed: both must outlive the slots that use
 *            them, the vocabulary the grammars made from it; its V must be cfg.vocab_size.  Set the grammar before the prompt's
 *            prefill: the last row of a prefill with want_logits is masked with the state as it stands, and nothing advances there.
 *   determinism  a row's result depends on (row, parameters, history, state) only: not on the batch, the replay route, eager or captured
 *            steps, or how steps are split over calls.
 * A step with a live grammar slot runs the grammar twin of the processing launch, in a captured plan of its own; every other step is the
 * program it was.  tl_grammar_create also walks every token of more than 16 bytes from every state, once, on the device, and keeps one bit
 * per (state, such token) beside the table (n_states x long tokens / 8 bytes), so that no step walks a long token.
 * The per-slot pointers and state records are allocated by the first tl_engine_set_grammar.  Bad input (offsets, a
 * transition outside the table, start, the EOS ids, a vocabulary of another size) is TL_ERR_INVALID with nothing changed. */
typedef struct tl_vocab tl_vocab;
typedef struct tl_grammar tl_grammar;
#define TL_GRAMMAR_END (-1)
int tl_vocab_create(int vocab, const int32_t *offsets, const uint8_t *bytes, void *stream, tl_vocab **out);
void tl_vocab_destroy(tl_vocab *v);
int tl_grammar_create(const tl_vocab *v, int n_states, const uint16_t *table, const uint8_t *accepting, int start, const int32_t *eos_ids,
                      int n_eos, void *stream, tl_grammar **out);
void tl_grammar_destroy(tl_grammar *g);
int tl_engine_set_grammar(tl_engine *e, int slot, const tl_grammar *g);
/* state of the slot's sequence INCLUDING its pending token (the host walks the pending token on its mirror when the device has not
 * consumed it yet); *accepting = 1 when EOS would be allowed next.  Synchronises. */
int tl_engine_grammar_state(tl_engine *e, int slot, int *state, int *accepting);
/* the routine over caller rows: out[i][j] = logits[i][j] where j is allowed in states_dev[i] (a state or TL_GRAMMAR_END), else -inf;
 * nothing else of the processing definition, nothing advanced.  Stream ordered. */
int tl_grammar_mask_rows(const tl_grammar *g, const void *logits_dev, int rows, const int32_t *states_dev, void *out_dev, void *stream);

/* Stack grammars: JSON mode (csrc/grammar_stack.h).  Nested brackets are not regular; a stack grammar is the
 * automaton above with a bounded stack beside the state.  It is a tl_grammar made by a second constructor: everything that takes a
 * tl_grammar accepts it (tl_engine_set_grammar in particular), and every rule of the grammar section holds with a CONFIGURATION in place
 * of a state.
 *   tables   table[n_states][256] uint16: 0xFFFF = no transition; otherwise the next state or, for a pop, an index into pop_table.
 *            ops[n_states][256] uint8: 0 = no stack operation, 1 .. 4 = push symbol op - 1 (four stack symbols), 5 = pop; any other
 *            value is TL_ERR_INVALID.  pop_table[n_pop][5] uint16, 0 <= n_pop <= 65,535: the state after a pop, indexed by the NEW top of
 *            the stack (0 .. 3), or 4 when the stack became empty; 0xFFFF = dead.  accepting, start, eos_ids as above.  A non-pop
 *            entry must be < n_states, a pop entry < n_pop, a pop_table entry 0xFFFF or < n_states.
 *   configuration  per slot (state, depth, stack): depth in 0 .. 32; stack a uint64 with the symbol of level i (0 = bottom) in bits
 *            2i, 2i + 1 and zero above bit 2 * depth.  TL_GRAMMAR_END is (-1, 0, 0).  tl_engine_set_grammar sets (start, 0, 0).
 *   one byte b from (s, d, stack):  t = table[s][b]; DEAD if t == 0xFFFF.  op 0: s' = t.  Push a: DEAD if d == 32, else append a and
 *            s' = t.  Pop: DEAD if d == 0, else drop the top; top' = the new top, or 4 when the stack is now empty;
 *            s' = pop_table[t][top'], DEAD if that is 0xFFFF.
 *   walk / advance / allowed  the definitions above on configurations, for a token of up to 16 bytes; the advance of a slot with its
 *            pending token walks the real stack at ANY token length.  EOS is allowed iff accepting[state] (acceptance by final state:
 *            an automaton that wants "empty stack" at the end encodes the top of the stack in its states, as grammar.compile_json
 *            does), or in END.
 *   long tokens  (more than 16 bytes) are not walked in a step, and a bit per (state, token) cannot know the stack.  A long token is
 *            allowed in (s, d, stack) iff its walk from (s, EMPTY stack) never dies -- so it never pops below the level it starts at --
 *            and the largest depth m that walk reaches satisfies d + m <= 32.  tl_grammar_create_stack computes one byte per
 *            (state, long token), once, on the device: m, or 0xFF.  RESTRICTION: a long token that closes a container opened before
 *            it is therefore never allowed, and one that returns to its starting level continues as if the stack were empty there;
 *            the text stays reachable through shorter tokens.
 *   life     as for any grammar: begin / release clear, move carries, fork copies the configuration; verify, rewind and set_token
 *            refuse the slot.
 * A step with a live stack-grammar slot runs the third twin of the processing launch, in a captured plan of its own; it serves the
 * regex-grammar and grammar-less rows of that step with the results the other twins give.  Every other step is the program it was. */
int tl_grammar_create_stack(const tl_vocab *v, int n_states, const uint16_t *table, const uint8_t *ops, int n_pop, const uint16_t *pop_table,
                            const uint8_t *accepting, int start, const int32_t *eos_ids, int n_eos, void *stream, tl_grammar **out);
/* companion of tl_engine_grammar_state (which keeps returning the state alone): the configuration of the slot's sequence INCLUDING its
 * pending token; a regex grammar reports depth 0 and an empty stack.  Synchronises. */
int tl_engine_grammar_config(tl_engine *e, int slot, int *state, int *depth, uint64_t *stack, int *accepting);
/* the routine over caller rows for a stack grammar: row i is masked in (states_dev[i], depths_dev[i], stacks_dev[i]); a state of
 * TL_GRAMMAR_END ignores the rest.  tl_grammar_mask_rows refuses a stack grammar, this routine a regex grammar (TL_ERR_INVALID). */
int tl_grammar_mask_rows_stack(const tl_grammar *g, const void *logits_dev, int rows, const int32_t *states_dev, const int32_t *depths_dev,
                               const uint64_t *stacks_dev, void *out_dev, void *stream);

/* Scoring a given text: behaves like tl_engine_prefill(e, slot, tokens, n, want_logits = 0) for the KV cache and the context (same
 * limits: n <= max_prefill_rows, chunks longer than 8 tokens need head_dim 128), and also keeps every row: the final RMSNorm over the
 * chunk, the lm_head through the W4 GEMM in blocks of rows into a scoring scratch (allocated on first use), then the log-probability
 * routine per row.  out_logprobs[i] = log p(tokens[i+1] | the sequence through tokens[i]) for i < n - 1, out_logprobs[n-1] = that of
 * next_token (NaN when next_token < 0: a caller chunking a long text passes the next chunk's first token); out_argmax[i] (may be NULL)
 * = row i's greedy id.  The pending token, the logits of tl_engine_logits_dev, the token ring and the produced count are untouched.
 * Works for bf16 and FP8 KV pages and MoE engines.  Synchronises. */
int tl_engine_score(tl_engine *e, int slot, const int32_t *tokens, int n, int32_t next_token, float *out_logprobs, int32_t *out_argmax);

/* Embeddings: a text's vector is pooled from the model's output rows -- the final RMSNorm of the last layer's hidden rows, bf16 -- and
 * optionally truncated and L2-normalised (csrc/pool.h).  Qwen3-Embedding models are plain Qwen3 decoders that pool
 * the last token's row and normalise it.
 *   pooling    TL_POOL_LAST: the row of the text's last token, widened to fp32.  TL_POOL_MEAN: the mean of the rows of all its tokens:
 *              fp32 column sums per chunk join a per-slot running sum [hidden] (allocated for all slots by the first MEAN call), divided
 *              by the number of rows on finish.  Fixed summation order, no atomics: a text's vector depends on its tokens and on how they
 *              were cut into chunks, not on its slot, its place in a pass or its neighbours.
 *   finish     the first `dim` (1 .. hidden_size) components; with normalize != 0 divided by their Euclidean norm (fp32; a vector of norm
 *              0 stays all zeros, NaN propagates).  fp32 [dim].
 * tl_engine_embed_packed behaves exactly like tl_engine_prefill_packed with want_logits = 0 for the KV cache, the contexts, the prefix
 * cache's token record and the limits (head_dim 128, 1 .. 16 sequences, sum of lens <= max_prefill_rows, everything checked before
 * anything is reserved); tl_engine_embed is one slot through tl_engine_prefill's path with that call's limits.  finish[i] != 0 marks the
 * chunk that ends its text: that sequence's vector goes to the next `dim` floats of out_host, in the order of the call (out_host may be
 * NULL when nothing finishes).  The call synchronises when some sequence finishes and only enqueues otherwise.  The pending token, the
 * logits of tl_engine_logits_dev, the token ring, the produced count and every sampling / grammar / penalty / logprob setting are untouched.
 *   running mean   per slot the engine knows how many rows its running sum holds, or that it holds none.  A MEAN chunk must start at
 *              context 0 (the mean restarts) or at a context of exactly that many rows; anything else -- a context that came from
 *              tl_engine_prefix_attach, a prefill, a decode step, a fork, a move, a rewind or an unpark -- is TL_ERR_INVALID with nothing
 *              changed.  begin, release, move, fork (the new slot), rewind, park and unpark forget the sum.  LAST has no such rule: a
 *              prompt whose prefix was attached from the prefix cache embeds from its remaining tokens.
 * TL_ERR_INVALID with nothing changed: an unknown pooling mode, dim out of range, a null pointer, a parked or dead slot, a slot named
 * twice, a token id out of range.  bf16 and FP8 KV pages and MoE engines work unchanged (pooling reads the hidden rows only). */
#define TL_POOL_LAST 0
#define TL_POOL_MEAN 1
int tl_engine_embed_packed(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, const int *finish, int pooling,
                           int normalize, int dim, float *out_host);
int tl_engine_embed(tl_engine *e, int slot, const int32_t *tokens, int n, int finish, int pooling, int normalize, int dim, float *out_host);

/* LoRA adapters: many fine-tunes over one resident base model, a different one per slot, mixed in one batch (csrc/lora.h; DESIGN.md
 * section 4).  For an adapted projection with base weight W and an adapter (A [rank, in], B [out, rank], scale), all bf16, row-major, the
 * PEFT orientation, and x the input as the base projection sees it (after the RMSNorm where the projection has one):
 *     y = W x + scale * B (A x)     A x and B t accumulate in fp32, scale multiplies in fp32, rounding to bf16 only where a value is
 *                                   stored: bf16(base + delta) for q, k, v, gate and up, bf16(residual + delta) ahead of the base
 *                                   projection's residual epilogue for o and down.
 * No float atomics, one summation order: a row's result does not depend on its slot, its neighbours or their adapters, and a slot without
 * an adapter gets exactly the base result of the route it ran on.
 *   load     tl_engine_lora_load copies the adapter into engine-owned device memory in the fused layouts of the base weights (qkv: the A of
 *            q, k, v stacked, B block-wise; gate|up: the A of gate and up stacked, B rows interleaved like wgu); a target with a NULL pair
 *            is not adapted and costs nothing.  rank a multiple of 8 up to TL_MAX_LORA_RANK, the same for all targets of one adapter and
 *            free per adapter; scale finite; up to TL_MAX_LORA_ADAPTERS resident; *adapter receives the lowest free id.  A NULL A with a
 *            non-NULL B (or the reverse), a layer without any target in every layer, a bad rank: TL_ERR_INVALID.  An MLP target (gate, up,
 *            down) on a MoE layer: TL_ERR_UNSUPPORTED (attention targets there are fine).  The first load allocates the device table, the
 *            per-slot ids and the workspaces; an engine that never loads an adapter allocates nothing.  Synchronises.
 *   unload   TL_ERR_INVALID while a live or parked slot carries the adapter; the id is reused by a later load.  Synchronises.
 *   slots    tl_engine_set_lora(e, slot, adapter): adapter -1 = none, or a resident id; only on a live slot whose context is 0 -- a
 *            sequence's K/V are all computed under one adapter.  tl_engine_begin / tl_engine_release reset the slot to none,
 *            tl_engine_move moves the id, tl_engine_fork copies it, park / unpark keep it.  tl_engine_slot_lora: the id, -1 = none
 *            (also for a free slot).
 *   decode   a step in which some live slot of [0, batch) carries an adapter is a plan of its own (bit 55 of the graph key): every
 *            projection leaves complete bf16 rows in the shared buffers (no fragment-order hand-over, no kept slice planes, attention merges
 *            its own windows, gate|up through the store epilogue), with the shrink / expand launches around them: 8 launches more per
 *            layer.  Such a plan replays through hipGraphLaunch (tl_engine_replay_route says so while such a slot is live).  Every other
 *            step is the program it was, launch for launch: loading, unloading or assigning an adapter re-captures nothing.
 *   prefill  tl_engine_prefill, _prefill_packed, _verify, _score, _embed and _embed_packed: a pass in which some sequence carries an
 *            adapter runs shrink / expand per adapted projection group over tiles of 16 rows that never straddle two sequences; a pass
 *            without adapters is unchanged.
 *   prefix cache  K/V depend on the adapter.  A slot with an adapter bypasses the cache: tl_engine_prefix_attach matches 0 tokens and
 *            the slot's token ids are not recorded as known, so its pages are never indexed or retained.  PER-ADAPTER CACHING IS OUT OF
 *            SCOPE; the cache's own semantics are unchanged.
 * Not covered: adapters on the embedding / lm_head, DoRA, MLP targets on MoE layers. */
#define TL_MAX_LORA_RANK 64
#define TL_MAX_LORA_ADAPTERS 32
enum { TL_LORA_Q, TL_LORA_K, TL_LORA_V, TL_LORA_O, TL_LORA_GATE, TL_LORA_UP, TL_LORA_DOWN, TL_LORA_TARGETS };
typedef struct tl_lora_layer {
    const void *a_dev[TL_LORA_TARGETS], *b_dev[TL_LORA_TARGETS]; /* A [rank, in], B [out, rank] bf16; NULL pair = not adapted */
} tl_lora_layer;
typedef struct tl_lora_stats {
    int resident;              /* adapters loaded */
    size_t bytes;              /* device bytes of their matrices */
    long adapter_steps;        /* decode steps that ran the adapter plan */
    long adapter_prefill_rows; /* rows of prefill passes that belonged to a sequence with an adapter */
} tl_lora_stats;
int tl_engine_lora_load(tl_engine *e, const tl_lora_layer *layers, int rank, float scale, int *adapter);
int tl_engine_lora_unload(tl_engine *e, int adapter);
int tl_engine_set_lora(tl_engine *e, int slot, int adapter);
int tl_engine_slot_lora(const tl_engine *e, int slot);
int tl_engine_lora_stats(const tl_engine *e, tl_lora_stats *out);

/* The LoRA routine over caller rows (csrc/lora.h): x_dev [rows, in] bf16, one projection group of out columns.  row_adapter_dev [rows]
 * int32 names each row's adapter (-1 = none) among adapters[n_adapters] (host array of device matrices in the FUSED layout: a_dev
 * [rank * present segments, in], b_dev [out, rank]; seg_mask bit s = segment s is present).  seg_mode 0: one segment; 1: three blocks of
 * columns [0, seg_end0), [seg_end0, seg_end1), [seg_end1, out) (q | k | v); 2: interleaved, column parity (gate | up).  Tiles: n_tiles = 0
 * cuts the rows into blocks of 16 that look every row's adapter up; otherwise tile i is rows [tile_row0[i], + tile_rows[i] <= 16) with
 * adapter tile_adapter[i] (-1 none, -2 = look up per row).  mode TL_LORA_ADD: out_dev [rows, out] += delta in place; TL_LORA_RESIDUAL_PRE:
 * out_dev = bf16(base_or_residual_dev + delta); TL_LORA_SWIGLU: base_or_residual_dev holds interleaved gate|up rows [rows, out], out_dev
 * [rows, out / 2].  norm_w_dev != NULL: x is the row BEFORE an RMSNorm of that weight and eps, applied inside.  Allocates its table and
 * workspace per call and synchronises the stream: a test and measurement aid. */
enum { TL_LORA_ADD = 0, TL_LORA_RESIDUAL_PRE = 1, TL_LORA_SWIGLU = 2 };
typedef struct tl_lora_matrices {
    const void *a_dev, *b_dev;
    int rank, seg_mask;
    float scale;
} tl_lora_matrices;
int tl_lora_rows(const void *x_dev, int rows, int in, int out, const int32_t *row_adapter_dev, const tl_lora_matrices *adapters, int n_adapters,
                 int seg_mode, int seg_end0, int seg_end1, const int *tile_row0, const int *tile_rows, const int *tile_adapter, int n_tiles, int mode,
                 const void *base_or_residual_dev, void *out_dev, const void *norm_w_dev, float eps, void *stream);

/* Stop conditions: stop ids, stop strings and token budgets, decided on the device (csrc/stop.h, csrc/stop_set.h).
 * A slot may be ARMED with a stop set and a budget.  From arming on, each token t the step end COMMITS for the slot -- the first token of a
 * prefill with want_logits, and each decode step -- is examined once, in this order:
 *   1. generated += 1;
 *   2. stop id   t is one of the set's ids: stop with reason TL_STOP_ID, index = the position of t in the id list.  The token's bytes do not
 *                count as text: text_bytes is unchanged and cut_bytes = text_bytes;
 *   3. stop string  otherwise the bytes of t (tl_vocab; a token may have none) join the slot's text and are walked through the set's
 *                automaton one byte at a time.  With j the first byte of this token at which at least one stop string ends in the text
 *                produced since arming: stop with reason TL_STOP_STRING, index = the LONGEST stop string ending there (the earliest
 *                start).  text_bytes includes the whole token; cut_bytes = the text bytes before the match starts.  Matches span token
 *                boundaries: the automaton's state is per slot, lives on the device and starts at the root at arming;
 *   4. budget    otherwise, if max_new_tokens > 0 and generated == max_new_tokens: stop with reason TL_STOP_LENGTH, cut_bytes = text_bytes.
 *   freeze    on a stop the slot FREEZES AT THAT TOKEN: the stopping token is the slot's pending token and the last entry of its id ring,
 *             `produced` and the context length are as the step end left them, and from the next launch on the slot is a slot without a
 *             running sequence, for the rest of the call and for later calls.  Context length, produced count and id ring, the
 *             log-probability ring and its pending record, the penalty history, the grammar state / configuration, Mirostat's mu and the
 *             sampling position stand exactly where a run that executed `generated` tokens and then stopped calling the engine would have
 *             left them.  Other slots of the batch are unaffected, bit for bit.  (The launch clears the slot's device live word; the step
 *             end, the log-probability record, the Mirostat update and the processing launch's count and grammar advance test it.  The
 *             step end still leaves the uncommitted choice's embedding row as the slot's next input, so the attention launch keeps
 *             rewriting the K/V row at position `context` of the slot: outside the context, in a page the slot owns privately or in none,
 *             and written again from the real pending token when the slot resumes.)
 *   sets      tl_stop_create: up to TL_MAX_STOP_IDS ids, distinct, in [0, V); up to TL_MAX_STOP_STRINGS byte strings (bytes + offsets
 *             [n_strings + 1], offsets[0] = 0), non-empty, distinct, TL_MAX_STOP_BYTES in all; at least one id or string.  A set with
 *             strings needs a tl_vocab (of the engine's vocabulary size: checked when a slot is armed); a set of ids needs none (v may be
 *             NULL; its ids are checked against the engine's size when a slot is armed).  TEXT IS COUNTED IN THE SET'S VOCABULARY: a slot
 *             armed with a set made without one, or with a budget alone, knows no token's bytes -- text_bytes and cut_bytes stay 0.  The library builds the byte automaton itself -- a
 *             dense Aho-Corasick DFA [n_states][256] uint16 with, per state, the longest string ending there and its length -- and uploads it
 *             once.  A set is immutable and may be shared between slots, like a tl_grammar; set and vocabulary are borrowed by the slots.
 *   arming    tl_engine_set_stop(e, slot, set, max_new_tokens): set may be NULL (a budget alone); NULL with max_new_tokens 0 disarms.  The
 *             call ALWAYS resets the slot's record (generated 0, automaton at the root, text 0) and clears a stopped state: it is the one
 *             way to resume a stopped slot.  The state lives in a host mirror and per-slot device arrays poked on the engine stream between
 *             steps; the first arming call allocates them, an engine that never arms a slot allocates nothing.
 *   state     tl_engine_stop_state: the slot's record -- reason TL_STOP_NONE while it runs -- and its context length.  Synchronises.
 *   plan      a step in which a running slot is armed ends with one more launch (one wave per row; an unarmed, dead or stopped row
 *             leaves at once) in a captured plan of its own, bit 54 of the plan key.  Such a plan replays through hipGraphLaunch
 *             (tl_engine_replay_route says so while such a slot runs): the launch reads a plain store of the step end and writes the live
 *             word the next step's launches read.  Every other step is the program it was: same key, same launches, same route.
 *   mirrors   the host mirrors advance per step for every running slot, so a slot that froze in mid-call leaves them ahead of the device.
 *             A call that enqueued a stop launch is followed by a reconciliation -- wait for the stream, read the records in one copy, give
 *             every newly stopped slot the device's context length and produced count, mark it stopped -- by tl_engine_decode before it
 *             plans and before it returns, and by every call below that asks about a stopped state.  Pages reserved for steps the slot did
 *             not take stay with it, as after tl_engine_reserve; release or a rewind returns them.  pages_in_use + pages_free +
 *             pages_retained == num_pages at every return.
 *   life      tl_engine_begin / tl_engine_release disarm; tl_engine_move carries set, record and stopped state; tl_engine_fork copies
 *             them; park / unpark keep them (an unparked stopped slot stays stopped).  tl_engine_rewind, tl_engine_set_token and the
 *             read calls work on a stopped slot.  tl_engine_prefill, _prefill_packed, _verify, _score, _embed and _embed_packed on a stopped
 *             slot are TL_ERR_INVALID with nothing changed (re-arm or disarm first).  tl_engine_decode treats a stopped slot as it treats a
 *             parked one.  Bad input anywhere is TL_ERR_INVALID with nothing changed.
 * tl_stop_rows: the routine over caller rows, stream ordered: row i examines tokens_dev[i] under `set` (NULL: a budget alone) and
 * max_new_dev[i], with its record states_dev[i] and automaton state automaton_dev[i] read and written in place (a fresh row: all zero).
 * armed_dev (may be NULL: every row is armed) marks the rows that take part; an unarmed row and a row whose record already holds a reason
 * are left bit-identical.  The record's context field is not touched. */
#define TL_MAX_STOP_IDS 16
#define TL_MAX_STOP_STRINGS 16
#define TL_MAX_STOP_BYTES 1024
enum { TL_STOP_NONE = 0, TL_STOP_ID = 1, TL_STOP_STRING = 2, TL_STOP_LENGTH = 3 };
typedef struct tl_stop tl_stop;
typedef struct tl_stop_state {
    int32_t reason, index, generated, context;
    uint32_t text_bytes, cut_bytes;
} tl_stop_state;
int tl_stop_create(const tl_vocab *v, const int32_t *ids, int n_ids, const uint8_t *bytes, const int32_t *offsets, int n_strings, void *stream,
                   tl_stop **out);
void tl_stop_destroy(tl_stop *s);
int tl_engine_set_stop(tl_engine *e, int slot, const tl_stop *set, int max_new_tokens);
int tl_engine_stop_state(tl_engine *e, int slot, tl_stop_state *out);
int tl_stop_rows(const tl_stop *set, const int32_t *tokens_dev, int rows, const int32_t *armed_dev, const int32_t *max_new_dev,
                 int32_t *automaton_dev, tl_stop_state *states_dev, void *stream);

/* ---- Beam search (csrc/beam.h, csrc/slot_table.h) ----------------------------------------------------------------
 * A beam group is `width` plain greedy slots [slot0, slot0 + width): it decodes through tl_engine_decode like any other slots (other
 * requests may live in other slots of the batch; no plan, key or kernel of the step knows of beams), and between two steps the caller
 *   1. selects: tl_engine_beam_select ranks the (beam, token) pairs of the step's logits rows on the device and returns the best n_cand;
 *   2. decides on the host which candidates finish a hypothesis and which become the next beams (tiny_llm_hip/beam.py);
 *   3. reorders: tl_engine_beam_reorder makes slot slot0 + i the continuation of slot slot0 + parents[i] with pending token tokens[i].
 *
 * Selection (tl_beam_rows; per row the log-normaliser of tl_engine_set_logprobs, bit for bit):
 *   per row    lse = m + log(sum_j exp(l_j - m)) in fp32 over non-NaN entries, m their maximum, the sum in the fixed order that makes
 *              the value depend on the row alone; logprob(t) = l_t - lse.  NaN logits are never ranked.  A row without a finite maximum
 *              (all NaN / -inf, or holding +inf) contributes no candidate; neither does a row whose score is not finite (-inf: a dead beam)
 *   candidate  (parent, token) with score = scores[parent] + logprob, one fp32 addition
 *   order      score descending; equal scores by the lower parent, then by the row's own order, which is the sampler's (logit
 *              descending, equal logits by the lower token id)
 *   output     the first n_cand candidates of that order over all rows x vocab pairs; entries past the rankable pairs are
 *              {-1, -1, -inf, -inf}.  The result is bit-identical from call to call.
 * TL_MAX_BEAM_CANDIDATES is 32, not TL_MAX_TOP_LOGPROBS: a search keeps max(2, 1 + n_eos) * num_beams candidates, 24 for 8 beams and two
 * EOS ids.  tl_beam_rows is the routine over caller rows: logits_dev [rows, vocab] bf16 (vocab <= 524,288), 1 <= rows <= TL_MAX_BEAMS,
 * scores_dev [rows] float, 1 <= n_cand <= TL_MAX_BEAM_CANDIDATES -> out_dev, n_cand records.  Two launches on `stream`: one 1,024-thread
 * workgroup per row finds the row's first n_cand, one workgroup ranks the survivors.  The 4 KB of survivors between them are allocated
 * and freed by the call, so it returns after its launches have run (the engine's entry point keeps its own scratch and only enqueues).
 *
 * tl_engine_beam_select: tl_beam_rows on the engine stream over rows [row0, row0 + rows) of the most recent logits (after a decode step
 * row i is slot i; after a prefill with want_logits there is one row, row 0, the prefilled slot's) with scores_host [rows] uploaded,
 * the n_cand records copied to out_host; SYNCHRONISES.  TL_ERR_INVALID with nothing changed when the rows are not inside the most
 * recent logits (or those are a packed prefill's), or when a slot behind a row is free, parked or stopped, samples, processes its
 * logits (penalties, bias, grammar), truncates, records log-probabilities or is armed with a stop set.  The scratch (about 5 KB) is
 * allocated by the first call: an engine that never selects allocates nothing.
 *
 * tl_engine_beam_reorder: before, slots [slot0, slot0 + n_src) are live, plain (as above) and not parked, slots [slot0 + n_src, slot0 +
 * width) are free; 1 <= n_src, width <= TL_MAX_BEAMS; parents[i] in [0, n_src), tokens[i] in [0, vocab), i < width.  After, slot
 * slot0 + i holds the sequence slot slot0 + parents[i] held: the same context length, pending token tokens[i].  One child of every
 * chosen parent inherits the parent's block-table row, private tail page included, as tl_engine_move does; every further child shares
 * the full pages by reference count and gets a copy of a partial tail page (one tl_kv_copy_rows launch per copy), as tl_engine_fork
 * does.  A parent nobody chose lets go of its pages as tl_engine_release does; sources at index >= width are released.  No spare slot
 * is needed.  All or nothing: the pages the copies need -- the further children of parents whose tail page is partial -- are compared
 * with the obtainable pages (free plus evictable) before anything changes; pages the unchosen parents would give back are NOT counted.
 * Failure is TL_ERR_INVALID "KV page pool exhausted" with every slot as it was; pages_in_use + pages_free + retained pages == num_pages
 * at every return.  The prefix-cache record and the LoRA adapter travel with the parent (moved to the inheriting child, copied to the
 * others); the token ring and `produced` restart as after a fork -- the caller holds the hypotheses' ids.  Stream work, does not
 * synchronise: stream order protects the tail copies. */
#define TL_MAX_BEAMS 8
#define TL_MAX_BEAM_CANDIDATES 32
typedef struct tl_beam_candidate { /* 16 bytes */
    int32_t parent; /* row of the call (beam of the group); -1: no candidate */
    int32_t token;
    float score;   /* scores[parent] + logprob */
    float logprob; /* of `token` in the parent's row */
} tl_beam_candidate;
int tl_beam_rows(const void *logits_dev, int rows, int vocab, const float *scores_dev, int n_cand, tl_beam_candidate *out_dev, void *stream);
int tl_engine_beam_select(tl_engine *e, int row0, int rows, const float *scores_host, int n_cand, tl_beam_candidate *out_host);
int tl_engine_beam_reorder(tl_engine *e, int slot0, int n_src, int width, const int *parents, const int32_t *tokens);

/* Run `steps` decode steps over the live slots [0, batch): each step feeds every
 * slot's pending token at position context_len, appends K/V, and leaves the next
 * token as the next pending token: the argmax, or, for a slot with a nonzero
 * temperature (tl_engine_set_sampling), the token drawn by the per-slot sampler on
 * the device.  A step in which some live slot samples ends with the sampling twin
 * of the step-end launch (its own captured plan; greedy slots inside it keep the
 * argmax and its tie rule); otherwise the step is the greedy program unchanged.  Generated ids are appended to an
 * on-device ring [capacity, max_batch] readable via tl_engine_read_tokens.
 * The step is captured in a hipGraph on first use (re-captured when the
 * attention split bucket or batch changes); use_graph = 0 launches eagerly.
 * Pages are reserved on demand (TL_ERR_INVALID if the pool is exhausted).
 * Synchronisation depends on the replay route (tl_engine_replay_route): on the
 * default "aql" route the call waits for the stream before its first captured
 * step and RETURNS DRAINED -- every step of the call has run (the engine's HSA
 * queue is not the stream, so nothing stream-ordered may follow undrained steps;
 * the host waits ~50 us spinning, then blocked on the completion signal).  On the
 * "hipgraph" route (TL_AQL=0, or a plan the AQL route does not take) and with
 * use_graph = 0 the call only enqueues on the engine stream and does not
 * synchronise: a caller that overlaps host work with decode steps (a draft
 * model free-running beside its target) wants that route.  A call in which a
 * running slot is armed with stop conditions (tl_engine_set_stop) RETURNS
 * SYNCHRONISED on every route: it reads the stop records before it returns.
 * Must be called with the engine's own device current (the one current at
 * tl_engine_create): anything else is TL_ERR_INVALID. */
int tl_engine_decode(tl_engine *e, int batch, int steps, int use_graph);

/* Copy the ids produced by the last `count` decode steps for `slot` to host
 * (synchronises the stream). */
int tl_engine_read_tokens(tl_engine *e, int slot, int count, int32_t *out);

/* Pending token ids of slots [0, count) to host memory, after synchronising the stream. */
int tl_engine_read_pending(tl_engine *e, int count, int32_t *out);

/* Device pointer to the most recent logits, [rows, vocab] bf16 (decode: rows =
 * batch of the last step; prefill with want_logits: 1 row). */
const void *tl_engine_logits_dev(const tl_engine *e);
/* Stream-ordered device-to-device copy of the first `rows` logits rows into dst_dev ([rows, vocab] bf16). */
int tl_engine_copy_logits(tl_engine *e, void *dst_dev, int rows);
/* The same for the PROCESSED rows of the last decode step in which some live slot processed its logits (penalties, bias, grammar): row
 * i is what slot i's token was chosen from; the row of a slot that does not process is its raw row.  TL_ERR_INVALID before any slot of
 * the engine has processed. */
int tl_engine_copy_processed_logits(tl_engine *e, void *dst_dev, int rows);
/* Device pointer to the pending token ids [max_batch] int32. */
const int32_t *tl_engine_tokens_dev(const tl_engine *e);

int tl_engine_get_stats(const tl_engine *e, tl_engine_stats *out);

/* How captured decode steps are replayed: "aql" -- hand-written AQL dispatch packets on the engine's own HSA queue, no cache
 * maintenance between the launches of a step (the default; csrc/aql.h) -- or "hipgraph: <why the AQL route is not available>"
 * (hipGraphLaunch; also TL_AQL=0).  The string lives until the calling thread's next call. */
const char *tl_engine_replay_route(const tl_engine *e);

/* Algorithmic HBM bytes of ONE decode step at the current state: all W4 weights
 * streamed once + K/V of every live context. */
size_t tl_engine_step_bytes(const tl_engine *e, int batch);

/* Measurement aid: runs ONE real decode step eagerly (same kernels, same state update as
 * tl_engine_decode(e, batch, 1, 0)) with every kernel stamping the device wall clock at its first
 * workgroup's start and its last wave's end.  kernel_us[k] / launches[k] are summed per kind:
 *   0 qkv GEMV, 1 wo GEMV, 2 gate|up GEMV, 3 w_down GEMV, 4 lm_head GEMV, 5 attention, 6 attention merge,
 *   7 step end (argmax + embed; with a processing slot also the logit-processing launch ahead of it).
 * gemv_bytes[k] = algorithmic W4 bytes those launches stream (packed nibbles + bf16 scales and biases).
 * span_us = first start to last end of the step (includes the small reduce kernels this mode inserts
 * between launches, so it is NOT the production step time).  Synchronises the stream.  Like tl_engine_decode it must be called
 * with the engine's own device current (TL_ERR_INVALID otherwise). */
typedef struct tl_step_profile {
    double kernel_us[8];
    int launches[8];
    double gemv_bytes[5];
    double span_us;
    int clock_khz;
    int n_splits;
} tl_step_profile;
int tl_engine_profile_step(tl_engine *e, int batch, tl_step_profile *out);

/* Test aid for the AQL replay route's invariant (csrc/aql.h: inside a replayed step no cache is written back or invalidated between
 * the launches, which is correct because every address one launch hands to a later launch of the step is WRITTEN ONCE PER STEP and
 * read only after it).  Runs ONE real decode step eagerly -- the kernels and the state update of tl_engine_decode(e, batch, 1, 0) --
 * with the per-layer hand-over buffers poisoned (every element a NaN) at the start and a checker behind every launch that compares
 * the hand-over regions (the shared activations of the arena; the per-layer buffers) with a shadow copy, element by 2-byte element:
 *   double_writes      elements a launch changed that an earlier launch of the step had already written (0 = the invariant holds for
 *                      this plan); first_launch / first_kind (tl_step_profile's kinds) / first_region (0 shared, 1 per-layer) /
 *                      first_offset (element index inside the region) name one offence of the earliest offending launch;
 *   written_once_plan  1 when the plan uses the per-layer buffers throughout -- the only plans the engine replays as AQL packets;
 *   a value read before the step wrote it is a NaN: the caller checks the logits (finite, and equal to an unchecked engine's).
 * A rewrite of an element with the value it already holds is not seen (and cannot be read stale).  Synchronises.  Like
 * tl_engine_decode it must be called with the engine's own device current (TL_ERR_INVALID otherwise), and it returns the status of
 * the stop reconciliation behind the step. */
typedef struct tl_step_check {
    int launches, written_once_plan, n_splits;
    long double_writes, elements_written;
    int first_launch, first_kind, first_region;
    long first_offset;
} tl_step_check;
int tl_engine_check_step(tl_engine *e, int batch, tl_step_check *out);

/* ===== kernel-level entry points of the decode path ===========================================
 * The launch code the engine runs per projection and per layer, on caller-owned device buffers: what the operator
 * microbenches time (reference benches/bench_week2_operators.py:355-358, bench_week3_attention.py:74-77) and what the
 * parity tests drive at the real Qwen3-4B shapes (tests/test_decode_kernels_gpu.py).  Not used by the engine itself. */

/* A W4 matrix re-packed into the decode layout ([rows/16][cols/128][64 lanes][4 words], csrc/qmv3.h).  `w` stays
 * borrowed (the packed-dot fallback reads the checkpoint layout); rows % 16 == 0, cols % 128 == 0.  Stream ordered. */
typedef struct tl_tiled_w4 tl_tiled_w4;
int tl_tiled_w4_create(const tl_w4 *w, void *stream, tl_tiled_w4 **out);
void tl_tiled_w4_destroy(tl_tiled_w4 *t);

/* Which kernel a projection ran: 1 = fused MFMA GEMV (qmv3: p = MR, KS, CW, LM, workgroups), 2 = skinny MFMA matmul +
 * slice reduction (qmm3: p = MB, TW, LM, slices, tile groups), 3 = packed-dot GEMV fallback, 4 = prefill GEMM path,
 * 5 = register-resident batched matmul (qmm6: p = MB, groups per wave, weight sets, row blocks, workgroups),
 * 6 = row-streaming batched matmul (qmm7: p = MB, groups per wave, tiles per workgroup, row blocks, workgroups). */
typedef struct tl_linear_info {
    int kernel;
    int launches;
    int rows_per_pass; /* activation rows per launch (the GEMV splits M when the staged rows exceed LDS) */
    int p[5]; /* GEMV: MR, KS, CW, LM, workgroups.  Skinny matmul: MB (16-row blocks), TW (tiles per wave; 0 = the persistent
                 grid, one workgroup per CU), LM (groups per slice), slices, workgroups */
} tl_linear_info;

/* out = epilogue(prologue(a) @ W^T) over M (1..64) bf16 rows, exactly as one projection of a decode step:
 *   prologue 0 none | 1 RMSNorm(a, norm_w, eps) rounded to bf16;  epilogue 0 store | 1 residual + bf16(acc) |
 *   2 SwiGLU over interleaved (gate_i, up_i) rows -> out [M, rows/2].
 *   kernel 0 = the routing of a single projection by M and matrix size, 1 = force the fused GEMV (M <= 8), 2 = force the skinny matmul
 *   (grid chosen by shape as the engine does), 3 / 4 = the skinny matmul on its one-shot / persistent grid, 5 = the register-resident
 *   matmul of a batched decode step (csrc/qmm6.h; prologue 0, or 3 through tl_decode_linear_ex), 6 = the row-streaming matmul
 *   (csrc/qmm7.h; prologue 3 with epilogue 0 or 2 through tl_decode_linear_ex -- bit-identical to kernel 5 on the same inputs).
 * The engine uses the pairs (1,0) qkv / lm_head, (0,1) wo / w_down, (1,2) gate|up, (0,0) -- and at 5..64 rows, through kernel 5,
 * (3,0) qkv / lm_head, (0,1) + ss_out + out_w for wo / w_down, (3,2) gate|up: rows travel weighted between the projections. */
size_t tl_decode_linear_workspace_bytes(int M, int rows, int cols);
int tl_decode_linear(const tl_tiled_w4 *w, const void *a_dev, void *out_dev, int M, int prologue, int epilogue,
                     const void *norm_w_dev, const void *residual_dev, float eps, int kernel, void *workspace_dev,
                     size_t workspace_bytes, void *stream, tl_linear_info *info);

/* The routes of the fused GEMV that only a whole engine step reached before round 4 -- the kernels BASELINE configs[1] times
 * (csrc/qmv3.h): the wo projection of ONE row forming its input row from the decode-attention split partials, the gate|up
 * projection over rows its producer left weighted, and the producer / consumer hand-over of RMSNorm sums of squares.  The
 * reference tests its matvec per shape against the dequantised product (tests_refsol/test_week_2_day_3.py:89-118); these
 * entry points let tests/test_decode_kernels_gpu.py do the same for exactly those instantiations.
 *   prologue 2 (with epilogue 1, M = 1, kernel 1): `a_dev` is not read; the activation row is the merge of
 *     merge_ws_dev [cols / 128 heads][n_splits][128 + 4] fp32 (128 value sums, running max in log2 units, running sum, 2 pad;
 *     n_splits 2 / 4 / 8): per column  bf16(sum_s v_s 2^(m_s - max m) / sum_s l_s 2^(m_s - max m)),  zero where the sum is zero.
 *   prologue 3 (with epilogue 2, M <= 8, kernel 1): a_dev holds bf16(x * norm_weight) (what a producer's out_w_dev holds) and
 *     ss_in_dev the sums of squares of x; out = SwiGLU(bf16(rsqrt(mean x^2 + eps) * (a @ W^T))).
 *   ss_in_dev [M][ss_in_n] (prologues 1 and 3): partial sums of squares of each row, added instead of re-derived (the GEMV: any
 *     multiple of 4 up to 256 partials, and so does the skinny matmul).
 *   epilogue 1 through the GEMV: ss_out_dev [M][rows / 16] receives the sum of squares of every 16 stored bf16 outputs;
 *     norm_out_dev [rows] + out_w_dev [M][rows]: also store bf16(out * norm_out).
 *   kernel 5 (M <= 64): prologue 3 with epilogue 0 or 2 (ss_in_dev required), prologue 0 with epilogue 0 or 1; epilogue 1 takes
 *     ss_out_dev / norm_out_dev + out_w_dev as above. */
typedef struct tl_linear_ex {
    const float *merge_ws_dev;
    int n_splits;
    const float *ss_in_dev;
    int ss_in_n;
    float *ss_out_dev;
    const void *norm_out_dev;
    void *out_w_dev;
    int fragment_order; /* kernels 2-5: the weighted rows on either side -- a_dev with prologue 3 (kernel 5), out_w_dev -- lie in the
                           batched step's FRAGMENT ORDER instead of row-major: [16-row block][128-column group][k-step t 0..3]
                           [lane = r + 16 c][8 elements] = row 16 block + r, columns 128 g + 32 c + 8 t .. + 7 (rows padded to 16: out_w_dev
                           holds ceil16(M) x rows elements).  The engine hands its rows over that way (every load of the consumer is one
                           contiguous 1 KiB). */
} tl_linear_ex;
int tl_decode_linear_ex(const tl_tiled_w4 *w, const void *a_dev, void *out_dev, int M, int prologue, int epilogue,
                        const void *norm_w_dev, const void *residual_dev, float eps, int kernel, void *workspace_dev,
                        size_t workspace_bytes, void *stream, const tl_linear_ex *ex, tl_linear_info *info);

/* The prefill projection of LARGE chunks (csrc/gemm8.h; the engine takes it from 1,792 rows): the reference's tile GEMM rounds the dequantised
 * weights to bf16 before the product (quantized_matmul.metal:96-249), so the weights are expanded ONCE --
 *   tl_prefill_weights_bf16: out_dev [rows, cols] bf16 = bf16(q * scale + bias) per element --
 * and the product is a plain bf16 GEMM with fp32 accumulation over the whole reduction (the unsplit tile kernel's arithmetic),
 *   tl_prefill_matmul_bf16: out [M, rows] = epilogue(a [M, cols] @ w_bf16^T); epilogue 0 store | 1 residual + bf16(acc) | 2 SwiGLU over
 *   interleaved (gate_i, up_i) weight rows -> out [M, rows / 2]; cols a multiple of 64, rows even.  Stream ordered. */
int tl_prefill_weights_bf16(const tl_w4 *w, void *out_dev, void *stream);
int tl_prefill_matmul_bf16(const void *a_dev, const void *w_bf16_dev, void *out_dev, int M, int rows, int cols, int epilogue,
                           const void *residual_dev, void *stream);

/* The attention launch of one decode layer: q/k-RMSNorm + RoPE at position context_lens[b] + append of the new K/V row to
 * the pages (IN PLACE) + GQA attention over context_lens[b] + 1 tokens (+ the merge launch when the context is split).
 *   qkv [batch, (Hq + 2 Hkv) D] bf16, pages [P, Hkv, page_size, D] bf16, block_table [batch, max_pages] int32,
 *   context_lens [batch] int32 (tokens already cached), out [batch, Hq D] bf16.
 * max_context: host upper bound of context_lens (sizes the context split exactly as tl_engine_decode does). */
/* Host-only (no device, no launch): the plans the decode path picks.  tl_decode_gemv_plan: MFMA GEMV of M rows against a
 * [rows, cols] W4 matrix -> out5 = {activation rows per workgroup, reduction split, waves, groups per wave, workgroups}; returns 1
 * when the MFMA GEMV takes the shape (0: the packed-dot GEMV would).  tl_decode_attention_plan: `batch` sequences whose longest
 * holds max_context tokens before this step -> out3 = {windows per sequence, tokens per window, query heads per workgroup}, at head size
 * 128 on 128-token pages. */
int tl_decode_gemv_plan(int M, int rows, int cols, int *out5);
/* 1 when the library holds a fused-GEMV kernel for (rows per workgroup, reduction split, waves, groups per wave): a plan is only
 * ever "taken" (tl_decode_gemv_plan returns 1) for such a combination; anything else decodes through the packed-dot GEMV. */
int tl_decode_gemv_variant_compiled(int MR, int KS, int CW, int LM);
/* The register-resident matmul of a batched decode step (csrc/qmm6.h): M rows against [rows, cols] -> out6 = {16-row blocks per
 * workgroup, quantisation groups per wave, weight sets, row blocks, workgroups per row block, tiles per workgroup}; returns 1 when
 * the kernel takes the shape.  tl_decode_batched_variant_compiled: 1 when the library holds a kernel for (row blocks, groups per wave). */
int tl_decode_batched_plan(int M, int rows, int cols, int *out6);
int tl_decode_batched_variant_compiled(int MB, int GPW);
/* The row-streaming matmul of a batched decode step (csrc/qmm7.h; gate|up and qkv where its plan exists): M rows against [rows, cols]
 * -> out4 = {16-row blocks, tiles per workgroup, quantisation groups per wave, workgroups}; returns 1 when the kernel takes the shape.
 * tl_decode_streaming_variant_compiled: 1 when the library holds the kernels for (tiles per workgroup, groups per wave) -- each pair
 * exists for 1 .. 4 row blocks and the store / SwiGLU epilogues. */
int tl_decode_streaming_plan(int M, int rows, int cols, int *out4);
int tl_decode_streaming_variant_compiled(int T, int GPW);
int tl_decode_attention_plan(int batch, int max_context, int num_heads, int num_kv_heads, int *out3);

typedef struct tl_attention_info {
    int n_splits, tokens_per_split, heads_per_workgroup;
    int launches;
} tl_attention_info;
size_t tl_decode_attention_fused_workspace_bytes(int batch, int num_heads, int head_dim);
int tl_decode_attention_fused(const void *qkv_dev, const void *q_norm_dev, const void *k_norm_dev, void *key_pages_dev,
                              void *value_pages_dev, const int32_t *block_table_dev, const int32_t *context_lens_dev,
                              void *out_dev, int batch, int num_heads, int num_kv_heads, int head_dim, int page_size,
                              int max_pages, float rope_theta, float eps, int max_context, void *workspace_dev,
                              size_t workspace_bytes, void *stream, tl_attention_info *info);
/* ... over FP8 (E4M3) pages: key_pages / value_pages [P, Hkv, page, 128] uint8 + key_scales / value_scales [P, Hkv, page] float32
 * (tl_engine_create_kv, include/tinyllm_hip.h "FP8 KV pages"); the appended row is quantised, head_dim 128 */
int tl_decode_attention_fused_fp8(const void *qkv_dev, const void *q_norm_dev, const void *k_norm_dev, void *key_pages_dev,
                                  float *key_scales_dev, void *value_pages_dev, float *value_scales_dev,
                                  const int32_t *block_table_dev, const int32_t *context_lens_dev, void *out_dev, int batch,
                                  int num_heads, int num_kv_heads, int head_dim, int page_size, int max_pages, float rope_theta,
                                  float eps, int max_context, void *workspace_dev, size_t workspace_bytes, void *stream,
                                  tl_attention_info *info);

/* The device sampler of tl_engine_set_sampling over caller rows: logits [rows, vocab] bf16 (vocab <= 524,288), per-row device arrays
 * temperature (float; 0 = greedy), top_k (int32), top_p (float), seed (uint64) and position (int32) -> ids_dev [rows] int32.  One
 * 1,024-thread workgroup per row, the engine's routine and semantics.  Stream ordered. */
int tl_sample_logits(const void *logits_dev, int rows, int vocab, const float *temperature_dev, const int32_t *top_k_dev,
                     const float *top_p_dev, const uint64_t *seed_dev, const int32_t *position_dev, int32_t *ids_dev, void *stream);

/* Speculative sampling over caller rows (csrc/spec_sample.h): row i holds a target logits row and the draft logits row its proposal was
 * drawn from, each [vocab] bf16 (vocab <= 524,288), and per-row device arrays: proposal (int32), the target's temperature / top_k / top_p
 * and the draft's, seed (uint64) and position (int32).  Kept set and weights are tl_engine_set_sampling's, applied to each row with its
 * own parameters: wp, Wp = sum wp (fp32) for the target, wq, Wq for the draft; a row with temperature 0, without a finite maximum or
 * holding +inf is one-hot (w = W = 1) at the id tl_sample_logits gives it.  Uniforms as the sampler's with the third counter word
 * 0x53504143 (u_acc) and 0x53505253 (u_res).
 *   proposal < 0   a bonus row: accept 0, alt = exactly what tl_sample_logits returns for the target row;
 *   proposal >= V  rejected without a read at it;
 *   accept         iff u_acc wq_x Wp < wp_x Wq in fp32, no division; alt = -1;
 *   reject         r_j = max(wp_j Wq - wq_j Wp, 0), R = sum r: alt = the first id in ascending order whose inclusive cumulative r exceeds
 *                  u_res R (rounding leaving none: the last id with r > 0; R == 0: the inverse-CDF draw from wp with u_res).
 * -> accept_dev, alt_dev [rows] int32.  Rows are independent; the caller picks the first rejection.  One 1,024-thread workgroup per row.
 * Stream ordered. */
int tl_spec_sample_rows(const void *target_logits_dev, const void *draft_logits_dev, int rows, int vocab, const int32_t *proposal_dev,
                        const float *temperature_dev, const int32_t *top_k_dev, const float *top_p_dev, const float *draft_temperature_dev,
                        const int32_t *draft_top_k_dev, const float *draft_top_p_dev, const uint64_t *seed_dev, const int32_t *position_dev,
                        int32_t *accept_dev, int32_t *alt_dev, void *stream);

/* The log-probability routine of tl_engine_set_logprobs over caller rows: logits [rows, vocab] bf16 (vocab <= 524,288); ids_dev [rows]
 * int32 (may be NULL: each row's greedy id, the first maximum; an id < 0 gives NaN) -> logprob_dev [rows] float; top_n 0 .. 20 ->
 * top_ids_dev / top_logprobs_dev [rows, top_n] (may be NULL when top_n is 0).  One 1,024-thread workgroup per row.  Stream ordered. */
int tl_logprob_rows(const void *logits_dev, int rows, int vocab, const int32_t *ids_dev, int top_n, float *logprob_dev, int32_t *top_ids_dev,
                    float *top_logprobs_dev, void *stream);

/* The pooling routine of tl_engine_embed over caller rows: rows_dev [total, hidden] bf16 (hidden even, 4-byte aligned), already final-normalised;
 * n_seqs (1 .. 16) sequences, sequence i the rows [row0[i], row0[i] + len[i]) (host arrays; the caller vouches for the rows).
 * TL_POOL_MEAN: the chunk's column sums join sums_dev [n_seqs, hidden] fp32, row i of it -- replacing it when prior[i] (the rows it
 * already holds, a host array) is 0; TL_POOL_LAST ignores prior and sums_dev (both may be NULL).  A sequence with finish[i] != 0 writes
 * its vector -- `dim` (1 .. hidden) components, divided by their norm when normalize != 0 -- to the next `dim` floats of out_dev, in
 * order.  Stream ordered. */
int tl_pool_rows(const void *rows_dev, int hidden, int n_seqs, const int *row0, const int *len, const int *finish, const int *prior, int pooling,
                 float *sums_dev, int normalize, int dim, float *out_dev, void *stream);

/* The router of a MoE layer (tl_engine_set_moe_layer) over caller rows: logits_dev [rows, num_experts] bf16, the router's logits ->
 * ids_dev [rows, top_k] int32 and scores_dev [rows, top_k] bf16.  Per row: softmax over the num_experts logits in fp32, each probability
 * rounded to bf16; the top_k largest in descending order, equal probabilities the lower expert index first; the scores are those
 * probabilities -- with norm_topk_prob != 0 divided by their sum (the fp32 sum in selection order rounded to bf16, each quotient rounded
 * once).  A row with NaN / Inf logits still gets top_k distinct ids in [0, num_experts); its scores are unspecified.  The limits of
 * tl_engine_set_moe_layer: 1 <= top_k <= min(16, num_experts), num_experts <= 1024; rows >= 1.  One launch of `rows` workgroups, the
 * engine's kernel.  Stream ordered, no synchronisation. */
int tl_moe_route_rows(const void *logits_dev, int rows, int num_experts, int top_k, int norm_topk_prob, int32_t *ids_dev, void *scores_dev,
                      void *stream);

/* Everything of a MoE layer's MLP behind the router, over caller rows, in the engine's five launches: xn_dev [rows, hidden] bf16 (the
 * normalised rows the experts read), h_dev [rows, hidden] bf16 (the residual), ids_dev / scores_dev [rows, top_k] (int32 in
 * [0, num_experts) -- the caller vouches for them -- and bf16; top_k = w->experts_per_token) -> out_dev [rows, hidden] bf16:
 *   gate, up [rows * top_k, I] = xn[token] x gate / up of the row's expert (one grouped GEMV launch each);  act = bf16(bf16(silu(gate)) * up);
 *   y [rows * top_k, hidden] = act x down of the row's expert;  out = bf16(h + bf16(sum_j bf16(y_j * score_j))), the sum over the token's
 *   top_k rows in fp32, in the order of its ids, rounded once.
 * Expert rows are token-major.  workspace_dev holds them for the caller to read, without gaps and in this order: gate, up, act
 * [rows * top_k, I], then y [rows * top_k, hidden] -- tl_moe_experts_workspace_bytes(rows, top_k, hidden, intermediate) bytes (0 for a
 * size that is not positive).  Of *w the expert tensors and the three sizes are read; router and norm_topk_prob are not.  Limits:
 * those of tl_engine_set_moe_layer, hidden a multiple of 128, 1 <= rows * top_k <= 65,535, every row pointer 16-byte aligned.
 * Stream ordered, no synchronisation. */
size_t tl_moe_experts_workspace_bytes(int rows, int top_k, int hidden, int intermediate);
int tl_moe_experts_rows(const void *xn_dev, const void *h_dev, const int32_t *ids_dev, const void *scores_dev, const tl_moe_weights *w, int rows,
                        int hidden, void *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* The truncation routine of tl_engine_set_truncation / tl_engine_set_mirostat over caller rows: logits [rows, vocab] bf16 (vocab <=
 * 524,288), per-row device arrays of temperature, min_p, typical_p and mu (NaN = no Mirostat; a Mirostat row ignores min_p and
 * typical_p), filtered rows into out_dev (never the input) and, where kept_logsum_dev is not null, per row ln sum_kept exp(x_i / T) of a
 * Mirostat row (NaN for any other).  tl_mirostat_update_rows: the update for the tokens ids_dev[rows] chosen from the filtered rows,
 * mu_dev[rows] in place; a row with tau 0, temperature 0, an id outside the vocabulary or a surprise that is not finite keeps its mu.
 * Stream ordered, no synchronisation. */
int tl_truncate_rows(const void *logits_dev, int rows, int vocab, const float *temperature_dev, const float *min_p_dev, const float *typical_p_dev,
                     const float *mu_dev, void *out_dev, float *kept_logsum_dev, void *stream);
int tl_mirostat_update_rows(const void *filtered_dev, int rows, int vocab, const int32_t *ids_dev, const float *temperature_dev,
                            const float *kept_logsum_dev, const float *tau_dev, const float *eta_dev, float *mu_dev, void *stream);

/* The processing routine of tl_engine_set_penalties / tl_engine_set_logit_bias over caller rows: logits [rows, vocab] bf16 (vocab <=
 * 524,288) -> out_dev [rows, vocab] bf16, the engine's kernel and semantics, nothing counted.  history_dev [rows, vocab]: one uint16 per
 * (row, token), bit 15 = prompt, bits 0-14 = count (saturated at 32,767).  repetition / presence / frequency [rows]; bias_n_dev [rows]
 * entries of each row's list in bias_ids_dev / bias_values_dev [rows, TL_MAX_LOGIT_BIAS] (distinct ids in [0, vocab); both may be NULL
 * when every n is 0).  A row whose parameters are all neutral and whose list is empty is copied bit for bit.  One launch of
 * ceil(vocab / 2,048) x rows workgroups.  Stream ordered. */
int tl_process_logits(const void *logits_dev, int rows, int vocab, const uint16_t *history_dev, const float *repetition_dev,
                      const float *presence_dev, const float *frequency_dev, const int32_t *bias_ids_dev, const float *bias_values_dev,
                      const int32_t *bias_n_dev, void *out_dev, void *stream);

/* The two launches of tl_engine_set_dry over caller rows: sequences_dev [rows, cap] int32 (row r holds S[start[r] .. end[r]], end[r] < cap;
 * a row with end < start is left alone), the per-row parameters [rows] (a row with multiplier 0 and no_repeat_ngram 0 is left alone),
 * breaker_ids_dev [rows, TL_MAX_DRY_BREAKERS] with n_breakers_dev [rows] entries each (the list may be NULL when every count is 0),
 * table_dev [rows, vocab] uint32, all zeros before the call and all zeros after it, and logits_dev [rows, vocab] bf16 (vocab <= 524,288),
 * rewritten in place.  The engine's kernels and semantics; nothing is stored to the sequences.  One launch of `rows` workgroups and one of
 * ceil(vocab / 2,048) x rows.  Stream ordered. */
int tl_dry_rows(int32_t *sequences_dev, int rows, int cap, const int32_t *start_dev, const int32_t *end_dev, const float *multiplier_dev,
                const float *base_dev, const int32_t *allowed_length_dev, const int32_t *range_dev, const int32_t *no_repeat_ngram_dev,
                const int32_t *breaker_ids_dev, const int32_t *n_breakers_dev, uint32_t *table_dev, void *logits_dev, int vocab, void *stream);

/* The prompt-lookup rule of tl_engine_lookup_propose over caller rows: sequences_dev [rows, cap] int32 (cap <= 16,777,216; row r holds
 * T[start[r] .. end[r]], end[r] < cap; a row with end < start has no proposals), max_ngram 1 .. 16, min_ngram 1 .. max_ngram,
 * num_proposals 1 .. 7 -> proposals_dev [rows, 8] (the proposals, -1 behind them), counts_dev [rows] and, where match_dev is not NULL,
 * match_dev [rows, 2]: the chosen position i and raw(i), (-1, 0) without a choice.  Ids outside [start, end] are never read as data.
 * One launch of `rows` workgroups; nothing is stored to the rows.  Stream ordered. */
int tl_lookup_rows(const int32_t *sequences_dev, int rows, int cap, const int32_t *start_dev, const int32_t *end_dev, int max_ngram, int min_ngram,
                   int num_proposals, int32_t *proposals_dev, int32_t *counts_dev, int32_t *match_dev, void *stream);

/* The attention stage of tl_engine_verify_batch over caller pools (csrc/verify_attn.h): qkv_dev [R, (Hq + 2 Hkv) * 128] bf16, the rows
 * of n_seqs (1 .. 64) sequences back to back; sequence i (host arrays) holds lens[i] (1 .. 8) rows at positions starts[i] .. of
 * block-table row slots[i] (R = sum of lens <= 64).  Per-head RMSNorm of q and k, RoPE, K and V appended to the pages the block table
 * names (key_scales_dev / value_scales_dev not NULL: FP8 pages, kv8.h; NULL: bf16), then row j of sequence i attends to its first
 * starts[i] + j + 1 tokens -> out_dev [R, Hq * 128] bf16, row-major.  head_dim 128.  The workspace is internal; *info (may be NULL)
 * reports the split plan used.  Stream ordered (returns after the stream has run the stage); bad input is TL_ERR_INVALID. */
int tl_verify_attention_rows(const void *qkv_dev, const void *q_norm_dev, const void *k_norm_dev, void *key_pages_dev, void *value_pages_dev,
                             float *key_scales_dev, float *value_scales_dev, const int32_t *block_table_dev, int n_seqs, const int *slots,
                             const int *starts, const int *lens, void *out_dev, int num_heads, int num_kv_heads, int page_size, int max_pages,
                             float rope_theta, float eps, void *stream, tl_attention_info *info);
/* The acceptance stage over caller rows: logits_dev [R, vocab] bf16; sequence i (host arrays) owns the rows [row0[i], row0[i] + lens[i]),
 * lens[i] 1 .. 8, every row below 64; tokens_dev [R] int32 the tokens the rows were fed -> out_dev [n_seqs] as tl_engine_verify_batch
 * defines them.  Stream ordered (returns after the stream has run it); bad input is TL_ERR_INVALID. */
int tl_verify_accept_rows(const void *logits_dev, int vocab, int n_seqs, const int *row0, const int *lens, const int32_t *tokens_dev,
                          tl_verify_result *out_dev, void *stream);
/* The acceptance stage of tl_engine_verify_batch_sampled over caller rows (csrc/verify_sample.h): target_logits_dev [R, vocab] bf16
 * (vocab <= 524,288); draft_logits_dev [R, vocab] (drafted proposals) or NULL (point proposals); sequence i (host arrays) owns the rows
 * [row0[i], row0[i] + lens[i]) and held starts[i] tokens before them; tokens_dev [R] int32 the tokens the rows were fed; the target's
 * temperature_dev / top_k_dev / top_p_dev / seed_dev hold one value per SEQUENCE, at i; one draft triple for the call.  -> out_dev
 * [n_seqs] as tl_engine_verify_batch_sampled defines them and, where not NULL, accept_dev / alt_dev [R] int32: every row's own decision
 * (alt -1 where accepted; a row no sequence owns: 0, -1).  Sequences are checked as tl_verify_accept_rows checks them.  Stream ordered
 * (returns after the stream has run it); bad input is TL_ERR_INVALID. */
int tl_verify_sample_rows(const void *target_logits_dev, const void *draft_logits_dev, int vocab, int n_seqs, const int *row0, const int *lens,
                          const int *starts, const int32_t *tokens_dev, const float *temperature_dev, const int32_t *top_k_dev,
                          const float *top_p_dev, const uint64_t *seed_dev, float draft_temperature, int draft_top_k, float draft_top_p,
                          int32_t *accept_dev, int32_t *alt_dev, tl_verify_result *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TINYLLM_ENGINE_H */
