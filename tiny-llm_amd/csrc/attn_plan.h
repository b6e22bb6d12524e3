// The plan of one decode-attention launch (host only: no HIP, no project include; tests/attention_plan_check.cpp compiles it with plain
// g++): the context split, the kernel that walks it, its grid and LDS bytes, and what merges the split partials -- everything a launch
// needs that is known before it.  decode_attention.h launches a plan; the engine, the operator entry points and the CPU tests ask the
// same function.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace tl {

constexpr int AD_RQ = 4;  // most query heads of one GQA group handled per workgroup
// row of split partials in global memory: D value sums + (max, sum) + 2 floats of padding, so that rows start on 16 bytes (the wo GEMV
// that merges them reads them with 16-byte loads); the LDS rows inside the kernels keep D + 2
constexpr int ATTN_WS_PAD = 4;
// dynamic LDS of the matrix-core walk ahead of its staged qkv rows (attn_mfma.h AM_OFF_QP, held equal there)
constexpr int ATTN_MFMA_LDS = 46240;

struct AttnGeometry {
    int num_heads = 0, num_kv_heads = 0, head_dim = 0, page_size = 0, max_pages = 0;
};

// the attention plan's lab knobs (environment, read when an engine -- or an operator entry point's context -- is set up)
struct AttnKnobs {
    int rq = 0;                   // query heads per decode-attention workgroup; 0 = by context (TL_ATTN_RQ at create: 1 or 4)
    int min_tokens = 64;          // tokens per attention workgroup before the context is split (TL_ATTN_MIN_TOKENS)
    bool min_tokens_auto = true;  // ... or more, by context and sequences (pick_decode_splits)
    int max_splits = 64;          // most context splits per sequence (TL_ATTN_MAX_SPLITS, a power of two <= 256)
    int max_splits_gqa = 32;      // ... when a workgroup takes a whole GQA group (TL_ATTN_MAX_SPLITS sets both)
    bool mfma = true;             // TL_ATTN_MFMA=0: the GQA-group walk on the VALU (attn_decode_fused_kernel), the A/B twin of attn_mfma.h
    // At 5 .. 64 decode rows the qkv projection's slice reduction is not launched; the decode-attention kernel adds the fp32 slice
    // partials itself (engine_kernels.h, QP).  Measured in round 3 (profiles/r03_labs/batched_decode_status.jsonl): 5 / 8 / 16 / 64
    // sequences 1.87 -> 1.81, 1.91 -> 1.89, 2.08 -> 2.03, 3.63 -> 3.52 ms per step.  tl_engine_set_option "attn_qkv_partials" = 0 launches the reduction.
    bool qkv_partials = true;
    void read_env() {
        if (const char *q = getenv("TL_ATTN_MFMA")) mfma = atoi(q) != 0;
        if (const char *q = getenv("TL_ATTN_RQ")) rq = atoi(q) <= 0 ? 0 : (atoi(q) == 1 ? 1 : AD_RQ);
        if (const char *q = getenv("TL_ATTN_MAX_SPLITS")) max_splits = max_splits_gqa = std::min(256, std::max(1, atoi(q)));
        if (const char *q = getenv("TL_ATTN_MIN_TOKENS")) min_tokens = std::max(64, atoi(q)), min_tokens_auto = false;
    }
};

// bytes of the split partials of `batch` sequences: the one expression every workspace size and every refusal reads
inline size_t attn_partials_bytes(int batch, int num_heads, int n_splits, int head_dim) {
    return (size_t)batch * num_heads * n_splits * (head_dim + ATTN_WS_PAD) * sizeof(float);
}
// what an engine of up to `max_batch` sequences keeps for them: at most 64 splits per row with many sequences, at most 256 split-rows per
// head with few (pick_decode_splits: max_splits <= 64 with the knobs unset)
inline size_t attn_partials_capacity(const AttnGeometry &g, int max_batch) {
    return attn_partials_bytes(1, g.num_heads, std::max(max_batch * 64, 4 * 256), g.head_dim);
}

enum class AttnWalk { MATRIX_CORE, SINGLE_PAGE, STAGE_PAGE, GENERAL };  // attn_mfma.h; attn_decode_fused_kernel<.., SP / IP / neither>
enum class AttnMerge { NONE, M2, M4, M8, COLUMNS };                     // attn_merge_kernel<2 / 4 / 8>, attn_merge_cols_kernel

// Context split of the decode attention: power-of-two bucket >= context, fixed windows of C tokens per workgroup.
struct AttnPlan {
    int n_splits = 1, tokens_per_split = 64;
    int rq = AD_RQ;  // query heads per workgroup
    int row_chunks = 1, rep = 1, split_shift = 0;
    int page_shift = -1;  // log2(page_size), or -1 when the page size is not a power of two
    int num_heads = 0, head_dim = 0;
    unsigned grid[3] = {1, 1, 1};  // (n_splits * row_chunks, KV heads, sequences)
    AttnWalk walk = AttnWalk::GENERAL;
    bool qp = false;   // the kernel adds the qkv projection's fp32 slice planes itself
    bool kv8 = false;  // FP8 pages (kv8.h)
    bool refuses_qkv_partials = false;  // slice partials were offered to a plan that cannot take them: the launch is an error
    size_t lds_bytes = 0;               // dynamic LDS of the walk
    // what merges the windows of a split context: a second launch, or -- NONE with n_splits > 1 -- the wo GEMV of the one row
    AttnMerge merge = AttnMerge::NONE;
    bool wo_merges() const { return n_splits > 1 && merge == AttnMerge::NONE; }
    int launches() const { return merge == AttnMerge::NONE ? 1 : 2; }
    size_t partials_bytes(int batch) const { return attn_partials_bytes(batch, num_heads, n_splits, head_dim); }
    long key() const { return ((long)rq << 40) | ((long)n_splits << 24) | (long)tokens_per_split; }
};

// The (VD = head_dim / 16, RQ, SP, IP, QP, KV8) instantiations of attn_decode_fused_kernel and the (QP, KV8) ones of attn_decode_mfma_kernel,
// written once: the launcher (decode_attention.h, attn_mfma.hip) is generated from these tables and the planner is held to them
// (tests/attention_plan_check.cpp: every plan is an entry, every entry is some plan's).  QP and KV8 exist at head_dim 128 only, QP with
// the whole GQA group.  (The order is the order the kernels have had in the code objects.)
#define ATTN_D128(X, SP, IP)                                                                                     \
    X(8, 4, SP, IP, true, true) X(8, 1, SP, IP, false, true) X(8, 4, SP, IP, false, true) X(8, 4, SP, IP, true, false) \
    X(8, 1, SP, IP, false, false) X(8, 4, SP, IP, false, false)
#define ATTN_PLAIN(X, VD, SP, IP) X(VD, 1, SP, IP, false, false) X(VD, 4, SP, IP, false, false)
#define ATTN_FUSED_TABLE(X)                                                                     \
    ATTN_D128(X, true, false) ATTN_D128(X, false, true) ATTN_D128(X, false, false)               \
    ATTN_PLAIN(X, 4, true, false) ATTN_PLAIN(X, 4, false, true) ATTN_PLAIN(X, 4, false, false)   \
    ATTN_PLAIN(X, 2, true, false) ATTN_PLAIN(X, 2, false, true) ATTN_PLAIN(X, 2, false, false)
#define ATTN_MFMA_TABLE(X) X(true, true) X(true, false) X(false, true) X(false, false)
static_assert(AD_RQ == 4, "the tables name the whole-group walk as RQ = 4");
inline bool attn_plan_has_variant(const AttnPlan &p) {
    if (p.walk == AttnWalk::MATRIX_CORE) {
#define ATTN_MEMBER(QP, KV8) if (p.qp == QP && p.kv8 == KV8) return p.head_dim == 128 && p.rq == AD_RQ;
        ATTN_MFMA_TABLE(ATTN_MEMBER)
#undef ATTN_MEMBER
        return false;
    }
    const bool sp = p.walk == AttnWalk::SINGLE_PAGE, ip = p.walk == AttnWalk::STAGE_PAGE;
#define ATTN_MEMBER(VD, RQ, SP, IP, QP, KV8) if (p.head_dim == 16 * VD && p.rq == RQ && sp == SP && ip == IP && p.qp == QP && p.kv8 == KV8) return true;
    ATTN_FUSED_TABLE(ATTN_MEMBER)
#undef ATTN_MEMBER
    return false;
}

// head_dim 128 with a whole GQA group per workgroup is the only shape that takes qkv slice partials (batched decode of 5+ rows)
inline bool attn_takes_qkv_partials(int head_dim, int rq) { return head_dim == 128 && rq == AD_RQ; }
// the matrix-core walk: head_dim 128, a whole GQA group per workgroup, and a wave's 32 tokens of a stage inside one page
inline bool attn_decode_mfma_applicable(int head_dim, int rq, int page_shift, int tokens_per_split) {
    return head_dim == 128 && rq == AD_RQ && page_shift >= 5 && tokens_per_split % 32 == 0;
}

// Measured on MI355X (profiles/README.md, profiles/r02_labs): a decode-attention workgroup is bound by its dependent latency
// chain and by how many L2 misses ONE CU keeps in flight (~32 KiB), not by chip bandwidth.  Few sequences and short
// contexts: one query head and a 64-token window (32 KiB of K/V) per workgroup, partials merged by the wo GEMV (2 / 4 / 8
// windows of one sequence) or by a second launch.  Many sequences or long contexts: one workgroup per GQA group walking 64-token
// stages, so that the K/V window is read from HBM once.  (A "wide" one-head kernel -- the whole 64..512-token window in one
// workgroup, no merge -- was built in round 2, lost on every context it was meant for (8.2 us per layer against 2.9 + 1.3) and was
// removed in round 3 together with the last-arriver in-kernel merge, which measured neutral.)
constexpr int ATTN_RQ1_CTX = 4096;  // contexts up to this many tokens use one query head per workgroup
constexpr int ATTN_RQ1_BATCH = 2;   // ... and up to this many sequences; at 4 the re-read windows cost 261 vs 180 us
constexpr int ATTN_WG_CAP = 0;      // most attention workgroups per launch; 0 = by sequences (below)
// the split and the grid of a plan; the launch's choices (walk, variant bits, merge) are plan_decode_launch's
inline AttnPlan pick_decode_splits(const AttnGeometry &g, const AttnKnobs &k, int batch, int max_ctx) {
    const int rep = g.num_heads / g.num_kv_heads;
    int rq = k.rq;
    // two sequences re-read twice the windows: the GQA-group walk takes over at a quarter of the context (round 3, 2 sequences at 1,500 tokens
    // one head per workgroup 1.326 against 1.383 ms per step, at 3,000 tokens 1.527 against 1.465)
    // (round 4, with the group walk on the matrix cores: 2 sequences at 1,500 tokens 1.46 -> 1.38 ms per step, at 700 a tie; one sequence
    // at 700 / 1,500 / 3,000 tokens 1.05 / 1.11 / 1.24 for one head per workgroup against 1.13 / 1.21 / 1.24)
    if (rq <= 0) rq = (max_ctx <= (batch <= 1 ? ATTN_RQ1_CTX : ATTN_RQ1_CTX / 4) && batch <= ATTN_RQ1_BATCH) ? 1 : AD_RQ;
    if (rq != 1) rq = AD_RQ;
    int bucket = 64;
    while (bucket < max_ctx) bucket *= 2;
    const int chunks = (rep + rq - 1) / rq;
    const int base = std::max(1, batch * g.num_kv_heads * chunks);
    int s = 1;
    // Windows grow with the context (round 3, tools/decode_ab.py; profiles/r03_labs/attention_window_size_*.jsonl).  Up to 512 tokens of
    // context 64-token windows are the best at 1-4 sequences (one sequence at 200 tokens: 128-token windows 1.022 against 0.993 ms).
    // Beyond, 256-token windows: one sequence 700 / 1,500 / 3,000 tokens 1.078 -> 1.060, 1.218 -> 1.143, 1.386 -> 1.246 ms per step (the wo
    // GEMV still merges the 4 / 8 windows up to 2k tokens, 16 stand where 64 stood at 4k), two sequences 1.310 -> 1.245, 1.510 -> 1.361,
    // 1.666 -> 1.540, four sequences at 1,000 tokens 1.762 -> 1.610.  Two exceptions at 257..512 tokens, both measured: one sequence
    // 128-token windows (4 instead of 8 partials for the wo GEMV: 1.018 -> 1.014), 5-8 sequences 128 (1.882 -> 1.824 at 8).
    // TL_ATTN_MIN_TOKENS pins one size (lab).
    // Batched steps (5+ sequences) up to 1,024 tokens of context, re-measured at the end of round 6 on the round's kernels (matrix-core walk, shared prologue;
    // tools/lab/ab_attn_splits_batched.sh, profiles/r06_labs/README.md section 9): ONE workgroup per CU at most and windows of 128+ tokens -- the merge launch
    // and the second dependent trip of a short window cost more than a longer walk once every sequence's KV head has a workgroup: 5 / 8 / 12 / 16 / 23 sequences
    // at ~600 tokens 1.47 / 1.52 / 1.56 / 1.59 / 2.04 -> 1.39 / 1.42 / 1.53 / 1.57 / 1.87 ms per step, 9-23 at ~300 tokens -3 ... -6 %.
    const bool batched_short = k.min_tokens_auto && batch >= 5 && bucket <= 1024;
    int min_tokens = k.min_tokens;
    if (k.min_tokens_auto) {
        if (bucket > 512 && batch <= 4) min_tokens = 256;
        else if (bucket == 512 && batch == 1) min_tokens = 128;
        else if (batched_short) min_tokens = 128;
    }
    // few sequences: split for latency (up to 2048 short-lived workgroups); many sequences: the chip is already full, longer
    // windows amortise the per-workgroup prologue and skip the merge launch (measured at 16 and 64 sequences)
    // (5-7 sequences beyond 1,024 tokens too: 4 windows on 160-224 workgroups against 8 on 320-448 -- 5 / 6 / 7 sequences at 2,000 tokens 1.64 / 1.67 / 1.71 ->
    // 1.57 / 1.63 / 1.70 ms per step, at 8,000 2.45 / 2.57 / 2.65 -> 2.26 / 2.43 / 2.62; 8 and 16 sequences keep 512: 8 x 4,000 2.11 against 2.19)
    // (... and 8-16 sequences, the round's last sweep at 1,500 / 3,000 / 6,000 tokens: 10 sequences 1.80 / 2.17 / 2.96 -> 1.72 / 2.03 / 2.74 ms per step, 12: 1.85 / 2.27 / 3.08 ->
    // 1.78 / 2.15 / 3.00, 14: -2 %, 8 and 16 within 1 % either way; from 17 sequences no split at all, below)
    const bool few_long = k.min_tokens_auto && batch >= 5 && batch <= 16 && bucket > 1024;
    // (2-4 sequences on the GQA-group walk likewise, end of round 6: one workgroup per CU -- 3 / 4 sequences at 4,500 tokens 1.80 / 1.97 -> 1.66 / 1.81 ms per step,
    // at 8,000 2.02 / 2.29 -> 1.86 / 2.10, two sequences at 4,500 / 8,000 1.42 / 1.59 -> 1.36 / 1.55, 4 x 32,000 4.55 -> 4.41; one sequence: 8 KV heads x 32 windows already)
    const bool few_gqa = k.min_tokens_auto && batch >= 2 && batch <= 4 && rq == AD_RQ;
    const int wg_cap = ATTN_WG_CAP > 0 ? ATTN_WG_CAP : (batch <= 4 ? (few_gqa ? 256 : 2048) : ((batched_short || few_long) ? 256 : 512));
    // a whole GQA group per workgroup (long contexts / several sequences): at most 32 windows -- one workgroup per CU for one sequence;
    // measured at 8k 666 -> 680 tok/s against 64 windows, 32k unchanged (round 3)
    int max_splits = rq == AD_RQ ? k.max_splits_gqa : k.max_splits;
    // (64 windows = two workgroups per CU for the matrix-core walk at 32k: 1.931 / 1.896 -> 1.898 / 1.866 ms per step in one same-box
    // A/B, 1.874 -> 1.891 in the next: within the noise, not taken)
    // Many sequences at short contexts: one window per sequence and NO merge launch (round 4, same-box A/B at ~190 / ~660 tokens,
    // profiles/r04_labs/README.md): 12 / 16 sequences 1.623 -> 1.603 / 1.661 -> 1.634 ms per step at ~190 tokens (at ~660 the split stays:
    // 16 sequences 1.885 against 2.000), 24 / 32 sequences 2.15 -> 2.03 / 2.215 -> 2.07 at ~190 and 32 sequences 2.56 -> 2.495 at ~660.
    // The merge launch and its boundary cost ~2.5 us per layer; the unsplit walk of a few stages costs less once every CU has a workgroup.
    // (from 5 sequences at up to 256 tokens since the end of round 6: 5 / 7 / 9 / 10 sequences at ~150 tokens 1.30 / 1.35 / 1.44 / 1.45 -> 1.26 / 1.28 / 1.31 / 1.33 ms per step)
    // (from 17 sequences up to 8,192 tokens too, end of round 6: 160+ workgroups walking whole contexts beat twice as many on halves + a merge launch -- 20 / 23 / 24 / 32
    // sequences at 1,500 tokens 2.49 / 2.56 / 2.63 / 2.82 -> 2.25 / 2.36 / 2.40 / 2.70 ms per step, 24 at 2,500 / 4,000 / 8,000 3.10 / 4.20 / 6.44 -> 2.91 / 3.98 / 6.12;
    // 16 sequences at 2,000 want their 4 windows: 2.16 against 2.29)
    if (k.min_tokens_auto && ((batch >= 24 && bucket <= 1024) || (batch >= 5 && bucket <= 256) || (batch >= 17 && bucket <= 8192))) max_splits = 1;  // (17-19 sequences measured last: 1,500 / 3,000 / 6,000 tokens 2.44 / 3.19 / 4.85 -> 2.20 / 2.87 / 4.13 ms per step)
    while (s * 2 <= bucket / min_tokens && s * 2 * base <= wg_cap && s * 2 <= max_splits) s *= 2;  // >= min_tokens per workgroup
    // Windows sized to the context, not to its power-of-two bucket: a workgroup walks its whole window in 64-token stages
    // whether or not the tokens exist, so a 33k context on a 64k bucket spent half of every window on masked loads (r02:
    // 63 us per layer in the step against 44 us for the same kernel on an exactly filled bucket).  The split COUNT stays a
    // power of two (the kernels decode blockIdx with shifts); the plan (and its captured graph) changes every 64 * s tokens.
    const int per_split = ((max_ctx + s - 1) / s + 63) / 64 * 64;
    AttnPlan p;
    p.n_splits = s, p.tokens_per_split = std::max(64, std::min(per_split, bucket / s)), p.rq = rq;
    p.row_chunks = chunks, p.rep = rep, p.num_heads = g.num_heads, p.head_dim = g.head_dim;
    while ((1 << p.split_shift) < s) ++p.split_shift;
    for (int sh = 0; sh < 30; ++sh)
        if ((1 << sh) == g.page_size) p.page_shift = sh;
    p.grid[0] = (unsigned)(s * chunks), p.grid[1] = (unsigned)g.num_kv_heads, p.grid[2] = (unsigned)batch;
    return p;
}

// The launch over a split: which kernel walks the windows, with which variant bits and how much LDS, and what merges them.
//   qkv_partials_offered: the qkv projection left its slice planes (KeptPartials) instead of the rows
//   wo_can_merge: the wo GEMV behind the launch takes the split partials of this row itself (decode_linear.h, wo_merge_applicable)
inline AttnPlan plan_decode_launch(AttnPlan p, const AttnGeometry &g, const AttnKnobs &k, bool kv8, bool qkv_partials_offered, bool wo_can_merge) {
    p.kv8 = kv8;
    p.refuses_qkv_partials = qkv_partials_offered && !attn_takes_qkv_partials(g.head_dim, p.rq);
    p.qp = qkv_partials_offered && !p.refuses_qkv_partials;
    const int C = p.tokens_per_split;
    // a whole GQA group per workgroup: the walk on the matrix cores (attn_mfma.h) from 128-token windows -- a stage is 4 waves x 32
    // tokens, and on 64-token windows half of the waves idle (round 4, same-box A/B: 4 / 8 sequences at ~230 tokens 1.445 / 1.539
    // against 1.416 / 1.527 ms per step for the VALU walk; 4 sequences at 2k 1.691 against 1.729, one at 8k / 32k 1.256 / 1.90
    // against 1.35 / 2.13)
    if (k.mfma && C >= 128 && attn_decode_mfma_applicable(g.head_dim, p.rq, p.page_shift, C)) p.walk = AttnWalk::MATRIX_CORE;
    else if (C <= g.page_size && g.page_size % C == 0) p.walk = AttnWalk::SINGLE_PAGE;
    // every 64-token stage of a window inside one page: windows are multiples of 64 tokens, pages a power of two >= 64
    else if (p.page_shift >= 6 && C % 64 == 0) p.walk = AttnWalk::STAGE_PAGE;
    else p.walk = AttnWalk::GENERAL;
    const size_t staged = p.qp ? (size_t)(2 + AD_RQ) * g.head_dim * sizeof(unsigned short) : 0;  // the q rows of the group, k and v, summed from the planes
    p.lds_bytes = (p.walk == AttnWalk::MATRIX_CORE ? (size_t)ATTN_MFMA_LDS : (size_t)16 * p.rq * (g.head_dim + 2) * sizeof(float)) + staged;
    // the consumer (the wo GEMV of a single row) merges the partials itself: no merge launch, `out` is not written
    if (p.n_splits == 1 || wo_can_merge) p.merge = AttnMerge::NONE;
    else p.merge = p.n_splits == 2 ? AttnMerge::M2 : (p.n_splits == 4 ? AttnMerge::M4 : (p.n_splits == 8 ? AttnMerge::M8 : AttnMerge::COLUMNS));
    return p;
}

inline AttnPlan plan_decode_attention(const AttnGeometry &g, const AttnKnobs &k, int batch, int max_ctx, bool kv8 = false,
                                      bool qkv_partials_offered = false, bool wo_can_merge = false) {
    return plan_decode_launch(pick_decode_splits(g, k, batch, max_ctx), g, k, kv8, qkv_partials_offered, wo_can_merge);
}

}  // namespace tl
