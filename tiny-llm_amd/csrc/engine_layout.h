// The engine's memory layout (DESIGN.md "The engine's memory layout"): the capacities its buffers are sized by and the four blocks that hold
// activation rows, beside slot_table.h and slot_settings.h.  Host only, no HIP include and no device pointer dereferenced: engine.hip asks
// a layout, allocates its bytes and binds its pointers, and tests/engine_layout_check.cpp checks the same code alone -- every piece aligned,
// disjoint and large enough for what its writers write.
//
//   capacities  one name per number that several files must agree on; engine.hip static_asserts the device headers' constants against them.
//   layouts     a pure function from the engine's configuration (`Config`: tl_engine_config, include/tinyllm_engine.h, or any record with
//               its fields) and the sizes only device-side headers know (LayoutInputs) to named pieces: offset and size in bytes, in the order
//               they lie in the block, every offset a multiple of 256.
//   Act         the hand-over buffers of one layer, bound from a layout: the arena's shared ones, a layer's own, the verification's.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace tl {

// ---- the capacities ---------------------------------------------------------------------------------------------------------------------
constexpr int PACKED_MAX_SEQS = 16;    // sequences of a packed pass: scratch_ctx, prefill_pass's per-sequence arrays, pool.h POOL_MAX_SEQS
constexpr int VERIFY_MAX_LEN = 8;      // rows of tl_engine_verify[_sampled] and of one sequence of a batched verification: verify_ids, the
                                       // tile maxima, SpecRecord's arrays, verify_attn_host.h VA_MAX_LEN, the floor of the logits rows
constexpr int VERIFY_BATCH_ROWS = 64;  // rows and sequences of a batched verification: its scratch, `desc`, verify_attn_host.h VA_MAX_ROWS
constexpr int LAYER_ACT_MAX_ROWS = 64;  // most rows the per-layer decode buffers hold (the batched-matmul step ends there)
constexpr int VERIFY_DESC_ARRAYS = 7;   // arrays of VERIFY_BATCH_ROWS words in the verification's `desc` (VerifyScratch::DESC_ARRAYS)
inline int layer_act_rows(int max_batch) { return std::min(max_batch, LAYER_ACT_MAX_ROWS); }
inline int logits_rows(int max_batch) { return std::max(max_batch, VERIFY_MAX_LEN); }  // decode rows, or the rows of a verification
template <class Config>
int prefill_rows(const Config &c) {  // rows of every prefill buffer (the engine's rows_cap)
    return std::max(c.max_prefill_rows, c.max_batch);
}

constexpr size_t LAYOUT_ALIGN = 256;
inline size_t ceil16(size_t rows) { return (rows + 15) / 16 * 16; }

// the sizes that come from the device headers and the engine's matrices (engine.hip computes them)
struct LayoutInputs {
    size_t attn_ws_bytes = 0;         // the arena's attention partials: decode windows, or the paged operator's splits of any chunk
    int attn_ws_pad = 0;              // engine_kernels.h ATTN_WS_PAD: floats behind the head_dim of a partial row
    int qm3_ss = 0;                   // qmm3.h QM3_SS: partial sums of squares per row
    size_t plane_bytes[2] = {0, 0};   // slice planes of one layer's wo / w_down on the batched step (multiples of LAYOUT_ALIGN)
    size_t matmul_ws_need = 0;        // verification: what the matmuls of VERIFY_BATCH_ROWS rows need ...
    size_t matmul_ws_engine = 0;      // ... and what the engine's own workspace holds
    bool aql = false;                 // the AQL route is on: the per-layer block exists
    int ring_cap = 0;                 // ids kept per slot
    size_t tile_max_bytes = 0;        // sizeof(f32x2): one (max, index) pair of the lm_head's tile maxima
    size_t verify_ws_rows = 0;        // verify_attn_host.h verify_ws_rows(): partial rows of [VERIFY head_dim + 2] floats
    int verify_head_dim = 0;          // verify_attn_host.h VA_D
    size_t verify_result_bytes = 0;   // sizeof(tl_verify_result)
    int moe_k = 0, moe_e = 0, moe_i = 0;  // MoE: the largest experts_per_token, num_experts, intermediate_size of any layer
};

struct Piece {
    size_t off = 0, bytes = 0;
};
// N pieces side by side, added in the order they lie in the block (the order of the block's enum); `bytes` is the block's size
template <int N>
struct Pieces {
    Piece p[N];
    size_t bytes = 0;
    void add(int id, size_t size) {
        p[id] = {bytes, size};
        bytes = (bytes + size + LAYOUT_ALIGN - 1) / LAYOUT_ALIGN * LAYOUT_ALIGN;
    }
    const Piece &operator[](int id) const { return p[id]; }
};

template <class Config>
size_t ss_row_floats(const Config &c, const LayoutInputs &in) {
    // per-row partial sums of squares: QM3_SS per row from the skinny-matmul reduction / the embedding kernels, one per 16-row tile
    // (hidden / 16) from the 1-4-row GEMVs
    return (size_t)std::max(in.qm3_ss, c.hidden_size / 16 + 1);
}
template <class Config>
size_t qkv_dim(const Config &c) {
    return (size_t)(c.num_heads + 2 * c.num_kv_heads) * c.head_dim;
}
template <class Config>
size_t q_dim(const Config &c) {
    return (size_t)c.num_heads * c.head_dim;
}

// ---- the arena: state words, then activations ----------------------------------------------------------------------------------------------
struct ArenaLayout : Pieces<24> {
    enum { BLOCK_TABLE, CONTEXT_LENS, TOKENS, LIVE, PRODUCED, RING, SCRATCH_CTX, PREFILL_TOKENS, X, H, XN, TMP, QKV, Q_T, ATTN_T, ATTN, GU, ACT,
           LOGITS, VERIFY_IDS, LM_TILE_MAX, SS_X, SS_H, ATTN_WS, COUNT };
    size_t act_off = 0;  // the state words end here: zeroed at create, the block table then filled with -1
};
inline const char *const ARENA_NAMES[ArenaLayout::COUNT] = {
    "block_table", "context_lens", "tokens", "live", "produced", "ring", "scratch_ctx", "prefill_tokens", "x", "h", "xn", "tmp", "qkv", "q_t",
    "attn_t", "attn", "gu", "act", "logits", "verify_ids", "lm_tile_max", "ss_x", "ss_h", "attn_ws"};

template <class Config>
ArenaLayout arena_layout(const Config &c, const LayoutInputs &in) {
    using A = ArenaLayout;
    const size_t B = (size_t)c.max_batch, R = (size_t)prefill_rows(c), H = (size_t)c.hidden_size, I = (size_t)c.intermediate_size;
    A a;
    a.add(A::BLOCK_TABLE, B * c.max_pages_per_seq * 4);
    a.add(A::CONTEXT_LENS, B * 4);
    a.add(A::TOKENS, B * 4);
    a.add(A::LIVE, B * 4);
    a.add(A::PRODUCED, B * 4);
    a.add(A::RING, B * in.ring_cap * 4);
    a.add(A::SCRATCH_CTX, (size_t)PACKED_MAX_SEQS * 4);  // the context length of every sequence of a packed pass
    a.add(A::PREFILL_TOKENS, R * 4);
    a.act_off = a.bytes;
    a.add(A::X, R * H * 2);
    a.add(A::H, R * H * 2);
    a.add(A::XN, ceil16(R) * H * 2);  // weighted rows of a batched step lie in 16-row fragment blocks (qmm6.h)
    a.add(A::TMP, R * H * 2);
    a.add(A::QKV, R * qkv_dim(c) * 2);
    a.add(A::Q_T, R * q_dim(c) * 2);
    a.add(A::ATTN_T, R * q_dim(c) * 2);
    a.add(A::ATTN, R * q_dim(c) * 2);
    a.add(A::GU, R * 2 * I * 2);
    a.add(A::ACT, R * I * 2);
    a.add(A::LOGITS, (size_t)logits_rows(c.max_batch) * c.vocab_size * 2);
    a.add(A::VERIFY_IDS, (size_t)VERIFY_MAX_LEN * 4);
    a.add(A::LM_TILE_MAX, (size_t)VERIFY_MAX_LEN * (c.vocab_size / 16 + 1) * in.tile_max_bytes);
    a.add(A::SS_X, B * ss_row_floats(c, in) * 4);
    a.add(A::SS_H, B * ss_row_floats(c, in) * 4);
    a.add(A::ATTN_WS, in.attn_ws_bytes);
    return a;
}

// ---- one layer's block of the per-layer decode activations (the AQL route; common.h "activations between the launches of a decode step") ----
// Every hand-over address of a step is written once per step.  The attention partials hold 16 windows per row (at most 1,024
// row-windows): a plan beyond that keeps the shared buffers and the graph route.
struct LayerLayout : Pieces<12> {
    enum { X_OUT, H, XN, XW, QKV, ATTN, ACT, SS_X_OUT, SS_H, ATTN_WS, PLANE0, PLANE1, COUNT };
    int rows = 0;  // rows the buffers hold (0: no block); `bytes` is the stride from one layer's block to the next
};
inline const char *const LAYER_NAMES[LayerLayout::COUNT] = {"x_out", "h", "xn", "xw", "qkv", "attn", "act", "ss_x_out", "ss_h", "attn_ws", "plane0",
                                                            "plane1"};

template <class Config>
LayerLayout layer_layout(const Config &c, const LayoutInputs &in) {
    using L = LayerLayout;
    L a;
    if (!in.aql) return a;
    const int rows = layer_act_rows(c.max_batch);
    const size_t R = (size_t)rows, H = (size_t)c.hidden_size;
    a.rows = rows;
    a.add(L::X_OUT, R * H * 2);
    a.add(L::H, R * H * 2);
    // weighted rows lie in 16-row fragment blocks (qmm6.h): a partly filled last block spans all 16 row slots -- sized like the shared xn.
    // With `rows` itself a batch of 17-24 on a 24-slot engine wrote its block past xn into xw and past xw into qkv: dead bytes at that
    // moment by the order of the launches, but a second write per step to addresses the replay route reads without cache maintenance
    a.add(L::XN, ceil16(R) * H * 2);
    a.add(L::XW, ceil16(R) * H * 2);
    a.add(L::QKV, R * qkv_dim(c) * 2);
    a.add(L::ATTN, R * q_dim(c) * 2);
    a.add(L::ACT, R * c.intermediate_size * 2);
    a.add(L::SS_X_OUT, R * ss_row_floats(c, in) * 4);
    a.add(L::SS_H, R * ss_row_floats(c, in) * 4);
    a.add(L::ATTN_WS, (size_t)std::min(rows * 64, std::max(4 * 64, std::min(rows * 16, 1024))) * c.num_heads * ((size_t)c.head_dim + in.attn_ws_pad) * 4);
    a.add(L::PLANE0, in.plane_bytes[0]);
    a.add(L::PLANE1, in.plane_bytes[1]);
    return a;
}

// ---- the scratch of a batched verification ----------------------------------------------------------------------------------------------------
struct VerifyLayout : Pieces<17> {
    enum { X, H, XN, TMP, QKV, Q, ATTN, GU, ACT, LOGITS, SS_X, SS_H, ATTN_WS, DESC, GREEDY, RESULTS, MATMUL_WS, COUNT };
    bool own_ws = false;  // the matmuls of VERIFY_BATCH_ROWS rows need more than the engine's workspace holds: MATMUL_WS is theirs
};
inline const char *const VERIFY_NAMES[VerifyLayout::COUNT] = {"x", "h", "xn", "tmp", "qkv", "q", "attn", "gu", "act", "logits", "ss_x", "ss_h",
                                                              "attn_ws", "desc", "greedy", "results", "matmul_ws"};

template <class Config>
VerifyLayout verify_layout(const Config &c, const LayoutInputs &in) {
    using V = VerifyLayout;
    const size_t R = VERIFY_BATCH_ROWS, H = (size_t)c.hidden_size, I = (size_t)c.intermediate_size;
    V a;
    a.own_ws = in.matmul_ws_need > in.matmul_ws_engine;
    a.add(V::X, R * H * 2);
    a.add(V::H, R * H * 2);
    a.add(V::XN, R * H * 2);
    a.add(V::TMP, R * H * 2);
    a.add(V::QKV, R * qkv_dim(c) * 2);
    a.add(V::Q, R * q_dim(c) * 2);
    a.add(V::ATTN, R * q_dim(c) * 2);
    a.add(V::GU, R * 2 * I * 2);
    a.add(V::ACT, R * I * 2);
    a.add(V::LOGITS, R * c.vocab_size * 2);
    a.add(V::SS_X, R * ss_row_floats(c, in) * 4);
    a.add(V::SS_H, R * ss_row_floats(c, in) * 4);
    a.add(V::ATTN_WS, in.verify_ws_rows * ((size_t)in.verify_head_dim + 2) * 4);
    a.add(V::DESC, (size_t)VERIFY_DESC_ARRAYS * VERIFY_BATCH_ROWS * 4);
    a.add(V::GREEDY, R * 4);
    a.add(V::RESULTS, R * in.verify_result_bytes);
    if (a.own_ws) a.add(V::MATMUL_WS, in.matmul_ws_need);  // (else the engine's own workspace: no piece)
    return a;
}

// ---- the MoE workspace: router logits, ids, scores, then the expert rows (prefill_rows x k of them) ------------------------------------------------
struct MoeLayout : Pieces<7> {
    enum { LOGITS, IDS, SCORES, GATE, UP, ACT, Y, COUNT };
};
inline const char *const MOE_NAMES[MoeLayout::COUNT] = {"logits", "ids", "scores", "gate", "up", "act", "y"};

template <class Config>
MoeLayout moe_layout(const Config &c, const LayoutInputs &in) {
    using M = MoeLayout;
    const size_t R = (size_t)prefill_rows(c), k = (size_t)in.moe_k, E = (size_t)in.moe_e, I = (size_t)in.moe_i;
    M a;
    a.add(M::LOGITS, R * E * 2);
    a.add(M::IDS, R * k * 4);
    a.add(M::SCORES, R * k * 2);
    a.add(M::GATE, R * k * I * 2);
    a.add(M::UP, R * k * I * 2);
    a.add(M::ACT, R * k * I * 2);
    a.add(M::Y, R * k * c.hidden_size * 2);
    return a;
}

// ---- the hand-over buffers of one layer -----------------------------------------------------------------------------------------------------
struct Act {
    uint16_t *x_out = nullptr, *h = nullptr, *xn = nullptr, *xw = nullptr, *qkv = nullptr, *attn = nullptr, *act = nullptr;
    float *ss_x_out = nullptr, *ss_h = nullptr, *attn_ws = nullptr;
    // 5 .. 64 rows of a per-layer block: the fp32 slice planes of the layer's K-sliced matmuls (wo at 17-32 rows, w_down at every row
    // count); null elsewhere: the projection router's own workspace
    float *planes[2] = {nullptr, nullptr};
};
template <class T>
T *piece_at(char *base, const Piece &p) {
    return (T *)(base + p.off);
}
// the arena's shared buffers (xw: the one weighted copy is xn itself)
inline Act arena_act(char *base, const ArenaLayout &a) {
    using A = ArenaLayout;
    Act b;
    b.x_out = piece_at<uint16_t>(base, a[A::X]), b.h = piece_at<uint16_t>(base, a[A::H]), b.xn = b.xw = piece_at<uint16_t>(base, a[A::XN]);
    b.qkv = piece_at<uint16_t>(base, a[A::QKV]), b.attn = piece_at<uint16_t>(base, a[A::ATTN]), b.act = piece_at<uint16_t>(base, a[A::ACT]);
    b.ss_x_out = piece_at<float>(base, a[A::SS_X]), b.ss_h = piece_at<float>(base, a[A::SS_H]), b.attn_ws = piece_at<float>(base, a[A::ATTN_WS]);
    return b;
}
// layer l's own buffers; `base`: the start of the per-layer allocation
inline Act layer_act(char *base, const LayerLayout &a, int l) {
    using L = LayerLayout;
    char *m = base + (size_t)l * a.bytes;
    Act b;
    b.x_out = piece_at<uint16_t>(m, a[L::X_OUT]), b.h = piece_at<uint16_t>(m, a[L::H]), b.xn = piece_at<uint16_t>(m, a[L::XN]);
    b.xw = piece_at<uint16_t>(m, a[L::XW]), b.qkv = piece_at<uint16_t>(m, a[L::QKV]), b.attn = piece_at<uint16_t>(m, a[L::ATTN]);
    b.act = piece_at<uint16_t>(m, a[L::ACT]), b.ss_x_out = piece_at<float>(m, a[L::SS_X_OUT]), b.ss_h = piece_at<float>(m, a[L::SS_H]);
    b.attn_ws = piece_at<float>(m, a[L::ATTN_WS]), b.planes[0] = piece_at<float>(m, a[L::PLANE0]), b.planes[1] = piece_at<float>(m, a[L::PLANE1]);
    return b;
}
// the verification's (nothing weighted there: xw stays null)
inline Act verify_act(char *base, const VerifyLayout &a) {
    using V = VerifyLayout;
    Act b;
    b.x_out = piece_at<uint16_t>(base, a[V::X]), b.h = piece_at<uint16_t>(base, a[V::H]), b.xn = piece_at<uint16_t>(base, a[V::XN]);
    b.qkv = piece_at<uint16_t>(base, a[V::QKV]), b.attn = piece_at<uint16_t>(base, a[V::ATTN]), b.act = piece_at<uint16_t>(base, a[V::ACT]);
    b.ss_x_out = piece_at<float>(base, a[V::SS_X]), b.ss_h = piece_at<float>(base, a[V::SS_H]), b.attn_ws = piece_at<float>(base, a[V::ATTN_WS]);
    return b;
}

}  // namespace tl
