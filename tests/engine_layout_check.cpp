// The engine's memory layout alone (csrc/engine_layout.h; DESIGN.md "The engine's memory layout"), without a device.
//
//   engine_layout_check check    over a grid of configurations: every piece of every block is 256-byte aligned, the pieces lie in the
//                                block's order, pairwise disjoint and inside the total, the state words wholly before act_off, and every
//                                piece holds what its writers write -- stated here, independently of the header's arithmetic.
//   engine_layout_check layout   reads configurations and inputs from stdin (one per line, the numbers of read_case), prints each one's
//                                four layouts as a JSON line: tests/test_engine_layout_cpu.py compares them with the recorded offsets.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/tinyllm_engine.h"
#include "engine_layout.h"

using namespace tl;

static long g_checks = 0;
static std::string g_case;
static void require(bool ok, const char *block, const char *piece, const char *what, size_t have, size_t want) {
    ++g_checks;
    if (ok) return;
    std::printf("FAILED %s: %s.%s %s: %zu against %zu\n", g_case.c_str(), block, piece, what, have, want);
    std::exit(1);
}

template <int N>
static void check_block(const char *block, const Pieces<N> &a, const char *const *names, int count) {
    size_t end = 0;
    for (int i = 0; i < count; ++i) {
        require(a[i].off % 256 == 0, block, names[i], "offset is not a multiple of 256", a[i].off, 256);
        require(a[i].off >= end, block, names[i], "starts inside the piece before it", a[i].off, end);
        end = a[i].off + a[i].bytes;
        require(end <= a.bytes, block, names[i], "ends past the block", end, a.bytes);
    }
    require(a.bytes % 256 == 0, block, "bytes", "total is not a multiple of 256", a.bytes, 256);
}
static void holds(const char *block, const char *piece, const Piece &p, size_t bytes, const char *what) {
    require(p.bytes >= bytes, block, piece, what, p.bytes, bytes);
}

static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

static void check_case(const tl_engine_config &c, const LayoutInputs &in) {
    using A = ArenaLayout;
    using L = LayerLayout;
    using V = VerifyLayout;
    using M = MoeLayout;
    const size_t B = c.max_batch, H = c.hidden_size, I = c.intermediate_size, Vo = c.vocab_size;
    const size_t QKV = (size_t)(c.num_heads + 2 * c.num_kv_heads) * c.head_dim, Q = (size_t)c.num_heads * c.head_dim;
    const size_t R = (size_t)(c.max_batch > c.max_prefill_rows ? c.max_batch : c.max_prefill_rows);
    const size_t ssr = (size_t)(H / 16 + 1 > 8 ? H / 16 + 1 : 8);  // floats per row of a sums-of-squares buffer (QM3_SS = 8, or one per 16-column tile)

    const A a = arena_layout(c, in);
    check_block("arena", a, ARENA_NAMES, A::COUNT);
    for (int i = 0; i < A::COUNT; ++i) {
        if (i < A::X) require(a[i].off + a[i].bytes <= a.act_off, "arena", ARENA_NAMES[i], "a state word lies past act_off", a[i].off + a[i].bytes, a.act_off);
        else require(a[i].off >= a.act_off, "arena", ARENA_NAMES[i], "an activation lies before act_off", a[i].off, a.act_off);
    }
    // the state words
    holds("arena", "block_table", a[A::BLOCK_TABLE], B * c.max_pages_per_seq * 4, "one row of page ids per slot");
    for (int i : {A::CONTEXT_LENS, A::TOKENS, A::LIVE, A::PRODUCED}) holds("arena", ARENA_NAMES[i], a[i], B * 4, "one word per slot");
    holds("arena", "ring", a[A::RING], B * in.ring_cap * 4, "ring_cap ids per slot");
    holds("arena", "scratch_ctx", a[A::SCRATCH_CTX], 16 * 4, "the context lengths of the 16 sequences of a packed pass");
    holds("arena", "prefill_tokens", a[A::PREFILL_TOKENS], R * 4, "the ids of a pass of R rows");
    // a prefill pass of R = max(max_batch, max_prefill_rows) rows
    for (int i : {A::X, A::H, A::XN, A::TMP}) holds("arena", ARENA_NAMES[i], a[i], R * H * 2, "R rows of the hidden size");
    holds("arena", "qkv", a[A::QKV], R * QKV * 2, "R rows of q|k|v");
    for (int i : {A::Q_T, A::ATTN_T, A::ATTN}) holds("arena", ARENA_NAMES[i], a[i], R * Q * 2, "R rows of the query heads");
    holds("arena", "gu", a[A::GU], R * 2 * I * 2, "R rows of gate|up");
    holds("arena", "act", a[A::ACT], R * I * 2, "R rows of the intermediate size");
    holds("arena", "attn_ws", a[A::ATTN_WS], in.attn_ws_bytes, "the attention partials");
    // the single-slot verification: 8 rows
    holds("arena", "verify_ids", a[A::VERIFY_IDS], 8 * 4, "the greedy ids of 8 verification rows");
    holds("arena", "lm_tile_max", a[A::LM_TILE_MAX], 8 * (Vo / 16) * in.tile_max_bytes, "the tile maxima of 8 rows");
    holds("arena", "logits", a[A::LOGITS], 8 * Vo * 2, "8 verification rows");

    const L ll = layer_layout(c, in);
    if (in.aql) {
        check_block("layer", ll, LAYER_NAMES, L::COUNT);
        require(ll.rows == (int)(B < 64 ? B : 64), "layer", "rows", "min(max_batch, 64)", ll.rows, B < 64 ? B : 64);
        holds("layer", "plane0", ll[L::PLANE0], in.plane_bytes[0], "the slice planes of wo");
        holds("layer", "plane1", ll[L::PLANE1], in.plane_bytes[1], "the slice planes of w_down");
    } else {
        require(ll.rows == 0 && ll.bytes == 0, "layer", "rows", "no block without the AQL route", ll.rows, 0);
    }
    // a decode step over b rows, shared buffers and (where the step may take them) the layer's own
    for (size_t b = 1; b <= B; ++b) {
        for (int i : {A::X, A::H}) holds("arena", ARENA_NAMES[i], a[i], b * H * 2, "b decode rows");
        holds("arena", "xn", a[A::XN], up16(b) * H * 2, "the 16-row fragment blocks of b weighted rows");
        holds("arena", "qkv", a[A::QKV], b * QKV * 2, "b decode rows");
        holds("arena", "attn", a[A::ATTN], b * Q * 2, "b decode rows");
        holds("arena", "act", a[A::ACT], b * I * 2, "b decode rows");
        for (int i : {A::SS_X, A::SS_H}) holds("arena", ARENA_NAMES[i], a[i], b * ssr * 4, "the sums of squares of b rows");
        holds("arena", "logits", a[A::LOGITS], (b > 8 ? b : 8) * Vo * 2, "max(b, 8) rows of logits");
        if (!in.aql || b > (size_t)ll.rows) continue;
        for (int i : {L::X_OUT, L::H}) holds("layer", LAYER_NAMES[i], ll[i], b * H * 2, "b decode rows");
        for (int i : {L::XN, L::XW}) holds("layer", LAYER_NAMES[i], ll[i], up16(b) * H * 2, "the 16-row fragment blocks of b weighted rows");
        holds("layer", "qkv", ll[L::QKV], b * QKV * 2, "b decode rows");
        holds("layer", "attn", ll[L::ATTN], b * Q * 2, "b decode rows");
        holds("layer", "act", ll[L::ACT], b * I * 2, "b decode rows");
        for (int i : {L::SS_X_OUT, L::SS_H}) holds("layer", LAYER_NAMES[i], ll[i], b * ssr * 4, "the sums of squares of b rows");
        // unsplit, a step needs no partials; a split plan is taken only where b * heads * splits rows fit (plan_step asks the piece)
    }

    // a batched verification: 64 rows, 64 sequences
    const V v = verify_layout(c, in);
    check_block("verify", v, VERIFY_NAMES, v.own_ws ? V::COUNT : V::COUNT - 1);
    require(v.own_ws == (in.matmul_ws_need > in.matmul_ws_engine), "verify", "matmul_ws", "its own exactly where the engine's is too small", v.own_ws, 0);
    for (int i : {V::X, V::H, V::XN, V::TMP}) holds("verify", VERIFY_NAMES[i], v[i], 64 * H * 2, "64 rows of the hidden size");
    holds("verify", "qkv", v[V::QKV], 64 * QKV * 2, "64 rows of q|k|v");
    for (int i : {V::Q, V::ATTN}) holds("verify", VERIFY_NAMES[i], v[i], 64 * Q * 2, "64 rows of the query heads");
    holds("verify", "gu", v[V::GU], 64 * 2 * I * 2, "64 rows of gate|up");
    holds("verify", "act", v[V::ACT], 64 * I * 2, "64 rows of the intermediate size");
    holds("verify", "logits", v[V::LOGITS], 64 * Vo * 2, "64 rows of logits");
    for (int i : {V::SS_X, V::SS_H}) holds("verify", VERIFY_NAMES[i], v[i], 64 * ssr * 4, "the sums of squares of 64 rows");
    holds("verify", "attn_ws", v[V::ATTN_WS], in.verify_ws_rows * (128 + 2) * 4, "the partial rows of verify_ws_rows()");
    holds("verify", "desc", v[V::DESC], 7 * 64 * 4, "seven arrays of 64 words");
    holds("verify", "greedy", v[V::GREEDY], 64 * 4, "64 greedy ids");
    holds("verify", "results", v[V::RESULTS], 64 * in.verify_result_bytes, "64 results");
    if (v.own_ws) holds("verify", "matmul_ws", v[V::MATMUL_WS], in.matmul_ws_need, "the matmul workspace of 64 rows");

    if (in.moe_k > 0) {
        const M m = moe_layout(c, in);
        check_block("moe", m, MOE_NAMES, M::COUNT);
        const size_t er = R * in.moe_k;  // expert rows
        holds("moe", "logits", m[M::LOGITS], R * in.moe_e * 2, "R rows of router logits");
        holds("moe", "ids", m[M::IDS], er * 4, "R * k expert ids");
        holds("moe", "scores", m[M::SCORES], er * 2, "R * k scores");
        for (int i : {M::GATE, M::UP, M::ACT}) holds("moe", MOE_NAMES[i], m[i], er * in.moe_i * 2, "R * k expert rows of the experts' intermediate size");
        holds("moe", "y", m[M::Y], er * H * 2, "R * k expert rows of the hidden size");
    }
}

struct Model {
    const char *name;
    int hidden, layers, heads, kv_heads, head_dim, inter, vocab;
};

static int run_check() {
    const Model models[] = {{"tiny", 256, 2, 4, 2, 128, 512, 1024},       {"wide", 1280, 1, 10, 2, 128, 2560, 4096},
                            {"tiny_d64", 256, 2, 4, 2, 64, 512, 1024},    {"tiny_d32", 256, 2, 4, 2, 32, 512, 1024},
                            {"odd_vocab", 384, 3, 6, 2, 64, 640, 1000},   {"qwen3-4b", 2560, 36, 32, 8, 128, 9728, 151936}};
    const int moes[][3] = {{0, 0, 0}, {2, 4, 256}, {8, 128, 768}};
    int configs = 0;
    for (const Model &m : models)
        for (int max_batch : {1, 2, 4, 7, 8, 9, 16, 17, 24, 63, 64, 65, 256})
            for (int rows : {1, 8, 15, 512, 2048})
                for (int aql = 0; aql < 2; ++aql)
                    for (const auto &moe : moes)
                        for (int own = 0; own < 2; ++own) {
                            if (std::string(m.name) == "qwen3-4b" && max_batch != 64 && max_batch != 256) continue;
                            tl_engine_config c{};
                            c.hidden_size = m.hidden, c.num_layers = m.layers, c.num_heads = m.heads, c.num_kv_heads = m.kv_heads, c.head_dim = m.head_dim;
                            c.intermediate_size = m.inter, c.vocab_size = m.vocab, c.page_size = 16, c.num_pages = 64, c.max_batch = max_batch;
                            c.max_pages_per_seq = 5, c.max_prefill_rows = rows;
                            LayoutInputs in;
                            in.attn_ws_pad = 4, in.qm3_ss = 8, in.ring_cap = 4096, in.tile_max_bytes = 8, in.verify_head_dim = 128, in.verify_result_bytes = 36;
                            in.attn_ws_bytes = (size_t)(max_batch * 64 > 1024 ? max_batch * 64 : 1024) * m.heads * (m.head_dim + 4) * 4 + 4 * own;
                            in.aql = aql != 0;
                            in.plane_bytes[0] = aql && max_batch >= 5 ? (size_t)256 * 40 * max_batch : 0, in.plane_bytes[1] = aql && max_batch >= 5 ? 256 * 97 : 0;
                            in.matmul_ws_need = (size_t)64 * m.inter * 4 * 8 + 12, in.matmul_ws_engine = own ? 4096 : in.matmul_ws_need * 2;
                            in.verify_ws_rows = 2048 + 64 * m.heads;
                            in.moe_k = moe[0], in.moe_e = moe[1], in.moe_i = moe[2];
                            g_case = std::string(m.name) + " max_batch=" + std::to_string(max_batch) + " max_prefill_rows=" + std::to_string(rows) +
                                     " aql=" + std::to_string(aql) + " moe_k=" + std::to_string(moe[0]) + " own_ws=" + std::to_string(own);
                            check_case(c, in);
                            ++configs;
                        }
    std::printf("ok configs=%d checks=%ld\n", configs, g_checks);
    return 0;
}

template <int N>
static void print_block(const char *block, const Pieces<N> &a, const char *const *names, int count, const std::string &extra) {
    std::printf("\"%s\": {", block);
    for (int i = 0; i < count; ++i) std::printf("\"%s\": %zu, ", names[i], a[i].off);
    std::printf("%s\"bytes\": %zu}", extra.c_str(), a.bytes);
}

// hidden layers heads kv_heads head_dim inter vocab page_size num_pages max_batch max_pages_per_seq max_prefill_rows | attn_ws_bytes attn_ws_pad
// qm3_ss plane0 plane1 matmul_ws_need matmul_ws_engine aql ring_cap tile_max_bytes verify_ws_rows verify_head_dim verify_result_bytes moe_k moe_e moe_i
static bool read_case(tl_engine_config &c, LayoutInputs &in) {
    long long v[28];
    for (auto &x : v)
        if (std::scanf("%lld", &x) != 1) return false;
    c = tl_engine_config{};
    c.hidden_size = (int)v[0], c.num_layers = (int)v[1], c.num_heads = (int)v[2], c.num_kv_heads = (int)v[3], c.head_dim = (int)v[4];
    c.intermediate_size = (int)v[5], c.vocab_size = (int)v[6], c.page_size = (int)v[7], c.num_pages = (int)v[8], c.max_batch = (int)v[9];
    c.max_pages_per_seq = (int)v[10], c.max_prefill_rows = (int)v[11];
    in = LayoutInputs{};
    in.attn_ws_bytes = (size_t)v[12], in.attn_ws_pad = (int)v[13], in.qm3_ss = (int)v[14], in.plane_bytes[0] = (size_t)v[15], in.plane_bytes[1] = (size_t)v[16];
    in.matmul_ws_need = (size_t)v[17], in.matmul_ws_engine = (size_t)v[18], in.aql = v[19] != 0, in.ring_cap = (int)v[20], in.tile_max_bytes = (size_t)v[21];
    in.verify_ws_rows = (size_t)v[22], in.verify_head_dim = (int)v[23], in.verify_result_bytes = (size_t)v[24];
    in.moe_k = (int)v[25], in.moe_e = (int)v[26], in.moe_i = (int)v[27];
    return true;
}

static int run_layout() {
    tl_engine_config c;
    LayoutInputs in;
    while (read_case(c, in)) {
        const ArenaLayout a = arena_layout(c, in);
        const LayerLayout l = layer_layout(c, in);
        const VerifyLayout v = verify_layout(c, in);
        const MoeLayout m = moe_layout(c, in);
        std::printf("{");
        print_block("arena", a, ARENA_NAMES, ArenaLayout::COUNT, "\"act_off\": " + std::to_string(a.act_off) + ", ");
        std::printf(", ");
        print_block("layer", l, LAYER_NAMES, in.aql ? LayerLayout::COUNT : 0, "\"rows\": " + std::to_string(l.rows) + ", ");
        std::printf(", ");
        print_block("verify", v, VERIFY_NAMES, v.own_ws ? VerifyLayout::COUNT : VerifyLayout::COUNT - 1, "\"own_ws\": " + std::to_string(v.own_ws ? 1 : 0) + ", ");
        std::printf(", ");
        print_block("moe", m, MOE_NAMES, MoeLayout::COUNT, "");
        std::printf("}\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "check";
    if (mode == "check") return run_check();
    if (mode == "layout") return run_layout();
    std::fprintf(stderr, "usage: engine_layout_check check | layout < cases\n");
    return 2;
}
