// The decode attention's plan alone (csrc/attn_plan.h), without a device.
//
//   attention_plan_check plans   reads one request per line from stdin -- num_heads num_kv_heads head_dim page_size batch max_ctx kv8
//                                qkv_partials_offered wo_can_merge -- and prints each plan as a JSON line (knobs: the TL_ATTN_* environment).
//                                tests/test_attention_plan_cpu.py compares them with the plans recorded before the header existed.
//   attention_plan_check check   sweeps head shapes, head sizes, page sizes, page formats, offered slice partials, batches and contexts and
//                                holds every plan to what the kernels require of a launch -- stated here, independently of the header's rules.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "attn_plan.h"

using namespace tl;

static long g_checks = 0, g_plans = 0;
static int g_case[9];  // the input under check: knob set, heads, KV heads, head_dim, page size, kv8, offered, batch, context
static void require(bool ok, const char *what) {
    ++g_checks;
    if (ok) return;
    std::printf("FAILED knobs %d heads %d/%d head_dim %d page %d kv8 %d offered %d batch %d ctx %d: %s\n", g_case[0], g_case[1], g_case[2], g_case[3],
                g_case[4], g_case[5], g_case[6], g_case[7], g_case[8], what);
    std::exit(1);
}

static const char *const WALKS[] = {"matrix_core", "single_page", "stage_page", "general"};
static const char *const MERGES[] = {"none", "2", "4", "8", "columns"};

static int run_plans() {
    AttnKnobs k;
    k.read_env();
    int h, kvh, d, page, batch, ctx, kv8, offered, wo;
    while (std::scanf("%d %d %d %d %d %d %d %d %d", &h, &kvh, &d, &page, &batch, &ctx, &kv8, &offered, &wo) == 9) {
        const AttnGeometry g{h, kvh, d, page, 1};
        const AttnPlan p = plan_decode_attention(g, k, batch, ctx, kv8 != 0, offered != 0, wo != 0);
        std::printf("{\"plan\":[%d,%d,%d],\"walk\":\"%s\",\"qp\":%d,\"kv8\":%d,\"refuses_qkv_partials\":%d,\"merge\":\"%s\",\"lds\":%zu,\"grid\":[%u,%u,%u],"
                    "\"variant\":%d,\"key\":%ld}\n",
                    p.n_splits, p.tokens_per_split, p.rq, WALKS[(int)p.walk], (int)p.qp, (int)p.kv8, (int)p.refuses_qkv_partials, MERGES[(int)p.merge],
                    p.lds_bytes, p.grid[0], p.grid[1], p.grid[2], (int)attn_plan_has_variant(p), p.key());
    }
    return 0;
}

static bool same(const AttnPlan &a, const AttnPlan &b) {
    return a.n_splits == b.n_splits && a.tokens_per_split == b.tokens_per_split && a.rq == b.rq && a.row_chunks == b.row_chunks && a.rep == b.rep &&
           a.split_shift == b.split_shift && a.page_shift == b.page_shift && a.num_heads == b.num_heads && a.head_dim == b.head_dim &&
           a.grid[0] == b.grid[0] && a.grid[1] == b.grid[1] && a.grid[2] == b.grid[2] && a.walk == b.walk && a.qp == b.qp && a.kv8 == b.kv8 &&
           a.refuses_qkv_partials == b.refuses_qkv_partials && a.lds_bytes == b.lds_bytes && a.merge == b.merge;
}
static bool pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

using Variant = std::tuple<int, int, bool, bool, bool, bool>;  // VD, RQ, SP, IP, QP, KV8 (the matrix-core walk: VD = 0)
static std::set<Variant> g_seen;

// one plan against what a launch of it needs
static void check_plan(const AttnGeometry &g, const AttnKnobs &k, int batch, int max_ctx, bool kv8, bool offered, bool wo, const AttnPlan &p) {
    ++g_plans;
    const int C = p.tokens_per_split, rep = g.num_heads / g.num_kv_heads;
    // coverage: a window plan that falls short drops tokens silently
    require(pow2(p.n_splits) && (1 << p.split_shift) == p.n_splits, "n_splits is not a power of two with its shift");
    require(C >= 64 && C % 64 == 0, "tokens_per_split is not a multiple of 64 of at least 64");
    require((long)p.n_splits * C >= max_ctx, "the windows do not cover the context");
    // grid
    require(p.rq == 1 || p.rq == AD_RQ, "heads per workgroup");
    require(p.rep == rep && p.row_chunks * p.rq >= rep && (p.row_chunks - 1) * p.rq < rep, "the row chunks do not cover the GQA group exactly");
    require(p.grid[0] == (unsigned)(p.n_splits * p.row_chunks) && p.grid[1] == (unsigned)g.num_kv_heads && p.grid[2] == (unsigned)batch, "grid");
    require(p.page_shift == (pow2(g.page_size) ? __builtin_ctz(g.page_size) : -1), "page_shift");
    require(p.num_heads == g.num_heads && p.head_dim == g.head_dim && p.partials_bytes(batch) == (size_t)batch * g.num_heads * p.n_splits * (g.head_dim + 4) * 4,
            "partials_bytes");
    // the walks
    const bool whole_group = p.rq == AD_RQ;
    switch (p.walk) {
        case AttnWalk::SINGLE_PAGE: require(C <= g.page_size && g.page_size % C == 0, "single-page walk: a window does not lie inside one page"); break;
        case AttnWalk::STAGE_PAGE: require(pow2(g.page_size) && g.page_size >= 64 && C % 64 == 0, "stage-page walk: a 64-token stage may cross a page"); break;
        case AttnWalk::MATRIX_CORE:
            require(g.head_dim == 128 && whole_group, "matrix-core walk: needs head_dim 128 and the whole GQA group");
            require(C >= 128 && C % 32 == 0, "matrix-core walk: windows of at least 128 tokens, a multiple of 32");
            require(pow2(g.page_size) && g.page_size >= 32, "matrix-core walk: a wave's 32 tokens may cross a page");
            require(k.mfma, "matrix-core walk with TL_ATTN_MFMA=0");
            break;
        case AttnWalk::GENERAL: break;
    }
    // the variant bits
    require(p.kv8 == kv8 && (!p.kv8 || g.head_dim == 128), "KV8 away from head_dim 128");
    require(!p.qp || (g.head_dim == 128 && whole_group && offered), "QP away from head_dim 128 with the whole group, or unasked");
    require(p.refuses_qkv_partials == (offered && !p.qp), "offered slice partials are neither taken nor refused");
    require(p.lds_bytes > 0 && p.lds_bytes <= 160 * 1024, "LDS bytes");
    if (!p.refuses_qkv_partials) {
        require(attn_plan_has_variant(p), "the chosen variant is not in the instantiation table");
        const bool mc = p.walk == AttnWalk::MATRIX_CORE;
        g_seen.insert(Variant{mc ? 0 : g.head_dim / 16, mc ? 0 : p.rq, p.walk == AttnWalk::SINGLE_PAGE, p.walk == AttnWalk::STAGE_PAGE, p.qp, p.kv8});
    }
    // the merge
    const AttnMerge by_count = p.n_splits == 2 ? AttnMerge::M2 : (p.n_splits == 4 ? AttnMerge::M4 : (p.n_splits == 8 ? AttnMerge::M8 : AttnMerge::COLUMNS));
    require(p.merge == (p.n_splits == 1 || wo ? AttnMerge::NONE : by_count), "merge");
    require(p.wo_merges() == (wo && p.n_splits > 1) && p.launches() == (p.merge == AttnMerge::NONE ? 1 : 2), "launch count");
}

static int run_check() {
    const int shapes[][2] = {{32, 8}, {16, 8}, {40, 8}, {64, 8}, {8, 8}, {4, 2}};
    const int max_batches[] = {1, 4, 16, 64, 256};
    std::vector<int> contexts = {1, 2, 63, 100, 140000};
    for (int b = 64; b <= 131072; b *= 2)
        for (int c : {b - 1, b, b + 1, b + b / 2})
            if (c <= 140000) contexts.push_back(c);
    // knob sets: unset; the VALU twin of the matrix-core walk; TL_ATTN_MAX_SPLITS above what an engine's workspace is sized for
    const char *const knob_sets[][2] = {{nullptr, nullptr}, {"TL_ATTN_MFMA", "0"}, {"TL_ATTN_MAX_SPLITS", "256"}};
    for (int ks = 0; ks < 3; ++ks) {
        for (const char *name : {"TL_ATTN_MFMA", "TL_ATTN_RQ", "TL_ATTN_MAX_SPLITS", "TL_ATTN_MIN_TOKENS"}) unsetenv(name);
        if (knob_sets[ks][0]) setenv(knob_sets[ks][0], knob_sets[ks][1], 1);
        AttnKnobs k;
        k.read_env();
        for (const auto &hs : shapes)
            for (int d : {32, 64, 128})
                for (int page : {16, 48, 64, 128, 256})
                    for (int kv8 = 0; kv8 <= (d == 128 ? 1 : 0); ++kv8)
                        for (int offered = 0; offered <= 1; ++offered) {
                            const AttnGeometry g{hs[0], hs[1], d, page, 1};
                            for (int batch = 1; batch <= (ks == 0 ? 256 : 64); ++batch) {
                                std::map<long, AttnPlan> by_key;
                                for (int ctx : contexts) {
                                    const int now[9] = {ks, hs[0], hs[1], d, page, kv8, offered, batch, ctx};
                                    std::copy(now, now + 9, g_case);
                                    const AttnPlan p = plan_decode_attention(g, k, batch, ctx, kv8 != 0, offered != 0, false);
                                    check_plan(g, k, batch, ctx, kv8 != 0, offered != 0, false, p);
                                    // keys: one key, one plan (the engine caches a captured step by (batch, key))
                                    const auto it = by_key.find(p.key());
                                    if (it == by_key.end()) by_key[p.key()] = p;
                                    else require(same(it->second, p), "two plans share a key");
                                    // workspace: what an engine of max_batch sequences keeps holds every plan of its batches
                                    for (int mb : max_batches) {
                                        if (mb < batch) continue;
                                        const bool fits = p.partials_bytes(batch) <= attn_partials_capacity(g, mb);
                                        if (ks != 2) require(fits, "the partials exceed attn_partials_capacity with the split knobs unset");
                                        // ... and beyond 64 splits a plan that does not fit is one the launch refuses (n_splits > 1).  (No shape of this
                                        // sweep gets there: the workgroup caps of the split rule bound batch x n_splits by 512.)
                                        else if (!fits) require(p.n_splits > 64, "the partials exceed attn_partials_capacity at no more than 64 splits");
                                    }
                                    // the wo GEMV of one row takes 2 / 4 / 8 windows at head_dim 128 (linear_plan.h, wo_merge_applicable)
                                    if (batch == 1 && d == 128 && (p.n_splits == 2 || p.n_splits == 4 || p.n_splits == 8)) {
                                        const AttnPlan q = plan_decode_attention(g, k, batch, ctx, kv8 != 0, offered != 0, true);
                                        check_plan(g, k, batch, ctx, kv8 != 0, offered != 0, true, q);
                                        AttnPlan r = q;
                                        r.merge = p.merge;
                                        require(same(r, p), "wo_can_merge changed more than the merge");
                                    }
                                }
                            }
                        }
    }
#define SEEN(VD, RQ, SP, IP, QP, KV8) require(g_seen.count(Variant{VD, RQ, SP, IP, QP, KV8}) == 1, "no input of the sweep chooses the table's (" #VD ", " #RQ ", " #SP ", " #IP ", " #QP ", " #KV8 ")");
    ATTN_FUSED_TABLE(SEEN)
#undef SEEN
#define SEEN(QP, KV8) require(g_seen.count(Variant{0, 0, false, false, QP, KV8}) == 1, "no input of the sweep chooses the matrix-core table's (" #QP ", " #KV8 ")");
    ATTN_MFMA_TABLE(SEEN)
#undef SEEN
    require(g_seen.size() == 34, "the sweep chose a variant outside both tables");
    std::printf("ok plans=%ld checks=%ld\n", g_plans, g_checks);
    return 0;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plans") return run_plans();
    if (mode == "check") return run_check();
    std::fprintf(stderr, "usage: attention_plan_check plans|check\n");
    return 2;
}
