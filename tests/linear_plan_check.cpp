// The plans of the decode projections alone (csrc/linear_plan.h), without a device.
//
//   linear_plan_check plans   reads one request per line from stdin and prints one record per request, in the formats of
//                             tests/golden/make_linear_plans.py (its recorder printed the same records from the planners the kernel headers
//                             held): qmv / qmv3 / qmm3 / qmm6 / qmm7 plan records and `route` lines, planned for 256 CUs.
//                             tests/test_linear_plan_cpu.py compares them with tests/golden/linear_plans.json.
//   linear_plan_check check   sweeps row counts, reductions, tile counts, CU counts, grids and knob sets and holds every plan to what a launch
//                             of it needs and every route to what the engine does with it -- stated here, independently of the header's rules.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "linear_plan.h"

using namespace tl;

static long g_checks = 0, g_plans = 0;
static const char *g_what = "";
static int g_case[5];  // the input under check: rows M, reduction N, output rows K, CUs, grid mode / row order
static void require(bool ok, const char *what) {
    ++g_checks;
    if (ok) return;
    std::printf("FAILED %s M %d N %d K %d cus %d arg %d: %s\n", g_what, g_case[0], g_case[1], g_case[2], g_case[3], g_case[4], what);
    std::exit(1);
}

// (hidden, Hq * D, (Hq + 2 Hkv) * D, intermediate, vocab): tests/test_decode_plans_cpu.py MODEL_SHAPES
struct Model {
    const char *name;
    int hidden, q_dim, qkv_dim, inter, vocab;
};
static const Model MODELS[] = {
    {"qwen3-0.6b", 1024, 2048, 4096, 3072, 151936}, {"qwen3-1.7b", 2048, 2048, 4096, 6144, 151936}, {"qwen3-4b", 2560, 4096, 6144, 9728, 151936},
    {"qwen3-8b", 4096, 4096, 6144, 12288, 151936},  {"qwen3-14b", 5120, 5120, 7168, 17408, 151936}, {"qwen3-32b", 5120, 8192, 10240, 25600, 151936},
    {"qwen2-7b", 3584, 3584, 4608, 18944, 152064},
};
static LayerShapes layer_of(const Model &m) {
    return LayerShapes{{m.qkv_dim, m.hidden, true}, {m.hidden, m.q_dim, true}, {2 * m.inter, m.hidden, true}, {m.hidden, m.inter, true}, true};
}
static ProjShape head_of(const Model &m) { return ProjShape{m.vocab, m.hidden, true}; }

// ---- plans: the records of the golden file ------------------------------------------------------------------
static void print_route(const LinearKnobs &k, const Model &m, int batch) {
    const LayerShapes w = layer_of(m);
    const ProjShape all[5] = {w.wqkv, w.wo, w.wgu, w.wdown, head_of(m)};
    std::printf("%d |", (int)gemv_takes_rows(k, batch));
    for (const ProjShape &p : all) std::printf(" %d%d", (int)qmm6_takes(k, p, batch), (int)takes_skinny_matmul(k, p, batch));
    std::printf(" | %d |", (int)weighted_rows_apply(k, w.wo, w.wgu, batch));
    for (int ns : {2, 4, 8}) std::printf(" %d", (int)wo_merge_applicable(k, w.wo, batch, ns, 128, m.q_dim / 128));
    const LayerRoute r = plan_layer(k, w, batch, false);
    std::printf(" | %d %d %d %d %d %d | %d\n", (int)r.batched, (int)r.qkv6, (int)r.wo6, (int)r.down, (int)r.gemv_weighted, (int)r.batched_written_once(),
                (int)rows_travel_in_fragment_order(k, w, batch));
}

static int run_plans() {
    const int ncu = 256;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        int M = 0, rows = 0, cols = 0, x = 0;
        if (what == "qmv") {
            in >> M >> rows >> cols;
            const QmvPlan p = qmv_plan(M, cols, rows);
            std::printf("%d %d %d %d %d %zu\n", p.MR, p.WN, p.RPL, p.RB, p.blocks, p.lds);
        } else if (what == "qmv3") {
            in >> M >> rows >> cols;
            const Qmv3Plan p = qmv3_plan(M, cols, rows);
            std::printf("%d %d %d %d %d %zu %d\n", p.MR, p.KS, p.CW, p.LM, p.blocks, p.lds, (int)p.ok);
        } else if (what == "qmm3") {
            in >> x >> M >> rows >> cols;
            const Qmm3Plan p = qmm3_plan(M, cols, rows, x, ncu);
            const Qmm3pGrid &g = p.pgrid;
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %zu %d\n", p.MB, p.TW, p.LM, p.slices, p.tile_groups, p.grid_x, p.persistent,
                        p.tiles_per_wg, p.NU, g.full_slices, g.wgs_full, g.tpw_full, g.last_groups, g.wgs_last, g.tpw_last, p.lds, p.partial_bytes, (int)p.ok);
        } else if (what == "qmm6") {
            in >> x >> M >> rows >> cols;
            const Qmm6Plan p = qmm6_plan(M, cols, rows, x != 0, ncu);
            std::printf("%d %d %d %d %d %d %zu %d\n", p.MB, p.GPW, p.NSETS, p.row_blocks, p.wgs, p.tiles_per_wg, p.lds, (int)p.ok);
        } else if (what == "qmm7") {
            in >> M >> rows >> cols;
            const Qmm7Plan p = qmm7_plan(M, cols, rows, ncu);
            std::printf("%d %d %d %d %d %zu %d\n", p.MB, p.T, p.GPW, p.wgs, p.row_blocks, p.lds, (int)p.ok);
        } else if (what == "route") {
            int k[10], batch = 0;
            Model m{"", 0, 0, 0, 0, 0};
            for (int &v : k) in >> v;
            in >> m.hidden >> m.q_dim >> m.qkv_dim >> m.inter >> m.vocab >> batch;
            LinearKnobs kn;
            kn.use_qmm3 = k[0], kn.use_qmm6 = k[1], kn.use_qmm7 = k[2], kn.force_qmm7 = k[3], kn.force_linear = k[4], kn.qmm3_min_rows = k[5];
            kn.qmm3_mode = k[6], kn.fuse_norm = k[7], kn.gemv_weighted_rows = k[8], kn.gemv_producer_ss = k[9], kn.ncu = ncu;
            print_route(kn, m, batch);
        } else {
            std::fprintf(stderr, "unknown request: %s\n", line.c_str());
            return 2;
        }
        if (!in) {
            std::fprintf(stderr, "short request: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}

// ---- check: every planner over the sweep --------------------------------------------------------------------
constexpr size_t LDS_LAUNCH_MAX = 150 * 1024;    // what every planner states for a launch (of the 160 KiB of a CU)
constexpr size_t LDS_ONE_SHOT_MAX = 100 * 1024;  // ... and the skinny matmul's one-shot grid for its slices
static bool shape_ok(int M, int N, int K, int max_rows) { return M >= 1 && M <= max_rows && N > 0 && N % 128 == 0 && K > 0 && K % 16 == 0; }

static std::set<std::tuple<int, int, int, int>> g_q3;
static std::set<std::tuple<int, int, int>> g_merge, g_qm3;
static std::set<std::pair<int, int>> g_qm3p, g_qm6, g_qm7;

static void check_qmv3(int M, int N, int K) {
    g_what = "qmv3_plan";
    const Qmv3Plan p = qmv3_plan(M, N, K);
    ++g_plans;
    if (!p.ok) return;
    const int G = N / 128, tiles = K / 16, wr = p.CW / p.KS;
    require(shape_ok(M, N, K, 8), "a plan for a shape the kernel does not take");
    require(qmv3_has_variant(p.MR, p.KS, p.CW, p.LM), "the variant is not in Q3_TABLE");
    require(p.MR >= M && (p.MR == 1 || p.MR / 2 < M), "rows per workgroup: the smallest of 1, 2, 4, 8 that holds M");
    require(p.lds <= LDS_LAUNCH_MAX && p.lds == qmv3_lds_bytes(p.MR, N, p.KS, p.CW), "LDS beyond the launch bound");
    require(p.CW % p.KS == 0 && wr >= 1, "the waves of a workgroup split into whole reduction slices");
    require(p.KS * p.LM >= G && p.KS * p.LM * 128 >= N && p.LM <= Q3_LMAX, "the reduction splits do not cover every group");
    require((long)p.blocks * wr >= tiles && tiles > (long)(p.blocks - 1) * wr, "the grid does not cover every tile exactly");
    g_q3.insert({p.MR, p.KS, p.CW, p.LM});
    if (M == 1 && qmv3_merge_has_variant(p.KS, p.CW, p.LM)) g_merge.insert({p.KS, p.CW, p.LM});
}

static void check_qmm3(int M, int N, int K, int mode, int ncu) {
    g_what = "qmm3_plan";
    g_case[4] = mode;
    const Qmm3Plan p = qmm3_plan(M, N, K, mode, ncu);
    ++g_plans;
    // (the planner's ok asks the instantiation tables since linear_plan.h: it must still be what it was -- the shape alone)
    require(p.ok == shape_ok(M, N, K, 64), "ok is no longer a matter of the shape alone: a plan without a compiled kernel");
    if (!p.ok) return;
    const int G = N / 128, tiles = K / 16;
    require(qmm3_has_variant(p.persistent, p.MB, p.persistent ? p.NU : p.TW, p.LM), "the variant is not in QM3_TABLE / QM3P_TABLE");
    require(p.MB * 16 >= M && (mode != 0 || p.persistent == 0) && (mode != 1 || p.persistent == 1), "row blocks / the pinned grid");
    require(p.lds == qmm3_lds_bytes(p.MB, p.LM) && p.lds <= (p.persistent ? LDS_LAUNCH_MAX : LDS_ONE_SHOT_MAX), "LDS beyond the planner's bound");
    require((long)p.slices * p.LM >= G && G > (long)(p.slices - 1) * p.LM, "the slices do not cover every group exactly");
    require(p.partial_bytes == (size_t)p.slices * M * K * 4, "partial_bytes is not what the slices need");
    if (p.persistent) {
        const Qmm3pGrid &g = p.pgrid;
        require(p.LM == 4 * p.NU && g.full_slices * p.LM + g.last_groups == G && g.last_groups >= 0 && g.last_groups < p.LM, "slices of 4 NU groups and a short last one");
        require(p.slices == g.full_slices + (g.last_groups ? 1 : 0), "slice count");
        require(p.grid_x == g.full_slices * g.wgs_full + g.wgs_last, "the shares do not sum to grid_x");
        if (g.full_slices) require((long)g.wgs_full * g.tpw_full >= tiles && tiles > (long)(g.wgs_full - 1) * g.tpw_full, "a full slice's workgroups do not cover every tile exactly");
        else require(g.wgs_full == 0, "workgroups for no full slice");
        if (g.last_groups) require((long)g.wgs_last * g.tpw_last >= tiles && tiles > (long)(g.wgs_last - 1) * g.tpw_last, "the last slice's workgroups do not cover every tile exactly");
        else require(g.wgs_last == 0, "workgroups for no last slice");
        require(p.grid_x <= ncu + p.slices, "more than one workgroup per CU (and one per slice for rounding) on the persistent grid");
        require(!g.full_slices || !g.last_groups || g.wgs_last <= g.wgs_full, "the short slice gets more workgroups than a full one");
        g_qm3p.insert({p.MB, p.NU});
    } else {
        require((long)p.grid_x * QM3_WAVES * p.TW >= tiles && tiles > (long)(p.grid_x - 1) * QM3_WAVES * p.TW, "the grid does not cover every tile exactly");
        g_qm3.insert({p.MB, p.TW, p.LM});
    }
}

static void check_qmm6(int M, int N, int K, bool frag, int ncu) {
    g_what = "qmm6_plan";
    g_case[4] = frag;
    const Qmm6Plan p = qmm6_plan(M, N, K, frag, ncu);
    ++g_plans;
    const int G = N / 128, tiles = K / 16, blocks16 = (M + 15) / 16;
    // every shape whose reduction fits 4 waves x 19 groups has a plan (the one-workgroup-per-CU rule chooses among candidates, it rejects none)
    require(p.ok == (shape_ok(M, N, K, 64) && G <= 4 * 19), "a shape within 4 x 19 groups without a plan, or a plan beyond it");
    if (!p.ok) return;
    require(qmm6_has_variant(p.MB, p.GPW), "the variant is not in QM6_TABLE");
    require(p.MB * p.GPW * 16 <= 320, "the fragments do not fit the registers of a wave");
    require(p.lds == qmm6_lds_bytes(p.MB, p.GPW, frag) && p.lds <= LDS_LAUNCH_MAX, "LDS beyond the launch bound");
    require(4 * p.GPW >= G && 4 * p.GPW * 128 >= N, "the four waves do not cover every group");
    require(p.MB * p.row_blocks >= blocks16 && p.MB * (p.row_blocks - 1) < blocks16, "the row blocks do not cover the rows exactly");
    const int spare = p.row_blocks > 1 ? 7 : 0;
    require((long)p.wgs * p.tiles_per_wg >= tiles && tiles > (long)(p.wgs - 1 - spare) * p.tiles_per_wg, "the grid does not cover every tile exactly");
    require(p.row_blocks == 1 || p.wgs % 8 == 0, "the workgroups of one tile range do not sit a multiple of 8 apart");
    require(p.NSETS >= 1 && p.NSETS <= p.tiles_per_wg && p.NSETS <= qmm6_sets(p.MB, p.GPW), "weight sets");
    require(4 * (QM6_RING - 1) + (p.NSETS - 1) * 2 * p.GPW <= 63, "the counted waits of the transposer do not hold 6 bits");
    g_qm6.insert({p.MB, p.GPW});
}

static void check_qmm7(int M, int N, int K, int ncu) {
    g_what = "qmm7_plan";
    const Qmm7Plan p = qmm7_plan(M, N, K, ncu);
    ++g_plans;
    if (!p.ok) return;
    const int G = N / 128, tiles = K / 16;
    require(shape_ok(M, N, K, 64), "a plan for a shape the kernel does not take");
    require(qmm7_has_variant(p.T, p.GPW), "the variant is not in QM7_TABLE");
    require(p.MB == (M + 15) / 16 && p.MB <= 4 && p.row_blocks == 1, "row blocks are exactly ceil(M / 16)");
    require(p.lds == qmm7_lds_bytes(p.MB, p.T) && p.lds <= LDS_LAUNCH_MAX, "LDS beyond the launch bound");
    require(4 * p.GPW >= G && 4 * p.GPW * 128 >= N, "the four waves do not cover every group");
    require((long)p.wgs * p.T >= tiles && tiles > (long)(p.wgs - 1) * p.T && p.wgs <= ncu, "the grid does not cover every tile exactly on one workgroup per CU");
    g_qm7.insert({p.T, p.GPW});
}

static void check_qmv(int M, int N, int K) {
    g_what = "qmv_plan";
    const QmvPlan p = qmv_plan(M, N, K);
    ++g_plans;
    require(p.MR >= std::min(M, 8) && p.WN >= 1 && p.RPL >= 1 && p.RB == 4 * (4 / p.WN) * p.RPL, "rows per workgroup");
    require((long)p.blocks * p.RB >= K && K > (long)(p.blocks - 1) * p.RB, "the grid does not cover every output row exactly");
    require(p.lds == qmv_lds_bytes(p.MR, N, p.WN, p.RPL), "LDS");
}

// the size of a table, counted over a box that holds every entry
template <typename F>
static int count4(F has, int a1, int b1, int c1, int d1) {
    int n = 0;
    for (int a = 0; a <= a1; ++a)
        for (int b = 0; b <= b1; ++b)
            for (int c = 0; c <= c1; ++c)
                for (int d = 0; d <= d1; ++d) n += has(a, b, c, d) ? 1 : 0;
    return n;
}

static void check_planners() {
    // tile counts: tests/test_decode_plans_cpu.py (test_every_compiled_gemv_variant_is_reached_by_some_shape) + every projection of MODEL_SHAPES
    std::set<int> tile_set;
    for (int t = 1; t < 64; ++t) tile_set.insert(t);
    for (int t : {96, 128, 160, 192, 256, 320, 384, 512, 608, 640, 768, 1024, 1216, 1280, 2048, 4748, 9496}) tile_set.insert(t);
    for (const Model &m : MODELS)
        for (int rows : {m.qkv_dim, m.hidden, 2 * m.inter, m.vocab}) tile_set.insert(rows / 16);
    const std::vector<int> tile_counts(tile_set.begin(), tile_set.end());
    for (int ncu : {256, 304, 64, 8})
        for (int M = 1; M <= 64; ++M)
            for (int G = 1; G <= 255; ++G)
                for (int tiles : tile_counts) {
                    const int N = G * 128, K = tiles * 16;
                    g_case[0] = M, g_case[1] = N, g_case[2] = K, g_case[3] = ncu, g_case[4] = 0;
                    if (ncu == 256 && M <= 8) check_qmv3(M, N, K), check_qmv(M, N, K);  // (no CU count in the GEMV plans)
                    // the full grid at 256 CUs; elsewhere the row counts at which a planner changes its mind
                    if (ncu != 256 && !(M % 16 <= 1 || M == 5 || M == 8 || M == 9)) continue;
                    for (int mode = -1; mode <= 1; ++mode) check_qmm3(M, N, K, mode, ncu);
                    if (G <= 80) check_qmm6(M, N, K, false, ncu), check_qmm6(M, N, K, true, ncu), check_qmm7(M, N, K, ncu);
                }
    // shapes no kernel takes have no plan
    g_what = "refusals";
    for (int ncu : {256, 64}) {
        require(!qmv3_plan(1, 2560, 100).ok && !qmv3_plan(9, 2560, 2560).ok && !qmv3_plan(0, 2560, 2560).ok && !qmv3_plan(1, 100, 2560).ok, "qmv3_plan");
        require(!qmm3_plan(65, 2560, 2560, -1, ncu).ok && !qmm3_plan(8, 2560, 100, -1, ncu).ok && !qmm3_plan(8, 100, 2560, -1, ncu).ok, "qmm3_plan");
        require(!qmm6_plan(65, 2560, 2560, false, ncu).ok && !qmm6_plan(8, 2560, 100, false, ncu).ok && !qmm6_plan(8, 100, 2560, false, ncu).ok &&
                    !qmm6_plan(8, 77 * 128, 2560, false, ncu).ok, "qmm6_plan");
        require(!qmm7_plan(65, 2560, 6144, ncu).ok && !qmm7_plan(8, 2560, 100, ncu).ok && !qmm7_plan(8, 100, 2560, ncu).ok, "qmm7_plan");
    }
    // every table: its size as pinned here, every entry reached by some swept shape, nothing outside it returned (held plan by plan above)
    g_what = "tables";
    auto report = [](const char *table, size_t reached, int size) {
        if ((int)reached != size) std::printf("%s: %zu of %d entries reached by the sweep\n", table, reached, size);
    };
    const int n_q3 = count4(qmv3_has_variant, 16, 16, 16, 16);
    const int n_merge = count4([](int ks, int cw, int lm, int) { return qmv3_merge_has_variant(ks, cw, lm); }, 16, 16, 16, 0);
    const int n_qm3 = count4([](int mb, int tw, int lm, int) { return qmm3_has_variant(0, mb, tw, lm); }, 8, 8, 16, 0);
    const int n_qm3p = count4([](int mb, int nu, int lm, int) { return qmm3_has_variant(1, mb, nu, lm); }, 8, 8, 16, 0);
    const int n_qm6 = count4([](int mb, int gpw, int, int) { return qmm6_has_variant(mb, gpw); }, 8, 32, 0, 0);
    const int n_qm7 = count4([](int t, int gpw, int, int) { return qmm7_has_variant(t, gpw); }, 16, 32, 0, 0);
    require(n_q3 == 53 && n_merge == 10 && n_qm3 == 11 && n_qm3p == 8 && n_qm6 == 12 && n_qm7 == 2, "an instantiation table lost or gained an entry");
    report("Q3_TABLE", g_q3.size(), n_q3), report("Q3_MERGE_TABLE", g_merge.size(), n_merge), report("QM3_TABLE", g_qm3.size(), n_qm3);
    report("QM3P_TABLE", g_qm3p.size(), n_qm3p), report("QM6_TABLE", g_qm6.size(), n_qm6), report("QM7_TABLE", g_qm7.size(), n_qm7);
    require((int)g_q3.size() == n_q3 && (int)g_merge.size() == n_merge && (int)g_qm3.size() == n_qm3 && (int)g_qm3p.size() == n_qm3p &&
                (int)g_qm6.size() == n_qm6 && (int)g_qm7.size() == n_qm7, "a compiled variant no swept shape reaches");
}

// ---- check: the routing ----------------------------------------------------------------------------------------
// does the GEMV path hold a plan for M rows of this matrix (engine_qmv: passes of at most 8 rows, halved until one fits)?
static bool gemv_route_ok(const ProjShape &w, int M) {
    for (int step = std::min(M, 8); step >= 1; step = step > 1 ? (step + 1) / 2 : 0)
        if ((w.tiled && qmv3_plan(step, w.cols, w.rows).ok) || qmv_plan(step, w.cols, w.rows).lds <= LDS_LAUNCH_MAX) return true;
    return false;
}

static void check_route(const LinearKnobs &k, const Model &m, int batch, bool defaults) {
    const LayerShapes w = layer_of(m);
    const ProjShape head = head_of(m);
    const LayerRoute r = plan_layer(k, w, batch, false);
    const bool gemv = gemv_takes_rows(k, batch);
    g_case[0] = batch, g_case[1] = m.hidden, g_case[2] = m.inter, g_case[3] = k.ncu, g_case[4] = k.force_linear;
    g_what = m.name;
    g_plans += 12;  // the plans behind the predicates of one layer's route
    // the GEMV's rows, stated from the options' own descriptions
    require(k.force_linear != 1 || gemv, "kernel 1 names the GEMV");
    require(k.force_linear != 2 || !gemv, "kernels 2 .. 4 name the skinny matmul");
    require(k.force_linear != 0 || gemv == (batch < k.qmm3_min_rows || (batch <= 8 && !k.use_qmm3)), "the GEMV takes the rows below qmm3_min_rows, and up to 8 without the skinny matmul");
    const ProjShape all[5] = {w.wqkv, w.wo, w.wgu, w.wdown, head};
    for (const ProjShape &p : all) {
        const bool t6 = qmm6_takes(k, p, batch), t3 = takes_skinny_matmul(k, p, batch);
        require(!t6 || (k.use_qmm6 && k.force_linear == 0 && batch >= k.qmm3_min_rows && qmm6_plan(batch, p.cols, p.rows, false, k.ncu).ok), "qmm6_takes without its option or its plan");
        require(!t6 || qmm6_plan(batch, p.cols, p.rows, true, k.ncu).ok, "qmm6_takes, but rows in fragment order have no plan");
        require(!t3 || (k.use_qmm3 && !gemv && qmm3_plan(batch, p.cols, p.rows, k.qmm3_mode, k.ncu).ok), "takes_skinny_matmul without its option or its plan");
    }
    require(!r.batched || (qmm6_takes(k, w.wgu, batch) && (r.wo6 || takes_skinny_matmul(k, w.wo, batch))), "a batched layer whose gate|up or wo has no kernel for weighted rows");
    require(!r.wo6 || qmm6_takes(k, w.wo, batch), "wo6 without a plan");
    require(!r.qkv6 || qmm6_takes(k, w.wqkv, batch), "qkv6 without a plan");
    require(r.down != LayerRoute::DOWN_QMM6 || (qmm6_takes(k, w.wdown, batch) && !(takes_skinny_matmul(k, w.wdown, batch) && k.fuse_norm)), "w_down on qmm6 without a plan, or past the sliced matmul");
    require(r.down != LayerRoute::DOWN_SLICED_WEIGHTED || (takes_skinny_matmul(k, w.wdown, batch) && k.fuse_norm && m.hidden <= QM3_SS * 1024), "w_down leaves weighted rows without the sliced matmul's plan");
    require(r.batched_written_once() == (r.batched && r.qkv6 && r.down != LayerRoute::DOWN_ROUTER), "batched_written_once");
    require(!r.gemv_weighted || (gemv && batch <= 8 && k.gemv_weighted_rows && k.gemv_producer_ss && qmv3_plan(batch, w.wo.cols, w.wo.rows).ok && qmv3_plan(batch, w.wgu.cols, w.wgu.rows).ok),
            "weighted rows between GEMVs that are not both single-pass MFMA GEMVs");
    for (int ns : {1, 2, 3, 4, 8, 16}) {
        const bool mg = wo_merge_applicable(k, w.wo, batch, ns, 128, m.q_dim / 128);
        const Qmv3Plan p1 = qmv3_plan(1, w.wo.cols, w.wo.rows);
        require(!mg || (batch == 1 && (ns == 2 || ns == 4 || ns == 8) && k.force_linear == 0 && gemv && p1.ok && p1.MR == 1 && qmv3_merge_has_variant(p1.KS, p1.CW, p1.LM) &&
                        w.wo.cols / 8 <= 2 * p1.CW * 64),
                "the wo GEMV merges attention partials without a compiled kernel for its plan");
        require(!wo_merge_applicable(k, w.wo, batch, ns, 64, m.q_dim / 64), "merging heads that are not 128 wide");
    }
    const bool frag = rows_travel_in_fragment_order(k, w, batch);
    require(batch <= 8 || frag, "rows travel in fragment order from 9 rows");
    require(batch > 8 || !frag || (k.use_qmm7 && qmm7_plan(batch, w.wgu.cols, w.wgu.rows, k.ncu).ok && qmm7_plan(batch, w.wqkv.cols, w.wqkv.rows, k.ncu).ok),
            "fragment order at up to 8 rows without the row-streaming matmul as the consumer");
    if (!defaults) return;
    // default knobs: every projection -- and the lm_head -- resolves to a kernel whose plan is ok, as the engine walks the route
    if (gemv) {
        for (const ProjShape &p : all) require(gemv_route_ok(p, batch), "no GEMV plan");
    } else {
        require(batch >= 5 && batch <= 64, "rows beyond the batched routes");
        require((r.batched && r.qkv6) || takes_skinny_matmul(k, w.wqkv, batch), "qkv has no kernel");
        require((r.batched && r.wo6) || takes_skinny_matmul(k, w.wo, batch), "wo has no kernel");
        require(r.batched || takes_skinny_matmul(k, w.wgu, batch), "gate|up has no kernel");
        require((r.batched && r.down == LayerRoute::DOWN_QMM6) || takes_skinny_matmul(k, w.wdown, batch), "w_down has no kernel");
        require(qmm6_takes(k, head, batch) || takes_skinny_matmul(k, head, batch), "lm_head has no kernel");
    }
}

static void check_routing() {
    std::vector<std::string> not_batched;
    for (const Model &m : MODELS)
        for (int ncu : {256, 304, 64})
            for (int batch = 1; batch <= 64; ++batch) {
                LinearKnobs k;
                k.ncu = ncu;
                check_route(k, m, batch, true);
                if (ncu != 256) continue;
                const LayerRoute r = plan_layer(k, layer_of(m), batch, false);
                if (batch >= 5 && !r.batched_written_once()) not_batched.push_back(std::string(m.name) + " at " + std::to_string(batch));
                // Qwen3-4B: the batched hand-over on per-layer buffers at every row count the GEMV does not take, the route the AQL replay needs
                if (m.hidden == 2560) require(r.batched_written_once() == (batch >= 5), "batched_written_once at Qwen3-4B shapes");
                if (m.hidden == 2560 && batch >= 5) require(r.qkv6 && r.wo6 && r.down == LayerRoute::DOWN_SLICED_WEIGHTED && !r.gemv_weighted, "the route of a Qwen3-4B layer");
                if (m.hidden == 2560 && batch < 5) require(r.gemv_weighted && !r.batched, "the GEMV route of a Qwen3-4B layer");
            }
    // (the widths that leave the batched, written-once route at some batch: a hole in a planner shows here)
    for (const std::string &s : not_batched) std::fprintf(stderr, "not on the batched written-once route: %s rows\n", s.c_str());
    g_what = "routing";
    require(not_batched.empty(), "a dense model leaves the batched written-once route at 5 .. 64 rows");
    // the knob combinations the engine options, TL_QMM3_MIN_M and the kernel numbers of tl_decode_linear can produce
    for (const Model &m : MODELS)
        for (int bits = 0; bits < 64; ++bits)
            for (int force = 0; force <= 2; ++force)
                for (int min_rows : {1, 5, 9})
                    for (int mode = -1; mode <= 1; ++mode) {
                        LinearKnobs k;
                        k.use_qmm3 = bits & 1, k.use_qmm6 = bits & 2, k.use_qmm7 = bits & 4, k.fuse_norm = bits & 8, k.gemv_weighted_rows = bits & 16, k.gemv_producer_ss = bits & 32;
                        k.force_linear = force, k.qmm3_min_rows = min_rows, k.qmm3_mode = mode;
                        if (mode >= 0 && (bits & 56) != 56) continue;  // a pinned grid comes through the entry points: the engine's twins stay on
                        for (int batch : {1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 40, 48, 49, 64}) check_route(k, m, batch, false);
                    }
    // a MoE layer, a layer without a dense MLP: no route of this record
    g_what = "plan_layer";
    LayerShapes none = layer_of(MODELS[2]);
    const LayerRoute moe = plan_layer(LinearKnobs{}, none, 16, true);
    none.dense_mlp = false;
    const LayerRoute bare = plan_layer(LinearKnobs{}, none, 16, false);
    require(!moe.batched && !moe.qkv6 && !moe.wo6 && !moe.gemv_weighted && moe.down == LayerRoute::DOWN_ROUTER && !bare.batched && !bare.qkv6, "a MoE layer has no dense route");
    require(!rows_travel_in_fragment_order(LinearKnobs{}, none, 8) && rows_travel_in_fragment_order(LinearKnobs{}, none, 9), "fragment order without a dense first layer");
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plans") return run_plans();
    if (mode != "check") {
        std::fprintf(stderr, "usage: linear_plan_check plans|check\n");
        return 2;
    }
    check_planners();
    check_routing();
    std::printf("ok plans=%ld checks=%ld\n", g_plans, g_checks);
    return 0;
}
