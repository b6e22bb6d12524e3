// The plans of the decode projections (host only: no device header, no project header -- plain g++ compiles it, and
// tests/linear_plan_check.cpp sweeps it under ASan / UBSan): the instantiation tables of the four projection kernels, written once each
// (the .hip launchers generate their dispatch from them, the *_has_variant predicates below their answers); the LDS sizes the kernels and
// their planners share; every plan record with its planner; and the routing -- which kernel takes one projection of M rows under the knobs
// an engine or an entry point set (LinearKnobs), the route of a layer (LayerRoute).  A planner reads its arguments and nothing else: the
// CU count is one of them (the engine and the entry points ask qmm3_num_cus() once).  tests/golden/linear_plans.json holds what the planners
// answered when they sat at the bottom of the kernel headers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace tl {

enum { PRO_NONE = 0, PRO_RMSNORM = 1, PRO_ATTN_MERGE = 2, PRO_RMS_WEIGHTED = 3 };  // the last two: qmv3.h only (Qmv3Args::merge_ws / ::ss_in)
enum { EPI_STORE = 0, EPI_RESIDUAL = 1, EPI_SWIGLU = 2 };

// ---- the packed-dot GEMV (qmv.h) ---------------------------------------------------------------------------
constexpr size_t qmv_lds_bytes(int MR, int N, int WN, int RPL) {
    size_t x = (size_t)MR * N * 2;
    size_t as = (size_t)MR * (N / 32) * 4;
    size_t red = WN > 1 ? (size_t)4 * RPL * 4 * MR * 4 : 0;  // [waves][RPL*4 rows][MR]
    return x + as + red + 64;
}

// Host-side launch heuristic shared by the operator and the decode fast path.
struct QmvPlan {
    int MR, WN, RPL, RB, blocks;
    size_t lds;
};
inline QmvPlan qmv_plan(int M, int N, int K) {
    QmvPlan pl;
    pl.MR = M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : 8));
    const int J = (N + 511) / 512;
    // rows per workgroup: largest tile that still yields >= 3 workgroups per CU
    // (256 CUs); small K falls back to splitting the reduction over the waves.
    int rb = 4;
    const int cands[3] = {32, 16, 8};
    for (int c : cands) {
        if ((K + c - 1) / c >= 768) {
            rb = c;
            break;
        }
    }
    if (rb == 32) {
        pl.WN = 1; pl.RPL = 2;
    } else if (rb == 16) {
        pl.WN = 1; pl.RPL = 1;
    } else if (rb == 8) {
        pl.WN = 2; pl.RPL = 1;
    } else {
        pl.WN = 4; pl.RPL = 1;
    }
    if (pl.WN > J) {  // not enough 512-column chunks to split: keep waves on rows
        pl.WN = J >= 2 ? 2 : 1;
        pl.RPL = 1;
    }
    pl.RB = 4 * (4 / pl.WN) * pl.RPL;
    pl.blocks = (K + pl.RB - 1) / pl.RB;
    pl.lds = qmv_lds_bytes(pl.MR, N, pl.WN, pl.RPL);
    return pl;
}

// ---- the MFMA GEMV over the tiled layout (qmv3.h) -----------------------------------------------------------
constexpr int Q3_LMAX = 10;  // most groups (1 KiB wave-loads) per compute wave; kernels are specialised on LM <= Q3_LMAX
constexpr int Q3_PAD = 8;    // bf16 elements of padding per activation row in LDS

// LDS: activation rows [MR][N + Q3_PAD] bf16, then Q3_LMAX zero groups (a wave's fixed-length body may run past the
// end of the row: it then reads finite data it multiplies by a zero scale); per-group sums [G + Q3_LMAX][16] fp32;
// split-K partials.
constexpr size_t qmv3_lds_xsum_off(int MR, int N) {
    return (((size_t)MR * (N + Q3_PAD) + (size_t)Q3_LMAX * 128) * 2 + 15) & ~(size_t)15;
}
constexpr size_t qmv3_lds_red_off(int MR, int N) {
    return qmv3_lds_xsum_off(MR, N) + (size_t)(N / 128 + Q3_LMAX) * 16 * 4;
}
constexpr size_t qmv3_lds_bytes(int MR, int N, int KS, int CW) {
    size_t red = KS > 1 ? (size_t)CW * MR * 16 * 4 : 0;
    return qmv3_lds_red_off(MR, N) + red + (size_t)MR * CW * 4 + 64;  // + RMSNorm partial sums of squares
}

// The instantiation table, written once: Q3_TABLE(X) expands X(MR, KS, CW, LM) for every compiled combination -- exactly the
// combinations qmv3_plan can return (round 5: the 45 of 98 that no shape reaches -- 8-wave workgroups with 2 / 4 reduction splits,
// 8 splits with 4 / 5 groups per wave, 8 rows on the finer cut of 1-4 rows -- are gone: 231 kernels; tests/linear_plan_check.cpp
// sweeps the planner and fails on an entry nothing reaches).  Laboratories instantiate what they sweep themselves (tools/lab/plan_lab.hip).
//   1 / 2 / 4 / 8 rows x {1, 2, 4 reduction splits on 4 waves} x {4, 5, 8, 10 groups per wave} (8 rows: 2 / 4 splits only beyond 10 groups,
//   i.e. 8 or 10 per wave -- the finer cut of short reductions is a rule for 1-4 rows); 8 splits on 8 waves with 8 or 10 groups per wave
//   (8 splits mean more than 40 groups; four rows over 65-80 groups go to 16 waves instead); 4 rows x 16 splits on 16 waves x {4, 5}.
#define Q3_LM4(X, MRv, KSv, CWv) X(MRv, KSv, CWv, 4) X(MRv, KSv, CWv, 5) X(MRv, KSv, CWv, 8) X(MRv, KSv, CWv, 10)
#define Q3_LMHI(X, MRv, KSv, CWv) X(MRv, KSv, CWv, 8) X(MRv, KSv, CWv, 10)
#define Q3_TABLE(X)                                                                                                     \
    Q3_LM4(X, 1, 1, 4) Q3_LM4(X, 1, 2, 4) Q3_LM4(X, 1, 4, 4) Q3_LMHI(X, 1, 8, 8)                                        \
    Q3_LM4(X, 2, 1, 4) Q3_LM4(X, 2, 2, 4) Q3_LM4(X, 2, 4, 4) Q3_LMHI(X, 2, 8, 8)                                        \
    Q3_LM4(X, 4, 1, 4) Q3_LM4(X, 4, 2, 4) Q3_LM4(X, 4, 4, 4) X(4, 8, 8, 8)                                              \
    X(4, 16, 16, 4) X(4, 16, 16, 5) /* qmv3_plan: four rows over a long reduction (8 x <= 10 groups cut 16 x <= 5) */   \
    Q3_LM4(X, 8, 1, 4) Q3_LMHI(X, 8, 2, 4) Q3_LMHI(X, 8, 4, 4) Q3_LMHI(X, 8, 8, 8)
// PRO_ATTN_MERGE + EPI_RESIDUAL, one row (the wo projection reading the decode-attention split partials): Q3_MERGE_TABLE(X) expands
// X(KS, CW, LM) for the plans a single row takes -- 4 waves with 2- or 4-way, 8 waves with 8-way reduction splits (8 splits mean more than
// 40 groups: 8 or 10 per wave) -- each compiled for 2 / 4 / 8 attention splits
#define Q3_MERGE_LM4(X, KSv, CWv) X(KSv, CWv, 4) X(KSv, CWv, 5) X(KSv, CWv, 8) X(KSv, CWv, 10)
#define Q3_MERGE_TABLE(X) Q3_MERGE_LM4(X, 2, 4) Q3_MERGE_LM4(X, 4, 4) X(8, 8, 8) X(8, 8, 10)

inline bool qmv3_has_variant(int MR, int KS, int CW, int LM) {
#define Q3_MEMBER(MRv, KSv, CWv, LMv) if (MR == MRv && KS == KSv && CW == CWv && LM == LMv) return true;
    Q3_TABLE(Q3_MEMBER)
#undef Q3_MEMBER
    return false;
}
inline bool qmv3_merge_has_variant(int KS, int CW, int LM) {
#define Q3_MEMBER(KSv, CWv, LMv) if (KS == KSv && CW == CWv && LM == LMv) return true;
    Q3_MERGE_TABLE(Q3_MEMBER)
#undef Q3_MEMBER
    return false;
}

struct Qmv3Plan {
    int MR, KS, CW, LM, blocks;
    size_t lds;
    bool ok;
};
inline int qmv3_round_lm(int lper) { return lper <= 4 ? 4 : (lper <= 5 ? 5 : (lper <= 8 ? 8 : Q3_LMAX)); }
inline Qmv3Plan qmv3_plan(int M, int N, int K, int force_ks = 0, int force_cw = 0) {
    Qmv3Plan pl{};
    pl.MR = M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : 8));
    const int G = N / 128;
    const int tiles = K / 16;
    int ks = 1;
    while (ks < 8 && (G + ks - 1) / ks > Q3_LMAX) ks *= 2;
    {
        // a grid of 1 .. 4 workgroups per CU with a ragged last round (gate|up: 608 workgroups on 256 CUs = 3 rounds for
        // 2.4 rounds of work) runs faster cut twice as fine (measured 7.3 -> 6.9 us); smaller and larger grids do not.
        // Up to 4 rows since round 3 (tools/lab/plan_lab, gate|up with weighted rows: 2 rows 8.32 -> 7.47 us, 4 rows 10.05 -> 9.39;
        // qkv and wo do not meet the condition and would lose: profiles/r03_labs/gemv_plan_sweep_rows_1_2_4.log)
        const int blocks = (tiles + (4 / ks) - 1) / (4 / (ks > 4 ? 4 : ks));
        const double x = blocks / 256.0;
        const double rounds = (double)(int)(x + 0.999999);
        if (M <= 4 && ks < 4 && x >= 1.0 && x < 4.0 && rounds / x > 1.2 && (G + 2 * ks - 1) / (2 * ks) >= 4) ks *= 2;
    }
    // four rows over a long reduction (w_down: 76 groups): 16 waves with 5 groups each stage the 4 x 9,728 activations and run
    // their chains twice as fast as 8 waves with 10 (tools/lab/plan_lab: 9.50 -> 7.65 us; at 1 / 2 rows the 8-wave cut wins,
    // 5.66 / 6.27 against 5.86 / 6.58)
    // (only where a 16-wave kernel exists: 4 or 5 groups per wave, i.e. reductions of up to 80 groups; longer ones keep 8 waves)
    if (pl.MR == 4 && ks == 8 && (G + 15) / 16 >= 4 && (G + 15) / 16 <= 5) ks = 16;
    if (force_ks > 0) ks = force_ks;
    pl.KS = ks;
    pl.CW = ks >= 8 ? ks : 4;
    if (force_cw > 0 && force_cw >= ks) pl.CW = force_cw;
    pl.LM = qmv3_round_lm((G + ks - 1) / ks);
    const int wr = pl.CW / pl.KS;
    pl.blocks = (tiles + wr - 1) / wr;
    pl.lds = qmv3_lds_bytes(pl.MR, N, pl.KS, pl.CW);
    // ok = the shape fits AND a kernel is compiled for (MR, KS, CW, LM): everything else goes to the packed-dot GEMV (qmv.h)
    pl.ok = K > 0 && K % 16 == 0 && N % 128 == 0 && M >= 1 && M <= 8 && (G + ks - 1) / ks <= Q3_LMAX &&
            pl.lds <= 150 * 1024 && qmv3_has_variant(pl.MR, pl.KS, pl.CW, pl.LM);
    return pl;
}

// PRO_RMS_WEIGHTED: the row must sit in the staging registers of one pass and its sums of squares in one 16-byte load per lane
inline bool qmv3_takes_weighted_rows(const Qmv3Plan &pl, int N, int ss_n) {
    return pl.ok && N / 8 <= (pl.MR <= 2 ? 3 : 2) * pl.CW * 64 && ss_n > 0 && ss_n <= 256 && (ss_n & 3) == 0;
}

// ---- the K-sliced skinny matmul (qmm3.h) --------------------------------------------------------------------
constexpr int QM3_WAVES = 8;
// The staged rows are NOT padded: a 128-element group is exactly one 64-bank row, and the 16-byte chunks inside it are
// XOR-swizzled by the row so that every ds_read_b128 service group ({0-3,12-15,20-27}, ...: MI355X_MICROARCH.md, LDS) hits 16
// different bank quads -- chunk j of row r sits at j ^ sw(r), sw(r) = (r & 15) ^ (4 if 4 <= (r & 15) < 12).  A padded row
// stride cannot do that for this lane -> (row, k-block) map (r02 lab: gate|up at 64 rows 29.1 -> 27.5 us).
constexpr int QM3_PAD = 0;  // bf16 elements of padding per staged activation row
constexpr int QM3_SS = 8;   // partial sums of squares kept per activation row (unused entries are zero)
constexpr int QM3_SS_MAX = 256;

constexpr size_t qmm3_lds_bytes(int MB, int LM) {
    return (size_t)MB * 16 * (LM * 128 + QM3_PAD) * 2 + (size_t)LM * MB * 16 * 4 + (size_t)MB * 16 * 4;  // rows, group sums, 1 / rms per row
}

// The instantiation tables, written once: QM3_TABLE(X) expands X(MB, TW, LM) for every compiled one-shot kernel (16-row blocks, tiles
// per wave, groups per slice), QM3P_TABLE(X) X(MB, NU) for every persistent one (units of 4 groups per slice), each with and without
// the fused RMSNorm
#define QM3_LM4(X, MBv, TWv) X(MBv, TWv, 4) X(MBv, TWv, 5) X(MBv, TWv, 8) X(MBv, TWv, 10)
#define QM3_TABLE(X) QM3_LM4(X, 1, 1) QM3_LM4(X, 2, 1) X(4, 1, 4) X(4, 1, 5) X(4, 2, 4)
#define QM3P_TABLE(X) X(1, 1) X(1, 2) X(2, 1) X(2, 2) X(3, 1) X(3, 2) X(4, 1) X(4, 2)

// persistent: (MB, NU) with LM = 4 NU; one-shot: (MB, TW, LM)
inline bool qmm3_has_variant(int persistent, int MB, int TW_or_NU, int LM) {
#define QM3_MEMBER(MBv, TWv, LMv) if (!persistent && MB == MBv && TW_or_NU == TWv && LM == LMv) return true;
    QM3_TABLE(QM3_MEMBER)
#undef QM3_MEMBER
#define QM3_MEMBER(MBv, NUv) if (persistent && MB == MBv && TW_or_NU == NUv && LM == 4 * NUv) return true;
    QM3P_TABLE(QM3_MEMBER)
#undef QM3_MEMBER
    return false;
}

struct Qmm3pGrid {
    int full_slices, wgs_full, tpw_full;  // slices of 4*NU groups: workgroups and tiles per workgroup of each
    int last_groups, wgs_last, tpw_last;  // the short last slice (0 groups = none)
};
struct Qmm3Plan {
    int MB, TW, LM, slices, tile_groups;
    int grid_x;        // one-shot: tile groups (one workgroup per (tile group, slice)); persistent: workgroups per slice
    int persistent;    // 0: qmm3_kernel, 1: qmm3p_kernel (one workgroup per CU walking tiles_per_wg tiles)
    int tiles_per_wg;  // persistent grids only
    int NU;            // qmm3p_kernel only: units (4 groups) per slice
    Qmm3pGrid pgrid;   // qmm3p_kernel only
    size_t lds, partial_bytes;
    bool ok;
};

// mode 0: the one-shot grid, LM the largest of {10, 8, 5, 4} whose slice fits the LDS and that still yields about one
// workgroup per CU.  mode 1: the persistent grid.  mode -1: by shape, from the r02 lab (profiles/r02_labs/qmm3_lab_r02*.log,
// matmul + slice reduction): the persistent grid wins where a CU has several tiles to walk -- gate|up (1,216 tiles) at any
// row count, lm_head (9,496) from 17 rows, w_down (76 groups: 10 slices instead of 16-19) from 17 rows -- and loses on the
// small projections (qkv, wo: 3-4 tiles per workgroup, the staged slice is most of the kernel) and on lm_head at <= 16 rows
// (two 10-group slices fit the one-shot grid there).  tl_decode_linear's kernel 3 / 4 pin a grid through `mode`.
inline bool qmm3_prefers_persistent(int MB, int G, int tiles) {
    if (MB >= 2) return tiles >= 1024 || G >= 64;
    return tiles >= 1024 && tiles < 4096;
}
inline Qmm3Plan qmm3_plan(int M, int N, int K, int mode, int ncu) {
    Qmm3Plan pl{};
    pl.ok = M >= 1 && M <= 64 && N > 0 && N % 128 == 0 && K > 0 && K % 16 == 0;
    if (!pl.ok) return pl;
    pl.MB = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
    const int G = N / 128, tiles = K / 16;
    if (mode < 0) mode = qmm3_prefers_persistent(pl.MB, G, tiles) ? 1 : 0;
    if (mode == 1) {
        // 33-48 rows: THREE row blocks on the persistent grid (round 6: a 48-row slice is 96 KiB of LDS instead of 128, 12 MFMAs per k-step pair instead of
        // 16 -- w_down at 33-48 rows cost what 64 rows cost)
        if (M > 32 && M <= 48) pl.MB = 3;
        // slices of 8 groups (two units) where the LDS holds them, workgroups shared out in proportion to the groups of a slice
        int nu = qmm3_lds_bytes(pl.MB, 8) <= 150 * 1024 && G > 4 ? 2 : 1;
        pl.NU = nu;
        pl.LM = 4 * nu;
        Qmm3pGrid &gr = pl.pgrid;
        gr.full_slices = G / pl.LM;
        gr.last_groups = G - gr.full_slices * pl.LM;
        pl.slices = gr.full_slices + (gr.last_groups ? 1 : 0);
        auto share = [&](int groups, int &wgs, int &tpw) {
            wgs = std::min(std::max(1, (int)((long)ncu * groups / G)), tiles);
            tpw = (tiles + wgs - 1) / wgs;
            wgs = (tiles + tpw - 1) / tpw;
        };
        gr.wgs_full = gr.tpw_full = gr.wgs_last = gr.tpw_last = 0;
        if (gr.full_slices) share(pl.LM, gr.wgs_full, gr.tpw_full);
        if (gr.last_groups) share(gr.last_groups, gr.wgs_last, gr.tpw_last);
        pl.grid_x = gr.full_slices * gr.wgs_full + gr.wgs_last;
        pl.tiles_per_wg = gr.full_slices ? gr.tpw_full : gr.tpw_last;
        pl.persistent = 1;
        pl.TW = 1;
        pl.tile_groups = (tiles + QM3_WAVES - 1) / QM3_WAVES;
    } else {
        pl.TW = (pl.MB == 4 && tiles >= 2048) ? 2 : 1;
        pl.tile_groups = (tiles + QM3_WAVES * pl.TW - 1) / (QM3_WAVES * pl.TW);
        const int cand[4] = {10, 8, 5, 4};
        pl.LM = 4;
        for (int lm : cand) {
            if (qmm3_lds_bytes(pl.MB, lm) > 100 * 1024) continue;
            if (pl.MB == 4 && pl.TW == 2 && lm == 5) continue;  // 64 rows x 2 tiles per wave x 5 groups spilled 14 VGPRs: removed in round 3
            const int slices = (G + lm - 1) / lm;
            pl.LM = lm;
            if ((long)slices * pl.tile_groups >= 192 || lm == 4) break;
        }
        pl.slices = (G + pl.LM - 1) / pl.LM;
        pl.grid_x = pl.tile_groups;
    }
    pl.lds = qmm3_lds_bytes(pl.MB, pl.LM);
    pl.partial_bytes = (size_t)pl.slices * M * K * 4;
    pl.ok = qmm3_has_variant(pl.persistent, pl.MB, pl.persistent ? pl.NU : pl.TW, pl.LM);  // a kernel is compiled for the answer
    return pl;
}
// the slice reduction leaves [M][QM3_SS] partial sums of squares of its bf16 output rows (EPI_STORE / EPI_RESIDUAL with K <= QM3_SS * 1024)
inline bool qmm3_reduce_can_emit_ss(int epi, int K) { return epi != EPI_SWIGLU && K % 4 == 0 && (K / 4 + 255) / 256 <= QM3_SS; }
// the fused RMSNorm of the skinny matmul takes any ss_n the staging prologue can fetch in four 16-byte loads per lane
inline bool qmm3_takes_ss(int ss_n) { return ss_n > 0 && ss_n <= QM3_SS_MAX && ss_n % 4 == 0; }

// ---- the register-resident matmul (qmm6.h) ------------------------------------------------------------------
constexpr int QM6_WAVES = 4;
// 4-KiB units (16 rows x one group) of a wave's transposer ring, and how many units back a slot is re-used: 8 slots, 5 units (20 KiB per
// wave, 80 per CU) in flight.  (Two workgroups per CU with half the ring and half the register file were measured and lost at every
// row count but lm_head at 8-16 rows: profiles/r04_labs/README.md.)
constexpr int QM6_RING = 8;
constexpr int QM6_SS_MAX = 256;  // partial sums of squares per row the prologue can fetch (16 lanes x 4 x 16 bytes)

// LDS: the four waves' transposer rings -- re-used, once every wave holds its fragments, for a tile's partial sums x 2 --, the
// per-(row, group) sums, 1 / rms per row
// (rows in fragment order need no rings: only the tiles' partial sums live there)
constexpr size_t qmm6_lds_ring_bytes(int MB, bool frag) { return frag ? (size_t)2 * QM6_WAVES * MB * 1024 : (size_t)QM6_WAVES * QM6_RING * 4096; }
constexpr size_t qmm6_lds_bytes(int MB, int GPW, bool frag = false) {
    return qmm6_lds_ring_bytes(MB, frag) + (size_t)QM6_WAVES * GPW * MB * 64 + (size_t)MB * 16 * 4;
}

// The instantiation table, written once: QM6_TABLE(X) expands X(MB, GPW) for every compiled pair: the register file of one wave per
// SIMD holds MB x GPW x 16 fragment registers (every entry within 320: asserted below, so the planner asks the table alone)
#define QM6_TABLE(X) X(1, 2) X(1, 4) X(1, 5) X(1, 8) X(1, 19) X(2, 2) X(2, 4) X(2, 5) X(2, 8) X(4, 2) X(4, 4) X(4, 5)
#define QM6_MEMBER(MBv, GPWv) static_assert(MBv * GPWv * 16 <= 320, "the fragments of a wave fit its registers");
QM6_TABLE(QM6_MEMBER)
#undef QM6_MEMBER
inline bool qmm6_has_variant(int MB, int GPW) {
#define QM6_MEMBER(MBv, GPWv) if (MB == MBv && GPW == GPWv) return true;
    QM6_TABLE(QM6_MEMBER)
#undef QM6_MEMBER
    return false;
}

struct Qmm6Plan {
    int MB, GPW, NSETS, row_blocks, wgs, tiles_per_wg;
    size_t lds;
    bool ok;
};
// weight sets of a workgroup that walks several tiles: tiles in flight ahead of the one computed = sets - 1, as many as the registers
// next to the fragments hold (a tile of few rows computes in a fraction of the memory latency) and the 6-bit vmcnt counts behind the
// first ring of units (4 (RING - 1) + (sets - 1) 2 GPW <= 63)
constexpr int qmm6_sets(int MB, int GPW) { return GPW > 8 ? 1 : (MB * GPW <= 5 ? 4 : (MB * GPW <= 10 ? 3 : 2)); }
// sets for a workgroup of `tpw` tiles: whole rounds of `sets` tiles run in the branch-free loop, the rest behind it (qmm6_kernel)
inline int qmm6_pick_sets(int MB, int GPW, int tpw) { return std::min(tpw, qmm6_sets(MB, GPW)); }
inline int qmm6_round_gpw(int gpw) { return gpw <= 2 ? 2 : (gpw <= 4 ? 4 : (gpw <= 5 ? 5 : (gpw <= 8 ? 8 : 19))); }
inline Qmm6Plan qmm6_plan(int M, int N, int K, bool frag, int ncu) {
    Qmm6Plan pl{};
    if (M < 1 || M > 64 || N <= 0 || N % 128 != 0 || K <= 0 || K % 16 != 0) return pl;
    const int G = N / 128, tiles = K / 16;
    if ((G + QM6_WAVES - 1) / QM6_WAVES > 19) return pl;
    pl.GPW = qmm6_round_gpw((G + QM6_WAVES - 1) / QM6_WAVES);
    // Row blocks per workgroup (MB = 1, 2 or 4 blocks of 16 rows; the rows beyond go to further workgroups over the same tiles).  Until round 6: the largest
    // block whose fragments fit the registers.  But what a workgroup costs is what its CU pulls -- MB x 16 rows of N columns + its tiles' weights, at ~13.5 ns
    // per KiB (the L2 -> CU path, profiles/r05_labs) -- plus its walk (a tile: the four waves' meeting and the stores, + MB x GPW x 4 MFMAs on one wave per
    // SIMD), and long rows against few tiles (wo: 4,096 columns, 160 tiles) are cheaper in MORE, SMALLER workgroups: 64 rows as 4 x 56 workgroups of 16 rows
    // x 3 tiles pull 227 KiB each where 2 x 80 of 32 rows x 2 tiles pull 326 (lab: 10.3 -> 9.1 us; 33-48 rows, three blocks instead of a padded four: 10.1
    // -> 7.2).  gate|up / lm_head (many tiles per workgroup) keep the largest block by the same arithmetic.
    const int blocks16 = (M + 15) / 16;
    auto shape_for = [&](int mb, Qmm6Plan &q) {
        q.MB = mb;
        q.row_blocks = (blocks16 + mb - 1) / mb;
        const int wgs = std::min(tiles, std::max(1, ncu / q.row_blocks));
        q.tiles_per_wg = (tiles + wgs - 1) / wgs;
        q.wgs = (tiles + q.tiles_per_wg - 1) / q.tiles_per_wg;
        // the workgroups of one tile range sit a multiple of 8 apart in the launch order: one XCD, one L2 for the weights they share
        if (q.row_blocks > 1) q.wgs = (q.wgs + 7) / 8 * 8;
    };
    const int mb_max = blocks16 >= 3 ? 4 : (blocks16 >= 2 ? 2 : 1);
    double best = 0.0;
    bool found = false;
    for (int mb = mb_max; mb >= 1; mb /= 2) {
        if (!qmm6_has_variant(mb, pl.GPW) || qmm6_lds_bytes(mb, pl.GPW, frag) > 150 * 1024) continue;
        Qmm6Plan q = pl;
        shape_for(mb, q);
        // (the arithmetic below decides for LONG rows against FEW tiles only -- 8 groups per wave and more, at most two tiles per workgroup on the largest
        // block: wo.  A projection whose workgroups walk more tiles keeps the largest block; so does qkv: the row-streaming kernel (qmm7.h) is its twin
        // bit for bit, and the order in which a group's four k-steps are added follows the row-block count -- CH below)
        if (found && (pl.tiles_per_wg > 2 || pl.GPW < 8)) break;
        // one workgroup per CU -- a rule for the ALTERNATIVES: the first candidate a kernel exists for is taken as it is (w_down-shaped rows of 19 groups
        // per wave have one candidate, 16-row blocks, and at 33-48 rows its three row blocks over 88 workgroups are 264)
        if (found && (long)q.wgs * q.row_blocks > ncu + 7) continue;
        const double kib = (double)std::min(mb * 16, M) * N * 2 / 1024.0 + (double)q.tiles_per_wg * G;
        // (plain rows come through each wave's 8-slot transposer ring: a second and third pass of the ring -- MB x GPW units -- is a dependent round trip each)
        const double us = 0.0135 * kib + q.tiles_per_wg * (0.35 + 0.03 * mb * pl.GPW) + 1.3 * ((mb * pl.GPW - 1) / QM6_RING);
        if (!found || us < best - 1e-9) pl.MB = q.MB, pl.row_blocks = q.row_blocks, pl.tiles_per_wg = q.tiles_per_wg, pl.wgs = q.wgs, best = us, found = true;
    }
    if (!found) return pl;
    pl.NSETS = qmm6_pick_sets(pl.MB, pl.GPW, pl.tiles_per_wg);
    pl.lds = qmm6_lds_bytes(pl.MB, pl.GPW, frag);
    pl.ok = pl.lds <= 150 * 1024;
    return pl;
}

// ---- the row-streaming matmul (qmm7.h) ----------------------------------------------------------------------
constexpr int QM7_WAVES = 4;
constexpr size_t qmm7_lds_bytes(int MB, int T) { return (size_t)QM7_WAVES * T * MB * 1024 + (size_t)MB * 16 * 4; }

// The instantiation table, written once: QM7_TABLE(X) expands X(T, GPW) for every compiled pair.  Every pair exists for 1 .. 4 row
// blocks and both epilogues.
#define QM7_TABLE(X) X(2, 5) X(5, 5)
inline bool qmm7_has_variant(int T, int GPW) {
#define QM7_MEMBER(Tv, GPWv) if (T == Tv && GPW == GPWv) return true;
    QM7_TABLE(QM7_MEMBER)
#undef QM7_MEMBER
    return false;
}

struct Qmm7Plan {
    int MB, T, GPW, wgs, row_blocks;
    size_t lds;
    bool ok;
};
inline Qmm7Plan qmm7_plan(int M, int N, int K, int ncu) {
    Qmm7Plan pl{};
    if (M < 1 || M > 64 || N <= 0 || N % 128 != 0 || K <= 0 || K % 16 != 0) return pl;
    const int G = N / 128, tiles = K / 16;
    pl.MB = (M + 15) / 16;
    pl.row_blocks = 1;
    const int gpw = (G + QM7_WAVES - 1) / QM7_WAVES;
    pl.GPW = gpw <= 5 ? 5 : 0;
    if (gpw < 4) return pl;  // a wave that idles through most of a 5-group body: the register-resident kernel's smaller variants take the shape
    const int tpw = (tiles + ncu - 1) / ncu;
    pl.T = tpw <= 2 ? 2 : (tpw <= 5 ? 5 : 0);
    if (!qmm7_has_variant(pl.T, pl.GPW)) return pl;
    pl.wgs = (tiles + pl.T - 1) / pl.T;
    pl.lds = qmm7_lds_bytes(pl.MB, pl.T);
    pl.ok = pl.lds <= 150 * 1024;
    return pl;
}

// ---- the routing ----------------------------------------------------------------------------------------------
// what the routing reads of an engine's -- or an entry point's -- settings (LinearCtx, decode_linear.h, derives from it)
struct LinearKnobs {
    // The 1-4-row GEMVs add the partial sums of squares their producer left instead of re-deriving them (a row without partials --
    // the first step after a MoE layer, a packed-dot fallback -- is still re-derived inside the kernel: qmv3.h, ss_given):
    // qkv -0.44 us, gate|up -1.1 us per layer (abl_lab, bit 8)
    bool gemv_producer_ss = true;
    // The wo GEMV of 1-4 decode rows also leaves h * post_attention_layernorm (bf16) and the gate|up GEMV stages THAT row and
    // multiplies its sums by the row's 1 / rms at the end (qmv3.h, PRO_RMS_WEIGHTED): the 1,216 workgroups of gate|up no longer
    // fetch the norm weights and normalise the whole row each.  tools/lab/trace_lab, back to back: gate|up 7.82 -> 7.08 us, wo
    // 3.91 -> 4.06; the qkv and lm_head GEMVs gain nothing from it and keep the fused RMSNorm (weighted_rows_apply decides by shape).
    bool gemv_weighted_rows = true;
    bool fuse_norm = true;                   // the skinny matmul normalises its own slice whenever its producer left sums of squares
    int qmm3_min_rows = 5;  // rows from which a projection uses the K-sliced skinny matmul instead of the GEMV (TL_QMM3_MIN_M)
    bool use_qmm3 = true;   // tl_engine_set_option "qmm3" = 0: rows > 8 go through the prefill GEMM path instead
    // 5 .. 64 rows: the register-resident matmul (qmm6.h) takes every projection whose plan fits; rows travel WEIGHTED between the
    // projections (qkv <- w_down / the embedding, gate|up <- wo).  tl_engine_set_option "qmm6" = 0: the K-sliced skinny matmul as before.
    bool use_qmm6 = true;
    // ... and, where its plan exists (round 6: gate|up and qkv of a 2,560-wide model), the row-streaming matmul (qmm7.h) instead of the
    // register-resident one: the rows' arrival overlaps the walk, a step costs by its 16-row blocks (3 included).  force_qmm7: the
    // kernel-level entry point asked for it by name (an error where it does not apply).
    bool use_qmm7 = true, force_qmm7 = false;
    int force_linear = 0;               // kernel-level entry points: 1 = fused GEMV, 2 = skinny matmul
    int qmm3_mode = -1;                 // skinny matmul grid: -1 by shape (qmm3_plan), 0 one-shot, 1 persistent
    int ncu = 256;                      // CUs of the device the plans are made for (qmm3_num_cus(); 256 when no device is visible)
    void read_env() { if (const char *q = getenv("TL_QMM3_MIN_M")) qmm3_min_rows = std::max(1, atoi(q)); }
};
// one W4 matrix as the routing sees it: out features, in features, whether its copy in the tiled MFMA layout exists
struct ProjShape {
    int rows = 0, cols = 0;
    bool tiled = false;
};

// rows that engine_linear hands to the GEMV before it considers anything else
inline bool gemv_takes_rows(const LinearKnobs &ctx, int M) {
    return ctx.force_linear == 1 || (ctx.force_linear != 2 && (M < ctx.qmm3_min_rows || (M <= 8 && !ctx.use_qmm3)));
}
// Does the register-resident matmul (qmm6.h) take this projection at M rows?
inline bool qmm6_takes(const LinearKnobs &ctx, const ProjShape &w, int M) {
    return ctx.use_qmm6 && ctx.force_linear == 0 && M >= ctx.qmm3_min_rows && M <= 64 && w.tiled && qmm6_plan(M, w.cols, w.rows, false, ctx.ncu).ok;
}
// Can `producer` (EPI_RESIDUAL) leave its rows weighted for `consumer` (PRO_RMS_WEIGHTED)?  Both must be single-pass MFMA GEMVs,
// the producer must leave the sums of squares, and the consumer's row must sit in its register chunks (qmv3.h, reg_path).
inline bool weighted_rows_apply(const LinearKnobs &ctx, const ProjShape &producer, const ProjShape &consumer, int M) {
    if (!ctx.gemv_weighted_rows || !ctx.gemv_producer_ss || !gemv_takes_rows(ctx, M) || M > 8) return false;
    if (!producer.tiled || !consumer.tiled) return false;
    const Qmv3Plan pp = qmv3_plan(M, producer.cols, producer.rows), pcn = qmv3_plan(M, consumer.cols, consumer.rows);
    if (!pp.ok || !pcn.ok || producer.rows != consumer.cols) return false;
    return qmv3_takes_weighted_rows(pcn, consumer.cols, producer.rows / 16);
}
// Does engine_linear send M rows of this projection to the K-sliced skinny matmul (qmm3.h), and on which plan?  ONE predicate for the router
// (which launches the plan) and for the route of a layer (plan_layer decides from it whether a producer will leave weighted rows).
inline Qmm3Plan skinny_matmul_plan(const LinearKnobs &ctx, const ProjShape &w, int M) {  // (not ok: the projection goes elsewhere)
    if (gemv_takes_rows(ctx, M) || !ctx.use_qmm3 || M > 64 || !w.tiled) return Qmm3Plan{};
    return qmm3_plan(M, w.cols, w.rows, ctx.qmm3_mode, ctx.ncu);
}
inline bool takes_skinny_matmul(const LinearKnobs &ctx, const ProjShape &w, int M) { return skinny_matmul_plan(ctx, w, M).ok; }

// Can the wo GEMV of ONE decode row take the attention split partials instead of the merged row (qmv3.hip,
// launch_qmv3_attn_merge_bf16: Q3_MERGE_TABLE)?  The answer is the attention plan's wo_can_merge (attn_plan.h).
// Single-row decode with the context split 2 / 4 / 8 ways: no merge launch behind the attention kernel -- the wo GEMV forms the
// merged row from the split partials while it stages it (qmv3.h, PRO_ATTN_MERGE).  Measured in round 3
// (profiles/r03_labs/wo_merges_attn_ab_after_dpp.jsonl): 4 windows 1.023 -> 0.993 ms per token, 8 windows 1.033 -> 1.009 (the
// merging GEMV costs +0.9 / +2.0 us per layer, the merge launch cost 0.6 us + a boundary); 64-token windows stay the best
// (128-token windows: 1.022).  Other split counts, more sequences or another head size keep the merge launch.
inline bool wo_merge_applicable(const LinearKnobs &ctx, const ProjShape &wo, int batch, int n_splits, int head_dim, int num_heads) {
    if (batch != 1 || ctx.force_linear != 0) return false;
    if (n_splits != 2 && n_splits != 4 && n_splits != 8) return false;
    if (head_dim != 128 || wo.cols != num_heads * 128 || !wo.tiled) return false;
    if (1 >= ctx.qmm3_min_rows && ctx.use_qmm3) return false;  // a single row would not take the GEMV
    const Qmv3Plan pl = qmv3_plan(1, wo.cols, wo.rows);
    return pl.ok && pl.MR == 1 && qmv3_merge_has_variant(pl.KS, pl.CW, pl.LM) && wo.cols / 8 <= 2 * pl.CW * 64;
}

// ---- the route of a layer -------------------------------------------------------------------------------
// Which kernel takes each projection of one layer at `batch` rows, decided once per step.  5 .. 64 rows take the BATCHED hand-over when
// gate|up is the register-resident matmul's (qmm6.h; its and lm_head's at every row count) and wo can leave h weighted for it: rows travel
// WEIGHTED between the projections (qkv <- w_down / the embedding, gate|up <- wo), plain beside them for the residual stream.  Measured:
//   qkv6    on the register-resident kernel at every row count since round 5 (rows in fragment order from 9 rows): same-box A/B at
//           128-token contexts, two alternating rounds, 24 / 32 / 48 / 64 sequences 1.91 / 1.95 / 2.56 / 2.69 -> 1.87 / 1.89 / 2.50 / 2.59 ms
//           per step (profiles/r05_labs/batched_qkv_on_qmm6_ab.log); the sliced matmul, whose slices the attention kernel adds, is the
//           route behind option "qmm6" = 0 only
//   wo6     likewise at EVERY row count (round 6: its planner deals 16-row blocks to more workgroups where the rows are long -- 17-32 rows
//           6.9 us against 8.4-9.1 for the sliced matmul + reduction that took them until then, 33-48 rows 10.1 -> 7.1; qmm6_plan)
//   down    76 groups against 160 tiles -- every workgroup of the register-resident kernel would pull 311 KB of rows for ONE tile
//           (measured 9.0 us at 8 rows, 18.9 at 64, against 6.5 / 13.0 for the K-sliced matmul + reduction): the sliced kernel keeps it
//           wherever its plan exists, and its reduction leaves the weighted rows
struct LayerRoute {
    bool batched = false;  // the batched hand-over (it also needs the row's sums of squares when the layer starts: enqueue_step)
    bool qkv6 = false, wo6 = false;  // batched: qkv / wo on engine_qmm6 (else engine_linear)
    enum Down { DOWN_ROUTER, DOWN_SLICED_WEIGHTED, DOWN_QMM6 } down = DOWN_ROUTER;  // batched: engine_linear (plain rows only), engine_linear leaving weighted rows, engine_qmm6
    bool gemv_weighted = false;  // not batched: the wo GEMV leaves h weighted for the gate|up GEMV (weighted_rows_apply)
    // every hand-over of the layer has a per-layer buffer to itself (an RMSNorm launch or a plain-row w_down goes through shared scratch)
    bool batched_written_once() const { return batched && qkv6 && down != DOWN_ROUTER; }
};
// the four matrices of a layer (dense_mlp: the layer has gate|up and w_down of its own -- not a MoE layer's)
struct LayerShapes {
    ProjShape wqkv, wo, wgu, wdown;
    bool dense_mlp = false;
};
inline LayerRoute plan_layer(const LinearKnobs &ctx, const LayerShapes &w, int batch, bool is_moe) {
    LayerRoute r;
    if (is_moe || !w.dense_mlp) return r;
    // the sliced matmul as the producer of weighted rows: the router's own predicate + what its reduction needs to emit the hand-over
    auto sliced_leaves_weighted = [&](const ProjShape &m) {
        return takes_skinny_matmul(ctx, m, batch) && ctx.fuse_norm && qmm3_reduce_can_emit_ss(EPI_RESIDUAL, m.rows);
    };
    auto qmm6_leaves_weighted = [&](const ProjShape &m) { return qmm6_takes(ctx, m, batch) && qmm3_takes_ss(m.rows / 16); };
    r.gemv_weighted = weighted_rows_apply(ctx, w.wo, w.wgu, batch);
    r.wo6 = qmm6_leaves_weighted(w.wo);
    r.batched = qmm6_takes(ctx, w.wgu, batch) && (r.wo6 || sliced_leaves_weighted(w.wo));
    r.qkv6 = qmm6_takes(ctx, w.wqkv, batch);
    r.down = sliced_leaves_weighted(w.wdown) ? LayerRoute::DOWN_SLICED_WEIGHTED
                                             : (qmm6_leaves_weighted(w.wdown) ? LayerRoute::DOWN_QMM6 : LayerRoute::DOWN_ROUTER);
    return r;
}
// The weighted rows of a batched step (5 .. 64 rows) travel in fragment order (qmm6.h) from 9 rows (same-box A/B,
// profiles/r04_labs/README.md: 16 / 32 / 64 sequences -1.5 / -4 / -1.3 % per step; at 8 sequences +2 %: row-major there) -- and from 5
// where the row-streaming matmul (qmm7.h) is the consumer (it reads nothing else): ONE answer per step for every producer and consumer.
inline bool rows_travel_in_fragment_order(const LinearKnobs &ctx, const LayerShapes &first, int batch) {
    if (batch > 8) return true;
    if (!ctx.use_qmm7 || !first.dense_mlp) return false;
    return qmm7_plan(batch, first.wgu.cols, first.wgu.rows, ctx.ncu).ok && qmm7_plan(batch, first.wqkv.cols, first.wqkv.rows, ctx.ncu).ok;
}

}  // namespace tl
