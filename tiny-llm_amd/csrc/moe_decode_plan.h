// The host-only planner of the decode-shaped expert route (moe_decode.h): how a stage's output features and quantisation groups are
// split over workgroups and waves.  No HIP include: tl_moe_decode_plan / tl_moe_decode_wave hand it to callers without a device, and
// the kernels call moe_decode_wave_at themselves, so what the tests sweep is what runs.
#pragma once

#if defined(__HIPCC__)
#define TL_MOE_DECODE_HD __host__ __device__
#else
#define TL_MOE_DECODE_HD
#endif

namespace tl {

constexpr int MOE_DEC_MAX_ROWS = 64;        // activation rows of a call
constexpr int MOE_DEC_MAX_K = 16;           // experts per token: at most 1,024 expert rows, 2 KiB of 16-bit ids in LDS
constexpr int MOE_DEC_MAX_E = 1024;         // 32 words of "named" bits
constexpr int MOE_DEC_LM = 4;               // groups a wave requests at once (one step): 4 x 16 bytes per lane and matrix
constexpr int MOE_DEC_WAVES = 4;            // waves of a workgroup at most: feature blocks x reduction slices

// One stage (gate | up, or down) over N reduced columns and K output features of every named expert.
struct MoeDecodeStage {
    int features;  // output features of a workgroup: 16 per feature block, 1, 2 or 4 blocks
    int wk;        // waves along the reduction
    int per;       // groups (128 columns) of a wave: wave slice ks reduces groups [ks * per, min(G, ks * per + per))
    int grid_x;    // K / features
    int grid_y;    // the host's bound on the experts named: min(rows * k, E)
    int threads;   // 64 * wk * (features / 16)
};

struct MoeDecodePlan {
    MoeDecodeStage gate_up, down;
};

// Waves along the reduction first: ceil(G / 4) groups each, as many waves as that leaves with work (6 groups: 3 waves of 2; 13: 4, 4,
// 4, 1).  The waves left over take further 16-feature blocks of the same expert (a power of two, so that it divides K / 16) -- unless
// the grid would then leave CUs without a workgroup, where the smaller workgroup spreads the same bytes over more of them.
inline MoeDecodeStage moe_decode_stage(int N, int K, int named_bound, int cus) {
    MoeDecodeStage s{};
    const int G = N / 128;
    s.per = (G + MOE_DEC_WAVES - 1) / MOE_DEC_WAVES;
    s.wk = (G + s.per - 1) / s.per;
    int wf = MOE_DEC_WAVES / s.wk;
    wf = wf >= 4 ? 4 : wf >= 2 ? 2 : 1;
    while (wf > 1 && (long)(K / (16 * wf)) * named_bound < 2L * cus) wf /= 2;
    s.features = 16 * wf;
    s.grid_x = K / s.features;
    s.grid_y = named_bound;
    s.threads = 64 * s.wk * wf;
    return s;
}

inline MoeDecodePlan moe_decode_split(int rows, int k, int E, int D, int I, int cus) {
    const int bound = rows * k < E ? rows * k : E;
    return {moe_decode_stage(D, I, bound, cus), moe_decode_stage(I, D, bound, cus)};
}

// What wave `wave` of workgroup `block` (blockIdx.x) computes: 16 features from *feature0, groups [*g0, *g1).
TL_MOE_DECODE_HD inline void moe_decode_wave_at(int features, int wk, int per, int G, int block, int wave, int *feature0, int *g0, int *g1) {
    *feature0 = block * features + (wave / wk) * 16;
    *g0 = (wave % wk) * per;
    *g1 = *g0 + per < G ? *g0 + per : G;
}

}  // namespace tl
