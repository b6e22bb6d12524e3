// Batched speculative verification (include/tinyllm_engine.h "tl_engine_verify_batch"): the attention stage and
// the acceptance launches of one pass over R <= 64 rows that belong to several sequences, up to 8 rows each.  The kernels, static like
// those of engine_kernels.h and compiled by verify_attn.hip alone (engine.hip calls the launch functions of verify_attn_host.h, so its
// device code is what it was).  Head dimension 128 only.
//
//   rows       row r of the pass belongs to block-table row row_slot[r] and stands at position row_pos[r].  Sequence b owns the rows
//              [seq_row0[b], seq_row0[b] + seq_len[b]) and ends the pass with seq_ctx[b] tokens.
//   visibility row j of sequence b sees the first seq_ctx[b] - seq_len[b] + j + 1 tokens of its slot: everything before the chunk and the
//              chunk's own rows up to itself, which verify_qkv_post_kernel has appended before verify_attention_kernel starts.
//   layout     q, and the attention output, are row-major [R, Hq, 128]: the rows wo reads, no per-sequence transposed copy.
#pragma once
#include "engine_kernels.h"
#include "verify_attn_host.h"

namespace tl {

// What qkv_post_kernel does for the rows of one chunk, for ragged rows: per-head RMSNorm of q and k, RoPE at the row's own position, K
// and V appended at page block_table[slot][pos / page_size], row pos % page_size (KV8: quantised as kv8.h does), q row-major.
//   grid = R; block = 256 (16 groups of 16 lanes; a group owns one head at a time).  A row without a page writes no K/V.
template <bool KV8>
static __global__ __launch_bounds__(256) void verify_qkv_post_kernel(const VerifyRowsArgs p) {
    constexpr int VD = 8, D = VA_D;
    const int r = blockIdx.x;
    const int g = threadIdx.x >> 4;
    const int t = threadIdx.x & 15;
    const int Hq = p.num_heads, Hkv = p.num_kv_heads;
    const int pos = p.row_pos[r];
    const int32_t *block_row = p.block_table + (long)p.row_slot[r] * p.max_pages;
    const uint16_t *row = p.qkv + (long)r * (Hq + 2 * Hkv) * D;
    float cs[VD], sn[VD];
    rope_factors<VD>(t, pos, p.rope_base, cs, sn);
    const int lp = pos / p.page_size;
    const int slot = pos - lp * p.page_size;
    const int page_id = (lp >= 0 && lp < p.max_pages) ? block_row[lp] : -1;
    for (int h = g; h < Hq + 2 * Hkv; h += 16) {
        float v[VD];
        if (h < Hq) {
            head_norm_rope<VD>(row + (long)h * D, p.q_norm_w, t, p.eps, cs, sn, v);
            store_row<VD>(p.q + ((long)r * Hq + h) * D + t * VD, v);
            continue;
        }
        const bool is_k = h < Hq + Hkv;
        if (is_k) head_norm_rope<VD>(row + (long)h * D, p.k_norm_w, t, p.eps, cs, sn, v);
        else load_row<VD>(row + (long)h * D + t * VD, v);
        const long prow = ((long)max(page_id, 0) * Hkv + (is_k ? h - Hq : h - Hq - Hkv)) * p.page_size + slot;
        uint16_t *pages = is_k ? p.key_pages : p.value_pages;
        if constexpr (KV8) {
            u32x2 codes;
            float sc, deq[8];
            kv8_quantize_row16(v, codes, sc, deq);
            if (page_id >= 0) {
                *reinterpret_cast<u32x2 *>(reinterpret_cast<uint8_t *>(pages) + prow * D + t * VD) = codes;
                if (t == 0) (is_k ? p.key_scales : p.value_scales)[prow] = sc;
            }
        } else if (page_id >= 0) {
            store_row<VD>(pages + prow * D + t * VD, v);
        }
    }
}

// The token walk and the online softmax of paged_decode_kernel (attention.hip) over the rows of several sequences in one launch.
//   grid = (n_splits * row_chunks, Hkv, n_seqs), row_chunks = ceil(rep * longest chunk / VA_RQ); workgroup = 16 groups x 16 lanes.
//   A workgroup owns one KV head of one sequence, VA_RQ rows of that head's GQA group (row rr -> query head rr / len, position rr % len)
//   and one slice of the context: every K/V byte of the slot is fetched once per group of rows.  A 16-lane group reads one token's K and
//   V row as 16 x 16 B.  n_splits == 1 writes the output rows, otherwise (m, l, acc) partials that verify_merge_kernel combines.
template <bool KV8>
static __global__ __launch_bounds__(256) void verify_attention_kernel(const VerifyAttnArgs p) {
    constexpr int VD = 8, D = VA_D, stride = D + 2;
    __shared__ __attribute__((aligned(16))) float psm[16 * VA_RQ * stride];
    const int n_splits = p.n_splits;
    const int split = blockIdx.x % n_splits;
    const int chunk = blockIdx.x / n_splits;
    const int kvh = blockIdx.y;
    const int b = blockIdx.z;
    const int Hq = p.num_heads, Hkv = p.num_kv_heads;
    const int rep = Hq / Hkv;
    const int len = p.seq_len[b], ctx = p.seq_ctx[b], row0 = p.seq_row0[b];
    const int R = rep * len;
    if (chunk * VA_RQ >= R) return;  // a shorter chunk than the call's longest: nothing for this workgroup (uniform)
    const int32_t *block_row = p.block_table + (long)p.seq_slot[b] * p.max_pages;
    const int g = threadIdx.x >> 4;
    const int t = threadIdx.x & 15;
    const float scale_log2 = p.scale * ENG_LOG2E;

    int rq_vis[VA_RQ];
    float qv[VA_RQ][VD], acc[VA_RQ][VD], m[VA_RQ], l[VA_RQ];
    int max_vis = 0;
#pragma unroll
    for (int r = 0; r < VA_RQ; ++r) {
        const int rr = chunk * VA_RQ + r;
        const bool ok = rr < R;
        const int hq = ok ? rr / len : 0;
        const int qp = ok ? rr - hq * len : 0;
        rq_vis[r] = ok ? min(max(ctx - len + qp + 1, 0), ctx) : 0;
        max_vis = max(max_vis, rq_vis[r]);
        m[r] = -1e30f;
        l[r] = 0.f;
        float f[VD];
        load_row<VD>(p.q + ((long)(row0 + qp) * Hq + kvh * rep + hq) * D + t * VD, f);
#pragma unroll
        for (int i = 0; i < VD; ++i) {
            qv[r][i] = ok ? f[i] * scale_log2 : 0.f;
            acc[r][i] = 0.f;
        }
    }
    // context slice of this split (multiples of 16 tokens so groups stay aligned)
    const int per = ((max_vis + n_splits - 1) / n_splits + 15) & ~15;
    const int t_begin = split * per;
    const int t_end = min(t_begin + per, max_vis);

    for (int tok = t_begin + g; tok < t_end; tok += 16) {
        const int lp = tok / p.page_size;
        const int slot = tok - lp * p.page_size;
        const int page_id = lp < p.max_pages ? block_row[lp] : -1;
        if (page_id < 0) continue;
        const long prow = ((long)page_id * Hkv + kvh) * p.page_size + slot;
        float kf[VD], vf[VD];
        float k_s = 1.f, v_s = 1.f;  // KV8: the rows' scales
        if constexpr (KV8) {
            const u32x2 kc = *reinterpret_cast<const u32x2 *>(reinterpret_cast<const uint8_t *>(p.key_pages) + prow * D + t * VD);
            const u32x2 vc = *reinterpret_cast<const u32x2 *>(reinterpret_cast<const uint8_t *>(p.value_pages) + prow * D + t * VD);
            k_s = p.key_scales[prow];
            v_s = p.value_scales[prow];
            kv8_unpack8(kc, kf);
            kv8_unpack8(vc, vf);
        } else {
            load_row<VD>(p.key_pages + prow * D + t * VD, kf);
            load_row<VD>(p.value_pages + prow * D + t * VD, vf);
        }
#pragma unroll
        for (int r = 0; r < VA_RQ; ++r) {
            float part = 0.f;
#pragma unroll
            for (int i = 0; i < VD; ++i) part += qv[r][i] * kf[i];
            const float score = KV8 ? group16_sum(part) * k_s : group16_sum(part);
            if (tok < rq_vis[r]) {
                const float nm = fmaxf(m[r], score);
                const float of = exp2_hw(m[r] - nm);
                const float sf = exp2_hw(score - nm);
                l[r] = l[r] * of + sf;
                const float sfv = KV8 ? sf * v_s : sf;
#pragma unroll
                for (int i = 0; i < VD; ++i) acc[r][i] = acc[r][i] * of + sfv * vf[i];
                m[r] = nm;
            }
        }
    }

    // merge the 16 groups
#pragma unroll
    for (int r = 0; r < VA_RQ; ++r) {
        float *dst = psm + (g * VA_RQ + r) * stride;
#pragma unroll
        for (int i = 0; i < VD; ++i) dst[t * VD + i] = acc[r][i];
        if (t == 0) {
            dst[D] = m[r];
            dst[D + 1] = l[r];
        }
    }
    __syncthreads();
    for (int item = threadIdx.x; item < VA_RQ * D; item += 256) {
        const int r = item / D;
        const int d = item - r * D;
        const int rr = chunk * VA_RQ + r;
        if (rr >= R) continue;
        const int hq = rr / len;
        const int qp = rr - hq * len;
        float gm = -1e30f;
#pragma unroll
        for (int j = 0; j < 16; ++j) gm = fmaxf(gm, psm[(j * VA_RQ + r) * stride + D]);
        float gl = 0.f, vs = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float *src = psm + (j * VA_RQ + r) * stride;
            const float f = exp2_hw(src[D] - gm);
            gl += src[D + 1] * f;
            vs += src[d] * f;
        }
        const long orow = (long)(row0 + qp) * Hq + kvh * rep + hq;  // row-major [R, Hq]
        if (n_splits == 1) {
            p.out[orow * D + d] = BF16::from_float(gl == 0.f ? 0.f : vs / gl);
        } else {
            float *w = p.ws + (orow * n_splits + split) * stride;
            w[d] = vs;
            if (d == 0) {
                w[D] = gm;
                w[D + 1] = gl;
            }
        }
    }
}

// The split partials of every (row, query head) combined: paged_merge_kernel over the row-major rows of the pass.  A (row, head) whose
// workgroup saw fewer tokens than the call's longest context left empty slices (l = 0) behind: they weigh nothing.
//   grid = R * Hq; block = 128
static __global__ __launch_bounds__(128) void verify_merge_kernel(const float *__restrict__ ws, uint16_t *__restrict__ out, int n_splits) {
    constexpr int D = VA_D, stride = D + 2;
    const long orow = blockIdx.x;
    const float *base = ws + orow * n_splits * stride;
    float gm = -1e30f;
    for (int s = 0; s < n_splits; ++s) gm = fmaxf(gm, base[s * stride + D]);
    const int d = threadIdx.x;
    float gl = 0.f, vs = 0.f;
    for (int s = 0; s < n_splits; ++s) {
        const float f = exp2_hw(base[s * stride + D] - gm);
        gl += base[s * stride + D + 1] * f;
        vs += base[s * stride + d] * f;
    }
    out[orow * D + d] = BF16::from_float(gl == 0.f ? 0.f : vs / gl);
}

// Greedy id of every row: the first maximum wins, NaN is never chosen (argmax_rows_kernel's rule; a row without any comparable value gives 0).
//   grid = rows, block = 1024
static __global__ __launch_bounds__(1024) void verify_accept_kernel(const uint16_t *__restrict__ logits, int vocab, int32_t *__restrict__ ids) {
    __shared__ float s_val[16];
    __shared__ int s_idx[16];
    const uint16_t *lg = logits + (long)blockIdx.x * vocab;
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    for (int c = threadIdx.x; c < vocab; c += 1024) {  // ascending per thread: the earliest index of a tie stays
        const float v = BF16::to_float(lg[c]);
        if (v > best || (v == best && c < best_i)) {
            best = v;
            best_i = c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        if (ov > best || (ov == best && oi < best_i)) {
            best = ov;
            best_i = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        s_val[threadIdx.x >> 6] = best;
        s_idx[threadIdx.x >> 6] = best_i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float bv = s_val[0];
        int bi = s_idx[0];
        for (int w = 1; w < 16; ++w) {
            if (s_val[w] > bv || (s_val[w] == bv && s_idx[w] < bi)) {
                bv = s_val[w];
                bi = s_idx[w];
            }
        }
        ids[blockIdx.x] = (bi < 0 || bi >= vocab) ? 0 : bi;
    }
}

// One thread per sequence: a = the first row j < len - 1 whose greedy id differs from the proposal tokens[row0 + j + 1] (len - 1 when
// none does); count = a + 1, ids[0 .. a] the greedy ids of rows 0 .. a, the rest -1.  Proposals that agree again behind the first
// mismatch are never looked at.
//   grid = ceil(n_seqs / 64), block = 64
static __global__ __launch_bounds__(64) void verify_scan_kernel(const int32_t *__restrict__ greedy, const int32_t *__restrict__ tokens,
                                                                const int32_t *__restrict__ seq_row0, const int32_t *__restrict__ seq_len,
                                                                int n_seqs, tl_verify_result *__restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_seqs) return;
    const int row0 = seq_row0[b], len = min(max(seq_len[b], 1), VA_MAX_LEN);
    int a = len - 1;
    for (int j = len - 2; j >= 0; --j)
        if (greedy[row0 + j] != tokens[row0 + j + 1]) a = j;
    tl_verify_result r;
    r.count = a + 1;
#pragma unroll
    for (int j = 0; j < VA_MAX_LEN; ++j) r.ids[j] = j <= a ? greedy[row0 + min(j, len - 1)] : -1;
    out[b] = r;
}

}  // namespace tl
