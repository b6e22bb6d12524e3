// Batched verification: the translation unit of its kernels (verify_attn.h), their launch functions (verify_attn_host.h; engine.hip's
// pass calls them) and the two routines over caller rows and pools.  A translation unit of its own, like spec_sample.hip: the decode
// step's kernels (engine.hip, and its device-only code object for the AQL route) are compiled without it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/tinyllm_engine.h"
#include "device_block.h"
#include "verify_attn.h"

namespace tl {

#define TL_TRY(expr)                    \
    do {                                \
        const int rc__ = (expr);        \
        if (rc__ != TL_OK) return rc__; \
    } while (0)

int paged_decode_splits(int B, int Hkv, int row_chunks, int max_ctx);  // attention.hip: the split rule of tl_paged_attention at L <= 8

// the split plan of one call: tl_paged_attention's rule for L <= 8 from the call's largest context and longest chunk, kept inside the
// partial rows the workspace holds
VerifySplit verify_pick_splits(int n_seqs, int num_heads, int num_kv_heads, int total_rows, int max_len, int max_ctx, size_t ws_rows) {
    VerifySplit s;
    s.row_chunks = ceil_div(num_heads / num_kv_heads * max_len, VA_RQ);
    s.n_splits = paged_decode_splits(n_seqs, num_kv_heads, s.row_chunks, max_ctx);
    while (s.n_splits > 1 && (size_t)total_rows * num_heads * s.n_splits > ws_rows) --s.n_splits;
    return s;
}
// Partial rows of [128 + 2] floats that hold every plan of that rule: n_splits <= 512 / base + 1 with base = n_seqs * Hkv * row_chunks >=
// n_seqs * Hkv * rep * max_len / 4, and total_rows <= n_seqs * max_len, so total_rows * Hq * n_splits <= 2048 + total_rows * Hq.
size_t verify_ws_rows(int num_heads) { return 2048 + (size_t)VA_MAX_ROWS * num_heads; }

// the attention stage of one layer over the rows described on the device: append + rotate, attend, merge
int launch_verify_attention(const VerifyRowsArgs &q, VerifyAttnArgs a, const VerifySplit &sp, int total_rows, int n_seqs, bool kv8,
                            hipStream_t st) {
    a.n_splits = sp.n_splits;
    const dim3 grid(sp.n_splits * sp.row_chunks, a.num_kv_heads, n_seqs);
    if (kv8) {
        hipLaunchKernelGGL((verify_qkv_post_kernel<true>), dim3(total_rows), dim3(256), 0, st, q);
        hipLaunchKernelGGL((verify_attention_kernel<true>), grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((verify_qkv_post_kernel<false>), dim3(total_rows), dim3(256), 0, st, q);
        hipLaunchKernelGGL((verify_attention_kernel<false>), grid, dim3(256), 0, st, a);
    }
    if (sp.n_splits > 1) hipLaunchKernelGGL(verify_merge_kernel, dim3(total_rows * a.num_heads), dim3(128), 0, st, a.ws, a.out, sp.n_splits);
    TL_CHECK_LAUNCH("verify attention");
    return TL_OK;
}

int launch_verify_accept(const uint16_t *logits, int vocab, int total_rows, int n_seqs, const int32_t *tokens, const int32_t *seq_row0,
                         const int32_t *seq_len, int32_t *greedy, tl_verify_result *out, hipStream_t st) {
    hipLaunchKernelGGL(verify_accept_kernel, dim3(total_rows), dim3(1024), 0, st, logits, vocab, greedy);
    hipLaunchKernelGGL(verify_scan_kernel, dim3(ceil_div(n_seqs, 64)), dim3(64), 0, st, greedy, tokens, seq_row0, seq_len, n_seqs, out);
    TL_CHECK_LAUNCH("verify accept");
    return TL_OK;
}

}  // namespace tl

using namespace tl;

// The two stages over caller rows and pools (header, last section): the launches of the pass with descriptors built from the host arrays.
// One allocation per call (descriptors, rotated queries, partials), released behind the synchronisation.
int tl::verify_rows_check(const char *who, int n_seqs, const int *row0_or_null, const int *lens, int *total_out) {
    const std::string w = std::string(who) + ": ";
    TL_REQUIRE(n_seqs >= 1 && n_seqs <= VA_MAX_ROWS && lens, w + "between 1 and 64 sequences");
    int total = 0;
    for (int i = 0; i < n_seqs; ++i) {
        TL_REQUIRE(lens[i] >= 1 && lens[i] <= VA_MAX_LEN, w + "between 1 and 8 rows per sequence");
        if (row0_or_null) TL_REQUIRE(row0_or_null[i] >= 0 && row0_or_null[i] + lens[i] <= VA_MAX_ROWS, w + "a sequence's rows lie outside [0, 64)");
        total += lens[i];
    }
    TL_REQUIRE(total <= VA_MAX_ROWS, w + "more than 64 rows");
    *total_out = total;
    return TL_OK;
}

extern "C" int tl_verify_attention_rows(const void *qkv_dev, const void *q_norm_dev, const void *k_norm_dev, void *key_pages_dev, void *value_pages_dev,
                                        float *key_scales_dev, float *value_scales_dev, const int32_t *block_table_dev, int n_seqs, const int *slots,
                                        const int *starts, const int *lens, void *out_dev, int num_heads, int num_kv_heads, int page_size,
                                        int max_pages, float rope_theta, float eps, void *stream, tl_attention_info *info) {
    TL_REQUIRE(qkv_dev && q_norm_dev && k_norm_dev && key_pages_dev && value_pages_dev && block_table_dev && slots && starts && out_dev,
               "verify_attention_rows: null argument");
    TL_REQUIRE((key_scales_dev != nullptr) == (value_scales_dev != nullptr), "verify_attention_rows: key and value scales come together");
    TL_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0 && page_size > 0 && max_pages > 0,
               "verify_attention_rows: num_heads must be a multiple of num_kv_heads; page_size and max_pages positive");
    int total = 0;
    TL_TRY(verify_rows_check("verify_attention_rows", n_seqs, nullptr, lens, &total));
    enum { ROW_SLOT, ROW_POS, SEQ_SLOT, SEQ_ROW0, SEQ_LEN, SEQ_CTX, ARRAYS };
    int32_t desc[ARRAYS * 64] = {};
    int rows = 0, max_len = 1, max_ctx = 1;
    for (int i = 0; i < n_seqs; ++i) {
        TL_REQUIRE(slots[i] >= 0 && starts[i] >= 0 && (long)starts[i] + lens[i] <= (long)max_pages * page_size,
                   "verify_attention_rows: a sequence lies outside its block-table row");
        for (int j = 0; j < i; ++j) TL_REQUIRE(slots[j] != slots[i], "verify_attention_rows: a slot appears twice");
        desc[SEQ_SLOT * 64 + i] = slots[i], desc[SEQ_ROW0 * 64 + i] = rows, desc[SEQ_LEN * 64 + i] = lens[i], desc[SEQ_CTX * 64 + i] = starts[i] + lens[i];
        for (int j = 0; j < lens[i]; ++j) desc[ROW_SLOT * 64 + rows + j] = slots[i], desc[ROW_POS * 64 + rows + j] = starts[i] + j;
        rows += lens[i], max_len = std::max(max_len, lens[i]), max_ctx = std::max(max_ctx, starts[i] + lens[i]);
    }
    const VerifySplit sp = verify_pick_splits(n_seqs, num_heads, num_kv_heads, total, max_len, max_ctx, verify_ws_rows(num_heads));
    hipStream_t st = (hipStream_t)stream;
    Carve carve;
    const size_t o_desc = carve(sizeof(desc)), o_q = carve((size_t)total * num_heads * VA_D * 2);
    const size_t o_ws = carve(sp.n_splits > 1 ? (size_t)total * num_heads * sp.n_splits * (VA_D + 2) * 4 : 16);
    DeviceBlock mem;  // (released behind the synchronisation below)
    TL_TRY(mem.alloc(carve.off, "verify_attention_rows: hipMalloc(workspace) failed"));
    int rc = TL_OK;
    if (hipMemcpyAsync(mem.at(o_desc), desc, sizeof(desc), hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(TL_ERR_HIP, "verify_attention_rows: hipMemcpy(descriptors) failed");
    if (rc == TL_OK) {
        const int32_t *d = mem.at<int32_t>(o_desc);
        VerifyRowsArgs q{};
        q.qkv = (const uint16_t *)qkv_dev, q.q_norm_w = (const uint16_t *)q_norm_dev, q.k_norm_w = (const uint16_t *)k_norm_dev, q.q = mem.at<uint16_t>(o_q);
        q.key_pages = (uint16_t *)key_pages_dev, q.value_pages = (uint16_t *)value_pages_dev, q.key_scales = key_scales_dev, q.value_scales = value_scales_dev;
        q.block_table = block_table_dev, q.row_slot = d + ROW_SLOT * 64, q.row_pos = d + ROW_POS * 64;
        q.page_size = page_size, q.max_pages = max_pages, q.num_heads = num_heads, q.num_kv_heads = num_kv_heads, q.eps = eps, q.rope_base = rope_theta;
        VerifyAttnArgs a{};
        a.q = q.q, a.key_pages = q.key_pages, a.value_pages = q.value_pages, a.key_scales = key_scales_dev, a.value_scales = value_scales_dev;
        a.block_table = block_table_dev, a.seq_slot = d + SEQ_SLOT * 64, a.seq_row0 = d + SEQ_ROW0 * 64, a.seq_len = d + SEQ_LEN * 64, a.seq_ctx = d + SEQ_CTX * 64;
        a.out = (uint16_t *)out_dev, a.ws = mem.at<float>(o_ws);
        a.page_size = page_size, a.max_pages = max_pages, a.num_heads = num_heads, a.num_kv_heads = num_kv_heads, a.scale = 1.0f / sqrtf((float)VA_D);
        rc = launch_verify_attention(q, a, sp, total, n_seqs, key_scales_dev != nullptr, st);
    }
    const hipError_t se = hipStreamSynchronize(st);
    if (rc == TL_OK && se != hipSuccess) rc = fail(TL_ERR_HIP, std::string("verify_attention_rows: ") + hipGetErrorString(se));
    if (rc == TL_OK && info) {
        *info = tl_attention_info{};
        info->n_splits = sp.n_splits, info->tokens_per_split = ((max_ctx + sp.n_splits - 1) / sp.n_splits + 15) & ~15;
        info->heads_per_workgroup = VA_RQ, info->launches = sp.n_splits > 1 ? 3 : 2;
    }
    return rc;
}

extern "C" int tl_verify_accept_rows(const void *logits_dev, int vocab, int n_seqs, const int *row0, const int *lens, const int32_t *tokens_dev,
                                     tl_verify_result *out_dev, void *stream) {
    TL_REQUIRE(logits_dev && row0 && tokens_dev && out_dev, "verify_accept_rows: null argument");
    TL_REQUIRE(vocab >= 1, "verify_accept_rows: vocab must be positive");
    int total = 0;
    TL_TRY(verify_rows_check("verify_accept_rows", n_seqs, row0, lens, &total));
    int32_t desc[2 * 64] = {};
    int last = 0;  // rows [0, last) get a greedy id
    for (int i = 0; i < n_seqs; ++i) desc[i] = row0[i], desc[64 + i] = lens[i], last = std::max(last, row0[i] + lens[i]);
    hipStream_t st = (hipStream_t)stream;
    DeviceBlock mem;  // (released behind the synchronisation below)
    TL_TRY(mem.alloc(sizeof(desc) + 64 * 4, "verify_accept_rows: hipMalloc(workspace) failed"));
    int rc = TL_OK;
    if (hipMemcpyAsync(mem.at(), desc, sizeof(desc), hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(TL_ERR_HIP, "verify_accept_rows: hipMemcpy(descriptors) failed");
    if (rc == TL_OK)
        rc = launch_verify_accept((const uint16_t *)logits_dev, vocab, last, n_seqs, tokens_dev, mem.at<int32_t>(), mem.at<int32_t>(64 * 4),
                                  mem.at<int32_t>(sizeof(desc)), out_dev, st);
    const hipError_t se = hipStreamSynchronize(st);
    if (rc == TL_OK && se != hipSuccess) rc = fail(TL_ERR_HIP, std::string("verify_accept_rows: ") + hipGetErrorString(se));
    return rc;
}

