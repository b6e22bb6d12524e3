// Host side of the batched verification's launches (verify_attn.h holds the kernels, verify_attn.hip compiles them): the argument
// blocks and the launch functions engine.hip calls.  No device code here, so engine.hip's kernels -- and its device-only code object for
// the AQL route -- are compiled without the verification's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/tinyllm_engine.h"

namespace tl {

constexpr int VA_RQ = 4;         // (query head, position) rows of one GQA group per workgroup: PD_RQ of paged_decode_kernel
constexpr int VA_MAX_ROWS = 64;  // rows per pass
constexpr int VA_MAX_LEN = 8;    // rows per sequence
constexpr int VA_D = 128;

struct VerifyRowsArgs {
    const uint16_t *qkv;  // [R, (Hq + 2 Hkv) * 128]
    const uint16_t *q_norm_w, *k_norm_w;
    uint16_t *q;  // [R, Hq, 128] normalised and rotated
    uint16_t *key_pages, *value_pages;
    float *key_scales, *value_scales;  // KV8: the row scales of FP8 pages (kv8.h)
    const int32_t *block_table;        // [slots, max_pages]
    const int32_t *row_slot, *row_pos;  // [R]
    int page_size, max_pages, num_heads, num_kv_heads;
    float eps, rope_base;
};

struct VerifyAttnArgs {
    const uint16_t *q;  // [R, Hq, 128]
    const uint16_t *key_pages, *value_pages;
    const float *key_scales, *value_scales;
    const int32_t *block_table;
    const int32_t *seq_slot, *seq_row0, *seq_len, *seq_ctx;  // [n_seqs]
    uint16_t *out;  // [R, Hq * 128]
    float *ws;      // [R * Hq, n_splits, 128 + 2] (value sums, running max, running sum) when n_splits > 1
    int page_size, max_pages, num_heads, num_kv_heads, n_splits;
    float scale;
};

struct VerifySplit {
    int n_splits = 1, row_chunks = 1;
};
// the split plan of one call: tl_paged_attention's rule for L <= 8 from the call's largest context and longest chunk, kept inside the
// partial rows the workspace holds
VerifySplit verify_pick_splits(int n_seqs, int num_heads, int num_kv_heads, int total_rows, int max_len, int max_ctx, size_t ws_rows);
// Partial rows of [128 + 2] floats that hold every plan of that rule: n_splits <= 512 / base + 1 with base = n_seqs * Hkv * row_chunks >=
// n_seqs * Hkv * rep * max_len / 4, and total_rows <= n_seqs * max_len, so total_rows * Hq * n_splits <= 2048 + total_rows * Hq.
size_t verify_ws_rows(int num_heads);

// the attention stage of one layer over the rows described on the device: append + rotate, attend, merge
int launch_verify_attention(const VerifyRowsArgs &q, VerifyAttnArgs a, const VerifySplit &sp, int total_rows, int n_seqs, bool kv8, hipStream_t st);
// greedy ids of `total_rows` rows into `greedy`, then one tl_verify_result per sequence
int launch_verify_accept(const uint16_t *logits, int vocab, int total_rows, int n_seqs, const int32_t *tokens, const int32_t *seq_row0,
                         const int32_t *seq_len, int32_t *greedy, tl_verify_result *out, hipStream_t st);

// The acceptance stage for slots that sample (verify_sample.h holds the kernels, verify_sample.hip compiles them): everything lives on
// the device, the draft's one parameter triple rides in the arguments.
struct VerifySampleArgs {
    const uint16_t *target;  // [R, vocab]
    const uint16_t *draft;   // [R, vocab], the row of a bonus proposal is never read; NULL: point proposals (one-hot at the proposed id)
    int vocab, n_seqs;
    const int32_t *tokens;                         // [R] the tokens the rows were fed
    const int32_t *seq_row0, *seq_len, *seq_ctx;   // [n_seqs]; seq_ctx = the context length behind the sequence's last row
    const int32_t *seq_index;                      // [n_seqs] where a sequence's parameters stand in the four arrays below (NULL: at i)
    const float *temperature;
    const int32_t *top_k;
    const float *top_p;
    const uint64_t *seed;
    float d_temperature;
    int d_top_k;
    float d_top_p;
    int32_t *accept, *alt;  // [R]
};
// the sequences of the routine over caller rows, handed over as kernel arguments (a.seq_* are not read then)
struct VerifySeqsInline {
    uint8_t row0[VA_MAX_ROWS], len[VA_MAX_ROWS];
    int32_t ctx[VA_MAX_ROWS];
};
// accept / alt of `total_rows` rows, then one tl_verify_result per sequence; seqs NULL: the descriptors a.seq_* on the device
int launch_verify_sample(const VerifySampleArgs &a, const VerifySeqsInline *seqs, int total_rows, tl_verify_result *out, hipStream_t st);
// what the routines over caller rows ask of their sequences (`who` names the routine in the message)
int verify_rows_check(const char *who, int n_seqs, const int *row0_or_null, const int *lens, int *total_out);

}  // namespace tl
