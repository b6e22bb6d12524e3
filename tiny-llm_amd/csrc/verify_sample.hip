// Batched speculative sampling: the translation unit of its kernels (verify_sample.h), their launch function (verify_attn_host.h;
// engine.hip's pass calls it) and the routine over caller rows.  A translation unit of its own, like spec_sample.hip: the decode step's
// kernels (engine.hip, and its device-only code object for the AQL route) are compiled without it, and no captured or AQL plan holds it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/tinyllm_engine.h"
#include "device_block.h"
#include "verify_sample.h"

namespace tl {

int launch_verify_sample(const VerifySampleArgs &a, const VerifySeqsInline *seqs, int total_rows, tl_verify_result *out, hipStream_t st) {
    if (seqs) {
        hipLaunchKernelGGL(verify_sample_rows_kernel, dim3(total_rows), dim3(1024), 0, st, a, *seqs);
        hipLaunchKernelGGL(verify_sample_rows_scan_kernel, dim3(ceil_div(a.n_seqs, 64)), dim3(64), 0, st, a.accept, a.alt, a.tokens, *seqs, a.n_seqs, out);
    } else {
        hipLaunchKernelGGL(verify_sample_kernel, dim3(total_rows), dim3(1024), 0, st, a);
        hipLaunchKernelGGL(verify_sample_scan_kernel, dim3(ceil_div(a.n_seqs, 64)), dim3(64), 0, st, a.accept, a.alt, a.tokens, a.seq_row0, a.seq_len,
                           a.n_seqs, out);
    }
    TL_CHECK_LAUNCH("verify sample");
    return TL_OK;
}

}  // namespace tl

using namespace tl;

// The two launches over caller rows (header, last section).  The sequences ride in the kernel arguments: nothing is uploaded, and
// nothing is allocated unless the caller wants no accept / alt (then one block, released behind the synchronisation).
extern "C" int tl_verify_sample_rows(const void *target_logits_dev, const void *draft_logits_dev, int vocab, int n_seqs, const int *row0, const int *lens,
                                     const int *starts, const int32_t *tokens_dev, const float *temperature_dev, const int32_t *top_k_dev,
                                     const float *top_p_dev, const uint64_t *seed_dev, float draft_temperature, int draft_top_k, float draft_top_p,
                                     int32_t *accept_dev, int32_t *alt_dev, tl_verify_result *out_dev, void *stream) {
    TL_REQUIRE(target_logits_dev && row0 && starts && tokens_dev && temperature_dev && top_k_dev && top_p_dev && seed_dev && out_dev,
               "verify_sample_rows: null argument");
    TL_REQUIRE(vocab >= 1 && vocab <= SMP_MAX_VOCAB, "verify_sample_rows: vocabulary out of range (1 .. 524,288)");
    TL_REQUIRE(std::isfinite(draft_temperature) && draft_temperature >= 0.f, "verify_sample_rows: the draft's temperature must be finite and >= 0");
    int total = 0;
    const int rc0 = verify_rows_check("verify_sample_rows", n_seqs, row0, lens, &total);
    if (rc0 != TL_OK) return rc0;
    VerifySeqsInline seqs{};
    int last = 0;  // rows [0, last) are launched
    for (int i = 0; i < n_seqs; ++i) {
        TL_REQUIRE(starts[i] >= 0 && (long)starts[i] + lens[i] <= 0x7fffffffL, "verify_sample_rows: a sequence's start is out of range");
        seqs.row0[i] = (uint8_t)row0[i], seqs.len[i] = (uint8_t)lens[i], seqs.ctx[i] = starts[i] + lens[i];
        last = std::max(last, row0[i] + lens[i]);
    }
    hipStream_t st = (hipStream_t)stream;
    DeviceBlock mem;
    if (!accept_dev || !alt_dev) {
        const int rc1 = mem.alloc(2 * (size_t)VA_MAX_ROWS * 4, "verify_sample_rows: hipMalloc(workspace) failed");
        if (rc1 != TL_OK) return rc1;
    }
    VerifySampleArgs a{};
    a.target = (const uint16_t *)target_logits_dev, a.draft = (const uint16_t *)draft_logits_dev, a.vocab = vocab, a.n_seqs = n_seqs;
    a.tokens = tokens_dev;
    a.temperature = temperature_dev, a.top_k = top_k_dev, a.top_p = top_p_dev, a.seed = seed_dev;
    a.d_temperature = draft_temperature, a.d_top_k = draft_top_k, a.d_top_p = draft_top_p;
    a.accept = accept_dev ? accept_dev : mem.at<int32_t>();
    a.alt = alt_dev ? alt_dev : mem.at<int32_t>((size_t)VA_MAX_ROWS * 4);
    int rc = launch_verify_sample(a, &seqs, last, out_dev, st);
    const hipError_t se = hipStreamSynchronize(st);
    if (rc == TL_OK && se != hipSuccess) rc = fail(TL_ERR_HIP, std::string("verify_sample_rows: ") + hipGetErrorString(se));
    return rc;
}
