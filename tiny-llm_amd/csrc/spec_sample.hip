// tl_spec_sample_rows: the speculative-sampling routine (spec_sample.h) over caller rows.  A translation unit of its own: the decode
// step's kernels (engine.hip, and its device-only code object for the AQL route) are compiled without it.
#include <hip/hip_runtime.h>

#include "../../include/tinyllm_engine.h"
#include "spec_sample.h"

using namespace tl;

extern "C" int tl_spec_sample_rows(const void *target_logits_dev, const void *draft_logits_dev, int rows, int vocab, const int32_t *proposal_dev,
                                   const float *temperature_dev, const int32_t *top_k_dev, const float *top_p_dev,
                                   const float *draft_temperature_dev, const int32_t *draft_top_k_dev, const float *draft_top_p_dev,
                                   const uint64_t *seed_dev, const int32_t *position_dev, int32_t *accept_dev, int32_t *alt_dev, void *stream) {
    TL_REQUIRE(target_logits_dev && draft_logits_dev && proposal_dev && temperature_dev && top_k_dev && top_p_dev && draft_temperature_dev &&
                   draft_top_k_dev && draft_top_p_dev && seed_dev && position_dev && accept_dev && alt_dev,
               "spec_sample_rows: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "spec_sample_rows: rows out of range");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "spec_sample_rows: vocabulary out of range (1 .. 524,288)");
    const SpecSampleArgs a{(const uint16_t *)target_logits_dev, (const uint16_t *)draft_logits_dev, vocab, proposal_dev, temperature_dev, top_k_dev,
                           top_p_dev, draft_temperature_dev, draft_top_k_dev, draft_top_p_dev, seed_dev, position_dev, accept_dev, alt_dev};
    hipLaunchKernelGGL(spec_sample_rows_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("spec_sample_rows");
    return TL_OK;
}
