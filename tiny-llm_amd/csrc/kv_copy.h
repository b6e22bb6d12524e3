// The tail copy of a prefix-cache hit (include/tinyllm_engine.h "Prefix cache", tl_kv_copy_rows): rows [0, rows) of one KV page into
// another, for every pool of the engine, in ONE launch.  copy_page (engine.hip) enqueues 2 x layers whole-page copies (4 x layers for
// FP8 pages); a hit with a tail happens at every admission of a serving loop.
//
// Pools are [pages][heads][page_size][row_bytes] bytes: the K and V pool of every layer, and for FP8 pages the two scale pools per
// layer (row_bytes 4).  Inside one (page, head) the rows are contiguous, so a workgroup copies ONE contiguous run of rows x row_bytes
// bytes: lane i moves the 16 bytes at 16 i of each 4 KiB stripe (the widest coalesced access, 1 KiB per wave instruction) when the
// run's ends are 16-byte aligned, 4 bytes per lane for the scale pools, single bytes otherwise.  No LDS, plain vector stores, nothing
// written outside rows [0, rows) of the destination page.
#pragma once

#include "common.h"
#include "../../include/tinyllm_engine.h"

namespace tl {

struct KvCopyArgs {
    const tl_kv_pool_desc *pools;  // [gridDim.x / heads]
    int heads, page_size, from_page, to_page, rows;
};

// grid = n_pools x heads, block = 256
static __global__ __launch_bounds__(256) void kv_copy_rows_kernel(const KvCopyArgs a) {
    const int pool = blockIdx.x / a.heads, head = blockIdx.x % a.heads;
    const tl_kv_pool_desc d = a.pools[pool];
    const size_t head_bytes = (size_t)a.page_size * d.row_bytes;
    const char *src = (const char *)d.base_dev + ((size_t)a.from_page * a.heads + head) * head_bytes;
    char *dst = (char *)d.base_dev + ((size_t)a.to_page * a.heads + head) * head_bytes;
    const size_t bytes = (size_t)a.rows * d.row_bytes;
    const size_t align = (size_t)(uintptr_t)src | (size_t)(uintptr_t)dst | bytes;
    if (align % 16 == 0) {
        const u32x4 *s = reinterpret_cast<const u32x4 *>(src);
        u32x4 *t = reinterpret_cast<u32x4 *>(dst);
        for (size_t i = threadIdx.x; i < bytes / 16; i += 256) t[i] = s[i];
    } else if (align % 4 == 0) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
        uint32_t *t = reinterpret_cast<uint32_t *>(dst);
        for (size_t i = threadIdx.x; i < bytes / 4; i += 256) t[i] = s[i];
    } else {
        for (size_t i = threadIdx.x; i < bytes; i += 256) dst[i] = src[i];
    }
}

// stream ordered; the caller has checked the page ids against its pools
static inline int kv_copy_rows(const tl_kv_pool_desc *pools_dev, int n_pools, int heads, int page_size, int from_page, int to_page,
                               int rows, hipStream_t stream) {
    TL_REQUIRE(pools_dev && n_pools >= 1 && heads >= 1 && page_size >= 1, "kv_copy_rows: need a pool table, heads and a page size");
    TL_REQUIRE(from_page >= 0 && to_page >= 0 && from_page != to_page, "kv_copy_rows: two different nonnegative page ids");
    TL_REQUIRE(rows >= 1 && rows <= page_size, "kv_copy_rows: between 1 and page_size rows");
    TL_REQUIRE((long)n_pools * heads <= 0x7fffffffL, "kv_copy_rows: too many workgroups");
    const KvCopyArgs a{pools_dev, heads, page_size, from_page, to_page, rows};
    hipLaunchKernelGGL(kv_copy_rows_kernel, dim3((unsigned)(n_pools * heads)), dim3(256), 0, stream, a);
    TL_CHECK_LAUNCH("kv_copy_rows");
    return TL_OK;
}

}  // namespace tl
