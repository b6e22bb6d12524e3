// KV swap: whole pages of every pool out of / back into the pools in ONE launch each (include/tinyllm_engine.h "KV swap",
// tl_kv_gather_pages / tl_kv_scatter_pages).  tl_engine_park moves a sequence's K/V to a pinned host arena through a
// contiguous device staging buffer: gather + one device-to-host copy per group of pages instead of one copy per (page, pool) --
// 72 pools at Qwen3-4B, 144 with FP8 scales.
//
// Pools are kv_copy.h's: [pages][heads][page_size][row_bytes] bytes each, named by a device table.  The staging buffer holds PAGE RECORDS:
// record j (of page page_ids[j]) lies at j * record_bytes and holds, pool after pool in table order, that pool's
// [heads][page_size][row_bytes_i] bytes; record_offsets[i] = heads * page_size * sum_{k < i} row_bytes_k is summed once on the host.
// Of the LAST page only rows [0, tail_rows) of every head move; the rest of its record (gather) / of the page (scatter) is left as it was.
//
// One workgroup per (page, pool, head): inside it the rows are one contiguous run on both sides, moved exactly as kv_copy_rows_kernel
// moves it -- 16 bytes per lane where both ends and the length are 16-byte aligned, 4 bytes per lane where they are 4-byte aligned,
// single bytes otherwise.  Plain vector loads and stores, no LDS.  Block size 256: a K / V head run of a 16-token page is 4 KiB = one
// 16-byte access per lane, and a 128-token page's 32 KiB run is eight coalesced 4 KiB stripes; the launch has pages x pools x heads
// workgroups (1,152 per page at Qwen3-4B), far more than the chip holds at once, so memory-level parallelism comes from the grid and a
// larger block would only idle lanes on the short runs (scale pools: 64 B).  Not measured against other sizes (profiles/kv_swap.json).
#pragma once

#include "common.h"
#include "../../include/tinyllm_engine.h"

namespace tl {

struct KvSwapArgs {
    const tl_kv_pool_desc *pools;   // [gridDim.x / heads]
    const size_t *record_offsets;   // [gridDim.x / heads]
    const int32_t *page_ids;        // [gridDim.y]
    char *staging;
    size_t record_bytes;
    int heads, page_size, tail_rows;
};

// grid = (n_pools x heads, n_pages), block = 256.  GATHER: pools -> staging; otherwise staging -> pools
template <bool GATHER>
static __global__ __launch_bounds__(256) void kv_swap_pages_kernel(const KvSwapArgs a) {
    const int pool = blockIdx.x / a.heads, head = blockIdx.x % a.heads;
    const int j = blockIdx.y;
    const int page = a.page_ids[j];
    if (page < 0) return;  // (uniform) an empty block-table entry names no page
    const tl_kv_pool_desc d = a.pools[pool];
    const size_t head_bytes = (size_t)a.page_size * d.row_bytes;
    char *in_pool = (char *)d.base_dev + ((size_t)page * a.heads + head) * head_bytes;
    char *in_rec = a.staging + (size_t)j * a.record_bytes + a.record_offsets[pool] + (size_t)head * head_bytes;
    const char *src = GATHER ? in_pool : in_rec;
    char *dst = GATHER ? in_rec : in_pool;
    const int rows = j == (int)gridDim.y - 1 ? a.tail_rows : a.page_size;
    const size_t bytes = (size_t)rows * d.row_bytes;
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

// bytes of one page record over a HOST copy of the pool table; 0 on bad input
static inline size_t kv_page_record_bytes(const tl_kv_pool_desc *pools_host, int n_pools, int heads, int page_size) {
    if (!pools_host || n_pools < 1 || heads < 1 || page_size < 1) return 0;
    size_t row_bytes = 0;
    for (int i = 0; i < n_pools; ++i) {
        if (pools_host[i].row_bytes == 0) return 0;
        row_bytes += pools_host[i].row_bytes;
    }
    return (size_t)heads * page_size * row_bytes;
}

// stream ordered; the caller keeps the page ids inside its pools and the staging buffer at n_pages * record_bytes bytes or more
template <bool GATHER>
static inline int kv_swap_pages(const tl_kv_pool_desc *pools_dev, const size_t *record_offsets_dev, int n_pools, int heads, int page_size,
                                const int32_t *page_ids_dev, int n_pages, int tail_rows, void *staging_dev, size_t record_bytes, hipStream_t stream) {
    const char *what = GATHER ? "kv_gather_pages" : "kv_scatter_pages";
    TL_REQUIRE(pools_dev && record_offsets_dev && page_ids_dev && staging_dev, std::string(what) + ": null argument");
    TL_REQUIRE(n_pools >= 1 && heads >= 1 && page_size >= 1 && record_bytes >= 1, std::string(what) + ": need pools, heads, a page size and a record size");
    TL_REQUIRE(n_pages >= 1 && n_pages <= 65535, std::string(what) + ": between 1 and 65,535 pages per launch");
    TL_REQUIRE(tail_rows >= 1 && tail_rows <= page_size, std::string(what) + ": between 1 and page_size rows in the last page");
    TL_REQUIRE((long)n_pools * heads <= 0x7fffffffL, std::string(what) + ": too many workgroups");
    const KvSwapArgs a{pools_dev, record_offsets_dev, page_ids_dev, (char *)staging_dev, record_bytes, heads, page_size, tail_rows};
    hipLaunchKernelGGL(kv_swap_pages_kernel<GATHER>, dim3((unsigned)(n_pools * heads), (unsigned)n_pages), dim3(256), 0, stream, a);
    TL_CHECK_LAUNCH(what);
    return TL_OK;
}

}  // namespace tl
