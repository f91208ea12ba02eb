// kv_copy.hip — copy whole KV blocks inside the GPU pools (prefix caching by block copy; no reference counterpart).
//
// One launch copies block src_ids[i] -> block dst_ids[i] in the K pool and in the V pool for every pair i. The id arrays
// are DEVICE arrays (uploaded with the block manager's pinned staging), so there is no host sync and no runtime call per
// block: swap_blocks.hip's way (one hipMemcpyAsync per run of consecutive ids per pool) costs the model thread two runtime
// calls per run, and the blocks of a cached prefix are scattered.
//
// The kernel works on bytes — a block is one contiguous run of block_bytes in each pool ([num_blocks, L, KVH, 16, D]) —
// so 16-bit and FP8 pools take the same entry. Grid (pair, slice of the block, pool): a workgroup of 256 lanes moves one
// 16 KiB slice, kVecs 16-byte loads per lane all issued before the first store; a copy of one 1 MiB block is already 128
// workgroups. Byte offsets are 64-bit (id * block_bytes passes 2^32 in product pools). A pair with src == dst or with an
// id outside [0, num_blocks) is skipped — the ids are wave-uniform, so the whole workgroup leaves together. No LDS, no
// atomics; plain vector stores. The distinct destinations must be disjoint from the sources (the caller's guarantee).
#include "swl_common.h"

namespace swl {

constexpr int kCopyLanes = 256;
constexpr int kCopyVecs = 4;                                   // 16-byte vectors per lane
constexpr int64_t kCopySlice = int64_t(kCopyLanes) * kCopyVecs; // vectors per workgroup: 16 KiB

typedef uint32_t copy_vec_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kCopyLanes) void kv_copy_blocks_kernel(
    char *k_cache, char *v_cache, const int *__restrict__ src_ids, const int *__restrict__ dst_ids,
    int64_t block_vecs, int64_t num_blocks) {
    const int64_t s = src_ids[blockIdx.x], d = dst_ids[blockIdx.x];
    if (s == d || s < 0 || s >= num_blocks || d < 0 || d >= num_blocks) return;
    char *pool = blockIdx.z ? v_cache : k_cache;
    const copy_vec_t *src = reinterpret_cast<const copy_vec_t *>(pool) + s * block_vecs;
    copy_vec_t *dst = reinterpret_cast<copy_vec_t *>(pool) + d * block_vecs;
    const int64_t at = blockIdx.y * kCopySlice + threadIdx.x;
    // The loads are unconditional — past the block's end a lane re-reads the block's last vector (in bounds, never
    // stored) — so that all of them are in flight before the first store; a load under a per-lane condition is waited for
    // on the spot. Non-temporal: the source is read once.
    const int64_t last = block_vecs - 1;
    copy_vec_t r[kCopyVecs];
#pragma unroll
    for (int u = 0; u < kCopyVecs; ++u) {
        const int64_t i = at + u * kCopyLanes;
        r[u] = __builtin_nontemporal_load(src + (i < last ? i : last));
    }
    // (ties the four results to this point: without it hipcc sinks a load into the conditional block of its store)
    asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]));
    static_assert(kCopyVecs == 4, "the tie above names four vectors");
#pragma unroll
    for (int u = 0; u < kCopyVecs; ++u) {
        const int64_t i = at + u * kCopyLanes;
        if (i < block_vecs) dst[i] = r[u];
    }
}

} // namespace swl

extern "C" int swl_kv_copy_blocks(void *k_cache, void *v_cache, const int32_t *src_ids, const int32_t *dst_ids,
                                  int64_t n, int64_t block_bytes, int64_t num_blocks, swl_stream_t stream) {
    if (n < 0 || block_bytes <= 0 || num_blocks <= 0) return SWL_ERR_BAD_ARG;
    if (n == 0) return SWL_OK;
    if (!k_cache || !v_cache || !src_ids || !dst_ids) return SWL_ERR_BAD_ARG;
    if (block_bytes % 16 != 0) return SWL_ERR_UNSUPPORTED;
    if (!swl::aligned16(k_cache) || !swl::aligned16(v_cache)) return SWL_ERR_BAD_ARG;
    const int64_t block_vecs = block_bytes / 16;
    const int64_t slices = (block_vecs + swl::kCopySlice - 1) / swl::kCopySlice;
    if (n > 0x7fffffff || slices > 65535) return SWL_ERR_UNSUPPORTED;      // (grid limits: 2^31 - 1 pairs, blocks below 1 GiB)
    hipLaunchKernelGGL(swl::kv_copy_blocks_kernel, dim3(static_cast<unsigned>(n), static_cast<unsigned>(slices), 2),
                       dim3(swl::kCopyLanes), 0, static_cast<hipStream_t>(stream), static_cast<char *>(k_cache),
                       static_cast<char *>(v_cache), src_ids, dst_ids, block_vecs, num_blocks);
    return swl::check_launch();
}
