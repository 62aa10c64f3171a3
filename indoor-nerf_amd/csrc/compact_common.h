// Stable compaction of the forward-only render paths: the kept items of a list, in ascending order, in two
// launches with one workspace of a count per block. Used by the point compaction (sparse_points.hip) and the
// ray gather (ray_span.hip). active.hip has the same scheme over two lists at once, on the training path; it
// stays on its own copy until a change there is measured by the training benchmark.
//
// Item k of thread t of block b is b * kCompactBlock + k * kCompactThreads + t: consecutive threads hold
// consecutive items, so a wave holds 64 consecutive items in lane order, the block's four waves 256
// consecutive items in wave order, and iteration k comes before iteration k + 1.
//   (1) count: every block stores the number of its kept items in block_counts[b] (compact_count);
//   (2) write: a block starts at the sum of the counts of the blocks before it (compact_block_offset) and, per
//       iteration, a kept item's rank is that base + the kept items of the waves before its own + the kept
//       lanes below its own in the wave's ballot (compact_place, which hands the rank to the caller's write).
// Why it is stable and deterministic: every term of a rank counts the kept items that precede the item in the
// order above, so the output is ascending in the item index whatever order blocks and waves run in; the only
// atomics are integer adds, whose sums do not depend on the order.
#pragma once
#include <algorithm>

#include "common.h"

namespace nerf {

constexpr int kCompactThreads = 256;
constexpr int kCompactWaves = kCompactThreads / 64;
constexpr int kCompactPer = 16;                                   // items per thread
constexpr int kCompactBlock = kCompactThreads * kCompactPer;      // 4096 items per block

// bytes of block_counts for n items (at least one count)
inline size_t compact_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return (size_t)std::max<int64_t>(1, (n + kCompactBlock - 1) / kCompactBlock) * sizeof(int32_t);
}

// item k of this thread (see above); the caller compares it with the number of items
__device__ __forceinline__ int64_t compact_item(int k) {
    return (int64_t)blockIdx.x * kCompactBlock + k * kCompactThreads + threadIdx.x;
}

// The count side: n = this thread's kept items. Stores the block's count and adds it to *total.
// Call once per kernel, from all threads.
__device__ __forceinline__ void compact_count(int n, int32_t* __restrict__ block_counts, int32_t* __restrict__ total) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __shared__ int s[kCompactWaves];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < kCompactWaves; ++i) t += s[i];
        block_counts[blockIdx.x] = t;
        if (t) atomicAdd(total, t);   // integer: the total does not depend on the order
    }
}

// The block offset: sum of block_counts[0, blockIdx.x), RETURNED TO EVERY THREAD (each thread sums the wave
// totals from LDS itself; nothing the caller needs stays in LDS). A thread adds more than one count only from
// block kCompactThreads + 1 on. Call once per kernel, from all threads; ends in a __syncthreads().
__device__ __forceinline__ int64_t compact_block_offset(const int32_t* __restrict__ block_counts) {
    const int b = blockIdx.x;
    int off = 0;
    for (int i = threadIdx.x; i < b; i += kCompactThreads) off += block_counts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    __shared__ int s_off[kCompactWaves];
    if ((threadIdx.x & 63) == 0) s_off[threadIdx.x >> 6] = off;
    __syncthreads();
    int64_t base = 0;
    for (int i = 0; i < kCompactWaves; ++i) base += s_off[i];
    __syncthreads();
    return base;
}

// The rank of one iteration: `on` = this thread's item is kept, `base` = the kept items before this
// iteration's 256 (compact_block_offset at first). Calls write(rank) for a kept item and advances base past
// the iteration. Call from all threads, once per iteration, from one place in the kernel: two __syncthreads()
// inside, the write between them (a wave's stores overlap the wait for the others: with the write after the
// second barrier a 128-block scatter measured about 2 us longer on the MI355X), the second one after every
// thread has read the waves' counts.
template <typename Write>
__device__ __forceinline__ void compact_place(bool on, int64_t& base, Write write) {
    __shared__ int s_cnt[kCompactWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t m = __ballot(on);
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (lane == 0) s_cnt[w] = __popcll(m);
    __syncthreads();
    int64_t idx = base + __popcll(m & below);
    for (int i = 0; i < w; ++i) idx += s_cnt[i];
    if (on) write(idx);
    for (int i = 0; i < kCompactWaves; ++i) base += s_cnt[i];
    __syncthreads();
}

}  // namespace nerf
