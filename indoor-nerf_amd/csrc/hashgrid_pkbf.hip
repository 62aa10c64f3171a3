// Packed bf16 hash features for forward-only rendering (render feature_precision="bf16").
//
// The bf16 MLP forward (field_x6.hip mlp_fwd_bf16_kernel) rounds each of a point's 32 fp32 features to bf16 before
// anything else, round to nearest even (v_cvt_pk_bf16_f32). The encoder here does that rounding itself and writes
// one 4-byte word {bf16 f0, bf16 f1} per (point, level) instead of a float2: a point writes 64 B of features and
// the MLP (mlp_fwd_bf16_kernel<true>) reads back 64 B, instead of 128 B each way, and uses the word as its matrix
// operand as it is.
//
// The kernel is hashgrid.hip's lane-pair forward (HALF: hashgrid_half.hip's, on the fp16 image): the same voxel
// math (fwd_axes, div_rn, the fast-division gate, the box / keep rule), the same gathers (fwd_gather /
// fwd_gather_half), the same grid (level-major rows, grouped coarse levels, kFwdRowPts points per thread on the
// single-level rows) and the same blend (fwd_blend). Only the store differs (fwd_finish_pkbf): after the blend
// both lanes of a pair hold both features, so lane 0 converts the pair once and stores one dword, and lane 1
// stores nothing. The words are therefore, bit for bit, pk_bf16 of the features the unpacked entry writes.
#include <stdint.h>

#include <atomic>

#include "hash_common.h"

namespace nerf {

template <bool HALF>
struct PkLvl {
    using type = FwdLvl;
};
template <>
struct PkLvl<true> {
    using type = FwdLvlHalf;
};

template <bool HALF, bool FAST>
__device__ __forceinline__ void pk_gather(float x, float y, float z, const HashParams& hp, int lvl, int xb,
                                          typename PkLvl<HALF>::type& s) {
    if constexpr (HALF) fwd_gather_half<FAST>(x, y, z, hp, lvl, xb, s);
    else fwd_gather<FAST>(x, y, z, hp, lvl, xb, s);
}

template <bool HALF>
__device__ __forceinline__ void pk_finish(typename PkLvl<HALF>::type& g, int lvl, int xb, bool valid, int64_t p,
                                          uint32_t* __restrict__ featw, int64_t sp, int64_t sl,
                                          uint8_t* __restrict__ keep) {
    if constexpr (HALF) {
        FwdLvl s = fwd_widen_half(g);
        fwd_finish_pkbf(s, lvl, xb, valid, p, featw, sp, sl, keep);
    } else {
        fwd_finish_pkbf(g, lvl, xb, valid, p, featw, sp, sl, keep);
    }
}

// hash_encode_fwd_pair_kernel<false> (hashgrid.hip) / hash_encode_fwd_half_pair_kernel (hashgrid_half.hip) with the
// packed store: same grid, same rows, same points per thread. sp, sl: strides of featw in words.
// KEEP IN STEP: pkbf_block below restates this body for the device-sized kernel; a change here is made there too.
template <bool HALF>
__global__ void __launch_bounds__(256) hash_encode_fwd_pkbf_kernel(
    const float* __restrict__ xyz, int64_t n, HashParams hp, int group, unsigned gx0, unsigned gx1,
    uint32_t* __restrict__ featw, int64_t sp, int64_t sl, uint8_t* __restrict__ keep) {
    using Lvl = typename PkLvl<HALF>::type;
    const unsigned b = blockIdx.x;
    const int xb = (int)(threadIdx.x & 1);
    if (group > 0 && b < gx0) {
        const int64_t p = ((int64_t)b * blockDim.x + threadIdx.x) >> 1;
        const bool valid = p < n;
        const int64_t pc = valid ? p : n - 1;         // invalid lanes mirror a valid point (no stores)
        const float x = xyz[3 * pc + 0], y = xyz[3 * pc + 1], z = xyz[3 * pc + 2];
        const bool fast = hp.fastdiv && __ballot(!fastdiv_point_ok(x, y, z)) == 0ull;   // wave-uniform
        for (int l0 = 0; l0 < group; l0 += kFwdGroupRound) {
            Lvl s[kFwdGroupRound];
#pragma unroll
            for (int g = 0; g < kFwdGroupRound; ++g) {
                if (l0 + g < group) {
                    if (fast) pk_gather<HALF, true>(x, y, z, hp, l0 + g, xb, s[g]);
                    else pk_gather<HALF, false>(x, y, z, hp, l0 + g, xb, s[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < kFwdGroupRound; ++g)
                if (l0 + g < group) pk_finish<HALF>(s[g], l0 + g, xb, valid, pc, featw, sp, sl, keep);
        }
        return;
    }
    const unsigned r = group > 0 ? b - gx0 : b;
    const int lvl = (group > 0 ? group : 0) + (int)(r / gx1);
    const int64_t p0 = (int64_t)(r % gx1) * (128 * kFwdRowPts) + (threadIdx.x >> 1);
    int64_t pc[kFwdRowPts];
    bool valid[kFwdRowPts];
    float x[kFwdRowPts], y[kFwdRowPts], z[kFwdRowPts];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kFwdRowPts; ++k) {
        const int64_t p = p0 + 128 * k;
        valid[k] = p < n;
        pc[k] = valid[k] ? p : n - 1;
        x[k] = xyz[3 * pc[k] + 0]; y[k] = xyz[3 * pc[k] + 1]; z[k] = xyz[3 * pc[k] + 2];
        ok = ok && fastdiv_point_ok(x[k], y[k], z[k]);
    }
    const bool fast = hp.fastdiv && __ballot(!ok) == 0ull;
    Lvl s[kFwdRowPts];
#pragma unroll
    for (int k = 0; k < kFwdRowPts; ++k) {
        if (fast) pk_gather<HALF, true>(x[k], y[k], z[k], hp, lvl, xb, s[k]);
        else pk_gather<HALF, false>(x[k], y[k], z[k], hp, lvl, xb, s[k]);
    }
#pragma unroll
    for (int k = 0; k < kFwdRowPts; ++k) pk_finish<HALF>(s[k], lvl, xb, valid[k], pc[k], featw, sp, sl, keep);
}

// Block b of hash_encode_fwd_pkbf_kernel's grid for n >= 1 points, for the device-sized kernel below, where b is a
// virtual block: that kernel's body restated line for line (b in place of blockIdx.x). The host-sized kernel does
// not call it: routed through a shared function the compiler schedules it differently, and its instructions are
// kept as they are. KEEP IN STEP with that kernel; fold the two together once its instructions may change.
template <bool HALF>
__device__ __forceinline__ void pkbf_block(const unsigned b, const float* __restrict__ xyz, int64_t n,
                                           const HashParams& hp, int group, unsigned gx0, unsigned gx1,
                                           uint32_t* __restrict__ featw, int64_t sp, int64_t sl,
                                           uint8_t* __restrict__ keep) {
    using Lvl = typename PkLvl<HALF>::type;
    const int xb = (int)(threadIdx.x & 1);
    if (group > 0 && b < gx0) {
        const int64_t p = ((int64_t)b * blockDim.x + threadIdx.x) >> 1;
        const bool valid = p < n;
        const int64_t pc = valid ? p : n - 1;         // invalid lanes mirror a valid point (no stores)
        const float x = xyz[3 * pc + 0], y = xyz[3 * pc + 1], z = xyz[3 * pc + 2];
        const bool fast = hp.fastdiv && __ballot(!fastdiv_point_ok(x, y, z)) == 0ull;   // wave-uniform
        for (int l0 = 0; l0 < group; l0 += kFwdGroupRound) {
            Lvl s[kFwdGroupRound];
#pragma unroll
            for (int g = 0; g < kFwdGroupRound; ++g) {
                if (l0 + g < group) {
                    if (fast) pk_gather<HALF, true>(x, y, z, hp, l0 + g, xb, s[g]);
                    else pk_gather<HALF, false>(x, y, z, hp, l0 + g, xb, s[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < kFwdGroupRound; ++g)
                if (l0 + g < group) pk_finish<HALF>(s[g], l0 + g, xb, valid, pc, featw, sp, sl, keep);
        }
        return;
    }
    const unsigned r = group > 0 ? b - gx0 : b;
    const int lvl = (group > 0 ? group : 0) + (int)(r / gx1);
    const int64_t p0 = (int64_t)(r % gx1) * (128 * kFwdRowPts) + (threadIdx.x >> 1);
    int64_t pc[kFwdRowPts];
    bool valid[kFwdRowPts];
    float x[kFwdRowPts], y[kFwdRowPts], z[kFwdRowPts];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kFwdRowPts; ++k) {
        const int64_t p = p0 + 128 * k;
        valid[k] = p < n;
        pc[k] = valid[k] ? p : n - 1;
        x[k] = xyz[3 * pc[k] + 0]; y[k] = xyz[3 * pc[k] + 1]; z[k] = xyz[3 * pc[k] + 2];
        ok = ok && fastdiv_point_ok(x[k], y[k], z[k]);
    }
    const bool fast = hp.fastdiv && __ballot(!ok) == 0ull;
    Lvl s[kFwdRowPts];
#pragma unroll
    for (int k = 0; k < kFwdRowPts; ++k) {
        if (fast) pk_gather<HALF, true>(x[k], y[k], z[k], hp, lvl, xb, s[k]);
        else pk_gather<HALF, false>(x[k], y[k], z[k], hp, lvl, xb, s[k]);
    }
#pragma unroll
    for (int k = 0; k < kFwdRowPts; ++k) pk_finish<HALF>(s[k], lvl, xb, valid[k], pc[k], featw, sp, sl, keep);
}

// The point count read on the device (render march_sizes="device"): the launch covers
// n = clamp(*total - base, 0, capacity) points. The grid is fixed by the capacity (launch_fwd_pkbf_dev); every block
// forms the grid of n points as fwd_for_ranges does on the host (gx0 grouped blocks, gx1 per single-level row) and
// walks its virtual blocks b = blockIdx.x, += gridDim.x: still level-major, so the blocks in flight at any time share
// a level's table as in the host-sized launch. A virtual block is pkbf_block, the host-sized kernel's body restated, so a
// point's words and keep byte are that kernel's, bit for bit: which block computes a point is all that changes.
// n == 0: every block returns after the one scalar load of the count; no point is read (the n - 1 mirror row of
// invalid lanes does not exist then) and nothing is written. Nothing at or beyond entry n is ever written: the
// stores are pkbf_block's, under valid = p < n. No block waits for another, so residency is not needed.
template <bool HALF>
__global__ void __launch_bounds__(256) hash_encode_fwd_pkbf_dev_kernel(
    const float* __restrict__ xyz, const int32_t* __restrict__ total, int64_t base, int64_t capacity, HashParams hp,
    int group, int single_levels, uint32_t* __restrict__ featw, int64_t sp, int64_t sl, uint8_t* __restrict__ keep) {
    int64_t n = (int64_t)*total - base;
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    if (n == 0) return;   // uniform over the grid
    const unsigned gx0 = group > 0 ? (unsigned)((2 * n + 255) / 256) : 0u;
    const unsigned gx1 = (unsigned)((2 * n + 256 * kFwdRowPts - 1) / (256 * kFwdRowPts));
    const unsigned nb = gx0 + gx1 * (unsigned)single_levels;   // <= the capacity's, below 2^32 / 256 (the host checks)
    for (unsigned b = blockIdx.x; b < nb; b += gridDim.x)
        pkbf_block<HALF>(b, xyz, n, hp, group, gx0, gx1, featw, sp, sl, keep);
}

// hp's tables are set; the launches of both entries
template <bool HALF>
static int launch_fwd_pkbf(const char* who, const float* d_xyz, int64_t n_points, int n_levels, int group,
                           const HashParams& hp, uint32_t* d_featw, int64_t sp, int64_t sl, uint8_t* d_keep,
                           void* stream) {
    return fwd_for_ranges(n_points, n_levels, group, kFwdRowPts,
                          [&](int64_t p0, int64_t n, unsigned nb, unsigned gx0, unsigned gx1) -> int {
        hipLaunchKernelGGL(hash_encode_fwd_pkbf_kernel<HALF>, dim3(nb), dim3(256), 0, as_stream(stream),
                           d_xyz + 3 * p0, n, hp, group, gx0, gx1, d_featw + p0 * sp, sp, sl,
                           d_keep ? d_keep + p0 : nullptr);
        NERF_CHECK_LAUNCH(who);
        return NERF_OK;
    });
}

// Resident blocks per CU the default grid of the device-sized launch assumes (256-thread blocks)
constexpr int kFwdDevBlocksPerCu = 8;

// The default grid cap: the current device's CU count times kFwdDevBlocksPerCu. The count is asked once per device
// and kept: this sits on a path whose point is to have no host work between launches.
static int fwd_dev_default_blocks() {
    constexpr int kMaxDevices = 64;
    static std::atomic<int> cus_of[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256 * kFwdDevBlocksPerCu;
    int cus = cus_of[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        cus_of[dev].store(cus, std::memory_order_relaxed);
    }
    return cus * kFwdDevBlocksPerCu;
}

// hp's tables are set; the launch of both device-sized entries. One launch: the virtual blocks of `capacity` points
// must fit one grid's index range (fwd_for_ranges would split there; 2^24 blocks is ~10^8 points at 16 levels,
// beyond the MLP's 32-bit row indexing), and the grid is min(those, max_blocks).
template <bool HALF>
static int launch_fwd_pkbf_dev(const char* who, const float* d_xyz, const int32_t* d_total, int64_t base,
                               int64_t capacity, int max_blocks, int n_levels, int group, const HashParams& hp,
                               uint32_t* d_featw, int64_t sp, int64_t sl, uint8_t* d_keep, void* stream) {
    const int single = n_levels - (group > 0 ? group : 0);
    const uint64_t gx0 = group > 0 ? (uint64_t)blocks_for(2 * capacity, 256) : 0u;
    const uint64_t nb = gx0 + (uint64_t)blocks_for(2 * capacity, 256 * kFwdRowPts) * (uint64_t)single;
    NERF_REQUIRE(capacity <= ((int64_t)1 << 30) && nb <= 0xFFFFFFFFull / 256,
                 "%s: capacity %lld exceeds one launch", who, (long long)capacity);
    if (max_blocks == 0) max_blocks = fwd_dev_default_blocks();
    const unsigned grid = (unsigned)(nb < (uint64_t)max_blocks ? nb : (uint64_t)max_blocks);
    hipLaunchKernelGGL(hash_encode_fwd_pkbf_dev_kernel<HALF>, dim3(grid), dim3(256), 0, as_stream(stream), d_xyz,
                       d_total, base, capacity, hp, group, single, d_featw, sp, sl, d_keep);
    NERF_CHECK_LAUNCH(who);
    return NERF_OK;
}

// the checks of the device-sized entries that the host-sized ones do not have
static int fwd_dev_args(const char* who, const int32_t* d_total, int64_t base, int64_t capacity, int max_blocks) {
    NERF_REQUIRE(capacity >= 0, "%s: capacity < 0", who);
    NERF_REQUIRE(base >= 0, "%s: base < 0", who);
    NERF_REQUIRE(max_blocks >= 0, "%s: max_blocks < 0", who);
    NERF_REQUIRE(d_total, "%s: null count", who);
    return NERF_OK;
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_hash_encode_fwd_pkbf(const float* d_xyz, int64_t n_points, const float* bbox_min3,
                                         const float* bbox_max3, const float* level_res, int n_levels, int log2_T,
                                         const float* const* d_tables, uint32_t* d_featw, int64_t feat_stride_point,
                                         int64_t feat_stride_level, uint8_t* d_keep, void* stream) {
    HashParams hp{};
    int group = 0;
    const int rc = fwd_host_params("hash_encode_fwd_pkbf", d_xyz, n_points, bbox_min3, bbox_max3, level_res, n_levels,
                                   log2_T, d_tables != nullptr, reinterpret_cast<const float*>(d_featw), hp, group);
    if (rc != NERF_OK || n_points == 0) return rc;
    for (int l = 0; l < n_levels; ++l) {
        NERF_REQUIRE(d_tables[l], "hash_encode_fwd_pkbf: table %d is null", l);
        hp.tables[l] = d_tables[l];
    }
    return launch_fwd_pkbf<false>("hash_encode_fwd_pkbf", d_xyz, n_points, n_levels, group, hp, d_featw,
                                  feat_stride_point, feat_stride_level, d_keep, stream);
}

extern "C" int nerf_hash_encode_fwd_half_pkbf(const float* d_xyz, int64_t n_points, const float* bbox_min3,
                                              const float* bbox_max3, const float* level_res, int n_levels,
                                              int log2_T, const void* d_half, uint32_t* d_featw,
                                              int64_t feat_stride_point, int64_t feat_stride_level, uint8_t* d_keep,
                                              void* stream) {
    HashParams hp{};
    int group = 0;
    const int rc = fwd_host_params("hash_encode_fwd_half_pkbf", d_xyz, n_points, bbox_min3, bbox_max3, level_res,
                                   n_levels, log2_T, d_half != nullptr, reinterpret_cast<const float*>(d_featw), hp,
                                   group);
    if (rc != NERF_OK || n_points == 0) return rc;
    const size_t level_bytes = ((size_t)1 << log2_T) * 4;
    for (int l = 0; l < n_levels; ++l)   // the kernel reads a level's base as the image's 4-byte entries
        hp.tables[l] = reinterpret_cast<const float*>(static_cast<const char*>(d_half) + (size_t)l * level_bytes);
    return launch_fwd_pkbf<true>("hash_encode_fwd_half_pkbf", d_xyz, n_points, n_levels, group, hp, d_featw,
                                 feat_stride_point, feat_stride_level, d_keep, stream);
}

// The two entries above with the point count read on the device (hash_encode_fwd_pkbf_dev_kernel): d_xyz, d_featw and
// d_keep point at the slice's first point, whose number in the list is `base`; the launch covers
// clamp(*d_total - base, 0, capacity) points. capacity == 0 launches nothing.
extern "C" int nerf_hash_encode_fwd_pkbf_dev(const float* d_xyz, const int32_t* d_total, int64_t base, int64_t capacity,
                                             int max_blocks, const float* bbox_min3, const float* bbox_max3,
                                             const float* level_res, int n_levels, int log2_T,
                                             const float* const* d_tables, uint32_t* d_featw,
                                             int64_t feat_stride_point, int64_t feat_stride_level, uint8_t* d_keep,
                                             void* stream) {
    const char* who = "hash_encode_fwd_pkbf_dev";
    int rc = fwd_dev_args(who, d_total, base, capacity, max_blocks);
    if (rc != NERF_OK) return rc;
    HashParams hp{};
    int group = 0;
    rc = fwd_host_params(who, d_xyz, capacity, bbox_min3, bbox_max3, level_res, n_levels, log2_T, d_tables != nullptr,
                         reinterpret_cast<const float*>(d_featw), hp, group);
    if (rc != NERF_OK || capacity == 0) return rc;
    for (int l = 0; l < n_levels; ++l) {
        NERF_REQUIRE(d_tables[l], "hash_encode_fwd_pkbf_dev: table %d is null", l);
        hp.tables[l] = d_tables[l];
    }
    return launch_fwd_pkbf_dev<false>(who, d_xyz, d_total, base, capacity, max_blocks, n_levels, group, hp, d_featw,
                                      feat_stride_point, feat_stride_level, d_keep, stream);
}

extern "C" int nerf_hash_encode_fwd_half_pkbf_dev(const float* d_xyz, const int32_t* d_total, int64_t base,
                                                  int64_t capacity, int max_blocks, const float* bbox_min3,
                                                  const float* bbox_max3, const float* level_res, int n_levels,
                                                  int log2_T, const void* d_half, uint32_t* d_featw,
                                                  int64_t feat_stride_point, int64_t feat_stride_level,
                                                  uint8_t* d_keep, void* stream) {
    const char* who = "hash_encode_fwd_half_pkbf_dev";
    int rc = fwd_dev_args(who, d_total, base, capacity, max_blocks);
    if (rc != NERF_OK) return rc;
    HashParams hp{};
    int group = 0;
    rc = fwd_host_params(who, d_xyz, capacity, bbox_min3, bbox_max3, level_res, n_levels, log2_T, d_half != nullptr,
                         reinterpret_cast<const float*>(d_featw), hp, group);
    if (rc != NERF_OK || capacity == 0) return rc;
    const size_t level_bytes = ((size_t)1 << log2_T) * 4;
    for (int l = 0; l < n_levels; ++l)
        hp.tables[l] = reinterpret_cast<const float*>(static_cast<const char*>(d_half) + (size_t)l * level_bytes);
    return launch_fwd_pkbf_dev<true>(who, d_xyz, d_total, base, capacity, max_blocks, n_levels, group, hp, d_featw,
                                     feat_stride_point, feat_stride_level, d_keep, stream);
}
