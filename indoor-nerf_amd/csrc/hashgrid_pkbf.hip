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
