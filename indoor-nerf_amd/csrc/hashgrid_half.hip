// fp16 hash tables for forward-only rendering (render table_precision="fp16").
//
// The image: level l at byte l * T * 4, entry h one 4-byte {f16 x, f16 y}, each fp32 table value rounded once to
// IEEE binary16, round to nearest even (subnormals kept, overflow to +-inf, NaN stays NaN). A level is 2 MiB at
// log2_T = 19 instead of 4 MiB: half of an XCD's L2 instead of all of it.
//
// The gather (hash_encode_fwd_half_pair_kernel) is hashgrid.hip's lane-pair forward with one 4-byte load per
// corner: the same voxel math (fwd_axes, div_rn, the fast-division gate, the box / keep rule), the same grid
// (level-major rows, grouped coarse levels, kFwdRowPts points per thread on the single-level rows), the same
// blend and store (fwd_finish<false>). The corners stay raw 32-bit words until the finish step widens them
// exactly, so a level in flight holds 4 VGPRs of entries instead of 8. Its features and keep flags are
// therefore, bit for bit, nerf_hash_encode_fwd's on tables replaced by half(t) widened back to fp32.
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <algorithm>

#include "hash_common.h"

namespace nerf {

// ---- fp32 tables -> the fp16 image ------------------------------------------------------------------
struct HalfSrc {
    const float* tables[NERF_MAX_LEVELS];
};

// __float2half_rn: v_cvt_f16_f32 in the default rounding mode (nearest even), never the round-toward-zero pack
__device__ __forceinline__ uint32_t half_entry(float x, float y) {
    return (uint32_t)__half_as_ushort(__float2half_rn(x)) | ((uint32_t)__half_as_ushort(__float2half_rn(y)) << 16);
}

// grid (blocks, levels): a lane reads 2 x 16 B (four entries) and writes their 16 B of the image
__global__ void __launch_bounds__(256) hash_tables_to_half_kernel(HalfSrc src, int64_t T, uint32_t* __restrict__ out) {
    const int lvl = (int)blockIdx.y;
    const float4* __restrict__ in = reinterpret_cast<const float4*>(src.tables[lvl]);
    uint4* __restrict__ o = reinterpret_cast<uint4*>(out + (size_t)lvl * (size_t)T);
    const int64_t n = T >> 2, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float4 a = in[2 * i], b = in[2 * i + 1];
        o[i] = make_uint4(half_entry(a.x, a.y), half_entry(a.z, a.w), half_entry(b.x, b.y), half_entry(b.z, b.w));
    }
}

// tables of fewer than four entries, or buffers off a 16-B boundary: one entry per lane
__global__ void __launch_bounds__(256) hash_tables_to_half_entry_kernel(HalfSrc src, int64_t T,
                                                                        uint32_t* __restrict__ out) {
    const int lvl = (int)blockIdx.y;
    const float2* __restrict__ in = reinterpret_cast<const float2*>(src.tables[lvl]);
    uint32_t* __restrict__ o = out + (size_t)lvl * (size_t)T;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += stride) {
        const float2 e = in[i];
        o[i] = half_entry(e.x, e.y);
    }
}

// ---- the gather ---------------------------------------------------------------------------------------
// FwdLvlHalf, fwd_gather_half and the exact widening live in hash_common.h (the packed-feature kernel of
// hashgrid_pkbf.hip gathers the same way)
__device__ __forceinline__ void fwd_finish_half(const FwdLvlHalf& h, int lvl, int xb, bool valid, int64_t p,
                                                float* __restrict__ feat, int64_t sp, int64_t sl,
                                                uint8_t* __restrict__ keep) {
    FwdLvl s = fwd_widen_half(h);
    fwd_finish<false>(s, lvl, xb, valid, p, feat, sp, sl, keep, nullptr);
}

// Points per thread on the single-level rows and levels per grouped round: the fp32 kernel's. The halved register
// cost of a level in flight would allow more of either; both were measured and rejected (DESIGN.md §18,
// tools/variants/half_row_pts4_rejected.diff, tools/variants/half_group_round3_rejected.diff).
constexpr int kHalfRowPts = kFwdRowPts;
constexpr int kHalfGroupRound = kFwdGroupRound;

// hash_encode_fwd_pair_kernel<false> (hashgrid.hip) on the image: same grid, same rows, same points per thread
__global__ void __launch_bounds__(256) hash_encode_fwd_half_pair_kernel(
    const float* __restrict__ xyz, int64_t n, HashParams hp, int group, unsigned gx0, unsigned gx1,
    float* __restrict__ feat, int64_t sp, int64_t sl, uint8_t* __restrict__ keep) {
    const unsigned b = blockIdx.x;
    const int xb = (int)(threadIdx.x & 1);
    if (group > 0 && b < gx0) {
        const int64_t p = ((int64_t)b * blockDim.x + threadIdx.x) >> 1;
        const bool valid = p < n;
        const int64_t pc = valid ? p : n - 1;         // invalid lanes mirror a valid point (no stores)
        const float x = xyz[3 * pc + 0], y = xyz[3 * pc + 1], z = xyz[3 * pc + 2];
        const bool fast = hp.fastdiv && __ballot(!fastdiv_point_ok(x, y, z)) == 0ull;   // wave-uniform
        for (int l0 = 0; l0 < group; l0 += kHalfGroupRound) {
            FwdLvlHalf s[kHalfGroupRound];
#pragma unroll
            for (int g = 0; g < kHalfGroupRound; ++g) {
                if (l0 + g < group) {
                    if (fast) fwd_gather_half<true>(x, y, z, hp, l0 + g, xb, s[g]);
                    else fwd_gather_half<false>(x, y, z, hp, l0 + g, xb, s[g]);
                }
            }
#pragma unroll
            for (int g = 0; g < kHalfGroupRound; ++g)
                if (l0 + g < group) fwd_finish_half(s[g], l0 + g, xb, valid, pc, feat, sp, sl, keep);
        }
        return;
    }
    const unsigned r = group > 0 ? b - gx0 : b;
    const int lvl = (group > 0 ? group : 0) + (int)(r / gx1);
    const int64_t p0 = (int64_t)(r % gx1) * (128 * kHalfRowPts) + (threadIdx.x >> 1);
    int64_t pc[kHalfRowPts];
    bool valid[kHalfRowPts];
    float x[kHalfRowPts], y[kHalfRowPts], z[kHalfRowPts];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kHalfRowPts; ++k) {
        const int64_t p = p0 + 128 * k;
        valid[k] = p < n;
        pc[k] = valid[k] ? p : n - 1;
        x[k] = xyz[3 * pc[k] + 0]; y[k] = xyz[3 * pc[k] + 1]; z[k] = xyz[3 * pc[k] + 2];
        ok = ok && fastdiv_point_ok(x[k], y[k], z[k]);
    }
    const bool fast = hp.fastdiv && __ballot(!ok) == 0ull;
    FwdLvlHalf s[kHalfRowPts];
#pragma unroll
    for (int k = 0; k < kHalfRowPts; ++k) {
        if (fast) fwd_gather_half<true>(x[k], y[k], z[k], hp, lvl, xb, s[k]);
        else fwd_gather_half<false>(x[k], y[k], z[k], hp, lvl, xb, s[k]);
    }
#pragma unroll
    for (int k = 0; k < kHalfRowPts; ++k) fwd_finish_half(s[k], lvl, xb, valid[k], pc[k], feat, sp, sl, keep);
}

}  // namespace nerf

using namespace nerf;

extern "C" size_t nerf_hash_half_bytes(int n_levels, int log2_T) {
    if (n_levels < 1 || n_levels > NERF_MAX_LEVELS || log2_T < 1 || log2_T > 30) return 0;
    return (size_t)n_levels * ((size_t)1 << log2_T) * 4;
}

extern "C" int nerf_hash_tables_to_half(const float* const* d_tables, int n_levels, int log2_T, void* d_half,
                                        void* stream) {
    NERF_REQUIRE(n_levels >= 1 && n_levels <= NERF_MAX_LEVELS, "hash_tables_to_half: n_levels %d", n_levels);
    NERF_REQUIRE(log2_T >= 1 && log2_T <= 30, "hash_tables_to_half: log2_T %d", log2_T);
    NERF_REQUIRE(d_tables && d_half, "hash_tables_to_half: null arg");
    HalfSrc src{};
    bool vec = log2_T >= 2 && (reinterpret_cast<uintptr_t>(d_half) & 15u) == 0;
    for (int l = 0; l < n_levels; ++l) {
        NERF_REQUIRE(d_tables[l], "hash_tables_to_half: table %d is null", l);
        src.tables[l] = d_tables[l];
        vec = vec && (reinterpret_cast<uintptr_t>(d_tables[l]) & 15u) == 0;
    }
    const int64_t T = (int64_t)1 << log2_T;
    uint32_t* out = reinterpret_cast<uint32_t*>(d_half);
    if (vec) {
        const dim3 grid((unsigned)std::min<int64_t>(blocks_for(T >> 2, 256), 4096), (unsigned)n_levels);
        hipLaunchKernelGGL(hash_tables_to_half_kernel, grid, dim3(256), 0, as_stream(stream), src, T, out);
    } else {
        const dim3 grid((unsigned)std::min<int64_t>(blocks_for(T, 256), 4096), (unsigned)n_levels);
        hipLaunchKernelGGL(hash_tables_to_half_entry_kernel, grid, dim3(256), 0, as_stream(stream), src, T, out);
    }
    NERF_CHECK_LAUNCH("hash_tables_to_half");
    return NERF_OK;
}

extern "C" int nerf_hash_encode_fwd_half(const float* d_xyz, int64_t n_points, const float* bbox_min3,
                                         const float* bbox_max3, const float* level_res, int n_levels, int log2_T,
                                         const void* d_half, float* d_feat, int64_t feat_stride_point,
                                         int64_t feat_stride_level, uint8_t* d_keep, void* stream) {
    HashParams hp{};
    int group = 0;
    const int rc = fwd_host_params("hash_encode_fwd_half", d_xyz, n_points, bbox_min3, bbox_max3, level_res, n_levels,
                                   log2_T, d_half != nullptr, d_feat, hp, group);
    if (rc != NERF_OK || n_points == 0) return rc;
    const size_t level_bytes = ((size_t)1 << log2_T) * 4;
    for (int l = 0; l < n_levels; ++l)   // the kernel reads a level's base as the image's 4-byte entries
        hp.tables[l] = reinterpret_cast<const float*>(static_cast<const char*>(d_half) + (size_t)l * level_bytes);
    return fwd_for_ranges(n_points, n_levels, group, kHalfRowPts,
                          [&](int64_t p0, int64_t n, unsigned nb, unsigned gx0, unsigned gx1) -> int {
        hipLaunchKernelGGL(hash_encode_fwd_half_pair_kernel, dim3(nb), dim3(256), 0, as_stream(stream),
                           d_xyz + 3 * p0, n, hp, group, gx0, gx1, d_feat + p0 * feat_stride_point,
                           feat_stride_point, feat_stride_level, d_keep ? d_keep + p0 : nullptr);
        NERF_CHECK_LAUNCH("hash_encode_fwd_half");
        return NERF_OK;
    });
}
