// Early ray termination for forward-only rendering.
//
// A field call over pts [R, S, 3] runs front to back in slabs [s0, s1) of samples. Every ray is alive in
// slab 0; after the field has run on a slab that is not the last, each ray still alive advances its
// optical depth over that slab's samples (ert_advance_kernel) and dies for every later slab once
// tau > tau_max = -log(eps): its transmittance is below eps, so nothing behind that point can change
// the pixel by more than eps.
//
// The rule (one thread per ray, fp32, strictly in sample order; the file is built with -ffp-contract=off,
// so no multiply-add is fused): norm_d = sqrtf(dx*dx + dy*dy + dz*dz) as composite_common.h's
// ray_forward; for i in [s0, s1): d = (z[i+1] - z[i]) * norm_d, s = sigma_i > 0 ? sigma_i : 0 (NaN gives
// 0), tau = tau + s * d. s1 < S always (no decision follows the last slab), so z[i+1] exists and
// compositing's 1e10 last delta is never needed. The same bits as its NumPy fp32 restatement
// (tests/test_gpu_early_stop.py).
//
// Compaction of one slab (ert_count_kernel / ert_scatter_kernel: occupancy.hip's wave-ballot + LDS-scan
// scheme over the R * (s1 - s0) candidates of the slab, enumerated ray-major so that the kept list is
// ascending in the point index p = r * S + s): a candidate is kept when its ray is alive, it lies inside
// the box and, with a grid, its cell is occupied (occ_common.h's cell rule). Every other candidate — every
// sample of a dead ray included — gets an all-zero raw row, which compositing gives weight 0 exactly
// (occupancy.hip, "why skipping is exact"): the result is the dense render with sigma masked per sample.
#include "occ_common.h"

namespace nerf {

constexpr int kErtThreads = 256;
constexpr int kErtPer = 16;                         // candidates per thread
constexpr int kErtBlockPts = kErtThreads * kErtPer;  // 4096 candidates per block

struct ErtCompactArgs {
    OccGrid g;
    const uint32_t* bits;    // NULL: no grid (kept = alive and inside the box)
    const float* pts;        // [R, S, 3]
    const uint8_t* alive;    // [R], or NULL: every ray is alive
    const float* sh_rays;    // [R, 40] per-ray SH records (nerf_sample_stratified_sh), or
    const float* viewdirs;   // [R, 3]
    int64_t N;               // candidates: R * (s1 - s0)
    int S, s0, width;        // samples per ray, first sample of the slab, s1 - s0
    uint32_t wd_m; int wd_s; // c / width (udiv_magic)
    int64_t capacity;        // rows of the compacted outputs
    int32_t* rows;           // out [capacity]: kept points (indices into [R * S]), ascending
    int32_t* counts;         // out [1]
    float* pts_c;            // out [capacity, 3]
    float* sh_c;             // out [capacity, 16]
    float* raw;              // [R * S, 4]: rows of the candidates not kept are zeroed
    int32_t* block_counts;   // workspace [n_blocks]
};

// candidate c < N -> its ray and its point index
__device__ __forceinline__ int64_t ert_point(const ErtCompactArgs& a, int64_t c, uint32_t& ray) {
    ray = udiv_magic((uint32_t)c, a.wd_m, a.wd_s);
    const int s = a.s0 + (int)((uint32_t)c - ray * (uint32_t)a.width);
    return (int64_t)ray * a.S + s;
}

__device__ __forceinline__ bool ert_kept(const ErtCompactArgs& a, uint32_t ray, float x, float y, float z) {
    if (a.alive && !a.alive[ray]) return false;
    int id;
    const bool inside = occ_cell(a.g, x, y, z, id);
    return inside && (!a.bits || occ_bit(a.bits, id));
}

// candidate k of thread t of block b: b * kErtBlockPts + k * kErtThreads + t
__global__ void __launch_bounds__(kErtThreads) ert_count_kernel(ErtCompactArgs a) {
    const int64_t base = (int64_t)blockIdx.x * kErtBlockPts;
    int n = 0;
#pragma unroll 4
    for (int k = 0; k < kErtPer; ++k) {
        const int64_t c = base + k * kErtThreads + threadIdx.x;
        if (c < a.N) {
            uint32_t ray;
            const int64_t p = ert_point(a, c, ray);
            if (ert_kept(a, ray, a.pts[3 * p], a.pts[3 * p + 1], a.pts[3 * p + 2])) ++n;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __shared__ int s[kErtThreads / 64];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < kErtThreads / 64; ++i) t += s[i];
        a.block_counts[blockIdx.x] = t;
        if (t) atomicAdd(a.counts, t);   // integer: the total does not depend on the order
    }
}

__global__ void __launch_bounds__(kErtThreads) ert_scatter_kernel(ErtCompactArgs a) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // this block's offset: the counts of the blocks before it
    int off = 0;
    for (int i = threadIdx.x; i < b; i += kErtThreads) off += a.block_counts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    __shared__ int s_off[kErtThreads / 64];
    __shared__ int s_cnt[kErtThreads / 64];
    if (lane == 0) s_off[w] = off;
    __syncthreads();
    int64_t base = 0;
    for (int i = 0; i < kErtThreads / 64; ++i) base += s_off[i];
    __syncthreads();
    const int64_t cbase = (int64_t)b * kErtBlockPts;
    for (int k = 0; k < kErtPer; ++k) {
        const int64_t c = cbase + k * kErtThreads + threadIdx.x;
        float x = 0.f, y = 0.f, z = 0.f;
        bool on = false;
        uint32_t ray = 0;
        int64_t p = 0;
        if (c < a.N) {
            p = ert_point(a, c, ray);
            x = a.pts[3 * p]; y = a.pts[3 * p + 1]; z = a.pts[3 * p + 2];
            on = ert_kept(a, ray, x, y, z);
            if (!on) *reinterpret_cast<float4*>(a.raw + 4 * p) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const uint64_t m = __ballot(on);
        const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        if (lane == 0) s_cnt[w] = __popcll(m);
        __syncthreads();
        int64_t idx = base + __popcll(m & below);
        for (int i = 0; i < w; ++i) idx += s_cnt[i];
        if (on && idx < a.capacity) {
            a.rows[idx] = (int32_t)p;
            a.pts_c[3 * idx] = x; a.pts_c[3 * idx + 1] = y; a.pts_c[3 * idx + 2] = z;
            float4* dst = reinterpret_cast<float4*>(a.sh_c + 16 * idx);
            if (a.sh_rays) {
                const float4* src = reinterpret_cast<const float4*>(a.sh_rays + (int64_t)kShRecord * ray);
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[q] = src[q];
            } else {
                float o[16];
                sh4_eval(a.viewdirs[3 * (int64_t)ray], a.viewdirs[3 * (int64_t)ray + 1], a.viewdirs[3 * (int64_t)ray + 2], o);
#pragma unroll
                for (int q = 0; q < 4; ++q) dst[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
            }
        }
        for (int i = 0; i < kErtThreads / 64; ++i) base += s_cnt[i];
        __syncthreads();
    }
}

// one thread per ray: R x (s1 - s0) strided sigma reads, small against the field call of the slab
__global__ void __launch_bounds__(256) ert_advance_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                          const float* __restrict__ rays_d, int64_t R, int S, int s0,
                                                          int s1, float tau_max, float* __restrict__ tau,
                                                          uint8_t* __restrict__ alive, int32_t* __restrict__ stop) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R || !alive[r]) return;
    const float dx = rays_d[3 * r + 0], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float norm_d = sqrtf(dx * dx + dy * dy + dz * dz);
    const float* zr = z + r * S;
    const float* rr = raw + 4 * (r * S) + 3;
    float t = tau[r];
    for (int i = s0; i < s1; ++i) {      // s1 < S: zr[i + 1] exists
        const float d = (zr[i + 1] - zr[i]) * norm_d;
        const float sg = rr[4 * i];
        const float s = sg > 0.f ? sg : 0.f;
        t = t + s * d;
    }
    tau[r] = t;
    if (t > tau_max) {
        alive[r] = 0;
        stop[r] = s1;
    }
}

}  // namespace nerf

using namespace nerf;

extern "C" size_t nerf_ert_compact_workspace_bytes(int64_t n_candidates) {
    if (n_candidates < 0) return 0;
    return (size_t)std::max<int64_t>(1, (n_candidates + kErtBlockPts - 1) / kErtBlockPts) * sizeof(int32_t);
}

extern "C" int nerf_ert_compact(const float* d_pts, int64_t n_rays, int64_t samples_per_ray, int64_t s0, int64_t s1,
                                const uint8_t* d_alive, const float* d_sh_rays, const float* d_viewdirs,
                                const float* bbox_min, const float* bbox_max, int res, const uint32_t* d_bits,
                                int stages, int64_t capacity, int32_t* d_rows, int32_t* d_counts, float* d_pts_c,
                                float* d_sh_c, float* d_raw, void* d_workspace, size_t workspace_bytes, void* stream) {
    OccGrid g;
    int rc = fill_grid(g, bbox_min, bbox_max, d_bits ? res : 1);   // no grid: one cell, only the box test is used
    if (rc) return rc;
    NERF_REQUIRE(samples_per_ray >= 1 && samples_per_ray <= INT32_MAX, "ert_compact: samples_per_ray %lld",
                 (long long)samples_per_ray);
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX / samples_per_ray, "ert_compact: n_rays %lld x %lld samples",
                 (long long)n_rays, (long long)samples_per_ray);
    NERF_REQUIRE(s0 >= 0 && s0 <= s1 && s1 <= samples_per_ray, "ert_compact: slab [%lld, %lld) of %lld samples",
                 (long long)s0, (long long)s1, (long long)samples_per_ray);
    const int64_t n_cand = n_rays * (s1 - s0);
    NERF_REQUIRE(stages >= 1 && stages <= 3, "ert_compact: stages %d (1 count, 2 scatter, 3 both)", stages);
    NERF_REQUIRE(d_counts && d_workspace && workspace_bytes >= nerf_ert_compact_workspace_bytes(n_cand),
                 "ert_compact: null counts / workspace, or workspace %zu B < %zu B", workspace_bytes,
                 nerf_ert_compact_workspace_bytes(n_cand));
    NERF_REQUIRE(capacity >= 0 && capacity <= n_cand, "ert_compact: capacity %lld of %lld candidates",
                 (long long)capacity, (long long)n_cand);
    if (n_cand > 0 && (stages & 2)) {
        NERF_REQUIRE(d_raw && ((uintptr_t)d_raw & 15) == 0, "ert_compact: raw rows must be non-null and 16-B aligned");
        NERF_REQUIRE((d_sh_rays != nullptr) != (d_viewdirs != nullptr),
                     "ert_compact: exactly one of the per-ray SH records and the view directions");
        NERF_REQUIRE(!d_sh_rays || ((uintptr_t)d_sh_rays & 15) == 0, "ert_compact: SH records must be 16-B aligned");
        NERF_REQUIRE(capacity == 0 || (d_rows && d_pts_c && d_sh_c && ((uintptr_t)d_sh_c & 15) == 0),
                     "ert_compact: null outputs, or sh_c not 16-B aligned");
    }
    NERF_REQUIRE(n_cand == 0 || d_pts, "ert_compact: null arg");
    if (stages & 1) {
        if (hipMemsetAsync(d_counts, 0, sizeof(int32_t), as_stream(stream)) != hipSuccess) {
            set_error("ert_compact: hipMemsetAsync failed");
            return NERF_E_LAUNCH;
        }
    }
    if (n_cand == 0) return NERF_OK;
    ErtCompactArgs a{};
    a.g = g; a.bits = d_bits; a.pts = d_pts; a.alive = d_alive; a.sh_rays = d_sh_rays; a.viewdirs = d_viewdirs;
    a.N = n_cand; a.S = (int)samples_per_ray; a.s0 = (int)s0; a.width = (int)(s1 - s0);
    ray_div_magic(s1 - s0, a.wd_m, a.wd_s);
    a.capacity = capacity; a.rows = d_rows; a.counts = d_counts; a.pts_c = d_pts_c; a.sh_c = d_sh_c; a.raw = d_raw;
    a.block_counts = static_cast<int32_t*>(d_workspace);
    const unsigned nb = blocks_for(n_cand, kErtBlockPts);
    if (stages & 1) hipLaunchKernelGGL(ert_count_kernel, dim3(nb), dim3(kErtThreads), 0, as_stream(stream), a);
    if (stages & 2) hipLaunchKernelGGL(ert_scatter_kernel, dim3(nb), dim3(kErtThreads), 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH("ert_compact");
    return NERF_OK;
}

extern "C" int nerf_ert_advance(const float* d_raw, const float* d_z, const float* d_rays_d, int64_t n_rays,
                                int64_t samples_per_ray, int64_t s0, int64_t s1, float tau_max, float* d_tau,
                                uint8_t* d_alive, int32_t* d_stop, void* stream) {
    NERF_REQUIRE(samples_per_ray >= 1 && samples_per_ray <= INT32_MAX, "ert_advance: samples_per_ray %lld",
                 (long long)samples_per_ray);
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX / samples_per_ray, "ert_advance: n_rays %lld x %lld samples",
                 (long long)n_rays, (long long)samples_per_ray);
    // s1 < S: the rule is applied after a slab that is not the last, and reads z[s1]
    NERF_REQUIRE(s0 >= 0 && s0 <= s1 && s1 < samples_per_ray,
                 "ert_advance: slab [%lld, %lld) must end before the last of %lld samples", (long long)s0,
                 (long long)s1, (long long)samples_per_ray);
    NERF_REQUIRE(tau_max > 0.f, "ert_advance: tau_max %g must be positive", (double)tau_max);
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_raw && d_z && d_rays_d && d_tau && d_alive && d_stop, "ert_advance: null arg");
    hipLaunchKernelGGL(ert_advance_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, as_stream(stream), d_raw, d_z,
                       d_rays_d, n_rays, (int)samples_per_ray, (int)s0, (int)s1, tau_max, d_tau, d_alive, d_stop);
    NERF_CHECK_LAUNCH("ert_advance");
    return NERF_OK;
}
