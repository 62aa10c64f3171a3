// The point compaction of the forward-only render paths: which samples of a field call
// the field has to run on.
//
// A field call over pts [R, S, 3] is compacted one slab [s0, s0 + width) of samples at a time. The slab's
// R * width candidates are enumerated ray-major (candidate c = ray c / width, sample s0 + c % width), so
// the kept list is ascending in the point index p = ray * S + sample. A candidate is kept when its ray is
// alive (no alive flags: every ray is), it lies inside the box and, with a grid, its cell is occupied
// (occ_common.h's cell rule). The kept points' indices, positions and their rays' SH4 rows (copied from the
// per-ray SH records, or evaluated from the view directions) are written in ascending order
// (compact_common.h's scheme, two launches: count / scatter); every other candidate — every sample of a dead
// ray included — gets an all-zero raw row, which compositing gives weight 0 exactly (occupancy.hip, "why
// skipping is exact").
//
// nerf_ert_compact is this for one slab of early ray termination (early_stop.hip has the rule that kills
// rays). nerf_occ_compact is the one-slab case of the occupancy path: s0 = 0, width = S = samples_per_ray, no
// alive flags and a grid, so candidate c is point c and n_points need not be a multiple of samples_per_ray.
#include "compact_common.h"
#include "occ_common.h"

namespace nerf {

struct PointCompactArgs {
    OccGrid g;
    const uint32_t* bits;    // NULL: no grid (kept = alive and inside the box)
    const float* pts;        // [R, S, 3]
    const uint8_t* alive;    // [R], or NULL: every ray is alive
    const float* sh_rays;    // [R, 40] per-ray SH records (nerf_sample_stratified_sh), or
    const float* viewdirs;   // [R, 3]
    int64_t N;               // candidates
    int S, s0, width;        // samples per ray, first sample of the slab, samples of the slab
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
__device__ __forceinline__ int64_t cand_point(const PointCompactArgs& a, int64_t c, uint32_t& ray) {
    ray = udiv_magic((uint32_t)c, a.wd_m, a.wd_s);
    const int s = a.s0 + (int)((uint32_t)c - ray * (uint32_t)a.width);
    return (int64_t)ray * a.S + s;
}

__device__ __forceinline__ bool cand_kept(const PointCompactArgs& a, uint32_t ray, float x, float y, float z) {
    if (a.alive && !a.alive[ray]) return false;
    int id;
    const bool inside = occ_cell(a.g, x, y, z, id);
    return inside && (!a.bits || occ_bit(a.bits, id));
}

__global__ void __launch_bounds__(kCompactThreads) point_count_kernel(PointCompactArgs a) {
    int n = 0;
#pragma unroll 4
    for (int k = 0; k < kCompactPer; ++k) {
        const int64_t c = compact_item(k);
        if (c < a.N) {
            uint32_t ray;
            const int64_t p = cand_point(a, c, ray);
            if (cand_kept(a, ray, a.pts[3 * p], a.pts[3 * p + 1], a.pts[3 * p + 2])) ++n;
        }
    }
    compact_count(n, a.block_counts, a.counts);
}

__global__ void __launch_bounds__(kCompactThreads) point_scatter_kernel(PointCompactArgs a) {
    int64_t base = compact_block_offset(a.block_counts);
    for (int k = 0; k < kCompactPer; ++k) {
        const int64_t c = compact_item(k);
        float x = 0.f, y = 0.f, z = 0.f;
        bool on = false;
        uint32_t ray = 0;
        int64_t p = 0;
        if (c < a.N) {
            p = cand_point(a, c, ray);
            x = a.pts[3 * p]; y = a.pts[3 * p + 1]; z = a.pts[3 * p + 2];
            on = cand_kept(a, ray, x, y, z);
            if (!on) *reinterpret_cast<float4*>(a.raw + 4 * p) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        compact_place(on, base, [&](int64_t idx) {
            if (idx >= a.capacity) return;
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
        });
    }
}

// What the two entries share: the checks that follow their own of the candidate count (`what` prefixes every
// message, `unit` names the candidates in it), the reset of the count and the launches. a holds the grid and
// N, S, s0, width.
static int point_compact(PointCompactArgs& a, const char* what, const char* unit, const float* d_pts,
                         const uint8_t* d_alive, const float* d_sh_rays, const float* d_viewdirs,
                         const uint32_t* d_bits, int stages, int64_t capacity, int32_t* d_rows, int32_t* d_counts,
                         float* d_pts_c, float* d_sh_c, float* d_raw, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
    const int64_t n = a.N;
    NERF_REQUIRE(stages >= 1 && stages <= 3, "%s: stages %d (1 count, 2 scatter, 3 both)", what, stages);
    NERF_REQUIRE(d_counts && d_workspace && workspace_bytes >= compact_workspace_bytes(n),
                 "%s: null counts / workspace, or workspace %zu B < %zu B", what, workspace_bytes,
                 compact_workspace_bytes(n));
    NERF_REQUIRE(capacity >= 0 && capacity <= n, "%s: capacity %lld of %lld %s", what, (long long)capacity,
                 (long long)n, unit);
    if (n > 0 && (stages & 2)) {
        NERF_REQUIRE(d_raw && ((uintptr_t)d_raw & 15) == 0, "%s: raw rows must be non-null and 16-B aligned", what);
        NERF_REQUIRE((d_sh_rays != nullptr) != (d_viewdirs != nullptr),
                     "%s: exactly one of the per-ray SH records and the view directions", what);
        NERF_REQUIRE(!d_sh_rays || ((uintptr_t)d_sh_rays & 15) == 0, "%s: SH records must be 16-B aligned", what);
        NERF_REQUIRE(capacity == 0 || (d_rows && d_pts_c && d_sh_c && ((uintptr_t)d_sh_c & 15) == 0),
                     "%s: null outputs, or sh_c not 16-B aligned", what);
    }
    NERF_REQUIRE(n == 0 || d_pts, "%s: null arg", what);
    if (stages & 1) {
        if (hipMemsetAsync(d_counts, 0, sizeof(int32_t), as_stream(stream)) != hipSuccess) {
            set_error("%s: hipMemsetAsync failed", what);
            return NERF_E_LAUNCH;
        }
    }
    if (n == 0) return NERF_OK;
    a.bits = d_bits; a.pts = d_pts; a.alive = d_alive; a.sh_rays = d_sh_rays; a.viewdirs = d_viewdirs;
    ray_div_magic(a.width, a.wd_m, a.wd_s);
    a.capacity = capacity; a.rows = d_rows; a.counts = d_counts; a.pts_c = d_pts_c; a.sh_c = d_sh_c; a.raw = d_raw;
    a.block_counts = static_cast<int32_t*>(d_workspace);
    const unsigned nb = blocks_for(n, kCompactBlock);
    if (stages & 1) hipLaunchKernelGGL(point_count_kernel, dim3(nb), dim3(kCompactThreads), 0, as_stream(stream), a);
    if (stages & 2) hipLaunchKernelGGL(point_scatter_kernel, dim3(nb), dim3(kCompactThreads), 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH(what);
    return NERF_OK;
}

}  // namespace nerf

using namespace nerf;

extern "C" size_t nerf_occ_compact_workspace_bytes(int64_t n_points) { return compact_workspace_bytes(n_points); }

extern "C" size_t nerf_ert_compact_workspace_bytes(int64_t n_candidates) {
    return compact_workspace_bytes(n_candidates);
}

extern "C" int nerf_occ_compact(const float* d_pts, int64_t n_points, const float* d_sh_rays, const float* d_viewdirs,
                                int64_t samples_per_ray, const float* bbox_min, const float* bbox_max, int res,
                                const uint32_t* d_bits, int stages, int64_t capacity, int32_t* d_rows,
                                int32_t* d_counts, float* d_pts_c, float* d_sh_c, float* d_raw, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    PointCompactArgs a{};
    int rc = fill_grid(a.g, bbox_min, bbox_max, res);
    if (rc) return rc;
    NERF_REQUIRE(n_points >= 0 && n_points <= INT32_MAX, "occ_compact: n_points %lld", (long long)n_points);
    NERF_REQUIRE(samples_per_ray >= 1, "occ_compact: samples_per_ray %lld", (long long)samples_per_ray);
    NERF_REQUIRE(n_points == 0 || d_bits, "occ_compact: null arg");
    // one slab of all the samples; rays longer than the call are one ray
    a.N = n_points; a.s0 = 0;
    a.S = a.width = (int)std::min<int64_t>(samples_per_ray, std::max<int64_t>(n_points, 1));
    return point_compact(a, "occ_compact", "points", d_pts, nullptr, d_sh_rays, d_viewdirs, d_bits, stages, capacity,
                         d_rows, d_counts, d_pts_c, d_sh_c, d_raw, d_workspace, workspace_bytes, stream);
}

extern "C" int nerf_ert_compact(const float* d_pts, int64_t n_rays, int64_t samples_per_ray, int64_t s0, int64_t s1,
                                const uint8_t* d_alive, const float* d_sh_rays, const float* d_viewdirs,
                                const float* bbox_min, const float* bbox_max, int res, const uint32_t* d_bits,
                                int stages, int64_t capacity, int32_t* d_rows, int32_t* d_counts, float* d_pts_c,
                                float* d_sh_c, float* d_raw, void* d_workspace, size_t workspace_bytes, void* stream) {
    PointCompactArgs a{};
    int rc = fill_grid(a.g, bbox_min, bbox_max, d_bits ? res : 1);   // no grid: one cell, only the box test is used
    if (rc) return rc;
    NERF_REQUIRE(samples_per_ray >= 1 && samples_per_ray <= INT32_MAX, "ert_compact: samples_per_ray %lld",
                 (long long)samples_per_ray);
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX / samples_per_ray, "ert_compact: n_rays %lld x %lld samples",
                 (long long)n_rays, (long long)samples_per_ray);
    NERF_REQUIRE(s0 >= 0 && s0 <= s1 && s1 <= samples_per_ray, "ert_compact: slab [%lld, %lld) of %lld samples",
                 (long long)s0, (long long)s1, (long long)samples_per_ray);
    a.N = n_rays * (s1 - s0); a.S = (int)samples_per_ray; a.s0 = (int)s0; a.width = (int)(s1 - s0);
    return point_compact(a, "ert_compact", "candidates", d_pts, d_alive, d_sh_rays, d_viewdirs, d_bits, stages,
                         capacity, d_rows, d_counts, d_pts_c, d_sh_c, d_raw, d_workspace, workspace_bytes, stream);
}
