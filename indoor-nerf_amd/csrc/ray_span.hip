// Per-ray sample bounds from the occupancy grid, for forward-only rendering.
//
// For a packed ray row [o, d, near, far(, viewdir)] the span kernel walks the grid's cells along the ray
// (a 3-D DDA after Amanatides & Woo) and reports whether the ray crosses an occupied cell inside
// [near, far] and, if so, the span [near', far'] between the first and the last such cell, widened by
// pad. The hit rows are then compacted (compact_common.h's scheme, with the count side done per wave by the
// span kernel itself) with columns 6 and 7 replaced by the span: render_rays runs on them unchanged.
//
// The rule (one thread per ray, fp32, every operation written out below; the file is built with
// -ffp-contract=off and correctly rounded division, so it is the same bits as its NumPy fp32 restatement in
// tests/test_gpu_ray_bounds.py):
//   edge_a(k) = (float)k * cell_a + lo_a for k < res, hi_a for k = res (occ_common.h's cells);
//   slab test: t0 = near, t1 = far; per axis with d_a != 0: ta = (lo_a - o_a) / d_a, tb = (hi_a - o_a) / d_a,
//     swapped for d_a < 0, t0 = max(t0, ta), t1 = min(t1, tb); an axis with d_a == 0 takes its constant cell
//     from occ_axis(o_a) and the ray misses when o_a is outside the box on it; the ray misses unless t0 < t1;
//   first cell: occ_axis of clamp(o_a + d_a * t0) per axis;
//   walk: the current cell ends at te = min(t1, tmax_a), tmax_a = (edge_a(next face) - o_a) / d_a (the
//     first axis wins a tie); a cell counts when te > t (it has positive length) and its bit is set: the
//     first such cell gives tn = t, every one gives tf = te; then step the axis that ended the cell, and
//     stop at t1 or at the box's face. At most 3 res + 1 cells.
//   near-ties: fp32 sample positions do not cross two faces in the order the walk does when the two depths
//     differ by less than their rounding, eps_a = (|o_a| + max(|lo_a|, |hi_a|)) * 2^-20 / |d_a| per axis. So
//     when the cell ends on axis ax and tmax_b - te <= eps_ax + eps_b for another axis b, every cell reached
//     by stepping a non-empty proper subset of {ax} and the tied axes counts too, at the depth max(te, t).
//   pad = 2^-4 * min over axes with d_a != 0 of cell_a / |d_a| (0 for d = 0);
//   near' = max(near, tn - pad), far' = min(far, tf + pad); a ray with far' <= near' is a miss.
// A missed ray reports the span [near, far]; a NaN in o, d, near or far is a miss.
// The span is conservative against fp32 sample positions o + d z up to a stated limit, not unconditionally:
// pad is a depth, and the position rounding it has to cover, divided by |d_a|, grows without bound as a
// face is met at a shallower slope (DESIGN.md §15 has the slope down to which it holds). Past that limit a
// sample within 2^-20 (|o_a| + |bound_a|) of an occupied cell's face may fall outside the span.
#include "compact_common.h"
#include "occ_common.h"

namespace nerf {

constexpr int kSpanThreads = kCompactThreads;   // a span block is one iteration of a compaction block

struct SpanArgs {
    OccGrid g;
    const uint32_t* bits;
    const float* rays;       // [R, C]
    int64_t R;
    int C;
    uint8_t* hit;            // [R]
    float* span;             // [R, 2]
    int64_t capacity;        // rows of the gathered outputs
    int32_t* rows;           // out [capacity]: hit rays, ascending
    float* rays_c;           // out [capacity, C]
    int32_t* counts;         // out [1]
    int32_t* block_counts;   // workspace [n_blocks]
};

// face k of an axis with cells of size cell over [lo, hi]
__device__ __forceinline__ float span_edge(int k, int res, float cell, float lo, float hi) {
    return k >= res ? hi : (float)k * cell + lo;
}

// the rule above; returns hit and writes the span
__device__ __forceinline__ bool ray_span(const OccGrid& g, const uint32_t* __restrict__ bits,
                                         const float* __restrict__ ray, float& sn, float& sf) {
    const float o[3] = {ray[0], ray[1], ray[2]}, d[3] = {ray[3], ray[4], ray[5]};
    const float near = ray[6], far = ray[7];
    sn = near; sf = far;
    float t0 = near, t1 = far, pad = INFINITY, eps[3] = {0.f, 0.f, 0.f};
    int idx[3] = {0, 0, 0}, step[3] = {0, 0, 0};
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.f) {
            idx[a] = occ_axis(o[a], g.bmin[a], g.bmax[a], g.cell[a], g.res, inside);
        } else if (d[a] > 0.f || d[a] < 0.f) {
            if (!(o[a] == o[a])) inside = false;   // NaN origin
            float ta = (g.bmin[a] - o[a]) / d[a], tb = (g.bmax[a] - o[a]) / d[a];
            if (d[a] < 0.f) { const float s = ta; ta = tb; tb = s; }
            if (ta > t0) t0 = ta;
            if (tb < t1) t1 = tb;
            step[a] = d[a] > 0.f ? 1 : -1;
            const float p = g.cell[a] / fabsf(d[a]);
            if (p < pad) pad = p;
            eps[a] = (fabsf(o[a]) + fmaxf(fabsf(g.bmin[a]), fabsf(g.bmax[a]))) * 0x1p-20f / fabsf(d[a]);
        } else {
            inside = false;   // NaN direction
        }
    }
    if (!inside || !(t0 < t1)) return false;
    pad = pad == INFINITY ? 0.f : 0.0625f * pad;
    float tmax[3] = {INFINITY, INFINITY, INFINITY};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (step[a] == 0) continue;
        const float p = fminf(fmaxf(o[a] + d[a] * t0, g.bmin[a]), g.bmax[a]);
        bool in = true;
        idx[a] = occ_axis(p, g.bmin[a], g.bmax[a], g.cell[a], g.res, in);
        tmax[a] = (span_edge(step[a] > 0 ? idx[a] + 1 : idx[a], g.res, g.cell[a], g.bmin[a], g.bmax[a]) - o[a]) / d[a];
    }
    float t = t0, tn = 0.f, tf = 0.f;
    bool hit = false;
    for (int it = 0; it <= 3 * g.res; ++it) {
        float te = t1;
        int ax = -1;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (tmax[a] < te) { te = tmax[a]; ax = a; }
        if (te > t && occ_bit(bits, (idx[0] * g.res + idx[1]) * g.res + idx[2])) {
            if (!hit) { tn = t; hit = true; }
            tf = te;
        }
        if (ax < 0) break;
        // near-ties: the cells a sample may land in around this corner
        const float ea = ax == 0 ? eps[0] : ax == 1 ? eps[1] : eps[2];
        int tied = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (a != ax && tmax[a] - te <= ea + eps[a]) tied |= 1 << a;
        if (tied) {
            const int all = tied | (1 << ax);
            const float tc = te > t ? te : t;
#pragma unroll
            for (int m = 1; m < 7; ++m) {
                if ((m & ~all) || m == all) continue;
                const int k0 = idx[0] + ((m & 1) ? step[0] : 0), k1 = idx[1] + ((m & 2) ? step[1] : 0),
                          k2 = idx[2] + ((m & 4) ? step[2] : 0);
                if (k0 < 0 || k0 >= g.res || k1 < 0 || k1 >= g.res || k2 < 0 || k2 >= g.res) continue;
                if (occ_bit(bits, (k0 * g.res + k1) * g.res + k2)) {
                    if (!hit) { tn = tc; hit = true; }
                    tf = tc;
                }
            }
        }
        // step axis ax (select chains: no dynamically indexed registers or kernel arguments)
#define SPAN_SEL(v) (ax == 0 ? v[0] : ax == 1 ? v[1] : v[2])
        const int st = SPAN_SEL(step), k = SPAN_SEL(idx) + st;
        if (k < 0 || k >= g.res) break;
        const float tm = (span_edge(st > 0 ? k + 1 : k, g.res, SPAN_SEL(g.cell), SPAN_SEL(g.bmin), SPAN_SEL(g.bmax)) -
                          SPAN_SEL(o)) / SPAN_SEL(d);
#undef SPAN_SEL
        if (ax == 0) { idx[0] = k; tmax[0] = tm; } else if (ax == 1) { idx[1] = k; tmax[1] = tm; } else { idx[2] = k; tmax[2] = tm; }
        if (te > t) t = te;
    }
    if (!hit) return false;
    const float lo = tn - pad, hi = tf + pad;
    const float n2 = lo > near ? lo : near, f2 = hi < far ? hi : far;
    if (!(f2 > n2)) return false;
    sn = n2; sf = f2;
    return true;
}

// one thread per ray (neighbouring threads are neighbouring pixels: a wave's walks are coherent); a wave adds
// its hits to the count of its compaction block of kCompactBlock rays and to the total (integer adds: the
// sums do not depend on the order)
__global__ void __launch_bounds__(kSpanThreads) ray_span_kernel(SpanArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kSpanThreads + threadIdx.x;
    bool h = false;
    if (r < a.R) {
        float sn, sf;
        h = ray_span(a.g, a.bits, a.rays + r * a.C, sn, sf);
        a.hit[r] = h ? 1 : 0;
        a.span[2 * r] = sn; a.span[2 * r + 1] = sf;
    }
    const int n = __popcll(__ballot(h));
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(a.block_counts + blockIdx.x / kCompactPer, n);
        atomicAdd(a.counts, n);
    }
}

__global__ void __launch_bounds__(kCompactThreads) ray_span_gather_kernel(SpanArgs a) {
    int64_t base = compact_block_offset(a.block_counts);
    for (int k = 0; k < kCompactPer; ++k) {
        const int64_t r = compact_item(k);
        const bool on = r < a.R && a.hit[r] != 0;
        compact_place(on, base, [&](int64_t idx) {
            if (idx >= a.capacity) return;
            a.rows[idx] = (int32_t)r;
            const float* src = a.rays + r * a.C;
            float* dst = a.rays_c + idx * a.C;
            for (int c = 0; c < a.C; ++c) dst[c] = src[c];
            dst[6] = a.span[2 * r]; dst[7] = a.span[2 * r + 1];
        });
    }
}

// the checks the two entries share
static int span_args(SpanArgs& a, const char* what, int64_t n_rays, int n_cols, const float* bmin, const float* bmax,
                     int res, void* d_workspace, size_t workspace_bytes, size_t need) {
    int rc = fill_grid(a.g, bmin, bmax, res);
    if (rc) return rc;
    // the pad's derivation needs more than fill_grid's 128 floats per cell: >= 2^13
    for (int ax = 0; ax < 3; ++ax) {
        const float big = std::max(std::fabs(bmin[ax]), std::fabs(bmax[ax]));
        NERF_REQUIRE(a.g.cell[ax] >= big * 0x1p-10f, "%s: cells below 2^-10 of the box bounds on axis %d", what, ax);
    }
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX, "%s: n_rays %lld", what, (long long)n_rays);
    NERF_REQUIRE(n_cols == 8 || n_cols == 11, "%s: ray rows of %d columns (8 or 11)", what, n_cols);
    NERF_REQUIRE(n_rays == 0 || (d_workspace && workspace_bytes >= need),
                 "%s: null workspace, or workspace %zu B < %zu B", what, workspace_bytes, need);
    a.R = n_rays; a.C = n_cols;
    a.block_counts = static_cast<int32_t*>(d_workspace);
    return NERF_OK;
}

}  // namespace nerf

using namespace nerf;

extern "C" size_t nerf_ray_span_workspace_bytes(int64_t n_rays) { return compact_workspace_bytes(n_rays); }

extern "C" int nerf_ray_span(const float* d_rays, int64_t n_rays, int n_cols, const float* bbox_min,
                             const float* bbox_max, int res, const uint32_t* d_bits, uint8_t* d_hit, float* d_span,
                             int32_t* d_counts, void* d_workspace, size_t workspace_bytes, void* stream) {
    SpanArgs a{};
    int rc = span_args(a, "ray_span", n_rays, n_cols, bbox_min, bbox_max, res, d_workspace, workspace_bytes,
                       nerf_ray_span_workspace_bytes(n_rays));
    if (rc) return rc;
    if (n_rays == 0) return NERF_OK;
    NERF_REQUIRE(d_rays && d_bits && d_hit && d_span && d_counts, "ray_span: null arg");
    if (hipMemsetAsync(d_counts, 0, sizeof(int32_t), as_stream(stream)) != hipSuccess ||
        hipMemsetAsync(d_workspace, 0, nerf_ray_span_workspace_bytes(n_rays), as_stream(stream)) != hipSuccess) {
        set_error("ray_span: hipMemsetAsync failed");
        return NERF_E_LAUNCH;
    }
    a.bits = d_bits; a.rays = d_rays; a.hit = d_hit; a.span = d_span; a.counts = d_counts;
    hipLaunchKernelGGL(ray_span_kernel, dim3(blocks_for(n_rays, kSpanThreads)), dim3(kSpanThreads), 0,
                       as_stream(stream), a);
    NERF_CHECK_LAUNCH("ray_span");
    return NERF_OK;
}

extern "C" int nerf_ray_span_gather(const float* d_rays, int64_t n_rays, int n_cols, const uint8_t* d_hit,
                                    const float* d_span, int64_t capacity, int32_t* d_rows, float* d_rays_c,
                                    const void* d_workspace, size_t workspace_bytes, void* stream) {
    NERF_REQUIRE(n_rays >= 0 && n_rays <= INT32_MAX, "ray_span_gather: n_rays %lld", (long long)n_rays);
    NERF_REQUIRE(n_cols == 8 || n_cols == 11, "ray_span_gather: ray rows of %d columns (8 or 11)", n_cols);
    NERF_REQUIRE(capacity >= 0 && capacity <= n_rays, "ray_span_gather: capacity %lld of %lld rays",
                 (long long)capacity, (long long)n_rays);
    if (n_rays == 0 || capacity == 0) return NERF_OK;
    NERF_REQUIRE(d_workspace && workspace_bytes >= nerf_ray_span_workspace_bytes(n_rays),
                 "ray_span_gather: null workspace, or workspace %zu B < %zu B", workspace_bytes,
                 nerf_ray_span_workspace_bytes(n_rays));
    NERF_REQUIRE(d_rays && d_hit && d_span && d_rows && d_rays_c, "ray_span_gather: null arg");
    SpanArgs a{};
    a.rays = d_rays; a.R = n_rays; a.C = n_cols; a.hit = const_cast<uint8_t*>(d_hit);
    a.span = const_cast<float*>(d_span); a.capacity = capacity; a.rows = d_rows; a.rays_c = d_rays_c;
    a.block_counts = static_cast<int32_t*>(const_cast<void*>(d_workspace));
    hipLaunchKernelGGL(ray_span_gather_kernel, dim3(blocks_for(n_rays, kCompactBlock)), dim3(kCompactThreads), 0,
                       as_stream(stream), a);
    NERF_CHECK_LAUNCH("ray_span_gather");
    return NERF_OK;
}
