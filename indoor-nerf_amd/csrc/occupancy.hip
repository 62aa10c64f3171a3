// Occupancy grid of the scene box: empty-space skipping for forward-only rendering.
//
// Layout. The box [bmin, bmax] is cut into res^3 cells; cell (ix, iy, iz) has the linear id
// (ix * res + iy) * res + iz and owns bit (id & 31) of the 32-bit word id >> 5 of a bitfield of
// ceil(res^3 / 32) words (the bits of the last word past res^3 stay 0).
//
// Cell rule (occ_cell, shared by every kernel here). Per axis, hash_common.h's axis_cell<false> at
// resolution res with cell = (bmax - bmin) / res as fill_cells computes it (two correctly rounded fp32
// operations on the host): base = (int)floorf((clamp(x, bmin, bmax) - bmin) / cell), index =
// min(base, res - 1) (the upper face belongs to the last cell), inside = (x == clamp(x)). A point is
// a candidate only when inside holds on all three axes — the hash encoder's own keep flag, so a point
// the grid skips for lying outside the box is one run_network gives sigma = 0 anyway. The file is built
// with -ffp-contract=off and correctly rounded division: the rule is the same bits as its NumPy fp32
// restatement (tests/test_gpu_occupancy.py).
//
// Why skipping is exact. raw2outputs gives a sample with relu(sigma) = 0 alpha = 0 and weight 0, so its
// colour multiplies a zero weight: writing an all-zero raw row for a point whose dense sigma would have
// been <= 0 changes no composited value. For any other point it equals masking sigma there.
//
// Kernels: cell_points (sample positions of a range of cells), mark (OR any_k(sigma > thresh) into the
// cells' bits), dilate (3x3x3 neighbourhood), query (per point: inside and bit set), compact (the
// render path: the kept points of a field call in ascending order, with their positions and their
// rays' SH4 rows gathered, and zero raw rows for the others; two launches, count / scatter, as
// active.hip).
#include "occ_common.h"   // OccGrid, the cell rule, fill_grid

namespace nerf {

// ---------------------------------------------------------------- builder
// coordinate of sample u in [0, 1) of cell i along one axis, moved inward (towards the cell centre, one
// float at a time) while rounding leaves it in a neighbouring cell or outside the box
__device__ __forceinline__ float occ_coord(float u, int i, float lo, float hi, float cell, int res) {
    const float centre = ((float)i + 0.5f) * cell + lo;
    float x = ((float)i + u) * cell + lo;
    for (int it = 0; it < 8; ++it) {
        bool inside = true;
        if (occ_axis(x, lo, hi, cell, res, inside) == i && inside) return x;
        x = nextafterf(x, centre);
    }
    return centre;
}

__global__ void __launch_bounds__(256) occ_cell_points_kernel(OccGrid g, int64_t cell_begin, int64_t n, int npc,
                                                              uint64_t seed, uint64_t offset,
                                                              float* __restrict__ pts) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t lc = t / npc;
    const int k = (int)(t - lc * npc);
    const int64_t id = cell_begin + lc;
    const int iz = (int)(id % g.res), iy = (int)((id / g.res) % g.res), ix = (int)(id / ((int64_t)g.res * g.res));
    float u[3] = {0.5f, 0.5f, 0.5f};   // sample 0: the centre
    if (k > 0) {
        const U4 r = philox_uniform4(seed, offset, (uint64_t)(id * npc + k));
        u[0] = fminf(r.x, 0x1.fffffep-1f); u[1] = fminf(r.y, 0x1.fffffep-1f); u[2] = fminf(r.z, 0x1.fffffep-1f);
    }
    pts[3 * t] = occ_coord(u[0], ix, g.bmin[0], g.bmax[0], g.cell[0], g.res);
    pts[3 * t + 1] = occ_coord(u[1], iy, g.bmin[1], g.bmax[1], g.cell[1], g.res);
    pts[3 * t + 2] = occ_coord(u[2], iz, g.bmin[2], g.bmax[2], g.cell[2], g.res);
}

// one wave = 64 consecutive cells = two words (cell_begin is 64-aligned): no two waves share a word
__global__ void __launch_bounds__(256) occ_mark_kernel(const float* __restrict__ raw, int64_t cell_begin,
                                                       int64_t n_cells, int npc, float thresh, int64_t grid_cells,
                                                       uint32_t* __restrict__ bits) {
    const int64_t lc = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (lc < n_cells && cell_begin + lc < grid_cells)
        for (int k = 0; k < npc; ++k) on = on || raw[4 * (lc * npc + k) + 3] > thresh;
    const uint64_t m = __ballot(on);
    if ((threadIdx.x & 63) == 0) {
        const int64_t w = (cell_begin + (lc & ~(int64_t)63)) >> 5;
        const int64_t n_words = (grid_cells + 31) >> 5;
        const uint32_t m0 = (uint32_t)m, m1 = (uint32_t)(m >> 32);
        if (m0 && w < n_words) bits[w] = bits[w] | m0;
        if (m1 && w + 1 < n_words) bits[w + 1] = bits[w + 1] | m1;
    }
}

__global__ void __launch_bounds__(256) occ_dilate_kernel(const uint32_t* __restrict__ in, int res, int64_t grid_cells,
                                                         uint32_t* __restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (id < grid_cells) {
        const int iz = (int)(id % res), iy = (int)((id / res) % res), ix = (int)(id / ((int64_t)res * res));
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    const int x = ix + dx, y = iy + dy, z = iz + dz;
                    if (x >= 0 && x < res && y >= 0 && y < res && z >= 0 && z < res)
                        on = on || occ_bit(in, (x * res + y) * res + z);
                }
    }
    const uint64_t m = __ballot(on);
    if ((threadIdx.x & 63) == 0) {
        const int64_t w = (id & ~(int64_t)63) >> 5;
        const int64_t n_words = (grid_cells + 31) >> 5;
        if (w < n_words) out[w] = (uint32_t)m;
        if (w + 1 < n_words) out[w + 1] = (uint32_t)(m >> 32);
    }
}

__global__ void __launch_bounds__(256) occ_query_kernel(OccGrid g, const uint32_t* __restrict__ bits,
                                                        const float* __restrict__ pts, int64_t P,
                                                        uint8_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < P) out[p] = occ_occupied(g, bits, pts + 3 * p) ? 1 : 0;
}

// ---------------------------------------------------------------- compaction (the render path)
constexpr int kOccThreads = 256;
constexpr int kOccPer = 16;                         // points per thread
constexpr int kOccBlockPts = kOccThreads * kOccPer;  // 4096 points per block

struct CompactArgs {
    OccGrid g;
    const uint32_t* bits;
    const float* pts;        // [P, 3]
    const float* sh_rays;    // [R, 40] per-ray SH records (nerf_sample_stratified_sh), or
    const float* viewdirs;   // [R, 3]
    int64_t P;
    uint32_t rd_m; int rd_s; // p / samples_per_ray (udiv_magic)
    int64_t capacity;        // rows of the compacted outputs
    int32_t* rows;           // out [capacity]: kept points, ascending
    int32_t* counts;         // out [1]
    float* pts_c;            // out [capacity, 3]
    float* sh_c;             // out [capacity, 16]
    float* raw;              // [P, 4]: rows of skipped points are zeroed
    int32_t* block_counts;   // workspace [n_blocks]
};

// point k of thread t of block b: b * kOccBlockPts + k * kOccThreads + t (consecutive threads, consecutive points)
__global__ void __launch_bounds__(kOccThreads) occ_count_kernel(CompactArgs a) {
    const int64_t base = (int64_t)blockIdx.x * kOccBlockPts;
    int n = 0;
#pragma unroll 4
    for (int k = 0; k < kOccPer; ++k) {
        const int64_t p = base + k * kOccThreads + threadIdx.x;
        if (p < a.P && occ_occupied(a.g, a.bits, a.pts + 3 * p)) ++n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __shared__ int s[kOccThreads / 64];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int i = 0; i < kOccThreads / 64; ++i) t += s[i];
        a.block_counts[blockIdx.x] = t;
        if (t) atomicAdd(a.counts, t);   // integer: the total does not depend on the order
    }
}

__global__ void __launch_bounds__(kOccThreads) occ_scatter_kernel(CompactArgs a) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // this block's offset: the counts of the blocks before it
    int off = 0;
    for (int i = threadIdx.x; i < b; i += kOccThreads) off += a.block_counts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
    __shared__ int s_off[kOccThreads / 64];
    __shared__ int s_cnt[kOccThreads / 64];
    if (lane == 0) s_off[w] = off;
    __syncthreads();
    int64_t base = 0;
    for (int i = 0; i < kOccThreads / 64; ++i) base += s_off[i];
    __syncthreads();
    const int64_t pbase = (int64_t)b * kOccBlockPts;
    for (int k = 0; k < kOccPer; ++k) {
        const int64_t p = pbase + k * kOccThreads + threadIdx.x;
        float x = 0.f, y = 0.f, z = 0.f;
        bool on = false;
        if (p < a.P) {
            x = a.pts[3 * p]; y = a.pts[3 * p + 1]; z = a.pts[3 * p + 2];
            int id;
            on = occ_cell(a.g, x, y, z, id) && occ_bit(a.bits, id);
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
            const uint32_t ray = udiv_magic((uint32_t)p, a.rd_m, a.rd_s);
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
        for (int i = 0; i < kOccThreads / 64; ++i) base += s_cnt[i];
        __syncthreads();
    }
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_occ_cell_points(const float* bbox_min, const float* bbox_max, int res, int64_t cell_begin,
                                    int64_t n_cells, int n_per_cell, unsigned long long seed,
                                    unsigned long long offset, float* d_pts, void* stream) {
    OccGrid g;
    int rc = fill_grid(g, bbox_min, bbox_max, res);
    if (rc) return rc;
    NERF_REQUIRE(cell_begin >= 0 && n_cells >= 0 && cell_begin + n_cells <= g.n_cells,
                 "occ_cell_points: cells [%lld, +%lld) of %lld", (long long)cell_begin, (long long)n_cells,
                 (long long)g.n_cells);
    NERF_REQUIRE(n_per_cell >= 1 && n_per_cell <= 64, "occ_cell_points: n_per_cell %d (1..64)", n_per_cell);
    if (n_cells == 0) return NERF_OK;
    NERF_REQUIRE(d_pts, "occ_cell_points: null output");
    const int64_t n = n_cells * n_per_cell;
    hipLaunchKernelGGL(occ_cell_points_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), g, cell_begin,
                       n, n_per_cell, (uint64_t)seed, (uint64_t)offset, d_pts);
    NERF_CHECK_LAUNCH("occ_cell_points");
    return NERF_OK;
}

extern "C" int nerf_occ_mark(const float* d_raw, int res, int64_t cell_begin, int64_t n_cells, int n_per_cell,
                             float sigma_thresh, uint32_t* d_bits, void* stream) {
    NERF_REQUIRE(res >= 1 && res <= 1024, "occ_mark: res %d (1..1024)", res);
    const int64_t grid_cells = (int64_t)res * res * res;
    NERF_REQUIRE(cell_begin >= 0 && n_cells >= 0 && cell_begin + n_cells <= grid_cells,
                 "occ_mark: cells [%lld, +%lld) of %lld", (long long)cell_begin, (long long)n_cells,
                 (long long)grid_cells);
    NERF_REQUIRE(cell_begin % 64 == 0, "occ_mark: cell_begin %lld must be a multiple of 64 (a wave owns two words)",
                 (long long)cell_begin);
    NERF_REQUIRE(n_per_cell >= 1 && n_per_cell <= 64, "occ_mark: n_per_cell %d (1..64)", n_per_cell);
    if (n_cells == 0) return NERF_OK;
    NERF_REQUIRE(d_raw && d_bits, "occ_mark: null arg");
    hipLaunchKernelGGL(occ_mark_kernel, dim3(blocks_for(n_cells, 256)), dim3(256), 0, as_stream(stream), d_raw,
                       cell_begin, n_cells, n_per_cell, sigma_thresh, grid_cells, d_bits);
    NERF_CHECK_LAUNCH("occ_mark");
    return NERF_OK;
}

extern "C" int nerf_occ_dilate(const uint32_t* d_bits_in, int res, uint32_t* d_bits_out, void* stream) {
    NERF_REQUIRE(res >= 1 && res <= 1024, "occ_dilate: res %d (1..1024)", res);
    NERF_REQUIRE(d_bits_in && d_bits_out && d_bits_in != d_bits_out, "occ_dilate: null or aliased bitfields");
    const int64_t grid_cells = (int64_t)res * res * res;
    hipLaunchKernelGGL(occ_dilate_kernel, dim3(blocks_for(grid_cells, 256)), dim3(256), 0, as_stream(stream), d_bits_in,
                       res, grid_cells, d_bits_out);
    NERF_CHECK_LAUNCH("occ_dilate");
    return NERF_OK;
}

extern "C" int nerf_occ_query(const float* d_pts, int64_t n_points, const float* bbox_min, const float* bbox_max,
                              int res, const uint32_t* d_bits, uint8_t* d_out, void* stream) {
    OccGrid g;
    int rc = fill_grid(g, bbox_min, bbox_max, res);
    if (rc) return rc;
    NERF_REQUIRE(n_points >= 0, "occ_query: n_points %lld", (long long)n_points);
    if (n_points == 0) return NERF_OK;
    NERF_REQUIRE(d_pts && d_bits && d_out, "occ_query: null arg");
    hipLaunchKernelGGL(occ_query_kernel, dim3(blocks_for(n_points, 256)), dim3(256), 0, as_stream(stream), g, d_bits,
                       d_pts, n_points, d_out);
    NERF_CHECK_LAUNCH("occ_query");
    return NERF_OK;
}

extern "C" size_t nerf_occ_compact_workspace_bytes(int64_t n_points) {
    if (n_points < 0) return 0;
    return (size_t)std::max<int64_t>(1, (n_points + kOccBlockPts - 1) / kOccBlockPts) * sizeof(int32_t);
}

extern "C" int nerf_occ_compact(const float* d_pts, int64_t n_points, const float* d_sh_rays, const float* d_viewdirs,
                                int64_t samples_per_ray, const float* bbox_min, const float* bbox_max, int res,
                                const uint32_t* d_bits, int stages, int64_t capacity, int32_t* d_rows,
                                int32_t* d_counts, float* d_pts_c, float* d_sh_c, float* d_raw, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    OccGrid g;
    int rc = fill_grid(g, bbox_min, bbox_max, res);
    if (rc) return rc;
    NERF_REQUIRE(n_points >= 0 && n_points <= INT32_MAX, "occ_compact: n_points %lld", (long long)n_points);
    NERF_REQUIRE(stages >= 1 && stages <= 3, "occ_compact: stages %d (1 count, 2 scatter, 3 both)", stages);
    NERF_REQUIRE(d_counts && d_workspace && workspace_bytes >= nerf_occ_compact_workspace_bytes(n_points),
                 "occ_compact: null counts / workspace, or workspace %zu B < %zu B", workspace_bytes,
                 nerf_occ_compact_workspace_bytes(n_points));
    NERF_REQUIRE(samples_per_ray >= 1, "occ_compact: samples_per_ray %lld", (long long)samples_per_ray);
    NERF_REQUIRE(capacity >= 0 && capacity <= n_points, "occ_compact: capacity %lld of %lld points",
                 (long long)capacity, (long long)n_points);
    if (n_points > 0 && (stages & 2)) {
        NERF_REQUIRE(d_raw && ((uintptr_t)d_raw & 15) == 0, "occ_compact: raw rows must be non-null and 16-B aligned");
        NERF_REQUIRE((d_sh_rays != nullptr) != (d_viewdirs != nullptr),
                     "occ_compact: exactly one of the per-ray SH records and the view directions");
        NERF_REQUIRE(!d_sh_rays || ((uintptr_t)d_sh_rays & 15) == 0, "occ_compact: SH records must be 16-B aligned");
        NERF_REQUIRE(capacity == 0 || (d_rows && d_pts_c && d_sh_c && ((uintptr_t)d_sh_c & 15) == 0),
                     "occ_compact: null outputs, or sh_c not 16-B aligned");
    }
    NERF_REQUIRE(n_points == 0 || (d_pts && d_bits), "occ_compact: null arg");
    if (stages & 1) {
        if (hipMemsetAsync(d_counts, 0, sizeof(int32_t), as_stream(stream)) != hipSuccess) {
            set_error("occ_compact: hipMemsetAsync failed");
            return NERF_E_LAUNCH;
        }
    }
    if (n_points == 0) return NERF_OK;
    CompactArgs a{};
    a.g = g; a.bits = d_bits; a.pts = d_pts; a.sh_rays = d_sh_rays; a.viewdirs = d_viewdirs; a.P = n_points;
    ray_div_magic(samples_per_ray, a.rd_m, a.rd_s);
    a.capacity = capacity; a.rows = d_rows; a.counts = d_counts; a.pts_c = d_pts_c; a.sh_c = d_sh_c; a.raw = d_raw;
    a.block_counts = static_cast<int32_t*>(d_workspace);
    const unsigned nb = blocks_for(n_points, kOccBlockPts);
    if (stages & 1) hipLaunchKernelGGL(occ_count_kernel, dim3(nb), dim3(kOccThreads), 0, as_stream(stream), a);
    if (stages & 2) hipLaunchKernelGGL(occ_scatter_kernel, dim3(nb), dim3(kOccThreads), 0, as_stream(stream), a);
    NERF_CHECK_LAUNCH("occ_compact");
    return NERF_OK;
}
