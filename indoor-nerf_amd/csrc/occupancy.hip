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
// cells' bits), dilate (3x3x3 neighbourhood), query (per point: inside and bit set). The render path's
// compaction of a field call's kept points (nerf_occ_compact) is sparse_points.hip.
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
