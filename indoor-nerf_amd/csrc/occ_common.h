// The occupancy grid's cell rule (occupancy.hip has the layout and the rule in words), shared by the
// grid's own kernels, the point compaction (sparse_points.hip) and the ray spans (ray_span.hip).
#pragma once
#include "field_common.h"

namespace nerf {

struct OccGrid {
    float bmin[3], bmax[3], cell[3];
    int res;
    int64_t n_cells;
};

__device__ __forceinline__ int occ_axis(float x, float lo, float hi, float cell, int res, bool& inside) {
    const AxisCell a = axis_cell<false>(x, lo, hi, cell);
    inside = inside && a.inside;
    return a.base < res - 1 ? a.base : res - 1;
}

// the cell rule: linear cell id of a point and whether it lies inside the box
__device__ __forceinline__ bool occ_cell(const OccGrid& g, float x, float y, float z, int& id) {
    bool inside = true;
    const int ix = occ_axis(x, g.bmin[0], g.bmax[0], g.cell[0], g.res, inside);
    const int iy = occ_axis(y, g.bmin[1], g.bmax[1], g.cell[1], g.res, inside);
    const int iz = occ_axis(z, g.bmin[2], g.bmax[2], g.cell[2], g.res, inside);
    id = (ix * g.res + iy) * g.res + iz;
    return inside;
}

__device__ __forceinline__ bool occ_bit(const uint32_t* __restrict__ bits, int id) {
    return (bits[id >> 5] >> (id & 31)) & 1u;
}

__device__ __forceinline__ bool occ_occupied(const OccGrid& g, const uint32_t* __restrict__ bits, const float* p) {
    int id;
    return occ_cell(g, p[0], p[1], p[2], id) && occ_bit(bits, id);
}

static int fill_grid(OccGrid& g, const float* bmin, const float* bmax, int res) {
    NERF_REQUIRE(bmin && bmax, "occupancy: null box");
    NERF_REQUIRE(res >= 1 && res <= 1024, "occupancy: res %d (1..1024)", res);
    float cell[1][3], rcell[1][3];
    const float fres = (float)res;
    const bool ok = fill_cells(cell, rcell, bmin, bmax, &fres, 1);
    for (int a = 0; a < 3; ++a) {
        NERF_REQUIRE(bmax[a] > bmin[a], "occupancy: empty box on axis %d", a);
        g.bmin[a] = bmin[a]; g.bmax[a] = bmax[a]; g.cell[a] = cell[0][a];
    }
    // the bounds fill_cells accepts for the fast division: cells of >= 2^-16 of the largest |bound|, so
    // a cell spans >= 128 floats per axis and cell_points' inward moves stay inside it
    NERF_REQUIRE(ok, "occupancy: box bounds / cells outside [2^-40, 2^40], or cells below 2^-16 of the bounds");
    g.res = res;
    g.n_cells = (int64_t)res * res * res;
    return NERF_OK;
}

}  // namespace nerf
