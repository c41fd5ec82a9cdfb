// lio_radius_dev.hpp — the radius query over the cell grid of dn_build_grid (lio_denoise.hpp), once: the cells a
// point's neighbours can lie in and the walk over their rows.  Device only; included by lio_denoise.hip (Kernel
// B) and, through lio_cluster_dev.hpp, by lio_cluster.hip and lio_dbscan.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_dev.hpp"
#include "lio_denoise.hpp"

namespace lio {

namespace {

// The cells a point's neighbours within r can lie in — cell_coord(p -+ (r + m)) per axis, m = 1e-5 r + 1e-6 |p|,
// clamped to the grid — as the rows of cells a kernel walks:
//
//     const auto b = cell_box<kLowerHalf>(g, x, y, z, r, j);
//     for (int cz = b.z0; cz <= b.z1; ++cz)
//         for (int cy = b.y0; cy <= b.y_last(cz); ++cy) {
//             uint32_t k, e;
//             b.row(g, start, cz, cy, k, e);  // the row's cells x0 .. x1 are the positions [k, e) of the gridded points
//
// NO NEIGHBOUR IS MISSED, whatever the cell size (the cell cap may have grown the edge far above r, and the
// assignment is rounded, so "the 27 cells around mine" is not the argument), with the inclusive test, which
// covers the strict one.  A point s with float sqdist3(p, s) <= r2, r2 = (float)((double)r * r), has float
// dx * dx <= r2 (the other squares are >= 0 and float addition is monotone), so |p.x - s.x| <= r (1 + 3e-7) (the
// roundings of the difference, the square and r2), so the float p.x - (r + m) is <= s.x <= the float
// p.x + (r + m); cell_coord is monotone (non-decreasing: float subtraction of a constant, multiplication by a
// positive constant, floor, clamp), so s's cell coordinate lies inside the range on every axis.
//
// COST.  With the cell edge at 1.001 r, r + m <= the edge while |p| <= 990 r: the range is 3 cells per axis then
// (the points below and above p by at most one edge).
//
// kLowerHalf, for the gridded point at position j: the positions below j only.  They lie in cells of linear index
// <= its own (my, mz: the cell the grid build assigned it, by the same float expression on the same values), so
// the rows up to its own with e clamped to j (5 rows of 3 cells in a volume): the rule by which a kernel tests
// every pair once, by its later point.
template <bool kLowerHalf>
struct CellBox {
    int x0, x1, y0, y1, z0, z1, my, mz;
    uint32_t j;
    __device__ __forceinline__ int y_last(int cz) const {  // rows behind my own hold later positions only
        return kLowerHalf && cz == mz ? min(y1, my) : y1;
    }
    __device__ __forceinline__ void row(const DnGeom& g, const uint32_t* __restrict__ start, int cz, int cy, uint32_t& k,
                                        uint32_t& e) const {
        const uint32_t base = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx;
        e = start[base + (uint32_t)x1 + 1u];
        if (kLowerHalf) e = min(e, j);
        k = start[base + (uint32_t)x0];
    }
};

template <bool kLowerHalf>
__device__ __forceinline__ CellBox<kLowerHalf> cell_box(const DnGeom& g, float x, float y, float z, float r,
                                                        uint32_t j = 0) {
    const auto reach = [r](float v) { return r + (1e-5f * r + 1e-6f * fabsf(v)); };  // r + m
    const float rx = reach(x), ry = reach(y), rz = reach(z);
    CellBox<kLowerHalf> b;
    b.x0 = max(cell_coord(x - rx, g.ox, g.inv), 0), b.x1 = min(cell_coord(x + rx, g.ox, g.inv), g.nx - 1);
    b.y0 = max(cell_coord(y - ry, g.oy, g.inv), 0), b.y1 = min(cell_coord(y + ry, g.oy, g.inv), g.ny - 1);
    b.z0 = max(cell_coord(z - rz, g.oz, g.inv), 0), b.z1 = min(cell_coord(z + rz, g.oz, g.inv), g.nz - 1);
    b.my = min(max(cell_coord(y, g.oy, g.inv), 0), g.ny - 1), b.mz = min(max(cell_coord(z, g.oz, g.inv), 0), g.nz - 1);
    if (kLowerHalf) b.z1 = min(b.z1, b.mz);
    if (b.x0 > b.x1) b.z1 = b.z0 - 1;  // beside the grid: no row at all
    b.j = j;
    return b;
}

}  // namespace

}  // namespace lio
