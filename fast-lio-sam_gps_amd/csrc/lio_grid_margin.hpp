// lio_grid_margin.hpp — the slack of the grid's computed cell faces (GridDev::margin), host only and free of
// HIP so that tests/cpp/grid_margin.cpp can hold it against the float arithmetic it has to cover.
//
// The searches (lio_dev.hpp, lio_icp.hip) skip cells and stop shell walks by the computed faces
//   face(k) = o + (float)k * cell,  lo + cell,  face(k) -/+ margin,
// while a point's cell is floorf((v - o) * (1 / cell)) (cell_coord).  Pruning is exact as long as the margin
// covers the distance between a computed face and the true boundary B_k of that assignment.  With
//   A   = the largest |coordinate| of the grid box (max over the axes of |o| and |o + n * cell|),
//   ext = the largest extent n * cell,  U = one float spacing at A (<= 2^-23 * A),
// the terms are, per axis:
//   face(k):      (float)k * cell rounds by <= 2^-24 * ext, the sum by <= U / 2;
//   B_k:          v - o rounds by <= 2^-24 * ext (exact inside one binade), 1 / cell is off by 2^-24 relative and
//                 the product rounds by 2^-24 relative: together <= 3 * 2^-24 * ext;
//   lo + cell:    one more rounding, U / 2 — so the upper face of a cell, and every stop radius own + s * cell
//                 derived from it, sits up to U + 4 * 2^-24 * ext past the first point it has not scanned;
//   face - m, (face - m) + (cell + 2 m): the margin is itself added in float at magnitude A, U / 2 per sum,
//                 so a box face can lose up to 2 U of it.
// Worst case: 2 U + 4 * 2^-24 * ext <= 2.4e-7 * (A + ext).  The value below keeps today's
// 1e-3 + 1e-4 * cell (which is that bound's match up to A + ext of about 3 km) and grows beyond it as
// 3 * 2^-23 * A + 3e-7 * ext.  The margin only widens what is scanned, never the result.
#pragma once
#include <algorithm>
#include <cmath>

namespace lio {

// Geom: any struct with ox, oy, oz, cell (float) and nx, ny, nz (int) — GridGeom
template <class Geom>
inline float grid_margin(const Geom& g) {
    const float base = 1e-3f + 1e-4f * g.cell;
    const double o[3] = {g.ox, g.oy, g.oz};
    const int n[3] = {g.nx, g.ny, g.nz};
    double amax = 0.0, ext = 0.0;
    for (int d = 0; d < 3; ++d) {
        const double e = (double)n[d] * (double)g.cell;
        amax = std::max(amax, std::max(std::fabs(o[d]), std::fabs(o[d] + e)));
        ext = std::max(ext, e);
    }
    const double grown = 3.0 * std::ldexp(amax, -23) + 3e-7 * ext;
    return std::max(base, (float)grown);
}

}  // namespace lio
