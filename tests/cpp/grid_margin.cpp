// grid_margin.cpp — csrc/lio_grid_margin.hpp against the float arithmetic it has to cover, host only.
//
// Restates cell_coord (floorf((v - o) * (1 / cell))) and the face formula (o + (float)k * cell) and sweeps cell
// sizes, origins and extents.  At every face k it finds the first float assigned to cell k (and with it the
// last float of cell k - 1) and checks, with m = grid_margin(geom):
//   |first - face(k)| <= m                       the computed face against the assignment
//   (face(k - 1) + cell) - m <= first            the upper face of cell k - 1 as the stop rules use it
//   face(k) - m <= first                         the lower box face of cell k as axis_gap uses it
//   (face(k - 1) - m) + (cell + 2 m) >= last     the upper box face of cell k - 1
// `grid_margin old` runs the same sweep with the former constant 1e-3f + 1e-4f * cell and reports the faces
// that exceed it (exit status 1).  Build: g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fast-lio-sam_gps_amd/csrc/lio_grid_margin.hpp"

struct Geom {
    float ox, oy, oz, cell;
    int nx, ny, nz;
};

static int cell_coord(float v, float o, float inv) {
    float f = std::floor((v - o) * inv);
    f = std::fmin(std::fmax(f, -1.0e9f), 1.0e9f);
    return (int)f;
}

static float face(float o, int k, float cell) { return o + (float)k * cell; }

int main(int argc, char** argv) {
    const bool old = argc > 1 && std::strcmp(argv[1], "old") == 0;
    const float cells[] = {0.3f, 0.6f, 0.7f, 1.0f, 2.3f};
    const float origins[] = {-3.1f, 2e4f, 1e5f, 1e6f};
    const double extents[] = {40.0, 3000.0, 5e4};
    long faces = 0, bad = 0;
    double worst = 0.0;
    for (float cell : cells)
        for (float o : origins)
            for (double ext : extents) {
                Geom g{o, o, o, cell, 0, 0, 0};
                g.nx = g.ny = g.nz = (int)std::floor(ext / cell) + 2;
                const float m = old ? 1e-3f + 1e-4f * cell : lio::grid_margin(g);
                const float inv = 1.0f / cell;
                const float w = cell + 2.f * m;
                long bad_here = 0;
                // every face of a short grid; a long one in strides, with its last 2000 faces
                const int step = g.nx > 20000 ? 7 : 1;
                for (int k = 1; k < g.nx; k += (k < g.nx - 2000 ? step : 1)) {
                    const float f = face(o, k, cell);
                    float v = f;
                    while (cell_coord(v, o, inv) >= k) v = std::nextafter(v, -INFINITY);
                    while (cell_coord(v, o, inv) < k) v = std::nextafter(v, INFINITY);
                    const float first = v, last = std::nextafter(v, -INFINITY);
                    const float below = face(o, k - 1, cell);
                    const double dev = std::fabs((double)first - (double)f);
                    worst = std::fmax(worst, dev / (double)m);
                    const bool ok = dev <= (double)m && (double)(below + cell) - (double)m <= (double)first &&
                                    f - m <= first && (below - m) + w >= last;
                    ++faces;
                    if (!ok) {
                        ++bad;
                        if (++bad_here <= 2)
                            std::printf("cell %g origin %g extent %g face %d: first %.9g face %.9g margin %.6g\n",
                                        (double)cell, (double)o, ext, k, (double)first, (double)f, (double)m);
                    }
                }
            }
    std::printf("%ld faces, %ld beyond the margin, worst |first - face| / margin %.3f\n", faces, bad, worst);
    if (bad) {
        std::printf("MARGIN EXCEEDED\n");
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
