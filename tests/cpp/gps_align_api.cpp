// The GPS alignment mirrors of include/lio_gpu.hpp as a C++ maintainer uses them: GpsAligner, fit_pairs and
// georeference on one FilterGPU — the calls of post_process/align_slam_gps_icp.py:81-156 and
// georeference_pcd.py:236-244.  On the GPU align() is checked bit for bit against the contract written out here
// in plain C++ (this file is built with -ffp-contract=off): a brute-force nearest neighbour with a strict <, sums
// by TREE, the closed-form rotation.  Exit 77: no device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::PointXYZI;

static uint32_t g_state = 24680u;
static double frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (double)(g_state >> 8) * (1.0 / 16777216.0);
}

// TREE (lio_gpu.h): blocks of 256 padded with +0.0, halving inside a block, block sums in ascending order
static double tree(const std::vector<double>& v) {
    double total = 0.0;
    for (size_t b = 0; b < v.size(); b += 256) {
        double a[256];
        for (size_t i = 0; i < 256; ++i) a[i] = b + i < v.size() ? v[b + i] : 0.0;
        for (int w = 128; w >= 1; w /= 2)
            for (int i = 0; i < w; ++i) a[i] = a[i] + a[i + w];
        total = total + a[0];
    }
    return total;
}

struct Ref {
    std::vector<double> S;
    std::vector<int32_t> nn;
    int iterations = 0;
    bool converged = false;
    double mean_error = 0.0;
    lio_gpu::Similarity2D total;
    double cB[2] = {0.0, 0.0};
};

static Ref reference(const std::vector<double>& gps, const std::vector<double>& slam, int max_iterations, double tol) {
    const size_t m = gps.size() / 2, n = slam.size() / 2;
    auto column = [](const std::vector<double>& p, int d) {
        std::vector<double> c(p.size() / 2);
        for (size_t i = 0; i < c.size(); ++i) c[i] = p[2 * i + (size_t)d];
        return c;
    };
    auto norm = [&](const std::vector<double>& p) {
        std::vector<double> q(p.size() / 2);
        for (size_t i = 0; i < q.size(); ++i) q[i] = p[2 * i] * p[2 * i] + p[2 * i + 1] * p[2 * i + 1];
        return std::sqrt(tree(q));
    };
    Ref r;
    const double cA[2] = {tree(column(slam, 0)) / (double)n, tree(column(slam, 1)) / (double)n};
    r.cB[0] = tree(column(gps, 0)) / (double)m, r.cB[1] = tree(column(gps, 1)) / (double)m;
    std::vector<double> S(slam), D(gps);
    for (size_t i = 0; i < n; ++i) S[2 * i] -= cA[0], S[2 * i + 1] -= cA[1];
    for (size_t i = 0; i < m; ++i) D[2 * i] -= r.cB[0], D[2 * i + 1] -= r.cB[1];
    const double sA = norm(S), sB = norm(D);
    const double s0 = sA > 1e-8 ? sB / sA : 1.0;
    for (double& v : S) v = s0 * v;
    double tS = s0, tC = 1.0, tSn = 0.0, tT[2] = {-(s0 * cA[0]), -(s0 * cA[1])};
    double prev = std::numeric_limits<double>::infinity();
    r.nn.assign(n, 0);
    std::vector<double> M(2 * n), dist(n), w(n);
    for (int it = 0; it < max_iterations; ++it) {
        for (size_t j = 0; j < n; ++j) {
            double best = std::numeric_limits<double>::infinity();
            int32_t bk = 0;
            for (size_t k = 0; k < m; ++k) {
                const double dx = S[2 * j] - D[2 * k], dy = S[2 * j + 1] - D[2 * k + 1];
                const double d2 = dx * dx + dy * dy;
                if (d2 < best) best = d2, bk = (int32_t)k;
            }
            r.nn[j] = bk;
            M[2 * j] = D[2 * (size_t)bk], M[2 * j + 1] = D[2 * (size_t)bk + 1];
            dist[j] = std::sqrt(best);
        }
        const double cs[2] = {tree(column(S, 0)) / (double)n, tree(column(S, 1)) / (double)n};
        const double cd[2] = {tree(column(M, 0)) / (double)n, tree(column(M, 1)) / (double)n};
        double h[6];
        for (int q = 0; q < 6; ++q) {
            for (size_t j = 0; j < n; ++j) {
                const double ax = S[2 * j] - cs[0], ay = S[2 * j + 1] - cs[1], bx = M[2 * j] - cd[0], by = M[2 * j + 1] - cd[1];
                const double all[6] = {ax * bx, ax * by, ay * bx, ay * by, ax * ax + ay * ay, bx * bx + by * by};
                w[j] = all[q];
            }
            h[q] = tree(w);
        }
        const double p = h[0] + h[3], q = h[1] - h[2], rr = std::sqrt(p * p + q * q);
        const double c = rr != 0.0 ? p / rr : 1.0, s = rr != 0.0 ? q / rr : 0.0;
        const double sc = std::sqrt(h[5]) / std::sqrt(h[4]);
        const double t[2] = {cd[0] - sc * (c * cs[0] - s * cs[1]), cd[1] - sc * (s * cs[0] + c * cs[1])};
        for (size_t j = 0; j < n; ++j) {
            const double x = S[2 * j], y = S[2 * j + 1];
            S[2 * j] = sc * (c * x - s * y) + t[0], S[2 * j + 1] = sc * (s * x + c * y) + t[1];
        }
        tS = sc * tS;
        const double nC = c * tC - s * tSn, nS = s * tC + c * tSn;
        tC = nC, tSn = nS;
        const double nx = sc * (c * tT[0] - s * tT[1]) + t[0], ny = sc * (s * tT[0] + c * tT[1]) + t[1];
        tT[0] = nx, tT[1] = ny;
        r.mean_error = tree(dist) / (double)n;
        r.iterations = it + 1;
        if (std::fabs(prev - r.mean_error) < tol) {
            r.converged = true;
            break;
        }
        prev = r.mean_error;
    }
    r.S = S;
    r.total = {tS, tC, tSn, {tT[0] + r.cB[0], tT[1] + r.cB[1]}};
    return r;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    try {
        lio_gpu::FilterGPU f;
        // a 600-pose trajectory and a 777-fix GPS track of the same path at national-grid offsets, 0.4 m of noise
        const size_t n = 600, m = 777;
        auto path = [](double u, double out[2]) {
            out[0] = 400.0 * u + 30.0 * std::sin(7.0 * u);
            out[1] = 140.0 * std::sin(3.0 * u) + 20.0 * std::cos(9.0 * u);
        };
        std::vector<double> slam(2 * n), gps(2 * m);
        for (size_t i = 0; i < n; ++i) path((double)i / (double)(n - 1), &slam[2 * i]);
        const double c0 = std::cos(0.6), s0 = std::sin(0.6);
        for (size_t i = 0; i < m; ++i) {
            double p[2];
            path((double)i / (double)(m - 1), p);
            gps[2 * i] = 1.02 * (c0 * p[0] - s0 * p[1]) + 836000.0 + 0.8 * (frand() - 0.5);
            gps[2 * i + 1] = 1.02 * (s0 * p[0] + c0 * p[1]) + 818000.0 + 0.8 * (frand() - 0.5);
        }
        lio_gpu::GpsAligner al(f);
        std::vector<double> aligned;
        al.setMaxIterations(0);
        try {  // no iteration: the library's argument error
            al.align(gps, slam, aligned);
            std::printf("FAIL: max_iterations 0 was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        for (int iters : {1, 50}) {
            al.setMaxIterations(iters);
            al.align(gps, slam, aligned);
            const Ref r = reference(gps, slam, iters, 1e-4);
            bool ok = al.iterations() == r.iterations && al.converged() == r.converged && same_bits(al.meanError(), r.mean_error) &&
                      al.nearest() == r.nn;
            const lio_gpu::Similarity2D T = al.total();
            ok = ok && same_bits(T.scale, r.total.scale) && same_bits(T.c, r.total.c) && same_bits(T.s, r.total.s) &&
                 same_bits(T.t[0], r.total.t[0]) && same_bits(T.t[1], r.total.t[1]);
            for (size_t j = 0; ok && j < n; ++j)
                ok = same_bits(aligned[2 * j], r.S[2 * j] + r.cB[0]) && same_bits(aligned[2 * j + 1], r.S[2 * j + 1] + r.cB[1]);
            if (!ok) {
                std::printf("FAIL: align(max_iterations %d) differs from the contract written out in C++ (%d / %d iterations)\n",
                            iters, al.iterations(), r.iterations);
                return 1;
            }
            double worst = 0.0;  // the total similarity reproduces the aligned points
            for (size_t j = 0; j < n; ++j) {
                double g[2];
                T.apply(&slam[2 * j], g);
                worst = std::fmax(worst, std::fmax(std::fabs(g[0] - aligned[2 * j]), std::fabs(g[1] - aligned[2 * j + 1])));
            }
            std::printf("max_iterations %d: %d iterations, converged %d, mean error %.6f m, total vs aligned %.3g m\n", iters,
                        al.iterations(), (int)al.converged(), al.meanError(), worst);
            if (!(worst < 1e-6)) {
                std::printf("FAIL: total() does not reproduce the aligned points\n");
                return 1;
            }
        }

        // pairs matched one to one: an exact similarity is recovered
        std::vector<double> dst(2 * n);
        const lio_gpu::Similarity2D truth{1.5, std::cos(-1.1), std::sin(-1.1), {12.0, -7.0}};
        for (size_t j = 0; j < n; ++j) truth.apply(&slam[2 * j], &dst[2 * j]);
        const lio_gpu::Similarity2D fit = lio_gpu::fit_pairs(f, slam, dst);
        if (!(std::fabs(fit.scale - truth.scale) < 1e-12 && std::fabs(fit.c - truth.c) < 1e-12 && std::fabs(fit.s - truth.s) < 1e-12 &&
              std::fabs(fit.t[0] - truth.t[0]) < 1e-9 && std::fabs(fit.t[1] - truth.t[1]) < 1e-9)) {
            std::printf("FAIL: fit_pairs does not recover the similarity\n");
            return 1;
        }

        // the map through the total similarity, with and without an origin
        std::vector<PointXYZI> cloud(1000), geo, geo0;
        for (auto& p : cloud) p = {(float)(400.0 * frand()), (float)(300.0 * frand() - 150.0), (float)(5.0 * frand()), (float)(255.0 * frand())};
        const lio_gpu::Similarity2D T = al.total();
        const double origin[2] = {836000.0, 818000.0};
        std::vector<double> xy;
        lio_gpu::georeference(f, cloud, T, geo0);
        lio_gpu::georeference(f, cloud, T, geo, origin, &xy);
        const double R4[4] = {T.c, -T.s, T.s, T.c};
        for (size_t i = 0; i < cloud.size(); ++i) {
            const double x = cloud[i].x, y = cloud[i].y;
            const double gx = (x * R4[0] + y * R4[1]) * T.scale + T.t[0], gy = (x * R4[2] + y * R4[3]) * T.scale + T.t[1];
            const bool ok = geo0[i].x == (float)gx && geo0[i].y == (float)gy && geo[i].x == (float)(gx - origin[0]) &&
                            geo[i].y == (float)(gy - origin[1]) && same_bits(xy[2 * i], gx - origin[0]) &&
                            same_bits(xy[2 * i + 1], gy - origin[1]) && geo[i].z == cloud[i].z &&
                            geo[i].intensity == cloud[i].intensity;
            if (!ok) {
                std::printf("FAIL: georeference differs at point %zu\n", i);
                return 1;
            }
        }
        std::printf("%zu poses aligned to %zu fixes, %zu map points georeferenced\nALL OK\n", n, m, cloud.size());
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
