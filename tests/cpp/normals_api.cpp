// The normal estimation mirror of include/lio_gpu.hpp as a C++ maintainer uses it: NormalEstimation<PointT> beside
// the other filters on one FilterGPU (pcl::NormalEstimation's setKSearch / setRadiusSearch / setViewPoint / compute).
// On the GPU compute() is checked exactly against the contract of lio_estimate_normals written here as a plain
// sequential loop: every pair's float distance, the k smallest under (distance, index) and / or the strict radius,
// the integer moments, the Jacobi sweeps in double, the pick and the orientation.  n = 4097.  Exit 77: no device.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::Normal;
using lio_gpu::PointXYZI;

static uint32_t g_state = 13579u;
static float frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

struct Ref {
    std::vector<Normal> normals;
    std::vector<int32_t> counts;
    int64_t stats[6] = {0, 0, 0, 0, 0, 0};
};

static bool finite3(const PointXYZI& p) { return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z); }

// vps: empty (the sign rule), one viewpoint, or one per point
static Ref brute_normals(const std::vector<PointXYZI>& c, float radius, int k, const std::vector<std::array<float, 3>>& vps) {
    const int n = (int)c.size();
    const float r2 = (float)((double)radius * (double)radius);
    Ref out;
    out.normals.assign((size_t)n, Normal{NAN, NAN, NAN, NAN});
    out.counts.assign((size_t)n, 0);
    std::vector<std::pair<float, int>> cand;
    for (int i = 0; i < n; ++i) {
        if (!finite3(c[(size_t)i])) continue;
        out.stats[0] += 1;
        cand.clear();
        for (int j = 0; j < n; ++j) {
            if (!finite3(c[(size_t)j])) continue;
            const float dx = c[(size_t)i].x - c[(size_t)j].x, dy = c[(size_t)i].y - c[(size_t)j].y, dz = c[(size_t)i].z - c[(size_t)j].z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (radius > 0.f && !(d2 < r2)) continue;
            cand.emplace_back(d2, j);
        }
        std::sort(cand.begin(), cand.end());  // (d2, then index)
        if (k > 0 && (int)cand.size() > k) cand.resize((size_t)k);
        const int64_t m = (int64_t)cand.size();
        out.counts[(size_t)i] = (int32_t)m;
        out.stats[4] = std::max(out.stats[4], m), out.stats[5] += m;
        if (m < 3) {
            out.stats[2] += 1;
            continue;
        }
        const float B = radius > 0.f ? r2 : cand.back().first;
        int e = 0;
        (void)std::frexp((double)B, &e);
        const double s = std::ldexp(1.0, 15 - (int)std::ceil(e / 2.0));
        int64_t S[3] = {0, 0, 0}, SS[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (const auto& cj : cand) {
            const PointXYZI& p = c[(size_t)cj.second];
            const float o[3] = {p.x - c[(size_t)i].x, p.y - c[(size_t)i].y, p.z - c[(size_t)i].z};
            int64_t q[3];
            for (int a = 0; a < 3; ++a) q[a] = (int64_t)std::rint((double)o[a] * s);
            for (int a = 0; a < 3; ++a) {
                S[a] += q[a];
                for (int b = 0; b < 3; ++b) SS[a][b] += q[a] * q[b];
            }
        }
        double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) A[a][b] = (double)SS[a][b] - ((double)S[a] * (double)S[b]) / (double)m;
        const double T = (A[0][0] + A[1][1]) + A[2][2];
        if (B == 0.f || !(T > 0.0)) {
            out.stats[3] += 1;
            continue;
        }
        const int pairs[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};
        for (int sweep = 0; sweep < 10; ++sweep) {
            if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
            for (const auto& pq : pairs) {
                const int p = pq[0], q = pq[1], r = pq[2];
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                const double arp = A[r][p], arq = A[r][q];
                A[r][p] = A[p][r] = cs * arp - sn * arq;
                A[r][q] = A[q][r] = sn * arp + cs * arq;
                for (int row = 0; row < 3; ++row) {
                    const double vp = V[row][p], vq = V[row][q];
                    V[row][p] = cs * vp - sn * vq;
                    V[row][q] = sn * vp + cs * vq;
                }
            }
        }
        int col = 0;
        if (A[1][1] < A[0][0]) col = 1;
        if (A[2][2] < A[col][col]) col = 2;
        double nv[3] = {V[0][col], V[1][col], V[2][col]};
        bool flip;
        if (!vps.empty()) {
            const std::array<float, 3>& v = vps.size() == 1 ? vps[0] : vps[(size_t)i];
            const double sd = (((double)v[0] - (double)c[(size_t)i].x) * nv[0] + ((double)v[1] - (double)c[(size_t)i].y) * nv[1]) +
                              ((double)v[2] - (double)c[(size_t)i].z) * nv[2];
            flip = sd < 0.0;
        } else {
            flip = nv[2] < 0.0 || (nv[2] == 0.0 && (nv[1] < 0.0 || (nv[1] == 0.0 && nv[0] < 0.0)));
        }
        if (flip) nv[0] = -nv[0], nv[1] = -nv[1], nv[2] = -nv[2];
        out.normals[(size_t)i] = {(float)nv[0], (float)nv[1], (float)nv[2], (float)(std::fabs(A[col][col]) / T)};
        out.stats[1] += 1;
    }
    return out;
}

static bool same_bits(const std::vector<Normal>& a, const std::vector<Normal>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        const float x[4] = {a[i].normal_x, a[i].normal_y, a[i].normal_z, a[i].curvature};
        const float y[4] = {b[i].normal_x, b[i].normal_y, b[i].normal_z, b[i].curvature};
        for (int d = 0; d < 4; ++d) {
            if (std::isnan(x[d]) && std::isnan(y[d])) continue;
            if (std::memcmp(&x[d], &y[d], 4) != 0) {
                std::printf("  point %zu field %d: %.9g / %.9g\n", i, d, (double)x[d], (double)y[d]);
                return false;
            }
        }
    }
    return true;
}

int main() {
    try {
        lio_gpu::FilterGPU f;
        // 4097 points: a rough ground, a wall, a pole, sparse clutter; a few rows non-finite, a few duplicated
        std::vector<PointXYZI> cloud(4097);
        for (size_t i = 0; i < cloud.size(); ++i) {
            const float u = frand(), a = frand(), b = frand(), cc = frand();
            if (u < 0.55f) cloud[i] = {12.f * a - 6.f, 12.f * b - 6.f, 0.02f * cc, 1.f};
            else if (u < 0.8f) cloud[i] = {3.f + 0.01f * cc, 6.f * a - 3.f, 3.f * b, 2.f};
            else if (u < 0.9f) cloud[i] = {-2.f + 0.03f * a, -2.f + 0.03f * b, 4.f * cc, 3.f};
            else cloud[i] = {40.f * a - 20.f, 40.f * b - 20.f, 8.f * cc, 4.f};
        }
        cloud[0].x = NAN, cloud[4096].z = INFINITY;
        for (size_t i = 11; i < cloud.size(); i += 409) cloud[i].y = NAN;
        for (size_t i = 100; i < 110; ++i) cloud[i] = cloud[99];

        lio_gpu::NormalEstimation<PointXYZI> ne(f);
        ne.setInputCloud(&cloud);
        std::vector<Normal> normals;
        try {  // PCL's defaults, k 0 and radius 0, are the library's argument error
            ne.compute(normals);
            std::printf("FAIL: k = 0 and radius = 0 were accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        std::vector<std::array<float, 3>> poses(cloud.size());
        for (size_t i = 0; i < poses.size(); ++i) poses[i] = {0.01f * (float)i - 20.f, 1.f, 1.5f};
        const struct {
            double radius;
            int k, vp_mode;
        } cases[4] = {{0.0, 16, 1}, {0.5, 0, 0}, {0.5, 30, 2}, {0.0, 255, 1}};
        for (const auto& cs : cases) {
            ne.setKSearch(cs.k);
            ne.setRadiusSearch(cs.radius);
            std::vector<std::array<float, 3>> vps;
            if (cs.vp_mode == 0) ne.useNoViewPoint();
            if (cs.vp_mode == 1) ne.setViewPoint(0.5f, -0.25f, 1.5f), vps = {{0.5f, -0.25f, 1.5f}};
            if (cs.vp_mode == 2) ne.setViewPoints(poses), vps = poses;
            ne.compute(normals);
            const Ref ref = brute_normals(cloud, (float)cs.radius, cs.k, vps);
            const bool ok = same_bits(normals, ref.normals) && ne.counts() == ref.counts &&
                            std::memcmp(ne.stats(), ref.stats, sizeof(ref.stats)) == 0;
            std::printf("radius %g, k %d, viewpoint mode %d: %lld finite, %lld normals, %lld short, %lld degenerate, max %lld, "
                        "sum %lld\n",
                        cs.radius, cs.k, cs.vp_mode, (long long)ref.stats[0], (long long)ref.stats[1], (long long)ref.stats[2],
                        (long long)ref.stats[3], (long long)ref.stats[4], (long long)ref.stats[5]);
            if (!ok || ref.stats[0] != 4097 - 12 || ref.stats[1] < 2000) {
                std::printf("FAIL: compute() differs from the host loop: stats %lld %lld %lld %lld %lld %lld\n",
                            (long long)ne.stats()[0], (long long)ne.stats()[1], (long long)ne.stats()[2], (long long)ne.stats()[3],
                            (long long)ne.stats()[4], (long long)ne.stats()[5]);
                return 1;
            }
        }
        std::printf("ALL OK\n");
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
