// The plane segmentation mirror of include/lio_gpu.hpp as a C++ maintainer uses it: PlaneSegmentation<PointT>
// beside the other filters on one FilterGPU, the ground removal of post_process/clustering.py:21-28 ahead of the
// clustering.  On the GPU segment() is checked exactly against the contract of lio_segment_plane written here
// as an O(K n) host loop in the same float order: the sampler's triples, the plane of every triple, count and
// the fixed-point squared sum per hypothesis, the winner by (-count, sq, index), its inliers.  Exit 77: no
// device.
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::PointXYZI;

static uint32_t g_state = 97531u;
static float frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}
static float gauss() {  // sum of 12 uniforms - 6
    float s = 0.f;
    for (int k = 0; k < 12; ++k) s += frand();
    return s - 6.f;
}

struct Best {
    int64_t t = -1, count = 0;
    uint64_t sq = 0;
    float plane[4] = {0.f, 0.f, 0.f, 0.f};
};

static Best brute_plane(const std::vector<PointXYZI>& c, float thr, int K, uint64_t seed, std::vector<int>& inliers,
                        int& n_degenerate) {
    const int n = (int)c.size();
    std::vector<int32_t> tri(3 * (size_t)K);
    if (lio_plane_sample_triples(seed, n, K, tri.data()) != LIO_OK) throw lio_gpu::Error(LIO_ERR_ARG, "sampler");
    const float thr2 = thr * thr;
    int e = 0;
    (void)std::frexp(thr2, &e);
    const double S = std::ldexp(1.0, 32 - e);
    Best best;
    n_degenerate = 0;
    for (int t = 0; t < K; ++t) {
        const PointXYZI &p0 = c[(size_t)tri[3 * t]], &p1 = c[(size_t)tri[3 * t + 1]], &p2 = c[(size_t)tri[3 * t + 2]];
        const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
        const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float len = std::sqrt((nx * nx + ny * ny) + nz * nz);
        const float a = nx / len, b = ny / len, cc = nz / len;
        const float d = -((a * p0.x + b * p0.y) + cc * p0.z);
        if (!(std::isfinite(len) && len > 0.f && std::isfinite(d))) {
            ++n_degenerate;
            continue;
        }
        int64_t count = 0;
        uint64_t sq = 0;
        for (int i = 0; i < n; ++i) {
            const float dist = std::fabs(((a * c[(size_t)i].x + b * c[(size_t)i].y) + cc * c[(size_t)i].z) + d);
            if (dist < thr) {
                ++count;
                sq += (uint64_t)std::floor((double)(float)(dist * dist) * S);
            }
        }
        if (best.t < 0 || count > best.count || (count == best.count && sq < best.sq)) {
            best.t = t, best.count = count, best.sq = sq;
            best.plane[0] = a, best.plane[1] = b, best.plane[2] = cc, best.plane[3] = d;
        }
    }
    inliers.clear();
    if (best.t >= 0)
        for (int i = 0; i < n; ++i) {
            const float dist = std::fabs(((best.plane[0] * c[(size_t)i].x + best.plane[1] * c[(size_t)i].y) +
                                          best.plane[2] * c[(size_t)i].z) + best.plane[3]);
            if (dist < thr) inliers.push_back(i);
        }
    return best;
}

int main() {
    try {
        lio_gpu::FilterGPU f;
        // 3000 points: a slightly tilted ground, a wall, 10 blobs standing on the ground; a few rows NaN and a
        // few duplicated (degenerate triples)
        float centre[10][3];
        for (auto& c : centre) c[0] = 30.f * frand() - 15.f, c[1] = 24.f * frand() - 12.f, c[2] = 0.5f + 2.f * frand();
        std::vector<PointXYZI> cloud(3000);
        for (size_t i = 0; i < cloud.size(); ++i) {
            const float u = frand();
            PointXYZI& p = cloud[i];
            if (u < 0.6f) {
                const float x = 40.f * frand() - 20.f, y = 40.f * frand() - 20.f;
                p = {x, y, 0.01f * x + 0.02f * gauss(), 10.f};
            } else if (u < 0.75f) {
                p = {40.f * frand() - 20.f, 15.f + 0.02f * gauss(), 8.f * frand(), 20.f};
            } else {
                const int who = (int)(frand() * 10.f) % 10;
                p = {centre[who][0] + 0.15f * gauss(), centre[who][1] + 0.15f * gauss(), centre[who][2] + 0.15f * gauss(), 30.f};
            }
        }
        for (size_t i = 7; i < cloud.size(); i += 307) cloud[i].y = NAN;
        for (size_t i = 1; i < 400; ++i) cloud[i] = cloud[0];

        lio_gpu::PlaneSegmentation<PointXYZI> seg(f);
        seg.setInputCloud(&cloud);
        lio_gpu::PointIndices inliers;
        std::array<float, 4> coef{};
        try {  // a threshold of 0 is the library's argument error
            seg.setDistanceThreshold(0.0);
            seg.segment(inliers, coef);
            std::printf("FAIL: threshold 0 was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        const struct {
            double thr;
            int iters;
            uint64_t seed;
        } cases[3] = {{0.2, 1000, 0}, {0.05, 257, 7}, {0.5, 64, 0xffffffffffffffffull}};
        for (const auto& cs : cases) {
            seg.setDistanceThreshold(cs.thr);
            seg.setMaxIterations(cs.iters);
            seg.setSeed(cs.seed);
            seg.segment(inliers, coef);
            std::vector<int> ref;
            int n_deg = 0;
            const Best best = brute_plane(cloud, (float)cs.thr, cs.iters, cs.seed, ref, n_deg);
            bool ok = seg.best_iteration() == best.t && inliers.indices == ref && (int64_t)ref.size() == best.count;
            for (int k = 0; k < 4; ++k) ok = ok && std::memcmp(&coef[(size_t)k], &best.plane[k], sizeof(float)) == 0;
            // the refit is close to the winner on this scene (a flat ground): a unit normal within 2.5 degrees
            const double* r = seg.refit();
            const double dot = (r[0] * coef[0] + r[1] * coef[1]) + r[2] * coef[2];
            ok = ok && dot > 0.999 && std::fabs(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) - 1.0) < 1e-12;
            if (!ok || best.t < 0 || n_deg == 0 || ref.size() < 1000) {
                std::printf("FAIL: segment(thr %g, %d iterations) differs from the host loop: t %lld / %lld, %zu / %zu inliers, "
                            "%d degenerate, dot %.9f\n",
                            cs.thr, cs.iters, (long long)seg.best_iteration(), (long long)best.t, inliers.indices.size(),
                            ref.size(), n_deg, dot);
                return 1;
            }
            std::printf("thr %g, %d iterations: winner %lld, %zu inliers, %d degenerate, plane %.6f %.6f %.6f %.6f\n", cs.thr,
                        cs.iters, (long long)best.t, ref.size(), n_deg, coef[0], coef[1], coef[2], coef[3]);
        }

        // the offline pipeline's next step on the same handle: the plane's inliers dropped, the rest clustered
        seg.setDistanceThreshold(0.2);
        seg.setMaxIterations(1000);
        seg.setSeed(0);
        seg.segment(inliers, coef);
        std::vector<char> ground(cloud.size(), 0);
        for (int i : inliers.indices) ground[(size_t)i] = 1;
        std::vector<PointXYZI> rest;
        for (size_t i = 0; i < cloud.size(); ++i)
            if (!ground[i]) rest.push_back(cloud[i]);
        lio_gpu::EuclideanClusterExtraction<PointXYZI> ec(f);
        ec.setInputCloud(&rest);
        ec.setClusterTolerance(0.5);
        ec.setMinClusterSize(10);
        ec.setMaxClusterSize(10000);
        std::vector<lio_gpu::PointIndices> clusters;
        ec.extract(clusters);
        if (clusters.size() < 5) {
            std::printf("FAIL: %zu clusters above the ground\n", clusters.size());
            return 1;
        }
        std::printf("%zu clusters above the ground (%zu of %zu points)\nALL OK\n", clusters.size(), rest.size(), cloud.size());
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
