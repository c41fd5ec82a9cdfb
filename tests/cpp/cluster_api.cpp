// The clustering mirror of include/lio_gpu.hpp as a C++ maintainer uses it: EuclideanClusterExtraction<PointT>
// beside the other filters on one FilterGPU, the block of fast_lio_sam.cpp:343-363.  On the GPU extract() is
// checked exactly against PCL's procedure written here — the seed loop in index order with `processed` flags,
// an O(n^2) breadth-first search per seed (float squared distances, strict), sorted indices, the size filter,
// clusters by size descending (equal sizes: lowest index first, the library's contract) — with the labels and
// the bounding boxes.  Exit 77: no device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::PointXYZI;

static uint32_t g_state = 2468u;
static float frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}
static float gauss() {  // sum of 12 uniforms - 6
    float s = 0.f;
    for (int k = 0; k < 12; ++k) s += frand();
    return s - 6.f;
}

static std::vector<std::vector<int>> brute_clusters(const std::vector<PointXYZI>& c, double tolerance, int min_size,
                                                    int max_size) {
    const int n = (int)c.size();
    const float r2 = (float)(tolerance * tolerance);
    std::vector<char> processed((size_t)n, 0);
    std::vector<std::vector<int>> out;
    for (int i = 0; i < n; ++i) {
        if (processed[(size_t)i] || !std::isfinite(c[(size_t)i].x)) continue;
        std::vector<int> q{i};
        processed[(size_t)i] = 1;
        for (size_t s = 0; s < q.size(); ++s) {
            const PointXYZI& a = c[(size_t)q[s]];
            for (int j = 0; j < n; ++j) {
                if (processed[(size_t)j]) continue;
                const float dx = a.x - c[(size_t)j].x, dy = a.y - c[(size_t)j].y, dz = a.z - c[(size_t)j].z;
                if ((dx * dx + dy * dy) + dz * dz < r2) {  // false for a NaN point
                    processed[(size_t)j] = 1;
                    q.push_back(j);
                }
            }
        }
        if ((int)q.size() >= min_size && (int)q.size() <= max_size) {
            std::sort(q.begin(), q.end());
            out.push_back(q);
        }
    }
    std::stable_sort(out.begin(), out.end(), [](const std::vector<int>& a, const std::vector<int>& b) {
        return a.size() != b.size() ? a.size() > b.size() : a[0] < b[0];
    });
    return out;
}

int main() {
    try {
        lio_gpu::FilterGPU f;
        // 2000 points: 30 blobs of sigma 0.12 m with skewed membership in a 40 m box, a few of them NaN
        float centre[30][3];
        for (auto& c : centre) c[0] = 40.f * frand(), c[1] = 40.f * frand(), c[2] = 4.f * frand();
        std::vector<PointXYZI> cloud(2000);
        for (auto& p : cloud) {
            const float u = frand();
            const int who = std::min((int)(u * u * 30.f), 29);
            p = {centre[who][0] + 0.12f * gauss(), centre[who][1] + 0.12f * gauss(), centre[who][2] + 0.12f * gauss(),
                 100.f * frand()};
        }
        for (size_t i = 5; i < cloud.size(); i += 211) cloud[i].x = NAN;

        lio_gpu::EuclideanClusterExtraction<PointXYZI> ec(f);
        ec.setInputCloud(&cloud);
        std::vector<lio_gpu::PointIndices> clusters;
        try {  // PCL's default tolerance 0: the library's argument error
            ec.extract(clusters);
            std::printf("FAIL: tolerance 0 was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        const int lims[3][2] = {{1, 2147483647}, {10, 250}, {5, 100}};
        size_t n_first = 0;
        for (const auto& lim : lims) {
            ec.setClusterTolerance(0.5);
            ec.setMinClusterSize(lim[0]);
            ec.setMaxClusterSize(lim[1]);
            ec.extract(clusters);
            const auto ref = brute_clusters(cloud, 0.5, lim[0], lim[1]);
            bool ok = clusters.size() == ref.size() && ec.aabbs().size() == ref.size() && ec.labels().size() == cloud.size();
            std::vector<int32_t> lab(cloud.size(), -1);
            int64_t in_clusters = 0;
            for (size_t k = 0; ok && k < ref.size(); ++k) {
                ok = clusters[k].indices == ref[k];
                float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (int i : ref[k]) {
                    const float v[3] = {cloud[(size_t)i].x, cloud[(size_t)i].y, cloud[(size_t)i].z};
                    for (int d = 0; d < 3; ++d) lo[d] = std::min(lo[d], v[d]), hi[d] = std::max(hi[d], v[d]);
                    lab[(size_t)i] = (int32_t)k;
                }
                in_clusters += (int64_t)ref[k].size();
                for (int d = 0; d < 3; ++d) ok = ok && ec.aabbs()[k].min[d] == lo[d] && ec.aabbs()[k].max[d] == hi[d];
            }
            ok = ok && lab == ec.labels() && ec.stats()[2] == (int64_t)ref.size() && ec.stats()[3] == in_clusters &&
                 ec.stats()[0] == 1990;
            if (!ok || ref.empty()) {
                std::printf("FAIL: extract(min %d, max %d) differs from the breadth-first restatement (%zu / %zu clusters)\n",
                            lim[0], lim[1], clusters.size(), ref.size());
                return 1;
            }
            if (!n_first) n_first = ref.size();
            std::printf("min %d max %d: %zu clusters, largest %zu, %lld of %lld components\n", lim[0], lim[1], ref.size(),
                        ref[0].size(), (long long)ec.stats()[2], (long long)ec.stats()[1]);
        }

        // the reference's block: keep the clusters of more than 100 points (fast_lio_sam.cpp:356-362)
        ec.setMinClusterSize(10);
        ec.setMaxClusterSize(25000);
        ec.extract(clusters);
        std::vector<PointXYZI> signboards;
        for (const auto& c : clusters)
            if (c.indices.size() > 100)
                for (int i : c.indices) signboards.push_back(cloud[(size_t)i]);
        lio_gpu::VoxelGrid<PointXYZI> vg(f);  // the same handle serves the other filters
        vg.setLeafSize(0.5f, 0.5f, 0.5f);
        vg.setInputCloud(&signboards);
        std::vector<PointXYZI> down;
        vg.filter(down);
        if (signboards.empty() || down.empty() || n_first == 0) {
            std::printf("FAIL: no cluster of more than 100 points\n");
            return 1;
        }
        std::printf("%zu points in clusters of more than 100\nALL OK\n", signboards.size());
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
