// The DBSCAN mirror of include/lio_gpu.hpp as a C++ maintainer uses it: DBSCAN<PointT> beside the other filters on
// one FilterGPU, the call of post_process/clustering.py:30-36.  On the GPU extract() is checked exactly against
// the sequential procedure written here — clusters opened in index order at unlabelled core points and expanded
// fully with a stack, an O(n^2) neighbour test (float squared distances, inclusive), a border point kept by the
// cluster that reaches it first — with the labels, the core flags and the bounding boxes.  Exit 77: no device.
#include <algorithm>
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

static bool neighbours(const PointXYZI& a, const PointXYZI& b, float e2) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz <= e2;  // false for a NaN point
}

// labels (-1: noise) and core flags by the sequential loop; returns the number of clusters
static int brute_dbscan(const std::vector<PointXYZI>& c, double eps, int64_t min_samples, std::vector<int32_t>& label,
                        std::vector<uint8_t>& core) {
    const int n = (int)c.size();
    const float e2 = (float)(eps * eps);
    core.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        int64_t cnt = 0;
        for (int j = 0; j < n; ++j) cnt += neighbours(c[(size_t)i], c[(size_t)j], e2) ? 1 : 0;
        core[(size_t)i] = cnt >= min_samples ? 1 : 0;
    }
    label.assign((size_t)n, -1);
    int next = 0;
    for (int i = 0; i < n; ++i) {
        if (label[(size_t)i] != -1 || !core[(size_t)i]) continue;
        std::vector<int> stack{i};
        label[(size_t)i] = next;
        while (!stack.empty()) {
            const int a = stack.back();
            stack.pop_back();
            if (!core[(size_t)a]) continue;  // a border point spreads nothing
            for (int j = 0; j < n; ++j)
                if (label[(size_t)j] == -1 && neighbours(c[(size_t)a], c[(size_t)j], e2)) {
                    label[(size_t)j] = next;
                    stack.push_back(j);
                }
        }
        ++next;
    }
    return next;
}

int main() {
    try {
        lio_gpu::FilterGPU f;
        // 2000 points: 30 blobs of sigma 0.12 m with skewed membership in a 40 m box (pairs of blobs 0.9 m apart, so
        // that border points lie between two clusters), 200 sprinkled points, a few NaN
        float centre[30][3];
        for (int k = 0; k < 30; k += 2) {
            centre[k][0] = 40.f * frand(), centre[k][1] = 40.f * frand(), centre[k][2] = 4.f * frand();
            centre[k + 1][0] = centre[k][0] + 0.9f, centre[k + 1][1] = centre[k][1], centre[k + 1][2] = centre[k][2];
        }
        std::vector<PointXYZI> cloud(2000);
        for (size_t i = 0; i < cloud.size(); ++i) {
            PointXYZI& p = cloud[i];
            if (i % 10 == 9) {
                p = {40.f * frand(), 40.f * frand(), 4.f * frand(), 1.f};
                continue;
            }
            const float u = frand();
            const int who = std::min((int)(u * u * 30.f), 29);
            p = {centre[who][0] + 0.12f * gauss(), centre[who][1] + 0.12f * gauss(), centre[who][2] + 0.12f * gauss(),
                 100.f * frand()};
        }
        for (size_t i = 5; i < cloud.size(); i += 211) cloud[i].x = NAN;

        lio_gpu::DBSCAN<PointXYZI> db(f);
        db.setInputCloud(&cloud);
        std::vector<lio_gpu::PointIndices> clusters;
        db.setEps(0.0);
        try {  // eps 0: the library's argument error
            db.extract(clusters);
            std::printf("FAIL: eps 0 was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        const struct {
            double eps;
            int64_t min_samples;
        } cases[4] = {{0.5, 10}, {0.3, 3}, {0.25, 12}, {1.0, 1}};
        size_t seen_border = 0, seen_clusters = 0;
        for (const auto& cs : cases) {
            db.setEps(cs.eps);
            db.setMinSamples(cs.min_samples);
            db.extract(clusters);
            std::vector<int32_t> lab;
            std::vector<uint8_t> core;
            const int m = brute_dbscan(cloud, cs.eps, cs.min_samples, lab, core);
            bool ok = (int)clusters.size() == m && (int)db.aabbs().size() == m && lab == db.labels() && core == db.core();
            int64_t n_core = 0, n_in = 0;
            for (size_t i = 0; i < cloud.size(); ++i) n_core += core[i], n_in += lab[i] >= 0 ? 1 : 0;
            for (int k = 0; ok && k < m; ++k) {
                std::vector<int> members;
                float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (size_t i = 0; i < cloud.size(); ++i)
                    if (lab[i] == k) {
                        members.push_back((int)i);
                        const float v[3] = {cloud[i].x, cloud[i].y, cloud[i].z};
                        for (int d = 0; d < 3; ++d) lo[d] = std::min(lo[d], v[d]), hi[d] = std::max(hi[d], v[d]);
                    }
                ok = clusters[(size_t)k].indices == members;
                for (int d = 0; d < 3; ++d)
                    ok = ok && db.aabbs()[(size_t)k].min[d] == lo[d] && db.aabbs()[(size_t)k].max[d] == hi[d];
            }
            ok = ok && db.stats()[0] == 1990 && db.stats()[1] == n_core && db.stats()[2] == m && db.stats()[3] == n_in;
            if (!ok) {
                std::printf("FAIL: extract(eps %g, min_samples %lld) differs from the sequential restatement (%zu / %d clusters)\n",
                            cs.eps, (long long)cs.min_samples, clusters.size(), m);
                return 1;
            }
            seen_border += (size_t)(n_in - n_core);
            seen_clusters += (size_t)m;
            std::printf("eps %g min_samples %lld: %d clusters, %lld core, %lld border, %lld noise\n", cs.eps,
                        (long long)cs.min_samples, m, (long long)n_core, (long long)(n_in - n_core),
                        (long long)(1990 - n_in));
        }
        if (!seen_border || !seen_clusters) {
            std::printf("FAIL: the cloud has no border point or no cluster\n");
            return 1;
        }

        // the clustered points go on through the same handle's other filters
        std::vector<PointXYZI> objects;
        db.setEps(0.5);
        db.setMinSamples(10);
        db.extract(clusters);
        for (const auto& c : clusters)
            for (int i : c.indices) objects.push_back(cloud[(size_t)i]);
        lio_gpu::VoxelGrid<PointXYZI> vg(f);
        vg.setLeafSize(0.5f, 0.5f, 0.5f);
        vg.setInputCloud(&objects);
        std::vector<PointXYZI> down;
        vg.filter(down);
        if (objects.empty() || down.empty()) {
            std::printf("FAIL: no clustered point\n");
            return 1;
        }
        std::printf("%zu points in %zu clusters\nALL OK\n", objects.size(), clusters.size());
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
