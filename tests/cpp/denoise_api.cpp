// The denoise mirrors of include/lio_gpu.hpp as a C++ maintainer uses them: StatisticalOutlierRemoval<PointT>
// beside VoxelGrid on one FilterGPU, DenoiseConfig and denoise_slam_map.  On the GPU the SOR result is checked
// exactly against a brute-force restatement (float squared distances, double square roots added in ascending
// order, PCL's threshold loop) and the denoised map against its own counts.  Exit 77: no device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::PointXYZI;

static uint32_t g_state = 12345u;
static float frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

static std::vector<PointXYZI> brute_sor(const std::vector<PointXYZI>& c, int k, double mul, bool negative, double* thr) {
    const size_t n = c.size();
    std::vector<float> dist(n, 0.f), d2(n);
    for (size_t i = 0; i < n; ++i) {
        for (size_t j = 0; j < n; ++j) {
            const float dx = c[i].x - c[j].x, dy = c[i].y - c[j].y, dz = c[i].z - c[j].z;
            d2[j] = (dx * dx + dy * dy) + dz * dz;
        }
        std::partial_sort(d2.begin(), d2.begin() + k + 1, d2.end());
        double s = 0.0;
        for (int t = 1; t <= k; ++t) s += std::sqrt((double)d2[t]);
        dist[i] = (float)(s / (double)k);
    }
    double sum = 0.0, sq = 0.0;
    for (size_t i = 0; i < n; ++i) {
        sum += dist[i];
        const float dd = dist[i] * dist[i];
        sq += (double)dd;
    }
    const double nv = (double)n, mean = sum / nv, var = (sq - sum * sum / nv) / (nv - 1.0);
    *thr = mean + mul * std::sqrt(var);
    std::vector<PointXYZI> out;
    for (size_t i = 0; i < n; ++i)
        if (!((!negative && dist[i] > *thr) || (negative && dist[i] <= *thr))) out.push_back(c[i]);
    return out;
}

static bool same(const std::vector<PointXYZI>& a, const std::vector<PointXYZI>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].x != b[i].x || a[i].y != b[i].y || a[i].z != b[i].z || a[i].intensity != b[i].intensity) return false;
    return true;
}

int main() {
    try {
        lio_gpu::FilterGPU f;
        std::vector<PointXYZI> cloud(3000);
        for (auto& p : cloud) p = {8.f * frand(), 8.f * frand(), 2.f * frand(), 500.f + 1500.f * frand()};
        for (int i = 0; i < 300; ++i)  // a signboard above seed_thres with a dimmer halo
            cloud[i] = {3.f + frand(), 4.f + 0.01f * frand(), 1.f + frand(), 2801.f + 600.f * frand()};
        for (int i = 300; i < 500; ++i)
            cloud[i] = {2.8f + 1.4f * frand(), 4.f + 0.15f * (frand() - 0.5f), 0.8f + 1.4f * frand(), 2000.f + 700.f * frand()};
        for (int i = 500; i < 600; ++i) cloud[i].intensity = 0.f;

        lio_gpu::StatisticalOutlierRemoval<PointXYZI> sor(f);
        sor.setInputCloud(&cloud);
        sor.setMeanK(20);
        sor.setStddevMulThresh(1.0);
        std::vector<PointXYZI> kept, removed;
        sor.filter(kept);
        double thr = 0.0;
        if (!same(kept, brute_sor(cloud, 20, 1.0, false, &thr)) || sor.stats()[2] != thr || sor.stats()[3] != 3000.0) {
            std::printf("FAIL: SOR differs from the brute-force restatement\n");
            return 1;
        }
        sor.setNegative(true);
        sor.filter(removed);
        if (!same(removed, brute_sor(cloud, 20, 1.0, true, &thr)) || kept.size() + removed.size() != cloud.size() ||
            kept.empty() || removed.empty()) {
            std::printf("FAIL: negative is not the complement\n");
            return 1;
        }

        lio_gpu::VoxelGrid<PointXYZI> vg(f);  // the same handle serves both filters
        vg.setLeafSize(0.5f, 0.5f, 0.5f);
        vg.setInputCloud(&cloud);
        std::vector<PointXYZI> down;
        vg.filter(down);

        lio_gpu::DenoiseConfig cfg;
        if (cfg.seed_thres != 2800.f || cfg.cluster_seed_radius != 1.0f || cfg.MeanK != 50 || cfg.denoise_en) return 1;
        cfg.cluster_seed_radius = 0.1f;
        std::vector<PointXYZI> map = cloud;
        int64_t counts[5] = {0, 0, 0, 0, 0};
        lio_gpu::denoise_slam_map(f, cfg, map, counts);
        bool ok = counts[0] == 300 && counts[1] >= counts[0] && counts[2] <= counts[1] && counts[3] <= counts[2] &&
                  (int64_t)map.size() == counts[3] + counts[4] && counts[1] + counts[4] == 2900;
        for (const auto& p : map) ok = ok && p.intensity != 0.f;
        if (!ok || down.empty()) {
            std::printf("FAIL: denoise_slam_map counts %lld %lld %lld %lld %lld, %zu points\n", (long long)counts[0],
                        (long long)counts[1], (long long)counts[2], (long long)counts[3], (long long)counts[4], map.size());
            return 1;
        }
        std::printf("SOR kept %zu of %zu; denoise: seeds %lld segmented %lld sor %lld denoised %lld remained %lld\nALL OK\n",
                    kept.size(), cloud.size(), (long long)counts[0], (long long)counts[1], (long long)counts[2],
                    (long long)counts[3], (long long)counts[4]);
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
