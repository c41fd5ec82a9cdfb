// The k-means mirror of include/lio_gpu.hpp as a C++ maintainer uses it: KMeans<PointT> beside the other filters
// on one FilterGPU, the cv::kmeans call of post_process/lidar_projection/src/lidar_projection.cpp:82-92.  On the
// GPU compute() is checked exactly against the contract of lio_kmeans written here as a plain sequential loop in
// the same float order: the two scales, the draws, the k-means++ seeding with three trials, Lloyd with the
// empty-cluster repair on integer sums, the best attempt, counts and boxes.  n = 4097, K = 5.  Exit 77: no device.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lio_gpu.hpp"

using lio_gpu::PointXYZI;

static uint32_t g_state = 24680u;
static float frand() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}
static float gauss() {  // sum of 12 uniforms - 6
    float s = 0.f;
    for (int k = 0; k < 12; ++k) s += frand();
    return s - 6.f;
}

static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Ref {
    std::vector<int> labels;
    std::vector<std::array<float, 3>> centers;
    std::vector<int64_t> counts;
    std::vector<lio_gpu::ClusterAABB> boxes;
    std::vector<int32_t> seeds;
    double compactness = 0.0;
    int64_t stats[6] = {0, 0, 0, 0, 0, 0};
};

static float d2(const PointXYZI& p, const float* c) {
    const float dx = p.x - c[0], dy = p.y - c[1], dz = p.z - c[2];
    return (dx * dx + dy * dy) + dz * dz;
}

static Ref brute_kmeans(const std::vector<PointXYZI>& c, int K, int max_iter, float eps, int attempts, uint64_t seed) {
    const int n = (int)c.size();
    std::vector<int> fin;
    for (int i = 0; i < n; ++i)
        if (std::isfinite(c[(size_t)i].x) && std::isfinite(c[(size_t)i].y) && std::isfinite(c[(size_t)i].z)) fin.push_back(i);
    const int64_t nf = (int64_t)fin.size();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i : fin) {
        const float v[3] = {c[(size_t)i].x, c[(size_t)i].y, c[(size_t)i].z};
        for (int d = 0; d < 3; ++d) lo[d] = std::min(lo[d], v[d]), hi[d] = std::max(hi[d], v[d]);
    }
    float A = 0.f;
    for (int d = 0; d < 3; ++d) A = std::max(A, std::max(std::fabs(lo[d]), std::fabs(hi[d])));
    const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
    const float D2 = (ex * ex + ey * ey) + ez * ez;
    int ec = 0, ed = 0;
    if (A != 0.f) (void)std::frexp(A, &ec);
    if (D2 != 0.f) (void)std::frexp(D2, &ed);
    const double sx = std::ldexp(1.0, 31 - ec), sd = std::ldexp(1.0, 31 - ed), inv = std::ldexp(1.0, ec - 31);
    auto q = [&](float d) { return (uint64_t)std::floor((double)d * sd); };
    auto qx = [&](float v) { return (int64_t)std::rint((double)v * sx); };
    auto r = [&](uint64_t cc) { return mix(seed + (cc + 1) * 0x9E3779B97F4A7C15ull); };
    auto xyz = [&](int i, int d) { return d == 0 ? c[(size_t)i].x : d == 1 ? c[(size_t)i].y : c[(size_t)i].z; };

    Ref best;
    uint64_t best_q = 0;
    int64_t repairs = 0;
    best.seeds.assign((size_t)(attempts * K), -1);
    for (int a = 0; a < attempts; ++a) {
        // ---- seeding ----
        std::vector<std::array<float, 3>> C((size_t)K);
        std::vector<uint64_t> w((size_t)n, 0), w2((size_t)n), wbest((size_t)n);
        int ci = fin[(size_t)(r((uint64_t)a * K * 3) % (uint64_t)nf)];
        for (int k = 0; k < K; ++k) {
            if (k > 0) {
                uint64_t sum0 = 0, sbest = 0;
                for (int i : fin) sum0 += w[(size_t)i];
                for (int j = 0; j < 3; ++j) {
                    const uint64_t u = r(((uint64_t)a * K + k) * 3 + j) >> 11;
                    const uint64_t t = (uint64_t)(((unsigned __int128)u * sum0) >> 53);
                    int cand = fin[0];
                    uint64_t pre = 0;
                    if (sum0)
                        for (int i : fin) {
                            pre += w[(size_t)i];
                            if (pre > t) {
                                cand = i;
                                break;
                            }
                        }
                    const float pc[3] = {c[(size_t)cand].x, c[(size_t)cand].y, c[(size_t)cand].z};
                    uint64_t s = 0;
                    for (int i : fin) s += (w2[(size_t)i] = std::min(q(d2(c[(size_t)i], pc)), w[(size_t)i]));
                    if (j == 0 || s < sbest) sbest = s, ci = cand, wbest = w2;
                }
                w = wbest;
            } else {
                const float pc[3] = {c[(size_t)ci].x, c[(size_t)ci].y, c[(size_t)ci].z};
                for (int i : fin) w[(size_t)i] = q(d2(c[(size_t)i], pc));
            }
            best.seeds[(size_t)(a * K + k)] = ci;
            C[(size_t)k] = {c[(size_t)ci].x, c[(size_t)ci].y, c[(size_t)ci].z};
        }
        // ---- Lloyd ----
        std::vector<int> lab((size_t)n, -1);
        std::vector<int64_t> cnt((size_t)K);
        auto assign = [&]() {
            for (int i : fin) {
                int b = 0;
                float bd = d2(c[(size_t)i], C[0].data());
                for (int k = 1; k < K; ++k) {
                    const float d = d2(c[(size_t)i], C[(size_t)k].data());
                    if (d < bd) bd = d, b = k;
                }
                lab[(size_t)i] = b;
            }
        };
        assign();
        int it = 1;
        for (;;) {
            std::vector<std::array<int64_t, 3>> S((size_t)K, {0, 0, 0});
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int i : fin) {
                const size_t k = (size_t)lab[(size_t)i];
                cnt[k] += 1;
                for (int d = 0; d < 3; ++d) S[k][(size_t)d] += qx(xyz(i, d));
            }
            for (int k = 0; k < K; ++k) {
                if (cnt[(size_t)k]) continue;
                int mk = 0;
                for (int j = 1; j < K; ++j)
                    if (cnt[(size_t)j] > cnt[(size_t)mk]) mk = j;
                float m[3];
                for (int d = 0; d < 3; ++d) m[d] = (float)(((double)S[(size_t)mk][(size_t)d] / (double)cnt[(size_t)mk]) * inv);
                int far = -1;
                float fd = -1.f;
                for (int i : fin)
                    if (lab[(size_t)i] == mk && d2(c[(size_t)i], m) > fd) fd = d2(c[(size_t)i], m), far = i;
                lab[(size_t)far] = k;
                for (int d = 0; d < 3; ++d) S[(size_t)mk][(size_t)d] -= qx(xyz(far, d)), S[(size_t)k][(size_t)d] = qx(xyz(far, d));
                cnt[(size_t)mk] -= 1, cnt[(size_t)k] = 1;
                ++repairs;
            }
            double shift = 0.0;
            for (int k = 0; k < K; ++k) {
                double t[3];
                for (int d = 0; d < 3; ++d) {
                    const float v = (float)(((double)S[(size_t)k][(size_t)d] / (double)cnt[(size_t)k]) * inv);
                    t[d] = (double)(v - C[(size_t)k][(size_t)d]);
                    C[(size_t)k][(size_t)d] = v;
                }
                shift = std::max(shift, (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
            }
            ++it;
            if (it == std::max(max_iter, 2) || shift <= (double)eps * eps) break;
            assign();
        }
        uint64_t cq = 0;
        for (int i : fin) cq += q(d2(c[(size_t)i], C[(size_t)lab[(size_t)i]].data()));
        std::printf("  attempt %d: %d iterations, cq %llu\n", a, it, (unsigned long long)cq);
        if (a == 0 || cq < best_q) {
            best_q = cq;
            best.labels = lab, best.centers = C, best.counts = cnt;
            best.stats[1] = a, best.stats[2] = it;
        }
    }
    best.compactness = std::ldexp((double)best_q, ed - 31);
    best.stats[0] = nf, best.stats[3] = repairs, best.stats[4] = ec, best.stats[5] = ed;
    best.boxes.assign((size_t)K, lio_gpu::ClusterAABB{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}});
    for (int i : fin) {
        lio_gpu::ClusterAABB& b = best.boxes[(size_t)best.labels[(size_t)i]];
        for (int d = 0; d < 3; ++d) b.min[d] = std::min(b.min[d], xyz(i, d)), b.max[d] = std::max(b.max[d], xyz(i, d));
    }
    return best;
}

int main() {
    try {
        lio_gpu::FilterGPU f;
        // 4097 points: five blobs on a ground, a few rows non-finite, a few duplicated
        float centre[5][3];
        for (auto& c : centre) c[0] = 80.f * frand() - 40.f, c[1] = 80.f * frand() - 40.f, c[2] = 4.f * frand();
        std::vector<PointXYZI> cloud(4097);
        for (size_t i = 0; i < cloud.size(); ++i) {
            const int who = (int)(frand() * 5.f) % 5;
            cloud[i] = {centre[who][0] + 3.f * gauss(), centre[who][1] + 3.f * gauss(), centre[who][2] + 0.3f * gauss(), 10.f * who};
        }
        cloud[0].x = NAN, cloud[4096].z = INFINITY;
        for (size_t i = 11; i < cloud.size(); i += 409) cloud[i].y = NAN;
        for (size_t i = 100; i < 140; ++i) cloud[i] = cloud[99];

        lio_gpu::KMeans<PointXYZI> km(f);
        km.setInputCloud(&cloud);
        std::vector<int> labels;
        std::vector<std::array<float, 3>> centers;
        try {  // K = 0 is the library's argument error
            km.setK(0);
            km.compute(labels, centers);
            std::printf("FAIL: K = 0 was accepted\n");
            return 1;
        } catch (const lio_gpu::Error& e) {
            if (e.code != LIO_ERR_ARG) throw;
        }
        const struct {
            int K, max_iter;
            double eps;
            int attempts;
            uint64_t seed;
        } cases[3] = {{5, 100, 0.1, 3, 0}, {5, 100, 0.0, 2, 7}, {3, 4, 0.1, 1, 0xffffffffffffffffull}};
        for (const auto& cs : cases) {
            km.setK(cs.K);
            km.setTermCriteria(cs.max_iter, cs.eps);
            km.setAttempts(cs.attempts);
            km.setSeed(cs.seed);
            const double compactness = km.compute(labels, centers);
            std::printf("K %d, (%d, %g), %d attempts:\n", cs.K, cs.max_iter, cs.eps, cs.attempts);
            const Ref ref = brute_kmeans(cloud, cs.K, cs.max_iter, (float)cs.eps, cs.attempts, cs.seed);
            bool ok = labels == ref.labels && compactness == ref.compactness && km.counts() == ref.counts &&
                      km.seeds() == ref.seeds && std::memcmp(km.stats(), ref.stats, sizeof(ref.stats)) == 0 &&
                      std::memcmp(centers.data(), ref.centers.data(), sizeof(float) * 3 * (size_t)cs.K) == 0 &&
                      std::memcmp(km.aabbs().data(), ref.boxes.data(), sizeof(lio_gpu::ClusterAABB) * (size_t)cs.K) == 0;
            if (!ok || ref.stats[0] != 4097 - 12) {
                std::printf("FAIL: compute() differs from the host loop: compactness %.17g / %.17g, stats %lld %lld %lld %lld / "
                            "%lld %lld %lld %lld\n",
                            compactness, ref.compactness, (long long)km.stats()[0], (long long)km.stats()[1],
                            (long long)km.stats()[2], (long long)km.stats()[3], (long long)ref.stats[0],
                            (long long)ref.stats[1], (long long)ref.stats[2], (long long)ref.stats[3]);
                return 1;
            }
            std::printf("  best attempt %lld, %lld iterations, compactness %.6f\n", (long long)ref.stats[1],
                        (long long)ref.stats[2], compactness);
        }

        // initial centres in place of the seeding: the five blob centres; no seeds then
        std::vector<std::array<float, 3>> init(5);
        for (size_t k = 0; k < 5; ++k) init[k] = {centre[k][0], centre[k][1], centre[k][2]};
        km.setK(5);
        km.setTermCriteria(100, 0.1);
        km.setAttempts(1);
        km.setInitialCenters(init);
        km.compute(labels, centers);
        int64_t total = 0;
        for (int64_t v : km.counts()) total += v;
        if (total != km.stats()[0] || km.seeds() != std::vector<int32_t>(5, -1) || labels[0] != -1) {
            std::printf("FAIL: initial centres: %lld points in clusters of %lld finite\n", (long long)total, (long long)km.stats()[0]);
            return 1;
        }
        std::printf("initial centres: %lld iterations\nALL OK\n", (long long)km.stats()[2]);
        return 0;
    } catch (const lio_gpu::Error& e) {
        std::printf("%s\n", e.what());
        return e.code == LIO_ERR_NODEV ? 77 : 1;
    }
}
