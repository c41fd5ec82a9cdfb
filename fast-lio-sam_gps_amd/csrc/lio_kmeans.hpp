// lio_kmeans.hpp — k-means with k-means++ seeding and per-cluster bounding boxes (lio_kmeans.hip): the
// cv::kmeans call of post_process/lidar_projection/src/lidar_projection.cpp:82-92 [U], restated as the contract
// of lio_kmeans (include/lio_gpu.h): fixed-point sums, counter-based draws, the best of `attempts` runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lio {

constexpr int kKmMaxK = 64;         // clusters
constexpr int kKmMaxAttempts = 16;
constexpr int kKmMaxIter = 1000;

// What the device keeps between the launches of one call (one copy, uploaded from and read back to h_pin).
constexpr int kKmSpread = 16;       // copies of a global accumulator, each on cache lines of its own

struct KmState {
    unsigned long long cq[kKmSpread * 8];  // compactness of the attempt: workgroup b adds to cq[(b % 16) * 8]
    unsigned long long amax;     // the repair's (float bits of d2, ~index)
    unsigned long long nf;       // finite points
    uint32_t bbox[6];            // of the finite points, as order-preserving keys: min x, y, z, max x, y, z
    uint32_t first_finite;       // lowest finite index
    int32_t cur;                 // slot of the current weights
    int32_t cand[3];             // the three trials' candidates
    int32_t pad;
};

// Scratch of lio_kmeans: ONE device arena sized for cap_n points, grown geometrically (counted:
// lio_alloc_count), and a small pinned block.  24 bytes per point.
struct KMeansBuf {
    void* arena = nullptr;
    size_t arena_bytes = 0;
    int64_t cap_n = 0;
    int32_t* labels[2] = {nullptr, nullptr};                // the running attempt's and the best attempt's
    uint32_t* w[4] = {nullptr, nullptr, nullptr, nullptr};  // seeding weights: current + three trials
    unsigned long long* part[4] = {nullptr, nullptr, nullptr, nullptr};  // per kKmChunk points: the sum of w
    unsigned long long* acc = nullptr;                      // kKmSpread copies of 4 per cluster: count, sum qx, qy, qz
    uint32_t* box = nullptr;                                // 6 per cluster, order-preserving keys
    int32_t* seeds = nullptr;                               // attempts x K
    KmState* state = nullptr;
    void* h_pin = nullptr;                                  // pinned: acc (every copy), state, seeds, boxes
};

struct KMeansArgs {
    int K = 5, max_iter = 100, attempts = 3;
    float eps = 0.1f;
    uint64_t seed = 0;
    const float* init_centers = nullptr;  // attempts x K x 3, host; null: k-means++ seeding
};

// Everything but the labels, on the host.  The labels of the best attempt are on the device at `labels`.
struct KMeansResult {
    const int32_t* labels = nullptr;
    float centers[3 * kKmMaxK];
    int64_t counts[kKmMaxK];
    float aabb[6 * kKmMaxK];
    int32_t seeds[kKmMaxAttempts * kKmMaxK];
    uint64_t attempt_q[kKmMaxAttempts];
    int32_t attempt_iters[kKmMaxAttempts];
    int64_t nf = 0, best = 0, repairs = 0;
    int ec = 0, ed = 0;
};

void kmeans_free(KMeansBuf& b);

// Clusters the n records at d_pts (device; h_pts: the same records on the host, read for the seeds' and the
// repaired points' coordinates).  One wait after the counting pass, one per attempt after the seeding, one per
// Lloyd iteration (the K x 4 integer sums), one per repaired cluster and one per attempt for its compactness.
// kArg with "fewer finite points than clusters" in last_error() when nf < K (nothing written).
// Status (lio_scratch.hpp): kOk, kArg, kHip (text in last_error()), kNoMem.
int kmeans(KMeansBuf& b, const float* d_pts, const float* h_pts, int64_t n, int stride, const KMeansArgs& a,
           bool want_boxes, KMeansResult* out, hipStream_t st);

}  // namespace lio
