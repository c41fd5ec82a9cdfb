// lio_plane.hpp — RANSAC plane segmentation (lio_plane.hip): Open3D's PointCloud::SegmentPlane [U] as the
// offline pipeline calls it (post_process/clustering.py:21-28), restated as the contract of lio_segment_plane
// (include/lio_gpu.h): every hypothesis evaluated, ranked by (inliers descending, fixed-point squared error
// ascending, hypothesis index ascending).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "lio_denoise.hpp"

namespace lio {

struct PlaneWinner {  // written by the selection kernel
    float plane[4];   // (0, 0, 0, 0) when best < 0
    int32_t best;     // winning hypothesis, -1: every hypothesis is degenerate
    int32_t pad;
};

// Scratch of the plane segmentation beside the DenoiseBuf it shares the flags and the scan with: ONE device
// arena sized for cap_n points and cap_k hypotheses, each grown geometrically (counted: lio_alloc_count), and
// a small pinned block.  5 bytes per point, 32 bytes per hypothesis.
struct PlaneBuf {
    void* arena = nullptr;
    size_t arena_bytes = 0;
    int64_t cap_n = 0, cap_k = 0;
    float4* planes = nullptr;            // per hypothesis (a, b, c, d); NaN when degenerate
    unsigned long long* cnt = nullptr;   // per hypothesis: inliers
    unsigned long long* sq = nullptr;    // per hypothesis: fixed-point sum of squared distances
    uint8_t* mask = nullptr;             // per point: 1 for an inlier of the winner
    int32_t* inliers = nullptr;          // the inliers, ascending
    double* part = nullptr;              // moment partials, 9 per block
    double* mom = nullptr;               // 10: sum of d (3), of d d^T (xx xy xz yy yz zz), the reference index
    PlaneWinner* win = nullptr;
    void* h_pin = nullptr;               // pinned: PlaneWinner, then mom
    std::vector<float> h_planes;         // host side of the hypotheses: 4 K
    std::vector<uint8_t> h_deg;          // K
    std::vector<int32_t> h_tri;          // 3 K, the built-in sampler's triples
};

struct PlaneResult {
    float plane[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t best = -1;
    int64_t n_inliers = 0;
    double refit[4] = {0.0, 0.0, 0.0, 0.0};
};

void plane_free(PlaneBuf& p);

// The built-in counter-based sampler (splitmix64 of seed + (c + 1) * 0x9E3779B97F4A7C15, c = 3 t + j): K triples
// of distinct indices in [0, n), n >= 3.  Host only.
void plane_sample_triples(uint64_t seed, int64_t n, int64_t K, int32_t* out);
// false when a triple holds an index outside [0, n) or a repeated one
bool plane_triples_valid(const int32_t* tri, int64_t K, int64_t n);
// The K planes of the triples, in float in the contract's order (host: divss / sqrtss are correctly rounded);
// a degenerate hypothesis gets deg = 1 and a NaN plane, which no point is an inlier of.
void plane_hypotheses(const float* pts, int stride, const int32_t* tri, int64_t K, float* planes4, uint8_t* deg);

// Scores the K planes in p.h_planes (plane_hypotheses) against the n >= 1 records at d_pts (device; h_pts: the
// same records on the host, read for the refit's reference point), selects the winner, flags, compacts and
// takes the moments of its inliers.  Results on the device in p.cnt / p.sq (K), p.mask (n), p.inliers; the
// rest in *out.  Waits for the stream.  Status (lio_scratch.hpp): kOk, kArg, kHip (text in
// last_error()), kNoMem.
int segment_plane(DenoiseBuf& b, PlaneBuf& p, const float* d_pts, const float* h_pts, int64_t n, int stride, float thr,
                  int64_t K, bool want_refit, PlaneResult* out, hipStream_t st);

}  // namespace lio
