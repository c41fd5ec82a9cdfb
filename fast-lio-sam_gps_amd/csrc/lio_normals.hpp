// lio_normals.hpp — surface normals and curvature per point (lio_normals.hip): pcl::NormalEstimation's
// setKSearch / setRadiusSearch [U] and Open3D's hybrid search [U], by the contract of lio_estimate_normals
// (include/lio_gpu.h).  The neighbour search runs on the grid of dn_build_grid (lio_denoise.hpp); the arithmetic
// behind it is lio_normals_math.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_denoise.hpp"

namespace lio {

constexpr int kNmMaxK = 255;

// Scratch of lio_estimate_normals: ONE device arena carved into the per-point outputs (sized for `cap` points,
// grown geometrically, counted: lio_alloc_count), the per-point viewpoints and the k search's moments (each grown
// on its own: not every call has them) and pinned host memory for the six counts.
struct NormalsBuf {
    void* arena = nullptr;
    size_t arena_bytes = 0;
    int64_t cap = 0;
    float* normals = nullptr;    // 3 cap
    float* curvature = nullptr;  // cap
    int32_t* counts = nullptr;   // cap
    unsigned long long* stats = nullptr;  // 6
    float* vp = nullptr;         // the viewpoints as uploaded
    int64_t vp_cap = 0;          // floats
    int64_t* sums = nullptr;     // the k search's moments, 10 per point: the nine sums and the bound's bits; grown on
    int64_t sums_cap = 0;        //   their own (points): the radius search keeps them in registers
    int64_t* h_stats = nullptr;  // pinned, 6
    size_t h_stats_bytes = 0;
};

void normals_free(NormalsBuf& nb);
// the outputs sized for n points; vp_floats: the viewpoint floats the call uploads into nb.vp (0: none);
// with_sums: the call has a k
int normals_reserve(NormalsBuf& nb, int64_t n, int64_t vp_floats, bool with_sums);

// Enqueued, after normals_reserve(nb, n, .., k > 0): nb.normals / nb.curvature / nb.counts of the n points of d_pts
// (n x stride floats) and the six counts in nb.h_stats (valid after the stream is waited for).  k = 0: the
// radius search alone; radius = 0: the k nearest alone.  d_vp: null, or the viewpoints on the device
// (vp_stride 0: one of 3 floats; 3..8: one row per point).
int estimate_normals(DenoiseBuf& b, NormalsBuf& nb, const float* d_pts, int64_t n, int stride, float radius, int k,
                     const float* d_vp, int vp_stride, hipStream_t st);

}  // namespace lio
