// lio_cluster.hpp — Euclidean cluster extraction with per-cluster bounding boxes (lio_cluster.hip):
// pcl::EuclideanClusterExtraction<PointT>::extract [U] as connected components of the radius graph
// (fast_lio_sam.cpp:343-363, post_process/clustering.py:39-75).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_denoise.hpp"

namespace lio {

// Scratch of the clustering beside the DenoiseBuf it shares the grid, the sorts and the scan with: ONE device
// arena sized for `cap` points, grown geometrically (counted: lio_alloc_count).  60 bytes per point.
struct ClusterBuf {
    void* arena = nullptr;
    size_t arena_bytes = 0;
    int64_t cap = 0;
    uint32_t* parent = nullptr;     // union-find over input indices
    uint32_t* run_of = nullptr;     // per position of the root-sorted order: its component (run) number
    uint32_t* run_start = nullptr;  // cap + 1: first position of every run, then the number of finite points
    int32_t* rank_of = nullptr;     // per run: its cluster rank, -1 when rejected
    int32_t* labels = nullptr;      // results, as lio_euclidean_clusters returns them
    int32_t* indices = nullptr;
    int64_t* offsets = nullptr;     // cap + 1
    float* aabb = nullptr;          // 6 cap
    uint32_t* cnt = nullptr;        // 16 words: [0] finite points, [1] accepted clusters
};

struct ClusterCounts {
    int64_t finite = 0, components = 0, clusters = 0, clustered_points = 0;
};

void cluster_free(ClusterBuf& c);
// every buffer sized for n points (lio_dbscan.hip shares the arena: parents, run tables, labels, indices, offsets,
// boxes; `rank_of` holds its core flags per input point)
int cluster_reserve(ClusterBuf& c, int64_t n);
// Clusters of the n records at d_pts (device; x, y, z first).  Results on the device in c.labels (n), c.indices
// (the accepted points in cluster order), and for the first min(clusters, cap_clusters) clusters c.offsets
// (+ 1 entry) and c.aabb; the counts on the host.  Waits for the stream twice (the component count, then the
// cluster count: two words each); the results are complete when the stream has drained.
// Status (lio_scratch.hpp): kOk, kArg bad arguments, kHip (text in last_error()), kNoMem.
int euclidean_clusters(DenoiseBuf& b, ClusterBuf& c, const float* d_pts, int64_t n, int stride, float tolerance,
                       int64_t min_size, int64_t max_size, int64_t cap_clusters, ClusterCounts* counts, hipStream_t st);

}  // namespace lio
