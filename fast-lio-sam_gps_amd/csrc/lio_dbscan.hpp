// lio_dbscan.hpp — DBSCAN with core flags and per-cluster bounding boxes (lio_dbscan.hip): the second clustering
// method of the offline pipeline (post_process/clustering.py:30-36, cluster_with_dbscan), scikit-learn's DBSCAN
// restated as sets (include/lio_gpu.h, lio_dbscan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lio_cluster.hpp"

namespace lio {

struct DbscanCounts {
    int64_t finite = 0, core = 0, clusters = 0, clustered_points = 0;
};

// DBSCAN of the n records at d_pts (device; x, y, z first).  It runs in the arenas of the Euclidean path (b: the
// grid, the sort and the scan; c: parents, run tables and results) and allocates nothing of its own.  Results on
// the device: c.labels (n), the core flags as n bytes at c.rank_of, c.indices (the clustered points in cluster
// order), and for the first min(clusters, cap_clusters) clusters c.offsets (+ 1 entry) and c.aabb; the counts on
// the host.  Waits for the stream once (the cluster count); the results are complete when the stream has drained.
// Status (lio_scratch.hpp): kOk, kArg bad arguments, kHip (text in last_error()), kNoMem.
int dbscan(DenoiseBuf& b, ClusterBuf& c, const float* d_pts, int64_t n, int stride, float eps, int64_t min_samples,
           int64_t cap_clusters, DbscanCounts* counts, hipStream_t st);

}  // namespace lio
