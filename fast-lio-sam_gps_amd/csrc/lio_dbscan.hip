// lio_dbscan.hip — DBSCAN on gfx950 with one core flag per point and one axis-aligned bounding box per cluster:
// cluster_with_dbscan of the offline pipeline (post_process/clustering.py:30-36), scikit-learn's DBSCAN [U]
// restated as set operations (this library's contract, include/lio_gpu.h):
//
//   neighbour  finite points i and j (j = i included) with float sqdist3 <= e2, e2 = (float)((double)eps * eps),
//              INCLUSIVE (DBSCAN's definition; the PCL-derived entries test strictly)
//   core       a finite point with >= min_samples neighbours, itself counted
//   cluster    a connected component of the neighbour graph restricted to core points, numbered by its lowest
//              core index, ascending
//   border     a finite non-core point with a core neighbour: it takes the lowest-numbered cluster among its core
//              neighbours' clusters and spreads nothing
//   noise      every other point, the non-finite ones among them: label -1
//
// Launch sequence (every step its own launch; the pieces named cl_* in brackets are lio_cluster_dev.hpp's, shared
// with lio_cluster.hip; every pass over neighbours walks the rows of cell_box, lio_radius_dev.hpp):
//   [cl_open: grid (dn_build_grid, cell edge 1.001 eps)] -> core pass (neighbour count, stopped at min_samples) ->
//   parent[i] = i, the core bit into the gridded points -> [cl_union_kernel<true>: the lock-free union-find, by
//   core points over core candidates, inclusive] -> key pass (a core point's key is its root, a border point's the
//   lowest root among its core neighbours, n for noise) -> [cl_sorted_runs: stable radix sort of (key, index) by
//   key -> run heads, scan (the cluster count crosses to the host) -> runs] -> labels and grouped indices ->
//   [cl_offsets_boxes: offsets, bounding boxes by chunks of positions].
// The sorted runs ARE the clusters in label order (the key of a cluster is its lowest core index), and indices
// ascend inside a run (the sort is stable from ascending indices), so no second sort is needed.  Sizes are run
// lengths; the only atomic counter is the number of core points of the whole call, one add per wave.  The boxes
// are integer atomic min / max from one wave per stretch of the sorted order: order-independent.
//
// NO KERNEL WAITS FOR ANOTHER WORKGROUP.  The core pass, the key pass and everything of the tail read what
// earlier launches wrote and write one slot per thread.  The core union's loops are those of lio_cluster.hip: a
// root is only ever hooked under a SMALLER index (CAS on parent[root]) and the shortening writes smaller values
// too (atomicMin), so parent[x] <= x always and never increases; a chase from x ends within x steps, a failed CAS
// has seen a strictly smaller parent, so every retry loop is bounded by the index it started from.  The key pass
// runs after the union kernel has ended: the forest is final, and its chases are plain bounded descents.
//
// DETERMINISM.  When the core union has ended, the trees are the components of the core graph whatever the
// schedule, and the root of each is its lowest core index: the cluster's number key.  A border point's key is a
// minimum over a set that does not depend on the schedule.  Everything after is a stable sort, scans and
// min / max.
#include <algorithm>
#include <cmath>

#include "lio_dev.hpp"
#include "lio_scratch.hpp"
#include "lio_dbscan.hpp"
#include "lio_cluster_dev.hpp"

namespace lio {

namespace {

// ---- the core pass ----------------------------------------------------------------------------------
// One thread per finite point, in cell order (position j of pts).  It counts the neighbours in the full cell
// range, itself among them, and STOPS AT `need` = min_samples: on dense ground a point has hundreds of neighbours
// and the answer is known after the first few.  Candidates are taken four at a time, their loads in flight
// together.  flags[j] (position order) and core[input index] = 1 for a core point.
__global__ void __launch_bounds__(256) db_core_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ start,
                                                      const DnGeom* __restrict__ geom, int64_t n, float r, float e2,
                                                      uint32_t need, uint32_t* __restrict__ flags,
                                                      uint8_t* __restrict__ core) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    if (j >= (int64_t)start[g.ncells]) return;  // past the finite points
    const float4 q = pts[j];
    uint32_t cnt = 0;
    const auto b = cell_box<false>(g, q.x, q.y, q.z, r);
    for (int cz = b.z0; cz <= b.z1 && cnt < need; ++cz)
        for (int cy = b.y0; cy <= b.y_last(cz) && cnt < need; ++cy) {
            uint32_t k, e;
            b.row(g, start, cz, cy, k, e);
            for (; k + 4u <= e && cnt < need; k += 4u) {
                float4 s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = pts[k + (uint32_t)u];
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt += sqdist3(q.x, q.y, q.z, s[u].x, s[u].y, s[u].z) <= e2 ? 1u : 0u;
            }
            for (; k < e && cnt < need; ++k) {
                const float4 s = pts[k];
                cnt += sqdist3(q.x, q.y, q.z, s.x, s.y, s.z) <= e2 ? 1u : 0u;  // inclusive: radius_neighbors [U]
            }
        }
    const uint32_t f = cnt >= need ? 1u : 0u;
    flags[j] = f;
    core[__float_as_uint(q.w)] = (uint8_t)f;
}

// parent[i] = i and the sort's (key, value) pairs preset to (n, i): what no later thread writes is noise.  The
// core flag of position i goes into bit 31 of that point's index word, where the candidate tests of the next two
// passes find it in the load they make anyway.  cnt[2] += core points (one add per wave), cnt[3] = finite points.
__global__ void __launch_bounds__(256) db_init_kernel(float4* pts, const uint32_t* __restrict__ start,
                                                      const DnGeom* __restrict__ geom, const uint32_t* __restrict__ flags,
                                                      int64_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals, uint32_t* cnt) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool is_core = false;
    if (i < n) {
        parent[i] = (uint32_t)i;
        keys[i] = (uint32_t)n;
        vals[i] = (uint32_t)i;
        const uint32_t nf = start[geom->ncells];
        if (i < (int64_t)nf && flags[i]) {
            is_core = true;
            uint32_t* w = reinterpret_cast<uint32_t*>(pts + i) + 3;
            *w |= kCoreBit;
        }
        if (i == 0) cnt[3] = nf;
    }
    const unsigned long long m = __ballot(is_core);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(cnt + 2, (uint32_t)__popcll(m));
}

// ---- the key pass (the forest is final: a launch of its own) -------------------------------------------
// One thread per finite point in cell order.  A core point's key is its root.  A non-core point scans its full
// cell range for core neighbours and takes the lowest of their roots (it has fewer than min_samples neighbours,
// so fewer chases than that); without one it keeps the preset key n: noise.  keys[] is indexed by input index.
__global__ void __launch_bounds__(256) db_key_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ start,
                                                     const DnGeom* __restrict__ geom, int64_t n, float r, float e2,
                                                     const uint32_t* __restrict__ parent, uint32_t* __restrict__ keys) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    if (j >= (int64_t)start[g.ncells]) return;  // past the finite points
    const float4 q = pts[j];
    const uint32_t w = __float_as_uint(q.w), me = w & ~kCoreBit;
    if (w & kCoreBit) {
        keys[me] = uf_root(parent, me);
        return;
    }
    uint32_t key = (uint32_t)n;
    const auto b = cell_box<false>(g, q.x, q.y, q.z, r);
    for (int cz = b.z0; cz <= b.z1; ++cz)
        for (int cy = b.y0; cy <= b.y_last(cz); ++cy) {
            uint32_t k, e;
            b.row(g, start, cz, cy, k, e);
            for (; k + 4u <= e; k += 4u) {
                float4 s[4];
                uint32_t par[4];
                bool hit[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = pts[k + (uint32_t)u];
#pragma unroll
                for (int u = 0; u < 4; ++u) hit[u] = radius_hit<true>(q, s[u], e2);
#pragma unroll
                for (int u = 0; u < 4; ++u) par[u] = hit[u] ? parent[index_of<true>(s[u])] : key;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (hit[u]) key = min(key, uf_root(parent, par[u]));
            }
            for (; k < e; ++k) {
                const float4 s = pts[k];
                if (radius_hit<true>(q, s, e2)) key = min(key, uf_root(parent, index_of<true>(s)));
            }
        }
    keys[me] = key;
}

// positions in key order: run r is cluster r, and its members stand at their final places already
__global__ void db_label_kernel(const uint32_t* __restrict__ svals, const uint32_t* __restrict__ run_of, int64_t n,
                                int32_t* __restrict__ labels, int32_t* __restrict__ indices) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = svals[j], run = run_of[j];
    if (run != kNoRun) indices[j] = (int32_t)i;
    labels[i] = run != kNoRun ? (int32_t)run : -1;
}

}  // namespace

int dbscan(DenoiseBuf& b, ClusterBuf& c, const float* d_pts, int64_t n, int stride, float eps, int64_t min_samples,
           int64_t cap_clusters, DbscanCounts* counts, hipStream_t st) {
    *counts = DbscanCounts{};
    if (n <= 0) return 0;
    int rc = cl_open(b, c, d_pts, n, stride, eps, min_samples, cap_clusters, st);
    if (rc) return rc;
    const float e2 = (float)((double)eps * (double)eps);
    // no point has 2^31 neighbours: a larger min_samples means "no core point" all the same
    const uint32_t need = (uint32_t)std::min<int64_t>(min_samples, (int64_t)1 << 31);
    uint8_t* core = reinterpret_cast<uint8_t*>(c.rank_of);  // n bytes of the 4 n that the Euclidean path's ranks take
    LIO_HIP(hipMemsetAsync(core, 0, (size_t)n, st));        // a non-finite point is not core
    LIO_HIP(hipMemsetAsync(c.run_start, 0, sizeof(uint32_t), st));  // the first offset, when there is no cluster
    db_core_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, eps, e2, need, b.flags, core);
    db_init_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, b.flags, n, c.parent, b.keys, b.vals, c.cnt);
    cl_union_kernel<true><<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, eps, e2, c.parent);
    db_key_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, eps, e2, c.parent, b.keys);
    int64_t nclusters = 0;  // a run is a cluster, and cnt[0] the clustered points
    if ((rc = cl_sorted_runs(b, c, n, 4, &nclusters, st))) return rc;
    counts->clustered_points = b.h_cnt[2];
    counts->core = b.h_cnt[4];
    counts->finite = b.h_cnt[5];
    counts->clusters = nclusters;
    db_label_kernel<<<nblk(n), 256, 0, st>>>(b.vals_alt, c.run_of, n, c.labels, c.indices);
    return cl_offsets_boxes(c, d_pts, stride, c.run_start, c.run_of, counts->clustered_points,
                            std::min(nclusters, cap_clusters), st);
}

}  // namespace lio
