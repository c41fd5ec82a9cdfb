// lio_cluster.hip — Euclidean cluster extraction on gfx950: pcl::EuclideanClusterExtraction<PointT>::extract
// [U] (fast_lio_sam.cpp:343-363) with the axis-aligned bounding box per cluster of the offline pipeline
// (post_process/clustering.py:39-75), as set operations:
//
//   edge       finite points i != j with float sqdist3 < r2, r2 = (float)((double)tolerance * tolerance), strict
//   cluster    a connected component of that graph with min_size <= size <= max_size
//   order      size descending, then lowest member index ascending; indices ascending inside a cluster
//
// Launch sequence (every step its own launch; no kernel waits for another workgroup; the pieces named cl_* in
// brackets are lio_cluster_dev.hpp's, shared with lio_dbscan.hip):
//   [cl_open: grid (dn_build_grid, cell edge about the tolerance)] -> parent[i] = i -> [cl_union_kernel<false>:
//   lock-free union-find, the hot kernel] -> flatten (root per point) -> [cl_sorted_runs: stable radix sort of
//   (root, index) by root -> run heads, scan -> runs] -> one 64-bit sort of the runs by (~size, root) -> ranks,
//   scan of the accepted sizes -> labels, grouped indices and the cluster per position of them ->
//   [cl_offsets_boxes: offsets, bounding boxes by chunks of positions].
//
// DETERMINISM.  A root is only ever hooked under a SMALLER input index (CAS on parent[root]), and the path
// shortening writes only smaller values too (atomicMin), so parent[x] <= x always and never increases: no
// cycle can form, every pointer chase ends after at most x steps, and every failed CAS has seen a strictly
// smaller parent, so every retry loop is bounded by the index it started from.  Each tree has exactly one
// root (a hook needs parent[hi] == hi, and the node it is hooked under lies in another tree: its root is
// <= lo < hi), and that root is the tree's lowest index.  When the union kernel has ended, the trees are the
// components, whatever the schedule; the root of a component is its lowest input index, which is also the
// key that orders clusters of equal size.  Everything after is sorts, scans and min / max.
#include <algorithm>
#include <cmath>

#include "lio_dev.hpp"
#include "lio_scratch.hpp"
#include "lio_cluster.hpp"
#include "lio_cluster_dev.hpp"  // the union-find and union kernel, the run and box kernels, the host sequences

namespace lio {

namespace {

__global__ void cl_init_kernel(uint32_t* __restrict__ parent, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
}

// root per point (the forest is final: a launch of its own), n for a non-finite point: the sort leaves them last
__global__ void cl_flatten_kernel(const float* __restrict__ p, int64_t n, int stride, const uint32_t* __restrict__ parent,
                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = p + (size_t)i * stride;
    uint32_t k = (uint32_t)n;
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) k = uf_root(parent, (uint32_t)i);
    keys[i] = k;
    vals[i] = (uint32_t)i;
}

// the sort key of a run: (~size, root) — ascending = size descending, then lowest member ascending; a run
// outside [min_size, max_size] gets the high word 0xffffffff (no size is 0) and sorts behind every accepted one
__global__ void cl_runkey_kernel(const uint32_t* __restrict__ run_start, const uint32_t* __restrict__ skeys, int64_t ncomp,
                                 int64_t min_size, int64_t max_size, uint64_t* __restrict__ k64, uint32_t* __restrict__ idx) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= ncomp) return;
    const uint32_t s = run_start[r], size = run_start[r + 1] - s;
    const bool ok = (int64_t)size >= min_size && (int64_t)size <= max_size;
    k64[r] = ((uint64_t)(ok ? ~size : 0xffffffffu) << 32) | skeys[s];
    idx[r] = (uint32_t)r;
}

// after the sort: rank t holds run idxs[t].  flags[t] = its size when accepted, else 0 (flags[ncomp] = 0): the
// scan gives the offsets; cnt[1] = accepted clusters (zeroed before)
__global__ void cl_rank_kernel(const uint64_t* __restrict__ k64s, const uint32_t* __restrict__ idxs, int64_t ncomp,
                               int32_t* __restrict__ rank_of, uint32_t* __restrict__ flags, uint32_t* __restrict__ cnt) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t > ncomp) return;
    uint32_t size = 0;
    if (t < ncomp) {
        const uint32_t hi = (uint32_t)(k64s[t] >> 32);
        const bool ok = hi != 0xffffffffu;
        if (ok) {
            size = ~hi;
            if (t + 1 == ncomp || (uint32_t)(k64s[t + 1] >> 32) == 0xffffffffu) cnt[1] = (uint32_t)(t + 1);
        }
        rank_of[idxs[t]] = ok ? (int32_t)t : -1;
    }
    flags[t] = size;
}

// positions in root order: indices ascend inside a run (the sort is stable from ascending indices), so the
// member at position j of run `run` is member j - run_start[run] of its cluster; cluster_of[] = the cluster per
// position of indices[] (rank order, which run_of's root order is not): what the box kernel walks
__global__ void cl_label_kernel(const uint32_t* __restrict__ svals, const uint32_t* __restrict__ run_of, int64_t n,
                                const uint32_t* __restrict__ run_start, const int32_t* __restrict__ rank_of,
                                const uint32_t* __restrict__ off, int32_t* __restrict__ labels,
                                int32_t* __restrict__ indices, uint32_t* __restrict__ cluster_of) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = svals[j], run = run_of[j];
    int32_t lab = -1;
    if (run != kNoRun) {
        lab = rank_of[run];
        if (lab >= 0) {
            const uint32_t at = off[lab] + ((uint32_t)j - run_start[run]);
            indices[at] = (int32_t)i;
            cluster_of[at] = (uint32_t)lab;
        }
    }
    labels[i] = lab;
}

}  // namespace

int cluster_reserve(ClusterBuf& c, int64_t n) {
    if (n <= c.cap && c.arena) return kOk;
    const int64_t cap = std::min<int64_t>(grown<int64_t>(n, c.cap, 4096), 0x7fffff00);
    dev_free(&c.arena);
    c.arena_bytes = 0, c.cap = 0;
    const size_t C = (size_t)cap;
    auto fields = [&](Carver& at) {  // the arena's fields, once each, in arena order
        at(c.parent, C), at(c.run_of, C), at(c.run_start, C + 1), at(c.rank_of, C);
        at(c.labels, C), at(c.indices, C), at(c.offsets, C + 1), at(c.aabb, 6 * C), at(c.cnt, 16);
    };
    const int rc = reserve_arena(&c.arena, c.arena_bytes, fields, 0);
    if (rc) return rc;
    c.cap = cap;
    return kOk;
}

void cluster_free(ClusterBuf& c) {
    dev_free(&c.arena);
    c = ClusterBuf{};
}

int euclidean_clusters(DenoiseBuf& b, ClusterBuf& c, const float* d_pts, int64_t n, int stride, float tolerance,
                       int64_t min_size, int64_t max_size, int64_t cap_clusters, ClusterCounts* counts, hipStream_t st) {
    *counts = ClusterCounts{};
    if (n <= 0) return 0;
    int rc = cl_open(b, c, d_pts, n, stride, tolerance, min_size, cap_clusters, st);
    if (rc) return rc;
    const float r2 = (float)((double)tolerance * (double)tolerance);  // PCL passes the tolerance, FLANN squares it [U]
    cl_init_kernel<<<nblk(n), 256, 0, st>>>(c.parent, n);
    cl_union_kernel<false><<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, tolerance, r2, c.parent);
    cl_flatten_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, stride, c.parent, b.keys, b.vals);
    int64_t ncomp = 0, npts = 0;  // a run is a component, its key the root, and cnt[0] the finite points
    if ((rc = cl_sorted_runs(b, c, n, 0, &ncomp, st))) return rc;
    if (ncomp > 0) {
        cl_runkey_kernel<<<nblk(ncomp), 256, 0, st>>>(c.run_start, b.keys_alt, ncomp, min_size, max_size, b.k64, b.idx);
        if ((rc = dn_sort64(b, ncomp, 64, st))) return rc;
        cl_rank_kernel<<<nblk(ncomp + 1), 256, 0, st>>>(b.k64_alt, b.idx_alt, ncomp, c.rank_of, b.flags, c.cnt);
    }
    LIO_HIP(hipMemcpyAsync(b.h_cnt + 2, c.cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (ncomp > 0) {
        if ((rc = dn_scan_count(b, ncomp, &npts, st))) return rc;  // b.pos[t] = offset of cluster t
    } else {
        LIO_HIP(hipStreamSynchronize(st));  // b.pos[0] = 0 from the first scan
    }
    counts->finite = b.h_cnt[2];
    counts->components = ncomp;
    counts->clusters = b.h_cnt[3];
    counts->clustered_points = npts;
    // b.keys, the first sort's input, is spent (both sorts write their _alt buffers only): the cluster per position
    uint32_t* cluster_of = b.keys;
    cl_label_kernel<<<nblk(n), 256, 0, st>>>(b.vals_alt, c.run_of, n, c.run_start, c.rank_of, b.pos, c.labels, c.indices,
                                             cluster_of);
    return cl_offsets_boxes(c, d_pts, stride, b.pos, cluster_of, npts, std::min(counts->clusters, cap_clusters), st);
}

}  // namespace lio
