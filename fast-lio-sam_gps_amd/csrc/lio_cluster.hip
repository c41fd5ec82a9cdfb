// lio_cluster.hip — Euclidean cluster extraction on gfx950: pcl::EuclideanClusterExtraction<PointT>::extract
// [U] (fast_lio_sam.cpp:343-363) with the axis-aligned bounding box per cluster of the offline pipeline
// (post_process/clustering.py:39-75), as set operations:
//
//   edge       finite points i != j with float sqdist3 < r2, r2 = (float)((double)tolerance * tolerance), strict
//   cluster    a connected component of that graph with min_size <= size <= max_size
//   order      size descending, then lowest member index ascending; indices ascending inside a cluster
//
// Launch sequence (every step its own launch; no kernel waits for another workgroup):
//   grid (dn_build_grid, cell edge about the tolerance) -> parent[i] = i -> union (lock-free union-find,
//   the hot kernel) -> flatten (root per point) -> stable radix sort of (root, index) by root -> run heads,
//   scan -> runs -> one 64-bit sort of the runs by (~size, root) -> ranks, scan of the accepted sizes ->
//   labels and grouped indices -> offsets, bounding boxes.
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
#include "lio_cluster_dev.hpp"  // ld_parent / uf_find / uf_unite, the run kernels (shared with lio_dbscan.hip)

namespace lio {

namespace {

__global__ void cl_init_kernel(uint32_t* __restrict__ parent, int64_t n) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
}

// ---- the union kernel -------------------------------------------------------------------------------
// One thread per finite point, in cell order (position j of pts); it tests the points of LOWER position in
// the cells from cell_coord(p - (r + m)) to cell_coord(p + (r + m)) per axis, m = 1e-5 r + 1e-6 |p|, so every
// pair is tested once, by its later point.
//
// NO PAIR IS MISSED, whatever the cell size (the cell cap may have grown the edge far above the tolerance,
// and the assignment is rounded, so "the 27 cells around mine" is not the argument).  A point s with float
// sqdist3(p, s) < r2 has |p.x - s.x| <= r (1 + 3e-7) (the roundings of the difference, the squares and r2),
// so the float p.x - (r + m) is <= s.x <= the float p.x + (r + m); cell_coord is monotone (non-decreasing:
// float subtraction of a constant, multiplication by a positive constant, floor, clamp), so s's cell
// coordinate lies inside the scanned range on every axis (Kernel B of lio_denoise.hip rests on the same rule).
//
// COST.  The cell edge is 1.001 r, so r + m <= the edge while |p| <= 990 r: the range is 3 cells per axis
// then (the points below and above p by at most one edge), and since positions below j lie in cells of linear
// index <= mine, only the rows up to my own (cz, cy) are visited: 5 rows of 3 cells.
//
// Pairs that are already in one set skip the union: the thread keeps `ra`, a node of its own tree that was
// the root when last seen, and a neighbour whose parent is `ra` needs nothing.  At the end the thread's own
// parent is shortened to `ra` (atomicMin: never increases a parent).
__global__ void __launch_bounds__(256) cl_union_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ start,
                                                       const DnGeom* __restrict__ geom, int64_t n, float r, float r2,
                                                       uint32_t* parent) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    if (j >= (int64_t)start[g.ncells]) return;  // past the finite points
    const float4 q = pts[j];
    const uint32_t me = __float_as_uint(q.w);
    uint32_t ra = me;
    const float rx = r + (1e-5f * r + 1e-6f * fabsf(q.x)), ry = r + (1e-5f * r + 1e-6f * fabsf(q.y)),
                rz = r + (1e-5f * r + 1e-6f * fabsf(q.z));
    // my own cell, as the grid build assigned it (the same float expression on the same values)
    const int my = min(max(cell_coord(q.y, g.oy, g.inv), 0), g.ny - 1), mz = min(max(cell_coord(q.z, g.oz, g.inv), 0), g.nz - 1);
    const int x0 = max(cell_coord(q.x - rx, g.ox, g.inv), 0), x1 = min(cell_coord(q.x + rx, g.ox, g.inv), g.nx - 1);
    const int y0 = max(cell_coord(q.y - ry, g.oy, g.inv), 0), y1 = min(cell_coord(q.y + ry, g.oy, g.inv), g.ny - 1);
    const int z0 = max(cell_coord(q.z - rz, g.oz, g.inv), 0), z1 = min(min(cell_coord(q.z + rz, g.oz, g.inv), g.nz - 1), mz);
    if (x0 <= x1)
        for (int cz = z0; cz <= z1; ++cz) {
            const int ye = cz == mz ? min(y1, my) : y1;  // rows behind my own hold later positions only
            for (int cy = y0; cy <= ye; ++cy) {
                const uint32_t base = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx;
                const uint32_t e = min(start[base + (uint32_t)x1 + 1u], (uint32_t)j);
                uint32_t k = start[base + (uint32_t)x0];
                // four candidates at a time: their loads, and the parent loads of those within the radius, are in
                // flight together (one dependent load per candidate otherwise).  A union inside the batch changes
                // `ra`, so a later hit of the batch may call uf_unite for a pair already in one set: it returns
                // the root and changes nothing.
                for (; k + 4u <= e; k += 4u) {
                    float4 s[4];
                    uint32_t par[4];
                    bool hit[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) s[u] = pts[k + (uint32_t)u];
#pragma unroll
                    for (int u = 0; u < 4; ++u) hit[u] = sqdist3(q.x, q.y, q.z, s[u].x, s[u].y, s[u].z) < r2;
#pragma unroll
                    for (int u = 0; u < 4; ++u) par[u] = hit[u] ? ld_parent(parent, __float_as_uint(s[u].w)) : ra;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (hit[u] && par[u] != ra) ra = uf_unite(parent, ra, __float_as_uint(s[u].w));
                }
                for (; k < e; ++k) {
                    const float4 s = pts[k];
                    if (sqdist3(q.x, q.y, q.z, s.x, s.y, s.z) < r2) {  // FLANN's radius set keeps dist < radius [U]
                        const uint32_t other = __float_as_uint(s.w);
                        if (ld_parent(parent, other) != ra) ra = uf_unite(parent, ra, other);
                    }
                }
            }
        }
    if (ra != me) atomicMin(parent + me, ra);
}

// root per point (the forest is final: a launch of its own), n for a non-finite point: the sort leaves them last
__global__ void cl_flatten_kernel(const float* __restrict__ p, int64_t n, int stride, const uint32_t* __restrict__ parent,
                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = p + (size_t)i * stride;
    uint32_t k = (uint32_t)n;
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) {
        uint32_t x = (uint32_t)i;
        for (uint32_t up = parent[x]; up != x; up = parent[x]) x = up;  // strictly decreasing
        k = x;
    }
    keys[i] = k;
    vals[i] = (uint32_t)i;
}

// run heads and the run table: cl_heads_kernel / cl_runs_kernel of lio_cluster_dev.hpp (here a run is a component,
// its key the root, and cnt[0] the finite points)

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
// member at position j of run `run` is member j - run_start[run] of its cluster
__global__ void cl_label_kernel(const uint32_t* __restrict__ svals, const uint32_t* __restrict__ run_of, int64_t n,
                                const uint32_t* __restrict__ run_start, const int32_t* __restrict__ rank_of,
                                const uint32_t* __restrict__ off, int32_t* __restrict__ labels,
                                int32_t* __restrict__ indices) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = svals[j], run = run_of[j];
    int32_t lab = -1;
    if (run != kNoRun) {
        lab = rank_of[run];
        if (lab >= 0) indices[off[lab] + ((uint32_t)j - run_start[run])] = (int32_t)i;
    }
    labels[i] = lab;
}

// offsets: cl_offsets_kernel of lio_cluster_dev.hpp

// one wave per cluster: float min / max of x, y, z over its members (order-independent)
__global__ void __launch_bounds__(256) cl_aabb_kernel(const float* __restrict__ p, int stride,
                                                      const int32_t* __restrict__ indices, const uint32_t* __restrict__ off,
                                                      int64_t m, float* __restrict__ aabb) {
    const int lane = threadIdx.x & 63;
    const int64_t t = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
    if (t >= m) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const uint32_t e = off[t + 1];
    for (uint32_t k = off[t] + (uint32_t)lane; k < e; k += 64u) {
        const float* q = p + (size_t)indices[k] * stride;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], q[d]);
            hi[d] = fmaxf(hi[d], q[d]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], o, 64));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o, 64));
        }
    if (lane == 0)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            aabb[t * 6 + d] = lo[d];
            aabb[t * 6 + 3 + d] = hi[d];
        }
}

}  // namespace

int cluster_reserve(ClusterBuf& c, int64_t n) {
    if (n <= c.cap && c.arena) return kOk;
    const int64_t cap = std::min<int64_t>(grown<int64_t>(n, c.cap, 4096), 0x7fffff00);
    dev_free(&c.arena);
    c.cap = 0;
    const size_t C = (size_t)cap;
    auto carve = [&](Carver at) {  // the arena's fields, once each, in arena order
        at(c.parent, C), at(c.run_of, C), at(c.run_start, C + 1), at(c.rank_of, C);
        at(c.labels, C), at(c.indices, C), at(c.offsets, C + 1), at(c.aabb, 6 * C), at(c.cnt, 16);
        return at.bytes();
    };
    const size_t total = carve(Carver{});
    count_alloc();
    if (hipMalloc(&c.arena, total) != hipSuccess) {
        c.arena = nullptr;
        return kNoMem;
    }
    carve(Carver{c.arena});
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
    if (stride < 3 || stride > 8 || !(tolerance > 0.f) || !std::isfinite(tolerance) || min_size < 1 || cap_clusters < 0)
        return kArg;
    int rc = denoise_reserve(b, n);
    if (!rc) rc = cluster_reserve(c, n);
    if (rc) return rc;
    const float r2 = (float)((double)tolerance * (double)tolerance);  // PCL passes the tolerance, FLANN squares it [U]
    LIO_HIP(hipMemsetAsync(c.cnt, 0, 64, st));
    if ((rc = dn_build_grid(b, d_pts, n, stride, 0.f, tolerance * 1.001f, st))) return rc;
    cl_init_kernel<<<nblk(n), 256, 0, st>>>(c.parent, n);
    cl_union_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, tolerance, r2, c.parent);
    cl_flatten_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, stride, c.parent, b.keys, b.vals);
    if ((rc = dn_sort32(b, n, dn_bit_width((uint32_t)n), st))) return rc;  // keys in [0, n]
    cl_heads_kernel<<<nblk(n + 1), 256, 0, st>>>(b.keys_alt, n, b.flags, c.cnt);
    int64_t ncomp = 0, npts = 0;
    if ((rc = dn_scan_count(b, n, &ncomp, st))) return rc;
    cl_runs_kernel<<<nblk(n), 256, 0, st>>>(b.flags, b.pos, n, c.cnt, c.run_of, c.run_start);
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
    cl_label_kernel<<<nblk(n), 256, 0, st>>>(b.vals_alt, c.run_of, n, c.run_start, c.rank_of, b.pos, c.labels, c.indices);
    const int64_t m = std::min(counts->clusters, cap_clusters);
    cl_offsets_kernel<<<nblk(m + 1), 256, 0, st>>>(b.pos, m, c.offsets);
    if (m > 0) cl_aabb_kernel<<<(unsigned)((m + 3) / 4), 256, 0, st>>>(d_pts, stride, c.indices, b.pos, m, c.aabb);
    LIO_HIP(hipGetLastError());
    return 0;
}

}  // namespace lio
