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
// Launch sequence (every step its own launch):
//   grid (dn_build_grid, cell edge 1.001 eps) -> core pass (neighbour count, stopped at min_samples) ->
//   parent[i] = i, the core bit into the gridded points -> core union (the lock-free union-find of
//   lio_cluster_dev.hpp, by core points over core candidates) -> key pass (a core point's key is its root, a
//   border point's the lowest root among its core neighbours, n for noise) -> stable radix sort of (key, index)
//   by key -> run heads, scan (the cluster count crosses to the host) -> runs -> labels and grouped indices ->
//   offsets, bounding boxes.
// The sorted runs ARE the clusters in label order (the key of a cluster is its lowest core index), and indices
// ascend inside a run (the sort is stable from ascending indices), so no second sort is needed.  Sizes are run
// lengths; the only atomic counter is the number of core points of the whole call, one add per wave.  The boxes
// are integer atomic min / max from one wave per stretch of the sorted order (below): order-independent.
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

constexpr uint32_t kCoreBit = 0x80000000u;  // n < 2^31: bit 31 of the index word of a gridded point is free

// The cells a point's neighbours can lie in: cell_coord(p -+ (r + m)) per axis, m = 1e-5 r + 1e-6 |p|.
//
// NO NEIGHBOUR IS MISSED, whatever the cell size, with the inclusive test as with the strict one.  A point s with
// float sqdist3(p, s) <= e2 has float dx * dx <= e2 (the other squares are >= 0 and float addition is monotone),
// so |p.x - s.x| <= r (1 + 3e-7) (the roundings of the difference, the square and e2: the bound never used that
// the comparison was strict), so the float p.x - (r + m) is <= s.x <= the float p.x + (r + m); cell_coord is
// monotone (non-decreasing: float subtraction of a constant, multiplication by a positive constant, floor,
// clamp), so s's cell coordinate lies inside the range on every axis (lio_cluster.hip's union kernel and Kernel
// B of lio_denoise.hip rest on the same rule).  With the edge at 1.001 r the range is 3 cells per axis while
// |p| <= 990 r.
struct CellBox {
    int x0, x1, y0, y1, z0, z1;
};

__device__ __forceinline__ CellBox db_box(const DnGeom& g, const float4& q, float r) {
    const float rx = r + (1e-5f * r + 1e-6f * fabsf(q.x)), ry = r + (1e-5f * r + 1e-6f * fabsf(q.y)),
                rz = r + (1e-5f * r + 1e-6f * fabsf(q.z));
    CellBox b;
    b.x0 = max(cell_coord(q.x - rx, g.ox, g.inv), 0), b.x1 = min(cell_coord(q.x + rx, g.ox, g.inv), g.nx - 1);
    b.y0 = max(cell_coord(q.y - ry, g.oy, g.inv), 0), b.y1 = min(cell_coord(q.y + ry, g.oy, g.inv), g.ny - 1);
    b.z0 = max(cell_coord(q.z - rz, g.oz, g.inv), 0), b.z1 = min(cell_coord(q.z + rz, g.oz, g.inv), g.nz - 1);
    return b;
}

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
    const CellBox b = db_box(g, q, r);
    uint32_t cnt = 0;
    if (b.x0 <= b.x1)
        for (int cz = b.z0; cz <= b.z1 && cnt < need; ++cz)
            for (int cy = b.y0; cy <= b.y1 && cnt < need; ++cy) {
                const uint32_t base = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx;
                const uint32_t e = start[base + (uint32_t)b.x1 + 1u];
                uint32_t k = start[base + (uint32_t)b.x0];
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

// ---- the core union ---------------------------------------------------------------------------------
// lio_cluster.hip's union kernel run by core points over core candidates with the inclusive test: one thread
// per core point in cell order; it tests the core points of LOWER position in its cell range (only the rows up
// to its own hold any), so every core pair is tested once, by its later point.  A hit whose parent is `ra`, the
// thread's last seen root, needs nothing; otherwise the larger root is hooked under the smaller by CAS.  At the
// end the thread's own parent is shortened to `ra` (atomicMin: never increases a parent).
__global__ void __launch_bounds__(256) db_union_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ start,
                                                       const DnGeom* __restrict__ geom, int64_t n, float r, float e2,
                                                       uint32_t* parent) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    if (j >= (int64_t)start[g.ncells]) return;  // past the finite points
    const float4 q = pts[j];
    const uint32_t w = __float_as_uint(q.w);
    if (!(w & kCoreBit)) return;
    const uint32_t me = w & ~kCoreBit;
    uint32_t ra = me;
    const CellBox b = db_box(g, q, r);
    // my own cell, as the grid build assigned it (the same float expression on the same values)
    const int my = min(max(cell_coord(q.y, g.oy, g.inv), 0), g.ny - 1), mz = min(max(cell_coord(q.z, g.oz, g.inv), 0), g.nz - 1);
    const int z1 = min(b.z1, mz);
    if (b.x0 <= b.x1)
        for (int cz = b.z0; cz <= z1; ++cz) {
            const int ye = cz == mz ? min(b.y1, my) : b.y1;  // rows behind my own hold later positions only
            for (int cy = b.y0; cy <= ye; ++cy) {
                const uint32_t base = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx;
                const uint32_t e = min(start[base + (uint32_t)b.x1 + 1u], (uint32_t)j);
                uint32_t k = start[base + (uint32_t)b.x0];
                // four candidates at a time: their loads, and the parent loads of the core points within the
                // radius, are in flight together.  A union inside the batch changes `ra`, so a later hit of the
                // batch may call uf_unite for a pair already in one set: it returns the root and changes nothing.
                for (; k + 4u <= e; k += 4u) {
                    float4 s[4];
                    uint32_t par[4];
                    bool hit[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) s[u] = pts[k + (uint32_t)u];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        hit[u] = (__float_as_uint(s[u].w) & kCoreBit) && sqdist3(q.x, q.y, q.z, s[u].x, s[u].y, s[u].z) <= e2;
#pragma unroll
                    for (int u = 0; u < 4; ++u) par[u] = hit[u] ? ld_parent(parent, __float_as_uint(s[u].w) & ~kCoreBit) : ra;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (hit[u] && par[u] != ra) ra = uf_unite(parent, ra, __float_as_uint(s[u].w) & ~kCoreBit);
                }
                for (; k < e; ++k) {
                    const float4 s = pts[k];
                    const uint32_t sw = __float_as_uint(s.w);
                    if ((sw & kCoreBit) && sqdist3(q.x, q.y, q.z, s.x, s.y, s.z) <= e2) {
                        const uint32_t other = sw & ~kCoreBit;
                        if (ld_parent(parent, other) != ra) ra = uf_unite(parent, ra, other);
                    }
                }
            }
        }
    if (ra != me) atomicMin(parent + me, ra);
}

// the root of x in the final forest: strictly decreasing, so at most x steps
__device__ __forceinline__ uint32_t db_root(const uint32_t* __restrict__ parent, uint32_t x) {
    for (uint32_t up = parent[x]; up != x; up = parent[x]) x = up;
    return x;
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
        keys[me] = db_root(parent, me);
        return;
    }
    uint32_t key = (uint32_t)n;
    const CellBox b = db_box(g, q, r);
    if (b.x0 <= b.x1)
        for (int cz = b.z0; cz <= b.z1; ++cz)
            for (int cy = b.y0; cy <= b.y1; ++cy) {
                const uint32_t base = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx;
                const uint32_t e = start[base + (uint32_t)b.x1 + 1u];
                uint32_t k = start[base + (uint32_t)b.x0];
                for (; k + 4u <= e; k += 4u) {
                    float4 s[4];
                    uint32_t par[4];
                    bool hit[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) s[u] = pts[k + (uint32_t)u];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        hit[u] = (__float_as_uint(s[u].w) & kCoreBit) && sqdist3(q.x, q.y, q.z, s[u].x, s[u].y, s[u].z) <= e2;
#pragma unroll
                    for (int u = 0; u < 4; ++u) par[u] = hit[u] ? parent[__float_as_uint(s[u].w) & ~kCoreBit] : key;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (hit[u]) key = min(key, db_root(parent, par[u]));
                }
                for (; k < e; ++k) {
                    const float4 s = pts[k];
                    const uint32_t sw = __float_as_uint(s.w);
                    if ((sw & kCoreBit) && sqdist3(q.x, q.y, q.z, s.x, s.y, s.z) <= e2)
                        key = min(key, db_root(parent, sw & ~kCoreBit));
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

// ---- bounding boxes -----------------------------------------------------------------------------------
// DBSCAN has no size filter, so one cluster may hold nearly every point (the ground with everything standing on
// it), and one wave per cluster — the Euclidean path's box kernel, whose clusters max_size bounds — would walk it
// alone.  Here one wave takes kBoxChunk consecutive positions of the key-sorted order, whatever clusters they
// belong to: it keeps the min / max of the run it is in in registers and hands them over with one atomic min /
// max per coordinate when the run changes and at its end.  Floats go through an order-preserving map to
// unsigned integers, so the atomics are integer ones and the result does not depend on their order.
constexpr int kBoxChunk = 1024;

__device__ __forceinline__ uint32_t ord_of(float v) {  // unsigned order = float order (-0 below +0); no NaN comes here
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ord_to(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

__global__ void db_box_init_kernel(uint32_t* __restrict__ box, int64_t m) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < 6 * m) box[t] = ord_of(t % 6 < 3 ? INFINITY : -INFINITY);
}

// the wave's min / max into box[run] (all lanes call it; lanes without a point hold +inf / -inf)
__device__ __forceinline__ void db_box_flush(uint32_t run, int64_t m, float (&lo)[3], float (&hi)[3], int lane,
                                             uint32_t* box) {
    if (run < (uint32_t)m) {  // wave-uniform; kNoRun and the runs past the capacity are dropped
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
                atomicMin(box + (size_t)run * 6 + d, ord_of(lo[d]));
                atomicMax(box + (size_t)run * 6 + 3 + d, ord_of(hi[d]));
            }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) lo[d] = INFINITY, hi[d] = -INFINITY;
}

__global__ void __launch_bounds__(256) db_box_kernel(const float* __restrict__ p, int stride,
                                                     const int32_t* __restrict__ indices, const uint32_t* __restrict__ run_of,
                                                     int64_t nin, int64_t m, uint32_t* box) {
    const int lane = threadIdx.x & 63;
    const int64_t begin = (blockIdx.x * (int64_t)4 + (threadIdx.x >> 6)) * kBoxChunk;
    if (begin >= nin) return;
    const int64_t end = min(begin + (int64_t)kBoxChunk, nin);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t cur = kNoRun;  // the run whose min / max the registers hold (wave-uniform)
    for (int64_t k = begin; k < end; k += 64) {
        const int64_t j = k + lane;
        const bool valid = j < end;
        const uint32_t run = valid ? run_of[j] : kNoRun;
        float v[3] = {0.f, 0.f, 0.f};
        if (valid) {
            const float* q = p + (size_t)indices[j] * stride;
            v[0] = q[0], v[1] = q[1], v[2] = q[2];
        }
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)run);  // lane 0 is valid: k < end
        const bool one_run = __all(!valid || run == first);
        if (!(one_run && first == cur)) db_box_flush(cur, m, lo, hi, lane, box);
        if (one_run) {
            cur = first;
            if (valid)
#pragma unroll
                for (int d = 0; d < 3; ++d) lo[d] = fminf(lo[d], v[d]), hi[d] = fmaxf(hi[d], v[d]);
        } else {  // a run ends inside these 64 positions: every point for itself
            cur = kNoRun;
            if (valid && run < (uint32_t)m)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    atomicMin(box + (size_t)run * 6 + d, ord_of(v[d]));
                    atomicMax(box + (size_t)run * 6 + 3 + d, ord_of(v[d]));
                }
        }
    }
    db_box_flush(cur, m, lo, hi, lane, box);
}

__global__ void db_box_decode_kernel(uint32_t* box, int64_t m) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < 6 * m) box[t] = __float_as_uint(ord_to(box[t]));
}

}  // namespace

int dbscan(DenoiseBuf& b, ClusterBuf& c, const float* d_pts, int64_t n, int stride, float eps, int64_t min_samples,
           int64_t cap_clusters, DbscanCounts* counts, hipStream_t st) {
    *counts = DbscanCounts{};
    if (n <= 0) return 0;
    if (stride < 3 || stride > 8 || !(eps > 0.f) || !std::isfinite(eps) || min_samples < 1 || cap_clusters < 0 ||
        n >= (int64_t)1 << 31)
        return kArg;
    int rc = denoise_reserve(b, n);
    if (!rc) rc = cluster_reserve(c, n);
    if (rc) return rc;
    const float e2 = (float)((double)eps * (double)eps);
    // no point has 2^31 neighbours: a larger min_samples means "no core point" all the same
    const uint32_t need = (uint32_t)std::min<int64_t>(min_samples, (int64_t)1 << 31);
    uint8_t* core = reinterpret_cast<uint8_t*>(c.rank_of);  // n bytes of the 4 n that the Euclidean path's ranks take
    LIO_HIP(hipMemsetAsync(c.cnt, 0, 64, st));
    LIO_HIP(hipMemsetAsync(core, 0, (size_t)n, st));        // a non-finite point is not core
    LIO_HIP(hipMemsetAsync(c.run_start, 0, sizeof(uint32_t), st));  // the first offset, when there is no cluster
    if ((rc = dn_build_grid(b, d_pts, n, stride, 0.f, eps * 1.001f, st))) return rc;
    db_core_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, eps, e2, need, b.flags, core);
    db_init_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, b.flags, n, c.parent, b.keys, b.vals, c.cnt);
    db_union_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, eps, e2, c.parent);
    db_key_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, eps, e2, c.parent, b.keys);
    if ((rc = dn_sort32(b, n, dn_bit_width((uint32_t)n), st))) return rc;  // keys in [0, n]
    cl_heads_kernel<<<nblk(n + 1), 256, 0, st>>>(b.keys_alt, n, b.flags, c.cnt);
    LIO_HIP(hipMemcpyAsync(b.h_cnt + 2, c.cnt, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    int64_t nclusters = 0;
    if ((rc = dn_scan_count(b, n, &nclusters, st))) return rc;
    counts->clustered_points = b.h_cnt[2];
    counts->core = b.h_cnt[4];
    counts->finite = b.h_cnt[5];
    counts->clusters = nclusters;
    cl_runs_kernel<<<nblk(n), 256, 0, st>>>(b.flags, b.pos, n, c.cnt, c.run_of, c.run_start);
    db_label_kernel<<<nblk(n), 256, 0, st>>>(b.vals_alt, c.run_of, n, c.labels, c.indices);
    const int64_t m = std::min(nclusters, cap_clusters);
    cl_offsets_kernel<<<nblk(m + 1), 256, 0, st>>>(c.run_start, m, c.offsets);
    if (m > 0) {  // every cluster has a member, so every box of the first m is written
        uint32_t* box = reinterpret_cast<uint32_t*>(c.aabb);
        const int64_t nin = counts->clustered_points, waves = (nin + kBoxChunk - 1) / kBoxChunk;
        db_box_init_kernel<<<nblk(6 * m), 256, 0, st>>>(box, m);
        db_box_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(d_pts, stride, c.indices, c.run_of, nin, m, box);
        db_box_decode_kernel<<<nblk(6 * m), 256, 0, st>>>(box, m);
    }
    LIO_HIP(hipGetLastError());
    return 0;
}

}  // namespace lio
