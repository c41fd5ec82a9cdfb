// lio_cluster_dev.hpp — what lio_cluster.hip (Euclidean clusters) and lio_dbscan.hip (DBSCAN) share: the
// lock-free union-find over input indices, whose root is the lowest index of its tree, the union kernel, the
// kernels of the tail that turns sorted (key, index) pairs into runs and offsets, the bounding boxes, and the
// three host sequences both drivers open, continue and end with (cl_open, cl_sorted_runs, cl_offsets_boxes).
// Included by those two files only; everything here is internal to the file that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "lio_cluster.hpp"
#include "lio_radius_dev.hpp"  // CellBox, cell_box
#include "lio_scratch.hpp"

namespace lio {

namespace {

constexpr uint32_t kNoRun = 0xffffffffu;
constexpr uint32_t kCoreBit = 0x80000000u;  // n < 2^31: bit 31 of the index word of a gridded point is free (DBSCAN)

// parent[] is read past the L1 (a relaxed agent-scope load): another CU's hook is seen as soon as it is in
// memory.  Correctness does not rest on that — an old value of parent[x] is still a node of x's tree that is
// <= x, and only a CAS on a node that IS its own parent hooks anything — it only saves retries.
__device__ __forceinline__ uint32_t ld_parent(const uint32_t* parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the chain from x: strictly decreasing, so at most x steps
__device__ __forceinline__ uint32_t uf_find(const uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = ld_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
}

// the root of x once the forest is final (a later launch than the union's): plain loads, at most x steps
__device__ __forceinline__ uint32_t uf_root(const uint32_t* __restrict__ parent, uint32_t x) {
    for (uint32_t up = parent[x]; up != x; up = parent[x]) x = up;
    return x;
}

// Unites the trees of a and b; returns a node of the united tree that was its root when seen.  The root with
// the larger index is hooked under the smaller.  A failed CAS returns parent[hi] < hi (hooked meanwhile by
// someone else): the search goes on from there, so a + b strictly decreases from retry to retry.
__device__ __forceinline__ uint32_t uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = old;
        b = lo;
    }
}

// the candidate test of the union and of DBSCAN's key pass.  kCoreOnly = false: FLANN's radius set keeps
// dist < radius [U], every point counts; true: radius_neighbors keeps dist <= radius [U], core points only
template <bool kCoreOnly>
__device__ __forceinline__ bool radius_hit(const float4& q, const float4& s, float r2) {
    const float d = sqdist3(q.x, q.y, q.z, s.x, s.y, s.z);
    return kCoreOnly ? (__float_as_uint(s.w) & kCoreBit) && d <= r2 : d < r2;
}
template <bool kCoreOnly>
__device__ __forceinline__ uint32_t index_of(const float4& s) {  // the input index of a gridded point
    return kCoreOnly ? __float_as_uint(s.w) & ~kCoreBit : __float_as_uint(s.w);
}

// ---- the union kernel -------------------------------------------------------------------------------
// One thread per finite point (kCoreOnly: per core point), in cell order (position j of pts); it tests the
// points (the core points) of LOWER position in its cell range (cell_box's lower half), so every pair is tested
// once, by its later point, strictly for the Euclidean clusters and inclusively for DBSCAN (radius_hit).
//
// Pairs that are already in one set skip the union: the thread keeps `ra`, a node of its own tree that was
// the root when last seen, and a neighbour whose parent is `ra` needs nothing.  At the end the thread's own
// parent is shortened to `ra` (atomicMin: never increases a parent).
template <bool kCoreOnly>
__global__ void __launch_bounds__(256) cl_union_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ start,
                                                       const DnGeom* __restrict__ geom, int64_t n, float r, float r2,
                                                       uint32_t* parent) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    if (j >= (int64_t)start[g.ncells]) return;  // past the finite points
    const float4 q = pts[j];
    if (kCoreOnly && !(__float_as_uint(q.w) & kCoreBit)) return;
    const uint32_t me = index_of<kCoreOnly>(q);
    uint32_t ra = me;
    const auto b = cell_box<true>(g, q.x, q.y, q.z, r, (uint32_t)j);
    for (int cz = b.z0; cz <= b.z1; ++cz)
        for (int cy = b.y0; cy <= b.y_last(cz); ++cy) {
            uint32_t k, e;
            b.row(g, start, cz, cy, k, e);
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
                for (int u = 0; u < 4; ++u) hit[u] = radius_hit<kCoreOnly>(q, s[u], r2);
#pragma unroll
                for (int u = 0; u < 4; ++u) par[u] = hit[u] ? ld_parent(parent, index_of<kCoreOnly>(s[u])) : ra;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (hit[u] && par[u] != ra) ra = uf_unite(parent, ra, index_of<kCoreOnly>(s[u]));
            }
            for (; k < e; ++k) {
                const float4 s = pts[k];
                if (radius_hit<kCoreOnly>(q, s, r2)) {
                    const uint32_t other = index_of<kCoreOnly>(s);
                    if (ld_parent(parent, other) != ra) ra = uf_unite(parent, ra, other);
                }
            }
        }
    if (ra != me) atomicMin(parent + me, ra);
}

// ---- the tail: sorted (key, index) pairs -> runs -> offsets ---------------------------------------------
// flags[j] = 1 at the first entry of every run of equal keys (flags[n] = 0); key n marks an entry outside
// every run, and those sort last; cnt[0] = entries in runs (zeroed before: no such entry leaves it 0)
__global__ void cl_heads_kernel(const uint32_t* __restrict__ skeys, int64_t n, uint32_t* __restrict__ flags,
                                uint32_t* __restrict__ cnt) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j > n) return;
    uint32_t f = 0;
    if (j < n) {
        const uint32_t k = skeys[j];
        if (k != (uint32_t)n) {
            f = j == 0 || skeys[j - 1] != k;
            if (j + 1 == n || skeys[j + 1] == (uint32_t)n) cnt[0] = (uint32_t)(j + 1);
        }
    }
    flags[j] = f;
}

// pos = exclusive scan of flags: the run of position j is pos[j] + flags[j] - 1
__global__ void cl_runs_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos, int64_t n,
                               const uint32_t* __restrict__ cnt, uint32_t* __restrict__ run_of,
                               uint32_t* __restrict__ run_start) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t nf = cnt[0];
    if (j >= (int64_t)nf) {
        run_of[j] = kNoRun;
        return;
    }
    const uint32_t run = pos[j] + flags[j] - 1u;
    run_of[j] = run;
    if (flags[j]) run_start[run] = (uint32_t)j;
    if (j + 1 == (int64_t)nf) run_start[run + 1u] = nf;
}

__global__ void cl_offsets_kernel(const uint32_t* __restrict__ off, int64_t m, int64_t* __restrict__ offsets) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t <= m) offsets[t] = (int64_t)off[t];
}

// ---- bounding boxes -----------------------------------------------------------------------------------
// One cluster may hold nearly every point (DBSCAN has no size filter and PCL's max_size defaults to INT_MAX: the
// ground with everything standing on it), and one wave per cluster would walk it alone.  Here one wave takes
// kBoxChunk consecutive positions of the grouped `indices` order, whatever clusters they belong to (run_of[j] is
// the cluster of position j): it keeps the min / max of the run it is in in registers and hands them over with
// one atomic min / max per coordinate when the run changes and at its end.  Floats go through an
// order-preserving map to unsigned integers, so the atomics are integer ones and the result does not depend on
// their order.
constexpr int kBoxChunk = 1024;

__device__ __forceinline__ uint32_t ord_of(float v) {  // unsigned order = float order (-0 below +0); no NaN comes here
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ord_to(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

__global__ void cl_box_init_kernel(uint32_t* __restrict__ box, int64_t m) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < 6 * m) box[t] = ord_of(t % 6 < 3 ? INFINITY : -INFINITY);
}

// the wave's min / max into box[run] (all lanes call it; lanes without a point hold +inf / -inf)
__device__ __forceinline__ void cl_box_flush(uint32_t run, int64_t m, float (&lo)[3], float (&hi)[3], int lane,
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

__global__ void __launch_bounds__(256) cl_box_kernel(const float* __restrict__ p, int stride,
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
        if (!(one_run && first == cur)) cl_box_flush(cur, m, lo, hi, lane, box);
        if (one_run) {
            cur = first;
            if (valid)
#pragma unroll
                for (int d = 0; d < 3; ++d) lo[d] = fminf(lo[d], v[d]), hi[d] = fmaxf(hi[d], v[d]);
        } else {  // a run ends inside these 64 positions: min / max over every stretch of lanes of one run (a
                  // segmented scan: runs are contiguous), handed over by the stretch's last lane
            cur = kNoRun;
            if (valid)
#pragma unroll
                for (int d = 0; d < 3; ++d) lo[d] = hi[d] = v[d];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const bool same = (uint32_t)__shfl_up((int)run, o, 64) == run && lane >= o;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float l = __shfl_up(lo[d], o, 64), h = __shfl_up(hi[d], o, 64);
                    if (same) lo[d] = fminf(lo[d], l), hi[d] = fmaxf(hi[d], h);
                }
            }
            const bool last = lane == 63 || (uint32_t)__shfl_down((int)run, 1, 64) != run;
            if (valid && last && run < (uint32_t)m)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    atomicMin(box + (size_t)run * 6 + d, ord_of(lo[d]));
                    atomicMax(box + (size_t)run * 6 + 3 + d, ord_of(hi[d]));
                }
#pragma unroll
            for (int d = 0; d < 3; ++d) lo[d] = INFINITY, hi[d] = -INFINITY;
        }
    }
    cl_box_flush(cur, m, lo, hi, lane, box);
}

__global__ void cl_box_decode_kernel(uint32_t* box, int64_t m) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < 6 * m) box[t] = __float_as_uint(ord_to(box[t]));
}

// ---- the host sequences both drivers share (n > 0; status as theirs) --------------------------------------
// the argument check, both arenas, the zeroed counters and the grid with cell edge 1.001 r (no host wait);
// `least` is min_size / min_samples
inline int cl_open(DenoiseBuf& b, ClusterBuf& c, const float* d_pts, int64_t n, int stride, float r, int64_t least,
                   int64_t cap_clusters, hipStream_t st) {
    if (stride < 3 || stride > 8 || !(r > 0.f) || !std::isfinite(r) || least < 1 || cap_clusters < 0 ||
        n >= (int64_t)1 << 31)
        return kArg;
    int rc = denoise_reserve(b, n);
    if (!rc) rc = cluster_reserve(c, n);
    if (rc) return rc;
    LIO_HIP(hipMemsetAsync(c.cnt, 0, 64, st));
    return dn_build_grid(b, d_pts, n, stride, 0.f, r * 1.001f, st);
}

// (b.keys, b.vals) = (key in [0, n], index) per point -> stable sort by key -> run heads -> *nruns (the ONE host
// wait; the first cnt_words words of c.cnt cross with it into b.h_cnt[2 ..]) -> c.run_of / c.run_start
inline int cl_sorted_runs(DenoiseBuf& b, ClusterBuf& c, int64_t n, int cnt_words, int64_t* nruns, hipStream_t st) {
    int rc = dn_sort32(b, n, dn_bit_width((uint32_t)n), st);
    if (rc) return rc;
    cl_heads_kernel<<<nblk(n + 1), 256, 0, st>>>(b.keys_alt, n, b.flags, c.cnt);
    if (cnt_words)
        LIO_HIP(hipMemcpyAsync(b.h_cnt + 2, c.cnt, cnt_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if ((rc = dn_scan_count(b, n, nruns, st))) return rc;
    cl_runs_kernel<<<nblk(n), 256, 0, st>>>(b.flags, b.pos, n, c.cnt, c.run_of, c.run_start);
    return kOk;
}

// c.offsets and c.aabb of the first m clusters: off[t] = first position of cluster t in c.indices, cluster_of[j]
// the cluster of position j < nin of c.indices.  Every cluster has a member, so every box of the first m is written.
inline int cl_offsets_boxes(ClusterBuf& c, const float* d_pts, int stride, const uint32_t* off,
                            const uint32_t* cluster_of, int64_t nin, int64_t m, hipStream_t st) {
    cl_offsets_kernel<<<nblk(m + 1), 256, 0, st>>>(off, m, c.offsets);
    if (m > 0) {
        uint32_t* box = reinterpret_cast<uint32_t*>(c.aabb);
        const int64_t waves = (nin + kBoxChunk - 1) / kBoxChunk;
        cl_box_init_kernel<<<nblk(6 * m), 256, 0, st>>>(box, m);
        cl_box_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(d_pts, stride, c.indices, cluster_of, nin, m, box);
        cl_box_decode_kernel<<<nblk(6 * m), 256, 0, st>>>(box, m);
    }
    LIO_HIP(hipGetLastError());
    return kOk;
}

}  // namespace

}  // namespace lio
