// lio_normals.hip — surface normals and curvature on gfx950, by the contract of lio_estimate_normals
// (include/lio_gpu.h): pcl::NormalEstimation's two searches [U] and Open3D's hybrid [U].
//
//   nm_knn_kernel     k given (with or without a radius): one wave per query in cell order over the density grid
//                     of dn_build_grid, the shell search of sor_knn_kernel (lio_denoise.hip) with unique 64-bit
//                     keys (d2 bits << 32 | input index), so that the k smallest under (d2, then index) are the
//                     k smallest keys; the lanes then stride over the kept neighbours and reduce the integer
//                     moments across the wave, and lane 0 writes them out
//   nm_solve_kernel   the eigen-step of the k search, one thread per point over those moments (solving in lane 0 of
//                     the search kernel instead leaves 63 lanes idle through some thousand cycles of double
//                     arithmetic: 12.2 ms against 7.5 + 0.14 ms at 2 M points, k = 20)
//   nm_radius_kernel  the radius alone: one thread per point in cell order over the rows of cell_box
//                     (lio_radius_dev.hpp) on a grid of edge 1.001 r, the moments in registers, the eigen-step
//                     in the thread
//   nm_stats_kernel   the six counts from the outputs (integer sums: no order)
//
// The arithmetic behind the search — quantisation, covariance, Jacobi, pick, orientation — is
// lio_normals_math.hpp's, the text a host build shares.  Every result is a function of the neighbour SET (integer
// sums) and of fixed-order double arithmetic, so no bit depends on the schedule.
#include <algorithm>
#include <cmath>

#include "lio_dev.hpp"
#include "lio_scratch.hpp"
#include "lio_normals.hpp"
#include "lio_normals_math.hpp"
#include "lio_radius_dev.hpp"

namespace lio {

namespace {

constexpr int kNmCand = 512;  // candidate keys a query's wave holds in LDS (4 KiB: the LDS of sor_knn_kernel's)
static_assert(kNmCand - 64 >= kNmMaxK, "the cut of a full buffer leaves k keys");

__device__ __forceinline__ void nm_cell_of(const DnGeom& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = min(max(cell_coord(x, g.ox, g.inv), 0), g.nx - 1);
    cy = min(max(cell_coord(y, g.oy, g.inv), 0), g.ny - 1);
    cz = min(max(cell_coord(z, g.oz, g.inv), 0), g.nz - 1);
}

// ascending bitonic sort of a[0 .. P) (P a power of two >= 64) by the block's single wave
__device__ __forceinline__ void nm_bitonic(uint64_t* a, int P, int lane) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = (i & k) == 0;
                const uint64_t x = a[i], y = a[l];
                if ((x > y) == up) {
                    a[i] = y;
                    a[l] = x;
                }
            }
            __syncthreads();
        }
}

// sorts the `count` keys and keeps the `need` smallest; returns the new count
__device__ __forceinline__ int nm_sort_keep(uint64_t* a, int count, int need, int lane) {
    int P = 64;
    while (P < count) P <<= 1;
    for (int i = count + lane; i < P; i += 64) a[i] = ~0ull;
    __syncthreads();
    nm_bitonic(a, P, lane);
    return min(count, need);
}

__device__ __forceinline__ long long nm_wave_sum(long long v) {  // the total in lane 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ void nm_write(const NmResult& r, uint32_t orig, int m, float* __restrict__ normals,
                                         float* __restrict__ curv, int32_t* __restrict__ counts) {
    normals[3 * (size_t)orig] = r.n[0], normals[3 * (size_t)orig + 1] = r.n[1], normals[3 * (size_t)orig + 2] = r.n[2];
    curv[orig] = r.curvature;
    counts[orig] = m;
}

__device__ __forceinline__ void nm_write_nan(uint32_t orig, int m, float* __restrict__ normals, float* __restrict__ curv,
                                             int32_t* __restrict__ counts) {
    NmResult r;
    r.n[0] = r.n[1] = r.n[2] = r.curvature = nm_nan();
    nm_write(r, orig, m, normals, curv, counts);
}

__device__ __forceinline__ const float* nm_viewpoint(const float* __restrict__ vp, int vp_stride, uint32_t orig) {
    return vp ? vp + (size_t)orig * (size_t)vp_stride : nullptr;  // vp_stride 0: the one viewpoint
}

// One wave (one 64-thread block) per query, queries in cell order: sor_knn_kernel's walk over growing cubes of
// cells (the 3x3x3 block, then one Chebyshev shell at a time, each as row segments flattened over the lanes) with
// need = k.  A candidate is a finite point with d2 < r2 when a radius is given; its key is d2 bits << 32 | input
// index — unique, and its unsigned order is (d2, then index).
//
// EXACTNESS.  (1) Stop: after the cube of radius r every point not yet visited has float d2 >= T (the argument
// of sor_knn_kernel).  When k candidates have d2 < T (STRICT: at d2 = T an unvisited point of lower index would
// come first), the k smallest keys are among the candidates; when T >= r2 no unvisited point is a candidate at
// all.  (2) Overflow: a full buffer is sorted and cut to its k smallest keys, and from then on only keys below
// the largest kept one enter; keys are unique, so exactly the keys below the final k-th survive.
//
// Lane 0 leaves the nine sums and the bound's bits in sums[10 orig ..] and m in counts; nm_solve_kernel solves.  A
// point without a normal for want of neighbours gets its NaN here.
__global__ void __launch_bounds__(64) nm_knn_kernel(const float4* __restrict__ g4, const uint32_t* __restrict__ start,
                                                    const DnGeom* __restrict__ geom, const float* __restrict__ pts,
                                                    int stride, int64_t n, int k, int has_r, float r2,
                                                    float* __restrict__ normals, float* __restrict__ curv,
                                                    int32_t* __restrict__ counts, int64_t* __restrict__ sums) {
    __shared__ uint64_t buf[kNmCand];
    __shared__ uint32_t s_beg[64], s_pre[64];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    const uint32_t nf = start[g.ncells];  // finite points
    const float4 q = g4[j];
    const uint32_t orig = __float_as_uint(q.w);
    if (j >= (int64_t)nf) {  // non-finite: nobody's neighbour
        if (lane == 0) nm_write_nan(orig, 0, normals, curv, counts);
        return;
    }
    const int need = k;
    int cx, cy, cz;
    nm_cell_of(g, q.x, q.y, q.z, cx, cy, cz);
    const int rmax = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
    int count = 0;
    bool have_tau = false;
    uint64_t tau = ~0ull;
    for (int r = 1;; ++r) {
        // the cube's rows inside the grid (clipped first: the row count stays below the cell count)
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        const uint32_t ny_r = (uint32_t)(y1 - y0 + 1), nseg = 2u * ny_r * (uint32_t)(z1 - z0 + 1);
        for (uint32_t s0 = 0; s0 < nseg; s0 += 64) {
            // lane's segment: row (dz, dy) of the cube; a boundary row is one segment [cx - r, cx + r], an inner
            // row two single cells (the shell's x faces).  r = 1 takes every row whole: the 3x3x3 block.
            const uint32_t s = s0 + (uint32_t)lane;
            uint32_t beg = 0, len = 0;
            if (s < nseg) {
                const uint32_t row = s >> 1;
                const int which = (int)(s & 1u);
                const int z = z0 + (int)(row / ny_r), y = y0 + (int)(row % ny_r);
                const int dz = z - cz, dy = y - cy;
                const bool whole = r == 1 || dz == r || dz == -r || dy == r || dy == -r;
                int xa, xb;
                if (whole) {
                    xa = which == 0 ? max(cx - r, 0) : 1;
                    xb = which == 0 ? min(cx + r, g.nx - 1) : 0;
                } else {
                    xa = xb = which ? cx + r : cx - r;
                    if (xa < 0 || xa >= g.nx) xb = xa - 1;
                }
                if (xa <= xb) {
                    const uint32_t base = ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx;
                    beg = start[base + (uint32_t)xa];
                    len = start[base + (uint32_t)xb + 1u] - beg;
                }
            }
            uint32_t incl = len;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
                if (lane >= o) incl += t;
            }
            const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
            __syncthreads();  // the previous chunk's readers are done
            s_beg[lane] = beg;
            s_pre[lane] = incl - len;
            __syncthreads();
            for (uint32_t t0 = 0; t0 < total; t0 += 64) {
                if (count + 64 > kNmCand) {  // count > kNmCand - 64 >= need: the cut always leaves `need` keys
                    __syncthreads();
                    count = nm_sort_keep(buf, count, need, lane);
                    tau = buf[need - 1];
                    have_tau = true;
                    __syncthreads();
                }
                const uint32_t e = t0 + (uint32_t)lane;
                bool take = false;
                uint64_t key = 0;
                if (e < total) {
                    int sg = 0;  // the last segment whose exclusive prefix is <= e
#pragma unroll
                    for (int w = 32; w > 0; w >>= 1)
                        if (s_pre[sg + w] <= e) sg += w;
                    const float4 p = g4[s_beg[sg] + (e - s_pre[sg])];
                    const float d = sqdist3(q.x, q.y, q.z, p.x, p.y, p.z);
                    key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)__float_as_uint(p.w);
                    take = (!has_r || d < r2) && (!have_tau || key < tau);
                }
                const uint64_t m = __ballot(take);
                if (take)
                    buf[count + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = key;
                count += (int)__popcll(m);
            }
        }
        if (r >= rmax) break;  // the cube covers the grid
        float b = INFINITY;
        if (cx - r > 0) b = fminf(b, q.x - (g.ox + (float)(cx - r) * g.cell));
        if (cx + r < g.nx - 1) b = fminf(b, (g.ox + (float)(cx + r + 1) * g.cell) - q.x);
        if (cy - r > 0) b = fminf(b, q.y - (g.oy + (float)(cy - r) * g.cell));
        if (cy + r < g.ny - 1) b = fminf(b, (g.oy + (float)(cy + r + 1) * g.cell) - q.y);
        if (cz - r > 0) b = fminf(b, q.z - (g.oz + (float)(cz - r) * g.cell));
        if (cz + r < g.nz - 1) b = fminf(b, (g.oz + (float)(cz + r + 1) * g.cell) - q.z);
        b -= g.margin;
        if (b > 1e-15f) {
            const float T = b * b * 0.99999f;
            if (has_r && T >= r2) break;  // nothing behind the cube lies within the radius
            if (count >= need) {
                __syncthreads();
                int c = 0;
                for (int i0 = 0; i0 < count; i0 += 64) {
                    const int i = i0 + lane;
                    c += (int)__popcll(__ballot(i < count && __uint_as_float((uint32_t)(buf[i] >> 32)) < T));
                }
                if (c >= need) break;
            }
        }
    }
    __syncthreads();
    const int m = nm_sort_keep(buf, count, need, lane);  // buf[0 .. m): N_i in (d2, index) order
    if (m < 3) {
        if (lane == 0) nm_write_nan(orig, m, normals, curv, counts);
        return;
    }
    const float B = has_r ? r2 : __uint_as_float((uint32_t)(buf[m - 1] >> 32));
    const double s = nm_scale(B);
    NmSums a;
    for (int i = lane; i < m; i += 64) {
        const float* p = pts + (size_t)(uint32_t)buf[i] * (size_t)stride;
        nm_add(a, p[0] - q.x, p[1] - q.y, p[2] - q.z, s);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.s[c] = nm_wave_sum(a.s[c]);
#pragma unroll
    for (int c = 0; c < 6; ++c) a.ss[c] = nm_wave_sum(a.ss[c]);
    if (lane != 0) return;
    int64_t* o = sums + 10 * (size_t)orig;
    for (int c = 0; c < 3; ++c) o[c] = a.s[c];
    for (int c = 0; c < 6; ++c) o[3 + c] = a.ss[c];
    o[9] = (int64_t)__float_as_uint(B);
    counts[orig] = m;
}

// the eigen-step of the k search: one thread per input point over what nm_knn_kernel left (a point with
// counts < 3 has its NaN already)
__global__ void nm_solve_kernel(const float* __restrict__ pts, int stride, int64_t n, const int64_t* __restrict__ sums,
                                const float* __restrict__ vp, int vp_stride, float* __restrict__ normals,
                                float* __restrict__ curv, const int32_t* __restrict__ counts) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = counts[i];
    if (m < 3) return;
    const int64_t* o = sums + 10 * (size_t)i;
    NmSums a;
    for (int c = 0; c < 3; ++c) a.s[c] = o[c];
    for (int c = 0; c < 6; ++c) a.ss[c] = o[3 + c];
    const float* p = pts + (size_t)i * stride;
    const NmResult r = nm_solve(a, m, __uint_as_float((uint32_t)o[9]), p[0], p[1], p[2], nm_viewpoint(vp, vp_stride, (uint32_t)i));
    normals[3 * (size_t)i] = r.n[0], normals[3 * (size_t)i + 1] = r.n[1], normals[3 * (size_t)i + 2] = r.n[2];
    curv[i] = r.curvature;
}

// One thread per point, points in cell order (neighbouring threads walk the same rows): every row of cell_box,
// which holds every point with d2 <= r2 whatever the cell size (lio_radius_dev.hpp).  B = r2 is known before
// the walk, so one pass gathers the count and the sums; they are integer sums, so the row order is immaterial.
__global__ void __launch_bounds__(256) nm_radius_kernel(const float4* __restrict__ g4, const uint32_t* __restrict__ start,
                                                        const DnGeom* __restrict__ geom, int64_t n, float radius, float r2,
                                                        const float* __restrict__ vp, int vp_stride,
                                                        float* __restrict__ normals, float* __restrict__ curv,
                                                        int32_t* __restrict__ counts) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    const float4 q = g4[j];
    const uint32_t orig = __float_as_uint(q.w);
    if (j >= (int64_t)start[g.ncells]) {  // non-finite
        nm_write_nan(orig, 0, normals, curv, counts);
        return;
    }
    const double s = nm_scale(r2);
    NmSums a;
    int m = 0;
    const auto b = cell_box<false>(g, q.x, q.y, q.z, radius);
    for (int cz = b.z0; cz <= b.z1; ++cz)
        for (int cy = b.y0; cy <= b.y_last(cz); ++cy) {
            uint32_t t, e;
            b.row(g, start, cz, cy, t, e);
            for (; t < e; ++t) {
                const float4 p = g4[t];
                if (sqdist3(q.x, q.y, q.z, p.x, p.y, p.z) < r2) {
                    nm_add(a, p.x - q.x, p.y - q.y, p.z - q.z, s);
                    ++m;
                }
            }
        }
    if (m < 3) {
        nm_write_nan(orig, m, normals, curv, counts);
        return;
    }
    nm_write(nm_solve(a, m, r2, q.x, q.y, q.z, nm_viewpoint(vp, vp_stride, orig)), orig, m, normals, curv, counts);
}

// stats[0 .. 6) += finite points, points with a normal, finite points with m < 3, degenerate points, sum of m;
// stats[4] = max m.  Per block in LDS, then one atomic per counter.
__global__ void __launch_bounds__(256) nm_stats_kernel(const float* __restrict__ pts, int stride, int64_t n,
                                                       const float* __restrict__ normals,
                                                       const int32_t* __restrict__ counts,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s[6];
    if (threadIdx.x < 6) s[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) {
        const float* p = pts + (size_t)i * stride;
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
            const int m = counts[i];
            const bool has = !isnan(normals[3 * (size_t)i]);
            atomicAdd(&s[0], 1ull);
            if (has) atomicAdd(&s[1], 1ull);
            else if (m < 3) atomicAdd(&s[2], 1ull);
            else atomicAdd(&s[3], 1ull);
            atomicMax(&s[4], (unsigned long long)m);
            atomicAdd(&s[5], (unsigned long long)m);
        }
    }
    __syncthreads();
    if (threadIdx.x < 6 && s[threadIdx.x]) {
        if (threadIdx.x == 4) atomicMax(&stats[4], s[4]);
        else atomicAdd(&stats[threadIdx.x], s[threadIdx.x]);
    }
}

}  // namespace

void normals_free(NormalsBuf& nb) {
    dev_free(&nb.arena, &nb.vp, &nb.sums);
    host_free(&nb.h_stats);
    nb = NormalsBuf{};
}

int normals_reserve(NormalsBuf& nb, int64_t n, int64_t vp_floats, bool with_sums) {
    int rc = grow_pinned(&nb.h_stats, nb.h_stats_bytes, 6 * sizeof(int64_t), 64);
    if (!rc && vp_floats > 0) rc = grow_buf(&nb.vp, nb.vp_cap, vp_floats);
    if (!rc && with_sums) rc = grow_buf(&nb.sums, nb.sums_cap, n, 10, 4096);
    if (rc || (n <= nb.cap && nb.arena)) return rc;
    const size_t C = (size_t)grown<int64_t>(n, nb.cap, 4096);
    dev_free(&nb.arena);
    nb.arena_bytes = 0, nb.cap = 0;
    auto fields = [&](Carver& at) {  // the arena's fields, once each, in arena order
        at(nb.normals, 3 * C), at(nb.curvature, C), at(nb.counts, C), at(nb.stats, 6);
    };
    rc = reserve_arena(&nb.arena, nb.arena_bytes, fields, 0);
    if (rc) return rc;
    nb.cap = (int64_t)C;
    return kOk;
}

int estimate_normals(DenoiseBuf& b, NormalsBuf& nb, const float* d_pts, int64_t n, int stride, float radius, int k,
                     const float* d_vp, int vp_stride, hipStream_t st) {
    const float r2 = (float)((double)radius * (double)radius);  // PCL passes radius * radius cast to float [U]
    if (n <= 0 || stride < 3 || stride > 8 || !(radius >= 0.f) || (k != 0 && (k < 3 || k > kNmMaxK)) ||
        (k == 0 && !(radius > 0.f)) || (radius > 0.f && (!(r2 > 0.f) || !std::isfinite(r2))) || n > nb.cap ||
        (k > 0 && n > nb.sums_cap))
        return kArg;
    int rc = denoise_reserve(b, n);
    if (rc) return rc;
    LIO_HIP(hipMemsetAsync(nb.stats, 0, 6 * sizeof(unsigned long long), st));
    if (k > 0) {
        // the density grid of the SOR search: a 3x3x3 block of cells holds about k points
        if ((rc = dn_build_grid(b, d_pts, n, stride, (float)k, 0.f, st))) return rc;
        nm_knn_kernel<<<(unsigned)n, 64, 0, st>>>(b.g4, b.start, b.geom, d_pts, stride, n, k, radius > 0.f, r2, nb.normals,
                                                   nb.curvature, nb.counts, nb.sums);
        nm_solve_kernel<<<nblk(n), 256, 0, st>>>(d_pts, stride, n, nb.sums, d_vp, vp_stride, nb.normals, nb.curvature,
                                                 nb.counts);
    } else {
        if ((rc = dn_build_grid(b, d_pts, n, stride, 0.f, radius * 1.001f, st))) return rc;  // the clusterers' edge
        nm_radius_kernel<<<nblk(n), 256, 0, st>>>(b.g4, b.start, b.geom, n, radius, r2, d_vp, vp_stride, nb.normals,
                                                  nb.curvature, nb.counts);
    }
    nm_stats_kernel<<<nblk(n), 256, 0, st>>>(d_pts, stride, n, nb.normals, nb.counts, nb.stats);
    LIO_HIP(hipGetLastError());
    LIO_HIP(hipMemcpyAsync(nb.h_stats, nb.stats, 6 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return kOk;
}

}  // namespace lio
