// lio_denoise.hip — the back end's intensity denoise on gfx950 (fast_lio_sam.cpp:262-365, 575-680,
// 941-1008; config.yaml:32-42):
//
//   sor_distances     the body of pcl::StatisticalOutlierRemoval [U]: per point the mean distance to its
//                     mean_k nearest neighbours (a (mean_k + 1)-NN search with the query dropped)
//   sor_filter        applyFilter: mean / stddev of those distances in PCL's double loop on the host
//                     (the order of the double sums), threshold, stable compaction on the device
//   radius_first_seed KdTreeFLANN::radiusSearch per seed [U], turned round: per cloud point the lowest seed
//                     index within the radius
//   denoise_slam_map  FastLioSam::denoise_slam_map as set operations on the device
//
// Both searches use one uniform cell grid built without a host wait: AABB partials -> geometry on the
// device -> cell keys -> stable radix sort -> CSR offsets by binary search -> points gathered in cell order.
//
// Exactness of the searches rests on ONE property of the cell assignment: cell_coord() is a monotone
// (non-decreasing) function of the coordinate — float subtraction of a constant, multiplication by a positive
// constant, floor and clamping all are.  Squared distances are sqdist3's float ((dx*dx + dy*dy) + dz*dz),
// the expression the ICP 1-NN uses for FLANN's L2 (-ffp-contract=off: no FMA).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lio_dev.hpp"
#include "lio_scratch_cub.hpp"
#include "lio_denoise.hpp"
#include "lio_radius_dev.hpp"  // cell_box: Kernel B's cell range (shared with the clusterers)

namespace lio {

namespace {

constexpr int kDnPartBlocks = 1024;  // AABB partials
constexpr int kCand = 1024;          // candidate squared distances a query's wave holds in LDS
constexpr int kMaxMeanK = 255;

// per block: min / max of the finite points it covers -> part[6 blockIdx.x ..] (lo xyz, hi xyz)
__device__ __forceinline__ void block_minmax6(float (*s)[256], const float* lo, const float* hi) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        s[d][tid] = lo[d];
        s[3 + d][tid] = hi[d];
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                s[d][tid] = fminf(s[d][tid], s[d][tid + w]);
                s[3 + d][tid] = fmaxf(s[3 + d][tid], s[3 + d][tid + w]);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) dn_minmax_kernel(const float* __restrict__ p, int64_t n, int stride,
                                                        float* __restrict__ part) {
    __shared__ float s[6][256];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float* q = p + (size_t)i * stride;
        const float x = q[0], y = q[1], z = q[2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
        lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), lo[2] = fminf(lo[2], z);
        hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y), hi[2] = fmaxf(hi[2], z);
    }
    block_minmax6(s, lo, hi);
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

// One block: the AABB from the partials, then the grid.  target > 0 (SOR): the cell edge from the cloud's
// density so that a 3x3x3 block of cells holds about `target` points — the largest of the volume, the
// largest-face and the longest-edge estimate, so that planar and linear clouds get sensible cells too.
// target == 0 (radius query): the edge is fixed_cell.  Either edge grows until the grid has at most cells_cap
// cells.  The dimensions come from cell_coord of the AABB maximum itself, so no finite point falls outside.
__global__ void __launch_bounds__(256) dn_geom_kernel(const float* __restrict__ part, int nbp, int64_t n, float target,
                                                      float fixed_cell, uint32_t cells_cap, DnGeom* __restrict__ out) {
    __shared__ float s[6][256];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nbp; b += 256) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], part[b * 6 + d]);
            hi[d] = fmaxf(hi[d], part[b * 6 + 3 + d]);
        }
    }
    block_minmax6(s, lo, hi);
    if (threadIdx.x != 0) return;
    float l3[3] = {s[0][0], s[1][0], s[2][0]}, h3[3] = {s[3][0], s[4][0], s[5][0]};
    if (!(l3[0] <= h3[0])) {  // no finite point
        for (int d = 0; d < 3; ++d) l3[d] = h3[d] = 0.f;
    }
    const double ex = (double)h3[0] - l3[0], ey = (double)h3[1] - l3[1], ez = (double)h3[2] - l3[2];
    double cell = fixed_cell;
    if (target > 0.f) {
        const double nn = (double)(n > 0 ? n : 1), t = target;
        const double c3 = cbrt(ex * ey * ez * t / (27.0 * nn));
        const double c2 = sqrt(fmax(ex * ey, fmax(ey * ez, ex * ez)) * t / (9.0 * nn));
        const double c1 = fmax(ex, fmax(ey, ez)) * t / (3.0 * nn);
        cell = fmax(c3, fmax(c2, c1));
    }
    float cf = (float)cell;
    if (!(cf > 1e-30f) || !isfinite(cf)) cf = 1.f;
    DnGeom g;
    for (int it = 0; it < 4096; ++it) {
        g.cell = cf;
        g.inv = 1.0f / cf;
        g.nx = max(cell_coord(h3[0], l3[0], g.inv) + 1, 1);
        g.ny = max(cell_coord(h3[1], l3[1], g.inv) + 1, 1);
        g.nz = max(cell_coord(h3[2], l3[2], g.inv) + 1, 1);
        if ((double)g.nx * (double)g.ny * (double)g.nz <= (double)cells_cap) break;
        cf *= 1.26f;
    }
    g.ox = l3[0], g.oy = l3[1], g.oz = l3[2];
    g.ncells = (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz;
    float mabs = 0.f;
    for (int d = 0; d < 3; ++d) mabs = fmaxf(mabs, fmaxf(fabsf(l3[d]), fabsf(h3[d])));
    // cell assignment against a face o + k * cell: (v - o) * inv carries three roundings of 2^-24 of the extent,
    // the face two more of the extent and of |o|: under 4e-7 of (extent + |coordinate|); 1e-6 covers it
    g.margin = 1e-6f * ((float)fmax(ex, fmax(ey, ez)) + mabs);
    *out = g;
}

__device__ __forceinline__ uint32_t dn_cell_of(const DnGeom& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = min(max(cell_coord(x, g.ox, g.inv), 0), g.nx - 1);
    cy = min(max(cell_coord(y, g.oy, g.inv), 0), g.ny - 1);
    cz = min(max(cell_coord(z, g.oz, g.inv), 0), g.nz - 1);
    return ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
}

// non-finite points get `invalid` (> every cell index): the sort leaves them last
__global__ void dn_key_kernel(const float* __restrict__ p, int64_t n, int stride, const DnGeom* __restrict__ geom,
                              uint32_t invalid, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DnGeom g = *geom;
    const float* q = p + (size_t)i * stride;
    uint32_t k = invalid;
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) {
        int cx, cy, cz;
        k = dn_cell_of(g, q[0], q[1], q[2], cx, cy, cz);
    }
    keys[i] = k;
    vals[i] = (uint32_t)i;
}

// start[c] = first sorted entry with key >= c, for c in [0, cells_cap]: CSR offsets; every c past the last
// cell (start[ncells] among them) gives the number of finite points
__global__ void dn_start_kernel(const uint32_t* __restrict__ skeys, int64_t n, uint32_t cells_cap,
                                uint32_t* __restrict__ start) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c > (int64_t)cells_cap) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skeys[mid] < (uint32_t)c) lo = mid + 1;
        else hi = mid;
    }
    start[c] = (uint32_t)lo;
}

__global__ void dn_gather_kernel(const float* __restrict__ p, int64_t n, int stride, const uint32_t* __restrict__ svals,
                                 float4* __restrict__ g4) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = svals[j];
    const float* q = p + (size_t)i * stride;
    g4[j] = make_float4(q[0], q[1], q[2], __uint_as_float(i));
}

// ---- kernel A ---------------------------------------------------------------------------------------
// ascending bitonic sort of a[0 .. P) (P a power of two >= 64) by the block's single wave
__device__ __forceinline__ void wave_bitonic(uint32_t* a, int P, int lane) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = (i & k) == 0;
                const uint32_t x = a[i], y = a[l];
                if ((x > y) == up) {
                    a[i] = y;
                    a[l] = x;
                }
            }
            __syncthreads();
        }
}

// sorts the `count` candidates (bit patterns of non-negative floats: unsigned order = float order) and keeps
// the `need` smallest; returns the new count
__device__ __forceinline__ int sort_keep(uint32_t* a, int count, int need, int lane) {
    int P = 64;
    while (P < count) P <<= 1;
    for (int i = count + lane; i < P; i += 64) a[i] = 0xffffffffu;
    __syncthreads();
    wave_bitonic(a, P, lane);
    return min(count, need);
}

// One wave (one 64-thread block) per query, queries in cell order.  The wave gathers the squared distances
// to the points of growing cubes of cells around the query's cell — the 3x3x3 block first, then one
// Chebyshev shell at a time, each shell as row segments (a row of cells is one contiguous range of the
// sorted points), flattened over the lanes with a prefix sum — into `buf`.
//
// EXACTNESS.  (1) Stop: after the cube of radius r, a point not yet visited has, on some axis, a cell index
// outside [c - r, c + r]; by the monotone cell assignment it lies beyond that face of the cube, so its
// distance is at least b = (smallest distance from the query to a cube face that still has cells behind
// it) - margin, and its float squared distance at least T = b * b * 0.99999 (rounding of sqdist3: < 4e-7
// relative).  When mean_k + 1 candidates are <= T, the mean_k + 1 smallest of all squared distances are
// among the candidates.  (2) Overflow: when the buffer cannot take another 64 candidates it is sorted and
// cut to its mean_k + 1 smallest, and from then on only candidates strictly below the largest kept value tau
// enter: a dropped value is >= tau >= the final (mean_k + 1)-th smallest, and equal values are
// interchangeable (the result uses no ids), so the multiset of the mean_k + 1 smallest is unchanged.
// Nothing is truncated.
__global__ void __launch_bounds__(64) sor_knn_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ start,
                                                     const DnGeom* __restrict__ geom, int64_t n, int mean_k,
                                                     float* __restrict__ dist) {
    __shared__ uint32_t buf[kCand];
    __shared__ uint32_t s_beg[64], s_pre[64];
    __shared__ double s_sq[kMaxMeanK + 1];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    if (j >= n) return;
    const DnGeom g = *geom;
    const uint32_t nf = start[g.ncells];  // finite points
    const float4 q = pts[j];
    const uint32_t orig = __float_as_uint(q.w);
    const int need = mean_k + 1;
    if (j >= (int64_t)nf || nf < (uint32_t)need) {  // non-finite, or nearestK comes back short [U]: not counted
        if (lane == 0) dist[orig] = -1.f;
        return;
    }
    int cx, cy, cz;
    (void)dn_cell_of(g, q.x, q.y, q.z, cx, cy, cz);
    const int rmax = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
    int count = 0;
    bool have_tau = false;
    float tau = INFINITY;
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
                {
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
                if (count + 64 > kCand) {  // count > kCand - 64 >= need: the cut always leaves `need` values
                    __syncthreads();
                    count = sort_keep(buf, count, need, lane);
                    tau = __uint_as_float(buf[need - 1]);
                    have_tau = true;
                    __syncthreads();
                }
                const uint32_t e = t0 + (uint32_t)lane;
                bool take = false;
                float d = 0.f;
                if (e < total) {
                    int sg = 0;  // the last segment whose exclusive prefix is <= e (empty ones share a prefix
                                 // with the segment after them, so the last one is the one that holds e)
#pragma unroll
                    for (int w = 32; w > 0; w >>= 1)
                        if (s_pre[sg + w] <= e) sg += w;
                    const float4 p = pts[s_beg[sg] + (e - s_pre[sg])];
                    d = sqdist3(q.x, q.y, q.z, p.x, p.y, p.z);
                    take = !have_tau || d < tau;
                }
                const uint64_t m = __ballot(take);
                if (take)
                    buf[count + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] =
                        __float_as_uint(d);
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
        if (b > 1e-15f && count >= need) {
            const float T = b * b * 0.99999f;
            __syncthreads();
            int c = 0;
            for (int i0 = 0; i0 < count; i0 += 64) {
                const int i = i0 + lane;
                c += (int)__popcll(__ballot(i < count && __uint_as_float(buf[i]) <= T));
            }
            if (c >= need) break;
        }
    }
    __syncthreads();
    count = sort_keep(buf, count, need, lane);  // count >= need: nf >= need and every cell was reachable
    // drop the first (PCL takes it for the query), sqrt of each float promoted to double [U], added in
    // ascending order into a double by one lane, / (double)mean_k, cast to float
    for (int i = lane; i < mean_k; i += 64) s_sq[i] = sqrt((double)__uint_as_float(buf[i + 1]));
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;
        for (int i = 0; i < mean_k; ++i) acc += s_sq[i];
        dist[orig] = count >= need ? (float)(acc / (double)mean_k) : -1.f;
    }
}

// ---- kernel B ---------------------------------------------------------------------------------------
// One thread per cloud point over the grid of the seeds: every row of cell_box (lio_radius_dev.hpp, with the
// reason why it holds every seed within the radius).  The lowest index wins, so the result does not depend on
// the scan order.
__global__ void radius_seed_kernel(const float* __restrict__ p, int64_t n, int stride, const float4* __restrict__ seeds,
                                   const uint32_t* __restrict__ start, const DnGeom* __restrict__ geom, float r, float r2,
                                   int32_t* __restrict__ seed_out, float* __restrict__ d2_out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DnGeom g = *geom;
    const float* q = p + (size_t)i * stride;
    const float x = q[0], y = q[1], z = q[2];
    int best = 0x7fffffff;
    float bd = 0.f;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
        const auto b = cell_box<false>(g, x, y, z, r);
        for (int cz = b.z0; cz <= b.z1; ++cz)
            for (int cy = b.y0; cy <= b.y_last(cz); ++cy) {
                uint32_t k, e;
                b.row(g, start, cz, cy, k, e);
                for (; k < e; ++k) {
                    const float4 s = seeds[k];
                    const float d = sqdist3(x, y, z, s.x, s.y, s.z);
                    const int id = __float_as_int(s.w);
                    if (d < r2 && id < best) best = id, bd = d;  // FLANN's radius set keeps dist < radius [U]
                }
            }
    }
    seed_out[i] = best == 0x7fffffff ? -1 : best;
    if (d2_out) d2_out[i] = bd;
}

__global__ void no_seed_kernel(int64_t n, int32_t* __restrict__ seed_out, float* __restrict__ d2_out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    seed_out[i] = -1;
    if (d2_out) d2_out[i] = 0.f;
}

// ---- flags and stable compaction (flags[n] = 0: the scan over n + 1 entries leaves the count at pos[n]) ---
// PCL's comparisons: removed when (!negative && d > thr) || (negative && d <= thr); a NaN threshold keeps all
__global__ void sor_flag_kernel(const float* __restrict__ dist, int64_t n, double thr, int negative,
                                uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0;
    if (i < n) {
        const double d = (double)fmaxf(dist[i], 0.f);  // not counted: distance 0
        f = ((!negative && d > thr) || (negative && d <= thr)) ? 0u : 1u;
    }
    flags[i] = f;
}

// mode 0: intensity > a (seeds); 1: intensity != 0 and a seed claimed it (segmented); 2: intensity != 0 and
// none did (remained); 3: not (intensity < a and a seed within the radius) (the noise_thres step)
__global__ void slam_flag_kernel(const float* __restrict__ p, int64_t n, int mode, float a,
                                 const int32_t* __restrict__ seed, uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0;
    if (i < n) {
        const float in = p[4 * (size_t)i + 3];
        if (mode == 0) f = in > a;
        else if (mode == 1) f = in != 0.0f && seed[i] >= 0;
        else if (mode == 2) f = in != 0.0f && seed[i] < 0;
        else f = !(in < a && seed[i] >= 0);
    }
    flags[i] = f;
}

__global__ void scatter_rows_kernel(const float* __restrict__ in, int64_t n, int stride, int out_stride,
                                    const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                    float* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const float* q = in + (size_t)i * stride;
    float* o = out + (size_t)pos[i] * out_stride;
    for (int f = 0; f < out_stride; ++f) o[f] = q[f];
}

// segmented points: input index and the sort key (claiming seed, d2 bits); sorted stably from ascending
// index, ties end in index order
__global__ void seg_scatter_kernel(int64_t n, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                   const int32_t* __restrict__ seed, const float* __restrict__ d2,
                                   uint32_t* __restrict__ idx, uint64_t* __restrict__ k64) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !flags[i]) return;
    idx[pos[i]] = (uint32_t)i;
    k64[pos[i]] = ((uint64_t)(uint32_t)seed[i] << 32) | __float_as_uint(d2[i]);
}

__global__ void gather_rows4_kernel(const float* __restrict__ in, const uint32_t* __restrict__ idx, int64_t m,
                                    float* __restrict__ out) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= m) return;
    reinterpret_cast<float4*>(out)[t] = reinterpret_cast<const float4*>(in)[idx[t]];
}

}  // namespace

// ---- host side (dn_*: shared with lio_cluster.hip through lio_denoise.hpp) ------------------------------
int dn_sort32(DenoiseBuf& b, int64_t n, int bits, hipStream_t st) {
    return cub_sort_pairs(b.tmp, b.tmp_bytes, kFixedScratch, b.keys, b.keys_alt, b.vals, b.vals_alt, n, bits, st);
}

int dn_sort64(DenoiseBuf& b, int64_t n, int bits, hipStream_t st) {
    return cub_sort_pairs(b.tmp, b.tmp_bytes, kFixedScratch, b.k64, b.k64_alt, b.idx, b.idx_alt, n, bits, st);
}

// pos = exclusive scan of flags[0 .. n]; *count = pos[n].  Waits for the stream.
int dn_scan_count(DenoiseBuf& b, int64_t n, int64_t* count, hipStream_t st) {
    const int rc = cub_exclusive_sum(b.tmp, b.tmp_bytes, kFixedScratch, b.flags, b.pos, n + 1, st);
    if (rc) return rc;
    LIO_HIP(hipMemcpyAsync(b.h_cnt, b.pos + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    *count = b.h_cnt[0];
    return 0;
}

int dn_bit_width(uint32_t v) {
    int b = 0;
    while (v) ++b, v >>= 1;
    return std::max(b, 1);
}

// the grid of the finite points of d_pts in b.g4 / b.start / b.geom, enqueued (no host wait)
int dn_build_grid(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, float target, float fixed_cell,
                  hipStream_t st) {
    const uint32_t cells_cap = (uint32_t)(n + 64);
    const int nbp = (int)std::min<int64_t>(kDnPartBlocks, (n + 255) / 256);
    dn_minmax_kernel<<<nbp, 256, 0, st>>>(d_pts, n, stride, b.part);
    dn_geom_kernel<<<1, 256, 0, st>>>(b.part, nbp, n, target, fixed_cell, cells_cap, b.geom);
    dn_key_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, stride, b.geom, cells_cap, b.keys, b.vals);
    const int rc = dn_sort32(b, n, dn_bit_width(cells_cap), st);
    if (rc) return rc;
    dn_start_kernel<<<nblk((int64_t)cells_cap + 1), 256, 0, st>>>(b.keys_alt, n, cells_cap, b.start);
    dn_gather_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, stride, b.vals_alt, b.g4);
    LIO_HIP(hipGetLastError());
    return 0;
}

void denoise_free(DenoiseBuf& b) {
    dev_free(&b.arena);
    host_free(&b.h_dist, &b.h_cnt);
    b = DenoiseBuf{};
}

int denoise_reserve(DenoiseBuf& b, int64_t n) {
    if (n >= (int64_t)0x7fffff00) return kArg;
    if (n <= b.cap && b.arena) return kOk;
    const int64_t c = std::min<int64_t>(grown<int64_t>(n, b.cap, 4096), 0x7fffff00);
    dev_free(&b.arena);
    host_free(&b.h_dist);
    b.arena_bytes = 0, b.h_dist_bytes = 0, b.cap = 0;
    if (!b.h_cnt) {
        count_alloc();
        if (hipHostMalloc(&b.h_cnt, 64) != hipSuccess) return kNoMem;
    }
    // the sort / scan scratch for the whole capacity, so a call up to it never allocates
    size_t s32 = 0, s64 = 0, sx = 0;
    LIO_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, s32, b.keys, b.keys_alt, b.vals, b.vals_alt, (int)c, 0, 32));
    LIO_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, s64, b.k64, b.k64_alt, b.idx, b.idx_alt, (int)c, 0, 64));
    LIO_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, sx, b.flags, b.pos, (int)(c + 1)));
    const size_t tmp = std::max(std::max(s32, s64), sx) + 256;
    const size_t C = (size_t)c;
    auto fields = [&](Carver& at) {  // the arena's fields, once each, in arena order
        at(b.keys, C), at(b.keys_alt, C), at(b.vals, C), at(b.vals_alt, C);
        at(b.start, C + 66), at(b.g4, C), at(b.part, 6 * kDnPartBlocks), at(b.geom, 1);
        at(b.dist, C), at(b.flags, C + 1), at(b.pos, C + 1);
        at(b.seeds_xyz, 3 * C), at(b.seed_id, C), at(b.seed_d2, C), at(b.idx, C), at(b.idx_alt, C);
        at(b.k64, C), at(b.k64_alt, C), at(b.cloud_a, 4 * C), at(b.cloud_b, 4 * C), at(b.tmp, tmp);
    };
    int rc = reserve_arena(&b.arena, b.arena_bytes, fields, 0);
    if (!rc) rc = grow_pinned(&b.h_dist, b.h_dist_bytes, C * sizeof(float), 0);  // exactly the capacity, with the arena
    if (rc) {
        dev_free(&b.arena);
        b.arena_bytes = 0;
        return rc;
    }
    b.tmp_bytes = tmp;
    b.cap = c;
    return kOk;
}

int sor_distances(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, int mean_k, float* d_dist, hipStream_t st) {
    if (n <= 0) return 0;
    if (stride < 3 || stride > 8 || mean_k < 1 || mean_k > kMaxMeanK) return kArg;
    int rc = denoise_reserve(b, n);
    if (rc) return rc;
    rc = dn_build_grid(b, d_pts, n, stride, (float)(mean_k + 1), 0.f, st);
    if (rc) return rc;
    sor_knn_kernel<<<(unsigned)n, 64, 0, st>>>(b.g4, b.start, b.geom, n, mean_k, d_dist);
    LIO_HIP(hipGetLastError());
    return 0;
}

int sor_filter(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, int mean_k, double stddev_mul, bool negative,
               float* d_out, int64_t* n_out, float* h_dist_out, double* stats4, hipStream_t st) {
    *n_out = 0;
    if (stride < 3 || stride > 8 || mean_k < 1 || mean_k > kMaxMeanK) return kArg;
    double sum = 0.0, sq_sum = 0.0;
    int64_t nv = 0;
    if (n > 0) {
        int rc = denoise_reserve(b, n);  // before b.dist is read: the arena's pointers are set here
        if (rc) return rc;
        rc = sor_distances(b, d_pts, n, stride, mean_k, b.dist, st);
        if (rc) return rc;
        LIO_HIP(hipMemcpyAsync(b.h_dist, b.dist, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
        LIO_HIP(hipStreamSynchronize(st));
        // PCL's loop [U], in index order: the float product d * d is promoted, the sums are double
        for (int64_t i = 0; i < n; ++i) {
            float d = b.h_dist[i];
            if (d < 0.f) d = 0.f;
            else ++nv;
            sum += d;
            const float dd = d * d;
            sq_sum += (double)dd;
            if (h_dist_out) h_dist_out[i] = d;
        }
    }
    const double dn = (double)nv;
    const double mean = sum / dn;
    const double variance = (sq_sum - sum * sum / dn) / (dn - 1.0);
    const double stddev = std::sqrt(variance);
    const double thr = mean + stddev_mul * stddev;
    if (stats4) stats4[0] = mean, stats4[1] = stddev, stats4[2] = thr, stats4[3] = dn;
    if (n <= 0) return 0;
    sor_flag_kernel<<<nblk(n + 1), 256, 0, st>>>(b.dist, n, thr, negative ? 1 : 0, b.flags);
    const int rc = dn_scan_count(b, n, n_out, st);
    if (rc) return rc;
    scatter_rows_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, stride, stride, b.flags, b.pos, d_out);
    LIO_HIP(hipGetLastError());
    return 0;
}

int radius_first_seed(DenoiseBuf& b, const float* d_pts, int64_t n, int stride, const float* d_seeds_xyz, int64_t ns,
                      float radius, int32_t* d_seed, float* d_d2, hipStream_t st) {
    if (n <= 0) return 0;
    if (stride < 3 || stride > 8 || ns < 0 || !(radius >= 0.f) || !std::isfinite(radius)) return kArg;
    int rc = denoise_reserve(b, std::max(n, ns));
    if (rc) return rc;
    if (ns == 0) {
        no_seed_kernel<<<nblk(n), 256, 0, st>>>(n, d_seed, d_d2);
        LIO_HIP(hipGetLastError());
        return 0;
    }
    rc = dn_build_grid(b, d_seeds_xyz, ns, 3, 0.f, radius > 0.f ? radius : 1.f, st);
    if (rc) return rc;
    const float r2 = (float)((double)radius * (double)radius);  // PCL passes radius * radius cast to float [U]
    radius_seed_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, stride, b.g4, b.start, b.geom, radius, r2, d_seed, d_d2);
    LIO_HIP(hipGetLastError());
    return 0;
}

int denoise_slam_map(DenoiseBuf& b, const float* d_pts, int64_t n, const DenoiseParams& p, float* d_out,
                     int64_t* n_out, int64_t* counts5, hipStream_t st) {
    *n_out = 0;
    int64_t cnt[5] = {0, 0, 0, 0, 0};
    if (counts5) std::memcpy(counts5, cnt, sizeof(cnt));
    if (p.mean_k < 1 || p.mean_k > kMaxMeanK || !(p.cluster_seed_radius >= 0.f) || !(p.denoise_radius >= 0.f) ||
        !std::isfinite(p.cluster_seed_radius) || !std::isfinite(p.denoise_radius))
        return kArg;
    if (n <= 0) return 0;
    int rc = denoise_reserve(b, n);
    if (rc) return rc;
    // 1. seeds: intensity > seed_thres, in input order
    slam_flag_kernel<<<nblk(n + 1), 256, 0, st>>>(d_pts, n, 0, p.seed_thres, nullptr, b.flags);
    if ((rc = dn_scan_count(b, n, &cnt[0], st))) return rc;
    scatter_rows_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, 4, 3, b.flags, b.pos, b.seeds_xyz);
    // 2. segmented: intensity != 0 and claimed by the lowest seed within cluster_seed_radius; the reference's
    //    loop emits them seed by seed, each seed's in ascending distance (ties: index order, this library's rule)
    if ((rc = radius_first_seed(b, d_pts, n, 4, b.seeds_xyz, cnt[0], p.cluster_seed_radius, b.seed_id, b.seed_d2, st)))
        return rc;
    slam_flag_kernel<<<nblk(n + 1), 256, 0, st>>>(d_pts, n, 1, 0.f, b.seed_id, b.flags);
    if ((rc = dn_scan_count(b, n, &cnt[1], st))) return rc;
    if (cnt[1] > 0) {
        seg_scatter_kernel<<<nblk(n), 256, 0, st>>>(n, b.flags, b.pos, b.seed_id, b.seed_d2, b.idx, b.k64);
        if ((rc = dn_sort64(b, cnt[1], 32 + dn_bit_width((uint32_t)cnt[0]), st))) return rc;
        gather_rows4_kernel<<<nblk(cnt[1]), 256, 0, st>>>(d_pts, b.idx_alt, cnt[1], b.cloud_a);
        // 4. denoise_map: SOR on segmented, then drop intensity < noise_thres with a seed within denoise_radius
        if ((rc = sor_filter(b, b.cloud_a, cnt[1], 4, p.mean_k, (double)p.stddev_mul, false, b.cloud_b, &cnt[2], nullptr,
                             nullptr, st)))
            return rc;
        if (cnt[2] > 0) {
            auto* nearby = reinterpret_cast<int32_t*>(b.idx);  // the sort's input is spent
            if ((rc = radius_first_seed(b, b.cloud_b, cnt[2], 4, b.seeds_xyz, cnt[0], p.denoise_radius, nearby, nullptr, st)))
                return rc;
            slam_flag_kernel<<<nblk(cnt[2] + 1), 256, 0, st>>>(b.cloud_b, cnt[2], 3, p.noise_thres, nearby, b.flags);
            if ((rc = dn_scan_count(b, cnt[2], &cnt[3], st))) return rc;
            scatter_rows_kernel<<<nblk(cnt[2]), 256, 0, st>>>(b.cloud_b, cnt[2], 4, 4, b.flags, b.pos, d_out);
        }
    }
    // 3. remained: intensity != 0 and not segmented, in input order, behind the denoised points
    slam_flag_kernel<<<nblk(n + 1), 256, 0, st>>>(d_pts, n, 2, 0.f, b.seed_id, b.flags);
    if ((rc = dn_scan_count(b, n, &cnt[4], st))) return rc;
    scatter_rows_kernel<<<nblk(n), 256, 0, st>>>(d_pts, n, 4, 4, b.flags, b.pos, d_out + 4 * (size_t)cnt[3]);
    LIO_HIP(hipGetLastError());
    *n_out = cnt[3] + cnt[4];
    if (counts5) std::memcpy(counts5, cnt, sizeof(cnt));
    return 0;
}

}  // namespace lio
