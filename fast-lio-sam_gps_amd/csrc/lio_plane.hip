// lio_plane.hip — RANSAC plane segmentation on gfx950: Open3D's PointCloud::SegmentPlane [U] as the offline
// pipeline calls it for ground removal (post_process/clustering.py:21-28: distance_threshold 0.2, ransac_n 3,
// num_iterations 1000), restated as the contract of lio_segment_plane (include/lio_gpu.h):
//
//   plane      of a triple (p0, p1, p2): the float cross product of p1 - p0 and p2 - p0, normalised; degenerate
//              (skipped) unless its length is finite and > 0 and d is finite
//   score      count of points with float |((a x + b y) + c z) + d| < thr (strict), and the fixed-point sum
//              sq = sum floor(dist^2 * 2^(32 - e)), thr^2 = m 2^e (frexp): an integer sum, the same in any order
//   winner     minimises (-count, sq, hypothesis index)
//
// Launch sequence (every step its own launch; no kernel waits for another workgroup):
//   planes on the host (K tiny float computations on the caller's records) -> upload -> evaluation (the hot
//   kernel: K x n point-plane tests) -> selection (one workgroup) -> inlier flags with the winning plane ->
//   scan (dn_scan_count) -> indices -> double moments about the lowest-index inlier, per-block partials
//   combined in block order -> 3 x 3 eigen solve on the host.
//
// DETERMINISM.  The only cross-workgroup accumulation of the evaluation is integer atomicAdd (device scope:
// the partial sums of a hypothesis come from every XCD), so count and sq do not depend on the schedule; the
// moments are summed by a fixed assignment of inliers to threads, a fixed tree per block and the blocks in
// order.  Repeated calls are bit-identical.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lio_scratch.hpp"
#include "lio_plane.hpp"

namespace lio {

namespace {

using ull = unsigned long long;
typedef float f2v __attribute__((ext_vector_type(2)));

constexpr int kHypBlock = 256;    // hypotheses per workgroup: one per thread
constexpr int kTile = 1024;       // points staged in LDS at a time (12 KiB)
constexpr int kChunk = 2048;      // points per workgroup: 2 M points x 1000 hypotheses = 3908 workgroups
constexpr int kMomBlocks = 256;   // most workgroups of the moment reduction
constexpr int kSelThreads = 1024;

// ---- the evaluation kernel ---------------------------------------------------------------------------
// Thread = hypothesis (its plane in four registers), workgroup = 256 hypotheses x one chunk of points.  The
// workgroup stages a tile of points as x[], y[], z[] in LDS (rows past the chunk's end as NaN: no plane has them
// as inliers, so the inner loop has no bound to test); then every lane reads the SAME tile entries (LDS reads
// of one address broadcast) and tests them against its own plane, two points at a time in packed FP32
// (v_pk_mul_f32 / v_pk_add_f32: per element the contract's mul, mul, add, mul, add, add — no FMA,
// -ffp-contract=off).  count (u32: a chunk holds 2048 points) and sq (u64) stay in registers; one pair of
// integer atomics per thread at the end, none for a hypothesis without inliers in the chunk (a degenerate one
// — NaN plane — never has any).
//
// The squared distance of an inlier is <= thr^2 < 2^e (rounding is monotone), so ldexpf(dd, 32 - e) < 2^32;
// scaling a float by a power of two is exact (a result below the normal range would round, but it is < 1
// and the conversion truncates it to 0 either way), and the conversion of a non-negative float below 2^32
// to uint32 is its floor.
__global__ void __launch_bounds__(kHypBlock) pl_eval_kernel(const float* __restrict__ pts, int64_t n, int stride,
                                                            const float4* __restrict__ planes, int64_t K, float thr, int sh,
                                                            ull* __restrict__ cnt, ull* __restrict__ sq) {
    __shared__ __attribute__((aligned(16))) float sx[kTile], sy[kTile], sz[kTile];
    const int64_t t = blockIdx.y * (int64_t)kHypBlock + threadIdx.x;
    const float4 pl = t < K ? planes[t] : make_float4(NAN, NAN, NAN, NAN);
    const f2v A = {pl.x, pl.x}, B = {pl.y, pl.y}, C = {pl.z, pl.z}, D = {pl.w, pl.w};
    const int64_t c0 = blockIdx.x * (int64_t)kChunk, c1 = c0 + kChunk < n ? c0 + kChunk : n;
    uint32_t count = 0;
    ull s = 0;
    for (int64_t base = c0; base < c1; base += kTile) {
        __syncthreads();  // the readers of the tile before are done
        for (int k = threadIdx.x; k < kTile; k += kHypBlock) {
            const int64_t i = base + k;
            float x = NAN, y = NAN, z = NAN;
            if (i < c1) {
                const float* q = pts + (size_t)i * stride;
                x = q[0], y = q[1], z = q[2];
            }
            sx[k] = x, sy[k] = y, sz[k] = z;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kTile; k += 2) {
            const f2v X = *reinterpret_cast<const f2v*>(sx + k), Y = *reinterpret_cast<const f2v*>(sy + k),
                      Z = *reinterpret_cast<const f2v*>(sz + k);
            const f2v e = ((A * X + B * Y) + C * Z) + D;  // the signed distances of two points
            const f2v ee = e * e;                         // == |e| * |e|
            const bool in0 = fabsf(e.x) < thr, in1 = fabsf(e.y) < thr;  // false for a NaN / infinite distance
            s += (ull)(uint32_t)ldexpf(in0 ? ee.x : 0.f, sh);
            s += (ull)(uint32_t)ldexpf(in1 ? ee.y : 0.f, sh);
            count += (in0 ? 1u : 0u) + (in1 ? 1u : 0u);
        }
    }
    if (t < K && count) {
        atomicAdd(cnt + t, (ull)count);
        atomicAdd(sq + t, s);
    }
}

// (count, sq, t) of a beats (count, sq, t) of b; t < 0: no candidate
__device__ __forceinline__ bool pl_better(ull ca, ull qa, int64_t ta, ull cb, ull qb, int64_t tb) {
    if (ta < 0) return false;
    if (tb < 0) return true;
    if (ca != cb) return ca > cb;
    if (qa != qb) return qa < qb;
    return ta < tb;
}

// one workgroup: the non-degenerate hypothesis that minimises (-count, sq, t)
__global__ void __launch_bounds__(kSelThreads) pl_select_kernel(const float4* __restrict__ planes, const ull* __restrict__ cnt,
                                                                const ull* __restrict__ sq, int64_t K,
                                                                PlaneWinner* __restrict__ win) {
    __shared__ ull s_c[kSelThreads], s_q[kSelThreads];
    __shared__ int64_t s_t[kSelThreads];
    ull bc = 0, bq = 0;
    int64_t bt = -1;
    for (int64_t t = threadIdx.x; t < K; t += kSelThreads) {
        if (planes[t].x != planes[t].x) continue;  // degenerate
        const ull c = cnt[t], q = sq[t];
        if (pl_better(c, q, t, bc, bq, bt)) bc = c, bq = q, bt = t;
    }
    s_c[threadIdx.x] = bc, s_q[threadIdx.x] = bq, s_t[threadIdx.x] = bt;
    __syncthreads();
    for (int o = kSelThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const int j = threadIdx.x + o;
            if (pl_better(s_c[j], s_q[j], s_t[j], s_c[threadIdx.x], s_q[threadIdx.x], s_t[threadIdx.x]))
                s_c[threadIdx.x] = s_c[j], s_q[threadIdx.x] = s_q[j], s_t[threadIdx.x] = s_t[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t t = s_t[0];
        const float4 pl = t >= 0 ? planes[t] : make_float4(0.f, 0.f, 0.f, 0.f);
        win->plane[0] = pl.x, win->plane[1] = pl.y, win->plane[2] = pl.z, win->plane[3] = pl.w;
        win->best = (int32_t)t;
        win->pad = 0;
    }
}

// flags[i] = mask[i] = inlier of the winning plane (flags[n] = 0: the scan leaves the count at pos[n])
__global__ void pl_flag_kernel(const float* __restrict__ pts, int64_t n, int stride, const PlaneWinner* __restrict__ win,
                               float thr, uint32_t* __restrict__ flags, uint8_t* __restrict__ mask) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0;
    if (i < n && win->best >= 0) {
        const float* q = pts + (size_t)i * stride;
        const float dist = fabsf(((win->plane[0] * q[0] + win->plane[1] * q[1]) + win->plane[2] * q[2]) + win->plane[3]);
        f = dist < thr ? 1u : 0u;
    }
    flags[i] = f;
    if (i < n) mask[i] = (uint8_t)f;
}

__global__ void pl_index_kernel(int64_t n, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                int32_t* __restrict__ inliers) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n && flags[i]) inliers[pos[i]] = (int32_t)i;
}

// Double first and second moments of the m >= 1 inliers about the lowest-index one (float -> double differences
// of floats are exact).  Workgroup b takes the inliers [b per, (b + 1) per), thread k of it every 256th from
// b per + k; the 256 thread sums are combined by a fixed tree: part[9 b ..].
__global__ void __launch_bounds__(256) pl_moment_kernel(const float* __restrict__ pts, int stride,
                                                        const int32_t* __restrict__ inliers, int64_t m, int64_t per,
                                                        double* __restrict__ part) {
    __shared__ double sh[9][256];
    const float* r = pts + (size_t)inliers[0] * stride;
    const double rx = r[0], ry = r[1], rz = r[2];
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t j0 = blockIdx.x * per, j1 = j0 + per < m ? j0 + per : m;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        const float* q = pts + (size_t)inliers[j] * stride;
        const double dx = (double)q[0] - rx, dy = (double)q[1] - ry, dz = (double)q[2] - rz;
        a[0] += dx, a[1] += dy, a[2] += dz;
        a[3] += dx * dx, a[4] += dx * dy, a[5] += dx * dz;
        a[6] += dy * dy, a[7] += dy * dz, a[8] += dz * dz;
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) sh[c][threadIdx.x] = a[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int c = 0; c < 9; ++c) sh[c][threadIdx.x] += sh[c][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 9) part[9 * (size_t)blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
}

// the partials in block order (staged in LDS first: the sums are serial, the loads need not be); mom[9] = the
// reference index.  One workgroup of kMomBlocks threads.
__global__ void __launch_bounds__(kMomBlocks) pl_moment_sum_kernel(const double* __restrict__ part, int nb,
                                                                   const int32_t* __restrict__ inliers,
                                                                   double* __restrict__ mom) {
    __shared__ double sh[9][kMomBlocks];
    if ((int)threadIdx.x < nb)
#pragma unroll
        for (int c = 0; c < 9; ++c) sh[c][threadIdx.x] = part[9 * (size_t)threadIdx.x + c];
    __syncthreads();
    if (threadIdx.x < 9) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += sh[threadIdx.x][b];
        mom[threadIdx.x] = s;
    } else if (threadIdx.x == 9) {
        mom[9] = (double)inliers[0];
    }
}

int plane_reserve(PlaneBuf& p, int64_t n, int64_t K) {
    if (!p.h_pin) {
        count_alloc();
        if (hipHostMalloc(&p.h_pin, 256) != hipSuccess) {
            p.h_pin = nullptr;
            return kNoMem;
        }
    }
    if (n <= p.cap_n && K <= p.cap_k && p.arena) return kOk;
    const int64_t cn = n <= p.cap_n ? p.cap_n : grown<int64_t>(n, p.cap_n, 4096);
    const int64_t ck = K <= p.cap_k ? p.cap_k : grown<int64_t>(K, p.cap_k, 1024);
    dev_free(&p.arena);
    p.arena_bytes = 0, p.cap_n = 0, p.cap_k = 0;
    const size_t N = (size_t)cn, H = (size_t)ck;
    auto fields = [&](Carver& at) {  // the arena's fields, once each, in arena order
        at(p.planes, H), at(p.cnt, H), at(p.sq, H), at(p.mask, N), at(p.inliers, N);
        at(p.part, 9 * kMomBlocks), at(p.mom, 10), at(p.win, 1);
    };
    const int rc = reserve_arena(&p.arena, p.arena_bytes, fields, 0);
    if (rc) return rc;
    p.cap_n = cn, p.cap_k = ck;
    return kOk;
}

// cyclic Jacobi on a symmetric 3 x 3 matrix: A becomes diagonal, the columns of V the eigenvectors
void jacobi3(double A[3][3], double V[3][3]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-60 * dia)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq, A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk, A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// Open3D's GetPlaneFromPoints [U]: the eigenvector of the smallest eigenvalue of the inliers' covariance, signed
// like the winner's normal; d = -n . centroid
void plane_refit(const double* mom, int64_t m, const float* ref, const float* win, double* out) {
    const double inv = 1.0 / (double)m;
    const double mx = mom[0] * inv, my = mom[1] * inv, mz = mom[2] * inv;
    double A[3][3], V[3][3];
    A[0][0] = mom[3] * inv - mx * mx, A[0][1] = A[1][0] = mom[4] * inv - mx * my, A[0][2] = A[2][0] = mom[5] * inv - mx * mz;
    A[1][1] = mom[6] * inv - my * my, A[1][2] = A[2][1] = mom[7] * inv - my * mz, A[2][2] = mom[8] * inv - mz * mz;
    jacobi3(A, V);
    int k = 0;
    if (A[1][1] < A[k][k]) k = 1;
    if (A[2][2] < A[k][k]) k = 2;
    double nx = V[0][k], ny = V[1][k], nz = V[2][k];
    const double len = std::sqrt((nx * nx + ny * ny) + nz * nz);
    nx /= len, ny /= len, nz /= len;
    if ((nx * (double)win[0] + ny * (double)win[1]) + nz * (double)win[2] < 0.0) nx = -nx, ny = -ny, nz = -nz;
    const double cx = (double)ref[0] + mx, cy = (double)ref[1] + my, cz = (double)ref[2] + mz;
    out[0] = nx, out[1] = ny, out[2] = nz, out[3] = -((nx * cx + ny * cy) + nz * cz);
}

inline uint64_t mix64(uint64_t z) {  // splitmix64's output function
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

void plane_free(PlaneBuf& p) {
    dev_free(&p.arena);
    host_free(&p.h_pin);
    p = PlaneBuf{};
}

void plane_sample_triples(uint64_t seed, int64_t n, int64_t K, int32_t* out) {
    const uint64_t N = (uint64_t)n;
    auto r = [&](uint64_t c) { return mix64(seed + (c + 1) * 0x9E3779B97F4A7C15ull); };
    for (int64_t t = 0; t < K; ++t) {
        const uint64_t c = 3 * (uint64_t)t;
        const uint64_t i0 = r(c) % N;
        uint64_t i1 = r(c + 1) % (N - 1);
        if (i1 >= i0) ++i1;
        uint64_t i2 = r(c + 2) % (N - 2);
        const uint64_t lo = std::min(i0, i1), hi = std::max(i0, i1);
        if (i2 >= lo) ++i2;
        if (i2 >= hi) ++i2;
        out[3 * t] = (int32_t)i0, out[3 * t + 1] = (int32_t)i1, out[3 * t + 2] = (int32_t)i2;
    }
}

bool plane_triples_valid(const int32_t* tri, int64_t K, int64_t n) {
    for (int64_t t = 0; t < K; ++t) {
        const int64_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        if (a < 0 || a >= n || b < 0 || b >= n || c < 0 || c >= n || a == b || a == c || b == c) return false;
    }
    return true;
}

void plane_hypotheses(const float* pts, int stride, const int32_t* tri, int64_t K, float* planes4, uint8_t* deg) {
    for (int64_t t = 0; t < K; ++t) {
        const float* p0 = pts + (size_t)tri[3 * t] * stride;
        const float* p1 = pts + (size_t)tri[3 * t + 1] * stride;
        const float* p2 = pts + (size_t)tri[3 * t + 2] * stride;
        const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
        const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float len = std::sqrt((nx * nx + ny * ny) + nz * nz);
        const float a = nx / len, b = ny / len, c = nz / len;
        const float d = -((a * p0[0] + b * p0[1]) + c * p0[2]);
        const bool ok = std::isfinite(len) && len > 0.f && std::isfinite(d);
        deg[t] = ok ? 0 : 1;
        float* o = planes4 + 4 * t;
        if (ok) o[0] = a, o[1] = b, o[2] = c, o[3] = d;
        else o[0] = o[1] = o[2] = o[3] = NAN;
    }
}

int segment_plane(DenoiseBuf& b, PlaneBuf& p, const float* d_pts, const float* h_pts, int64_t n, int stride, float thr,
                  int64_t K, bool want_refit, PlaneResult* out, hipStream_t st) {
    *out = PlaneResult{};
    const float thr2 = thr * thr;
    if (n < 1 || n >= (int64_t)1 << 31 || K < 1 || K > (int64_t)1 << 20 || stride < 3 || stride > 8 || !(thr > 0.f) ||
        !std::isfinite(thr2) || (int64_t)p.h_planes.size() < 4 * K)
        return kArg;
    int rc = denoise_reserve(b, n);
    if (!rc) rc = plane_reserve(p, n, K);
    if (rc) return rc;
    int e = 0;
    (void)std::frexp(thr2, &e);
    LIO_HIP(hipMemcpyAsync(p.planes, p.h_planes.data(), (size_t)K * 16, hipMemcpyHostToDevice, st));
    LIO_HIP(hipMemsetAsync(p.cnt, 0, (size_t)K * 8, st));
    LIO_HIP(hipMemsetAsync(p.sq, 0, (size_t)K * 8, st));
    const dim3 grid((unsigned)((n + kChunk - 1) / kChunk), (unsigned)((K + kHypBlock - 1) / kHypBlock));
    pl_eval_kernel<<<grid, kHypBlock, 0, st>>>(d_pts, n, stride, p.planes, K, thr, 32 - e, p.cnt, p.sq);
    pl_select_kernel<<<1, kSelThreads, 0, st>>>(p.planes, p.cnt, p.sq, K, p.win);
    pl_flag_kernel<<<nblk(n + 1), 256, 0, st>>>(d_pts, n, stride, p.win, thr, b.flags, p.mask);
    LIO_HIP(hipMemcpyAsync(p.h_pin, p.win, sizeof(PlaneWinner), hipMemcpyDeviceToHost, st));
    int64_t m = 0;
    if ((rc = dn_scan_count(b, n, &m, st))) return rc;  // waits: the winner is on the host too
    PlaneWinner w;
    std::memcpy(&w, p.h_pin, sizeof(w));
    std::memcpy(out->plane, w.plane, sizeof(w.plane));
    out->best = w.best;
    out->n_inliers = m;
    for (int k = 0; k < 4; ++k) out->refit[k] = (double)w.plane[k];
    if (m > 0) {
        pl_index_kernel<<<nblk(n), 256, 0, st>>>(n, b.flags, b.pos, p.inliers);
        if (want_refit && m >= 3) {
            const int nb = (int)std::min<int64_t>(kMomBlocks, (m + 255) / 256);
            const int64_t per = (m + nb - 1) / nb;
            double* h_mom = reinterpret_cast<double*>(static_cast<uint8_t*>(p.h_pin) + 64);
            pl_moment_kernel<<<nb, 256, 0, st>>>(d_pts, stride, p.inliers, m, per, p.part);
            pl_moment_sum_kernel<<<1, kMomBlocks, 0, st>>>(p.part, nb, p.inliers, p.mom);
            LIO_HIP(hipMemcpyAsync(h_mom, p.mom, 10 * sizeof(double), hipMemcpyDeviceToHost, st));
            LIO_HIP(hipStreamSynchronize(st));
            plane_refit(h_mom, m, h_pts + (size_t)(int64_t)h_mom[9] * stride, w.plane, out->refit);
        }
    }
    LIO_HIP(hipGetLastError());
    return 0;
}

}  // namespace lio
