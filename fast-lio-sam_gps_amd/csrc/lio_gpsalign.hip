// lio_gpsalign.hip — GPS-to-SLAM trajectory alignment and map georeferencing on gfx950: the reference's offline
// GPS leg (post_process/align_slam_gps_icp.py:81-156 icp_alignment, georef_mapmatch.py:115-135
// align_trajectories_horn, post_process/georeference_pcd.py:236-244), restated as IEEE double + - x / sqrt in a
// written order (include/lio_gpu.h: lio_gps_align, lio_similarity2d_fit, lio_georeference_xy).  The file is
// compiled with -ffp-contract=off, host and device: no multiply-add is fused anywhere.
//
// TREE(v), the only summation: blocks of 256 consecutive elements (the last padded with +0.0); inside a block
// a[i] = a[i] + a[i + w] for i < w, w = 128, 64, ..., 1; the block sums added in ascending block order into a
// scalar that starts at 0.0.  A block IS a 256-thread workgroup: w = 128 and 64 are LDS steps, 32 ... 1 are
// __shfl_down in wave 0 (block_tree), and the host adds the block sums (tree_total).
//
// Launch sequence of gps_align (every step its own launch, nothing waits for another workgroup):
//   start      ga_sum_xy (cA, cB) -> ga_centre (Ac, Bc, the squared norms) -> ga_scale (S = s0 Ac)
//   iteration  ga_nn (grid: source blocks x target chunks; targets through LDS in tiles, every lane reads the
//              same LDS address, a broadcast; strict < over ascending k keeps the lowest index) ->
//              ga_merge (chunks in ascending order, strict <: the lower k wins an equal d2; nn, matched target,
//              dist = sqrt(d2)) -> ga_stats1 (TREE of Sx, Sy, Mx, My, dist) -> host: cs, cd, mean_error ->
//              ga_stats2 (TREE of the six centred moments) -> host: the six scalar steps (rotation, scale,
//              translation; g++-equal arithmetic, sqrt and / correctly rounded) -> ga_apply.
// The host reads the block sums after each statistics pass (three short waits per iteration).  The chunk width
// (ga_chunk_width) only decides which workgroup looks at which targets: the minimum under (d2, k) is the same.
//
// similarity2d_fit runs ga_stats1 / ga_stats2 and the same host steps on given pairs; georeference_xy is one
// memory-bound pass over the records.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "lio_scratch.hpp"
#include "lio_gpsalign.hpp"

namespace lio {

namespace {

constexpr int kGaMaxSums = 6;

// TREE inside one block for K values per thread: the block sums in thread 0 (v[] of the other threads is scratch).
// s: K x 256 doubles of LDS.
template <int K>
__device__ __forceinline__ void block_tree(double (&v)[K], double* s) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) s[k * 256 + t] = v[k];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k * 256 + t] = s[k * 256 + t] + s[k * 256 + t + 128];
    }
    __syncthreads();
    if (t < 64) {  // wave 0
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double a = s[k * 256 + t] + s[k * 256 + t + 64];
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) a = a + __shfl_down(a, w, 64);  // lanes i < w hold a[i] + a[i + w]
            v[k] = a;
        }
    }
}

template <int K>
__device__ __forceinline__ void store_block_sums(const double (&v)[K], double* part, int64_t nb) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[k * nb + blockIdx.x] = v[k];
    }
}

// part[0 .. nb) = block sums of x, part[nb .. 2 nb) of y
__global__ void __launch_bounds__(256) ga_sum_xy_kernel(const double2* __restrict__ p, int64_t n, double* __restrict__ part,
                                                        int64_t nb) {
    __shared__ double s[2 * 256];
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (j < n) {
        const double2 q = p[j];
        v[0] = q.x, v[1] = q.y;
    }
    block_tree<2>(v, s);
    store_block_sums<2>(v, part, nb);
}

// out = p - c; part = block sums of (ox ox + oy oy)
__global__ void __launch_bounds__(256) ga_centre_kernel(const double2* __restrict__ p, int64_t n, double cx, double cy,
                                                        double2* __restrict__ out, double* __restrict__ part, int64_t nb) {
    __shared__ double s[256];
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    double v[1] = {0.0};
    if (j < n) {
        const double2 q = p[j];
        const double ox = q.x - cx, oy = q.y - cy;
        out[j] = make_double2(ox, oy);
        v[0] = ox * ox + oy * oy;
    }
    block_tree<1>(v, s);
    store_block_sums<1>(v, part, nb);
}

__global__ void __launch_bounds__(256) ga_scale_kernel(double2* p, int64_t n, double s0) {
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (j >= n) return;
    const double2 q = p[j];
    p[j] = make_double2(s0 * q.x, s0 * q.y);
}

// One thread per source point j, one workgroup column per target chunk [blockIdx.y chunk, + chunk): the chunk's
// nearest target under (d2, k) into part_d2 / part_k [blockIdx.y n + j].  An empty comparison (every d2 +inf)
// leaves the chunk's first index with d2 = +inf.
__global__ void __launch_bounds__(256) ga_nn_kernel(const double2* __restrict__ S, int64_t n, const double2* __restrict__ D,
                                                    int64_t m, int64_t chunk, double* __restrict__ part_d2,
                                                    int32_t* __restrict__ part_k) {
    __shared__ double2 tile[kGaTile];
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    const int64_t k0 = blockIdx.y * chunk, k1 = k0 + chunk < m ? k0 + chunk : m;
    const double2 q = j < n ? S[j] : make_double2(0.0, 0.0);
    double best = INFINITY;
    int32_t bk = (int32_t)k0;
    for (int64_t t0 = k0; t0 < k1; t0 += kGaTile) {  // block-uniform
        const int cnt = k1 - t0 < kGaTile ? (int)(k1 - t0) : kGaTile;
        __syncthreads();  // the previous tile's readers are done
        for (int i = threadIdx.x; i < cnt; i += 256) tile[i] = D[t0 + i];
        __syncthreads();
        const int32_t base = (int32_t)t0;
        int i = 0;
        for (; i + 4 <= cnt; i += 4) {
            double d2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double2 t = tile[i + u];
                const double dx = q.x - t.x, dy = q.y - t.y;
                d2[u] = dx * dx + dy * dy;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (d2[u] < best) best = d2[u], bk = base + i + u;
        }
        for (; i < cnt; ++i) {
            const double2 t = tile[i];
            const double dx = q.x - t.x, dy = q.y - t.y;
            const double d2 = dx * dx + dy * dy;
            if (d2 < best) best = d2, bk = base + i;
        }
    }
    if (j < n) {
        part_d2[blockIdx.y * n + j] = best;
        part_k[blockIdx.y * n + j] = bk;
    }
}

// the chunks' answers in ascending chunk order, strict <: the lower k keeps an equal d2
__global__ void __launch_bounds__(256) ga_merge_kernel(const double* __restrict__ part_d2, const int32_t* __restrict__ part_k,
                                                       int64_t n, int nchunks, const double2* __restrict__ D,
                                                       int32_t* __restrict__ nn, double2* __restrict__ M,
                                                       double* __restrict__ dist) {
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (j >= n) return;
    double best = part_d2[j];
    int32_t bk = part_k[j];
    for (int c = 1; c < nchunks; ++c) {
        const double d2 = part_d2[c * n + j];
        const int32_t k = part_k[c * n + j];
        if (d2 < best) best = d2, bk = k;
    }
    nn[j] = bk;
    M[j] = D[bk];
    dist[j] = __dsqrt_rn(best);
}

// TREE of Sx, Sy, Mx, My (and dist): part[k nb + block]
template <bool DIST>
__global__ void __launch_bounds__(256) ga_stats1_kernel(const double2* __restrict__ S, const double2* __restrict__ M,
                                                        const double* __restrict__ dist, int64_t n,
                                                        double* __restrict__ part, int64_t nb) {
    constexpr int K = DIST ? 5 : 4;
    __shared__ double s[K * 256];
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    double v[K] = {};
    if (j < n) {
        const double2 a = S[j], b = M[j];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
        if constexpr (DIST) v[4] = dist[j];
    }
    block_tree<K>(v, s);
    store_block_sums<K>(v, part, nb);
}

// TREE of ax bx, ax by, ay bx, ay by, ax ax + ay ay, bx bx + by by with a = S - cs, b = M - cd
__global__ void __launch_bounds__(256) ga_stats2_kernel(const double2* __restrict__ S, const double2* __restrict__ M, int64_t n,
                                                        double csx, double csy, double cdx, double cdy,
                                                        double* __restrict__ part, int64_t nb) {
    __shared__ double s[6 * 256];
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    double v[6] = {};
    if (j < n) {
        const double2 p = S[j], q = M[j];
        const double ax = p.x - csx, ay = p.y - csy, bx = q.x - cdx, by = q.y - cdy;
        v[0] = ax * bx, v[1] = ax * by, v[2] = ay * bx, v[3] = ay * by;
        v[4] = ax * ax + ay * ay;
        v[5] = bx * bx + by * by;
    }
    block_tree<6>(v, s);
    store_block_sums<6>(v, part, nb);
}

// S <- (sc (c Sx - s Sy) + tx, sc (s Sx + c Sy) + ty)
__global__ void __launch_bounds__(256) ga_apply_kernel(double2* S, int64_t n, double sc, double c, double s, double tx,
                                                       double ty) {
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (j >= n) return;
    const double2 p = S[j];
    S[j] = make_double2(sc * (c * p.x - s * p.y) + tx, sc * (s * p.x + c * p.y) + ty);
}

// georeference_pcd.py:236-244 per record, in double from the float x, y; the other fields bit-copied
__global__ void __launch_bounds__(256) ga_georef_kernel(const float* __restrict__ in, int64_t n, int stride, double r00,
                                                        double r01, double r10, double r11, double scale, double tx,
                                                        double ty, double ox, double oy, float* __restrict__ out,
                                                        double2* __restrict__ xy) {
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(in) + j * stride;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out) + j * stride;
    const double x = (double)in[j * stride], y = (double)in[j * stride + 1];
    const double gx = ((x * r00 + y * r01) * scale + tx) - ox;
    const double gy = ((x * r10 + y * r11) * scale + ty) - oy;
    out[j * stride] = (float)gx;
    out[j * stride + 1] = (float)gy;
    for (int f = 2; f < stride; ++f) dst[f] = src[f];
    if (xy) xy[j] = make_double2(gx, gy);
}

// ---- host ------------------------------------------------------------------------------------------
int64_t nblocks(int64_t n) { return (n + 255) / 256; }

int ga_reserve(GpsAlignBuf& g, int64_t n, int64_t m, int64_t nchunks) {
    const int64_t nb = nblocks(std::max(n, m));
    auto fields = [&](Carver& c) {
        c(g.a_in, (size_t)n);
        c(g.b_in, (size_t)m);
        c(g.d, (size_t)m);
        c(g.mt, (size_t)n);
        c(g.dist, (size_t)n);
        c(g.nn, (size_t)n);
        c(g.part_d2, (size_t)(nchunks * n));
        c(g.part_k, (size_t)(nchunks * n));
        c(g.part, (size_t)(kGaMaxSums * nb));
    };
    const int rc = reserve_arena(&g.arena, g.arena_bytes, fields);
    if (rc) return rc;
    return grow_pinned(&g.h_part, g.h_bytes, (size_t)(kGaMaxSums * nb) * sizeof(double), (size_t)1 << 16);
}

// the block sums of k TREEs to the host, each added in ascending block order from 0.0
int tree_totals(GpsAlignBuf& g, int k, int64_t nb, double* tot, hipStream_t st) {
    LIO_HIP(hipGetLastError());
    LIO_HIP(hipMemcpyAsync(g.h_part, g.part, (size_t)(k * nb) * sizeof(double), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < k; ++q) {
        double t = 0.0;
        for (int64_t b = 0; b < nb; ++b) t = t + g.h_part[q * nb + b];
        tot[q] = t;
    }
    return kOk;
}

struct Step {  // one iteration's similarity: steps 2-5
    double mean_error = 0, csx = 0, csy = 0, cdx = 0, cdy = 0, sc = 0, c = 1, s = 0, tx = 0, ty = 0;
};

// steps 2-5 on the n pairs (S[j], M[j]); dist (may be null): step 7's mean_error
int fit_step(GpsAlignBuf& g, const double2* S, const double2* M, const double* dist, int64_t n, Step* o, hipStream_t st) {
    const int64_t nb = nblocks(n);
    const int gb = (int)nb;
    const double dn = (double)n;
    double t[6];
    int rc;
    if (dist) ga_stats1_kernel<true><<<gb, 256, 0, st>>>(S, M, dist, n, g.part, nb);
    else ga_stats1_kernel<false><<<gb, 256, 0, st>>>(S, M, nullptr, n, g.part, nb);
    if ((rc = tree_totals(g, dist ? 5 : 4, nb, t, st))) return rc;
    o->csx = t[0] / dn, o->csy = t[1] / dn, o->cdx = t[2] / dn, o->cdy = t[3] / dn;
    o->mean_error = dist ? t[4] / dn : 0.0;
    ga_stats2_kernel<<<gb, 256, 0, st>>>(S, M, n, o->csx, o->csy, o->cdx, o->cdy, g.part, nb);
    if ((rc = tree_totals(g, 6, nb, t, st))) return rc;
    const double h00 = t[0], h01 = t[1], h10 = t[2], h11 = t[3], saa = t[4], sbb = t[5];
    const double p = h00 + h11, q = h01 - h10;
    const double r = std::sqrt(p * p + q * q);
    o->c = 1.0, o->s = 0.0;
    if (r != 0.0) o->c = p / r, o->s = q / r;
    o->sc = std::sqrt(sbb) / std::sqrt(saa);
    if (saa == 0.0 || !std::isfinite(o->sc)) {
        last_error() = "the source points have zero variance or the scale is not finite";
        return kGaState;
    }
    o->tx = o->cdx - o->sc * (o->c * o->csx - o->s * o->csy);
    o->ty = o->cdy - o->sc * (o->s * o->csx + o->c * o->csy);
    return kOk;
}

}  // namespace

int64_t ga_chunk_width(int64_t n, int64_t m) {
    const int64_t want = std::min(kGaMaxChunks, std::max<int64_t>(1, (kGaWantGroups + nblocks(n) - 1) / nblocks(n)));
    const int64_t w = ((m + want - 1) / want + kGaTile - 1) / kGaTile * kGaTile;
    return std::max(w, kGaChunkMin);
}

void gps_align_free(GpsAlignBuf& g) {
    dev_free(&g.arena, &g.geo_xy);
    host_free(&g.h_part);
    g = GpsAlignBuf{};
}

int gps_align(GpsAlignBuf& g, const double* gps, int64_t m, const double* slam, int64_t n, int max_iterations,
              double tolerance, double* aligned, int32_t* nn_opt, double* out, hipStream_t st) {
    const int64_t chunk = ga_chunk_width(n, m), nchunks = (m + chunk - 1) / chunk;
    int rc = ga_reserve(g, n, m, nchunks);
    if (rc) return rc;
    for (int k = 0; k < kGaLen; ++k) out[k] = 0.0;
    LIO_HIP(hipMemcpyAsync(g.a_in, slam, (size_t)n * sizeof(double2), hipMemcpyHostToDevice, st));
    LIO_HIP(hipMemcpyAsync(g.b_in, gps, (size_t)m * sizeof(double2), hipMemcpyHostToDevice, st));
    const int64_t nbA = nblocks(n), nbB = nblocks(m);
    double2* S = g.a_in;  // centred and scaled in place
    double t[2], cA[2], cB[2], sA, sB;
    // start: centroids, centred sets, norms
    ga_sum_xy_kernel<<<(int)nbA, 256, 0, st>>>(g.a_in, n, g.part, nbA);
    if ((rc = tree_totals(g, 2, nbA, t, st))) return rc;
    cA[0] = t[0] / (double)n, cA[1] = t[1] / (double)n;
    ga_sum_xy_kernel<<<(int)nbB, 256, 0, st>>>(g.b_in, m, g.part, nbB);
    if ((rc = tree_totals(g, 2, nbB, t, st))) return rc;
    cB[0] = t[0] / (double)m, cB[1] = t[1] / (double)m;
    ga_centre_kernel<<<(int)nbA, 256, 0, st>>>(g.a_in, n, cA[0], cA[1], S, g.part, nbA);
    if ((rc = tree_totals(g, 1, nbA, t, st))) return rc;
    sA = std::sqrt(t[0]);
    ga_centre_kernel<<<(int)nbB, 256, 0, st>>>(g.b_in, m, cB[0], cB[1], g.d, g.part, nbB);
    if ((rc = tree_totals(g, 1, nbB, t, st))) return rc;
    sB = std::sqrt(t[0]);
    if (sA == 0.0 || sB == 0.0) {
        last_error() = "a point set has zero variance";
        return kArg;
    }
    const double s0 = sA > 1e-8 ? sB / sA : 1.0;
    ga_scale_kernel<<<(int)nbA, 256, 0, st>>>(S, n, s0);
    out[kGaS0] = s0;
    out[kGaCA] = cA[0], out[kGaCA + 1] = cA[1];
    out[kGaCB] = cB[0], out[kGaCB + 1] = cB[1];
    // the total similarity, slam_xy -> GPS frame
    double tS = s0, tC = 1.0, tSn = 0.0, tT[2] = {-(s0 * cA[0]), -(s0 * cA[1])};
    double prev = std::numeric_limits<double>::infinity();
    Step sp;
    int iters = 0, converged = 0;
    const dim3 nn_grid((unsigned)nbA, (unsigned)nchunks);
    for (int i = 0; i < max_iterations; ++i) {
        ga_nn_kernel<<<nn_grid, 256, 0, st>>>(S, n, g.d, m, chunk, g.part_d2, g.part_k);
        ga_merge_kernel<<<(int)nbA, 256, 0, st>>>(g.part_d2, g.part_k, n, (int)nchunks, g.d, g.nn, g.mt, g.dist);
        if ((rc = fit_step(g, S, g.mt, g.dist, n, &sp, st))) return rc;
        ga_apply_kernel<<<(int)nbA, 256, 0, st>>>(S, n, sp.sc, sp.c, sp.s, sp.tx, sp.ty);
        tS = sp.sc * tS;
        const double nC = sp.c * tC - sp.s * tSn, nS = sp.s * tC + sp.c * tSn;
        tC = nC, tSn = nS;
        const double nTx = sp.sc * (sp.c * tT[0] - sp.s * tT[1]) + sp.tx, nTy = sp.sc * (sp.s * tT[0] + sp.c * tT[1]) + sp.ty;
        tT[0] = nTx, tT[1] = nTy;
        iters = i + 1;
        if (std::fabs(prev - sp.mean_error) < tolerance) {
            converged = 1;
            break;
        }
        prev = sp.mean_error;
    }
    LIO_HIP(hipGetLastError());
    LIO_HIP(hipMemcpyAsync(aligned, S, (size_t)n * sizeof(double2), hipMemcpyDeviceToHost, st));
    if (nn_opt) LIO_HIP(hipMemcpyAsync(nn_opt, g.nn, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    out[kGaIters] = (double)iters;
    out[kGaConverged] = (double)converged;
    out[kGaMeanError] = sp.mean_error;
    out[kGaSc] = sp.sc, out[kGaC] = sp.c, out[kGaS] = sp.s;
    out[kGaT] = sp.tx, out[kGaT + 1] = sp.ty;
    out[kGaCD] = sp.cdx, out[kGaCD + 1] = sp.cdy;
    // the reference's own closing formula (align_slam_gps_icp.py:152-154): the LAST increment only
    const double ux = cB[0] - sp.tx, uy = cB[1] - sp.ty;
    const double rx = sp.c * ux + sp.s * uy, ry = sp.c * uy - sp.s * ux;  // R^T u
    const double vx = sp.cdx - s0 * rx, vy = sp.cdy - s0 * ry;
    out[kGaRefScale] = s0 * sp.sc;
    out[kGaRefC] = sp.c, out[kGaRefS] = sp.s;
    out[kGaRefT] = cB[0] + sp.sc * (sp.c * vx - sp.s * vy);
    out[kGaRefT + 1] = cB[1] + sp.sc * (sp.s * vx + sp.c * vy);
    out[kGaTotScale] = tS, out[kGaTotC] = tC, out[kGaTotS] = tSn;
    out[kGaTotT] = tT[0] + cB[0], out[kGaTotT + 1] = tT[1] + cB[1];
    return kOk;
}

int similarity2d_fit(GpsAlignBuf& g, const double* src, const double* dst, int64_t n, double* out, hipStream_t st) {
    int rc = ga_reserve(g, n, n, 0);
    if (rc) return rc;
    for (int k = 0; k < kSimLen; ++k) out[k] = 0.0;
    LIO_HIP(hipMemcpyAsync(g.a_in, src, (size_t)n * sizeof(double2), hipMemcpyHostToDevice, st));
    LIO_HIP(hipMemcpyAsync(g.b_in, dst, (size_t)n * sizeof(double2), hipMemcpyHostToDevice, st));
    Step sp;
    if ((rc = fit_step(g, g.a_in, g.b_in, nullptr, n, &sp, st))) return rc;
    out[kSimScale] = sp.sc, out[kSimC] = sp.c, out[kSimS] = sp.s;
    out[kSimT] = sp.tx, out[kSimT + 1] = sp.ty;
    return kOk;
}

int georeference_xy(const float* d_in, int64_t n, int stride, const double p[9], float* d_out, double* d_xy,
                    hipStream_t st) {
    if (n <= 0) return kOk;
    ga_georef_kernel<<<nblk(n), 256, 0, st>>>(d_in, n, stride, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], d_out,
                                              reinterpret_cast<double2*>(d_xy));
    LIO_HIP(hipGetLastError());
    return kOk;
}

}  // namespace lio
