// lio_kmeans.hip — k-means on gfx950: the cv::kmeans call of the reference's projection tool
// (post_process/lidar_projection/src/lidar_projection.cpp:82-92: K 5, TermCriteria(EPS + MAX_ITER, 100, 0.1), 3
// attempts, KMEANS_PP_CENTERS) [U], restated as the contract of lio_kmeans (include/lio_gpu.h):
//
//   scales     coordinates as integers qx = rint(x 2^(31 - ec)), squared distances as q(d) = floor(d 2^(31 - ed)),
//              both from the bounding box of the finite points; every sum is an integer sum
//   seeding    k-means++ with 3 trials per centre: a prefix search over the weights w = q(min d2 to the centres
//              so far), the draws from the counter-based sampler of lio_plane_sample_triples
//   Lloyd      assign by float d2 (strict <, ascending k), centres from the integer sums, empty clusters repaired
//              from the largest one, the labels that produced the final centres kept
//   result     the attempt with the smallest compactness cq, the lowest attempt among equals
//
// Launch sequence (every step its own launch on one stream; no kernel waits for another workgroup):
//   count (finite flags, their number, the box)                                            -> wait
//   per attempt: centre 0 (pick), weights (minsum); per further centre 3 x (pick, minsum), choose  -> wait
//   per iteration: assign-and-accumulate (the hot kernel)                                 -> wait (K x 4 integers)
//                  the centres, the shift and the stop test on the host; a repair: argmax -> wait, relabel
//   per attempt: compactness                                                              -> wait
//   boxes of the best attempt                                                             -> wait
//
// ATOMICS.  Adds of many workgroups to ONE word queue up at the memory side: with one accumulator the kernels
// here ran at the rate of that queue, not of the memory (profiles/kmeans_kernel_stats.md).  So a sum that every
// workgroup contributes to is either left as per-chunk partials that the next one-workgroup kernel adds up (the
// seeding weights: the prefix search reads them anyway), or spread over kKmSpread copies on cache lines of their
// own that the host adds up (the cluster sums, the compactness); a min / max is sent only when it would change
// the word as the workgroup sees it (a stale view costs an atomic too many, never one too few).
//
// DETERMINISM.  Every cross-thread accumulation is an integer add, min or max, so no result depends on the
// schedule; the float arithmetic of a point is its thread's alone.  Repeated calls are bit-identical.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lio_scratch.hpp"
#include "lio_kmeans.hpp"

namespace lio {

namespace {

using ull = unsigned long long;

constexpr int kKmChunk = 1024;       // points per workgroup and step: 256 threads x 4
constexpr int kKmPickThreads = 1024;
constexpr int kKmAssignBlocks = 2048;  // most workgroups of the assign kernel (it strides over the chunks)
constexpr int kAccWords = 4 * kKmMaxK;  // one copy of the cluster sums: 2 KiB
// the pinned block: acc (every copy), the state, an attempt's seeds, the boxes
constexpr size_t kPinAcc = 0, kPinState = (size_t)kKmSpread * kAccWords * 8, kPinSeeds = kPinState + 2048,
                 kPinBox = kPinSeeds + 256, kPinBytes = kPinBox + 6 * kKmMaxK * 4;
static_assert(sizeof(KmState) <= kPinSeeds - kPinState, "pinned layout");

struct KmCentres {  // a kernel argument: the K centres are uniform
    float c[3 * kKmMaxK];
};
struct KmSlots {
    uint32_t* w[4];
    ull* part[4];
};

// unsigned order = float order (-0 below +0); no NaN comes here
__host__ __device__ inline uint32_t km_ord_of(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__host__ __device__ inline uint32_t km_ord_to(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }

// The four points of a thread in its workgroup's chunk: i[r] = chunk * 1024 + r * 256 + thread (-1 past the end),
// loaded together so that the loads are in flight at once.  fin[r]: inside the cloud and finite.
struct KmFour {
    int64_t i[4];
    float x[4], y[4], z[4];
    bool fin[4];
};
__device__ __forceinline__ KmFour km_load4(const float* __restrict__ pts, int64_t n, int stride, int64_t chunk) {
    KmFour p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = chunk * kKmChunk + r * 256 + threadIdx.x;
        p.i[r] = i < n ? i : -1;
        p.x[r] = p.y[r] = p.z[r] = NAN;
        if (i < n) {
            const float* q = pts + (size_t)i * stride;
            p.x[r] = q[0], p.y[r] = q[1], p.z[r] = q[2];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)  // false for NaN
        p.fin[r] = fabsf(p.x[r]) < INFINITY && fabsf(p.y[r]) < INFINITY && fabsf(p.z[r]) < INFINITY;
    return p;
}
__device__ __forceinline__ float km_d2(float x, float y, float z, float cx, float cy, float cz) {
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    return (dx * dx + dy * dy) + dz * dz;
}
// floor(d 2^(31 - ed)): scaling by a power of two is exact in double, the conversion truncates (d >= 0)
__device__ __forceinline__ ull km_q(float d, double sd) { return (ull)((double)d * sd); }

// sum of v over the workgroup's threads (a power of two of them), in every thread
__device__ __forceinline__ ull km_block_sum(ull v, ull* sh) {
    __syncthreads();  // the readers of sh before are done
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// ---- the counting pass: w[0] = 1 for a finite point (so the pick kernel finds the t-th finite point), their
// number per chunk and in all, the lowest finite index, the box ----
__global__ void __launch_bounds__(256) km_count_kernel(const float* __restrict__ pts, int64_t n, int stride,
                                                       uint32_t* __restrict__ w, ull* __restrict__ part, KmState* s) {
    __shared__ ull sh[256];
    __shared__ uint32_t sbox[6], sfirst;
    if (threadIdx.x < 6) sbox[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    if (threadIdx.x == 6) sfirst = 0xffffffffu;
    __syncthreads();
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, first = 0xffffffffu;
    ull cnt = 0;
    const KmFour p = km_load4(pts, n, stride, blockIdx.x);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (p.i[r] < 0) continue;
        w[p.i[r]] = p.fin[r] ? 1u : 0u;
        if (!p.fin[r]) continue;
        ++cnt;
        first = min(first, (uint32_t)p.i[r]);
        const float v[3] = {p.x[r], p.y[r], p.z[r]};
        for (int d = 0; d < 3; ++d) {
            const uint32_t k = km_ord_of(__float_as_uint(v[d]));
            lo[d] = min(lo[d], k), hi[d] = max(hi[d], k);
        }
    }
    if (cnt) {
        for (int d = 0; d < 3; ++d) atomicMin(&sbox[d], lo[d]), atomicMax(&sbox[3 + d], hi[d]);
        atomicMin(&sfirst, first);
    }
    const ull total = km_block_sum(cnt, sh);  // its barriers order the LDS atomics above, too
    if (threadIdx.x == 0) part[blockIdx.x] = total;
    if (!total) return;
    const int t = threadIdx.x;
    if (t < 3) {
        if (sbox[t] < s->bbox[t]) atomicMin(&s->bbox[t], sbox[t]);
    } else if (t < 6) {
        if (sbox[t] > s->bbox[t]) atomicMax(&s->bbox[t], sbox[t]);
    } else if (t == 6) {
        if (sfirst < s->first_finite) atomicMin(&s->first_finite, sfirst);
    }
}

// nf = the sum of the per-chunk counts, one workgroup
__global__ void __launch_bounds__(kKmPickThreads) km_total_kernel(const ull* __restrict__ part, int64_t nb, KmState* s) {
    __shared__ ull sh[kKmPickThreads];
    ull mine = 0;
    for (int64_t b = threadIdx.x; b < nb; b += kKmPickThreads) mine += part[b];
    const ull total = km_block_sum(mine, sh);
    if (threadIdx.x == 0) s->nf = total;
}

// inclusive scan of v over the kKmPickThreads threads
__device__ __forceinline__ ull km_pick_scan(ull v, ull* sh) {
    __syncthreads();  // the readers of sh before are done
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < kKmPickThreads; o <<= 1) {
        const ull a = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += a;
        __syncthreads();
    }
    return sh[threadIdx.x];
}

// ---- the prefix search, one workgroup: *out = the lowest index whose inclusive prefix sum of w exceeds t; sum0
// is the sum of the per-chunk sums.  trial < 0: w is slot 0 (the finite flags, sum0 = nf) and t = r mod sum0
// (centre 0: the t-th finite point).  trial j >= 0: w is the current slot, t = (r * sum0) >> 53 with the 128-bit
// product (r < 2^53), the lowest finite index when sum0 = 0; out = &cand[j].  Two levels: the chunk from the
// per-chunk sums, then the point inside the chunk.
__global__ void __launch_bounds__(kKmPickThreads) km_pick_kernel(KmSlots sl, int64_t n, int64_t nb, int trial, ull r,
                                                                 KmState* s, int32_t* out_opt) {
    __shared__ ull sh[kKmPickThreads];
    __shared__ ull s_rest;
    __shared__ long long s_blk;
    const int in = trial < 0 ? 0 : s->cur;
    int32_t* out = trial < 0 ? out_opt : &s->cand[trial];
    if (threadIdx.x == 0) {
        s_blk = -1, s_rest = 0;
        *out = (int32_t)s->first_finite;  // sum0 = 0; replaced below otherwise
    }
    const ull* __restrict__ part = sl.part[in];
    const uint32_t* __restrict__ w = sl.w[in];
    const int64_t per = (nb + kKmPickThreads - 1) / kKmPickThreads;
    const int64_t b0 = threadIdx.x * per < nb ? threadIdx.x * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    ull mine = 0;
    for (int64_t b = b0; b < b1; ++b) mine += part[b];
    const ull incl = km_pick_scan(mine, sh);
    const ull sum0 = sh[kKmPickThreads - 1];
    if (sum0 == 0) return;
    const ull t = trial < 0 ? r % sum0 : ((__umul64hi(r, sum0) << 11) | ((r * sum0) >> 53));
    if (t >= sum0) return;  // cannot be (r < 2^53): no search outside the table
    if (incl - mine <= t && t < incl) {
        ull at = incl - mine;
        for (int64_t b = b0; b < b1; ++b) {
            const ull v = part[b];
            if (at + v > t) {
                s_blk = b, s_rest = t - at;
                break;
            }
            at += v;
        }
    }
    __syncthreads();
    const long long blk = s_blk;
    if (blk < 0) return;
    const ull rest = s_rest;
    const int64_t i = blk * (int64_t)kKmChunk + threadIdx.x;
    const ull v = i < n ? (ull)w[i] : 0;
    const ull inc2 = km_pick_scan(v, sh);
    if (inc2 - v <= rest && rest < inc2) *out = (int32_t)i;
}

// ---- the min-and-sum pass: w'[i] = min(q(d2(p_i, p_ci)), w[i]) (first: q alone), 0 for a non-finite point, and
// its sum per chunk.  first: ci = *cand_opt, into slot 0; else ci = cand[trial], from the current slot into slot
// (cur + 1 + trial) & 3.
__global__ void __launch_bounds__(256) km_minsum_kernel(const float* __restrict__ pts, int64_t n, int stride, KmSlots sl,
                                                        const KmState* __restrict__ s, const int32_t* cand_opt, int trial,
                                                        double sd) {
    __shared__ ull sh[256];
    const bool first = trial < 0;
    const int cur = first ? 0 : s->cur, dst = first ? 0 : (cur + 1 + trial) & 3;
    const int64_t ci = first ? *cand_opt : s->cand[trial];
    const float* c = pts + (size_t)ci * stride;
    const float cx = c[0], cy = c[1], cz = c[2];
    const uint32_t* __restrict__ win = sl.w[cur];
    uint32_t* __restrict__ wout = sl.w[dst];
    const KmFour p = km_load4(pts, n, stride, blockIdx.x);
    uint32_t old[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) old[r] = !first && p.fin[r] ? win[p.i[r]] : 0xffffffffu;
    ull sum = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (p.i[r] < 0) continue;
        ull q = 0;
        if (p.fin[r]) q = min(km_q(km_d2(p.x[r], p.y[r], p.z[r], cx, cy, cz), sd), (ull)old[r]);
        wout[p.i[r]] = (uint32_t)q;
        sum += q;
    }
    const ull total = km_block_sum(sum, sh);
    if (threadIdx.x == 0) sl.part[dst][blockIdx.x] = total;
}

// attempt a begins: slot 0 is the current one
__global__ void km_begin_kernel(KmState* s) { s->cur = 0; }

// centre k of attempt a, one workgroup: the trial with the smallest sum of its weights, the lowest among equals;
// its weights become current
__global__ void __launch_bounds__(kKmPickThreads) km_choose_kernel(KmSlots sl, int64_t nb, KmState* s, int32_t* seed_out) {
    __shared__ ull sh[kKmPickThreads];
    const int cur = s->cur;
    ull tot[3];
    for (int j = 0; j < 3; ++j) {
        const ull* __restrict__ part = sl.part[(cur + 1 + j) & 3];
        ull mine = 0;
        for (int64_t b = threadIdx.x; b < nb; b += kKmPickThreads) mine += part[b];
        tot[j] = km_block_sum(mine, sh);
    }
    if (threadIdx.x) return;
    int bj = 0;
    for (int j = 1; j < 3; ++j)
        if (tot[j] < tot[bj]) bj = j;
    *seed_out = s->cand[bj];
    s->cur = (cur + 1 + bj) & 3;
}

// ---- the hot kernel: assign and accumulate.  Thread = four points of a chunk (the workgroups stride over the
// chunks): the centres sit in LDS (every lane reads the same entry: a broadcast), the argmin is the contract's
// strict < over ascending k, and (1, qx, qy, qz) goes into the workgroup's per-cluster 64-bit integer
// accumulators in LDS.  A wave whose 64 points all chose one cluster (the usual case in scan order) sums across
// its lanes first and adds once; otherwise every lane adds for itself.  At the end one global atomic per
// workgroup, cluster and component, into copy blockIdx % kKmSpread of the sums (accw words apart: 4 K rounded up
// to whole cache lines).
__global__ void __launch_bounds__(256) km_assign_kernel(const float* __restrict__ pts, int64_t n, int stride, int K,
                                                        KmCentres cs, double sx, int32_t* __restrict__ labels,
                                                        ull* __restrict__ acc, int accw) {
    __shared__ float sc[3 * kKmMaxK];
    __shared__ ull sacc[kAccWords];
    for (int t = threadIdx.x; t < 3 * K; t += 256) sc[t] = cs.c[t];
    for (int t = threadIdx.x; t < 4 * K; t += 256) sacc[t] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t chunks = (n + kKmChunk - 1) / kKmChunk;
    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const KmFour p = km_load4(pts, n, stride, chunk);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool valid = p.fin[r];
            int lab = -1;
            long long qx = 0, qy = 0, qz = 0;
            if (valid) {
                const float x = p.x[r], y = p.y[r], z = p.z[r];
                lab = 0;
                float best = km_d2(x, y, z, sc[0], sc[1], sc[2]);
                for (int k = 1; k < K; ++k) {
                    const float d = km_d2(x, y, z, sc[3 * k], sc[3 * k + 1], sc[3 * k + 2]);
                    if (d < best) best = d, lab = k;
                }
                qx = (long long)rint((double)x * sx), qy = (long long)rint((double)y * sx), qz = (long long)rint((double)z * sx);
            }
            if (p.i[r] >= 0) labels[p.i[r]] = lab;
            const ull vm = __ballot(valid);
            if (vm == 0) continue;  // wave-uniform
            const int l0 = __shfl(lab, __ffsll((long long)vm) - 1);
            if (__ballot(valid && lab == l0) == vm) {  // wave-uniform: one cluster for the whole wave
                for (int o = 32; o > 0; o >>= 1) qx += __shfl_xor(qx, o), qy += __shfl_xor(qy, o), qz += __shfl_xor(qz, o);
                if (lane == 0) {
                    atomicAdd(&sacc[4 * l0], (ull)__popcll(vm));
                    atomicAdd(&sacc[4 * l0 + 1], (ull)qx), atomicAdd(&sacc[4 * l0 + 2], (ull)qy), atomicAdd(&sacc[4 * l0 + 3], (ull)qz);
                }
            } else if (valid) {
                atomicAdd(&sacc[4 * lab], 1ull);
                atomicAdd(&sacc[4 * lab + 1], (ull)qx), atomicAdd(&sacc[4 * lab + 2], (ull)qy), atomicAdd(&sacc[4 * lab + 3], (ull)qz);
            }
        }
    }
    __syncthreads();
    ull* __restrict__ mine = acc + (size_t)(blockIdx.x % kKmSpread) * accw;
    for (int t = threadIdx.x; t < 4 * K; t += 256)
        if (sacc[t]) atomicAdd(mine + t, sacc[t]);
}

// the attempt's compactness: the sum of q(d2(p_i, c_label_i)) over the labelled points, spread as the header says
__global__ void __launch_bounds__(256) km_cq_kernel(const float* __restrict__ pts, int64_t n, int stride, int K, KmCentres cs,
                                                    double sd, const int32_t* __restrict__ labels, KmState* s) {
    __shared__ float sc[3 * kKmMaxK];
    __shared__ ull sh[256];
    for (int t = threadIdx.x; t < 3 * K; t += 256) sc[t] = cs.c[t];
    __syncthreads();
    const KmFour p = km_load4(pts, n, stride, blockIdx.x);
    int lab[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lab[r] = p.i[r] >= 0 ? labels[p.i[r]] : -1;
    ull sum = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (lab[r] >= 0 && lab[r] < K)
            sum += km_q(km_d2(p.x[r], p.y[r], p.z[r], sc[3 * lab[r]], sc[3 * lab[r] + 1], sc[3 * lab[r] + 2]), sd);
    const ull total = km_block_sum(sum, sh);
    if (threadIdx.x == 0 && total) atomicAdd(&s->cq[(blockIdx.x % kKmSpread) * 8], total);
}

// the repair's argmax: over the members of cluster mk, the largest (float bits of d2 to its mean, ~index) — d2 >= 0,
// so its bits order as its value, and the complemented index makes the lowest index win among equals
__global__ void __launch_bounds__(256) km_argmax_kernel(const float* __restrict__ pts, int64_t n, int stride,
                                                        const int32_t* __restrict__ labels, int mk, float mx, float my,
                                                        float mz, KmState* s) {
    __shared__ ull sbest;
    if (threadIdx.x == 0) sbest = 0;
    __syncthreads();
    const KmFour p = km_load4(pts, n, stride, blockIdx.x);
    ull best = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (p.i[r] < 0 || labels[p.i[r]] != mk) continue;
        const ull key = ((ull)__float_as_uint(km_d2(p.x[r], p.y[r], p.z[r], mx, my, mz)) << 32) | (ull)(~(uint32_t)p.i[r]);
        best = max(best, key);
    }
    if (best) atomicMax(&sbest, best);
    __syncthreads();
    if (threadIdx.x == 0 && sbest > s->amax) atomicMax(&s->amax, sbest);
}

__global__ void km_relabel_kernel(int32_t* labels, int64_t i, int k) { labels[i] = k; }

__global__ void km_box_init_kernel(uint32_t* __restrict__ box, int K) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 6 * K) box[t] = t % 6 < 3 ? 0xffffffffu : 0u;
}

// per cluster the min / max of x, y, z over its members, as order-preserving keys: integer atomics in LDS, then
// at most one global atomic per workgroup and word
__global__ void __launch_bounds__(256) km_box_kernel(const float* __restrict__ pts, int64_t n, int stride, int K,
                                                     const int32_t* __restrict__ labels, uint32_t* __restrict__ box) {
    __shared__ uint32_t sb[6 * kKmMaxK];
    for (int t = threadIdx.x; t < 6 * K; t += 256) sb[t] = t % 6 < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    const KmFour p = km_load4(pts, n, stride, blockIdx.x);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (p.i[r] < 0) continue;
        const int lab = labels[p.i[r]];
        if (lab < 0 || lab >= K) continue;
        const float v[3] = {p.x[r], p.y[r], p.z[r]};
        for (int d = 0; d < 3; ++d) {
            const uint32_t k = km_ord_of(__float_as_uint(v[d]));
            atomicMin(&sb[6 * lab + d], k), atomicMax(&sb[6 * lab + 3 + d], k);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 6 * K; t += 256) {
        if (t % 6 < 3) {
            if (sb[t] < box[t]) atomicMin(box + t, sb[t]);
        } else if (sb[t] > box[t]) {
            atomicMax(box + t, sb[t]);
        }
    }
}

int kmeans_reserve(KMeansBuf& b, int64_t n) {
    if (!b.h_pin) {
        count_alloc();
        if (hipHostMalloc(&b.h_pin, kPinBytes) != hipSuccess) {
            b.h_pin = nullptr;
            return kNoMem;
        }
    }
    if (n <= b.cap_n && b.arena) return kOk;
    const int64_t cn = grown<int64_t>(n, b.cap_n, 4096);
    dev_free(&b.arena);
    b.arena_bytes = 0, b.cap_n = 0;
    const size_t N = (size_t)cn, NB = (size_t)((cn + kKmChunk - 1) / kKmChunk);
    auto fields = [&](Carver& at) {  // the arena's fields, once each, in arena order
        at(b.labels[0], N), at(b.labels[1], N);
        for (int k = 0; k < 4; ++k) at(b.w[k], N), at(b.part[k], NB);
        at(b.acc, (size_t)kKmSpread * kAccWords), at(b.box, 6 * kKmMaxK), at(b.seeds, kKmMaxAttempts * kKmMaxK);
        at(b.state, 1);
    };
    const int rc = reserve_arena(&b.arena, b.arena_bytes, fields, 0);
    if (rc) return rc;
    b.cap_n = cn;
    return kOk;
}

inline uint64_t mix64(uint64_t z) {  // splitmix64's output function
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline float as_float(uint32_t b) {
    float f;
    std::memcpy(&f, &b, sizeof(f));
    return f;
}

}  // namespace

void kmeans_free(KMeansBuf& b) {
    dev_free(&b.arena);
    host_free(&b.h_pin);
    b = KMeansBuf{};
}

int kmeans(KMeansBuf& b, const float* d_pts, const float* h_pts, int64_t n, int stride, const KMeansArgs& a,
           bool want_boxes, KMeansResult* out, hipStream_t st) {
    const int K = a.K;
    if (n < 1 || n >= (int64_t)1 << 31 || stride < 3 || stride > 8 || K < 1 || K > kKmMaxK || a.attempts < 1 ||
        a.attempts > kKmMaxAttempts || a.max_iter < 1 || a.max_iter > kKmMaxIter || !(a.eps >= 0.f) || !std::isfinite(a.eps))
        return kArg;
    int rc = kmeans_reserve(b, n);
    if (rc) return rc;
    uint8_t* pin = static_cast<uint8_t*>(b.h_pin);
    ull* h_acc = reinterpret_cast<ull*>(pin + kPinAcc);
    KmState* h_state = reinterpret_cast<KmState*>(pin + kPinState);
    int32_t* h_seeds = reinterpret_cast<int32_t*>(pin + kPinSeeds);
    uint32_t* h_box = reinterpret_cast<uint32_t*>(pin + kPinBox);
    const int64_t nb = (n + kKmChunk - 1) / kKmChunk;
    KmSlots sl;
    for (int k = 0; k < 4; ++k) sl.w[k] = b.w[k], sl.part[k] = b.part[k];

    // ---- the counting pass and the two scales ----
    *h_state = KmState{};
    for (int d = 0; d < 3; ++d) h_state->bbox[d] = 0xffffffffu;
    h_state->first_finite = 0xffffffffu;
    LIO_HIP(hipMemcpyAsync(b.state, h_state, sizeof(KmState), hipMemcpyHostToDevice, st));
    km_count_kernel<<<(unsigned)nb, 256, 0, st>>>(d_pts, n, stride, b.w[0], b.part[0], b.state);
    km_total_kernel<<<1, kKmPickThreads, 0, st>>>(b.part[0], nb, b.state);
    LIO_HIP(hipMemcpyAsync(h_state, b.state, sizeof(KmState), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    const int64_t nf = (int64_t)h_state->nf;
    if (nf < K) {
        last_error() = "fewer finite points than clusters";
        return kArg;
    }
    float lo[3], hi[3], A = 0.f;
    for (int d = 0; d < 3; ++d) {
        lo[d] = as_float(km_ord_to(h_state->bbox[d])), hi[d] = as_float(km_ord_to(h_state->bbox[3 + d]));
        A = std::max(A, std::max(std::fabs(lo[d]), std::fabs(hi[d])));
    }
    const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
    const float D2 = (ex * ex + ey * ey) + ez * ez;
    if (!std::isfinite(D2)) {
        last_error() = "the squared diagonal of the cloud's box is not a finite float";
        return kArg;
    }
    int ec = 0, ed = 0;
    if (A != 0.f) (void)std::frexp(A, &ec);
    if (D2 != 0.f) (void)std::frexp(D2, &ed);
    const double sx = std::ldexp(1.0, 31 - ec), sd = std::ldexp(1.0, 31 - ed), inv = std::ldexp(1.0, ec - 31);
    auto quant = [&](float v) { return (int64_t)std::rint((double)v * sx); };
    auto draw = [&](uint64_t c) { return mix64(a.seed + (c + 1) * 0x9E3779B97F4A7C15ull); };

    out->nf = nf, out->ec = ec, out->ed = ed, out->repairs = 0, out->best = 0;
    const bool seeding = a.init_centers == nullptr;
    if (seeding)  // centre 0 of every attempt, while slot 0 still holds the finite flags
        for (int t = 0; t < a.attempts; ++t)
            km_pick_kernel<<<1, kKmPickThreads, 0, st>>>(sl, n, nb, -1, (ull)draw((uint64_t)t * K * 3), b.state, b.seeds + t * K);
    const double eps2 = (double)a.eps * a.eps;
    const int last_it = std::max(a.max_iter, 2);
    const unsigned assign_blocks = (unsigned)std::min<int64_t>(kKmAssignBlocks, nb);
    const int accw = (4 * K + 7) & ~7;  // one copy of the cluster sums, in whole 64-byte lines
    const size_t acc_bytes = (size_t)kKmSpread * accw * sizeof(ull);
    int run_buf = 0, best_buf = 1;
    uint64_t best_q = 0;
    for (int t = 0; t < a.attempts; ++t) {
        KmCentres C;
        std::memset(&C, 0, sizeof(C));
        int32_t* seeds_t = out->seeds + t * K;
        if (!seeding) {
            std::memcpy(C.c, a.init_centers + (size_t)t * K * 3, (size_t)K * 3 * sizeof(float));
            for (int k = 0; k < K; ++k) seeds_t[k] = -1;
        } else {
            km_begin_kernel<<<1, 1, 0, st>>>(b.state);
            km_minsum_kernel<<<(unsigned)nb, 256, 0, st>>>(d_pts, n, stride, sl, b.state, b.seeds + t * K, -1, sd);
            for (int k = 1; k < K; ++k) {
                for (int j = 0; j < 3; ++j) {
                    const ull u = draw(((uint64_t)t * K + k) * 3 + j) >> 11;
                    km_pick_kernel<<<1, kKmPickThreads, 0, st>>>(sl, n, nb, j, u, b.state, nullptr);
                    km_minsum_kernel<<<(unsigned)nb, 256, 0, st>>>(d_pts, n, stride, sl, b.state, nullptr, j, sd);
                }
                km_choose_kernel<<<1, kKmPickThreads, 0, st>>>(sl, nb, b.state, b.seeds + t * K + k);
            }
            LIO_HIP(hipMemcpyAsync(h_seeds, b.seeds + t * K, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            LIO_HIP(hipStreamSynchronize(st));
            for (int k = 0; k < K; ++k) {
                const int64_t i = h_seeds[k];
                if (i < 0 || i >= n) {
                    last_error() = "the seeding chose an index outside the cloud";
                    return kHip;
                }
                seeds_t[k] = (int32_t)i;
                for (int d = 0; d < 3; ++d) C.c[3 * k + d] = h_pts[(size_t)i * stride + d];
            }
        }
        int64_t cnt[kKmMaxK], S[kKmMaxK][3];
        int it = 1;
        for (;;) {
            LIO_HIP(hipMemsetAsync(b.acc, 0, acc_bytes, st));
            km_assign_kernel<<<assign_blocks, 256, 0, st>>>(d_pts, n, stride, K, C, sx, b.labels[run_buf], b.acc, accw);
            LIO_HIP(hipMemcpyAsync(h_acc, b.acc, acc_bytes, hipMemcpyDeviceToHost, st));
            LIO_HIP(hipStreamSynchronize(st));
            for (int k = 0; k < K; ++k) {  // the copies added up (mod 2^64: the sums are signed)
                ull v[4] = {0, 0, 0, 0};
                for (int c = 0; c < kKmSpread; ++c)
                    for (int d = 0; d < 4; ++d) v[d] += h_acc[(size_t)c * accw + 4 * k + d];
                cnt[k] = (int64_t)v[0];
                for (int d = 0; d < 3; ++d) S[k][d] = (int64_t)v[1 + d];
            }
            for (int k = 0; k < K; ++k) {  // the repair: rare
                if (cnt[k]) continue;
                int mk = 0;
                for (int j = 1; j < K; ++j)
                    if (cnt[j] > cnt[mk]) mk = j;
                float m[3];
                for (int d = 0; d < 3; ++d) m[d] = (float)(((double)S[mk][d] / (double)cnt[mk]) * inv);
                LIO_HIP(hipMemsetAsync(&b.state->amax, 0, sizeof(ull), st));
                km_argmax_kernel<<<(unsigned)nb, 256, 0, st>>>(d_pts, n, stride, b.labels[run_buf], mk, m[0], m[1], m[2], b.state);
                LIO_HIP(hipMemcpyAsync(&h_state->amax, &b.state->amax, sizeof(ull), hipMemcpyDeviceToHost, st));
                LIO_HIP(hipStreamSynchronize(st));
                const int64_t i = (int64_t)(uint32_t)~(uint32_t)h_state->amax;
                if (h_state->amax == 0 || i >= n) {
                    last_error() = "the repair found no member of the largest cluster";
                    return kHip;
                }
                for (int d = 0; d < 3; ++d) {
                    const int64_t q = quant(h_pts[(size_t)i * stride + d]);
                    S[mk][d] -= q, S[k][d] = q;
                }
                cnt[mk] -= 1, cnt[k] = 1;
                km_relabel_kernel<<<1, 1, 0, st>>>(b.labels[run_buf], i, k);
                out->repairs += 1;
            }
            double shift = 0.0;
            for (int k = 0; k < K; ++k) {
                double sk[3];
                for (int d = 0; d < 3; ++d) {
                    const float c = (float)(((double)S[k][d] / (double)cnt[k]) * inv);
                    sk[d] = (double)(c - C.c[3 * k + d]);
                    C.c[3 * k + d] = c;
                }
                shift = std::max(shift, (sk[0] * sk[0] + sk[1] * sk[1]) + sk[2] * sk[2]);
            }
            ++it;
            if (it == last_it || shift <= eps2) break;
        }
        LIO_HIP(hipMemsetAsync(b.state->cq, 0, sizeof(b.state->cq), st));
        km_cq_kernel<<<(unsigned)nb, 256, 0, st>>>(d_pts, n, stride, K, C, sd, b.labels[run_buf], b.state);
        LIO_HIP(hipMemcpyAsync(h_state->cq, b.state->cq, sizeof(b.state->cq), hipMemcpyDeviceToHost, st));
        LIO_HIP(hipStreamSynchronize(st));
        uint64_t cq = 0;
        for (int c = 0; c < kKmSpread; ++c) cq += h_state->cq[c * 8];
        out->attempt_q[t] = cq, out->attempt_iters[t] = it;
        if (t == 0 || cq < best_q) {
            best_q = cq, out->best = t;
            std::swap(run_buf, best_buf);
            std::memcpy(out->centers, C.c, (size_t)K * 3 * sizeof(float));
            std::memcpy(out->counts, cnt, (size_t)K * sizeof(int64_t));
        }
    }
    out->labels = b.labels[best_buf];
    if (want_boxes) {
        km_box_init_kernel<<<2, 256, 0, st>>>(b.box, K);
        km_box_kernel<<<(unsigned)nb, 256, 0, st>>>(d_pts, n, stride, K, out->labels, b.box);
        LIO_HIP(hipMemcpyAsync(h_box, b.box, (size_t)6 * K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        LIO_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < 6 * K; ++k) out->aabb[k] = as_float(km_ord_to(h_box[k]));
    }
    LIO_HIP(hipGetLastError());
    return kOk;
}

}  // namespace lio
