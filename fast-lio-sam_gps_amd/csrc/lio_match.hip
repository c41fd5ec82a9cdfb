// lio_match.hip — FAST-LIO h_share_model on gfx950.
//
// Per h-evaluation:
//
//   ekfom_data.converge == true (redo the kNN):
//     knn_near_kernel  256 threads = 32 points, 8 lanes per point:
//       body->world (double, stored float) -> exact grid 5-NN over shells 0-1,
//       cell points scanned lane-strided (coalesced), private top-5 lists
//       merged by a shuffle butterfly; unresolved points -> far queue (one
//       64-byte entry each: index, world point, list).  Later kNN evaluations
//       of a scan: bound = the previous neighbours' exact d2 (re-gathered)
//     knn_far_kernel   one block per queued point, the rest of its search box
//     plane_kernel     lane = point: gate (found == 5 && d2[4] <= 5) ->
//       esti_plane (QR, registers) -> pd2, s-gate -> H row (double) ->
//       30-value DPP wave reduction -> block partial
//     writes: nn_idx[5] (20 B), plane abcd (16 B), sel (1 B)
//   ekfom_data.converge == false: h_model_reuse_kernel, lane = point
//     body->world -> cached plane -> pd2, s-gate -> H row -> block partial
//   the last block of plane/reuse to finish (agent-scope counter) sums the
//     block partials in a fixed order (deterministic) into host-mapped memory
//     + a sequence number (zero-copy result, no finalize launch)
//
// The per-point dense H (effct x 12 doubles) of the reference is never
// materialised: the IESKF only consumes H^T H and H^T h.
#include <hip/hip_ext.h>

#include "lio_dev.hpp"
#include "lio_kernels.hpp"

#include <algorithm>

namespace lio {

constexpr int kBlock = 256;  // partial-slot granule (the plane / reuse grids below never exceed n / 256 blocks)
constexpr int kPlaneBlock = 512;  // plane pass: 512 threads, 1 point per lane
constexpr int kReuseBlock = 512;  // reuse pass: 512 threads, 2 points per lane
constexpr int kReusePpl = 2;
constexpr int kNearBlock = 256;   // near pass: 32 queries per block

constexpr int kGroup = 8;   // lanes cooperating on one query's kNN
constexpr int kFarBlock = 128;  // threads per far query (64 / 256 / 512 measured slower)
constexpr int kFarBlocks = 1024;  // blocks striding the far queue (one query per block)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// pd2 / s-gate / H row of one selected point (h_share_model [U])
__device__ __forceinline__ bool residual_row(const MatchArgs& a, const PoseArg& ps, float bx, float by, float bz, float wx, float wy,
                                             float wz, const float4& pl, double J[6], double& h, double& res) {
    const float pd2 = ((pl.x * wx + pl.y * wy) + pl.z * wz) + pl.w;
    const double b0 = bx, b1 = by, b2 = bz;
    const double pn = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
    const float s = (float)(1.0 - a.s_coef * (double)fabsf(pd2) / sqrt(pn));
    if (!((double)s > a.s_gate)) return false;
    h_row(ps, bx, by, bz, pl.x, pl.y, pl.z, J);
    h = -(double)pd2;
    res = (double)fabsf(pd2);
    return true;
}

// ekfom_data.converge == true, pass 1: 512 threads = 64 queries, 8 lanes per
// query run the exact 5-NN over shells 0-1 cooperatively (group_knn_near).
// Queries whose 5th neighbour is not yet provably final (sparse
// neighbourhoods, ~0.4% of a dense scan) are queued, with their list, for
// the wave-per-query far pass instead of holding their wave: a kernel runs as
// long as its slowest wave.  Written for 8 waves/SIMD (<= 64 VGPRs).
// U / UO: loads in flight in the seeded table scan / own-cell scan (2 keeps the kernel at <= 64 VGPRs
// without scratch).
template <bool DBG, bool SEEDED, int U, int NB, int UO>
__global__ void __launch_bounds__(NB) __attribute__((amdgpu_waves_per_eu(8, 8))) knn_near_kernel(MatchArgs a) {
    const PoseArg& ps = a.pose;
    constexpr int G = kGroup;
    constexpr int QPB = NB / G;  // 64 queries per block
    __shared__ uint32_t s_tab[QPB][72];      // per-group shell-1 slot table
    __shared__ float s_q[3][QPB];            // per query: world point
    __shared__ int s_c[3][QPB];              //            its cell
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int sub = threadIdx.x % G;
    const int q = threadIdx.x / G;
    const int i = blk * QPB + q;
    // the per-query transforms once per query, not once per lane of its group: wave 0, lane = query
    const int iq = blk * QPB + (int)threadIdx.x;
    const bool lead = threadIdx.x < QPB && iq < a.n;
    float bx, by, bz;  // set and read under `lead` only
    if (lead) bx = a.body[3 * iq], by = a.body[3 * iq + 1], bz = a.body[3 * iq + 2];
    // seeded pass: lane sub < 5 fetches the query's previous neighbour `sub` (its own nn_idx row, rewritten only at
    // the end).  Neither load needs the world point: the ids travel with the body loads, the gathers beside wave
    // 0's transforms.
    int pid = -1;
    float4 pp = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (SEEDED) {
        if (sub < 5 && i < a.n) pid = a.nn_idx[5 * (size_t)i + sub];
        if (pid >= 0) pp = a.map_by_id[pid];
    }
    if (lead) {
        // the body point is first used here: otherwise its conversion to double is hoisted to its load, which then
        // is waited for before the seeded pass's ids are even requested
        asm volatile("" : "+v"(bx), "+v"(by), "+v"(bz));
        float wx, wy, wz;
        body_to_world(ps, bx, by, bz, wx, wy, wz);
        s_q[0][threadIdx.x] = wx;
        s_q[1][threadIdx.x] = wy;
        s_q[2][threadIdx.x] = wz;
        s_c[0][threadIdx.x] = cell_coord(wx, a.grid.ox, a.grid.inv_cell);
        s_c[1][threadIdx.x] = cell_coord(wy, a.grid.oy, a.grid.inv_cell);
        s_c[2][threadIdx.x] = cell_coord(wz, a.grid.oz, a.grid.inv_cell);
    }
    __syncthreads();
    if (i >= a.n) return;
    const float wx = s_q[0][q], wy = s_q[1][q], wz = s_q[2][q];
    TopK<5> tk;
    tk.init(a.range_sq);
    SearchStats st{0, 0, 0};
    bool done, whole = false;
    if constexpr (SEEDED) {  // this scan's previous kNN against the same map: its neighbours' exact d2 bound this one
        const int cx = s_c[0][q], cy = s_c[1][q], cz = s_c[2][q];
        const bool inside = (unsigned)cx < (unsigned)a.grid.nx && (unsigned)cy < (unsigned)a.grid.ny &&
                            (unsigned)cz < (unsigned)a.grid.nz;
        // lanes 0-4: the neighbour's d2 as the scan will compute it (+inf: no such neighbour, the list was not
        // full); lanes 5-7 do not count
        float d = sub < 5 ? INFINITY : 0.f;
        if (pid >= 0) d = sqdist3(wx, wy, wz, pp.x, pp.y, pp.z);
        const float bound = seeded_bound(inside, group_max<G>(d), a.range_sq, a.seed_scale);
        const int r = group_knn_seeded<5, G, U>(a.grid, bound, cx, cy, cz, wx, wy, wz, a.range_sq, sub,
                                                tk, s_tab[threadIdx.x / G]);
        done = r > 0;
        whole = r < 0;
    } else {
        done = group_knn_near<5, G, false, U, UO>(a.grid, wx, wy, wz, s_c[0][q], s_c[1][q], s_c[2][q], 1, sub, tk,
                                              DBG ? &st : nullptr, s_tab[threadIdx.x / G]);
    }
    const bool far = !done && a.max_shell > 1;
    if constexpr (DBG) {
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            st.cells += __shfl_xor(st.cells, off, 64);
            st.points += __shfl_xor(st.points, off, 64);
        }
        if (sub == 0) {
            a.dbg[3 * (size_t)i] = st.cells;
            a.dbg[3 * (size_t)i + 1] = st.points;
            a.dbg[3 * (size_t)i + 2] = far ? 2 : st.shell;
        }
    }
    if (far) {
        if (sub == 0) {
            const int slot = atomicAdd(a.far_count, 1);  // < n: a query is queued once
            FarEntry e;
            e.i = whole ? (int)((unsigned)i | 0x80000000u) : i;  // sign bit: search the block too
            e.w[0] = wx, e.w[1] = wy, e.w[2] = wz;
#pragma unroll
            for (int j = 0; j < 5; ++j) e.k[j] = tk.k[j];
            e.pad = 0;
            a.far_q[slot] = e;
        }
        return;
    }
#pragma unroll
    for (int js = 0; js < 5; js += G) {
        const int jj = js + sub;
        if (jj < 5) {
            int v = tk.id(0);
#pragma unroll
            for (int j = 1; j < 5; ++j)
                if (jj == j) v = tk.id(j);
            a.nn_idx[5 * (size_t)i + jj] = v == kNone ? -1 : v;
        }
    }
    if (sub == 5) a.nn_d5[i] = tk.id(4) == kNone ? INFINITY : tk.d(4);
}

// Pass 2: the queued queries, one block each (block_knn_box_flat over the
// rest of the query's search box).  Fixed grid; every block strides the queue
// and exits once past its end.  A block's first entry is loaded together with
// the queue length (the queue holds at least gridDim.x entries, far_entries)
// and used only if the queue reaches it: one round trip before the search.
template <int NT = kFarBlock>
__global__ void __launch_bounds__(NT) knn_far_kernel(MatchArgs a) {
    __shared__ uint32_t s_b[NT], s_off[NT + 1], s_w[NT / 64];
    __shared__ uint64_t s_lists[(NT / 64) * 5];
    const FarEntry* __restrict__ fq = a.far_q;
    FarEntry e = fq[blockIdx.x];
    int cnt = *a.far_count;
    // both loads above are in flight before either is waited for (without this the compiler sinks the entry's
    // load behind the branch on the count: two dependent round trips)
    asm volatile("" : "+s"(cnt), "+v"(e.i), "+v"(e.w[0]), "+v"(e.k[0]), "+v"(e.k[2]), "+v"(e.k[4]));
    for (int f = blockIdx.x; f < cnt;) {
        const int i = e.i & 0x7fffffff;
        TopK<5> tk;
#pragma unroll
        for (int j = 0; j < 5; ++j) tk.k[j] = e.k[j];
        block_knn_box_flat<5, NT>(a.grid, e.w[0], e.w[1], e.w[2], s_b, s_off, s_w, s_lists, tk, e.i < 0);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 5; ++j) a.nn_idx[5 * (size_t)i + j] = tk.id(j) == kNone ? -1 : tk.id(j);
            a.nn_d5[i] = tk.id(4) == kNone ? INFINITY : tk.d(4);
        }
        f += gridDim.x;
        if (f < cnt) e = fq[f];
    }
}

// Block partial -> global, and the LAST block to finish sums all partials
// (fixed order: deterministic) into the host-mapped result + sequence number,
// so no separate finalize launch.  Hand-off per MI355X_MICROARCH.md
// § visibility, row "one lane of each storing workgroup ... agent-scope atomic
// add / the workgroup whose add came last": the partial is stored
// write-through (sc1: agent-scope relaxed atomic store), the storing wave
// drains (vmcnt(0)), a barrier, ONE lane adds to the counter; the block
// whose add returns nblocks-1 reads every partial with sc1 loads
// (agent-scope relaxed atomic loads) after a barrier.  No release fence (an
// agent release per block writes back the XCD's L2: 8 -> 35 us measured).
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) unsigned int guint;
typedef __attribute__((address_space(1))) unsigned long long gull;

// Host hand-off in ONE round trip: wave lanes 0-31 store the 32 sums, lane 32
// the sequence number, lane 33 a checksum of (sums, seq), all write-through at
// system scope (sc0 sc1) and unordered.  The host (lio_capi.cpp wait_result)
// accepts a result once it reads the expected sequence number AND sums whose
// checksum matches: a word still in flight (or the previous evaluation's)
// fails the check and the host polls again; once the kernel has completed,
// every word has landed.  No system release (its write-back and the wait for
// the sums' completion before the flag cost 1.7-2 us per evaluation).
// Called by all 64 lanes of one wave; lane l < 32 passes sum l.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {  // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ void publish_host(double t, double* out, unsigned long long* seq_out, unsigned long long seq) {
    const int lane = threadIdx.x & 63;
    unsigned long long h =
        lane < 32 ? mix64((unsigned long long)__double_as_longlong(t) ^ ((unsigned long long)lane * 0x9e3779b97f4a7c15ull))
                  : 0ull;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) h ^= __shfl_xor(h, off, 64);
    h = __shfl(h, 0, 64);
    if (lane < 32) __hip_atomic_store((gdouble*)(out + lane), t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (lane == 32) __hip_atomic_store((gull*)seq_out, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (lane == 33) __hip_atomic_store((gull*)(seq_out + 1), h ^ mix64(seq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Block partial -> global; returns true in the LAST block to finish, whose
// lanes < 32 then hold the 32 fixed-order sums in `t` (wave 0; block-uniform
// return value).
// slot: this block's partial index (-1: none); npart partials are summed; ncount
// blocks take part in the counter.  All threads of the block call it.
template <int BS = kBlock>
__device__ __forceinline__ bool block_partial_last(const MatchArgs& a, double (*red)[32], double& t, int slot, int npart,
                                                   int ncount) {
    __shared__ int s_last;
    const int nb = npart;
    t = 0.0;
    if (slot >= 0 && threadIdx.x < 32) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < BS / 64; ++w) s += red[w][threadIdx.x];
        __hip_atomic_store((gdouble*)(a.partials + (size_t)slot * 32 + threadIdx.x), s, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the storing wave drains
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add((guint*)a.done_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = old == (unsigned)(ncount - 1);
    }
    __syncthreads();
    if (!s_last) return false;  // block-uniform
    // fixed-order sum: 8 row groups x 32 columns, then the groups in order
    const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
    constexpr int NG = BS / 32;
    const int per = (nb + NG - 1) / NG;
    const int b0 = grp * per, b1 = min(nb, b0 + per);
    double acc = 0.0;
    int b = b0;
    // batches of 32 sc1 loads in flight per thread (cross-XCD: each batch is an L2 miss), the
    // last batch masked rather than finished one load at a time (a serial tail of 27 loads
    // doubled the kernel at C5's 469 blocks)
    for (; b < b1; b += 32) {
        double v[32];
#pragma unroll
        for (int k = 0; k < 32; ++k)
            v[k] = b + k < b1 ? __hip_atomic_load((gdouble*)(a.partials + (size_t)(b + k) * 32 + col), __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT)
                              : 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) acc += v[k];
    }
    __shared__ double sg[NG][33];
    sg[grp][col] = acc;
    __syncthreads();
    if (threadIdx.x < 32)
#pragma unroll
        for (int g = 0; g < NG; ++g) t += sg[g][threadIdx.x];
    if (threadIdx.x == 0)
        __hip_atomic_store((guint*)a.done_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
    return true;
}

// the last block publishes the sums to the host (lio_match)
template <int BS = kBlock>
__device__ __forceinline__ void publish_and_finalize(const MatchArgs& a, double (*red)[32]) {
    double t;
    if (block_partial_last<BS>(a, red, t, blockIdx.x, gridDim.x, gridDim.x) && threadIdx.x < 64)
        publish_host(t, a.sums_out, a.seq_out, a.seq);
}

// One lane's H-row contribution [HTH(21), HTh(6), cnt, res, hh] added into v[32].
__device__ __forceinline__ void accum_row(double (&v)[32], const double J[6], double h, double res, double cnt) {
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) v[q++] += J[r] * J[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) v[21 + r] += J[r] * h;
    v[27] += cnt;
    v[28] += res;
    v[29] += h * h;
}

// Plane pass body, lane = PPL points (strided by the block size, coalesced): gate
// (found == 5 && d2[4] <= 5), esti_plane, pd2, s-gate, H row, summed into v.
template <int PPL, int BS = kBlock>
__device__ __forceinline__ void plane_points(const MatchArgs& a, const PoseArg& ps, int blk, double (&v)[32]) {
    const int i0 = blk * BS * PPL + threadIdx.x;
    // all points' ids first, then all neighbour gathers: PPL independent chains in flight
    int id[PPL][5];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        const int i = i0 + k * BS;
#pragma unroll
        for (int j = 0; j < 5; ++j) id[k][j] = i < a.n ? a.nn_idx[5 * (size_t)i + j] : -1;
    }
    float P[PPL][5][3];
#pragma unroll
    for (int k = 0; k < PPL; ++k)
        if (id[k][4] >= 0)
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float4 q = a.map_by_id[id[k][j]];
                P[k][j][0] = q.x;
                P[k][j][1] = q.y;
                P[k][j][2] = q.z;
            }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        const int i = i0 + k * BS;
        if (i < a.n) {
            // sorted list: the 5th exists => all exist, d2 <= range by construction
            bool sel = id[k][4] >= 0;
            if (sel) {
                const float bx = a.body[3 * i], by = a.body[3 * i + 1], bz = a.body[3 * i + 2];
                float abcd[4];
                sel = esti_plane_dev(P[k], a.plane_thr, abcd);
                const float4 pl = make_float4(abcd[0], abcd[1], abcd[2], abcd[3]);
                a.planes[i] = pl;
                if (sel) {
                    float wx, wy, wz;
                    body_to_world(ps, bx, by, bz, wx, wy, wz);
                    double J[6], h, res;
                    sel = residual_row(a, ps, bx, by, bz, wx, wy, wz, pl, J, h, res);
                    if (sel) accum_row(v, J, h, res, 1.0);
                }
            }
            a.sel[i] = sel ? 1 : 0;
        }
    }
}

// Reuse pass body (ekfom_data.converge == false: cached Nearest_Points / planes), PPL points per lane.
template <int PPL, int BS = kBlock>
__device__ __forceinline__ void reuse_points(const MatchArgs& a, const PoseArg& ps, int blk, double (&v)[32]) {
    const int i0 = blk * BS * PPL + threadIdx.x;
    // every point's three loads issued together (one round trip instead of sel -> body/plane)
    bool sel[PPL];
    float b[PPL][3];
    float4 pl[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        const int i = i0 + k * BS;
        sel[k] = false;
        if (i < a.n) {
            sel[k] = a.sel[i] != 0;
            b[k][0] = a.body[3 * i];
            b[k][1] = a.body[3 * i + 1];
            b[k][2] = a.body[3 * i + 2];
            pl[k] = a.planes[i];
        }
    }
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        if (sel[k]) {
            const int i = i0 + k * BS;
            float wx, wy, wz;
            body_to_world(ps, b[k][0], b[k][1], b[k][2], wx, wy, wz);
            double J[6], h, res;
            const bool s = residual_row(a, ps, b[k][0], b[k][1], b[k][2], wx, wy, wz, pl[k], J, h, res);
            if (s) accum_row(v, J, h, res, 1.0);
            a.sel[i] = s ? 1 : 0;
        }
    }
}

// Pass 3 (kNN evaluations): plane_points, wave sums, the block's wave partials
// combined in LDS -> block partial; the last block publishes.  Resets the far
// queue for the next kNN evaluation.
template <int PPL, int BS>
__global__ void __launch_bounds__(BS) plane_kernel(MatchArgs a) {
    const PoseArg& ps = a.pose;
    __shared__ double red[BS / 64][32];
    double v[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) v[q] = 0.0;
    plane_points<PPL, BS>(a, ps, blockIdx.x, v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double tot = wave_sum32(v, lane);
    if (lane < 32) red[wid][wave_sum32_index(lane)] = tot;
    __syncthreads();
    publish_and_finalize<BS>(a, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.far_count = 0;
}

// ekfom_data.converge == false: reuse_points, same reduction and publish.
template <int PPL, int BS>
__global__ void __launch_bounds__(BS) h_model_reuse_kernel(MatchArgs a) {
    const PoseArg& ps = a.pose;
    __shared__ double red[BS / 64][32];
    double v[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) v[q] = 0.0;
    reuse_points<PPL, BS>(a, ps, blockIdx.x, v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double tot = wave_sum32(v, lane);
    if (lane < 32) red[wid][wave_sum32_index(lane)] = tot;
    __syncthreads();
    publish_and_finalize<BS>(a, red);
}

// ikd-Tree Nearest_Search(point, k, Nearest_Points, Point_Distance, max_dist)
// over a batch of query points: 8 lanes per query, exact (d2, id)-ordered
// 5-NN within d2 <= bound (bound = INFINITY: unbounded, any number of shells),
// the first k kept.  Missing neighbours: id -1, d2 = INFINITY.
__global__ void __launch_bounds__(256) map_knn_kernel(GridDev g, const float* __restrict__ q, int n, float bound,
                                                      int max_shell, int k, int32_t* __restrict__ idx,
                                                      float* __restrict__ d2) {
    constexpr int G = kGroup;
    const int sub = threadIdx.x % G;
    const int i = blockIdx.x * (256 / G) + threadIdx.x / G;
    if (i >= n) return;
    TopK<5> tk;
    tk.init(bound);
    const float qx = q[3 * (size_t)i], qy = q[3 * (size_t)i + 1], qz = q[3 * (size_t)i + 2];
    // a query that is not finite has no neighbours (group-uniform: the whole group skips the walk, which
    // would otherwise visit every shell, and for an infinite query accept every point at d2 = inf)
    if (isfinite(qx) && isfinite(qy) && isfinite(qz)) group_knn_exact<5, G>(g, qx, qy, qz, max_shell, sub, tk);
    if (sub < k) {
        int v = tk.id(0);
        float d = tk.d(0);
#pragma unroll
        for (int j = 1; j < 5; ++j)
            if (sub == j) {
                v = tk.id(j);
                d = tk.d(j);
            }
        const bool ok = v != kNone;
        idx[(size_t)i * k + sub] = ok ? v : -1;
        if (d2) d2[(size_t)i * k + sub] = ok ? d : INFINITY;
    }
}

// Debug: world points, d2 of the stored neighbours, pd2 of selected points.
__global__ void debug_kernel(MatchArgs a, float* __restrict__ world, float* __restrict__ d2,
                             float* __restrict__ abcd_pd2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    float wx, wy, wz;
    body_to_world(a.pose, a.body[3 * i], a.body[3 * i + 1], a.body[3 * i + 2], wx, wy, wz);
    if (world) {
        world[3 * i] = wx;
        world[3 * i + 1] = wy;
        world[3 * i + 2] = wz;
    }
    if (d2) {
        for (int j = 0; j < 5; ++j) {
            int id = a.nn_idx[5 * (size_t)i + j];
            float v = INFINITY;
            if (id >= 0) {
                float4 q = a.map_by_id[id];
                v = sqdist3(wx, wy, wz, q.x, q.y, q.z);
            }
            d2[5 * (size_t)i + j] = v;
        }
    }
    if (abcd_pd2) {
        float4 pl = make_float4(0, 0, 0, 0);
        float pd2 = 0.f;
        if (a.sel[i]) {
            pl = a.planes[i];
            pd2 = ((pl.x * wx + pl.y * wy) + pl.z * wz) + pl.w;
        }
        abcd_pd2[4 * (size_t)i] = pl.x;
        abcd_pd2[4 * (size_t)i + 1] = pl.y;
        abcd_pd2[4 * (size_t)i + 2] = pl.z;
        abcd_pd2[4 * (size_t)i + 3] = pd2;
    }
}

// Ordered compaction of the H rows of selected points (dof < 23 branch only):
// one block walks the points in index order.
__global__ void __launch_bounds__(1024) h_rows_kernel(MatchArgs a, double* __restrict__ rows, int64_t max_rows,
                                                      int64_t* __restrict__ n_rows) {
    __shared__ int wave_cnt[16];
    __shared__ int64_t base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int64_t off = 0; off < a.n; off += 1024) {
        const int64_t i = off + threadIdx.x;
        const bool s = i < a.n && a.sel[i];
        const unsigned long long m = __ballot(s);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wid] = __popcll(m);
        __syncthreads();
        int wbase = 0, tot = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wid) wbase += wave_cnt[w];
            tot += wave_cnt[w];
        }
        if (s) {
            const int64_t r = base + wbase + before;
            if (r < max_rows) {
                const float bx = a.body[3 * i], by = a.body[3 * i + 1], bz = a.body[3 * i + 2];
                float wx, wy, wz;
                body_to_world(a.pose, bx, by, bz, wx, wy, wz);
                const float4 pl = a.planes[i];
                const float pd2 = ((pl.x * wx + pl.y * wy) + pl.z * wz) + pl.w;
                double J[6];
                h_row(a.pose, bx, by, bz, pl.x, pl.y, pl.z, J);
                for (int k = 0; k < 6; ++k) rows[7 * r + k] = J[k];
                rows[7 * r + 6] = -(double)pd2;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_rows = base;
}

// ---------------------------------------------------------------- launchers
// The measured-best forms only (A/B history: DESIGN §4): near pass in 32-query blocks with 2 loads in
// flight in the seeded table scan and in the own-cell scan (no scratch spills); far pass one
// 128-thread block per queued query on a fixed 1024-block grid; plane pass 512 x 1 point per lane;
// reuse pass 512 x 2 points per lane.
int launch_h_model(const MatchArgs& a, bool redo, hipStream_t st, hipEvent_t* marks) {
    if (a.n == 0) return 0;
    // hipExtLaunchKernelGGL with null events is a plain launch; with events (timing) the command
    // processor stamps them at the kernel's own start / end
    hipEvent_t m[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (marks)
        for (int k = 0; k < 8; ++k) m[k] = marks[k];
    if (redo) {
        constexpr int qpb = kNearBlock / kGroup;
        const int nq = (a.n + qpb - 1) / qpb;
        if (a.dbg) {  // search statistics (lio_ctx_knn_stats): the per-query group walk
            hipExtLaunchKernelGGL((knn_near_kernel<true, false, 4, kNearBlock, 2>), dim3(nq), dim3(kNearBlock), 0, st,
                                  m[0], m[1], 0, a);
        } else if (a.prior) {
            hipExtLaunchKernelGGL((knn_near_kernel<false, true, 2, kNearBlock, 4>), dim3(nq), dim3(kNearBlock), 0, st,
                                  m[0], m[1], 0, a);
        } else {
            hipExtLaunchKernelGGL((knn_near_kernel<false, false, 4, kNearBlock, 2>), dim3(nq), dim3(kNearBlock), 0, st,
                                  m[0], m[1], 0, a);
        }
        if (a.max_shell > 1)
            hipExtLaunchKernelGGL((knn_far_kernel<kFarBlock>), dim3(kFarBlocks), dim3(kFarBlock), 0, st, m[2], m[3], 0, a);
        const int nbp = (a.n + kPlaneBlock - 1) / kPlaneBlock;
        hipExtLaunchKernelGGL((plane_kernel<1, kPlaneBlock>), dim3(nbp), dim3(kPlaneBlock), 0, st, m[4], m[5], 0, a);
        return nbp;
    }
    const int nbr = (a.n + kReusePpl * kReuseBlock - 1) / (kReusePpl * kReuseBlock);
    hipExtLaunchKernelGGL((h_model_reuse_kernel<kReusePpl, kReuseBlock>), dim3(nbr), dim3(kReuseBlock), 0, st, m[6],
                          m[7], 0, a);
    return nbr;
}

void launch_debug(const MatchArgs& a, float* world, float* d2, float* abcd_pd2, hipStream_t st) {
    if (a.n == 0) return;
    debug_kernel<<<(a.n + 255) / 256, 256, 0, st>>>(a, world, d2, abcd_pd2);
}

void launch_h_rows(const MatchArgs& a, double* rows, int64_t max_rows, int64_t* n_rows, hipStream_t st) {
    h_rows_kernel<<<1, 1024, 0, st>>>(a, rows, max_rows, n_rows);
}

void launch_map_knn(const GridDev& g, const float* q, int n, float bound, int max_shell, int k, int32_t* idx,
                    float* d2, hipStream_t st) {
    if (n <= 0) return;
    map_knn_kernel<<<(n + 256 / kGroup - 1) / (256 / kGroup), 256, 0, st>>>(g, q, n, bound, max_shell, k, idx, d2);
}

int64_t far_entries(int64_t n) {  // a far block loads entry blockIdx.x before it knows the queue's length
    return std::max<int64_t>(n, kFarBlocks);
}

int match_blocks(int n) {  // partial slots (plane / reuse kernels): n / 256 bounds both grids
    return (n + kBlock - 1) / kBlock;
}

}  // namespace lio
