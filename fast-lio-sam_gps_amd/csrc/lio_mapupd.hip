// lio_mapupd.hip — incremental map maintenance on gfx950:
//
//   map_add      ikd-Tree Add_Points(PointToAdd, downsample_on) [U]
//   map_delete   ikd-Tree Delete_Point_Boxes(cub_needrm) [U]
//   incremental  FAST-LIO map_incremental() [U] over a ctx's scan
//
// Add_Points processes its points one after another; the only coupling
// between points is through their downsample voxel, so the GPU groups the
// points by voxel (a hash table of voxel keys, a chain of input indices per
// voxel) and one lane per voxel replays its points in input order against the
// map points already in that voxel (found through the grid).  Survivors are
// appended to the id-order array in input order, replaced points become
// tombstones (by_id alive bit cleared, their grid slots compacted away) and the
// new ids go into the gapped grid's per-cell blocks (lio_grid.hip) — every step
// is O(points of this call), none touches the rest of the map, and an update is
// enqueued with ONE host synchronisation at its end (the counts stay on the
// device; launch sizes are the call's upper bounds).
// Semantics restated in oracle/lio_oracle.cpp (DynMap, map_incremental).
#include <rocprim/block/block_radix_sort.hpp>
#include <rocprim/block/block_scan.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "lio_grid_dev.hpp"
#include "lio_kernels.hpp"
#include "lio_mapupd.hpp"
#include "lio_scratch_cub.hpp"

namespace lio {

namespace {

constexpr int kVoxBits = 21;
constexpr int kVoxOff = 1 << 20;

__device__ __forceinline__ float calc_dist(float ax, float ay, float az, float bx, float by, float bz) {
    return sqdist3(ax, ay, az, bx, by, bz);
}
__device__ __forceinline__ bool same_point(float ax, float ay, float az, float bx, float by, float bz) {
    return fabsf(ax - bx) < 1e-6f && fabsf(ay - by) < 1e-6f && fabsf(az - bz) < 1e-6f;
}

struct VoxBox {
    float lo[3], hi[3], mid[3];
};

// Add_Points box: [floor(p/ds)*ds, +ds) (float), centre min + (max-min)/2.0 (double -> float)
__device__ __forceinline__ VoxBox vox_box(float x, float y, float z, float ds) {
    VoxBox b;
    const float p[3] = {x, y, z};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        b.lo[d] = floorf(p[d] / ds) * ds;
        b.hi[d] = b.lo[d] + ds;
        b.mid[d] = (float)((double)b.lo[d] + (double)(b.hi[d] - b.lo[d]) / 2.0);
    }
    return b;
}
__device__ __forceinline__ bool in_box(const VoxBox& b, float x, float y, float z) {
    return b.lo[0] <= x && b.hi[0] > x && b.lo[1] <= y && b.hi[1] > y && b.lo[2] <= z && b.hi[2] > z;
}

// per-call counters (device, u32: MapUpdBuf::d_cnt)
enum : int {
    kCTrig = 0,    // Add_Points triggers (voxels that changed)
    kCDead = 1,    // map points replaced (tombstones)
    kCAdd = 2,     // points offered to the downsampled add (PointToAdd)
    kCNoNeed = 3,  // PointNoNeedDownsample
    kCVox = 4,     // voxels touched by the downsampled add
    kCNew = 5,     // ids appended (survivors + no-need)
    kCSurv = 6,    // survivors of the downsampled add
    kCDirty = 7,   // grid cells holding tombstones
    kCPend = 8,    // map_incremental points queued for the unbounded kNN
    kCFlags = 9,   // 1 a point outside the grid, 2 slot pool exhausted, 4 tombstone cell list full
    kCTouch = 10,  // grid cells receiving points
    kCRuns = 11,   // voxel runs listed by group_sort_kernel
};
// kCFlags bit 16: some voxel's points span more than kMaxRuns sort blocks (group_sort_kernel): the update
// did nothing but reset the voxel table, and the host redoes it through the globally sorted path
constexpr uint32_t kFlagRuns = 16u;
// grouped update: sort blocks of kGrpB consecutive points (group_sort_kernel), the append in the same
// blocks (update_kernel)
constexpr int kGrpT = 256, kGrpI = 4, kGrpB = kGrpT * kGrpI;
constexpr int kMaxRuns = 64;  // runs a voxel may have (its points spread over <= 64 sort blocks)
// vox_resolve_kernel's trigger / tombstone totals: one pair of counters per 64-byte line, kSpread of them
// (block b adds to line b % kSpread), folded into cnt[kCTrig] / cnt[kCDead] and cleared by append_kernel.
// Thousands of waves adding to ONE device-scope counter serialise at the memory-side atomic unit
// (measured: 87 -> 35 us for vox_resolve at C3 without them, scripts/vox_ab.sh)
constexpr int kSpread = 64, kSpreadOff = 32, kSpreadStride = 16;
constexpr int kCntWords = kSpreadOff + kSpread * kSpreadStride;

constexpr unsigned long long kEmptyKey = ~0ull;

// map_incremental point classes
enum : uint8_t { kSkip = 0, kToAdd = 1, kNoNeed = 2 };

__device__ __forceinline__ unsigned long long voxel_key(float x, float y, float z, float ds) {
    const float p[3] = {x, y, z};
    unsigned long long k = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float f = floorf(p[d] / ds);
        const int v = (int)fminf(fmaxf(f, (float)-kVoxOff), (float)(kVoxOff - 1));
        k = (k << kVoxBits) | (unsigned long long)(uint32_t)(v + kVoxOff);
    }
    return k;
}

__device__ __forceinline__ uint32_t hash_slot(unsigned long long k, uint32_t mask) {  // splitmix64 finaliser
    k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ull;
    k = (k ^ (k >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)(k ^ (k >> 31)) & mask;
}

// Group the points [0, cnt[kCAdd]) by downsample voxel: an open-addressing table of voxel keys
// (linear probing, CAS), the lane that claims a slot lists the voxel; every point emits (slot, index)
// for a stable sort (points past the count: the sentinel slot hcap, sorted last), so each voxel's
// points end up contiguous and in input order whatever the voxel's size.
__global__ void vox_group_kernel(const float* __restrict__ xyz, float ds, unsigned long long* __restrict__ hkey,
                                 uint32_t hmask, int n_max, uint32_t* __restrict__ skey, uint32_t* __restrict__ sval,
                                 uint32_t* __restrict__ vlist, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if ((int)i >= n_max) return;
    sval[i] = i;
    if (i >= cnt[kCAdd]) {
        skey[i] = hmask + 1;
        return;
    }
    const unsigned long long key = voxel_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ds);
    uint32_t h = hash_slot(key, hmask);
    bool claimed = false;
    for (uint32_t probe = 0;; ++probe) {  // load <= 1/4: a free slot is always near
        const unsigned long long prev = atomicCAS(&hkey[h], kEmptyKey, key);
        if (prev == kEmptyKey) {
            claimed = true;
            break;
        }
        if (prev == key) break;
        if (probe > hmask) {  // unreachable for a clean table (guard): the point joins no voxel
            h = hmask + 1;
            break;
        }
        h = (h + 1) & hmask;
    }
    skey[i] = h;
    // the wave's new voxels listed with one counter add
    const uint64_t m = __ballot(claimed);
    if (claimed) {
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(&cnt[kCVox], (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader, 64);
        vlist[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = h;
    }
}

// the sorted run of each voxel: hhead[slot] = first entry, hend[slot] = one past the last
__global__ void vox_runs_kernel(const uint32_t* __restrict__ skey2, const uint32_t* __restrict__ sval2,
                                const float* __restrict__ xyz, int n_max, uint32_t hmask, int* __restrict__ hhead,
                                int* __restrict__ hend, float4* __restrict__ xs) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_max) return;
    const uint32_t k = skey2[j];
    if (k > hmask) return;
    if (j == 0 || skey2[j - 1] != k) hhead[k] = j;
    if (j == n_max - 1 || skey2[j + 1] != k) hend[k] = j + 1;
    const uint32_t i = sval2[j];  // the point in sorted order: one contiguous 16-B load per point later
    xs[j] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f);
}

// the cells a box [lo, hi) can touch: a point with lo <= p < hi has its (clamped) cell between the
// cells of lo and of the largest float below hi (the build's assignment is monotone per coordinate)
struct CellRange {
    int x0, x1, y0, y1, z0, z1;
};
__device__ __forceinline__ CellRange box_cells(const GridDev& g, const VoxBox& b, int grid_n) {
    CellRange r{0, -1, 0, -1, 0, -1};
    if (grid_n <= 0) return r;
    r.x0 = min(max(cell_coord(b.lo[0], g.ox, g.inv_cell), 0), g.nx - 1);
    r.x1 = min(max(cell_coord(nextafterf(b.hi[0], -INFINITY), g.ox, g.inv_cell), 0), g.nx - 1);
    r.y0 = min(max(cell_coord(b.lo[1], g.oy, g.inv_cell), 0), g.ny - 1);
    r.y1 = min(max(cell_coord(nextafterf(b.hi[1], -INFINITY), g.oy, g.inv_cell), 0), g.ny - 1);
    r.z0 = min(max(cell_coord(b.lo[2], g.oz, g.inv_cell), 0), g.nz - 1);
    r.z1 = min(max(cell_coord(nextafterf(b.hi[2], -INFINITY), g.oz, g.inv_cell), 0), g.nz - 1);
    return r;
}

// wave scans for vox_resolve_kernel (64 lanes, DPP: row shifts inside rows of 16, then row_bcast:15 /
// row_bcast:31 carry the row results forward; lanes without a source keep the identity)
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ float dpp_id_f(float v, float id) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(id), __float_as_int(v), CTRL, ROWS, 0xf, false));
}
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ int dpp_id_i(int v, int id) {
    return __builtin_amdgcn_update_dpp(id, v, CTRL, ROWS, 0xf, false);
}
__device__ __forceinline__ float wave_excl_min(float v, float init) {  // min(init, v of lanes below)
    v = fminf(v, dpp_id_f<0x111>(v, INFINITY));  // row_shr:1
    v = fminf(v, dpp_id_f<0x112>(v, INFINITY));  // row_shr:2
    v = fminf(v, dpp_id_f<0x114>(v, INFINITY));  // row_shr:4
    v = fminf(v, dpp_id_f<0x118>(v, INFINITY));  // row_shr:8
    v = fminf(v, dpp_id_f<0x142, 0xa>(v, INFINITY));  // row_bcast:15
    v = fminf(v, dpp_id_f<0x143, 0xc>(v, INFINITY));  // row_bcast:31
    return fminf(dpp_id_f<0x138>(v, INFINITY), init);  // wave_shr:1 -> exclusive
}
__device__ __forceinline__ int wave_excl_max(int v) {  // max(-1, v of lanes below)
    v = max(v, dpp_id_i<0x111>(v, -1));
    v = max(v, dpp_id_i<0x112>(v, -1));
    v = max(v, dpp_id_i<0x114>(v, -1));
    v = max(v, dpp_id_i<0x118>(v, -1));
    v = max(v, dpp_id_i<0x142, 0xa>(v, -1));
    v = max(v, dpp_id_i<0x143, 0xc>(v, -1));
    return dpp_id_i<0x138>(v, -1);
}
__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
// vox_resolve_kernel's super-chunk: K contiguous points per lane (one 128-byte line), all loads in flight
constexpr int kVoxK = 8;
__device__ __forceinline__ void load_super(const float4* __restrict__ xs, int lb, int s1, float4 (&q)[kVoxK]) {
#pragma unroll
    for (int k = 0; k < kVoxK; ++k) q[k] = lb + k < s1 ? xs[lb + k] : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The box's cells cb .. cb + 63 (of nbc): lane l loads cell cb + l's range; tb[0 .. 64) range starts,
// tb[64 .. 129) exclusive offsets (tb[64 + 64] = total).  Returns the round's point count T.
__device__ __forceinline__ uint32_t box_cell_index(const GridDev& g, const CellRange& cr, int k, int bnx, int bny) {
    const int x = cr.x0 + k % bnx, y = cr.y0 + (k / bnx) % bny, z = cr.z0 + k / (bnx * bny);
    return ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx + (uint32_t)x;
}
__device__ __forceinline__ uint32_t box_table(const GridDev& g, const CellRange& cr, int cb, int nbc, int bnx, int bny,
                                              uint32_t* tb) {
    const int lane = threadIdx.x & 63;
    const int k = cb + lane;
    uint32_t rb = 0, rn = 0;
    if (k < nbc) {
        const uint2 r = g.rng[box_cell_index(g, cr, k, bnx, bny)];
        rb = r.x;
        rn = r.y - r.x;
    }
    uint32_t incl = rn;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    const uint32_t T = (uint32_t)__shfl(incl, 63, 64);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the previous round's readers are done
    __builtin_amdgcn_wave_barrier();
    tb[lane] = rb;
    tb[64 + lane] = incl - rn;
    if (lane == 63) tb[128] = T;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return T;
}
// the table entry (box cell of this round) holding concatenated point t: last k with off[k] <= t
__device__ __forceinline__ int box_cell_of(const uint32_t* tb, uint32_t t) {
    int lo = 0, hi = 64;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb[64 + mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t box_slot(const uint32_t* tb, uint32_t t) {
    const int k = box_cell_of(tb, t);
    return tb[k] + (t - tb[64 + k]);
}

// One WAVE per voxel: Add_Points' sequence for the voxel's points (input order) against the alive
// map points in its box [U] (oracle DynMap::add_points):
//   S := map points in the box; for each new point q:
//     winner = q unless some s in S has calc_dist(s, mid) < calc_dist(q, mid) (strict: among equal
//              distances the first in id order);
//     if |S| > 1 or same_point(q, winner): S := {winner}, counter++
// then every map point of the box except a surviving map point becomes a tombstone (by_id alive
// bit cleared, its grid slot marked (id bits kNone) for grid_compact_cells, its cell listed once),
// and add_flag marks the new point that survives (at most one per voxel).  The table slot is reset
// for the next call.  The voxel's points are sval2[hhead .. hend), ascending input indices.
// The lanes stride the box's cells (count, nearest map point, tombstones), and the sequence runs 64
// points at a time as scans: q wins iff !(running minimum before it < its distance), the running
// minimum is a prefix min, the winner q is compared with (same_point) is the last earlier winner
// (a prefix max of winner positions), the survivor is the last winner — the sequential result.
//
// The voxel's points come as runs of sorted positions: RUNS = false, one run sval2 / xs[hhead .. hend)
// of the globally sorted arrays; RUNS = true, the runs group_sort_kernel listed for the voxel (one per
// sort block holding its points, each in input order), sorted by position here, so that their
// concatenation is the voxel's points in input order.  The wave's run table (starts, offsets) maps a
// voxel position p (0 .. c) to a sorted position.
struct VoxArgs {
    const uint32_t* vlist;
    unsigned long long* hkey;
    int* hhead;              // RUNS = false: first sorted entry; RUNS = true: the voxel's run list (-1)
    const int* hend;         // RUNS = false: one past the last entry
    uint32_t* vnruns;        // RUNS = true: runs per voxel (reset here)
    const uint4* runs;       // RUNS = true: run records {first sorted position, count, next, -}
    const uint32_t* sval;    // input index at each sorted position
    const float4* xs;        // its coordinates
    const float* xyz;
    float ds;
    GridDev g;
    int grid_n;
    float4* pts;
    float4* by_id;
    uint8_t* dirty;
    uint32_t* dlist;
    uint32_t dcap;
    uint32_t* cnt;
    uint32_t* add_flag;
    uint32_t* blk_surv;      // RUNS = true: survivors per sort block (the append ranks)
};

// sorted position of voxel position p (rt: run starts, ro: run offsets, R runs, ro[R] = count)
__device__ __forceinline__ uint32_t run_pos(const uint32_t* rt, const uint32_t* ro, int R, uint32_t p) {
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ro[mid] <= p) lo = mid;
        else hi = mid;
    }
    return rt[lo] + (p - ro[lo]);
}
// lane's K points p0 .. p0 + K - 1 (< c) through the run table (one search, then run steps)
__device__ __forceinline__ void load_super_runs(const float4* __restrict__ xs, const uint32_t* rt, const uint32_t* ro,
                                                int R, uint32_t p0, uint32_t c, float4 (&q)[kVoxK]) {
    if (R == 1) {  // wave-uniform: one contiguous run
        load_super(xs, (int)(rt[0] + p0), (int)(rt[0] + c), q);
        return;
    }
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ro[mid] <= p0) lo = mid;
        else hi = mid;
    }
#pragma unroll
    for (int k = 0; k < kVoxK; ++k) {
        const uint32_t p = p0 + (uint32_t)k;
        while (lo + 1 < R && ro[lo + 1] <= p) ++lo;
        q[k] = p < c ? xs[rt[lo] + (p - ro[lo])] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <bool RUNS>
__global__ void __launch_bounds__(256) vox_resolve_kernel(VoxArgs a) {
    __shared__ uint32_t s_tab[4][2 * 64 + 1 + 64];  // per wave: box-cell table + tombstone flags
    __shared__ uint32_t s_run[4][2 * 64 + 1];       // per wave: run table (starts, offsets)
    const int lane = threadIdx.x & 63;
    __shared__ uint32_t s_tot[2][4];
    const uint32_t nvox = a.cnt[kCVox];
    const GridDev& g = a.g;
    // RUNS: a voxel spanning too many sort blocks -> reset the table only (the host redoes the update)
    const bool abandon = RUNS && (a.cnt[kCFlags] & kFlagRuns);
    uint32_t trig_acc = 0, dead_acc = 0;  // this lane's share of the block's totals
    for (uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6); v < nvox; v += gridDim.x * 4u) {  // wave-uniform
        const uint32_t h = a.vlist[v];
        const unsigned long long vkey = a.hkey[h];
        uint32_t* rt = s_run[threadIdx.x >> 6];
        uint32_t* ro = rt + 64;
        int R = 1;
        uint32_t c = 0;
        if constexpr (RUNS) {
            if (abandon) {
                if (lane == 0) {
                    a.hkey[h] = kEmptyKey;
                    a.hhead[h] = -1;
                    a.vnruns[h] = 0u;
                }
                continue;
            }
            // walk the voxel's run list (a few runs: one per sort block holding its points), lane r keeps
            // run r; sort the runs by position (bitonic over the wave), prefix their counts
            int rec = a.hhead[h];
            unsigned long long key = ~0ull;
            R = 0;
            while (rec >= 0 && R < 64) {  // wave-uniform (group_sort_kernel flags > kMaxRuns runs)
                const uint4 rr = a.runs[rec];
                if (lane == R) key = ((unsigned long long)rr.x << 32) | rr.y;
                rec = (int)rr.z;
                ++R;
            }
            if (R == 0) continue;
            if (R > 1) {
#pragma unroll
                for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
                    for (int j = k >> 1; j > 0; j >>= 1) {
                        const unsigned long long o = __shfl_xor(key, j, 64);
                        const bool keep_min = ((lane & k) == 0) == ((lane & j) == 0);
                        key = keep_min ? (o < key ? o : key) : (o > key ? o : key);
                    }
            }
            const uint32_t cntr = lane < R ? (uint32_t)key : 0u;
            uint32_t incl = cntr;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = __shfl_up(incl, off, 64);
                if (lane >= off) incl += y;
            }
            c = (uint32_t)__shfl((int)incl, 63, 64);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the previous voxel's readers are done
            __builtin_amdgcn_wave_barrier();
            rt[lane] = (uint32_t)(key >> 32);
            ro[lane] = incl - cntr;
            if (lane == 63) ro[64] = c;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            const int s0 = a.hhead[h], s1 = a.hend[h];
            if (s0 < 0) continue;
            c = (uint32_t)(s1 - s0);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) rt[0] = (uint32_t)s0, ro[0] = 0u, ro[1] = c;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        // the first super-chunk of the voxel's points (lane l: points l * K .. l * K + K - 1, contiguous),
        // loaded while the map side runs
        float4 q[kVoxK];
        load_super_runs(a.xs, rt, ro, R, (uint32_t)(lane * kVoxK), c, q);
        // the box from the voxel key (floor(p / ds) per axis, vox_box's own values) unless an axis was
        // clamped in the key: then from the voxel's first point, as before
        VoxBox b;
        bool clamped = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float ds = a.ds;
            const int idx = (int)((vkey >> (kVoxBits * (2 - d))) & ((1ull << kVoxBits) - 1)) - kVoxOff;
            clamped |= idx <= -kVoxOff || idx >= kVoxOff - 1;
            b.lo[d] = (float)idx * ds;
            b.hi[d] = b.lo[d] + ds;
            b.mid[d] = (float)((double)b.lo[d] + (double)(b.hi[d] - b.lo[d]) / 2.0);
        }
        const float ds = a.ds;
        if (clamped) {
            const int first_i = (int)a.sval[rt[0]];
            b = vox_box(a.xyz[3 * first_i], a.xyz[3 * first_i + 1], a.xyz[3 * first_i + 2], ds);
        }
        const CellRange cr = box_cells(g, b, a.grid_n);
        // the box's cells (<= 64 handled per round: one per lane), their ranges concatenated through the
        // wave's LDS table so the lanes stride all the box's map points at once (no per-cell round trips)
        const int bnx = cr.x1 - cr.x0 + 1, bny = cr.y1 - cr.y0 + 1;
        const int nbc = cr.x0 > cr.x1 ? 0 : bnx * bny * (cr.z1 - cr.z0 + 1);
        uint32_t* tb = s_tab[threadIdx.x >> 6];
        // map points in the box: how many, and the nearest to the centre (lowest id among equals)
        int cnt_l = 0;
        unsigned long long best_l = ~0ull;
        float blx = 0.f, bly = 0.f, blz = 0.f;
        uint32_t T1 = 0;  // one round (<= 64 box cells): the table stays in LDS for the tombstone pass
        for (int cb = 0; cb < nbc; cb += 64) {
            const uint32_t T = box_table(g, cr, cb, nbc, bnx, bny, tb);
            T1 = T;
            for (uint32_t t = (uint32_t)lane; t < T; t += 64u) {
                const float4 p = a.pts[box_slot(tb, t)];
                if (!in_box(b, p.x, p.y, p.z)) continue;
                ++cnt_l;
                const float dd = calc_dist(p.x, p.y, p.z, b.mid[0], b.mid[1], b.mid[2]);
                const unsigned long long kk =
                    ((unsigned long long)__float_as_uint(dd) << 32) | (uint32_t)__float_as_int(p.w);
                if (kk < best_l) {
                    best_l = kk;
                    blx = p.x;
                    bly = p.y;
                    blz = p.z;
                }
            }
        }
        const int cnt_e = wave_sum_i(cnt_l);
        const unsigned long long best = wave_min_u64(best_l);
        const int best_id = cnt_e > 0 ? (int)(uint32_t)best : -1;
        float sx = 0.f, sy = 0.f, sz = 0.f;  // the current winner (the nearest map point first)
        if (cnt_e > 0) {  // from the lane that holds it (keys are unique: (distance, id))
            const unsigned long long hm = __ballot(best_l == best);
            const int src = __ffsll((long long)hm) - 1;
            sx = __shfl(blx, src, 64);
            sy = __shfl(bly, src, 64);
            sz = __shfl(blz, src, 64);
        }
        // the sequence, 64 x K points per super-chunk: each lane walks its K contiguous points three times
        // (its minimum; after the wave's exclusive prefix minimum, its winners; after the wave's
        // exclusive last-winner scan, its triggers), so a voxel of c points costs c / (64 K) wave scans
        // instead of c / 64 (the densest voxel of a Livox scan holds thousands of points)
        float sd = cnt_e > 0 ? __uint_as_float((uint32_t)(best >> 32)) : INFINITY;
        int surv_pos = -1;  // voxel position of the last new winner
        const int s0 = 0, s1 = (int)c;
        for (int e0 = s0; e0 < s1; e0 += 64 * kVoxK) {
            if (e0 != s0) load_super_runs(a.xs, rt, ro, R, (uint32_t)(e0 + lane * kVoxK), c, q);
            const int lb = e0 + lane * kVoxK;  // this lane's first point
            float qd[kVoxK];
            float m = INFINITY;
#pragma unroll
            for (int k = 0; k < kVoxK; ++k) {
                qd[k] = lb + k < s1 ? calc_dist(q[k].x, q[k].y, q[k].z, b.mid[0], b.mid[1], b.mid[2]) : INFINITY;
                m = fminf(m, qd[k]);
            }
            // q wins iff !(running minimum before it < its distance)
            float r = wave_excl_min(m, sd);
            uint32_t wbits = 0;
            int lastk = -1;
            float wxl = 0.f, wyl = 0.f, wzl = 0.f;  // this lane's last winner
#pragma unroll
            for (int k = 0; k < kVoxK; ++k) {
                if (lb + k < s1 && !(r < qd[k])) {
                    wbits |= 1u << k;
                    lastk = k;
                    wxl = q[k].x;
                    wyl = q[k].y;
                    wzl = q[k].z;
                }
                r = fminf(r, qd[k]);
            }
            // the winner in force at this lane's first point: the last winner of the lanes below, else
            // the one carried in from the previous super-chunk (or the nearest map point)
            const int lw = wave_excl_max(lastk >= 0 ? lane : -1);
            const int src = lw < 0 ? 0 : lw;
            float cx = __shfl(wxl, src, 64), cy = __shfl(wyl, src, 64), cz = __shfl(wzl, src, 64);
            if (lw < 0) cx = sx, cy = sy, cz = sz;
#pragma unroll
            for (int k = 0; k < kVoxK; ++k) {
                const bool w = (wbits >> k) & 1u;
                const bool tr = lb + k < s1 && ((lb + k == s0 && cnt_e > 1) || w || same_point(q[k].x, q[k].y, q[k].z, cx, cy, cz));
                trig_acc += tr ? 1u : 0u;
                if (w) cx = q[k].x, cy = q[k].y, cz = q[k].z;
            }
            const unsigned long long wm = __ballot(lastk >= 0);
            if (wm) {  // the super-chunk's last winner: the survivor so far
                const int last = 63 - __clzll((long long)wm);
                sx = __shfl(wxl, last, 64);
                sy = __shfl(wyl, last, 64);
                sz = __shfl(wzl, last, 64);
                surv_pos = e0 + last * kVoxK + __shfl(lastk, last, 64);
            }
            sd = fminf(sd, wave_min_f(m));
        }
        const int surv_new = surv_pos >= 0 ? (int)a.sval[run_pos(rt, ro, R, (uint32_t)surv_pos)] : -1;
        if (cnt_e > 0 && (surv_new >= 0 || cnt_e > 1)) {
            for (int cb = 0; cb < nbc; cb += 64) {
                const uint32_t T = nbc <= 64 ? T1 : box_table(g, cr, cb, nbc, bnx, bny, tb);
                uint32_t* marked = tb + 2 * 64 + 1;  // per box cell of this round: holds a new tombstone
                marked[lane] = 0u;
                __builtin_amdgcn_wave_barrier();
                for (uint32_t t = (uint32_t)lane; t < T; t += 64u) {
                    const uint32_t slot = box_slot(tb, t);
                    const float4 p = a.pts[slot];
                    if (!in_box(b, p.x, p.y, p.z)) continue;
                    const int id = __float_as_int(p.w);
                    if (surv_new < 0 && id == best_id) continue;
                    a.by_id[id].w = 0.f;
                    a.pts[slot].w = __int_as_float(kNone);
                    ++dead_acc;
                    marked[box_cell_of(tb, t)] = 1u;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int kk = cb + lane;
                uint32_t cc = 0;
                bool fresh = false;  // list the cell once: the wave that sets its dirty byte
                if (kk < nbc && marked[lane]) {
                    cc = box_cell_index(g, cr, kk, bnx, bny);
                    unsigned int* wp = reinterpret_cast<unsigned int*>(a.dirty + (cc & ~3u));
                    const unsigned int bit = 1u << (8u * (cc & 3u));
                    fresh = !(atomicOr(wp, bit) & bit);
                }
                const uint64_t fm = __ballot(fresh);
                if (fm) {  // the wave's fresh cells listed with one counter add
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&a.cnt[kCDirty], (uint32_t)__popcll(fm));
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    if (fresh) {
                        const uint32_t sl = base + lane_rank(fm);
                        if (sl < a.dcap) a.dlist[sl] = cc;
                        else atomicOr(&a.cnt[kCFlags], 4u);  // list full: the caller rebuilds the grid
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (lane == 0) {
            if (surv_new >= 0) {
                a.add_flag[surv_new] = 1u;
                if constexpr (RUNS) atomicAdd(&a.blk_surv[surv_new / kGrpB], 1u);
            }
            a.hkey[h] = kEmptyKey;  // the table is clean again for the next call
            a.hhead[h] = -1;
            if constexpr (RUNS) a.vnruns[h] = 0u;
        }
    }
    // the block's totals: one add per counter to this block's spread line
    const int tw = wave_sum_i((int)trig_acc), dw = wave_sum_i((int)dead_acc);
    if (lane == 0) {
        s_tot[0][threadIdx.x >> 6] = (uint32_t)tw;
        s_tot[1][threadIdx.x >> 6] = (uint32_t)dw;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t t = s_tot[threadIdx.x][0] + s_tot[threadIdx.x][1] + s_tot[threadIdx.x][2] + s_tot[threadIdx.x][3];
        if (t) atomicAdd(&a.cnt[kSpreadOff + (blockIdx.x % kSpread) * kSpreadStride + threadIdx.x], t);
    }
}

// survivors (add_flag, pos = its exclusive scan) then the no-need points appended as ids id0 ..;
// thread 0 publishes the counts
__global__ void append_kernel(const float* __restrict__ xyz_a, const uint32_t* __restrict__ add_flag,
                              const uint32_t* __restrict__ pos, const float* __restrict__ xyz_b, int n_max, int64_t id0,
                              float4* __restrict__ by_id, uint32_t* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_add = cnt[kCAdd], n_nn = cnt[kCNoNeed];
    const uint32_t n_surv = pos[n_add];
    if (i == 0) {
        cnt[kCSurv] = n_surv;
        cnt[kCNew] = n_surv + n_nn;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {  // vox_resolve's spread totals -> cnt[kCTrig], cnt[kCDead]
        uint32_t* sp = cnt + kSpreadOff + threadIdx.x * kSpreadStride;
        const int t = wave_sum_i((int)sp[0]), d = wave_sum_i((int)sp[1]);
        sp[0] = 0u;
        sp[1] = 0u;
        if (threadIdx.x == 0) {
            cnt[kCTrig] += (uint32_t)t;
            cnt[kCDead] += (uint32_t)d;
        }
    }
    if (i >= n_max) return;
    if ((uint32_t)i < n_add && add_flag[i])
        by_id[id0 + pos[i]] = make_float4(xyz_a[3 * i], xyz_a[3 * i + 1], xyz_a[3 * i + 2], 1.f);
    if ((uint32_t)i < n_nn) by_id[id0 + n_surv + i] = make_float4(xyz_b[3 * i], xyz_b[3 * i + 1], xyz_b[3 * i + 2], 1.f);
}

__global__ void set_u32_kernel(uint32_t* __restrict__ p, uint32_t v) { *p = v; }

// ---- grouped update: voxels grouped inside sort blocks, no global sort ------------------------
//
// group_sort_kernel: one block per kGrpB consecutive points.  Each point offered to the downsampled add
// claims its voxel's table slot (CAS; the claimer lists the voxel), the block sorts its points by slot
// (LSD radix sort: stable, so each slot's points stay in input order) and lists one run per slot present
// in the block on the slot's run list {first sorted position, count, next}.  A voxel's points are the
// concatenation of its runs in block order (vox_resolve_kernel<true> sorts the few runs by position).
// Replaces the global (slot, index) sort: one launch instead of ten (rocprim block sort + 7 merges).

struct GroupArgs {
    const float* xyz;   // n x 3
    const uint8_t* cls; // per point class, or null: every point is all_cls
    int all_cls;
    int n;
    float ds;
    unsigned long long* hkey;
    uint32_t hmask;
    int hbits;
    int* vhead;         // per slot: run list head (-1)
    uint32_t* vnruns;   // per slot: runs listed
    uint4* runs;        // run records
    uint32_t* sidx;     // n: input index at each sorted position
    float4* xs;         // n: its coordinates
    uint32_t* vlist;
    uint32_t* add_flag; // n: cleared here (vox_resolve marks the survivors)
    uint32_t* cnt;
    uint32_t* blk_surv; // per block: survivors (zeroed here, counted by vox_resolve)
    uint32_t* blk_nn;   // per block: no-need points
};

__global__ void __launch_bounds__(kGrpT) group_sort_kernel(GroupArgs a) {
    using Sort = rocprim::block_radix_sort<uint32_t, kGrpT, kGrpI, uint32_t>;
    using Scan = rocprim::block_scan<uint32_t, kGrpT>;
    __shared__ typename Sort::storage_type s_sort;
    __shared__ typename Scan::storage_type s_scan;
    __shared__ uint32_t s_keys[kGrpB + 1];
    __shared__ uint32_t s_add[2][4];
    const int lane = threadIdx.x & 63;
    const int base = (int)blockIdx.x * kGrpB;
    const uint32_t sent = a.hmask + 1;  // sorts last: points not offered to the downsampled add
    // 1. striped (item base + j * kGrpT + t: 64 consecutive points per wave and j): classify, voxel key,
    // claim.  Points of one voxel are mostly consecutive, so the wave's lanes are grouped by key first
    // (ballot matching) and only one lane per distinct key probes the table — thousands of CAS on one
    // slot (a dense voxel) would serialise at the atomic unit.
    uint32_t n_add = 0, n_nn = 0;
#pragma unroll 1
    for (int j = 0; j < kGrpI; ++j) {
        const int off = j * kGrpT + (int)threadIdx.x, i = base + off;
        bool want = false;
        unsigned long long vk = 0;
        if (i < a.n) {
            a.add_flag[i] = 0u;
            const int c = a.cls ? (int)a.cls[i] : a.all_cls;
            if (c == kToAdd) {
                vk = voxel_key(a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2], a.ds);
                want = true;
                ++n_add;
            }
            n_nn += c == kNoNeed ? 1u : 0u;
        }
        // runs of equal keys among neighbouring lanes: the run's first lane probes for all of them (all
        // run leaders probe at once; a key repeated further away probes again and finds its slot)
        const unsigned long long vprev = (unsigned long long)__shfl_up((long long)vk, 1, 64);
        const bool wprev = __shfl_up((int)want, 1, 64) != 0;
        const uint64_t starts = __ballot(want && (lane == 0 || !wprev || vprev != vk));
        const int ld = want ? 63 - __clzll((long long)(starts & (~0ull >> (63 - lane)))) : lane;
        uint32_t h = 0, mine = 0;
        bool listed = false;  // this lane claimed a new voxel's slot (`mine`)
        if (want && ld == lane) {
            h = hash_slot(vk, a.hmask);
            for (uint32_t probe = 0;; ++probe) {  // load <= 1/4: a free slot is always near
                const unsigned long long prev = atomicCAS(&a.hkey[h], kEmptyKey, vk);
                if (prev == kEmptyKey) {
                    listed = true;
                    mine = h;
                    break;
                }
                if (prev == vk) break;
                if (probe > a.hmask) {  // unreachable for a clean table (guard): the points join no voxel
                    h = sent;
                    break;
                }
                h = (h + 1u) & a.hmask;
            }
        }
        h = (uint32_t)__shfl((int)h, ld, 64);
        const uint32_t slot = want ? h : sent;
        s_keys[off] = slot;
        const uint64_t lm = __ballot(listed);
        if (lm) {  // the wave's new voxels listed with one counter add
            uint32_t b0 = 0;
            if (lane == 0) b0 = atomicAdd(&a.cnt[kCVox], (uint32_t)__popcll(lm));
            b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
            if (listed) a.vlist[b0 + lane_rank(lm)] = mine;
        }
    }
    {  // points offered to the downsampled add: one counter add per block; the block's no-need points
        const int w = wave_sum_i((int)n_add), w2 = wave_sum_i((int)n_nn);
        if (lane == 0) s_add[0][threadIdx.x >> 6] = (uint32_t)w, s_add[1][threadIdx.x >> 6] = (uint32_t)w2;
    }
    __syncthreads();
    // 2. blocked (thread t: points t K .. t K + K - 1, the sort's input order) for the stable sort
    uint32_t key[kGrpI], val[kGrpI];
#pragma unroll
    for (int j = 0; j < kGrpI; ++j) {
        key[j] = s_keys[threadIdx.x * kGrpI + j];
        val[j] = (uint32_t)(base + (int)threadIdx.x * kGrpI + j);
    }
    __syncthreads();  // s_keys is rewritten below
    Sort().sort(key, val, s_sort, 0, (unsigned)a.hbits + 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = s_add[0][0] + s_add[0][1] + s_add[0][2] + s_add[0][3];
        if (t) atomicAdd(&a.cnt[kCAdd], t);
        a.blk_nn[blockIdx.x] = s_add[1][0] + s_add[1][1] + s_add[1][2] + s_add[1][3];
        a.blk_surv[blockIdx.x] = 0u;
    }
#pragma unroll
    for (int j = 0; j < kGrpI; ++j) s_keys[threadIdx.x * kGrpI + j] = key[j];
    if (threadIdx.x == 0) s_keys[kGrpB] = ~0u;
    __syncthreads();
    uint32_t st[kGrpI];
    bool end[kGrpI];
#pragma unroll
    for (int j = 0; j < kGrpI; ++j) {
        const uint32_t p = threadIdx.x * kGrpI + (uint32_t)j;
        st[j] = (p == 0 || s_keys[p - 1] != key[j]) ? p : 0u;
        end[j] = s_keys[p + 1] != key[j];
    }
    uint32_t rs[kGrpI];  // each point's run start: inclusive max scan of the start positions
    Scan().inclusive_scan(st, rs, s_scan, rocprim::maximum<uint32_t>());
#pragma unroll
    for (int j = 0; j < kGrpI; ++j) {
        const uint32_t p = threadIdx.x * kGrpI + (uint32_t)j;
        const bool valid = key[j] < sent;
        if (valid) {
            const uint32_t i = val[j];
            a.sidx[base + p] = i;
            a.xs[base + p] = make_float4(a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2], 0.f);
        }
        const bool emit = valid && end[j];
        const uint64_t m = __ballot(emit);
        if (m) {  // the wave's runs: one counter add, then each run pushed on its slot's list
            uint32_t b0 = 0;
            if (lane == 0) b0 = atomicAdd(&a.cnt[kCRuns], (uint32_t)__popcll(m));
            b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
            if (emit) {
                const uint32_t rec = b0 + lane_rank(m);
                const int next = atomicExch(&a.vhead[key[j]], (int)rec);
                a.runs[rec] = make_uint4((uint32_t)base + rs[j], p - rs[j] + 1u, (uint32_t)next, 0u);
                if (atomicAdd(&a.vnruns[key[j]], 1u) >= (uint32_t)kMaxRuns) atomicOr(&a.cnt[kCFlags], kFlagRuns);
            }
        }
    }
}

// One launch for everything between vox_resolve and the block growth: blocks [0, nb_app) take the
// sort blocks' points again (kGrpB each) and append the survivors (ids id0 + rank, input order), then
// the no-need points (id0 + survivors + rank) to by_id, ranking each new id in its grid cell
// (insert_rank_point); a rank = the earlier blocks' counts (blk_surv / blk_nn, <= a few hundred) + a
// block scan, so no device-wide scan.  The other blocks compact the cells holding tombstones (one wave
// per cell): disjoint state.  Block 0 also folds vox_resolve's spread counters and publishes the counts.
struct UpdArgs {
    const float* xyz;
    const uint8_t* cls;
    int all_cls;
    int n;
    const uint32_t* add_flag;
    const uint32_t* blk_surv;
    const uint32_t* blk_nn;
    int64_t id0;
    float4* by_id;
    GridGeom geom;
    uint32_t* addc;
    uint32_t* tmp_cell;
    uint32_t* tmp_rank;
    uint32_t* tlist;
    uint32_t* cnt;
    float4* pts;
    uint2* rng;
    uint8_t* dirty;
    const uint32_t* dlist;
    uint32_t dcap;
    int nb_app;
};

__global__ void __launch_bounds__(kGrpT) update_kernel(UpdArgs a) {
    using Scan = rocprim::block_scan<unsigned long long, kGrpT>;
    __shared__ typename Scan::storage_type s_scan;
    __shared__ uint32_t s_pre[3];
    if (a.cnt[kCFlags] & kFlagRuns) return;  // abandoned update (block-uniform)
    const int lane = threadIdx.x & 63;
    const int b = (int)blockIdx.x;
    if (b < a.nb_app) {
        if (threadIdx.x < 64) {  // wave 0: the earlier blocks' counts and the survivor total
            uint32_t sb = 0, nb = 0, st = 0, nt = 0;
            for (int k = lane; k < a.nb_app; k += 64) {
                const uint32_t s1 = a.blk_surv[k], n1 = a.blk_nn[k];
                st += s1;
                nt += n1;
                if (k < b) sb += s1, nb += n1;
            }
            sb = (uint32_t)wave_sum_i((int)sb);
            nb = (uint32_t)wave_sum_i((int)nb);
            st = (uint32_t)wave_sum_i((int)st);
            nt = (uint32_t)wave_sum_i((int)nt);
            if (lane == 0) {
                s_pre[0] = sb;
                s_pre[1] = nb;
                s_pre[2] = st;
                if (b == 0) {
                    a.cnt[kCSurv] = st;
                    a.cnt[kCNew] = st + nt;
                    a.cnt[kCNoNeed] = nt;
                }
            }
            if (b == 0) {  // vox_resolve's spread totals -> cnt[kCTrig], cnt[kCDead]
                uint32_t* sp = a.cnt + kSpreadOff + threadIdx.x * kSpreadStride;
                const int t = wave_sum_i((int)sp[0]), d = wave_sum_i((int)sp[1]);
                sp[0] = 0u;
                sp[1] = 0u;
                if (threadIdx.x == 0) {
                    a.cnt[kCTrig] += (uint32_t)t;
                    a.cnt[kCDead] += (uint32_t)d;
                }
            }
        }
        unsigned long long f[kGrpI], r[kGrpI];
#pragma unroll
        for (int j = 0; j < kGrpI; ++j) {  // blocked, as group_sort_kernel: input order
            const int i = b * kGrpB + (int)threadIdx.x * kGrpI + j;
            f[j] = 0ull;
            if (i < a.n) {
                const int c = a.cls ? (int)a.cls[i] : a.all_cls;
                f[j] = (unsigned long long)(a.add_flag[i] ? 1u : 0u) | ((unsigned long long)(c == kNoNeed ? 1u : 0u) << 32);
            }
        }
        Scan().exclusive_scan(f, r, 0ull, s_scan);  // (survivor, no-need) ranks inside the block
        __syncthreads();
        const uint32_t sb = s_pre[0], nb = s_pre[1], st = s_pre[2];
#pragma unroll
        for (int j = 0; j < kGrpI; ++j) {
            const int i = b * kGrpB + (int)threadIdx.x * kGrpI + j;
            const bool act = f[j] != 0ull;
            uint32_t id = 0;
            float x = 0.f, y = 0.f, z = 0.f;
            if (act) {
                id = (f[j] & 1ull) ? sb + (uint32_t)r[j] : st + nb + (uint32_t)(r[j] >> 32);
                x = a.xyz[3 * i];
                y = a.xyz[3 * i + 1];
                z = a.xyz[3 * i + 2];
                a.by_id[a.id0 + id] = make_float4(x, y, z, 1.f);
            }
            insert_rank_point(act, id, x, y, z, a.geom, a.addc, a.tmp_cell, a.tmp_rank, a.tlist, a.cnt + kCTouch,
                              a.cnt + kCFlags);
        }
    } else {
        const uint32_t nd = min(a.cnt[kCDirty], a.dcap);
        const uint32_t nw = (gridDim.x - (uint32_t)a.nb_app) * 4u;
        for (uint32_t k = ((uint32_t)b - (uint32_t)a.nb_app) * 4u + (threadIdx.x >> 6); k < nd; k += nw)
            compact_cell_wave(a.pts, a.rng, a.dirty, a.dlist[k]);
    }
}

// add_flag[0 .. n] = 0 (the scan's slot n included)
__global__ void zero_u32_kernel(uint32_t* __restrict__ p, int n1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n1) p[i] = 0u;
}

// Delete_Point_Boxes: alive ids inside any box (min <= x < max) -> tombstones
__global__ void delete_boxes_kernel(float4* __restrict__ by_id, int64_t n, const float* __restrict__ boxes, int nb,
                                    uint32_t* __restrict__ counter) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    uint32_t hit = 0;
    if (i < n) {
        const float4 p = by_id[i];
        if (p.w != 0.f) {
            for (int k = 0; k < nb; ++k) {
                const float* bx = boxes + 6 * k;
                if (bx[0] <= p.x && bx[3] > p.x && bx[1] <= p.y && bx[4] > p.y && bx[2] <= p.z && bx[5] > p.z) {
                    by_id[i].w = 0.f;
                    hit = 1;
                    break;
                }
            }
        }
    }
    const uint32_t m = (uint32_t)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, m);
}

// ---- map_incremental ---------------------------------------------------------

// FAST-LIO map_incremental() classification of one point given its nearest
// points (ascending, nf >= 1 of them).  The reference's list holds
// min(5, map size) points and its re-add loop only runs when it holds 5; list
// entries beyond the ones given here cannot pass the voxel-centre test
// (incr_classify_kernel checks that), so the loop runs over the nf given.
__device__ __forceinline__ uint8_t classify(const IncrArgs& a, float wx, float wy, float wz, const int* nn, int nf) {
    const double fs = a.fs;
    const float mx = (float)(floor((double)wx / fs) * fs + 0.5 * fs);
    const float my = (float)(floor((double)wy / fs) * fs + 0.5 * fs);
    const float mz = (float)(floor((double)wz / fs) * fs + 0.5 * fs);
    const float dist = calc_dist(wx, wy, wz, mx, my, mz);
    const float4 n0 = a.map_by_id[nn[0]];
    if (fabsf(n0.x - mx) > 0.5 * fs && fabsf(n0.y - my) > 0.5 * fs && fabsf(n0.z - mz) > 0.5 * fs) return kNoNeed;
    if (a.map_alive >= 5) {
        for (int j = 0; j < nf; ++j) {
            const float4 q = a.map_by_id[nn[j]];
            if (calc_dist(q.x, q.y, q.z, mx, my, mz) < dist) return kSkip;
        }
    }
    return kToAdd;
}

// Pass 1, lane = point: world point (final pose), classification from the
// bounded kNN lists of the last evaluation.  A bounded list equals the
// reference's unbounded 5-NN when it is full; when it is partial, the missing
// neighbours lie beyond sqrt(range) of the kNN-pose point and cannot beat the
// voxel-centre test unless the pose moved by ~sqrt(range) - 2 * half-diagonal
// (checked); otherwise (and for empty lists) the point is queued for an
// unbounded 5-NN.
__global__ void incr_classify_kernel(IncrArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float bx = a.body[3 * i], by = a.body[3 * i + 1], bz = a.body[3 * i + 2];
    float wx, wy, wz;
    body_to_world(a.pose, bx, by, bz, wx, wy, wz);
    a.world[3 * i] = wx;
    a.world[3 * i + 1] = wy;
    a.world[3 * i + 2] = wz;
    if (a.map_alive == 0) {
        a.cls[i] = kToAdd;
        return;
    }
    int nn[5];
    int nf = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        nn[j] = a.nn_idx[5 * i + j];
        nf += nn[j] >= 0;
    }
    bool exact = nf >= (a.map_alive < 5 ? (int)a.map_alive : 5);
    if (!exact && nf > 0) {
        float kx, ky, kz;
        body_to_world(a.pose_knn, bx, by, bz, kx, ky, kz);
        const float delta = sqrtf(sqdist3(wx, wy, wz, kx, ky, kz));
        const float hd = 0.8660254f * (float)a.fs;  // half diagonal of the voxel
        exact = sqrtf(a.range_sq) - delta - 2.f * hd > 1e-3f;
    }
    if (!exact) {
        a.cls[i] = kSkip;
        a.pending[atomicAdd(a.pending_count, 1)] = i;
        return;
    }
    a.cls[i] = classify(a, wx, wy, wz, nn, nf);
}

// Pass 2: queued points, 8 lanes each: unbounded 5-NN at the kNN-pose point
// (ikd-Tree Nearest_Search with max_dist = INF), then the classification.
__global__ void __launch_bounds__(256) incr_pending_kernel(IncrArgs a) {
    constexpr int G = 8;
    const int sub = threadIdx.x % G;
    const int cnt = *a.pending_count;
    for (int f = blockIdx.x * (256 / G) + threadIdx.x / G; f < cnt; f += gridDim.x * (256 / G)) {
        const int i = a.pending[f];
        float kx, ky, kz;
        body_to_world(a.pose_knn, a.body[3 * i], a.body[3 * i + 1], a.body[3 * i + 2], kx, ky, kz);
        TopK<5> tk;
        tk.init(INFINITY);
        group_knn_exact<5, G>(a.grid, kx, ky, kz, 0x3fffffff, sub, tk);
        if (sub == 0) {
            int nn[5];
            int nf = 0;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                nn[j] = tk.id(j) == kNone ? -1 : tk.id(j);
                nf += nn[j] >= 0;
            }
            a.cls[i] = classify(a, a.world[3 * i], a.world[3 * i + 1], a.world[3 * i + 2], nn, nf);
        }
    }
}

// packed class flags for ONE scan of both compactions: low word PointToAdd, high word no-need
// (slot n = 0: the totals); also clears the survivor flags for this call
__global__ void incr_flags_kernel(const uint8_t* __restrict__ cls, int n, unsigned long long* __restrict__ f,
                                  uint32_t* __restrict__ add_flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const uint8_t c = i < n ? cls[i] : kSkip;
    f[i] = (c == kToAdd ? 1ull : 0ull) | (c == kNoNeed ? (1ull << 32) : 0ull);
    add_flag[i] = 0u;
}

__global__ void incr_scatter_kernel(const float* __restrict__ world, const uint8_t* __restrict__ cls, int n,
                                    const unsigned long long* __restrict__ pos, float* __restrict__ o_add,
                                    float* __restrict__ o_nn, uint32_t* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        cnt[kCAdd] = (uint32_t)pos[n];
        cnt[kCNoNeed] = (uint32_t)(pos[n] >> 32);
        return;
    }
    const uint8_t c = cls[i];
    float* o = c == kToAdd ? o_add + 3 * (size_t)(uint32_t)pos[i]
                           : (c == kNoNeed ? o_nn + 3 * (size_t)(uint32_t)(pos[i] >> 32) : nullptr);
    if (!o) return;
    o[0] = world[3 * i];
    o[1] = world[3 * i + 1];
    o[2] = world[3 * i + 2];
}

// per-point scratch for calls of up to n points (the voxel table at <= 1/4 load).  The table is
// initialised on `st`, the map's (non-blocking) stream: a plain hipMemset runs on the null stream,
// which a non-blocking stream does not wait for.
int ensure_pts(MapUpdBuf& u, int64_t n, hipStream_t st) {
    if (!u.cnt) {
        LIO_HIP(hipMalloc(&u.cnt, kCntWords * sizeof(uint32_t)));
        LIO_HIP(hipMemsetAsync(u.cnt, 0, kCntWords * sizeof(uint32_t), st));  // spread lines: cleared by their reader
        LIO_HIP(hipHostMalloc(&u.h_cnt, 32 * sizeof(uint32_t)));
    }
    if (n <= u.cap && u.world) return 0;
    const size_t c = (size_t)grown<int64_t>(n, u.cap);
    uint32_t hc = 1024;
    int hb = 10;
    while ((int64_t)hc < 4 * (int64_t)c) {
        hc <<= 1;
        ++hb;
    }
    const size_t blk_cap = (c + kGrpB - 1) / kGrpB + 1;
    u.cap = 0;
    // every per-point buffer, once: all allocated, or (kNoMem) all null with cap 0
    const int rc = dev_alloc_all({
        dev_req(u.f64, c + 1), dev_req(u.pos64, c + 1), dev_req(u.add_flag, c + 1), dev_req(u.pos, c + 1),
        dev_req(u.cls, c + 64), dev_req(u.world, c * 3), dev_req(u.xyz_a, c * 3), dev_req(u.xyz_b, c * 3),
        dev_req(u.pending, c), dev_req(u.skey, c), dev_req(u.sval, c), dev_req(u.skey2, c), dev_req(u.sval2, c),
        dev_req(u.xs, c), dev_req(u.vlist, c),
        dev_req(u.dlist, c * 27),  // dirty cells: <= 27 per voxel box at any cell size
        dev_req(u.tmp_cell, c), dev_req(u.tmp_rank, c), dev_req(u.tlist, c), dev_req(u.hkey, hc), dev_req(u.hhead, hc),
        dev_req(u.hend, hc), dev_req(u.vnruns, hc),
        dev_req(u.runs, c),               // a run holds >= 1 point
        dev_req(u.blk, 2 * blk_cap),      // survivors | no-need per sort block
    });
    if (rc) return rc;
    u.blk_cap = blk_cap;
    LIO_HIP(hipMemsetAsync(u.vnruns, 0, (size_t)hc * sizeof(uint32_t), st));
    u.hbits = hb;
    LIO_HIP(hipMemsetAsync(u.hkey, 0xff, (size_t)hc * sizeof(unsigned long long), st));  // empty keys
    LIO_HIP(hipMemsetAsync(u.hhead, 0xff, (size_t)hc * sizeof(int), st));                // empty chains (-1)
    u.hcap = hc;
    u.cap = c;
    return 0;
}

// The downsampled add of the cnt[kCAdd] points xyz[0 ..) (<= n_max) and the append of the
// cnt[kCNoNeed] points xyz_nn, then the grid: tombstoned cells compacted, new ids inserted.  All
// enqueued; cnt[] holds the counts once the stream reaches the end.
// tombstone cell list capacity (cells per update: <= 27 per offered point; tests may shorten it)
uint32_t dcap_of(const MapUpdBuf& u) {
    const int64_t d = u.cap * 27;
    return (uint32_t)(u.dcap_limit > 0 ? std::min<int64_t>(d, u.dcap_limit) : d);
}

int enqueue_add(GridBuf& g, MapUpdBuf& u, const float* xyz, int n_max, const float* xyz_nn, float ds, int64_t id0,
                hipStream_t st) {
    const int nb = (n_max + 255) / 256;
    vox_group_kernel<<<nb, 256, 0, st>>>(xyz, ds, u.hkey, u.hcap - 1, n_max, u.skey, u.sval, u.vlist, u.cnt);
    // (slot, index) stable by slot: every voxel's points contiguous in input order (slot hcap: unused)
    int rc = cub_sort_pairs(u.tmp, u.tmp_bytes, kGrowScratch, u.skey, u.skey2, u.sval, u.sval2, n_max, u.hbits + 1, st);
    if (rc) return rc;
    vox_runs_kernel<<<nb, 256, 0, st>>>(u.skey2, u.sval2, xyz, n_max, u.hcap - 1, u.hhead, u.hend, u.xs);
    VoxArgs va{u.vlist, u.hkey, u.hhead, u.hend, nullptr, nullptr, u.sval2, u.xs, xyz, ds, grid_view(g), (int)g.n,
               g.pts, g.by_id, g.dirty, u.dlist, dcap_of(u), u.cnt, u.add_flag};
    vox_resolve_kernel<false><<<std::min(2048, (n_max + 3) / 4), 256, 0, st>>>(va);
    rc = cub_exclusive_sum(u.tmp, u.tmp_bytes, kGrowScratch, static_cast<const uint32_t*>(u.add_flag), u.pos, n_max + 1, st);
    if (rc) return rc;
    append_kernel<<<nb, 256, 0, st>>>(xyz, u.add_flag, u.pos, xyz_nn, n_max, id0, g.by_id, u.cnt);
    grid_compact_cells(g, u.dlist, u.cnt + kCDirty, dcap_of(u), n_max * 27, st);
    GridInsertScratch sc{u.tmp_cell, u.tmp_rank, u.tlist, u.cnt + kCTouch};
    grid_insert_ids(g, id0, u.cnt + kCNew, n_max, sc, u.cnt + kCFlags, st);
    LIO_HIP(hipGetLastError());
    return 0;
}

// The grouped update of n points xyz (class per point: cls, or all_cls for all): PointToAdd points
// through the downsampled add, then the no-need points appended — group_sort, vox_resolve<true>, one
// scan, the fused append / rank / compaction kernel, the block growth.  Counters zeroed by the caller.
int enqueue_grouped(GridBuf& g, MapUpdBuf& u, const float* xyz, const uint8_t* cls, int all_cls, int n, float ds,
                    int64_t id0, hipStream_t st) {
    GroupArgs ga{xyz,      cls,    all_cls, n,    ds,   u.hkey,     u.hcap - 1, u.hbits, u.hhead,
                 u.vnruns, u.runs, u.sval2, u.xs, u.vlist, u.add_flag, u.cnt,      u.blk,   u.blk + u.blk_cap};
    const int nblk = (n + kGrpB - 1) / kGrpB;
    group_sort_kernel<<<nblk, kGrpT, 0, st>>>(ga);
    const uint32_t dcap = dcap_of(u);
    VoxArgs va{u.vlist, u.hkey,   u.hhead, nullptr,    u.vnruns, u.runs, u.sval2, u.xs,   xyz,       ds,  grid_view(g),
               (int)g.n, g.pts,   g.by_id, g.dirty,    u.dlist,  dcap,   u.cnt,   u.add_flag, u.blk};
    vox_resolve_kernel<true><<<std::min(2048, (n + 3) / 4), 256, 0, st>>>(va);
    const int nb_comp = std::min(512, std::max(8, nblk * 8));
    UpdArgs ua{xyz,    cls,        all_cls,    n,      u.add_flag, u.blk, u.blk + u.blk_cap, id0,   g.by_id, g.geom, g.addc,
               u.tmp_cell, u.tmp_rank, u.tlist, u.cnt,  g.pts,      g.rng, g.dirty,            u.dlist, dcap,    nblk};
    update_kernel<<<nblk + nb_comp, kGrpT, 0, st>>>(ua);
    GridInsertScratch sc{u.tmp_cell, u.tmp_rank, u.tlist, u.cnt + kCTouch};
    grid_insert_finish(g, id0, u.cnt + kCNew, n, sc, u.cnt + kCFlags, st);
    LIO_HIP(hipGetLastError());
    return 0;
}

constexpr int kRedo = 1;  // finish_add: the grouped update was abandoned (kFlagRuns), nothing changed

// the one host synchronisation of an update: counts back, the map's host view updated; a point
// outside the grid or an exhausted slot pool -> full rebuild (by_id is complete either way)
int finish_add(GridBuf& g, MapUpdBuf& u, int64_t id0, float slack, hipStream_t st) {
    LIO_HIP(hipMemcpyAsync(u.h_cnt, u.cnt, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    const uint32_t* c = u.h_cnt;
    if (c[kCFlags] & kFlagRuns) return kRedo;
    g.n_ids = id0 + c[kCNew];
    g.n = g.n - (int64_t)c[kCDead] + (int64_t)c[kCNew];
    if (c[kCFlags]) return grid_rebuild(g, g.geom.cell, slack, st);
    return 0;
}

}  // namespace

void mapupd_free(MapUpdBuf& u) {
    dev_free(&u.f64, &u.pos64, &u.add_flag, &u.pos, &u.cls, &u.world, &u.xyz_a, &u.xyz_b, &u.pending, &u.skey, &u.sval,
             &u.skey2, &u.sval2, &u.xs, &u.vlist, &u.dlist, &u.tmp_cell, &u.tmp_rank, &u.tlist, &u.hkey, &u.hhead, &u.hend,
             &u.tmp, &u.cnt, &u.boxes, &u.vnruns, &u.runs, &u.blk);
    host_free(&u.h_cnt);
    u = MapUpdBuf{};
}

// Add_Points(xyz[0..n), downsample) for device points; out: [triggers / added, tombstones]
int map_add_device(GridBuf& g, MapUpdBuf& u, const float* d_xyz, int64_t n64, bool downsample, float ds,
                   float slack, int64_t out[2], hipStream_t st) {
    out[0] = out[1] = 0;
    if (n64 <= 0) return 0;
    if (n64 >= (int64_t)1 << 30) return kArg;
    const int n = (int)n64;
    if (const int rc = ensure_pts(u, n, st)) return rc;
    const int64_t id0 = g.n_ids;
    int rc = grid_reserve_ids(g, id0 + n, st);
    if (rc) return rc;
    LIO_HIP(hipMemsetAsync(u.cnt, 0, 16 * sizeof(uint32_t), st));
    rc = enqueue_grouped(g, u, d_xyz, nullptr, downsample ? kToAdd : kNoNeed, n, ds, id0, st);
    if (rc) return rc;
    rc = finish_add(g, u, id0, slack, st);
    if (rc != kRedo) {
        out[0] = downsample ? (int64_t)u.h_cnt[kCTrig] : n;
        out[1] = u.h_cnt[kCDead];
        return rc;
    }
    // a voxel spread over more than kMaxRuns sort blocks: the globally sorted path
    LIO_HIP(hipMemsetAsync(u.cnt, 0, 16 * sizeof(uint32_t), st));
    zero_u32_kernel<<<(n + 1 + 255) / 256, 256, 0, st>>>(u.add_flag, n + 1);
    if (downsample) {
        set_u32_kernel<<<1, 1, 0, st>>>(u.cnt + kCAdd, (uint32_t)n);
        rc = enqueue_add(g, u, d_xyz, n, nullptr, ds, id0, st);
    } else {  // every point appended (as the no-need points of map_incremental)
        set_u32_kernel<<<1, 1, 0, st>>>(u.cnt + kCNoNeed, (uint32_t)n);
        rc = enqueue_add(g, u, nullptr, n, d_xyz, ds, id0, st);
    }
    if (rc) return rc;
    rc = finish_add(g, u, id0, slack, st);
    out[0] = downsample ? (int64_t)u.h_cnt[kCTrig] : n;
    out[1] = u.h_cnt[kCDead];
    return rc;
}

int map_delete_boxes(GridBuf& g, MapUpdBuf& u, const float* boxes, int nb, float slack, int64_t* n_deleted,
                     hipStream_t st) {
    *n_deleted = 0;
    if (nb <= 0 || g.n_ids == 0) return 0;
    if (const int rc = ensure_pts(u, 1, st)) return rc;
    if (!u.boxes || nb > u.boxes_cap) {
        u.boxes_cap = 0;
        if (dev_alloc_all({dev_req(u.boxes, (size_t)nb * 6)})) return kNoMem;
        u.boxes_cap = nb;
    }
    LIO_HIP(hipMemcpyAsync(u.boxes, boxes, (size_t)nb * 6 * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP(hipMemsetAsync(u.cnt, 0, 16 * sizeof(uint32_t), st));
    delete_boxes_kernel<<<(int)((g.n_ids + 255) / 256), 256, 0, st>>>(g.by_id, g.n_ids, u.boxes, nb, u.cnt + kCDead);
    LIO_HIP(hipMemcpyAsync(u.h_cnt, u.cnt, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP(hipStreamSynchronize(st));
    *n_deleted = u.h_cnt[kCDead];
    if (*n_deleted == 0) return 0;
    return grid_rebuild(g, g.geom.cell, slack, st);  // bulk deletes (the local map moved): re-lay once
}

// map_incremental(): classification (+ unbounded 5-NN for queued points), then
// Add_Points(PointToAdd, true) and Add_Points(PointNoNeedDownsample, false) with one grid update and
// one host synchronisation.  out: [to_add, no_need, skipped, added_by_downsample_call]
// The update scratch sized for n offered points before the first update (lio_map_build): the first
// map_incremental of a stream then allocates nothing (~8 ms of set-up on the first call)
// an empty launch from this file: with HIP's deferred code-object loading the first launch from a code
// object loads it (8-12 ms measured on the first map_incremental, 0.19 ms with HIP_ENABLE_DEFERRED_LOADING=0:
// scripts/map_first_call.py), so lio_map_build pays it instead of the first update
__global__ void mapupd_warm_kernel(uint32_t* __restrict__ p) {
    if (p && threadIdx.x == 1024) p[0] = 0u;  // never true: keeps the kernel non-empty for the compiler
}

int mapupd_presize(MapUpdBuf& u, int64_t n, hipStream_t st) {
    if (n <= 0) return 0;
    mapupd_warm_kernel<<<1, 64, 0, st>>>(nullptr);
    LIO_HIP(hipGetLastError());
    if (n >= (int64_t)1 << 30) return kArg;
    if (const int rc = ensure_pts(u, n, st)) return rc;
    size_t b1 = 0, b2 = 0, b3 = 0;
    LIO_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b1, u.add_flag, u.pos, (int)n + 1, st));
    LIO_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, u.f64, u.pos64, (int)n + 1, st));
    LIO_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b3, u.skey, u.skey2, u.sval, u.sval2, (int)n, 0, u.hbits + 1, st));
    return grow_scratch(&u.tmp, u.tmp_bytes, std::max(b1, std::max(b2, b3)));
}

int map_incremental(GridBuf& g, MapUpdBuf& u, IncrArgs a, float ds, float slack, int64_t out[4], hipStream_t st) {
    for (int k = 0; k < 4; ++k) out[k] = 0;
    const int n = a.n;
    if (n <= 0) return 0;
    if (const int rc = ensure_pts(u, n, st)) return rc;
    const int64_t id0 = g.n_ids;
    int rc = grid_reserve_ids(g, id0 + n, st);
    if (rc) return rc;
    a.grid = grid_view(g);
    a.map_by_id = g.by_id;
    a.map_alive = g.n;
    a.world = u.world;
    a.cls = u.cls;
    a.pending = u.pending;
    a.pending_count = reinterpret_cast<int*>(u.cnt + kCPend);
    LIO_HIP(hipMemsetAsync(u.cnt, 0, 16 * sizeof(uint32_t), st));
    const int nb = (n + 255) / 256;
    incr_classify_kernel<<<nb, 256, 0, st>>>(a);
    incr_pending_kernel<<<128, 256, 0, st>>>(a);
    // the classes are final: PointToAdd / PointNoNeedDownsample straight from the per-point classes
    rc = enqueue_grouped(g, u, u.world, u.cls, 0, n, ds, id0, st);
    if (rc) return rc;
    rc = finish_add(g, u, id0, slack, st);
    uint32_t n_add = u.h_cnt[kCAdd];
    if (rc == kRedo) {  // a voxel spread over more than kMaxRuns sort blocks: compact, then the sorted path
        LIO_HIP(hipMemsetAsync(u.cnt, 0, 16 * sizeof(uint32_t), st));
        incr_flags_kernel<<<(n + 1 + 255) / 256, 256, 0, st>>>(u.cls, n, u.f64, u.add_flag);
        rc = cub_exclusive_sum(u.tmp, u.tmp_bytes, kGrowScratch, static_cast<const unsigned long long*>(u.f64), u.pos64,
                               n + 1, st);
        if (rc) return rc;
        incr_scatter_kernel<<<(n + 1 + 255) / 256, 256, 0, st>>>(u.world, u.cls, n, u.pos64, u.xyz_a, u.xyz_b, u.cnt);
        rc = enqueue_add(g, u, u.xyz_a, n, u.xyz_b, ds, id0, st);
        if (rc) return rc;
        rc = finish_add(g, u, id0, slack, st);
        n_add = u.h_cnt[kCAdd];
    }
    const uint32_t* c = u.h_cnt;
    (void)n_add;
    out[0] = c[kCAdd];
    out[1] = c[kCNoNeed];
    out[2] = n - (int64_t)c[kCAdd] - (int64_t)c[kCNoNeed];
    out[3] = c[kCTrig];
    return rc;
}

namespace {
__global__ void gather_ids_kernel(const float4* __restrict__ by_id, int64_t n_ids, const int32_t* __restrict__ ids,
                                  int64_t n, float* __restrict__ xyz) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t id = ids[i];
    float4 p = make_float4(NAN, NAN, NAN, 0.f);
    if (id >= 0 && id < n_ids) p = by_id[id];
    xyz[3 * i] = p.x;
    xyz[3 * i + 1] = p.y;
    xyz[3 * i + 2] = p.z;
}
}  // namespace

void map_gather_ids(const GridBuf& g, const int32_t* d_ids, int64_t n, float* d_xyz, hipStream_t st) {
    if (n <= 0) return;
    gather_ids_kernel<<<(int)((n + 255) / 256), 256, 0, st>>>(g.by_id, g.n_ids, d_ids, n, d_xyz);
}

}  // namespace lio
