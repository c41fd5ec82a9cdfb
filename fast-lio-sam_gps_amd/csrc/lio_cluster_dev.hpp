// lio_cluster_dev.hpp — the device code lio_cluster.hip (Euclidean clusters) and lio_dbscan.hip (DBSCAN) share:
// the lock-free union-find over input indices, whose root is the lowest index of its tree, and the kernels of
// the tail that turns sorted (key, index) pairs into runs and offsets.  Included by
// those two files only; every kernel here is internal to the file that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lio {

namespace {

constexpr uint32_t kNoRun = 0xffffffffu;

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

}  // namespace

}  // namespace lio
