// lio_icp_hooks.cpp — the loop ICP's test hooks and host mirrors: entry points of include/lio_gpu.h that no
// alignment calls (the seqsum path on its own, the sharded chains' exchange logic on the host, the records' sum,
// the float Umeyama, the shard ranges, the allocation counter).
#include "lio_icp_handle.hpp"
#include "lio_icp_math.hpp"

using namespace lio::icp;

extern "C" int64_t lio_alloc_count(void) { return lio::alloc_counter().load(std::memory_order_relaxed); }

extern "C" int lio_icp_shard_range(int64_t ns, int rank, int world, int64_t* begin, int64_t* count) {
    if (ns < 0 || world < 1 || rank < 0 || rank >= world || !begin || !count)
        return fail(LIO_ERR_ARG, "lio_icp_shard_range: bad arguments");
    shard_range(ns, rank, world, *begin, *count);
    return LIO_OK;
}

extern "C" int lio_icp_umeyama_pcl_float(const float* sums16, float* T16) {
    if (!sums16 || !T16) return fail(LIO_ERR_ARG, "lio_icp_umeyama_pcl_float: bad arguments");
    umeyama_pcl_float(sums16, T16);
    return LIO_OK;
}

extern "C" int lio_icp_umeyama_pcl_float_order(const float* sums16, int order, float* T16) {
    if (!sums16 || !T16 || order < 1 || order > 3) return fail(LIO_ERR_ARG, "lio_icp_umeyama_pcl_float_order: bad arguments");
    umeyama_pcl_float(sums16, T16, order);
    return LIO_OK;
}

// test hook: the seqsum path on 6 interleaved chains, re-passes as in pcl_finish; -1 passes: serial needed
extern "C" int lio_seqsum6(int device, const float* x, int64_t n, int flags, float* sums6, int* passes_out) {
    if (!x || n < 1 || !sums6 || n >= ((int64_t)1 << 31)) return fail(LIO_ERR_ARG, "lio_seqsum6: bad arguments");
    int rc = lio::capi::check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    lio::SeqSumBuf b;
    b.dbg_noinc = flags & 1;
    float* d_x = nullptr;
    uint32_t* d_n = nullptr;
    uint32_t stat[2] = {0, 0};
    int passes = 0;
    const uint32_t n32 = (uint32_t)n;
    auto done = [&](int code, const char* msg) {
        lio::seqsum_free(b);
        lio::dev_free(&d_x, &d_n);
        (void)hipStreamDestroy(st);
        return code ? fail(code, msg) : LIO_OK;
    };
    if (lio::seqsum_reserve(b, 6, n, st) || hipMalloc(&d_x, (size_t)n * 6 * sizeof(float)) != hipSuccess ||
        hipMalloc(&d_n, sizeof(uint32_t)) != hipSuccess)
        return done(LIO_ERR_NOMEM, "lio_seqsum6: allocation");
    if (flags & 2) b.evcap = std::min<int64_t>(4, b.evcap_alloc);  // overflow: the caller's serial fallback
    if (hipMemcpyAsync(d_x, x, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_n, &n32, sizeof(n32), hipMemcpyHostToDevice, st) != hipSuccess)
        return done(LIO_ERR_HIP, "lio_seqsum6: upload");
    for (int pass = 1; pass <= 3; ++pass) {
        lio::seqsum_launch(lio::SeqPairs{d_x}, 6, d_n, b, pass, st);
        if (hipMemcpyAsync(stat, b.status, sizeof(stat), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(sums6, b.result, 6 * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return done(LIO_ERR_HIP, "lio_seqsum6: kernels");
        passes = pass;
        if ((stat[0] | stat[1]) == 0 || stat[1]) break;
    }
    if (passes_out) *passes_out = (stat[0] | stat[1]) ? -1 : passes;
    return done(LIO_OK, "");
}

// host mirrors of the sharded float chains' exchange logic (the device kernels run the same seq_shard_* helpers,
// lio_seqsum.hpp): the gathered totals -> one window's offsets; the gathered event messages -> one chain's global
// event lists.  tests/test_dist_gloo.py drives them with messages all-gathered over gloo.
extern "C" int lio_seq_shard_offsets(const double* recv, int64_t stride, int64_t nb_slot, int rank, int world, int nch,
                                     double* off0, double* var0, int32_t* floor_e, int64_t* gbase_nglobal) {
    if (!recv || !off0 || !var0 || !floor_e || !gbase_nglobal || world < 1 || rank < 0 || rank >= world || nch < 1 ||
        nch > lio::kSeqMaxChains || nb_slot < 1 || stride < lio::seq_tot_words(nch, nb_slot))
        return fail(LIO_ERR_ARG, "lio_seq_shard_offsets: bad arguments");
    for (int c = 0; c < nch; ++c) {
        int fl;
        lio::seq_shard_offsets_chain(recv, stride, nb_slot, rank, world, c, off0[c], var0[c], fl, gbase_nglobal[0],
                                     gbase_nglobal[1]);
        floor_e[c] = fl;
    }
    return LIO_OK;
}

extern "C" int lio_seq_shard_merge(const double* recv, int64_t stride, int world, int slot, int chain, int64_t evs,
                                   int32_t* pos, uint64_t* P, float* x, int32_t* nev_ptot_bad, uint64_t* ptot, float* x0) {
    if (!recv || !pos || !P || !x || !nev_ptot_bad || !ptot || !x0 || world < 1 || world > 64 || slot < 0 || chain < 0 ||
        chain >= lio::kSeqMaxChains || stride < lio::seqsum_msg_words(chain + 1, slot))
        return fail(LIO_ERR_ARG, "lio_seq_shard_merge: bad arguments");
    int eoff[65];
    uint64_t poff[65];
    int64_t ppos[65];
    int mx = 0;
    const int bad = lio::seq_shard_merge_chain(recv, stride, world, slot, chain, evs, eoff, poff, ppos, *x0, mx);
    nev_ptot_bad[0] = eoff[world];
    nev_ptot_bad[1] = mx;
    nev_ptot_bad[2] = bad;
    *ptot = poff[world];
    if (bad) return LIO_OK;
    for (int r = 0; r < world; ++r) {  // seq_shard_merge's copy: every rank's events moved by the ranks before it
        const double* ev = recv + (int64_t)r * stride + lio::kSeqHdrWords + (int64_t)chain * 2 * slot;
        for (int j = 0; j < eoff[r + 1] - eoff[r]; ++j) {
            const uint64_t w = (uint64_t)lio::seq_bits(ev[2 * j + 1]);
            P[eoff[r] + j] = poff[r] + (uint64_t)lio::seq_bits(ev[2 * j]);
            pos[eoff[r] + j] = (int32_t)(ppos[r] + (int64_t)(uint32_t)w);
            uint32_t xb = (uint32_t)(w >> 32);
            std::memcpy(&x[eoff[r] + j], &xb, sizeof(float));
        }
    }
    return LIO_OK;
}

extern "C" int lio_icp_combine(const double* recv, int64_t ns, int world, double* out17) {
    if (!recv || !out17 || world < 1 || ns < 0) return fail(LIO_ERR_ARG, "lio_icp_combine: bad arguments");
    combine_records(recv, ns, world, records_count(ns, world), out17);
    return LIO_OK;
}

