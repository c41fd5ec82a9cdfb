// lio_icp_handle.hpp — the loop-ICP handle (C-ABI lio_icp_*) and what its files share.  Private, like
// lio_capi_util.hpp.  The files, by concern:
//   lio_icp_setup.cpp     create / destroy, the shard, the target's and the source's set-up
//   lio_icp_host.cpp      the correspondence pass, lio_icp_align, the getters
//   lio_icp_exchange.cpp  the ranks' message sizes, the exchange buffers, the one all-gather
//   lio_icp_stats.cpp     the PCL float statistics of a pass: one rank and sharded, re-passes, serial fallback
//   lio_icp_math.cpp      Umeyama (double and PCL float), the convergence criteria            (lio_icp_math.hpp)
//   lio_icp_policy.hpp    the re-pass policy, the event slot, the polled mailbox              (no HIP)
//   lio_icp_hooks.cpp     test hooks and host mirrors (lio_seqsum6, lio_seq_shard_*, lio_icp_combine, ...)
#pragma once
#include "lio_capi_base.hpp"

#include <algorithm>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "lio_icp_policy.hpp"
#include "lio_kernels.hpp"
#include "lio_pcl.hpp"
#include "lio_scratch.hpp"

struct EvPair {
    hipEvent_t a = nullptr, b = nullptr;
    hipEvent_t m = nullptr;     // between the correspondence and statistics kernels
    hipEvent_t done = nullptr;  // a pass's statistics have reached the host
};

struct lio_icp {
    int dev = 0;
    hipStream_t st = nullptr;
    lio_icp_params p{};
    lio::GridBuf tgt;
    float* d_tgt = nullptr;
    int64_t tgt_cap = 0;
    int64_t nt = 0;
    bool tgt_dirty = false;      // setInputTarget staged; uploaded and gridded at the next align (as PCL builds
                                 // its kd-tree lazily in align), on st2, overlapped with the source preparation
    hipStream_t st2 = nullptr;
    float* h_tgt = nullptr;      // pinned staging: the target, the full source
    int64_t h_tgt_cap = 0;
    float* h_src = nullptr;
    int64_t h_src_cap = 0;
    double c0[3] = {0, 0, 0};
    int64_t ns = 0;
    int rank = 0, world = 1;
    lio_allgather_fn fn = nullptr;
    void* user = nullptr;
    lio_allgather_dev_fn fn_dev = nullptr;  // device-side exchange (lio_icp_set_shard_device)
    void* user_dev = nullptr;
    double* d_xsend = nullptr;  // exchange buffers: this rank's records / all ranks' (device)
    double* d_xrecv = nullptr;
    int64_t x_len = 0;          // doubles per rank they hold
    bool x_ext = false;         // caller-owned (lio_icp_set_exchange_buffers)
    double* h_out17 = nullptr;  // host-mapped record-order sums (device exchange)
    double* h_out17_dev = nullptr;
    // shard buffers
    int64_t sh_begin = 0, sh_n = 0, cap = 0;
    float* d_src = nullptr;
    float* d_cur = nullptr;
    float* d_thist = nullptr;  // transforms applied this alignment (the correspondence kernel's history)
    int thist_cap = 0, nT = 0;
    float* d_fd2 = nullptr;
    int* d_fid = nullptr;
    lio::GridBuf qgrid;      // the shard's source binned by tile cell (icp_build_tiles)
    uint2* d_tiles = nullptr;
    uint32_t* d_tscratch = nullptr;
    void* d_ttmp = nullptr;
    size_t ttmp_bytes = 0;
    int64_t tscratch_cap = 0;
    int ntiles = 0;
    float tile_cell = 2.0f;
    bool have_prior = false;  // nn ids of this alignment's previous pass are in d_fid
    uint32_t* d_tcost = nullptr;  // per tile: candidates of the last pass
    uint32_t* d_order = nullptr;  // longest-first tile order (valid when have_order)
    bool have_order = false;
    unsigned long long* d_dbg = nullptr;  // search counters (diagnostics build: LIO_DIAG + LIO_ICP_DEBUG)
    size_t dbg_bytes = 0;
    double* h_super = nullptr;      // pinned, host-mapped: the pass's 4096-point records
    double* h_super_dev = nullptr;  // device view of h_super (the statistics kernel writes it, zero-copy)
    int64_t super_cap = 0;
    std::vector<double> rec_send, rec_recv;  // the records-only host exchange's messages (the double statistics)
    bool src_dirty = true;
    float* d_pcl16 = nullptr;  // umeyama_float: the serial float sums (launch_icp_pcl_stats: the fallback)
    lio::PclBuf pcl;           // umeyama_float: compacted pairs + seqsum chains
    float* d_pclout = nullptr; // pcl_pack output (kPclOutWords)
    float* h_pclout = nullptr; // pinned, host-mapped: a copy, or the pack's own stores (one rank: box polls [23])
    float* h_pclout_dev = nullptr;
    lio::icp::Mailbox box;     // h_pclout[23] and the sequence numbers handed to the pack
    void* x_owner = nullptr;   // exchange state owned by the handle (lio_icp_mp.cpp: shm segment, RCCL comm)
    void (*x_owner_free)(void*) = nullptr;
    // sharded PCL float modes (fid_sharded): only this rank's shard on the device; the float chains split by
    // window (lio_seqsum.hpp), the per-rank event-list slot of the exchange (grown from what the last pass
    // needed, the same on every rank), pinned staging for a host exchange, the serial fallback's gathered pairs
    int ev_slot = 2048, ev_slot_s = 2048;
    double* h_xs = nullptr;
    double* h_xr = nullptr;
    int64_t hx_cap = 0;
    lio::PclBuf pg;
    int64_t fid_stats[4] = {0, 0, 0, 0};  // re-passes, serial fallbacks, events of the last pass, passes
    float last_pcl16[16] = {};            // the last correspondence pass's float statistics (lio_icp_get_umeyama_stats)
    bool have_pcl16 = false;
    int fid_flags = 0;
    int64_t fid_evcap = 0;
    bool timing = false;
    lio_kernel_timing tm{};
    EvPair ev;
    // set-up started by lio_icp_set_target / _set_source that runs on behind the caller (the target's upload
    // and grid on st2, the source's upload and binning on st): every other entry point joins them first; a
    // failure leaves the dirty flag set, so lio_icp_align repeats the step and reports it
    std::thread bg_tgt, bg_src;
    std::string bg_tgt_err, bg_src_err;  // why a background set-up failed (reported if align's retry fails too)
};

namespace lio::icp {

using lio::capi::fail;

// the two set-ups touch disjoint state (target: st2, d_tgt, tgt grid, c0; source: st, the shard buffers),
// so a new target only waits for the previous target's thread and a new source for the previous source's
inline void icp_join_tgt(lio_icp* h) {
    if (h->bg_tgt.joinable()) h->bg_tgt.join();
}
inline void icp_join_src(lio_icp* h) {
    if (h->bg_src.joinable()) h->bg_src.join();
}
inline void icp_join(lio_icp* h) {
    icp_join_src(h);
    icp_join_tgt(h);
}

// `job` on thread t, behind the caller; where no thread can be had, here and now
template <class Job>
void run_behind(std::thread& t, Job job) {
    try {
        t = std::thread(job);
    } catch (...) {
        job();
    }
}

// the PCL float modes with more than one rank: the float chains run split over the ranks' windows
inline bool fid_sharded(const lio_icp* h) { return h->p.umeyama_float > 0 && h->world > 1; }

// Capacities grow geometrically from a floor sized for the reference's largest submaps (C4: 500 k points): a
// loop-closure node whose submaps change size on every 2 Hz loopTimerFunc call (fast_lio_sam.cpp:682-730) then
// allocates on its first call and (almost) never again — a hipFree synchronises the device, and a re-allocation
// per call showed up as a 9 ms cold loop leg against 1.1 ms warm.
constexpr int64_t kIcpCapFloor = (int64_t)1 << 19;
inline int64_t icp_cap(int64_t need, int64_t cap) { return std::max(std::max(need + need / 2, 2 * cap), kIcpCapFloor); }

// dev_alloc_all (all or nothing, one lio_alloc_count per buffer) with the C-ABI's code and message
inline int alloc_all(std::initializer_list<lio::DevReq> reqs, const char* what) {
    if (lio::dev_alloc_all(reqs) != lio::kOk) return fail(LIO_ERR_NOMEM, std::string(what) + ": hipMalloc failed");
    return LIO_OK;
}

// a pinned block the device writes and the host reads without a copy: *host and its device view *dev
template <class T>
int mapped_alloc(T** host, T** dev, size_t bytes) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(host), bytes, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(dev), *host, 0));
    return LIO_OK;
}

// ---- lio_icp_exchange.cpp
void shard_range(int64_t ns, int rank, int world, int64_t& b, int64_t& n);
int64_t shard_points_max(int64_t ns, int world);
int64_t ev_slot_cap(int64_t ns, int world);
int64_t records_count(int64_t ns, int world);
int64_t tot_blocks(int64_t ns, int world);
int64_t tot_words(int64_t ns, int world, int nch);
int64_t exchange_len(int64_t ns, int world);
void combine_records(const double* recv, int64_t ns, int world, int64_t stride, double out17[17]);
int exchange_reserve(lio_icp* h);
// `cnt` doubles per rank all-gathered (rank r's at r * cnt of the result) in the handle's stream order.  A device
// callback is enqueued from d_xsend into d_xrecv.  A host callback gathers h_send into h_recv; with none given,
// d_xsend goes through the pinned staging and the result back into d_xrecv (one wait).
int allgather(lio_icp* h, int64_t cnt, const double* h_send = nullptr, double* h_recv = nullptr);

// ---- lio_icp_stats.cpp
// one rank: the float statistics of the pass's compacted pairs enqueued, the pack last; *seq is what
// pcl_wait waits for
int enqueue_pcl(lio_icp* h, uint32_t* seq);
int pcl_wait(lio_icp* h, uint32_t seq);
// h_pclout holds a pass's first output: re-passes, re-exchanges and the serial fallback until it is final
int pcl_finish(lio_icp* h, const lio::IcpArgs& a);
// one correspondence pass of the sharded PCL float modes (a: this rank's shard, as icp_pass built it)
int icp_pass_fsh(lio_icp* h, const lio::IcpArgs& a, bool apply_T, double out17[17], float* pcl16);

// ---- lio_icp_setup.cpp
// the staged target: upload + grid + accumulation centre, on st2 (called from a helper thread)
int target_build(lio_icp* h);
// this rank's shard of the staged source: its buffers, upload and tiles, on st
int icp_prepare(lio_icp* h);

// ---- lio_icp_host.cpp
// the pass's event-timed kernels (ev.a .. ev.m .. ev.b) added to the handle's timing
void add_pass_timing(lio_icp* h);

}  // namespace lio::icp
