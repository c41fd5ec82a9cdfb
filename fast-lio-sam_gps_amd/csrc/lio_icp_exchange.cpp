// lio_icp_exchange.cpp — the loop ICP over several ranks: what one rank sends per pass, the buffers that hold
// it, and the one all-gather every exchange of lio_icp_host.cpp and lio_icp_stats.cpp goes through.
#include "lio_icp_handle.hpp"

namespace lio::icp {

void shard_range(int64_t ns, int rank, int world, int64_t& b, int64_t& n) {
    const int64_t nsup = (ns + lio::kIcpSuper - 1) / lio::kIcpSuper;
    const int64_t s0 = nsup * rank / world, s1 = nsup * (rank + 1) / world;
    b = std::min<int64_t>(s0 * lio::kIcpSuper, ns);
    n = std::min<int64_t>(s1 * lio::kIcpSuper, ns) - b;
}

// Exchange messages of one rank, in doubles (all-gathered, rank r's at r * count of the receive buffer):
//   records   every pass: its 4096-point records (slot = ceil(records / world) of kIcpStride); in the sharded
//             PCL float modes followed by its windows' chain totals (lio_seqsum.hpp, kTotPad)
//   events    sharded PCL float modes: the seqsum event message of its window (ev_slot events per chain),
//             for the means with its first kPclMaxKc pairs (SeqHeads, lio_seqsum.hpp)
//   blocks    sharded orders 2 / 3: its depth blocks of sigma and the verification statuses
//   gather    the sharded serial fallback: its pairs in rounds
// exchange_len is the capacity of every one of them (the event slot up to ev_slot_cap).
static int64_t exchange_slot(int64_t ns, int world) {
    const int64_t nsup = (ns + lio::kIcpSuper - 1) / lio::kIcpSuper;
    return (nsup + world - 1) / world;
}
int64_t shard_points_max(int64_t ns, int world) { return exchange_slot(ns, world) * lio::kIcpSuper; }
int64_t ev_slot_cap(int64_t ns, int world) { return std::max<int64_t>(4096, shard_points_max(ns, world) / 8); }
int64_t records_count(int64_t ns, int world) { return exchange_slot(ns, world) * lio::kIcpStride; }
// blocks of a window in the block-sum message (seq_bsum's tot_out)
int64_t tot_blocks(int64_t ns, int world) { return (shard_points_max(ns, world) + lio::kSeqBlock - 1) / lio::kSeqBlock + 1; }
int64_t tot_words(int64_t ns, int world, int nch) { return lio::seq_tot_words(nch, tot_blocks(ns, world)); }
int64_t exchange_len(int64_t ns, int world) {
    const int64_t rec = records_count(ns, world) + tot_words(ns, world, lio::kSeqMaxChains);
    const int64_t ev = lio::seqsum_msg_words(lio::kSeqMaxChains, (int)ev_slot_cap(ns, world)) + lio::pcl_heads_words();  // >= 6 chains' heads
    const int64_t x3 = lio::pcl_x3_words(lio::pcl_blocks_slot(shard_points_max(ns, world)));
    return std::max(std::max(rec, ev), std::max(x3, (int64_t)4096));
}

// the records of every rank (rank r at recv + r * stride doubles) summed in global record order
void combine_records(const double* recv, int64_t ns, int world, int64_t stride, double out17[17]) {
    const int64_t nsup = (ns + lio::kIcpSuper - 1) / lio::kIcpSuper;
    for (int k = 0; k < 17; ++k) out17[k] = 0.0;
    for (int r = 0; r < world; ++r) {
        const int64_t s0 = nsup * r / world, s1 = nsup * (r + 1) / world;
        for (int64_t s = s0; s < s1; ++s) {
            const double* rec = &recv[(size_t)r * (size_t)stride + (size_t)(s - s0) * lio::kIcpStride];
            for (int k = 0; k < 17; ++k) out17[k] += rec[k];
        }
    }
}

// device exchange buffers for the current source (the handle's own unless the caller's are large enough): the
// sharded PCL float modes need exchange_len, the double statistics only the records
int exchange_reserve(lio_icp* h) {
    const int64_t need = std::max<int64_t>(fid_sharded(h) ? exchange_len(h->ns, h->world) : records_count(h->ns, h->world),
                                           lio::kIcpStride);
    if (!h->h_out17)  // the record-order sums land here whoever owns the exchange buffers
        if (const int rc = mapped_alloc(&h->h_out17, &h->h_out17_dev, 32 * sizeof(double))) return rc;
    if (!h->h_out17_dev) return fail(LIO_ERR_STATE, "lio_icp_align: no device view of the result block");
    if (h->x_ext) {
        if (h->x_len < need)
            return fail(LIO_ERR_ARG, "lio_icp_align: caller exchange buffers too small (lio_icp_exchange_len: " +
                                         std::to_string(need) + " doubles per rank)");
        return LIO_OK;
    }
    if (h->x_len < need || !h->d_xsend || !h->d_xrecv) {
        const int64_t c = std::max(need + need / 2, 2 * h->x_len);
        h->x_len = 0;
        if (const int rc = alloc_all({lio::dev_req(h->d_xsend, (size_t)c), lio::dev_req(h->d_xrecv, (size_t)c * h->world)},
                                     "lio_icp_align: exchange buffers"))
            return rc;
        h->x_len = c;
    }
    return LIO_OK;
}

// the callback itself; what it left in last_error() (the library's own exchanges do: lio_icp_mp.cpp) survives
static int call_allgather(lio_icp* h, const double* send, int64_t cnt, double* recv) {
    lio::last_error().clear();
    const int rc = h->fn_dev ? h->fn_dev(send, cnt, recv, (void*)h->st, h->user_dev) : h->fn(send, cnt, recv, h->user);
    if (rc == 0) return LIO_OK;
    const std::string why = lio::last_error();
    return fail(LIO_ERR_STATE, std::string(h->fn_dev ? "device all-gather callback failed" : "allgather callback failed") +
                                   (why.empty() ? "" : ": " + why));
}

int allgather(lio_icp* h, int64_t cnt, const double* h_send, double* h_recv) {
    const bool staged = !h->fn_dev && !h_send;
    if ((h->fn_dev || staged) && cnt > h->x_len)
        return fail(LIO_ERR_STATE, "lio_icp_align: an exchange message is larger than the buffers");
    if (h->fn_dev) return call_allgather(h, h->d_xsend, cnt, h->d_xrecv);
    if (!h->fn) return fail(LIO_ERR_STATE, "lio_icp_align: sharded without an exchange");
    if (!staged) return call_allgather(h, h_send, cnt, h_recv);
    if (h->hx_cap < h->x_len) {
        lio::host_free(&h->h_xs, &h->h_xr);
        h->hx_cap = 0;
        lio::count_alloc(2);
        HIP_TRY(hipHostMalloc(&h->h_xs, (size_t)h->x_len * sizeof(double), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(&h->h_xr, (size_t)h->x_len * h->world * sizeof(double), hipHostMallocDefault));
        h->hx_cap = h->x_len;
    }
    HIP_TRY(hipMemcpyAsync(h->h_xs, h->d_xsend, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    if (const int rc = call_allgather(h, h->h_xs, cnt, h->h_xr)) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_xrecv, h->h_xr, (size_t)cnt * h->world * sizeof(double), hipMemcpyHostToDevice, h->st));
    return LIO_OK;
}

}  // namespace lio::icp

using namespace lio::icp;

extern "C" {

int lio_icp_exchange_len(int64_t n_source, int world, int64_t* n_per_rank) {
    if (n_source < 0 || world < 1 || !n_per_rank) return fail(LIO_ERR_ARG, "lio_icp_exchange_len: bad arguments");
    *n_per_rank = std::max<int64_t>(exchange_len(n_source, world), lio::kIcpStride);
    return LIO_OK;
}

int lio_icp_set_exchange_buffers(lio_icp* h, double* d_send, double* d_recv, int64_t n_per_rank) {
    if (!h || !d_send || !d_recv || n_per_rank <= 0) return fail(LIO_ERR_ARG, "lio_icp_set_exchange_buffers: bad arguments");
    icp_join(h);
    HIP_TRY(hipSetDevice(h->dev));
    if (!h->x_ext) lio::dev_free(&h->d_xsend, &h->d_xrecv);
    h->d_xsend = d_send;
    h->d_xrecv = d_recv;
    h->x_len = n_per_rank;
    h->x_ext = true;
    return LIO_OK;
}

}  // extern "C"
