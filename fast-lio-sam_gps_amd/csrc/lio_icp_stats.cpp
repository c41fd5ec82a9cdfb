// lio_icp_stats.cpp — the PCL float statistics of a correspondence pass (lio_icp_params.umeyama_float 1..3):
// the sequential float chains computed in parallel and verified on the device (lio_pcl.hpp, lio_seqsum.hpp), on
// one rank or split over the ranks' windows.  A chain that failed its verification is re-run with the
// predictions of its reconstruction; an event-list overflow or a chain that keeps failing falls back to the
// serial kernels (one lane per chain, the sums in order).  What follows which status is lio_icp_policy.hpp's
// next_step; pcl_finish launches what it says.
#include "lio_icp_handle.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace lio::icp {

namespace {

// word w of the pass's status block (h_pclout[16 ..], after the pass's wait)
uint32_t pcl_word(const lio_icp* h, int w) {
    uint32_t u;
    std::memcpy(&u, h->h_pclout + 16 + w, sizeof(u));
    return u;
}

// test hook (lio_icp_set_fidelity_debug): report a look-back time-out for this pass
int hook_lb_timeout(lio_icp* h) {
    if (h->fid_flags & 4) HIP_TRY(hipMemsetAsync(h->pcl.small + lio::kPclTicket + 1, 1, sizeof(uint32_t), h->st));
    return LIO_OK;
}

}  // namespace

// one rank: the pack stores its words straight into h_pclout (host-mapped) and its sequence number last; the host
// polls that word (h->box) instead of a copy launch and an event wait (the pass's last launch is the pack)
int pcl_wait(lio_icp* h, uint32_t seq) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0; !h->box.arrived(seq); ++spin) {
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HIP_TRY(hipStreamSynchronize(h->st));  // a failed launch reports here
            if (!h->box.arrived(seq)) return fail(LIO_ERR_STATE, "lio_icp_align: the statistics never arrived");
            break;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return LIO_OK;
}

// the pairs were compacted by the statistics launch (icp_pass: launch_icp_stats with IcpCompact)
int enqueue_pcl(lio_icp* h, uint32_t* seq) {
    const int order = h->p.umeyama_float;
    if (const int rc = hook_lb_timeout(h)) return rc;
    lio::launch_pcl_means(h->pcl, 1, h->st);
    lio::launch_pcl_sigma(h->pcl, order, 1, h->st);
    *seq = h->box.post();
    lio::launch_pcl_pack(h->pcl, order, h->h_pclout_dev, h->st, nullptr, *seq);
    return LIO_OK;
}

// ---------------------------------------------------------------- the sharded PCL float statistics
// Per correspondence pass (world > 1, umeyama_float 1..3), three all-gathers on the handle's stream:
//   records   the tile kernel, the records, the window's compaction, the means chains' block sums and the
//             window's totals -> all-gather -> the records' sum (MSE, counts) and every window's place in the
//             chains (seq_shard_offsets)
//   events    the means chains counted and their events listed on the window -> all-gather (+ each window's
//             first kPclMaxKc pairs) -> the global event lists, the walk over all of them (every rank: the serial
//             floor), the window verified
//   blocks    orders 2 / 3: the GEMM depth blocks starting in the window -> all-gather -> res += alpha * C_b over
//             all blocks in order (order 1: the sigma chains take the means' three steps themselves)
// so per-rank work and memory follow the window (source / world) except the walk and the order-of-blocks
// sums, and every rank gets the one-rank transform bit for bit (the verification covers every element).
namespace {

lio::SeqPairs fsh_means_src(const lio_icp* h) { return lio::SeqPairs{h->pcl.pairs, h->pcl.cap}; }
lio::SeqSigma fsh_sigma_src(const lio_icp* h) { return lio::SeqSigma{h->pcl.pairs, h->pcl.mean6, h->pcl.cap}; }

// the means' event message is packed (seqsum_shard_mid / _repack): + the window's first pairs -> all-gather ->
// the pairs after the window appended, the global lists, the walk, the window's verification
int fsh_heads(const lio_icp* h) { return h->p.umeyama_float != 1 ? lio::kPclMaxKc : 0; }
int fsh_means_events(lio_icp* h, int pass) {
    lio::PclBuf& P = h->pcl;
    const int64_t m2 = lio::seqsum_msg_words(6, h->ev_slot, fsh_heads(h));
    if (const int rc = allgather(h, m2)) return rc;
    lio::SeqHeads hd;
    if (fsh_heads(h)) hd = lio::SeqHeads{lio::kPclMaxKc, P.pairs, P.cap, P.ghead, lio::kPclTinyN};
    lio::seqsum_shard_tail(fsh_means_src(h), 6, P.small + lio::kPclN, P.means, pass, h->d_xrecv, m2, h->rank, h->world,
                           h->ev_slot, hd, h->st);
    return LIO_OK;
}

// sigma and the result: order 1 the nine sigma chains sharded like the means (stage 0: from pass spass's block
// sums; stage 1: the same lists exchanged again with a larger slot), orders 2 / 3 the depth blocks; then the
// block exchange, the statuses combined, pcl_pack, and the pass's output on the host (one wait).  All
// kPclOutWords are copied: the finish loop reads [20] .. [22], and [23] is the mailbox's word, which the next
// one-rank post() zeroes
int fsh_sigma_pack(lio_icp* h, int spass, int stage = 0) {
    lio::PclBuf& P = h->pcl;
    const int order = h->p.umeyama_float;
    const uint32_t* dn = P.small + lio::kPclN;
    const int64_t nq_slot = lio::pcl_blocks_slot(shard_points_max(h->ns, h->world));
    int rc = LIO_OK;
    if (order == 1) {
        const lio::SeqSigma ss = fsh_sigma_src(h);
        if (stage == 0) {
            lio::launch_pcl_mean6(P, P.means.result, h->st);
            const int64_t nbs = tot_blocks(h->ns, h->world), tw = tot_words(h->ns, h->world, 9);
            if (spass <= 1) {
                lio::seqsum_shard_head(ss, 9, dn, P.sig, h->d_xsend, nbs, h->st);
                if ((rc = allgather(h, tw))) return rc;
            }
            lio::seqsum_shard_mid(ss, 9, dn, P.sig, spass, h->d_xrecv, tw, nbs, h->rank, h->world, h->d_xsend,
                                  h->ev_slot_s, 0, h->st);
        } else {
            HIP_TRY(hipMemsetAsync(P.sig.status + 1, 0, sizeof(uint32_t), h->st));
            lio::seqsum_shard_repack(ss, 9, dn, P.sig, h->d_xsend, h->ev_slot_s, 0, h->st);
        }
        const int64_t m = lio::seqsum_msg_words(9, h->ev_slot_s);
        if ((rc = allgather(h, m))) return rc;
        lio::seqsum_shard_tail(ss, 9, dn, P.sig, spass, h->d_xrecv, m, h->rank, h->world, h->ev_slot_s, lio::SeqHeads{},
                               h->st);
    }
    lio::launch_pcl_sigma_shard(P, order, h->d_xsend, nq_slot, h->st);
    const int64_t m3 = order == 1 ? lio::kPclX3Hdr : lio::pcl_x3_words(nq_slot);
    if ((rc = allgather(h, m3))) return rc;
    lio::launch_pcl_x3_merge(P, order, h->d_xrecv, m3, h->world, nq_slot, h->d_pclout, h->st);
    lio::launch_pcl_pack_shard(P, order, h->d_pclout, h->st);
    HIP_TRY(hipMemcpyAsync(h->h_pclout, h->d_pclout, lio::kPclOutWords * sizeof(float), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return LIO_OK;
}

// the serial fallback, sharded: every window's pairs gathered on every rank (in rounds that fit the exchange
// buffers; O(source) memory for this path only) into h->pg, their serial means in d_pcl16
int fsh_gather_pairs(lio_icp* h, const lio::IcpArgs& a, bool lb_timeout) {
    lio::PclBuf& P = h->pcl;
    lio::PclBuf& G = h->pg;
    const uint32_t* dn = P.small + lio::kPclN;
    if (lb_timeout) {  // the window's pairs re-compacted by the serial kernel (its count lands in d_pcl16[6])
        lio::launch_icp_pcl_means_serial(a, P.pairs, P.cap, h->d_pcl16, h->st);
        dn = reinterpret_cast<const uint32_t*>(h->d_pcl16 + 6);
        HIP_TRY(hipMemsetAsync(P.small + lio::kPclTicket + 1, 0, sizeof(uint32_t), h->st));
    }
    if (lio::pcl_reserve_plain(G, std::max<int64_t>(h->ns, 1), h->st)) return fail(LIO_ERR_NOMEM, "lio_icp_align: fallback pairs");
    const int64_t chunk = (exchange_len(h->ns, h->world) - 2) / 3;  // the capacity every exchange offers
    const int64_t rounds = (shard_points_max(h->ns, h->world) + chunk - 1) / chunk;
    for (int64_t t = 0; t < rounds; ++t) {
        lio::launch_pcl_gather_pack(P, dn, t, chunk, h->d_xsend, h->st);
        if (const int rc = allgather(h, lio::pcl_gather_words(chunk))) return rc;
        lio::launch_pcl_gather_unpack(G, h->d_xrecv, lio::pcl_gather_words(chunk), h->world, t, chunk, h->st);
    }
    lio::launch_icp_pcl_means_pairs(G.pairs, G.cap, G.small + lio::kPclN, h->d_pcl16, h->st);
    return LIO_OK;
}

// The serial kernels, one lane per chain.  One rank: over the pass's correspondences, re-compacted (a look-back
// time-out left pairs that cannot be trusted; the flag is cleared here, or every later pass would see it:
// ADVICE r05).  Sharded: over every rank's pairs, gathered.  Only the 16 statistics reach h_pclout, and the two
// status words are zeroed: nothing after this reads the rest of the pass's block.
int pcl_serial(lio_icp* h, const lio::IcpArgs& a, bool lb_timeout) {
    ++h->fid_stats[1];
    const int order = h->p.umeyama_float;
    const bool fsh = fid_sharded(h);
    lio::PclBuf& B = fsh ? h->pg : h->pcl;  // the pairs the chains run over
    const float* out = h->d_pcl16;
    if (fsh) {
        if (const int rc = fsh_gather_pairs(h, a, lb_timeout)) return rc;
        if (order == lio::kPclSeq) lio::launch_icp_pcl_sigma_serial(B.pairs, B.cap, h->d_pcl16, h->st);
    } else {
        if (lb_timeout) HIP_TRY(hipMemsetAsync(B.small + lio::kPclTicket + 1, 0, sizeof(uint32_t), h->st));
        if (order == lio::kPclSeq) lio::launch_icp_pcl_stats(a, B.pairs, B.cap, h->d_pcl16, h->st);
        else lio::launch_icp_pcl_means_serial(a, B.pairs, B.cap, h->d_pcl16, h->st);
    }
    if (order != lio::kPclSeq) {  // sigma in Eigen's GEMM order from the serial means
        lio::launch_pcl_sigma(B, order, 1, h->st, h->d_pcl16);
        lio::launch_pcl_pack(B, order, h->d_pclout, h->st, h->d_pcl16);
        out = h->d_pclout;
    }
    HIP_TRY(hipMemcpyAsync(h->h_pclout, out, 16 * sizeof(float), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    h->h_pclout[16] = h->h_pclout[17] = 0.f;
    return LIO_OK;
}

// one rank: the chains named by `step` again, the pack, the wait
int repass_one(lio_icp* h, Step step, const PassCounters& c) {
    const int order = h->p.umeyama_float;
    if (step == Step::RepassMeans) lio::launch_pcl_means(h->pcl, c.mpass, h->st);
    lio::launch_pcl_sigma(h->pcl, order, c.spass, h->st);
    const uint32_t seq = h->box.post();
    lio::launch_pcl_pack(h->pcl, order, h->h_pclout_dev, h->st, nullptr, seq);
    return pcl_wait(h, seq);
}

// sharded: a re-pass exchanges the chains' new event lists; a re-exchange only the same lists with the slot they
// need (every step ends in fsh_sigma_pack's wait)
int repass_fsh(lio_icp* h, Step step, const PassCounters& c) {
    lio::PclBuf& P = h->pcl;
    const uint32_t* dn = P.small + lio::kPclN;
    if (step == Step::ReexchangeSigma) return fsh_sigma_pack(h, c.spass, 1);
    if (step == Step::RepassSigma) return fsh_sigma_pack(h, c.spass);
    if (step == Step::ReexchangeMeans) {
        HIP_TRY(hipMemsetAsync(P.means.status + 1, 0, sizeof(uint32_t), h->st));
        lio::seqsum_shard_repack(fsh_means_src(h), 6, dn, P.means, h->d_xsend, h->ev_slot, fsh_heads(h), h->st);
    } else {  // RepassMeans
        lio::seqsum_shard_mid(fsh_means_src(h), 6, dn, P.means, c.mpass, nullptr, 0, 0, h->rank, h->world, h->d_xsend,
                              h->ev_slot, fsh_heads(h), h->st);
    }
    const int rc = fsh_means_events(h, c.mpass);
    return rc ? rc : fsh_sigma_pack(h, 1);  // sigma depends on the means: its chains restart from pass 1
}

}  // namespace

int pcl_finish(lio_icp* h, const lio::IcpArgs& a) {
    const bool fsh = fid_sharded(h);
    lio::PclBuf& P = h->pcl;
    ++h->fid_stats[3];
    h->fid_stats[2] = (int)pcl_word(h, 2);
    const bool lb_timeout = pcl_word(h, 3) != 0;  // the compaction's look-back timed out (never expected)
    const int64_t cap = ev_slot_cap(h->ns, h->world);
    static const bool trace = std::getenv("LIO_FSH_TRACE") != nullptr;  // diagnostics: the re-pass decisions
    PassCounters c;
    for (;;) {
        PassStatus s{pcl_word(h, 0), pcl_word(h, 1)};
        if (fsh) s = {s.bad, s.over, pcl_word(h, 4), (int)pcl_word(h, 5), (int)pcl_word(h, 6)};  // every rank's, combined
        if (trace && fsh)
            std::fprintf(stderr, "fsh rank %d: bad %x over %x xflags %x longest %d/%d mpass %d spass %d slot %d look-back %d\n",
                         h->rank, s.bad, s.over, s.xf, s.mm, s.ms, c.mpass, c.spass, h->ev_slot, (int)lb_timeout);
        if (!lb_timeout) {
            if (fsh) {
                h->ev_slot = next_slot(s.mm, h->ev_slot, cap);
                if (h->p.umeyama_float == 1 && s.ms > 0) h->ev_slot_s = next_slot(s.ms, h->ev_slot_s, cap);
            }
            // a failed verification set forced-event bits: whatever runs next (a re-pass, a restarted sigma pass
            // 1, the serial fallback), the next pass 1 must clear them (stale bits only add events)
            if (s.bad) P.means.forced_dirty = P.sig.forced_dirty = true;
        }
        const Step step = next_step(s, cap, lb_timeout, c);
        if (step == Step::Done) break;
        if (step == Step::Serial) {
            if (trace && fsh) std::fprintf(stderr, "fsh rank %d: serial fallback\n", h->rank);
            if (const int rc = pcl_serial(h, a, lb_timeout)) return rc;
            break;
        }
        if (const int rc = fsh ? repass_fsh(h, step, c) : repass_one(h, step, c)) return rc;
        if (step == Step::RepassMeans || step == Step::RepassSigma) {  // a re-exchange is no re-pass
            ++h->fid_stats[0];
            ++h->fid_stats[3];
        }
    }
    HIP_TRY(hipGetLastError());
    return LIO_OK;
}

int icp_pass_fsh(lio_icp* h, const lio::IcpArgs& a, bool apply_T, double out17[17], float* pcl16) {
    if (h->world > 64) return fail(LIO_ERR_ARG, "lio_icp_align: the sharded float statistics take at most 64 ranks");
    int rc = exchange_reserve(h);
    if (rc) return rc;
    lio::PclBuf& P = h->pcl;
    const uint32_t* dn = P.small + lio::kPclN;
    const int64_t rec = records_count(h->ns, h->world), nbs = tot_blocks(h->ns, h->world);
    const int64_t cnt1 = rec + tot_words(h->ns, h->world, 6);
    const int64_t nsup = (h->ns + lio::kIcpSuper - 1) / lio::kIcpSuper;
    if (h->timing) HIP_TRY(hipEventRecord(h->ev.a, h->st));
    if (h->sh_n > 0) lio::launch_icp_tiles(a, h->ntiles, h->st);
    if (h->timing) HIP_TRY(hipEventRecord(h->ev.m, h->st));
    const lio::IcpCompact cpa = lio::pcl_compact_args(P);  // the window's pairs compacted by the same launch
    if (h->sh_n > 0) lio::launch_icp_stats(a, h->d_xsend, h->st, h->d_order, h->ntiles, &cpa);
    else HIP_TRY(hipMemsetAsync(cpa.d_n, 0, sizeof(uint32_t), h->st));  // an empty window: no pairs
    if (h->timing) HIP_TRY(hipEventRecord(h->ev.b, h->st));
    if ((rc = hook_lb_timeout(h))) return rc;
    lio::seqsum_shard_head(fsh_means_src(h), 6, dn, P.means, h->d_xsend + rec, nbs, h->st);
    if ((rc = allgather(h, cnt1))) return rc;
    // the records' sum in record order rides the offsets launch (lio_icp_combine's order)
    const lio::SeqRecordSum rs{h->d_xrecv, nsup, h->world, cnt1, lio::kIcpStride, 17, h->h_out17_dev};
    lio::seqsum_shard_mid(fsh_means_src(h), 6, dn, P.means, 1, h->d_xrecv + rec, cnt1, nbs, h->rank, h->world,
                          h->d_xsend, h->ev_slot, fsh_heads(h), h->st, &rs);
    if ((rc = fsh_means_events(h, 1))) return rc;
    if ((rc = fsh_sigma_pack(h, 1))) return rc;  // waits for the pass
    HIP_TRY(hipGetLastError());
    h->have_prior = true;
    if (h->sh_n > 0) h->have_order = true;
    if (apply_T) ++h->nT;
    add_pass_timing(h);
    std::memcpy(out17, h->h_out17, 17 * sizeof(double));
    if ((rc = pcl_finish(h, a))) return rc;
    std::memcpy(pcl16, h->h_pclout, 16 * sizeof(float));
    return LIO_OK;
}

}  // namespace lio::icp
