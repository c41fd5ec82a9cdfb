// lio_icp_host.cpp — LoopClosure::icpAlignment replacement (C-ABI lio_icp_*): the correspondence pass and the
// alignment loop (lio_icp_handle.hpp lists the files the rest is in).
//
// Host loop = pcl::IterativeClosestPoint::computeTransformation as configured at
// fast_lio_sam/src/loop_closure.cpp:3-14 (PCL 1.10 semantics [U]):
//   repeat { correspondences (1-NN, d2 <= max_corr_dist^2) on the incrementally
//            transformed source; < 3 => not converged, stop;
//            T_inc = Umeyama(src_corr, tgt_corr) (TransformationEstimationSVD);
//            transform source by T_inc; final = T_inc * final; ++iter;
//            DefaultConvergenceCriteria }
//   score = getFitnessScore() (unbounded 1-NN of src*final), is_valid =
//   converged && score < icp_score_threshold (loop_closure.cpp:85-90).
// Per iteration the GPU returns Umeyama sufficient statistics per 4096-point
// record; ranks all-gather the records and every rank sums them in record
// order, so the result is bit-identical for any number of ranks.
#include "lio_icp_handle.hpp"
#include "lio_icp_math.hpp"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>

using namespace lio::icp;

// the kernels' arguments of one pass over this rank's shard
static lio::IcpArgs pass_args(const lio_icp* h, bool fitness, bool apply_T, const float* T, double max_d2) {
    lio::IcpArgs a{};
    a.grid = lio::grid_view(h->tgt);
    a.tgt_by_id = h->tgt.by_id;
    a.cur = h->d_cur;
    a.src = h->d_src;
    a.thist = h->d_thist;
    a.nT = h->nT;
    a.n = (int)h->sh_n;
    a.apply_T = apply_T ? 1 : 0;
    std::memcpy(a.T, T, sizeof(a.T));
    std::memcpy(a.c0, h->c0, sizeof(a.c0));
    a.max_d2 = max_d2;
    a.fitness = fitness ? 1 : 0;
    a.prior = h->have_prior ? 1 : 0;
    // first bound box: the tile's own cells (r0 = 0; with the per-batch bound and the centre-out rows, pair A
    // 0.221 -> 0.212 ms per alignment against r0 = 1, pair B unchanged: profiles/r05_icp_r0_ab.txt)
    a.r0 = 0;
    a.nn_d2 = h->d_fd2;
    a.nn_id = h->d_fid;
    a.qpts = h->qgrid.pts;
    a.tiles = h->d_tiles;
    a.tile_cost = h->d_tcost;
    a.order = h->have_order ? h->d_order : nullptr;
    return a;
}

#ifdef LIO_DIAG
// diagnostics build, LIO_ICP_DEBUG set: the search counters of a pass (diag_arm before it, diag_print after)
static bool diag_on() {
    static const bool on = std::getenv("LIO_ICP_DEBUG") != nullptr;
    return on;
}
static int diag_arm(lio_icp* h, lio::IcpArgs& a) {
    if (!diag_on()) return LIO_OK;
    // 8 counters + (start, end) wall clock per tile + (growth candidates, final candidates, final rows, rounds)
    const size_t bytes = (8 + 6 * (size_t)std::max(h->ntiles, 1)) * sizeof(unsigned long long);
    if (h->d_dbg && h->dbg_bytes < bytes) lio::dev_free(&h->d_dbg);
    if (!h->d_dbg) {
        HIP_TRY(hipMalloc(&h->d_dbg, bytes));
        h->dbg_bytes = bytes;
    }
    HIP_TRY(hipMemsetAsync(h->d_dbg, 0, bytes, h->st));
    a.dbg = h->d_dbg;
    return LIO_OK;
}
static int diag_print(lio_icp* h) {
    if (!diag_on()) return LIO_OK;
    unsigned long long c[5];
    HIP_TRY(hipMemcpy(c, h->d_dbg, sizeof(c), hipMemcpyDeviceToHost));
    std::fprintf(stderr,
                 "icp dbg: tiles|waves %llu lanes %llu cand/tile %.1f tested/tile %.1f rounds/tile %.2f cand/lane %.1f\n",
                 c[2], c[3], (double)c[0] / c[2], (double)c[4] / c[2], (double)c[1] / c[2], (double)c[0] / c[3]);
    // per-tile timeline (wall clock, 100 MHz): span, duration percentiles, the tail
    std::vector<unsigned long long> tt(2 * (size_t)h->ntiles);
    std::vector<uint32_t> cost(h->ntiles);
    HIP_TRY(hipMemcpy(tt.data(), h->d_dbg + 8, tt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cost.data(), h->d_tcost, cost.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull, t1 = 0;
    std::vector<double> dur(h->ntiles);
    int imax = 0;
    for (int t = 0; t < h->ntiles; ++t) {
        t0 = std::min(t0, tt[2 * t]);
        t1 = std::max(t1, tt[2 * t + 1]);
        dur[t] = (double)(tt[2 * t + 1] - tt[2 * t]) * 0.01;  // us
        if (dur[t] > dur[imax]) imax = t;
    }
    unsigned long long last_start = 0;
    int late = 0;
    for (int t = 0; t < h->ntiles; ++t) {
        last_start = std::max(last_start, tt[2 * t]);
        if (tt[2 * t] > t0 + (t1 - t0) / 2) ++late;
    }
    std::vector<double> sd = dur;
    std::sort(sd.begin(), sd.end());
    auto pct = [&](double q) { return sd[std::min(sd.size() - 1, (size_t)(q * (double)sd.size()))]; };
    std::fprintf(stderr,
                 "icp tiles: span %.1f us | tile us p50 %.2f p90 %.2f p99 %.2f max %.2f (cost %u, median cost %u) | "
                 "last tile starts at %.1f us | tiles starting in the second half %d of %d\n",
                 (double)(t1 - t0) * 0.01, pct(0.5), pct(0.9), pct(0.99), sd.back(), cost[imax],
                 [&] { std::vector<uint32_t> c2 = cost; std::nth_element(c2.begin(), c2.begin() + c2.size() / 2, c2.end()); return c2[c2.size() / 2]; }(),
                 (double)(last_start - t0) * 0.01, late, h->ntiles);
    // the slowest tiles' search: candidates streamed while growing / in the final round, final rows, rounds
    std::vector<unsigned long long> ex(4 * (size_t)h->ntiles);
    HIP_TRY(hipMemcpy(ex.data(), h->d_dbg + 8 + 2 * (size_t)h->ntiles, ex.size() * sizeof(unsigned long long),
                   hipMemcpyDeviceToHost));
    std::vector<int> idx(h->ntiles);
    for (int t = 0; t < h->ntiles; ++t) idx[t] = t;
    const int nshow = std::min(5, h->ntiles);
    std::partial_sort(idx.begin(), idx.begin() + nshow, idx.end(), [&](int u, int v) { return dur[u] > dur[v]; });
    for (int k = 0; k < nshow; ++k) {
        const int t = idx[k];
        std::fprintf(stderr, "  slow tile %d: %.1f us, starts %.1f us, growth cand %llu, final cand %llu, final rows %llu, rounds %llu, cost %u\n",
                     t, dur[t], (double)(tt[2 * t] - t0) * 0.01, ex[4 * t], ex[4 * t + 1], ex[4 * t + 2], ex[4 * t + 3], cost[t]);
    }
    return LIO_OK;
}
#endif

namespace lio::icp {
void add_pass_timing(lio_icp* h) {
    if (!h->timing || h->sh_n <= 0) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev.a, h->ev.b) == hipSuccess) {
        h->tm.icp_ms += ms;
        ++h->tm.icp_launches;
    }
    if (hipEventElapsedTime(&ms, h->ev.a, h->ev.m) == hipSuccess) {
        h->tm.icp_nn_ms += ms;
        ++h->tm.icp_nn_launches;
    }
}
}  // namespace lio::icp

// One correspondence (or fitness) pass: GPU kernels + exchange + ordered sum.
static int icp_pass(lio_icp* h, bool fitness, bool apply_T, const float* T, double max_d2, double out17[17],
                    float* pcl16 = nullptr) {
    if (!fitness && apply_T && h->nT >= h->thist_cap) return fail(LIO_ERR_STATE, "lio_icp_align: transform history full");
    lio::IcpArgs a = pass_args(h, fitness, apply_T, T, max_d2);
#ifdef LIO_DIAG
    if (const int rc = diag_arm(h, a)) return rc;
#endif
    const int nsup_loc = (int)((h->sh_n + lio::kIcpSuper - 1) / lio::kIcpSuper);
    const bool dev_x = h->world > 1 && h->fn_dev;  // device-side exchange: records stay on the device
    // the sharded PCL float modes' correspondence passes: icp_pass_fsh (the chains split over the ranks' windows)
    if (pcl16 && fid_sharded(h) && !fitness) return icp_pass_fsh(h, a, apply_T, out17, pcl16);
    const int64_t cnt = records_count(h->ns, h->world);  // doubles per rank this pass
    if (dev_x)
        if (const int rc = exchange_reserve(h)) return rc;
    if (h->sh_n > 0 || dev_x) {
        if (h->timing) HIP_TRY(hipEventRecord(h->ev.a, h->st));
        if (h->sh_n > 0) lio::launch_icp_tiles(a, h->ntiles, h->st);
        if (h->timing) HIP_TRY(hipEventRecord(h->ev.m, h->st));
        // the PCL float modes: the accepted pairs compacted by the same launch (one rank: the whole source)
        lio::IcpCompact cpa;
        if (pcl16 && !fitness) cpa = lio::pcl_compact_args(h->pcl);
        const lio::IcpCompact* cp = pcl16 && !fitness ? &cpa : nullptr;
        if (dev_x) {  // records -> device send buffer -> in-stream all-gather -> record-order sum
            if (h->sh_n > 0) lio::launch_icp_stats(a, h->d_xsend, h->st, fitness ? nullptr : h->d_order, h->ntiles, cp);
            HIP_TRY(hipGetLastError());
            if (const int rc = allgather(h, cnt)) return rc;
            const int64_t nsup = (h->ns + lio::kIcpSuper - 1) / lio::kIcpSuper;
            lio::launch_icp_combine(h->d_xrecv, nsup, h->world, cnt, h->h_out17_dev, h->st);
        } else if (h->sh_n > 0) {
            // records straight to host memory; the next pass's tile order in the same launch
            lio::launch_icp_stats(a, h->h_super_dev, h->st, fitness ? nullptr : h->d_order, h->ntiles, cp);
        }
        if (cp && h->sh_n == 0) HIP_TRY(hipMemsetAsync(cp->d_n, 0, sizeof(uint32_t), h->st));  // no pairs
        if (h->timing) HIP_TRY(hipEventRecord(h->ev.b, h->st));
        uint32_t seq = 0;
        if (pcl16)  // one rank: the float statistics of its correspondences
            if (const int rc = enqueue_pcl(h, &seq)) return rc;
        HIP_TRY(hipGetLastError());
        if (pcl16 && !h->timing) {  // the pack's sequence number (it is the pass's last launch)
            if (const int rc = pcl_wait(h, seq)) return rc;
        } else {
            HIP_TRY(hipEventRecord(h->ev.done, h->st));
            HIP_TRY(hipEventSynchronize(h->ev.done));
        }
    } else {
        HIP_TRY(hipStreamSynchronize(h->st));
    }
    h->have_prior = true;
    if (!fitness && h->sh_n > 0) h->have_order = true;
    if (!fitness && apply_T) ++h->nT;
#ifdef LIO_DIAG
    if (const int rc = diag_print(h)) return rc;
#endif
    add_pass_timing(h);
    if (!dev_x && h->world > 1) {
        // host exchange: fixed-size slots (max records per rank), summed in global record order
        h->rec_send.assign((size_t)cnt, 0.0);
        h->rec_recv.resize((size_t)cnt * h->world);
        std::memcpy(h->rec_send.data(), h->h_super, (size_t)nsup_loc * lio::kIcpStride * sizeof(double));
        if (const int rc = allgather(h, cnt, h->rec_send.data(), h->rec_recv.data())) return rc;
        combine_records(h->rec_recv.data(), h->ns, h->world, cnt, out17);
    } else if (dev_x) {  // the record-order sums of every rank's records, computed on the device
        std::memcpy(out17, h->h_out17, 17 * sizeof(double));
    } else {
        for (int k = 0; k < 17; ++k) out17[k] = 0.0;
        for (int s = 0; s < nsup_loc; ++s)
            for (int k = 0; k < 17; ++k) out17[k] += h->h_super[(size_t)s * lio::kIcpStride + k];
    }
    if (pcl16) {
        if (const int rc = pcl_finish(h, a)) return rc;
        std::memcpy(pcl16, h->h_pclout, 16 * sizeof(float));
    }
    return LIO_OK;
}

// the PCL float modes' buffers for the staged source: the window's pairs (sharded: + the kPclMaxKc pairs of the
// ranks after it, for the depth blocks that start in the window and end in the next), the chains, the outputs
static int pcl_prepare(lio_icp* h) {
    const bool fsh = fid_sharded(h);
    lio::PclBuf& P = h->pcl;
    if (lio::pcl_reserve(P, std::max<int64_t>(h->sh_n + (fsh ? lio::kPclMaxKc : 0), kIcpCapFloor), h->p.umeyama_float, h->st))
        return fail(LIO_ERR_NOMEM, "lio_icp_align: fidelity buffers");
    P.means.dbg_noinc = P.sig.dbg_noinc = h->fid_flags & 1;
    P.n_hint = fsh ? 0 : h->sh_n;  // one rank: the accepted pairs are a subset of the source
    for (lio::SeqSumBuf* b : {&P.means, &P.sig})
        b->evcap = h->fid_evcap > 0 ? std::min(h->fid_evcap, b->evcap_alloc) : b->evcap_alloc;
    P.mean6 = reinterpret_cast<float*>(P.small + lio::kPclMean6);
    if (lio::seqsum_shard(P.means, fsh, h->st) ||
        (h->p.umeyama_float == lio::kPclSeq && lio::seqsum_shard(P.sig, fsh, h->st)) ||
        (fsh && lio::pcl_shard_reserve(P, h->ns / 340 + 4, h->st)))
        return fail(LIO_ERR_NOMEM, "lio_icp_align: sharded fidelity buffers");
    P.n_all = fsh ? reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(P.means.sh) +
                                                      offsetof(lio::SeqShard, n32))
                  : nullptr;
    if (fsh) {
        const int cap = (int)ev_slot_cap(h->ns, h->world);
        h->ev_slot = std::min(h->ev_slot, cap);
        h->ev_slot_s = std::min(h->ev_slot_s, cap);
    }
    if (!h->d_pcl16) HIP_TRY(hipMalloc(&h->d_pcl16, 16 * sizeof(float)));
    if (!h->d_pclout) HIP_TRY(hipMalloc(&h->d_pclout, 32 * sizeof(float)));
    if (!h->h_pclout) {
        if (const int rc = mapped_alloc(&h->h_pclout, &h->h_pclout_dev, 32 * sizeof(float))) return rc;
        h->box = Mailbox(h->h_pclout + 23);
    }
    return LIO_OK;
}

extern "C" {

int lio_icp_get_fidelity_stats(lio_icp* h, int64_t* out4) {
    if (!h || !out4) return fail(LIO_ERR_ARG, "lio_icp_get_fidelity_stats: bad arguments");
    icp_join(h);
    std::memcpy(out4, h->fid_stats, sizeof(h->fid_stats));
    return LIO_OK;
}

int lio_icp_get_umeyama_stats(lio_icp* h, float* out16) {
    if (!h || !out16) return fail(LIO_ERR_ARG, "lio_icp_get_umeyama_stats: bad arguments");
    icp_join(h);
    if (h->p.umeyama_float <= 0) return fail(LIO_ERR_STATE, "lio_icp_get_umeyama_stats: the handle runs the double statistics");
    if (!h->have_pcl16) return fail(LIO_ERR_STATE, "lio_icp_get_umeyama_stats: no pass run yet");
    std::memcpy(out16, h->last_pcl16, sizeof(h->last_pcl16));
    return LIO_OK;
}

int lio_icp_set_fidelity_debug(lio_icp* h, int flags, int64_t evcap) {
    if (!h || evcap < 0) return fail(LIO_ERR_ARG, "lio_icp_set_fidelity_debug: bad arguments");
    icp_join(h);
    h->fid_flags = flags;
    h->fid_evcap = evcap;
    return LIO_OK;
}

int lio_icp_align(lio_icp* h, const float* guess16, lio_icp_result* out, float* aligned) {
    if (!h || !out) return fail(LIO_ERR_ARG, "lio_icp_align: bad arguments");
    icp_join(h);
    if (h->nt == 0) return fail(LIO_ERR_STATE, "lio_icp_align: no target");
    HIP_TRY(hipSetDevice(h->dev));
    const bool pcl_float = h->p.umeyama_float > 0;  // (normalised at create: 0 = the double statistics)
    // the target (st2, helper thread) and the source (st, this thread) prepared side by side
    int rc = LIO_OK, trc = LIO_OK;
    std::string terr;
    std::thread tth;
    if (h->tgt_dirty) {
        run_behind(tth, [&] {
            trc = target_build(h);
            if (trc) terr = lio::last_error();
        });
    }
    rc = icp_prepare(h);
    if (tth.joinable()) tth.join();
    // a set-up that failed in the background and again here: both reasons
    if (trc) return fail(trc, terr + (h->bg_tgt_err.empty() ? "" : " (setInputTarget: " + h->bg_tgt_err + ")"));
    if (rc) return fail(rc, lio::last_error() + (h->bg_src_err.empty() ? "" : " (setInputSource: " + h->bg_src_err + ")"));
    h->bg_tgt_err.clear();
    h->bg_src_err.clear();
    if (pcl_float && (rc = pcl_prepare(h))) return rc;
    float fin[16], G[16];
    bool ident = true;
    for (int i = 0; i < 16; ++i) {
        G[i] = guess16 ? guess16[i] : ((i % 5 == 0) ? 1.f : 0.f);
        fin[i] = G[i];
        if (G[i] != ((i % 5 == 0) ? 1.f : 0.f)) ident = false;
    }
    if (h->sh_n > 0)
        HIP_TRY(hipMemcpyAsync(h->d_cur, h->d_src, h->sh_n * 3 * sizeof(float), hipMemcpyDeviceToDevice, h->st));
    const int hist_need = std::max(h->p.max_iter, 1) + 4;  // one T per iteration plus the guess
    if (hist_need > h->thist_cap) {
        lio::dev_free(&h->d_thist);
        h->thist_cap = 0;
        HIP_TRY(hipMalloc(&h->d_thist, (size_t)hist_need * 16 * sizeof(float)));
        h->thist_cap = hist_need;
    }
    h->nT = 0;
    h->have_pcl16 = false;
    h->have_prior = false;
    h->have_order = false;  // every alignment starts in cell order (its first pass measures the tiles)
    const double max_d2 = h->p.max_corr_dist * h->p.max_corr_dist;
    double prev_mse = std::numeric_limits<double>::max();
    int iters = 0;
    bool apply = !ident;
    float Tapply[16];
    std::memcpy(Tapply, G, sizeof(G));
    std::memset(out, 0, sizeof(*out));  // state 0, not converged
    for (;;) {
        double st[17];
        float pcl16[16];
        rc = icp_pass(h, false, apply, Tapply, max_d2, st, pcl_float ? pcl16 : nullptr);
        if (rc) return rc;
        if (pcl_float) {
            std::memcpy(h->last_pcl16, pcl16, sizeof(pcl16));
            h->have_pcl16 = true;
        }
        out->last_corr = (int64_t)st[0];
        if (st[0] < 3) {
            out->state = 5;
            break;
        }
        float Ti[16];
        if (pcl_float)
            umeyama_pcl_float(pcl16, Ti, h->p.umeyama_float);
        else
            umeyama(st, h->c0, Ti);
        compose4f(Ti, fin);
        ++iters;
        const double mse = st[16] / st[0];
        out->last_mse = mse;
        const bool done = convergence_step(Ti, mse, prev_mse, iters, h->p, &out->state);
        prev_mse = mse;
        std::memcpy(Tapply, Ti, sizeof(Ti));
        apply = true;
        if (done) {
            out->is_converged = 1;
            break;
        }
    }
    out->iterations = iters;
    std::memcpy(out->T, fin, sizeof(fin));
    // getFitnessScore(): original source * final, unbounded 1-NN
    double fs[17];
    rc = icp_pass(h, true, true, fin, std::numeric_limits<double>::infinity(), fs);
    if (rc) return rc;
    out->score = fs[0] > 0 ? fs[16] / fs[0] : std::numeric_limits<double>::max();
    out->is_valid = (out->is_converged && out->score < h->p.score_threshold) ? 1 : 0;
    if (aligned && h->sh_n > 0) {
        HIP_TRY(hipMemcpyAsync(aligned, h->d_cur, h->sh_n * 3 * sizeof(float), hipMemcpyDeviceToHost, h->st));
        HIP_TRY(hipStreamSynchronize(h->st));
    }
    return LIO_OK;
}

int icp_align(const float* src, int64_t ns, const float* dst, int64_t nd, const lio_icp_params* p, int n_gpus,
              float* T_out, double* fitness, int* converged, int* iters, float* aligned) {
    if (!p) return fail(LIO_ERR_ARG, "icp_align: NULL params");
    // n_gpus > 1: devices p->device .. p->device + n_gpus - 1, source sharded, records all-gathered over
    // RCCL (lio_icp_group); n_gpus <= 1: one handle on p->device
    const int ng = n_gpus > 1 ? n_gpus : 1;
    std::vector<int> devs(ng);
    for (int r = 0; r < ng; ++r) devs[r] = p->device + r;
    lio_icp_group* g = nullptr;
    int rc = lio_icp_group_create(p, ng, devs.data(), &g);
    if (rc) return rc;
    rc = lio_icp_group_set_target(g, dst, nd);
    if (!rc) rc = lio_icp_group_set_source(g, src, ns);
    lio_icp_result r{};
    if (!rc) rc = lio_icp_group_align(g, nullptr, &r, aligned);
    if (!rc) {
        if (T_out) std::memcpy(T_out, r.T, sizeof(r.T));
        if (fitness) *fitness = r.score;
        if (converged) *converged = r.is_converged;
        if (iters) *iters = r.iterations;
    }
    lio_icp_group_destroy(g);
    return rc;
}

int lio_icp_get_correspondences(lio_icp* h, int32_t* ids, float* d2) {
    if (!h || !ids || !d2) return fail(LIO_ERR_ARG, "bad arguments");
    icp_join(h);
    if (!h->have_prior) return fail(LIO_ERR_STATE, "lio_icp_get_correspondences: no pass run yet");
    HIP_TRY(hipSetDevice(h->dev));
    if (h->sh_n > 0) {
        HIP_TRY(hipMemcpyAsync(ids, h->d_fid, h->sh_n * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
        HIP_TRY(hipMemcpyAsync(d2, h->d_fd2, h->sh_n * sizeof(float), hipMemcpyDeviceToHost, h->st));
        HIP_TRY(hipStreamSynchronize(h->st));
    }
    return LIO_OK;
}

int lio_icp_set_timing(lio_icp* h, int enable) {
    if (!h) return fail(LIO_ERR_ARG, "NULL handle");
    icp_join(h);
    h->timing = enable != 0;
    return LIO_OK;
}
int lio_icp_get_timing(lio_icp* h, lio_kernel_timing* out) {
    if (!h || !out) return fail(LIO_ERR_ARG, "bad arguments");
    icp_join(h);
    *out = h->tm;
    return LIO_OK;
}

}  // extern "C"
