// lio_icp_setup.cpp — the loop-ICP handle's life and set-up (C-ABI lio_icp_create .. lio_icp_set_shard*): the
// target and the source staged in pinned memory, uploaded and binned behind the caller.
#include "lio_icp_handle.hpp"
#include "lio_pool.hpp"

using namespace lio::icp;

extern "C" {

int lio_icp_create(const lio_icp_params* p, lio_icp** out) {
    if (!p || !out) return fail(LIO_ERR_ARG, "bad arguments");
    *out = nullptr;
    if (p->umeyama_float < LIO_ICP_UMEYAMA_DOUBLE || p->umeyama_float > LIO_ICP_UMEYAMA_PCL_GEMM48)
        return fail(LIO_ERR_ARG, "lio_icp_create: umeyama_float must be -1 (double statistics), 0 (default) or 1..3");
    if (const int rc = lio::capi::check_device(p->device)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    auto* h = new lio_icp();
    h->dev = p->device;
    h->p = *p;
    // the default is the reference's float arithmetic (Eigen 3.3 GEMM order, loop_closure.h:42); the double
    // statistics are an explicit opt-in (-1), stored as 0 from here on
    if (h->p.umeyama_float == LIO_ICP_UMEYAMA_DEFAULT) h->p.umeyama_float = LIO_ICP_UMEYAMA_PCL_GEMM32;
    else if (h->p.umeyama_float == LIO_ICP_UMEYAMA_DOUBLE) h->p.umeyama_float = 0;
    if (!(h->p.cell_size > 0.f)) h->p.cell_size = 1.0f;  // 0.3 m voxelised submaps: 1 m target cells (scripts/icp_cells.py)
    // the grids' capacity floors: a C4-sized submap (500 k points, ~1 M target cells at 1 m) fits from the start
    h->tgt.min_entries = h->qgrid.min_entries = kIcpCapFloor;
    h->tgt.min_cells = 1u << 20;
    h->qgrid.min_cells = 1u << 17;
    if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->st2, hipStreamNonBlocking) != hipSuccess) {
        if (h->st) (void)hipStreamDestroy(h->st);
        delete h;
        return fail(LIO_ERR_HIP, "icp stream/alloc failed");
    }
    (void)hipEventCreate(&h->ev.a);
    (void)hipEventCreate(&h->ev.b);
    (void)hipEventCreate(&h->ev.m);
    (void)hipEventCreateWithFlags(&h->ev.done, hipEventDisableTiming);
    *out = h;
    return LIO_OK;
}

// internal (lio_icp_mp.cpp): hand the exchange state of a multi-process shard to the handle (freed with it,
// or when another exchange replaces it)
void lio_icp_set_exchange_owner(lio_icp* h, void* owner, void (*free_fn)(void*)) {
    icp_join(h);
    if (h->x_owner && h->x_owner_free) {
        (void)hipSetDevice(h->dev);
        (void)hipStreamSynchronize(h->st);
        h->x_owner_free(h->x_owner);
    }
    h->x_owner = owner;
    h->x_owner_free = free_fn;
}

int lio_icp_device(const lio_icp* h) { return h->dev; }

int lio_icp_destroy(lio_icp* h) {
    if (!h) return LIO_OK;
    icp_join(h);
    (void)hipSetDevice(h->dev);
    (void)hipStreamSynchronize(h->st);
    lio_icp_set_exchange_owner(h, nullptr, nullptr);
    lio::grid_free(h->tgt);
    lio::grid_free(h->qgrid);
    lio::pcl_free(h->pg);
    lio::pcl_free(h->pcl);
    lio::dev_free(&h->d_thist, &h->d_tgt, &h->d_src, &h->d_cur, &h->d_fd2, &h->d_fid, &h->d_tiles, &h->d_tscratch,
                  &h->d_ttmp, &h->d_dbg, &h->d_tcost, &h->d_order, &h->d_pcl16, &h->d_pclout);
    if (!h->x_ext) lio::dev_free(&h->d_xsend, &h->d_xrecv);
    for (hipEvent_t e : {h->ev.a, h->ev.b, h->ev.m, h->ev.done})
        if (e) (void)hipEventDestroy(e);
    (void)hipStreamSynchronize(h->st2);  // a target upload may still read its staging buffer
    lio::host_free(&h->h_xs, &h->h_xr, &h->h_super, &h->h_pclout, &h->h_out17, &h->h_tgt, &h->h_src);
    (void)hipStreamDestroy(h->st2);
    (void)hipStreamDestroy(h->st);
    delete h;
    return LIO_OK;
}

// host copy into the handle's pinned staging buffer (grown geometrically), split over a few threads for
// large clouds: the caller's buffer may go away after the call (PCL copies the cloud too)
static int stage_pinned(float*& buf, int64_t& cap, const float* xyz, int64_t n) {
    if (n > cap || !buf) {
        lio::host_free(&buf);
        cap = 0;
        const int64_t c = icp_cap(n, cap);
        lio::count_alloc();
        if (hipHostMalloc(reinterpret_cast<void**>(&buf), (size_t)c * 3 * sizeof(float), hipHostMallocDefault) != hipSuccess)
            return fail(LIO_ERR_NOMEM, "ICP staging: hipHostMalloc failed");
        cap = c;
    }
    const size_t bytes = (size_t)n * 3 * sizeof(float);
    const int nt = bytes >= ((size_t)1 << 20) ? 4 : 1;  // the host pool's threads (no thread created per call)
    if (nt == 1) {
        std::memcpy(buf, xyz, bytes);
    } else {
        const int64_t per = (3 * n + nt - 1) / nt;
        lio::HostPool::get().parallel_for(nt, [&](int t) {
            const int64_t b = std::min<int64_t>(3 * n, t * per), e = std::min<int64_t>(3 * n, b + per);
            std::memcpy(buf + b, xyz + b, (size_t)(e - b) * sizeof(float));
        });
    }
    return LIO_OK;
}

int lio_icp_set_target(lio_icp* h, const float* xyz, int64_t n) {
    if (!h || n <= 0 || !xyz) return fail(LIO_ERR_ARG, "lio_icp_set_target: bad arguments");
    icp_join_tgt(h);
    HIP_TRY(hipSetDevice(h->dev));
    HIP_TRY(hipStreamSynchronize(h->st2));  // a previous target upload may still read the staging buffer
    if (const int rc = stage_pinned(h->h_tgt, h->h_tgt_cap, xyz, n)) return rc;
    h->nt = n;
    h->tgt_dirty = true;
    h->bg_tgt_err.clear();
    // upload + grid on st2 behind the caller: overlaps the source's set-up and whatever the caller does next
    // (no thread: the set-up runs here; a failure of either form leaves tgt_dirty for align to retry)
    run_behind(h->bg_tgt, [h] {
        if (target_build(h) != LIO_OK) h->bg_tgt_err = lio::last_error();
    });
    return LIO_OK;
}

int lio_icp_set_source(lio_icp* h, const float* xyz, int64_t n) {
    if (!h || n < 0 || (n > 0 && !xyz) || n >= (int64_t)1 << 30) return fail(LIO_ERR_ARG, "lio_icp_set_source: bad arguments");
    icp_join_src(h);
    HIP_TRY(hipSetDevice(h->dev));
    HIP_TRY(hipStreamSynchronize(h->st));  // the previous source upload may still read the staging buffer
    if (n > 0)
        if (const int rc = stage_pinned(h->h_src, h->h_src_cap, xyz, n)) return rc;
    h->ns = n;
    h->src_dirty = true;
    h->bg_src_err.clear();
    // this rank's shard uploaded and binned on st behind the caller (a later lio_icp_set_shard* marks it
    // dirty again and align repeats it for the new shard)
    run_behind(h->bg_src, [h] {
        if (hipSetDevice(h->dev) != hipSuccess) h->bg_src_err = "hipSetDevice";
        else if (icp_prepare(h) != LIO_OK) h->bg_src_err = lio::last_error();
    });
    return LIO_OK;
}

// the ranks' exchange is a host callback or a device callback, never both; the shard changes, so the source is
// prepared again
static int set_shard(lio_icp* h, int rank, int world, lio_allgather_fn fn, lio_allgather_dev_fn fn_dev, void* user,
                     const char* bad) {
    if (!h || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn && !fn_dev)) return fail(LIO_ERR_ARG, bad);
    icp_join(h);
    h->rank = rank;
    h->world = world;
    h->fn = fn;
    h->user = fn ? user : nullptr;
    h->fn_dev = fn_dev;
    h->user_dev = fn_dev ? user : nullptr;
    h->src_dirty = true;
    return LIO_OK;
}

int lio_icp_set_shard(lio_icp* h, int rank, int world, lio_allgather_fn fn, void* user) {
    return set_shard(h, rank, world, fn, nullptr, user, "lio_icp_set_shard: bad arguments");
}

int lio_icp_set_shard_device(lio_icp* h, int rank, int world, lio_allgather_dev_fn fn, void* user) {
    return set_shard(h, rank, world, nullptr, fn, user, "lio_icp_set_shard_device: bad arguments");
}

}  // extern "C"

namespace lio::icp {

// the staged target: upload + grid + accumulation centre, on st2 (called from a helper thread)
int target_build(lio_icp* h) {
    HIP_TRY(hipSetDevice(h->dev));
    const int64_t n = h->nt;
    if (n > h->tgt_cap || !h->d_tgt) {
        const int64_t c = icp_cap(n, h->tgt_cap);
        h->tgt_cap = 0;
        if (const int rc = alloc_all({lio::dev_req(h->d_tgt, (size_t)c * 3)}, "ICP target")) return rc;
        h->tgt_cap = c;
    }
    HIP_TRY(hipMemcpyAsync(h->d_tgt, h->h_tgt, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, h->st2));
    int rc = lio::grid_build(h->tgt, h->d_tgt, n, h->p.cell_size, h->st2);
    if (rc) return fail(rc == -5 ? LIO_ERR_NOMEM : LIO_ERR_HIP, "target grid build failed");
    HIP_TRY(hipStreamSynchronize(h->st2));
    // fixed accumulation centre: target bounding-box centre (float)
    const float* bb = h->tgt.aabb_host;
    for (int d = 0; d < 3; ++d) h->c0[d] = (double)(0.5f * (bb[d] + bb[3 + d]));
    h->tgt_dirty = false;
    return LIO_OK;
}

// this rank's shard of the staged source: its buffers, upload and tiles, on st
int icp_prepare(lio_icp* h) {
    if (!h->src_dirty) return LIO_OK;
    shard_range(h->ns, h->rank, h->world, h->sh_begin, h->sh_n);
    if (h->sh_n > h->cap || !h->d_src) {
        const size_t n = (size_t)icp_cap(h->sh_n, h->cap), nt = n + n / lio::kIcpTileQ;
        h->cap = 0;  // a failed allocation below leaves no buffer that looks usable (and nothing freed twice)
        const int rc = alloc_all({lio::dev_req(h->d_src, n * 3), lio::dev_req(h->d_cur, n * 3), lio::dev_req(h->d_fd2, n),
                                  lio::dev_req(h->d_fid, n), lio::dev_req(h->d_tiles, nt + 1),
                                  lio::dev_req(h->d_tcost, nt + 1), lio::dev_req(h->d_order, nt + 64)},  // + the 9 share offsets
                                 "ICP source");
        if (rc) return rc;
        h->cap = (int64_t)n;
    }
    const int64_t nsup_all = (h->ns + lio::kIcpSuper - 1) / lio::kIcpSuper + 1;
    if (nsup_all > h->super_cap) {
        lio::host_free(&h->h_super);
        h->h_super_dev = nullptr;
        // icp_cap counts points: the records' points in, records out (with the record count in, every source got
        // the floor's 129 records, and one above 129 * 4096 points had its last records written past the end)
        const int64_t c = icp_cap(nsup_all * lio::kIcpSuper, h->super_cap * lio::kIcpSuper) / lio::kIcpSuper + 1;
        h->super_cap = 0;
        lio::count_alloc();
        if (const int rc = mapped_alloc(&h->h_super, &h->h_super_dev, c * lio::kIcpStride * sizeof(double))) return rc;
        h->super_cap = c;
    }
    h->ntiles = 0;
    h->have_order = false;  // new tiles: cell order until a pass has measured them
    if (h->sh_n > 0) {
        HIP_TRY(hipMemcpyAsync(h->d_src, h->h_src + 3 * h->sh_begin, h->sh_n * 3 * sizeof(float),
                               hipMemcpyHostToDevice, h->st));
        // bin the shard by tile cell: tiles of <= 64 spatially compact queries (perf only: every
        // query's 1-NN is exact whatever tile it is in)
        int rc = lio::grid_build(h->qgrid, h->d_src, h->sh_n, h->tile_cell, h->st);
        if (rc) return fail(rc == -5 ? LIO_ERR_NOMEM : LIO_ERR_HIP, "source binning failed");
        const int64_t need = 6 * ((int64_t)h->qgrid.geom.ncells + 1);  // icp_build_tiles' scratch
        if (need > h->tscratch_cap) {
            const int64_t c = std::max(need + need / 2, 2 * h->tscratch_cap);
            h->tscratch_cap = 0;
            if ((rc = alloc_all({lio::dev_req(h->d_tscratch, (size_t)c)}, "ICP tile scratch"))) return rc;
            h->tscratch_cap = c;
        }
        const int nt = lio::icp_build_tiles(h->qgrid, h->d_tiles, h->d_tscratch, h->d_ttmp, h->ttmp_bytes, h->st);
        if (nt < 0) return fail(nt == -5 ? LIO_ERR_NOMEM : LIO_ERR_HIP, "tile list failed");
        h->ntiles = nt;
    }
    h->src_dirty = false;
    return LIO_OK;
}

}  // namespace lio::icp
