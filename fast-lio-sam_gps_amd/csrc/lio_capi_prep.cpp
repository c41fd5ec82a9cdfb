// lio_capi_prep.cpp — the C-ABI (include/lio_gpu.h) of the filter handle's create / destroy, the voxel grid, the
// loop leg's submap voxelize, and the sweep preprocessing (Preprocess + UndistortPcl + downSizeFilterSurf) on a
// filter (lio_preprocess) and on a scan context (lio_scan_preprocess*), with the readers of its undistorted cloud.
// The row selection of a sweep upload is lio_sweep_select.hpp; the offline leg on a lio_filter is lio_capi_post.cpp.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lio_capi_online.hpp"
#include "lio_pool.hpp"
#include "lio_sweep_select.hpp"

using namespace lio::capi;

static lio::UndistortEnd undistort_end(const lio_pose* e) {
    lio::UndistortEnd u{};
    if (!e) {
        for (int k = 0; k < 9; ++k) u.R[k] = u.R_LI[k] = (k % 4 == 0) ? 1.0 : 0.0;
        u.q[0] = u.q_LI[0] = 1.0;
        return u;
    }
    const lio_pose f = filled(*e);
    std::memcpy(u.pos, f.t, sizeof(u.pos));
    std::memcpy(u.R, f.R, sizeof(u.R));
    std::memcpy(u.R_LI, f.R_LI, sizeof(u.R_LI));
    std::memcpy(u.t_LI, f.t_LI, sizeof(u.t_LI));
    std::memcpy(u.q, f.q, sizeof(u.q));
    std::memcpy(u.q_LI, f.q_LI, sizeof(u.q_LI));
    return u;
}

static_assert(sizeof(lio_imu_pose) == sizeof(lio::ImuPose), "lio_imu_pose layout");

// the filter's pinned staging buffer holds `need` bytes: max(need, 1.5 x old), no floor
static int reserve_stage(lio::FilterBuf& b, size_t need) {
    if (lio::grow_pinned(&b.h_stage, b.stage_bytes, need, 0)) return fail(LIO_ERR_NOMEM, "sweep staging: hipHostMalloc failed");
    return LIO_OK;
}

// The host half of lio_scan_preprocess_cloud2's upload (byte records, not floats: the selection by |p| waits for
// the device's decode): rows i % every == 0 — Preprocess's point_filter_num drops the others
// by index alone, so they never cross PCIe — and the IMU poses packed into the filter's pinned staging
// buffer, for one DMA each (pageable sources would be staged by the runtime anyway).  *u = rows staged;
// the poses start at byte *pose_off.
static int stage_sweep(lio::FilterBuf& b, const void* rows, int64_t n, size_t row_bytes, int every,
                       const lio_imu_pose* poses, int np, int64_t* u, size_t* pose_off) {
    every = std::max(every, 1);
    *u = (n + every - 1) / every;
    *pose_off = ((size_t)*u * row_bytes + 255) & ~(size_t)255;
    const size_t need = *pose_off + (size_t)np * sizeof(lio_imu_pose);
    if (int rc = reserve_stage(b, need)) return rc;
    auto* dst = static_cast<uint8_t*>(b.h_stage);
    const auto* src = static_cast<const uint8_t*>(rows);
    if (every == 1) {
        std::memcpy(dst, src, (size_t)n * row_bytes);
    } else if (row_bytes % 4 == 0 && row_bytes <= 4 * lio::kMaxFields) {
        const int nw = (int)(row_bytes / 4);
        const auto* s = reinterpret_cast<const float*>(rows);
        auto* d = reinterpret_cast<float*>(dst);
        for (int64_t r = 0; r < *u; ++r)
            for (int k = 0; k < nw; ++k) d[r * nw + k] = s[r * every * nw + k];
    } else {
        for (int64_t r = 0; r < *u; ++r) std::memcpy(dst + r * row_bytes, src + r * every * row_bytes, row_bytes);
    }
    if (np) std::memcpy(dst + *pose_off, poses, (size_t)np * sizeof(lio_imu_pose));
    return LIO_OK;
}

// What a float sweep's upload leaves for the device half: the selected rows (lio_sweep_select.hpp) in *d_raw
// behind the piece table, and the IMU poses behind them.
struct SweepUpload {
    int64_t rows = 0;   // Preprocess's selection, in input order
    int presel = 0;     // 1: their times never decrease
    lio::RowPieces rp;  // logical row -> staged row
    const lio::ImuPose* d_poses = nullptr;
    std::chrono::steady_clock::time_point staged;  // when the host half was done (LIO_PREP_PROFILE)
};

// The host half lio_preprocess and lio_scan_preprocess share: the selection packed into b's pinned staging buffer
// (large sweeps by the host pool in up to kMaxPieces pieces, each at the upper bound of its rows), the poses
// behind it at a 256-byte boundary, *d_raw grown to hold both, and the whole — pieces with their gaps, then
// poses — moved in one DMA.
static int upload_sweep(lio::FilterBuf& b, const float* raw, int64_t n, int stride, const lio_scan_prep_params* p,
                        const lio_imu_pose* poses, int np, float** d_raw, int64_t& raw_cap, hipStream_t st,
                        SweepUpload* u) {
    const int every = std::max(p->point_filter_num, 1);
    const int64_t ub = lio::sweep_candidates(n, every);
    const size_t pose_off = ((size_t)ub * stride * sizeof(float) + 255) & ~(size_t)255;
    const size_t staged = pose_off + (size_t)np * sizeof(lio_imu_pose);
    if (int rc = reserve_stage(b, staged)) return rc;
    const int pieces = ub >= 16384 ? std::min(lio::kMaxPieces, lio::HostPool::get().threads()) : 1;
    const lio::SweepSelection s = lio::select_sweep(
        raw, n, stride, every, p->blind, p->time_field, static_cast<float*>(b.h_stage), pieces, [](int np_, auto& piece) {
            if (np_ == 1) piece(0);
            else lio::HostPool::get().parallel_for(np_, piece);
        });
    if (np) std::memcpy(static_cast<uint8_t*>(b.h_stage) + pose_off, poses, (size_t)np * sizeof(lio_imu_pose));
    u->rows = s.rows;
    u->presel = s.sorted ? 1 : 0;
    u->staged = std::chrono::steady_clock::now();
    if (int rc = grow(d_raw, raw_cap, (int64_t)((staged + 3) / 4) + 1)) return rc;
    if (staged) HIP_TRY(hipMemcpyAsync(*d_raw, b.h_stage, staged, hipMemcpyHostToDevice, st));
    u->rp.n = pieces;
    uint32_t at = 0;
    for (int t = 0; t < pieces; ++t) {
        u->rp.start[t] = at;
        u->rp.src[t] = (uint32_t)s.plan.src_row[t];
        at += (uint32_t)s.plan.rows[t];
    }
    u->d_poses = reinterpret_cast<const lio::ImuPose*>(reinterpret_cast<const uint8_t*>(*d_raw) + pose_off);
    return LIO_OK;
}

// attempt(k) enqueues a preprocessing and finishes it.  2 from it says the voxel key width was learnt too narrow
// (the finish has reset it): the same input goes once more; a second 2 is the device's fault, kHip.
template <class Attempt>
static int twice_if_narrow(Attempt&& attempt) {
    int rc = 2;
    for (int k = 0; k < 2 && rc == 2; ++k) rc = attempt(k);
    return rc == 2 ? lio::kHip : rc;
}

extern "C" {

int lio_filter_create(int device, lio_filter** out) { return open_handle(device, out, "out is NULL"); }

int lio_filter_destroy(lio_filter* f) {
    return close_handle(f, [](lio_filter& h) {
        lio::filter_free(h.b);
        lio::denoise_free(h.dn);
        lio::cluster_free(h.cl);
        lio::plane_free(h.pl);
        lio::kmeans_free(h.km);
        lio::normals_free(h.nm);
        lio::gps_align_free(h.ga);
        lio::project_free(h.pj);
        lio::dev_free(&h.d_in, &h.d_out, &h.d_seg, &h.d_T, &h.d_poses);
    });
}

int lio_voxel_grid(lio_filter* f, const float* pts, int64_t n, int stride, const float leaf[3], float* out,
                   int64_t* n_out) {
    if (!f || !leaf || !n_out || n < 0 || (n > 0 && (!pts || !out)) || stride < 3 || stride > lio::kMaxFields ||
        !(leaf[0] > 0.f && leaf[1] > 0.f && leaf[2] > 0.f))
        return fail(LIO_ERR_ARG, "lio_voxel_grid: bad arguments");
    *n_out = 0;
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    int rc = grow(&f->d_out, f->out_cap, n * stride);
    if (!rc) rc = upload_in(f, pts, n * stride);
    if (rc) return rc;
    int64_t m = 0;
    rc = lio::voxel_grid(f->b, f->d_in, n, stride, leaf, f->d_out, &m, f->st);
    if (rc) return status(rc, "lio_voxel_grid");
    return download_out(f, m, stride, out, n_out);
}

int lio_submap_voxelize(lio_filter* f, const float* pts, const int64_t* seg_off, int nk, int stride,
                        const double* poses16, float voxel_res, float* out, int64_t* n_out) {
    if (!f || !seg_off || !n_out || nk < 0 || stride < 3 || stride > lio::kMaxFields || !(voxel_res > 0.f) ||
        (nk > 0 && !poses16))
        return fail(LIO_ERR_ARG, "lio_submap_voxelize: bad arguments");
    *n_out = 0;
    const int64_t n = nk > 0 ? seg_off[nk] : 0;
    for (int k = 0; k < nk; ++k)
        if (seg_off[k] < 0 || seg_off[k + 1] < seg_off[k]) return fail(LIO_ERR_ARG, "lio_submap_voxelize: bad segments");
    if (seg_off[0] != 0) return fail(LIO_ERR_ARG, "lio_submap_voxelize: seg_off[0] must be 0");
    if (n == 0) return LIO_OK;
    if (!pts || !out) return fail(LIO_ERR_ARG, "lio_submap_voxelize: bad arguments");
    HIP_TRY(hipSetDevice(f->dev));
    // the loop leg's submaps change size on every loop timer call: the buffers are sized once for a C4-sized
    // submap (2 x 11 keyframes) and grow geometrically past it
    constexpr int64_t kSubmapFloor = (int64_t)1 << 19;
    f->b.min_cap = kSubmapFloor;
    const int64_t nf = std::max(n, kSubmapFloor);
    int rc = grow(&f->d_in, f->in_cap, nf * stride);
    if (!rc) rc = grow(&f->d_out, f->out_cap, 2 * nf * stride);
    if (!rc) rc = grow(&f->d_seg, f->seg_cap, std::max<int64_t>(nk + 1, 64));
    if (!rc) rc = grow(&f->d_T, f->T_cap, 16 * std::max<int64_t>(nk, 64));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(f->d_in, pts, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice, f->st));
    HIP_TRY(hipMemcpyAsync(f->d_seg, seg_off, (size_t)(nk + 1) * sizeof(int64_t), hipMemcpyHostToDevice, f->st));
    HIP_TRY(hipMemcpyAsync(f->d_T, poses16, (size_t)nk * 16 * sizeof(double), hipMemcpyHostToDevice, f->st));
    float* d_tf = f->d_out + (size_t)n * stride;  // transformed, concatenated cloud
    rc = lio::transform_segments(f->d_in, n, stride, f->d_seg, nk, f->d_T, d_tf, f->st);
    if (rc) return status(rc, "lio_submap_voxelize");
    const float leaf[3] = {voxel_res, voxel_res, voxel_res};
    int64_t m = 0;
    rc = lio::voxel_grid(f->b, d_tf, n, stride, leaf, f->d_out, &m, f->st);
    if (rc) return status(rc, "lio_submap_voxelize");
    return download_out(f, m, stride, out, n_out);
}

static int prep_args_ok(const float* raw, int64_t n, int stride, const lio_scan_prep_params* p,
                        const lio_imu_pose* poses, int n_poses) {
    if (!p || n < 0 || (n > 0 && !raw) || stride < 4 || stride > lio::kMaxFields || p->time_field < 3 ||
        p->time_field >= stride || n_poses < 0 || (n_poses > 0 && !poses) || n >= (int64_t)1 << 30)
        return fail(LIO_ERR_ARG, "scan preprocessing: bad arguments");
    return LIO_OK;
}

int lio_preprocess(lio_filter* f, const float* raw, int64_t n, int stride, const lio_scan_prep_params* p,
                   const lio_imu_pose* poses, int n_poses, const lio_pose* end, float* out, int64_t* n_out) {
    if (!f || !n_out || (n > 0 && !out)) return fail(LIO_ERR_ARG, "lio_preprocess: bad arguments");
    int rc = prep_args_ok(raw, n, stride, p, poses, n_poses);
    if (rc) return rc;
    *n_out = 0;
    if (n == 0) return LIO_OK;
    HIP_TRY(hipSetDevice(f->dev));
    hipStream_t st = f->st;
    lio::ScanPrepParams sp{p->point_filter_num, p->blind, p->filter_size_surf, p->time_field};
    SweepUpload u;
    rc = upload_sweep(f->b, raw, n, stride, p, poses, n_poses, &f->d_in, f->in_cap, st, &u);
    if (!rc && u.rows) rc = grow(&f->d_out, f->out_cap, u.rows * stride);
    if (rc || u.rows == 0) {  // nothing selected: nothing to do
        (void)hipStreamSynchronize(st);  // the staging buffer is reused by the next call
        return rc;
    }
    int64_t m = 0;
    rc = twice_if_narrow([&](int) {
        const int r = lio::scan_preprocess_enqueue(f->b, f->d_in, u.rows, stride, sp, u.d_poses, n_poses,
                                                   undistort_end(end), f->d_out, st, u.presel, nullptr, nullptr, u.rp);
        return r ? r : lio::scan_preprocess_finish(f->b, stride, f->d_out, &m, nullptr, st);
    });
    if (rc < 0) {
        (void)hipStreamSynchronize(st);  // the staging buffer is reused by the next call
        return status(rc, "lio_preprocess");
    }
    if (m) HIP_TRY(hipMemcpyAsync(out, f->d_out, (size_t)m * stride * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_out = m;
    return LIO_OK;
}

// LIO_PREP_PROFILE=1 (diagnostics): host-side phases of every lio_scan_preprocess on stderr
static bool prep_profile() {
    static const bool on = std::getenv("LIO_PREP_PROFILE") != nullptr;
    return on;
}
static double prep_us(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
}

// the device half shared by lio_scan_preprocess and lio_scan_preprocess_cloud2: c->d_raw holds `rows`
// records; every stage is queued, the scan buffers set up behind it, and the host waits once
static int scan_prep_device(lio_ctx* c, int64_t rows, int stride, const lio::ScanPrepParams& sp, int n_poses,
                            const lio_pose* end, int64_t* n_down, const char* what, int presel = -1,
                            const lio::ImuPose* d_poses = nullptr, const lio::RowPieces& rp = lio::RowPieces{}) {
    if (!d_poses) d_poses = c->d_poses;
    hipStream_t st = c->map->st;
    c->undist_n = -1;
    auto bail = [&](int r) {
        (void)hipStreamSynchronize(st);  // nothing queued may outlive the call (the staging buffer is reused)
        return r;
    };
    int rc = ctx_reserve(c, rows);  // sized for the row bound; c->n set to the count below
    if (rc) return bail(rc);
    int64_t m = 0, mu = 0;
    rc = twice_if_narrow([&](int attempt) {
        const bool vox = sp.leaf > 0.f;  // the centroid pass writes the scan's xyz and flags itself
        int r = lio::scan_preprocess_enqueue(c->filt, c->d_raw, rows, stride, sp, d_poses, n_poses, undistort_end(end),
                                             c->d_rec, st, presel, vox ? c->d_body : nullptr, vox ? c->d_sel : nullptr, rp);
        if (!r && !vox) r = lio::records_to_xyz_sel(c->d_rec, rows, stride, c->d_body, c->d_sel, st);
        if (r) return r;  // the internal statuses are negative
        const auto tw = std::chrono::steady_clock::now();
        r = lio::scan_preprocess_finish(c->filt, stride, c->d_rec, &m, &mu, st);
        if (prep_profile())
            std::fprintf(stderr, "prep_profile wait_us %.1f attempt %d\n", prep_us(tw, std::chrono::steady_clock::now()),
                         attempt);
        return r;
    });
    if (rc < 0) return bail(status(rc, what));
    if (rc == 1) {  // VoxelGrid index overflow: the output is the undistorted input, its xyz again
        rc = lio::records_to_xyz_sel(c->d_rec, m, stride, c->d_body, c->d_sel, st);
        if (rc) return bail(status(rc, what));
        HIP_TRY(hipStreamSynchronize(st));
    }
    c->n = m;
    c->undist_n = mu;
    c->undist_stride = stride;
    if (n_down) *n_down = m;
    return LIO_OK;
}

int lio_scan_preprocess(lio_ctx* c, const float* raw, int64_t n, int stride, const lio_scan_prep_params* p,
                        const lio_imu_pose* poses, int n_poses, const lio_pose* end, int64_t* n_down) {
    if (!c) return fail(LIO_ERR_ARG, "lio_scan_preprocess: NULL ctx");
    int rc = prep_args_ok(raw, n, stride, p, poses, n_poses);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c->map->dev));
    hipStream_t st = c->map->st;
    lio::ScanPrepParams sp{p->point_filter_num, p->blind, p->filter_size_surf, p->time_field};
    SweepUpload u;
    rc = upload_sweep(c->filt, raw, n, stride, p, poses, n_poses, &c->d_raw, c->raw_cap, st, &u);
    if (!rc) rc = grow(&c->d_rec, c->rec_cap, std::max<int64_t>(u.rows, 1) * stride);
    if (rc) {
        (void)hipStreamSynchronize(st);  // the staging buffer is reused by the next call
        return rc;
    }
    const auto t2 = std::chrono::steady_clock::now();
    rc = scan_prep_device(c, u.rows, stride, sp, n_poses, end, n_down, "lio_scan_preprocess", u.presel, u.d_poses, u.rp);
    if (prep_profile()) {
        const auto t3 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "prep_profile rows %lld presel %d stage_us %.1f upload_enqueue_us %.1f device_us %.1f total_us %.1f\n",
                     (long long)u.rows, u.presel, prep_us(t0, u.staged), prep_us(u.staged, t2), prep_us(t2, t3),
                     prep_us(t0, t3));
    }
    return rc;
}

int lio_scan_get_undistorted(lio_ctx* c, float* out, int64_t cap_points, int64_t* n_points, int* stride) {
    if (!c || !n_points) return fail(LIO_ERR_ARG, "lio_scan_get_undistorted: bad arguments");
    if (c->undist_n < 0) return fail(LIO_ERR_STATE, "lio_scan_get_undistorted: no lio_scan_preprocess* on this ctx");
    *n_points = c->undist_n;
    if (stride) *stride = c->undist_stride;
    if (!out || c->undist_n == 0) return LIO_OK;
    if (cap_points < c->undist_n) return fail(LIO_ERR_ARG, "lio_scan_get_undistorted: out too small");
    HIP_TRY(hipSetDevice(c->map->dev));
    HIP_TRY(hipMemcpyAsync(out, c->filt.c, (size_t)c->undist_n * c->undist_stride * sizeof(float),
                           hipMemcpyDeviceToHost, c->map->st));
    HIP_TRY(hipStreamSynchronize(c->map->st));
    return LIO_OK;
}

int lio_scan_keyframe_cloud(lio_ctx* c, const lio_pose* pose, const double* T16, float* out, int64_t cap_points,
                            int64_t* n_points) {
    if (!c || !pose || !T16 || !n_points) return fail(LIO_ERR_ARG, "lio_scan_keyframe_cloud: bad arguments");
    if (c->undist_n < 0) return fail(LIO_ERR_STATE, "lio_scan_keyframe_cloud: no lio_scan_preprocess* on this ctx");
    *n_points = c->undist_n;
    if (!out || c->undist_n == 0) return LIO_OK;
    if (cap_points < c->undist_n) return fail(LIO_ERR_ARG, "lio_scan_keyframe_cloud: out too small");
    HIP_TRY(hipSetDevice(c->map->dev));
    int rc = grow(&c->d_kf, c->kf_cap, c->undist_n * 4);
    if (rc) return rc;
    lio::PoseArg ps;
    const lio_pose pf = filled(*pose);  // matrix-only callers: q / q_LI derived from R / R_LI (body_to_world rotates with them)
    std::memcpy(&ps, &pf, sizeof(ps));
    if (lio::keyframe_cloud(c->filt.c, c->undist_n, c->undist_stride, ps, T16, c->d_kf, c->map->st))
        return fail(LIO_ERR_HIP, "keyframe cloud kernel failed");
    HIP_TRY(hipMemcpyAsync(out, c->d_kf, (size_t)c->undist_n * 4 * sizeof(float), hipMemcpyDeviceToHost, c->map->st));
    HIP_TRY(hipStreamSynchronize(c->map->st));
    return LIO_OK;
}

int lio_scan_preprocess_cloud2(lio_ctx* c, const uint8_t* data, int64_t n_points, int32_t point_step,
                               int is_bigendian, const lio_cloud_field fields[5], const lio_scan_prep_params* p,
                               const lio_imu_pose* poses, int n_poses, const lio_pose* end, int64_t* n_down) {
    if (!c || !fields || point_step <= 0 || n_points < 0 || (n_points > 0 && !data))
        return fail(LIO_ERR_ARG, "lio_scan_preprocess_cloud2: bad arguments");
    lio_scan_prep_params pp = p ? *p : lio_scan_prep_params{1, 0.f, 0.f, 4};
    pp.time_field = 4;
    int rc = prep_args_ok(nullptr, 0, 5, &pp, poses, n_poses);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->map->dev));
    hipStream_t st = c->map->st;
    lio::ScanPrepParams sp{pp.point_filter_num, pp.blind, pp.filter_size_surf, 4};
    int64_t rows = n_points;
    size_t pose_off = 0;
    // the records Preprocess keeps by index, still packed
    rc = stage_sweep(c->filt, data, n_points, (size_t)point_step, pp.point_filter_num, poses, n_poses, &rows, &pose_off);
    if (rc) return rc;
    sp.point_filter_num = 1;
    const int64_t bytes = rows * point_step;
    rc = grow(&c->d_rec, c->rec_cap, std::max<int64_t>((bytes + 3) / 4, rows * 5 + 1));  // staging for the bytes
    if (!rc) rc = grow(&c->d_raw, c->raw_cap, std::max<int64_t>(rows, 1) * 5);
    if (!rc && n_poses) rc = grow(&c->d_poses, c->poses_cap, n_poses);
    if (rc) return rc;
    const auto* stage = static_cast<const uint8_t*>(c->filt.h_stage);
    if (rows)
        HIP_TRY(hipMemcpyAsync(c->d_rec, stage, (size_t)bytes, hipMemcpyHostToDevice, st));
    if (n_poses)
        HIP_TRY(hipMemcpyAsync(c->d_poses, stage + pose_off,
                               (size_t)n_poses * sizeof(lio::ImuPose), hipMemcpyHostToDevice, st));
    rc = lio::cloud_decode(reinterpret_cast<const uint8_t*>(c->d_rec), rows, point_step, is_bigendian != 0,
                           reinterpret_cast<const lio::CloudField*>(fields), 5, c->d_raw, st);
    if (rc) {
        (void)hipStreamSynchronize(st);
        return status(rc, "lio_scan_preprocess_cloud2");
    }
    return scan_prep_device(c, rows, 5, sp, n_poses, end, n_down, "lio_scan_preprocess_cloud2");
}

}  // extern "C"
